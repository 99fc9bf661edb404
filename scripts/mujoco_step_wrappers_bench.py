#!/usr/bin/env python3
"""One RepeatAction(4) step of a MuJoCo env against four plain steps of the parent build's kernels, one MI355X, two library builds side by side.

    python scripts/mujoco_step_wrappers_bench.py --parent PATH/TO/PARENT/libmi355env.so [--rounds 3] [--out profiles/mujoco_step_wrappers_ab.txt]

scripts/step_wrappers_bench.py's scheme: every measurement in its own process (MI355ENV_LIBRARY selects the build), interleaved parent / this / parent /
this ..., `--rounds` times.  A process measures, for HalfCheetah-v5 at 65 536 and Humanoid-v5 at 32 768 sub-environments with output="torch" and a fixed
device action tensor, the ms per step() call -- a host clock around STEPS calls that end in a device synchronise; these steps run milliseconds, so the
clock reads kernel time -- of the plain env and (this build only) of wrappers.RepeatAction(env, 4).  With random-free constant actions nothing finishes
early at the default limit in these few steps, so the wrapped step runs all four trips: the comparison is launch for launch.  Experiment infrastructure
only: no test reads its numbers.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("HalfCheetah-v5", 65536, 40), ("Humanoid-v5", 32768, 8))  # (id, sub-environments, plain steps per window)
K, WINDOWS = 4, 3


def child():
    sys.path.insert(0, ROOT)
    import torch

    import gymnasium_amd
    from gymnasium_amd import wrappers

    def per_call(env, steps):
        env.reset(seed=0)
        env.action_space.seed(1)
        a = torch.as_tensor(env.action_space.sample()).cuda()
        for _ in range(3):
            env.step(a)
        torch.cuda.synchronize()
        best = []
        for _ in range(WINDOWS):
            env.reset(seed=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                env.step(a)
            torch.cuda.synchronize()
            best.append((time.perf_counter() - t0) / steps * 1e3)
        env.close()
        return sorted(best)[len(best) // 2]  # ms per call, median window

    out = {}
    for env_id, n, steps in CASES:
        kw = dict(num_envs=n, output="torch", copy=False, terminate_when_unhealthy=False) if env_id != "HalfCheetah-v5" else dict(num_envs=n, output="torch", copy=False)
        out[f"{env_id} plain"] = per_call(gymnasium_amd.make_vec(env_id, **kw), steps)
        probe = gymnasium_amd.make_vec(env_id, num_envs=8, output="torch")
        has = probe._step_wrappers_refusal() is None
        probe.close()
        if has:
            try:
                out[f"{env_id} k{K}"] = per_call(wrappers.RepeatAction(gymnasium_amd.make_vec(env_id, **kw), K), steps // K)
            except Exception:  # the parent build: its entry point refuses the MuJoCo kinds
                pass
    print("RESULT " + json.dumps(out), flush=True)


def median(x):
    return sorted(x)[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libmi355env.so built from the parent commit")
    ap.add_argument("--this", default=os.path.join(ROOT, "gymnasium_amd", "csrc", "libmi355env.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    res = {"parent": {}, "this": {}}
    for rnd in range(args.rounds):
        for name, path in (("parent", args.parent), ("this", args.this)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", args.parent],
                               env=dict(os.environ, MI355ENV_LIBRARY=os.path.abspath(path)), capture_output=True, text=True, timeout=300)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"{name} round {rnd} failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")
            for k, v in json.loads(lines[-1][7:]).items():
                res[name].setdefault(k, []).append(v)
    rows = [f"mujoco_step_wrappers_bench: {args.rounds} rounds interleaved, median of {WINDOWS} windows; ms per call"]
    for env_id, n, steps in CASES:
        pa, th, w = res["parent"][f"{env_id} plain"], res["this"][f"{env_id} plain"], res["this"][f"{env_id} k{K}"]
        rows.append(f"{env_id} x{n}: plain step() parent {median(pa):.3f} ms (rounds {' '.join(f'{v:.3f}' for v in pa)}), this {median(th):.3f} ms "
                    f"(rounds {' '.join(f'{v:.3f}' for v in th)}), this / parent = {median(th) / median(pa):.3f}; RepeatAction({K}) step() {median(w):.3f} ms "
                    f"(rounds {' '.join(f'{v:.3f}' for v in w)}) against {K} plain steps of the parent = {K * median(pa):.3f} ms: ratio {median(w) / (K * median(pa)):.3f}")
    text = "\n".join(rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
