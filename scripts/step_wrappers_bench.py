#!/usr/bin/env python3
"""RepeatAction inside the step against plain stepping at 65 536 sub-environments, one MI355X, two library builds side by side.

    python scripts/step_wrappers_bench.py --parent PATH/TO/PARENT/libmi355env.so [--rounds 5] [--out profiles/step_wrappers_ab.txt]

Every measurement runs in its own process (scripts/ab_bench.py's scheme: MI355ENV_LIBRARY selects the build), interleaved parent / this / parent /
this ..., `--rounds` times.  A process measures, for CartPole-v1 and Pendulum-v1 with output="torch" and a fixed device action tensor,

  plain   us per step() launch: a host clock around STEPS calls that end in a device synchronise (the per-step API is launch-bound: this is what
          a policy loop pays per call)
  k4, k8  (this build only) us per step() of wrappers.RepeatAction(env, 4) / (env, 8)

and the parent prints (a) plain of this build against plain of the parent build, with the run-to-run spread of the SAME build (max - min over the
rounds, as a share of the median) that the difference has to be read against, and (b) one RepeatAction(k) step against k plain steps of the
parent build.  Experiment infrastructure only: no test reads its numbers.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WARMUP, STEPS, WINDOWS = 65536, 200, 4000, 5
IDS = ("CartPole-v1", "Pendulum-v1")


def child():
    sys.path.insert(0, ROOT)
    import torch

    import gymnasium_amd
    from gymnasium_amd import wrappers

    def per_call(env):
        env.reset(seed=0)
        env.action_space.seed(1)
        a = torch.from_numpy(env.action_space.sample()).cuda()
        for _ in range(WARMUP):
            env.step(a)
        torch.cuda.synchronize()
        best = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(STEPS):
                env.step(a)
            torch.cuda.synchronize()
            best.append((time.perf_counter() - t0) / STEPS * 1e6)
        env.close()
        return sorted(best)[len(best) // 2]  # us per call, median window

    out = {}
    for env_id in IDS:
        out[f"{env_id} plain"] = per_call(gymnasium_amd.make_vec(env_id, num_envs=N, output="torch", copy=False))
        probe = gymnasium_amd.make_vec(env_id, num_envs=8, output="torch")
        has = probe._step_wrappers_refusal() is None
        probe.close()
        for k in (4, 8) if has else ():
            out[f"{env_id} k{k}"] = per_call(wrappers.RepeatAction(gymnasium_amd.make_vec(env_id, num_envs=N, output="torch", copy=False), k))
    print("RESULT " + json.dumps(out), flush=True)


def median(x):
    return sorted(x)[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libmi355env.so built from the parent commit")
    ap.add_argument("--this", default=os.path.join(ROOT, "gymnasium_amd", "csrc", "libmi355env.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    res = {"parent": {}, "this": {}}
    for rnd in range(args.rounds):
        for name, path in (("parent", args.parent), ("this", args.this)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--parent", args.parent],
                               env=dict(os.environ, MI355ENV_LIBRARY=os.path.abspath(path)), capture_output=True, text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"{name} round {rnd} failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")
            for k, v in json.loads(lines[-1][7:]).items():
                res[name].setdefault(k, []).append(v)
    rows = [f"step_wrappers_bench: {N} sub-environments, {args.rounds} rounds interleaved, {STEPS} calls per window, median of {WINDOWS} windows; us per call"]
    for env_id in IDS:
        pa, th = res["parent"][f"{env_id} plain"], res["this"][f"{env_id} plain"]
        spread = lambda x: (max(x) - min(x)) / median(x)  # noqa: E731
        rows.append(f"(a) {env_id} plain step(): parent {median(pa):.2f} us (rounds {' '.join(f'{v:.2f}' for v in pa)}; spread {100 * spread(pa):.1f} %), "
                    f"this {median(th):.2f} us (rounds {' '.join(f'{v:.2f}' for v in th)}; spread {100 * spread(th):.1f} %): "
                    f"this / parent = {median(th) / median(pa):.3f}")
        for k in (4, 8):
            w = res["this"][f"{env_id} k{k}"]
            rows.append(f"(b) {env_id} RepeatAction(k = {k}): {median(w):.2f} us per step() (rounds {' '.join(f'{v:.2f}' for v in w)}) against {k} plain "
                        f"steps of the parent = {k * median(pa):.2f} us: x{k * median(pa) / median(w):.2f}; against ONE plain step: x{median(w) / median(pa):.2f}")
    text = "\n".join(rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
