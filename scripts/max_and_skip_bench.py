#!/usr/bin/env python3
"""MaxAndSkipObservation(4) inside the step against RepeatAction(4) and four plain steps at 65 536 sub-environments, one MI355X, one session.

    python scripts/max_and_skip_bench.py [--rounds 5] [--parent PATH/TO/PARENT/libmi355env.so] [--out profiles/max_and_skip_bench.txt]

Every measurement runs in its own process (scripts/step_wrappers_bench.py's scheme), `--rounds` times; with --parent the parent build's processes
(MI355ENV_LIBRARY selects the build) are interleaved with this build's and measure RepeatAction(4) and the plain step alone -- RepeatAction's device
code is the parent's, and this is the run-to-run noise its figure has to be read against.  A process measures, for CartPole-v1 and Pendulum-v1 with
output="torch" and fixed device action tensors,

  step     us per step() call: a host clock around STEPS calls that end in a device synchronise (the per-step API is launch-bound)
  rollout  us per 128-step rollout(128, actions): a host clock around ROLLOUTS calls that end in a device synchronise

under `maxskip` (wrappers.MaxAndSkipObservation(env, 4)), `repeat` (wrappers.RepeatAction(env, 4)) and `plain` (the bare env; the report multiplies
its step by four and sets a 512-step rollout beside the two 128-step ones: the same number of inner steps).  Experiment infrastructure only: no test
reads its numbers.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, T, WARMUP, STEPS, ROLLOUTS, WINDOWS = 65536, 4, 128, 200, 4000, 40, 5
IDS = ("CartPole-v1", "Pendulum-v1")


def child():
    sys.path.insert(0, ROOT)
    import torch

    import gymnasium_amd
    from gymnasium_amd import wrappers

    def windows(call, count, warmup):
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        took = []
        for _ in range(WINDOWS):
            t0 = time.perf_counter()
            for _ in range(count):
                call()
            torch.cuda.synchronize()
            took.append((time.perf_counter() - t0) / count * 1e6)
        return sorted(took)[len(took) // 2]  # us per call, median window

    def measure(build, steps):
        env = build(gymnasium_amd.make_vec(env_id, num_envs=N, output="torch", copy=False))
        env.reset(seed=0)
        env.action_space.seed(1)
        a = torch.from_numpy(env.action_space.sample()).cuda()
        block = a.unsqueeze(0).repeat(steps, *([1] * a.dim())).contiguous()
        per_step = windows(lambda: env.step(a), STEPS, WARMUP)
        per_rollout = windows(lambda: env.rollout(steps, block, return_actions=False), ROLLOUTS, 5)
        env.close()
        return per_step, per_rollout

    out = {}
    for env_id in IDS:
        probe = gymnasium_amd.make_vec(env_id, num_envs=8, output="torch")
        has = hasattr(probe, "_max_and_skip_refusal") and probe._max_and_skip_refusal() is None
        probe.close()
        forms = [("repeat", lambda e: wrappers.RepeatAction(e, K), T), ("plain", lambda e: e, K * T)]
        if has:
            forms.insert(0, ("maxskip", lambda e: wrappers.MaxAndSkipObservation(e, K), T))
        for name, build, steps in forms:
            out[f"{env_id} {name} step"], out[f"{env_id} {name} rollout"] = measure(build, steps)
    print("RESULT " + json.dumps(out), flush=True)


def median(x):
    return sorted(x)[len(x) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libmi355env.so built from the parent commit")
    ap.add_argument("--this", default=os.path.join(ROOT, "gymnasium_amd", "csrc", "libmi355env.so"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    builds = ([("parent", args.parent)] if args.parent else []) + [("this", args.this)]
    res = {name: {} for name, _ in builds}
    for rnd in range(args.rounds):
        for name, path in builds:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, MI355ENV_LIBRARY=os.path.abspath(path)),
                               capture_output=True, text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"{name} round {rnd} failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")
            for k, v in json.loads(lines[-1][7:]).items():
                res[name].setdefault(k, []).append(v)
            print(f"round {rnd} {name} done", flush=True)
    spread = lambda x: 100 * (max(x) - min(x)) / median(x)  # noqa: E731
    show = lambda x: f"{median(x):.2f} us (spread {spread(x):.1f} %)"  # noqa: E731
    rows = [f"max_and_skip_bench: {N} sub-environments, {args.rounds} rounds, median of {WINDOWS} windows of {STEPS} step() calls / {ROLLOUTS} rollouts; "
            "median over the rounds, spread = (max - min) / median over the rounds"]
    th = res["this"]
    for env_id in IDS:
        m, r, p = th[f"{env_id} maxskip step"], th[f"{env_id} repeat step"], th[f"{env_id} plain step"]
        rows.append(f"{env_id} step(): MaxAndSkipObservation(4) {show(m)} | RepeatAction(4) {show(r)} | four plain steps {K * median(p):.2f} us "
                    f"(one: {show(p)}) | MaxAndSkip / RepeatAction = {median(m) / median(r):.3f}")
        m, r, p = th[f"{env_id} maxskip rollout"], th[f"{env_id} repeat rollout"], th[f"{env_id} plain rollout"]
        rows.append(f"{env_id} rollout({T}): MaxAndSkipObservation(4) {show(m)} | RepeatAction(4) {show(r)} | plain rollout({K * T}) {show(p)} "
                    f"| MaxAndSkip / RepeatAction = {median(m) / median(r):.3f}")
        if args.parent:
            for what in ("repeat step", "repeat rollout", "plain step", "plain rollout"):
                a, b = res["parent"][f"{env_id} {what}"], th[f"{env_id} {what}"]
                rows.append(f"  {env_id} {what}: parent {show(a)}, this {show(b)}: this / parent = {median(b) / median(a):.3f}")
    text = "\n".join(rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
