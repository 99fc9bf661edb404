#!/usr/bin/env python3
"""lookahead() against rollout(128, actions) at the same number of lane-steps, one MI355X, one session.

    python scripts/lookahead_bench.py [--rounds 5] [--parent PATH/TO/PARENT/libmi355env.so] [--out profiles/lookahead_ab.txt]

Every measurement runs in its own process, `--rounds` times, this build's and -- with --parent -- the parent build's interleaved
(scripts/bench_rounds.py).  A process measures, for CartPole-v1 and Pendulum-v1 with output="torch" and fixed device
action tensors, the time per call -- device events around CALLS calls, median of WINDOWS windows -- of

  rollout          rollout(128, actions, return_actions=False) on 65 536 sub-environments: the path a planner had before (every build)
  lookahead_1024   lookahead(actions[128, 64, 1024])       } 8 388 608 lane-steps each, like the rollout
  lookahead_65536  lookahead(actions[128, 1, 65536])       } (this build only: the parent has no such entry point)

Random valid actions; gamma = 0.99.  Experiment infrastructure only: no test reads its numbers.

    python scripts/lookahead_bench.py --scaling [--out profiles/lookahead_scaling.txt]

One process, this build: lookahead(actions[128, K, 65536]) for K = 1, 2, 4 and all five ids -- beyond 65 536 lanes several wavefronts share a SIMD.
"""
import argparse
import json
import os
import sys

from bench_rounds import finish, median_window, run_rounds, spread

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, CALLS, WINDOWS, WARMUP = 128, 200, 7, 20
IDS = ("CartPole-v1", "Pendulum-v1")


def child():
    sys.path.insert(0, ROOT)
    import torch

    import gymnasium_amd

    def windows(call):
        return median_window(torch, call, WARMUP, CALLS, WINDOWS)

    def actions(env_id, shape):
        g = torch.Generator().manual_seed(3)
        if env_id == "CartPole-v1":
            return torch.randint(0, 2, shape, dtype=torch.int64, generator=g).cuda()
        return (torch.rand(shape + (1,), generator=g) * 4.0 - 2.0).cuda()

    out = {}
    for env_id in IDS:
        row = {}
        env = gymnasium_amd.make_vec(env_id, num_envs=65536, output="torch", copy=False)
        env.reset(seed=0)
        block = actions(env_id, (H, 65536))
        row["rollout"] = windows(lambda: env.rollout(H, block, return_actions=False))
        if hasattr(env._engine.lib, "lookahead"):
            cand = actions(env_id, (H, 1, 65536))
            row["lookahead_65536"] = windows(lambda: env.lookahead(cand, 0.99))
            env.close()
            env = gymnasium_amd.make_vec(env_id, num_envs=1024, output="torch", copy=False)
            env.reset(seed=0)
            cand = actions(env_id, (H, 64, 1024))
            row["lookahead_1024"] = windows(lambda: env.lookahead(cand, 0.99))
        env.close()
        out[env_id] = row
    print("RESULT " + json.dumps(out))


def scaling(out_path):
    sys.path.insert(0, ROOT)
    import torch

    import gymnasium_amd

    ids = {"CartPole-v1": 2, "Pendulum-v1": 0, "Acrobot-v1": 3, "MountainCar-v0": 3, "MountainCarContinuous-v0": 0}
    lines = [f"lookahead(actions[{H}, K, 65536]), us per call (device events around 50 calls, median of 5 windows) and lane-steps per second"]
    for env_id, n_act in ids.items():
        env = gymnasium_amd.make_vec(env_id, num_envs=65536, output="torch", copy=False)
        env.reset(seed=0)
        for K in (1, 2, 4):
            g = torch.Generator().manual_seed(3)
            if n_act:
                cand = torch.randint(0, n_act, (H, K, 65536), dtype=torch.int64, generator=g).cuda()
            else:
                cand = (torch.rand((H, K, 65536, 1), generator=g) * 2.0 - 1.0).cuda()
            us = median_window(torch, lambda: env.lookahead(cand, 0.99), 5, 50, 5)
            lines.append(f"{env_id:26s} K = {K}  {us:9.1f} us  {H * K * 65536 / us * 1e6:.3e} lane-steps/s")
            print(lines[-1], flush=True)
        env.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scaling", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    if args.scaling:
        return scaling(args.out)
    rows, lines = run_rounds(__file__, args.rounds, args.parent, timeout=600)
    lines.append("")
    lines.append(f"us per call, {H} steps x 65 536 lanes = 8 388 608 lane-steps; median [min .. max] of {args.rounds} processes")
    for (env_id, name, what), v in sorted(rows.items()):
        lines.append(f"{env_id:12s} {name:6s} {what:16s} {spread(v, 9)}")
    finish(lines, args.out)


if __name__ == "__main__":
    main()
