#!/usr/bin/env python3
"""The price of per-sub-environment model fields: env-steps/s of rollout(8) for HalfCheetah-v5, Ant-v5 and Humanoid-v5 at 32 768 robots and Hopper-v5
at 65 536, one MI355X, in three configurations:

  coop      the cooperative kernel where the robot has one (today's default for the first three; forced with MI355ENV_MJ_COOP=1 for Hopper, whose
            default is the one-lane kernel)
  one-lane  the stock one-lane kernel (MI355ENV_MJ_SERIAL=1)
  per-lane  the one-lane kernel with every model field set per sub-environment (set_attr: three parameter sets, lane i on set i % 3)

    python scripts/model_attrs_bench.py [--rounds 3] [--out profiles/model_attrs_bench.txt]

Every measurement runs in its own process (the two environment variables are read when an env is created), the configurations interleaved,
`--rounds` times; a process times WINDOWS windows of LAUNCHES rollout(8) calls that end in a device synchronise and reports the median window.
Experiment infrastructure only: no test reads its numbers; they are the documented price of the switch (docs/results_log.md)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("HalfCheetah-v5", 32768), ("Ant-v5", 32768), ("Humanoid-v5", 32768), ("Hopper-v5", 65536))
CONFIGS = ("coop", "one-lane", "per-lane")
T, WARMUP, LAUNCHES, WINDOWS = 8, 2, 4, 3


def child(env_id, n, config):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import gymnasium_amd

    env = gymnasium_amd.make_vec(env_id, num_envs=n, output="torch")
    if config == "per-lane":
        scale = np.array([1.0, 0.6, 1.4])[np.arange(n) % 3][:, None]
        for name in ("gravity", "actuator_gear", "dof_damping", "geom_friction"):
            env.set_attr(name, torch.from_numpy(np.stack(env.get_attr(name)) * scale).cuda())
    env.reset(seed=0)
    env.action_space.seed(1)
    for _ in range(WARMUP):
        env.rollout(T, return_actions=False)
    torch.cuda.synchronize()
    rates = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(LAUNCHES):
            env.rollout(T, return_actions=False)
        torch.cuda.synchronize()
        rates.append(LAUNCHES * T * n / (time.perf_counter() - t0))
    env.close()
    print("RESULT " + json.dumps(sorted(rates)[len(rates) // 2]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, metavar=("ENV_ID", "N", "CONFIG"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.child[2])
    res = {}
    for _ in range(args.rounds):
        for env_id, n in CASES:
            for config in CONFIGS:
                env = {k: v for k, v in os.environ.items() if k not in ("MI355ENV_MJ_SERIAL", "MI355ENV_MJ_COOP")}
                if config == "coop":
                    env["MI355ENV_MJ_COOP"] = "1"
                if config == "one-lane":
                    env["MI355ENV_MJ_SERIAL"] = "1"
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env_id, str(n), config], env=env, capture_output=True, text=True, timeout=600)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not lines:
                    sys.exit(f"{env_id} {config} failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")
                res.setdefault((env_id, config), []).append(json.loads(lines[-1][7:]))
    rows = [f"model_attrs_bench: rollout({T}), {args.rounds} rounds interleaved, median of {WINDOWS} windows of {LAUNCHES} launches; M env-steps/s"]
    for env_id, n in CASES:
        med = {c: sorted(res[env_id, c])[len(res[env_id, c]) // 2] / 1e6 for c in CONFIGS}
        rows.append(f"{env_id} @ {n}: " + ", ".join(f"{c} {med[c]:.3f} (rounds {' '.join(f'{v / 1e6:.3f}' for v in res[env_id, c])})" for c in CONFIGS) +
                    f"; per-lane / one-lane = {med['per-lane'] / med['one-lane']:.3f}, per-lane / coop = {med['per-lane'] / med['coop']:.3f}")
    text = "\n".join(rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
