#!/usr/bin/env python3
"""What the body mass scale costs the per-lane kernels, by the method of scripts/model_attrs_bench.py (every measurement in its own process, the
configurations interleaved, median window of rollout(8) calls that end in a device synchronise):

  1. one-lane LaneModel throughput of HalfCheetah-v5, Ant-v5, Humanoid-v5 (32 768 robots) and Hopper-v5 (65 536) with ONLY gravity set per
     sub-environment, for two builds of the library -- `--old` (a build of the parent commit) against `--new` (this tree's, the default): what the
     mass fields cost a per-lane user that does not set them (with the mass rows inside the one LaneFields: up to 5.7 %, docs/results_log.md; hence
     mjx::MassLaneModel, a model type of their own);
  2. the same with body_mass_scale set as well (new build only): the MassLaneModel kernels;
  3. the time of one set_attr("body_mass_scale", tensor) at 32 768 Ants and Humanoids: the transposition and mj_model_constants_kernel.

    python scripts/body_mass_bench.py --old /path/to/parent/libmi355env.so [--rounds 3] [--out profiles/body_mass_bench.txt]

Experiment infrastructure only: no test reads its numbers (docs/results_log.md holds them)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("HalfCheetah-v5", 32768), ("Ant-v5", 32768), ("Humanoid-v5", 32768), ("Hopper-v5", 65536))
T, WARMUP, LAUNCHES, WINDOWS = 8, 2, 4, 3


def child(env_id, n, config):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import gymnasium_amd

    env = gymnasium_amd.make_vec(env_id, num_envs=n, output="torch")
    sel = np.arange(n) % 3
    g = np.stack(env.get_attr("gravity")) * np.array([1.0, 0.6, 1.4])[sel][:, None]
    env.set_attr("gravity", torch.from_numpy(g).cuda())
    if config == "set":  # the time of one set_attr of the mass scale, after a first one (which loads the kernel)
        nb = len(env.get_attr("body_mass_scale")[0])
        s = torch.from_numpy(np.array([1.0, 0.6, 1.5])[sel][:, None] * np.ones((n, nb))).cuda()
        env.set_attr("body_mass_scale", s)
        times = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.set_attr("body_mass_scale", s)  # (returns after the engine's stream has run the kernels)
            times.append(time.perf_counter() - t0)
        env.close()
        print("RESULT " + json.dumps(sorted(times)[len(times) // 2]), flush=True)
        return
    if config == "mass":
        nb = len(env.get_attr("body_mass_scale")[0])
        env.set_attr("body_mass_scale", torch.from_numpy(np.array([1.0, 0.6, 1.5])[sel][:, None] * np.ones((n, nb))).cuda())
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


def run(env_id, n, config, library):
    env = {k: v for k, v in os.environ.items() if k not in ("MI355ENV_MJ_SERIAL", "MI355ENV_MJ_COOP", "MI355ENV_LIBRARY")}
    if library:
        env["MI355ENV_LIBRARY"] = library
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env_id, str(n), config], env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.exit(f"{env_id} {config} {library} failed ({p.returncode}): {p.stdout[-500:]} {p.stderr[-1500:]}")
    return json.loads(lines[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="libmi355env.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, default=None, metavar=("ENV_ID", "N", "CONFIG"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), args.child[2])
    configs = ([("old", "gravity", args.old)] if args.old else []) + [("new", "gravity", None), ("new+mass", "mass", None)]
    res = {}
    for _ in range(args.rounds):
        for env_id, n in CASES:
            for tag, config, library in configs:
                res.setdefault((env_id, tag), []).append(run(env_id, n, config, library))
    rows = [f"body_mass_bench: rollout({T}) of the per-lane kernels, {args.rounds} rounds interleaved, median of {WINDOWS} windows of {LAUNCHES} launches; M env-steps/s"]
    for env_id, n in CASES:
        med = {tag: sorted(res[env_id, tag])[len(res[env_id, tag]) // 2] / 1e6 for tag, _, _ in configs}
        row = f"{env_id} @ {n}: " + ", ".join(f"{tag} {med[tag]:.3f} (rounds {' '.join(f'{v / 1e6:.3f}' for v in res[env_id, tag])})" for tag, _, _ in configs)
        if args.old:
            spread = (max(res[env_id, "old"]) - min(res[env_id, "old"])) / med["old"] / 1e6
            row += f"; new / old = {med['new'] / med['old']:.3f} (run-to-run spread of old {100 * spread:.1f} %)"
        rows.append(row)
    for env_id, n in (("Ant-v5", 32768), ("Humanoid-v5", 32768)):
        rows.append(f"set_attr('body_mass_scale', tensor) @ {n} {env_id}: {1e3 * run(env_id, n, 'set', None):.3f} ms (median of 7)")
    text = "\n".join(rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
