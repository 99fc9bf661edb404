"""Per-sub-environment attributes (set_attr) against the uniform kernels at 65 536 x 128, one MI355X.

    python scripts/env_attrs_bench.py [--out profiles/env_attrs_ab.txt]

Per environment: rollout(T) of the collector's configuration (NEXT_STEP, on-device policy, all outputs) -- uniform one-role kernel
(MI355ENV_ROLLOUT_DUO=0), uniform two-role kernel (the default, for context) and the per-lane kernel with three attributes varying per
sub-environment -- and step() with device tensors, uniform against per-lane.  Times are device events around REPS launches after a warm-up,
alternating the configurations, median of ROUNDS.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gymnasium_amd  # noqa: E402

N, T, REPS, ROUNDS, STEPS = 65536, 128, 10, 5, 200
VARY = {"CartPole-v1": ("length", "masspole", "force_mag"), "Pendulum-v1": ("g", "m", "l"),
        "MountainCar-v0": ("force", "gravity", "max_speed"), "MountainCarContinuous-v0": ("power", "max_speed", "goal_position")}


def make(env_id, per_lane):
    env = gymnasium_amd.make_vec(env_id, num_envs=N, output="torch")
    env.reset(seed=0)
    env.action_space.seed(1)
    if per_lane:
        g = torch.Generator(device="cuda").manual_seed(2)
        for name in VARY[env_id]:
            base = env.get_attr(name)[0]
            env.set_attr(name, base * (0.8 + 0.4 * torch.rand(N, device="cuda", dtype=torch.float64, generator=g)))
    return env


def time_rollout(env, duo):
    os.environ["MI355ENV_ROLLOUT_DUO"] = "1" if duo else "0"
    env.rollout(T)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        env.rollout(T)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / REPS  # us per launch


def time_step(env):
    a = torch.from_numpy(env.action_space.sample()).cuda()
    for _ in range(10):
        env.step(a)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        env.step(a)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / STEPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"per-lane attributes vs uniform kernels, N={N}, T={T}; rollout: us per launch (device events, median of {ROUNDS} x {REPS}); "
             f"step(): us per call with device tensors (host clock, {STEPS} calls)"]
    for env_id in VARY:
        uni, lane = make(env_id, False), make(env_id, True)
        r = {"one": [], "duo": [], "lane": [], "step_u": [], "step_l": []}
        for _ in range(ROUNDS):
            r["one"].append(time_rollout(uni, False))
            r["lane"].append(time_rollout(lane, False))
            r["duo"].append(time_rollout(uni, True))
            r["step_u"].append(time_step(uni))
            r["step_l"].append(time_step(lane))
        m = {k: float(np.median(v)) for k, v in r.items()}
        rate = lambda us: N * T / (us * 1e-6)  # noqa: E731
        lines.append(f"{env_id:26s} rollout one-role uniform {m['one']:8.1f} us ({rate(m['one']):.3e} env-steps/s)  per-lane {m['lane']:8.1f} us "
                     f"({rate(m['lane']):.3e})  ratio {m['one'] / m['lane']:.3f}  | two-role uniform {m['duo']:8.1f} us ({rate(m['duo']):.3e})  "
                     f"| step() uniform {m['step_u']:.2f} us  per-lane {m['step_l']:.2f} us  (+{m['step_l'] - m['step_u']:.2f})  "
                     f"[varying: {', '.join(VARY[env_id])}]")
        print(lines[-1], flush=True)
        uni.close(), lane.close()
    os.environ.pop("MI355ENV_ROLLOUT_DUO", None)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
