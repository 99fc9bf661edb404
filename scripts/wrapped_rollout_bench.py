"""CartPole-v1 x N, T steps through ClipReward(NormalizeReward(NormalizeObservation(env))), three ways in one process:

  raw      env.rollout(T)            the bare trajectory (one launch)
  wrapped  w.rollout(T)              the same rollout + the whole-trajectory wrapper passes (mi_normalize_*_steps, mi_clip_reward)
  steps    T x w.step(actions[t])    the wrappers as the step kernel's output stage: two launches per step

The three alternate round by round (warmed up, every measurement synchronised, each variant at least `--seconds` of work in total); the
result line has the median and the min..max spread of every variant in microseconds per T steps.  `--only wrapped` runs one variant alone
(for `rocprofv3 --kernel-trace --stats`, profiles/wrapped_rollout.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gymnasium_amd
from gymnasium_amd import wrappers as gw

ap = argparse.ArgumentParser()
ap.add_argument("--num-envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--only", default=None, choices=["raw", "wrapped", "steps"])
a = ap.parse_args()
import torch

N, T = a.num_envs, a.steps


def wrapped_env():
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, output="torch")
    w = gw.ClipReward(gw.NormalizeReward(gw.NormalizeObservation(env)), -5.0, 5.0)
    w.reset(seed=0)
    env.action_space.seed(0)
    return env, w


def make_raw():
    raw = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, output="torch")
    raw.reset(seed=0)
    raw.action_space.seed(0)
    return lambda: raw.rollout(T)


def make_wrapped():
    _, w = wrapped_env()
    return lambda: w.rollout(T)


def make_steps():
    env, w = wrapped_env()
    acts = torch.from_numpy(env.action_space.sample()).cuda()

    def run():
        for _ in range(T):
            w.step(acts)
    return run


makers = {"raw": make_raw, "wrapped": make_wrapped, "steps": make_steps}
variants = {k: make() for k, make in makers.items() if a.only in (None, k)}
times = {k: [] for k in variants}
for f in variants.values():  # warm-up: kernels load on first use, the caching allocator learns the sizes
    for _ in range(3):
        f()
torch.cuda.synchronize()
while min(sum(v) for v in times.values()) < a.seconds:
    for k, f in variants.items():
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
out = {"num_envs": N, "steps": T, "rounds": len(next(iter(times.values())))}
for k, v in times.items():
    out[k] = {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6,
              "env_steps_per_s": N * T / statistics.median(v)}
print(json.dumps(out))
