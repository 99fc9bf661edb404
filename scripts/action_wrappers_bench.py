"""Pendulum-v1 x N with device tensors: what ClipAction's extra launch (mi_transform_actions) costs, several ways in one process:

  step_raw      K x env.step(a)                          the bare step
  step_wrapped  K x w.step(a)                            ClipAction: one transform launch + the step
  step_clamp    K x env.step(torch.clamp(a, lo, hi))     the clamp by hand: one torch launch + the step
  roll_raw      env.rollout(T, actions)                  the bare rollout over a given [T, N, 1] block
  roll_wrapped  w.rollout(T, actions)                    one transform launch over the block + the rollout
  pass_f32      the transform pass alone over the [T, N, 1] float32 block (8 bytes per element: 4 read, 4 written)
  pass_f64      the same over a float64 block (12 bytes per element)
  pass_f32_a8   the float32 pass over [T, N / 8, 8]: the same bytes with eight parameter rows (an Ant-shaped block)

The variants alternate round by round (warmed up, every measurement synchronised, each at least `--seconds` of work in total); the result line
has the median and the min..max spread of every variant in microseconds per call, and for the passes the bytes per second the median stands
for.  `--only NAME` runs one variant alone (for `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gymnasium_amd
from gymnasium_amd import wrappers as gw
from gymnasium_amd.gym_api import batch_space, spaces

ap = argparse.ArgumentParser()
ap.add_argument("--num-envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=128, help="T of the rollouts and of the transformed block")
ap.add_argument("--step-calls", type=int, default=64, help="K: step() calls per measurement")
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--only", default=None)
a = ap.parse_args()
import numpy as np
import torch

N, T, K = a.num_envs, a.steps, a.step_calls
PASSES = 20  # transform passes per measurement: one alone is shorter than the synchronise behind it
gen = torch.Generator(device="cuda").manual_seed(0)
block = (torch.rand((T, N, 1), device="cuda", generator=gen) * 6.0 - 3.0).contiguous()  # a third of the entries outside +-2
batch = block[0].contiguous()


def pendulum():
    env = gymnasium_amd.make_vec("Pendulum-v1", num_envs=N, output="torch")
    env.reset(seed=0)
    return env


def make_step_raw():
    env = pendulum()
    return lambda: [env.step(batch) for _ in range(K)]


def make_step_wrapped():
    w = gw.ClipAction(pendulum())
    return lambda: [w.step(batch) for _ in range(K)]


def make_step_clamp():
    env = pendulum()
    lo, hi = (torch.from_numpy(b).cuda() for b in (env.single_action_space.low, env.single_action_space.high))
    return lambda: [env.step(torch.clamp(batch, lo, hi)) for _ in range(K)]


def make_roll_raw():
    env = pendulum()
    return lambda: env.rollout(T, block)


def make_roll_wrapped():
    w = gw.ClipAction(pendulum())
    return lambda: w.rollout(T, block)


class _Spaces:  # a vector env that has only spaces: the pass alone needs no engine
    metadata = {}

    def __init__(self, dim, rows):
        self.num_envs = rows
        self.single_action_space = spaces.Box(-2.0, 2.0, shape=(dim,), dtype=np.float32)
        self.action_space = batch_space(self.single_action_space, rows)


def make_pass(dtype, dim):
    w = gw.ClipAction(_Spaces(dim, N // dim))
    x = block.to(dtype).reshape(T, N // dim, dim).contiguous()
    return lambda: [w._actions_of_steps(x, T) for _ in range(PASSES)]


makers = {"step_raw": make_step_raw, "step_wrapped": make_step_wrapped, "step_clamp": make_step_clamp, "roll_raw": make_roll_raw,
          "roll_wrapped": make_roll_wrapped, "pass_f32": lambda: make_pass(torch.float32, 1), "pass_f64": lambda: make_pass(torch.float64, 1),
          "pass_f32_a8": lambda: make_pass(torch.float32, 8)}
pass_bytes = {"pass_f32": 8 * T * N, "pass_f64": 12 * T * N, "pass_f32_a8": 8 * T * N}
calls = {"step_raw": K, "step_wrapped": K, "step_clamp": K, "pass_f32": PASSES, "pass_f64": PASSES, "pass_f32_a8": PASSES}
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
out = {"num_envs": N, "steps": T, "step_calls": K, "rounds": len(next(iter(times.values())))}
for k, v in times.items():
    per = calls.get(k, 1)
    out[k] = {"median_us": statistics.median(v) * 1e6 / per, "min_us": min(v) * 1e6 / per, "max_us": max(v) * 1e6 / per}
    if k in pass_bytes:
        out[k]["bytes"] = pass_bytes[k]
        out[k]["bytes_per_s"] = pass_bytes[k] * per / statistics.median(v)
print(json.dumps(out))
