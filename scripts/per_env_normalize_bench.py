"""CartPole-v1 x N with device tensors: what the per-sub-environment normalisations (wrappers.per_env) cost next to the bare env and to the vector pair.

  step      per-step wall time of env.step(a), of per_env.NormalizeReward(per_env.NormalizeObservation(env)).step(a) (ONE launch behind the step's) and
            of the vector NormalizeReward(NormalizeObservation(env)).step(a) (fused into the step kernel: two launches)
  rollout   env.rollout(T), the per_env pair's rollout(T) (the same launch + ONE trajectory pass) and the vector pair's (the whole-trajectory passes of
            wrappers.hip, as scripts/wrapped_rollout_bench.py measures them)
  pass      the trajectory pass alone (mi_per_env_normalize_steps over buffers that stay put), timed with events over `--reps` back-to-back launches:
            time, and achieved bytes per second for its algorithmic traffic -- one read and one write of the observation and reward blocks plus one read
            of the two flag blocks

The variants of a group alternate round by round in one process (warmed up, every measurement synchronised, each at least `--seconds` of work); one JSON
line with medians and min .. max in microseconds."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gymnasium_amd
from gymnasium_amd import _native, wrappers as gw
from gymnasium_amd.wrappers import per_env

ap = argparse.ArgumentParser()
ap.add_argument("--num-envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=200)
a = ap.parse_args()
import torch

N, T = a.num_envs, a.steps


def make(kind):
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, output="torch")
    w = env
    if kind == "per_env":
        w = per_env.NormalizeReward(per_env.NormalizeObservation(env))
    elif kind == "vector":
        w = gw.NormalizeReward(gw.NormalizeObservation(env))
    w.reset(seed=0)
    env.action_space.seed(0)
    return env, w


def alternate(variants, inner):
    times, spent = {k: [] for k in variants}, {k: 0.0 for k in variants}
    for f in variants.values():  # warm-up: kernels load on first use, the caching allocator learns the sizes
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    while min(spent.values()) < a.seconds:
        for k, f in variants.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            spent[k] += dt
            times[k].append(dt / inner)
    return {k: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "rounds": len(v)} for k, v in times.items()}


def step_group():
    variants = {}
    for kind in ("bare", "per_env", "vector"):
        env, w = make(kind)
        acts = torch.from_numpy(env.action_space.sample()).cuda()

        def run(w=w, acts=acts):
            for _ in range(100):
                w.step(acts)
        variants[kind] = run
    return alternate(variants, 100)


def rollout_group():
    variants = {}
    for kind in ("bare", "per_env", "vector"):
        _, w = make(kind)
        variants[kind] = lambda w=w: w.rollout(T)
    return alternate(variants, 1)


def trajectory_pass():
    env, w = make("per_env")
    out = env.rollout(T)
    obs, rew = out["obs"].contiguous(), out["rewards"].contiguous()
    te, tr = out["terminations"].view(torch.uint8), out["truncations"].view(torch.uint8)
    on, rn = w._pair()
    lib = _native.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def launch():
        lib.check(lib.per_env_normalize_steps(0, stream, C.byref(w._state(on, rn)), T, N, p(obs), p(obs), p(rew), p(te), p(tr), p(rew)))
        on._phase ^= 1

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    samples = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    traffic = 2 * obs.numel() * obs.element_size() + 2 * rew.numel() * 8 + 2 * te.numel()
    us = statistics.median(samples)
    return {"median_us": us, "min_us": min(samples), "max_us": max(samples), "bytes": traffic, "bytes_per_s": traffic / (us * 1e-6)}


print(json.dumps({"num_envs": N, "steps": T, "step": step_group(), "rollout": rollout_group(), "pass": trajectory_pass()}))
