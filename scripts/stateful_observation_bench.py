"""CartPole-v1 x N with device tensors: what per_env.FrameStackObservation(env, 4) costs next to the bare env and to the torch ops a user would
otherwise write.

  step      per-step wall time of env.step(a) and of FrameStackObservation(env, 4).step(a) (ONE launch behind the step's)
  rollout   env.rollout(T) and the wrapper's rollout(T) (the same launch + ONE trajectory pass, a torch.empty for its output and a copy of the last stack)
  pass      the trajectory pass alone (mi_stateful_observation_steps into a buffer that stays put), timed with events over `--reps` back-to-back
            launches, next to a torch composition of the same result -- unfold over the trajectory extended by the carried frames, then the
            episode-boundary padding as cummax / gather / where over the reset flags -- which is checked against the wrapper's output first.  Achieved
            bytes per second are over the bytes the pass must move: T N D elements and the two flag blocks read, T N k D elements written; the
            fraction is of the HBM peak bench.py uses.

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
from gymnasium_amd import _native
from gymnasium_amd.wrappers import per_env

ap = argparse.ArgumentParser()
ap.add_argument("--num-envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--stack", type=int, default=4)
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=100)
a = ap.parse_args()
import torch

N, T, K = a.num_envs, a.steps, a.stack
HBM_PEAK_GBS = 8000.0  # bench.py's roofline: the 8.0 TB/s spec (a float4 copy measures 6.29 TB/s)


def make(kind):
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, output="torch")
    w = per_env.FrameStackObservation(env, K) if kind == "stack" else env
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
    for kind in ("bare", "stack"):
        env, w = make(kind)
        acts = torch.from_numpy(env.action_space.sample()).cuda()

        def run(w=w, acts=acts):
            for _ in range(100):
                w.step(acts)
        variants[kind] = run
    return alternate(variants, 100)


def rollout_group():
    variants = {}
    for kind in ("bare", "stack"):
        _, w = make(kind)
        variants[kind] = lambda w=w: w.rollout(T)
    return alternate(variants, 1)


def torch_stack(carried, obs, done, pending):
    """FrameStackObservation(padding_type="reset") over a NEXT_STEP trajectory with torch ops: carried [N, K, D] (the last stack), obs [T, N, D],
    done [T, N] bool (terminated | truncated), pending [N] bool -> [T, N, K, D]."""
    steps = obs.shape[0]
    extended = torch.cat([carried[:, 1:].transpose(0, 1), obs]) if K > 1 else obs  # steps -(K - 1) .. T - 1
    windows = extended.unfold(0, K, 1).permute(0, 1, 3, 2)  # [T, N, K, D]: slot j of step t is step t - (K - 1 - j)
    resets = torch.cat([pending[None], done[:-1]])  # the row resets AT step t
    at = torch.arange(steps, device=obs.device)
    latest = torch.where(resets, at[:, None], -1).cummax(0).values  # [T, N]: the latest reset up to t, or -1
    source = at[:, None] - (K - 1 - torch.arange(K, device=obs.device))[None, :]  # [T, K]
    padded = (latest[:, :, None] >= 0) & (latest[:, :, None] > source[:, None, :])  # the slot's step lies before that reset
    reset_obs = obs.gather(0, latest.clamp(min=0)[:, :, None].expand(-1, -1, obs.shape[2]))  # [T, N, D]
    return torch.where(padded[..., None], reset_obs[:, :, None, :], windows)


def trajectory_pass():
    env, w = make("stack")
    w.rollout(7)  # (state to carry in: frames of running episodes, pending rows)
    carried, pending = w._last.clone(), torch.from_numpy(w.pending_autoreset).cuda()
    out = env.rollout(T)
    obs = out["obs"].contiguous()
    te, tr = out["terminations"].view(torch.uint8), out["truncations"].view(torch.uint8)
    done = out["terminations"] | out["truncations"]
    res = torch.empty((T, N, K) + tuple(obs.shape[2:]), dtype=obs.dtype, device=obs.device)
    lib = _native.load_library()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    state = w._state()  # (the same carried state for every launch: nothing is swapped)

    def launch():
        lib.check(lib.stateful_observation_steps(0, stream, C.byref(state), T, N, p(obs), p(res), p(te), p(tr)))

    launch()
    composed = torch_stack(carried, obs, done, pending)
    assert composed.shape == res.shape and torch.equal(composed, res), "the torch composition and the kernel disagree"
    assert bool(done.any()) and bool((res[:, :, 0] == res[:, :, -1]).all(-1).any()), "no padded stack in the trajectory"
    del composed
    timings = {}
    for name, f, reps in (("kernel", launch, a.reps), ("torch", lambda: torch_stack(carried, obs, done, pending), max(a.reps // 10, 3))):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        samples = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) * 1e3 / reps)
        timings[name] = samples
    traffic = obs.numel() * obs.element_size() + 2 * te.numel() + res.numel() * res.element_size()
    us = statistics.median(timings["kernel"])
    rate = traffic / (us * 1e-6)
    return {"median_us": us, "min_us": min(timings["kernel"]), "max_us": max(timings["kernel"]), "bytes": traffic, "bytes_per_s": rate,
            "hbm_fraction": rate / (HBM_PEAK_GBS * 1e9), "torch_median_us": statistics.median(timings["torch"]), "torch_min_us": min(timings["torch"]),
            "torch_max_us": max(timings["torch"])}


print(json.dumps({"num_envs": N, "steps": T, "stack": K, "step": step_group(), "rollout": rollout_group(), "pass": trajectory_pass()}))
