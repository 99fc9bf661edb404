"""What the infos of a rollout cost: one configuration three ways in one process, alternating round by round,

  plain  env.rollout(T)                  the bare trajectory (mi_rollout)
  infos  env.rollout(T, infos=True)      the same steps with final observations / episode statistics / info columns stored per step (mi_rollout_infos)
  steps  T x env.step(actions)           the only way to those values before: one launch per step, device-resident infos

    python scripts/rollout_infos_bench.py --env CartPole-v1 --num-envs 65536 --steps 128 --mode SameStep [--stats] [--seconds 1.0]

Every call is synchronised and timed on the host (3 warm-up calls per variant, then rounds until every variant has `--seconds` of work).  The
result line has the median and the min..max spread per variant in microseconds per T steps, and the algorithmic bytes per sub-environment
step of the two rollouts (the tensors the call returns, summed, over T * N) next to the HBM time those bytes alone would take."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gymnasium_amd

ap = argparse.ArgumentParser()
ap.add_argument("--env", default="CartPole-v1")
ap.add_argument("--num-envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--mode", default="SameStep", choices=["NextStep", "SameStep"])
ap.add_argument("--stats", action="store_true", help="record_episode_statistics=True")
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth for the roofline column (MI355X: 8 TB/s)")
a = ap.parse_args()
import torch

N, T = a.num_envs, a.steps


def make():
    env = gymnasium_amd.make_vec(a.env, num_envs=N, output="torch", autoreset_mode=a.mode, record_episode_statistics=a.stats)
    env.reset(seed=0)
    env.action_space.seed(0)
    return env


def nbytes(x):
    if isinstance(x, dict):
        return sum(nbytes(v) for v in x.values())
    return x.numel() * x.element_size()


envs = {k: make() for k in ("plain", "infos", "steps")}
acts = torch.from_numpy(envs["steps"].action_space.sample()).cuda()


def run_steps():
    env = envs["steps"]
    for _ in range(T):
        env.step(acts)


variants = {"plain": lambda: envs["plain"].rollout(T), "infos": lambda: envs["infos"].rollout(T, infos=True), "steps": run_steps}
out = {"env": a.env, "num_envs": N, "steps": T, "mode": a.mode, "stats": a.stats}
for k in ("plain", "infos"):  # algorithmic bytes: what the kernels store for the call (the trajectory tensors; for "infos" also the extras' arrays --
    res = variants[k]()       # the masks and "t" of the dict are torch arithmetic on the done flags, not stores of the rollout)
    keys = {x: nbytes(v) for x, v in res.items() if x != "infos"}
    if k == "infos":
        keys["infos"] = nbytes(envs["infos"]._rollout_extra_buffers(T))
    b = sum(keys.values()) / (T * N)
    out[k + "_bytes_per_env_step"] = b
    out[k + "_hbm_floor_us"] = b * T * N / (a.hbm_gbs * 1e9) * 1e6
times = {k: [] for k in variants}
for f in variants.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
while min(sum(v) for v in times.values()) < a.seconds or len(times["plain"]) < 3:
    for k, f in variants.items():
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
out["rounds"] = len(times["plain"])
for k, v in times.items():
    out[k] = {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6, "env_steps_per_s": N * T / statistics.median(v)}
print(json.dumps(out))
