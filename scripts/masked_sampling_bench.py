"""What `action_space.sample(mask=...)` / `sample(probability=...)` cost on the device, one configuration several ways in one process, alternating round
by round:

  host      the space's own NumPy path (MultiDiscrete._apply_mask: a Python walk over the rows) -- what every masked call took before
  masked    env.action_space.sample(mask=<device tensor>)          mi_action_sample_masked, five launches
  masked_np env.action_space.sample(mask=<ndarray>)                the same through the staging copies (MI_HOST)
  weighted  env.action_space.sample(probability=<device tensor>)   mi_action_sample_weighted, three launches
  plain     one batch of the plain sampler (mi_action_sample, T = 1) into a device tensor: one launch
  step      env.step(<device tensor>): the step kernel the batch feeds

    python scripts/masked_sampling_bench.py --env Taxi-v4 --num-envs 65536 [--seconds 1.0] [--host-calls 3]

Every call is synchronised and timed on the host (3 warm-up calls per variant, then rounds until every device variant has `--seconds` of work; the host
path, seconds per call, runs `--host-calls` times).  One JSON line: median and min..max per variant in microseconds."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gymnasium_amd
from gymnasium_amd import _native
from gymnasium_amd.gym_api import batch_space

ap = argparse.ArgumentParser()
ap.add_argument("--env", default="Taxi-v4")
ap.add_argument("--num-envs", type=int, default=65536)
ap.add_argument("--seconds", type=float, default=1.0)
ap.add_argument("--host-calls", type=int, default=3)
a = ap.parse_args()
import torch

N = a.num_envs
env = gymnasium_amd.make_vec(a.env, num_envs=N, output="torch", sample_output="torch")
_, info = env.reset(seed=0)
env.action_space.seed(0)
A = int(env.single_action_space.n)
rng = np.random.default_rng(0)
masks = np.ascontiguousarray(info["action_mask"]) if "action_mask" in info else (rng.random((N, A)) < 0.6).astype(np.int8)
w = rng.random((N, A)) + 0.01
probs = np.ascontiguousarray(w / w.sum(axis=1, keepdims=True))
d_masks, d_probs = torch.from_numpy(masks).cuda(), torch.from_numpy(probs).cuda()
actions = env.action_space.sample(mask=d_masks)
plain_out = torch.empty((N,), dtype=torch.int64, device="cuda")
eng = env._engine


def plain():
    env.action_space.hip_use_stream()
    eng.action_sample(1, plain_out.data_ptr(), _native.MI_DEVICE)


variants = {"masked": lambda: env.action_space.sample(mask=d_masks), "masked_np": lambda: env.action_space.sample(mask=masks),
            "weighted": lambda: env.action_space.sample(probability=d_probs), "plain": plain, "step": lambda: env.step(actions)}
host_space = batch_space(env.single_action_space, N)
host_space.seed(0)
mask_rows = tuple(masks)
out = {"env": a.env, "num_envs": N, "actions": A, "mask_ones_per_row": float(masks.sum(axis=1).mean())}
host = []
for _ in range(max(1, a.host_calls)):
    t0 = time.perf_counter()
    host_space.sample(mask=mask_rows)
    host.append(time.perf_counter() - t0)
times = {k: [] for k in variants}
for f in variants.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
while min(sum(v) for v in times.values()) < a.seconds or len(times["masked"]) < 3:
    for k, f in variants.items():
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
env.synchronize()
out["rounds"] = len(times["masked"])
out["host"] = {"median_us": statistics.median(host) * 1e6, "min_us": min(host) * 1e6, "max_us": max(host) * 1e6, "calls": len(host)}
for k, v in times.items():
    out[k] = {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6}
print(json.dumps(out))
