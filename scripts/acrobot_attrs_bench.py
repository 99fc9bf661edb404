"""Acrobot's per-sub-environment kernels against its uniform kernel at 65 536 x 128, one MI355X.

    python scripts/acrobot_attrs_bench.py [--out profiles/acrobot_attrs.txt]

rollout(T) of the collector's configuration (NEXT_STEP, on-device policy, all outputs) in three configurations, interleaved round by round:
  (i)   the uniform kernel (no set_attr)
  (ii)  two attributes randomised per sub-environment (LINK_MASS_2, LINK_COM_POS_2); the other nine are the defaults, no noise
  (iii) all eleven set per sub-environment, torque noise on in every sub-environment (one draw of its generator per step), half of them "nips"
Times are device events around REPS launches after a warm-up launch, median of ROUNDS.  The register figures of the kernels that ran are
appended from the library's metadata (scripts/kernel_resources.py).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import gymnasium_amd  # noqa: E402

N, T, REPS, ROUNDS = 65536, 128, 10, 7


def make(config):
    env = gymnasium_amd.make_vec("Acrobot-v1", num_envs=N, output="torch")
    env.reset(seed=0)
    env.action_space.seed(1)
    g = torch.Generator(device="cuda").manual_seed(2)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(N, device="cuda", dtype=torch.float64, generator=g)  # noqa: E731
    if config == "two":
        env.set_attr("LINK_MASS_2", u(0.8, 1.2)), env.set_attr("LINK_COM_POS_2", u(0.4, 0.6))
    elif config == "all":
        for name, lo, hi in (("LINK_LENGTH_1", 0.8, 1.2), ("LINK_MASS_1", 0.8, 1.2), ("LINK_MASS_2", 0.8, 1.2), ("LINK_COM_POS_1", 0.4, 0.6),
                             ("LINK_COM_POS_2", 0.4, 0.6), ("LINK_MOI", 0.8, 1.2), ("MAX_VEL_1", 10.0, 14.0), ("MAX_VEL_2", 24.0, 30.0),
                             ("dt", 0.15, 0.25), ("torque_noise_max", 0.5, 1.5)):
            env.set_attr(name, u(lo, hi))
        env.set_attr("book_or_nips", ["book", "nips"] * (N // 2))
    return env


def time_rollout(env):
    env.rollout(T)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        env.rollout(T)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / REPS  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    envs = {k: make(k) for k in ("uniform", "two", "all")}
    r = {k: [] for k in envs}
    for _ in range(ROUNDS):
        for k, env in envs.items():
            r[k].append(time_rollout(env))
    m = {k: float(np.median(v)) for k, v in r.items()}
    rate = lambda us: N * T / (us * 1e-6)  # noqa: E731
    lines = [f"Acrobot-v1 rollout(), N={N}, T={T}, NEXT_STEP, on-device policy, all outputs; us per launch (device events, median of {ROUNDS} x {REPS}, "
             "configurations interleaved)",
             f"(i)   uniform kernel                 {m['uniform']:9.1f} us  {rate(m['uniform']):.3e} env-steps/s",
             f"(ii)  two attributes per lane        {m['two']:9.1f} us  {rate(m['two']):.3e} env-steps/s  ratio to (i) {m['uniform'] / m['two']:.3f}",
             f"(iii) all eleven per lane, noise on  {m['all']:9.1f} us  {rate(m['all']):.3e} env-steps/s  ratio to (i) {m['uniform'] / m['all']:.3f}",
             "rounds (us): " + "; ".join(f"{k} " + " ".join(f"{v:.0f}" for v in vs) for k, vs in r.items())]
    for env in envs.values():
        env.close()
    from kernel_resources import resources

    lines.append("registers (VGPR + AGPR) / spilled / SGPR / LDS bytes / scratch bytes of the Acrobot step and rollout kernels:")
    for row in resources(os.path.join(ROOT, "gymnasium_amd", "csrc", "libmi355env.so")):
        if "Acrobot" in row["name"] and "FastMath" not in row["name"] and ("rollout" in row["name"] or "step_kernel" in row["name"]):
            lines.append(f"  {row['vgpr_count']:>4} {row.get('vgpr_spill_count', '0'):>3} {row['sgpr_count']:>4} {row['group_segment_fixed_size']:>6} "
                         f"{row['private_segment_fixed_size']:>4}  {row['name'].split('(')[0][:150]}")
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
