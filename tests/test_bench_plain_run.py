"""bench.py without --full: set-up, warm-up, EXACTLY K timed launches and the line, nothing else; --dump-outputs writes what the last timed launch
computed.  Executed on the CPU checker through tests/bench_dryrun.py at world size 1 (the same control flow as on the GPU; the numbers are not
measurements), plus dump_outputs' sampling on its own."""
import json
import os
import subprocess
import sys

import numpy as np

import bench
from conftest import ROOT


def _dryrun(extra, num_envs=256, inner=8):
    env = dict(os.environ, OMP_NUM_THREADS="1", MI355ENV_CPU_WORKERS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_dryrun.py"), "--gpus", "1", "--num-envs", str(num_envs), "--inner", str(inner), *extra],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"exactly one line on stdout, got {len(lines)}"
    return json.loads(lines[0])


def _load(d):
    return [np.load(os.path.join(d, f"{name}.npy")) for name in bench.DUMP_NAMES]


def test_plain_run_times_exactly_k_launches_and_dumps_the_last(tmp_path):
    N, T, K = 256, 8, 3
    r = _dryrun(["--steps", str(K), "--warmup", "1", "--dump-outputs", str(tmp_path / "a")], num_envs=N, inner=T)
    assert r["steps"] == K and r["warmup"] == 1 and r["n_gpus"] == 1 and r["metric"] == bench.METRIC and r["unit"] == "env-steps/s"
    assert r["higher_is_better"] is True and r["dtype"] == "f64" and "oracle" in r["engine"]
    assert 0.8 * N * T * K < r["value"] * r["ms_per_step"] * 1e-3 * K <= N * T * K  # ms_per_step: one of the K launches; autoreset steps are not counted
    # what --full adds is not done
    assert r["cpu_baseline"] is None and r["verified"] is None and r["output_sha256"] is None and r["verified_all_ranks"] is None
    assert r["sustained"] is None and "secondary" not in r and "full" not in r
    assert r["roofline"]["algorithmic_bytes_per_launch"] == (34 * T + 96) * N
    # the dump is the LAST of the K launches: steps (K-1)T .. KT-1 of the rollout from reset(seed=0) under the policy seeded 0
    ref = bench.oracle_trajectory("CartPole-v1", N, K * T, offset=0, policy_seed=0)
    got = _load(tmp_path / "a")
    for name, g, x in zip(bench.DUMP_NAMES, got, ref):
        assert g.dtype == (np.float32 if x.dtype in (np.float32, np.bool_) else np.float64), name
        assert np.array_equal(g, x[-T:].astype(g.dtype)), name
    assert np.array_equal(np.load(tmp_path / "a" / "env_index.npy"), np.arange(N, dtype=np.float64))
    # the same arguments: the same outputs
    _dryrun(["--steps", str(K), "--warmup", "1", "--dump-outputs", str(tmp_path / "b")], num_envs=N, inner=T)
    assert all(np.array_equal(a, b) for a, b in zip(got, _load(tmp_path / "b")))


def test_full_run_keeps_the_checks():
    r = _dryrun(["--full", "--steps", "2", "--warmup", "1", "--sustained", "0", "--cpu-budget", "0.5"], num_envs=64, inner=4)
    assert r["verified"]["ok"] is True and r["verified_all_ranks"] is True and len(r["output_sha256"]) == 64
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["kind"] == "port"


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr


def test_dump_outputs_takes_a_fixed_sample_within_its_budget(tmp_path):
    T, N = 4, 1000
    rng = np.random.default_rng(1)
    traj = (rng.integers(0, 2, (T, N)), rng.random((T, N, 4)).astype(np.float32), rng.random((T, N)), rng.random((T, N)) < 0.1, rng.random((T, N)) < 0.1)
    per_env = 8 + T * (8 + 16 + 8 + 4 + 4)
    idx = bench.dump_outputs(str(tmp_path / "a"), traj, budget=100 * per_env)
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and np.array_equal(idx, bench.dump_outputs(str(tmp_path / "b"), traj, budget=100 * per_env))
    total = 0
    for name, a, d in zip(bench.DUMP_NAMES, traj, _load(tmp_path / "a")):
        assert d.dtype == (np.float32 if a.dtype in (np.float32, np.bool_) else np.float64) and np.array_equal(d, a[:, idx].astype(d.dtype)), name
        total += d.nbytes
    env_index = np.load(tmp_path / "a" / "env_index.npy")
    assert np.array_equal(env_index, idx.astype(np.float64)) and total + env_index.nbytes <= 100 * per_env
    # everything fits: no sample
    assert np.array_equal(bench.dump_outputs(str(tmp_path / "c"), traj), np.arange(N))
    # rank 1 of 2: files of its own, global indices, half the budget
    idx = bench.dump_outputs(str(tmp_path / "d"), traj, rank=1, world=2, budget=100 * per_env)
    assert len(idx) == 50 and np.array_equal(np.load(tmp_path / "d" / "rank1_env_index.npy"), idx + 1000.0)
    assert np.array_equal(np.load(tmp_path / "d" / "rank1_rewards.npy"), traj[2][:, idx])
