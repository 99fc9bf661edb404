"""CPU side of wrappers.per_env.NormalizeObservation / NormalizeReward (one set of running statistics per sub-environment): the NumPy restatement and
the arithmetic header, compiled for the host, reproduce the fixtures recorded from the reference bit for bit; the constructors validate and refuse as
documented; the fixture generator reproduces its files.  What the kernels compute is a GPU matter (tests/test_gpu_per_env_normalize.py)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import AutoresetMode, error, spaces
from gymnasium_amd.wrappers import per_env
from conftest import GOLDEN, REFERENCE, ROOT

import per_env_normalize_cases as cases

KEYS = [f"{k}_{m}" for k in cases.IDS for m in cases.MODES]
FILES = sorted([f"per_env_normalize_{k}.npz" for k in KEYS] + ["per_env_normalize_float64_replay.npz"])


def check_replay(fix, mode, dtype, **impl):
    got = cases.replay(fix, mode, dtype, **impl)
    assert got["obs0"].dtype == np.float32 and got["obs"].dtype == np.float32 and got["reward"].dtype == np.float64
    assert np.array_equal(got["obs0"], fix["obs0"])
    assert np.array_equal(got["obs"], fix["obs"])
    assert np.array_equal(got["reward"], fix["reward"])
    if mode == "same":
        assert fix["final_mask"].any() and np.array_equal(got["final_obs"], fix["final_obs"])
    if mode == "disabled":
        assert fix["reset_mask"].any() and np.array_equal(got["reset_obs"], fix["reset_obs"])
    on, rn = got["on"], got["rn"]
    for name, have in (("obs_mean", on.mean), ("obs_var", on.var), ("obs_count", on.count), ("ret_mean", rn.mean), ("ret_var", rn.var),
                       ("ret_count", rn.count), ("acc", rn.acc)):
        assert have.dtype == fix[name].dtype and np.array_equal(have, fix[name]), name


# -- 1. the restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_the_reference(key):
    fix = cases.fixture(key)
    assert fix["obs"].shape[:2] == (cases.T, cases.N) and fix["raw_obs"].dtype == np.float32
    check_replay(fix, key.rsplit("_", 1)[1], np.float32)


def test_restatement_reproduces_the_float64_stream_and_its_first_update():
    fix = cases.fixture("float64_replay")
    assert fix["raw_obs"].dtype == np.float64 and fix["obs_mean"].dtype == np.float64
    check_replay(fix, "disabled", np.float64)

    class NoQuirk(cases.ObsNormalizer):  # the recurrence in float64 throughout: the fixture must tell it from the reference's
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.first[:] = False

    got = cases.replay(fix, "disabled", np.float64, obs_cls=NoQuirk)
    assert not (np.array_equal(got["obs"], fix["obs"]) and np.array_equal(got["obs0"], fix["obs0"]))


def test_fixture_coverage():
    fix = cases.fixture("cartpole_next")
    assert fix["term"].sum() >= 50 and (fix["trunc"] & ~fix["term"]).sum() >= 10
    pend = cases.fixture("pendulum_next")
    assert not pend["term"].any() and pend["trunc"].sum() >= cases.N and np.all(pend["acc"] != 0.0)  # truncation never clears the accumulator
    for name in FILES:
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 500_000, name


# -- 2. the arithmetic header on the host ---------------------------------------------------------------------------------------------------------
SHIM = r"""
#include <stdint.h>
#include "per_env_normalize_internal.h"
using namespace mi_per_env;
extern "C" {
void pen_obs_f32(int rows, int dim, const uint8_t *mask, const float *x, float *mean, float *var, double *count, int update, double eps, float *out) {
    for (int r = 0; r < rows; r++) {
        if (!mask[r]) continue;
        double after = count[r];
        for (int k = 0; k < dim; k++) {
            const int i = r * dim + k;
            double c = count[r];
            if (update) update_f32(x[i], mean[i], var[i], c);
            out[i] = normalize_f32(x[i], mean[i], var[i], eps);
            after = c;
        }
        count[r] = after;
    }
}
void pen_obs_f64(int rows, int dim, const uint8_t *mask, const double *x, double *mean, double *var, double *count, uint8_t *first, int update, double eps,
                 float *out) {
    for (int r = 0; r < rows; r++) {
        if (!mask[r]) continue;
        double after = count[r];
        for (int k = 0; k < dim; k++) {
            const int i = r * dim + k;
            double c = count[r];
            if (update) update_f64(x[i], mean[i], var[i], c, first[r] != 0);
            out[i] = normalize_f64(x[i], mean[i], var[i], eps);
            after = c;
        }
        count[r] = after;
        if (update) first[r] = 0;
    }
}
void pen_reward(int rows, const uint8_t *live, const double *reward, const uint8_t *terminated, double gamma, int update, double eps, double *acc,
                double *mean, double *var, double *count, double *out) {
    for (int r = 0; r < rows; r++) {
        out[r] = 0.0;
        if (!live[r]) continue;
        reward_step(reward[r], terminated[r] != 0, gamma, update != 0, acc[r], mean[r], var[r], count[r]);
        out[r] = normalize_reward(reward[r], var[r], eps);
    }
}
}
"""


@pytest.fixture(scope="module")
def header_lib(tmp_path_factory):
    cxx = shutil.which("g++") or (os.environ.get("HIPCC", "/opt/rocm/bin/hipcc") if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) else None)
    if cxx is None:
        pytest.skip("no C++ compiler to build the arithmetic header for the host with")
    d = tmp_path_factory.mktemp("per_env_header")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    cmd = [cxx] + ([] if cxx.endswith("g++") else ["-x", "c++"]) + ["-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                                                                   "-I", os.path.join(ROOT, "gymnasium_amd", "csrc"), "-o", str(d / "libshim.so"), str(src)]
    subprocess.run(cmd, check=True)
    return C.CDLL(str(d / "libshim.so"))


def _p(a):
    return C.c_void_p(a.ctypes.data)


def header_classes(lib):
    lib.pen_obs_f32.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_double, C.c_void_p]
    lib.pen_obs_f64.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_double, C.c_void_p]
    lib.pen_reward.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_double, C.c_int, C.c_double] + [C.c_void_p] * 5
    for f in (lib.pen_obs_f32, lib.pen_obs_f64, lib.pen_reward):
        f.restype = None

    class HeaderObs(cases.ObsNormalizer):
        def observe(self, x, rows=None):
            x = np.ascontiguousarray(x, dtype=self.dtype)
            n, dim = x.shape
            mask = (np.ones(n, dtype=bool) if rows is None else np.asarray(rows, dtype=bool)).view(np.uint8).copy()
            out = self.last.copy()
            first = self.first.view(np.uint8)
            if self.dtype == np.float32:
                lib.pen_obs_f32(n, dim, _p(mask), _p(x), _p(self.mean), _p(self.var), _p(self.count), int(self.update_running_mean), self.epsilon, _p(out))
            else:
                lib.pen_obs_f64(n, dim, _p(mask), _p(x), _p(self.mean), _p(self.var), _p(self.count), _p(first), int(self.update_running_mean),
                                self.epsilon, _p(out))
            self.last = out
            return out

    class HeaderReward(cases.RewardNormalizer):
        def step(self, reward, terminated, truncated):
            reward = np.ascontiguousarray(reward, dtype=np.float64)
            te = np.ascontiguousarray(terminated, dtype=bool).view(np.uint8)
            live = (~self.was_done if self.mode == "next" else np.ones(len(reward), dtype=bool)).view(np.uint8).copy()
            out = np.empty(len(reward))
            lib.pen_reward(len(reward), _p(live), _p(reward), _p(te), self.gamma, int(self.update_running_mean), self.epsilon, _p(self.acc), _p(self.mean),
                           _p(self.var), _p(self.count), _p(out))
            self.was_done = np.asarray(terminated, dtype=bool) | np.asarray(truncated, dtype=bool)
            return out

    return dict(obs_cls=HeaderObs, reward_cls=HeaderReward)


@pytest.mark.parametrize("key", KEYS)
def test_header_on_the_host_reproduces_the_float32_fixtures(header_lib, key):
    check_replay(cases.fixture(key), key.rsplit("_", 1)[1], np.float32, **header_classes(header_lib))


def test_header_on_the_host_reproduces_the_float64_fixture(header_lib):
    check_replay(cases.fixture("float64_replay"), "disabled", np.float64, **header_classes(header_lib))


# -- 3. validation, refusals, stacking --------------------------------------------------------------------------------------------------------------
def make(env_id, factory, **kw):
    return gymnasium_amd.make_vec(env_id, num_envs=4, _engine_factory=factory, **kw)


@pytest.fixture
def device_engine(monkeypatch):
    """Lets the host classes be constructed over the checker backend: nothing in these tests reaches the statistics."""
    monkeypatch.setattr(per_env, "_require_device_engine", lambda base, what: None)


def test_constructors_validate_like_the_reference_then_ask_for_the_device_engine(oracle_factory):
    assert {"per_env_normalize_step", "per_env_normalize_steps"} <= set(_native.WRAPPER_SYMBOLS)
    env = make("CartPole-v1", oracle_factory)
    for bad in (0, -1e-8):
        with pytest.raises(error.InvalidBound, match="epsilon"):
            per_env.NormalizeObservation(env, epsilon=bad)
        with pytest.raises(error.InvalidBound, match="epsilon"):
            per_env.NormalizeReward(env, epsilon=bad)
    for bad in (-0.1, 1.01):
        with pytest.raises(error.InvalidBound, match="gamma"):
            per_env.NormalizeReward(env, gamma=bad)
    with pytest.raises(error.Error, match="device engine"):
        per_env.NormalizeObservation(env)
    with pytest.raises(error.Error, match="device engine"):
        per_env.NormalizeReward(env, gamma=1.0)
    env.close()


@pytest.mark.parametrize("env_id", ["FrozenLake-v1", "Blackjack-v1"])
def test_discrete_and_tuple_observations_are_refused(oracle_factory, device_engine, env_id):
    env = make(env_id, oracle_factory)
    with pytest.raises(error.Error, match="FlattenObservation"):
        per_env.NormalizeObservation(env)
    w = per_env.NormalizeReward(env)  # rewards are float64 [N] everywhere
    assert w._pair() == (None, w)
    env.close()


def test_stacking_rules(oracle_factory, device_engine, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    on = per_env.NormalizeObservation(env)
    assert on.single_observation_space == spaces.Box(-np.inf, np.inf, (4,), np.float32) and on.observation_space.shape == (4, 4)
    assert on._pair() == (on, None) and on.update_running_mean is True
    with pytest.raises(error.Error, match="at most one"):
        per_env.NormalizeObservation(on)
    rn = per_env.NormalizeReward(on, gamma=0.9)
    assert rn._pair() == (on, rn) and rn.obs_rms is on.obs_rms and rn.gamma == 0.9
    for build in (lambda: per_env.NormalizeReward(rn), lambda: per_env.NormalizeObservation(rn)):
        with pytest.raises(error.Error, match="at most one"):
            build()
    env2 = make("CartPole-v1", oracle_factory)
    on2 = per_env.NormalizeObservation(per_env.NormalizeReward(env2))  # the other order
    assert on2._pair() == (on2, on2.env) and on2.return_rms is on2.env.return_rms
    # every vector wrapper goes ABOVE them ...
    top = wrappers.RecordEpisodeStatistics(wrappers.ClipReward(wrappers.TransformObservation(rn, lambda o: o), -10, 10))
    assert top.unwrapped is env and not env._can_fuse()
    # ... never below
    for inner in (wrappers.ClipAction(make("Pendulum-v1", oracle_factory)), wrappers.RecordEpisodeStatistics(make("CartPole-v1", oracle_factory))):
        for cls in (per_env.NormalizeObservation, per_env.NormalizeReward):
            with pytest.raises(error.Error, match="directly over"):
                cls(inner)
    # RepeatAction / StickyAction are sub-environment wrappers too: the normalisations go over them
    env3 = make("CartPole-v1", oracle_factory)
    monkeypatch.setattr(env3._engine.lib, "set_step_wrappers", True, raising=False)
    monkeypatch.setattr(env3._engine, "set_step_wrappers", lambda *a: None)
    w = per_env.NormalizeReward(per_env.NormalizeObservation(wrappers.StickyAction(wrappers.RepeatAction(env3, 4), 0.25)))
    assert w._base is env3
    for e in (env, env2, env3):
        e.close()


def test_capture_steps_and_same_step_rollouts_are_refused(oracle_factory, device_engine):
    env = make("CartPole-v1", oracle_factory, autoreset_mode=AutoresetMode.SAME_STEP, output="torch")
    w = per_env.NormalizeReward(per_env.NormalizeObservation(env))
    for x in (w, w.env):
        with pytest.raises(error.Error, match="capture_steps"):
            x.capture_steps(steps=2, policy="random")
        with pytest.raises(error.Error, match="SAME_STEP"):
            x.rollout(4)
    env.close()


# -- 4. the fixtures --------------------------------------------------------------------------------------------------------------------------------
def test_generator_regenerates_its_files_bit_for_bit(tmp_path):
    if not os.path.isdir(os.path.join(REFERENCE, "gymnasium")):
        pytest.skip("the reference tree is not on this machine: the fixtures were recorded where it is")
    script = os.path.join(GOLDEN, "make_golden_per_env_normalize.py")
    env = dict(os.environ, GYM_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, script, str(tmp_path)], check=True, cwd=ROOT, env=env, capture_output=True)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz")) == FILES
    for name in FILES:
        new, old = np.load(tmp_path / name), np.load(os.path.join(GOLDEN, name))
        assert new.files == old.files, name
        for k in new.files:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)
