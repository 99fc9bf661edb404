"""CPU side of HipVectorEnv.lookahead(): every refusal and validation error, the checker backend being told apart by the missing entry point, the
ctypes mirror of mi_lookahead_io against the header, the wrappers' refusal, and the shared helper (tests/lookahead_cases.py) against a hand-written
scalar loop.  What the kernel computes is a GPU matter (tests/test_gpu_lookahead.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import error
from conftest import ROOT
from lookahead_cases import (CLASSIC_IDS, KINDS_AND_MODES_WITHOUT, METHODS, cartpole_near_thresholds, check_struct_layout, expected_lookahead, good_actions, make,
                             random_actions)


# -- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_a_host_symbol_of_abi_10():
    assert "lookahead" in _native.HOST_SYMBOLS and "lookahead" not in _native.SYMBOLS and _native.ABI_VERSION == 10
    from gymnasium_amd.csrc import build as B

    assert "lookahead.hip" in B.SOURCES and B.TU_FLAGS["lookahead.hip"] == B.TU_FLAGS["classic.hip"]
    lib = _native.load_library()
    assert hasattr(lib, "lookahead") and hasattr(lib.dll, "mi_lookahead")


def test_struct_layout_matches_the_header(tmp_path):
    ct = _native.MiLookaheadIO
    assert ctypes.sizeof(ct) == 2 * 4 + 6 * 8 + 2 * 4 + 8
    check_struct_layout(ct, "mi_lookahead_io", os.path.join(ROOT, "include", "mi355env.h"), tmp_path)


# -- refusals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_checker_backend_needs_the_device_engine(oracle_factory, env_id):
    env = make(env_id, oracle_factory)
    env.reset(seed=0)
    before = env.get_state()
    with pytest.raises(error.Error, match=r"needs the device engine \(mi_lookahead\)"):
        env.lookahead(good_actions(env))
    with pytest.raises(error.Error, match=r"needs the device engine \(mi_lookahead\)"):
        env.lookahead(good_actions(env), 0.9, final_obs=True)
    assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state()))
    env.close()


@pytest.mark.parametrize("method", sorted(METHODS))
def test_numpy_output_is_refused(oracle_factory, method):
    good, call, _ = METHODS[method]
    env = make("CartPole-v1", oracle_factory, output="numpy")
    env.reset(seed=0)
    with pytest.raises(error.Error, match="output='torch'"):
        call(env, good(env).numpy())
    env.close()


@pytest.mark.parametrize("env_id,kw,why", KINDS_AND_MODES_WITHOUT)
def test_kinds_and_modes_without_lookahead(oracle_factory, env_id, kw, why):
    env = make(env_id, oracle_factory, **kw)
    env.reset(seed=0)
    with pytest.raises(error.Error, match=why):
        env.lookahead(torch.zeros((2, 2, 4), dtype=torch.int64))
    env.close()


# (the refusals below are the same for both methods but for the name: one test over both, tests/test_lookahead_policy_host.py has none of them)
@pytest.mark.parametrize("method", sorted(METHODS))
def test_envs_that_step_through_wrappers_are_refused(oracle_factory, monkeypatch, method):
    good, call, nothing_else = METHODS[method]
    env = make("CartPole-v1", oracle_factory)
    env.reset(seed=0)
    x = good(env)
    monkeypatch.setattr(env, "_step_wrappers", (2, 0.0, 0), raising=False)
    with pytest.raises(error.Error, match="set_step_wrappers"):
        call(env, x)
    monkeypatch.setattr(env, "_step_wrappers", (0, 0.25, 3), raising=False)
    with pytest.raises(error.Error, match="set_step_wrappers"):
        call(env, x)
    monkeypatch.setattr(env, "_step_wrappers", (0, 0.0, 0), raising=False)
    monkeypatch.setattr(env, "_max_and_skip", 4, raising=False)
    with pytest.raises(error.Error, match="set_max_and_skip"):
        call(env, x)
    monkeypatch.setattr(env, "_max_and_skip", 0, raising=False)
    env._fusion_state()["chain"].append(("obs", object()))  # what a fused NormalizeObservation registers (HipVectorEnv._fuse)
    with pytest.raises(error.Error, match="fused"):
        call(env, x)
    env._fusion_state()["chain"].clear()
    with pytest.raises(error.Error, match=nothing_else):  # nothing else stands in the way
        call(env, x)
    env.close()


@pytest.mark.parametrize("method", sorted(METHODS))
def test_before_reset_and_after_close(oracle_factory, method):
    good, call, _ = METHODS[method]
    env = make("CartPole-v1", oracle_factory)
    x = good(env)
    with pytest.raises(AssertionError, match="reset"):
        call(env, x)
    env.reset(seed=0)
    env.close()
    with pytest.raises(error.ClosedEnvironmentError):
        call(env, x)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_wrappers_refuse_and_name_the_unwrapped_call(oracle_factory, method):
    good, call, _ = METHODS[method]
    env = make("CartPole-v1", oracle_factory)
    env.reset(seed=0)
    x = good(env)
    more = {"hidden": 0} if method == "lookahead_policy" else {}
    for w in (wrappers.RecordEpisodeStatistics(env), wrappers.ClipReward(env, -1.0, 1.0), wrappers.TransformReward(env, lambda r: r),
              wrappers.NumpyToTorch(wrappers.VectorWrapper(env))):
        with pytest.raises(error.Error, match=rf"env\.unwrapped\.{method}\b"):
            call(w, x)
        with pytest.raises(error.Error, match=rf"env\.unwrapped\.{method}\b"):
            call(w, x, 0.9, final_obs=True, **more)
    env.close()


# -- validation: before any launch, so the checker backend sees it too ------------------------------------------------------------------------------
def test_discrete_actions_are_validated(oracle_factory):
    env = make("CartPole-v1", oracle_factory)
    env.reset(seed=0)
    for bad in (torch.zeros((3, 2, 4), dtype=torch.int32), torch.zeros((3, 2, 4), dtype=torch.float32), np.zeros((3, 2, 4), dtype=np.float64)):
        with pytest.raises(TypeError, match="int64"):
            env.lookahead(bad)
    with pytest.raises(TypeError, match="tensor"):
        env.lookahead([[[0, 1, 0, 1]]])
    for shape in ((3, 2), (3, 2, 5), (3, 2, 4, 1), (3, 8)):
        with pytest.raises(ValueError, match="shape"):
            env.lookahead(torch.zeros(shape, dtype=torch.int64))
    for shape in ((0, 2, 4), (3, 0, 4)):
        with pytest.raises(ValueError, match="H >= 1 and K >= 1"):
            env.lookahead(torch.zeros(shape, dtype=torch.int64))
    env.close()


@pytest.mark.parametrize("method", sorted(METHODS))
def test_candidates_times_envs_must_fit_31_bits(oracle_factory, method):
    good, call, _ = METHODS[method]
    env = make("CartPole-v1", oracle_factory, n=4)
    env.reset(seed=0)
    x = good(env, K=1)  # expanded along K: a view, no memory behind the 2^31 lanes
    with pytest.raises(ValueError, match=r"K \* N < 2\*\*31"):
        call(env, x.expand(-1, 2 ** 29, -1) if method == "lookahead" else x.expand(2 ** 29, -1))
    env.close()


@pytest.mark.parametrize("env_id", ["Pendulum-v1", "MountainCarContinuous-v0"])
def test_box_actions_are_validated(oracle_factory, env_id):
    env = make(env_id, oracle_factory)
    env.reset(seed=0)
    for bad in (torch.zeros((3, 2, 4, 1), dtype=torch.int64), torch.zeros((3, 2, 4, 1), dtype=torch.float16)):
        with pytest.raises(TypeError, match="float32 or float64"):
            env.lookahead(bad)
    for shape in ((3, 2, 4, 2), (3, 2, 5, 1), (3, 2, 5), (3, 4), (3, 2, 4, 1, 1)):
        with pytest.raises(ValueError, match="shape"):
            env.lookahead(torch.zeros(shape, dtype=torch.float32))
    for ok in (torch.zeros((3, 2, 4, 1)), torch.zeros((3, 2, 4)), torch.zeros((3, 2, 4), dtype=torch.float64)):  # (a trailing act_dim of 1 may be omitted)
        with pytest.raises(error.Error, match="mi_lookahead"):
            env.lookahead(ok)
    env.close()


@pytest.mark.parametrize("method", sorted(METHODS))
def test_gamma_is_validated(oracle_factory, method):
    good, call, needs_engine = METHODS[method]
    env = make("CartPole-v1", oracle_factory)
    env.reset(seed=0)
    x = good(env)
    for bad in (-0.01, 1.0000001, float("nan"), float("inf"), 2):
        with pytest.raises(ValueError, match="gamma"):
            call(env, x, bad)
    for bad in ("0.9", None, True, [0.9]):
        with pytest.raises(TypeError, match="gamma"):
            call(env, x, bad)
    for ok in (0, 1, 0.0, 1.0, np.float64(0.5), np.float32(0.25)):
        with pytest.raises(error.Error, match=needs_engine):
            call(env, x, ok)
    env.close()


# -- the helper itself ----------------------------------------------------------------------------------------------------------------------------
def test_helper_equals_a_scalar_loop_on_cartpole(oracle_factory):
    """expected_lookahead() for N = 3, K = 2, H = 5 against one single-sub-environment env per candidate, stepped until it is done."""
    N, K, H, gamma, cap = 3, 2, 5, 0.9, 12
    state = cartpole_near_thresholds(N, 3)
    elapsed = np.array([0, 9, 10], dtype=np.int32)  # (row 1 is truncated by its third step, row 2 by its second)
    flags = np.zeros(N, dtype=np.uint8)
    actions = random_actions("CartPole-v1", H, K, N, 7)

    def make_env(n):
        return gymnasium_amd.make_vec("CartPole-v1", num_envs=n, max_episode_steps=cap, _engine_factory=oracle_factory)

    one = make_env(1)
    one.reset(seed=0)
    one.set_state(state[:1], elapsed[:1], flags[:1])
    present = np.stack([state[i].astype(np.float32) for i in range(N)])  # cartpole.py:214: the observation is the state in float32
    got = expected_lookahead(make_env, state, elapsed, flags, actions, gamma, present_obs=present)
    ended = 0
    for k in range(K):
        for i in range(N):
            one.set_state(state[i:i + 1], elapsed[i:i + 1], flags[i:i + 1])
            G, disc, steps, te, tr, obs = 0.0, 1.0, 0, False, False, None
            for t in range(H):
                o, r, te_, tr_, _ = one.step(actions[t, k, i:i + 1])
                G = G + disc * float(r[0])
                disc = disc * gamma
                steps, te, tr, obs = steps + 1, bool(te_[0]), bool(tr_[0]), o[0].copy()
                if te or tr:
                    break
            ended += te or tr
            assert got["returns"][k, i] == G and got["steps"][k, i] == steps, (k, i)
            assert got["terminated"][k, i] == te and got["truncated"][k, i] == tr, (k, i)
            assert np.array_equal(got["final_obs"][k, i], obs), (k, i)
    assert 0 < ended < K * N and got["truncated"].any()  # (both kinds of candidate were in the comparison)
    assert got["returns"].dtype == np.float64 and got["steps"].dtype == np.int32 and got["final_obs"].dtype == np.float32
    one.close()


def test_helper_leaves_lanes_that_wait_for_a_reset_alone(oracle_factory):
    N, K, H = 3, 2, 4
    state = cartpole_near_thresholds(N, 5) * 0.1  # (far from the thresholds: nobody ends inside the horizon)
    flags = np.array([0, 1, 0], dtype=np.uint8)
    present = state.astype(np.float32)
    actions = random_actions("CartPole-v1", H, K, N, 1)
    make_env = lambda n: gymnasium_amd.make_vec("CartPole-v1", num_envs=n, _engine_factory=oracle_factory)
    got = expected_lookahead(make_env, state, np.zeros(N, np.int32), flags, actions, 1.0, present_obs=present)
    assert (got["steps"][:, 1] == 0).all() and (got["returns"][:, 1] == 0).all() and not got["terminated"][:, 1].any() and not got["truncated"][:, 1].any()
    assert np.array_equal(got["final_obs"][:, 1], np.stack([present[1]] * K))
    assert (got["steps"][:, [0, 2]] == H).all() and (got["returns"][:, [0, 2]] == H).all()
    with pytest.raises(ValueError, match="present_obs"):
        expected_lookahead(make_env, state, np.zeros(N, np.int32), flags, actions, 1.0)
