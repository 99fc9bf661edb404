"""CPU side of HipVectorEnv.lookahead_policy(): every refusal and validation error, the checker backend being told apart by the missing entry point, the
ctypes mirror of mi_lookahead_policy_io against the header, policy_param_layout, and the shared helper
(tests/lookahead_policy_cases.py) against a hand-written scalar loop and a float64 evaluation.  What the kernel computes is a GPU matter
(tests/test_gpu_lookahead_policy.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gymnasium_amd
from gymnasium_amd import _native
from gymnasium_amd.gym_api import error
from conftest import ROOT
from lookahead_cases import CLASSIC_IDS, DISCRETE_ACTIONS, KINDS_AND_MODES_WITHOUT, cartpole_near_thresholds, check_struct_layout, good_params, make
from lookahead_policy_cases import (OBS_DIM, expected_lookahead_policy, n_outputs, param_size, policy_actions, policy_logits, random_params,
                                    split_params)

NEEDS_ENGINE = r"needs the device engine \(mi_lookahead_policy\)"


# -- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_a_host_symbol_of_abi_10():
    assert "lookahead_policy" in _native.HOST_SYMBOLS and "lookahead_policy" not in _native.SYMBOLS and _native.ABI_VERSION == 10
    from gymnasium_amd.csrc import build as B

    assert "lookahead_policy.hip" in B.SOURCES and B.TU_FLAGS["lookahead_policy.hip"] == B.TU_FLAGS["lookahead.hip"] == B.MAXILP
    assert "-ffp-contract=off" in B.FLAGS and not any("denormal" in f or "flush" in f or "fast-math" in f for f in B.FLAGS)  # the arithmetic contract
    lib = _native.load_library()
    assert hasattr(lib, "lookahead_policy") and hasattr(lib.dll, "mi_lookahead_policy")


def test_struct_layout_matches_the_header(tmp_path):
    ct = _native.MiLookaheadPolicyIO
    assert [f for f, _ in ct._fields_] == ["struct_size", "params", "returns", "steps", "terminated", "truncated", "final_obs", "horizon", "candidates",
                                           "hidden", "gamma"]
    assert ctypes.sizeof(ct) == 8 + 6 * 8 + 3 * 4 + 4 + 8
    check_struct_layout(ct, "mi_lookahead_policy_io", os.path.join(ROOT, "include", "mi355env.h"), tmp_path)


# -- policy_param_layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [0, 1, 64])
@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_param_layout(oracle_factory, env_id, hidden):
    env = make(env_id, oracle_factory, output="numpy")  # (a question about the spaces: any output, before reset)
    lay = env.policy_param_layout(hidden)
    obs, A = OBS_DIM[env_id], n_outputs(env_id)
    assert lay["size"] == param_size(env_id, hidden) == (A * (obs + 1) if hidden == 0 else hidden * (obs + 1) + A * (hidden + 1))
    names = ["W", "b"] if hidden == 0 else ["W1", "b1", "W2", "b2"]
    assert list(lay) == names + ["size"]
    shapes = {"W": (A, obs), "b": (A,), "W1": (hidden, obs), "b1": (hidden,), "W2": (A, hidden), "b2": (A,)}
    at = 0
    for name in names:  # contiguous, in the header's order
        sl, shape = lay[name]
        assert shape == shapes[name] and (sl.start, sl.stop, sl.step) == (at, at + int(np.prod(shape)), None), name
        at = sl.stop
    assert at == lay["size"]
    # ... and they are the parts the helper reads
    row = np.arange(lay["size"], dtype=np.float32)[None]
    for name, part in zip(names, split_params(env_id, row, hidden)):
        sl, shape = lay[name]
        assert np.array_equal(row[0, sl].reshape(shape), part[0]), name
    env.close()


def test_param_layout_refusals(oracle_factory):
    env = make("CartPole-v1", oracle_factory)
    for bad in (-1, 257):
        with pytest.raises(ValueError, match=r"hidden must be in \[0, 256\]"):
            env.policy_param_layout(bad)
    for bad in (1.0, "1", None, True):
        with pytest.raises(TypeError, match="hidden"):
            env.policy_param_layout(bad)
    assert env.policy_param_layout(256)["size"] == 256 * 5 + 2 * 257 and env.policy_param_layout(np.int64(3))["size"] == 3 * 5 + 2 * 4
    env.close()
    other = make("HalfCheetah-v5", oracle_factory)
    with pytest.raises(error.Error, match="lookahead_policy exists for CartPole-v1"):
        other.policy_param_layout(0)
    other.close()


# -- refusals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_checker_backend_needs_the_device_engine(oracle_factory, env_id):
    env = make(env_id, oracle_factory)
    env.reset(seed=0)
    before = env.get_state()
    with pytest.raises(error.Error, match=NEEDS_ENGINE):
        env.lookahead_policy(good_params(env), 3)
    with pytest.raises(error.Error, match=NEEDS_ENGINE):
        env.lookahead_policy(good_params(env, 3, 7), 5, 0.9, hidden=7, final_obs=True)
    assert all(np.array_equal(x, y) for x, y in zip(before, env.get_state()))
    env.close()


@pytest.mark.parametrize("env_id,kw,why", KINDS_AND_MODES_WITHOUT)
def test_kinds_and_modes_without_lookahead(oracle_factory, env_id, kw, why):
    env = make(env_id, oracle_factory, **kw)
    env.reset(seed=0)
    with pytest.raises(error.Error, match=why):
        env.lookahead_policy(torch.zeros((2, 10), dtype=torch.float32), 3)
    env.close()


# -- validation: before any launch, so the checker backend sees it too ------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1"])
def test_params_are_validated(oracle_factory, env_id):
    env = make(env_id, oracle_factory)
    env.reset(seed=0)
    P0, P7 = param_size(env_id, 0), param_size(env_id, 7)
    for bad in (torch.zeros((2, P0), dtype=torch.float64), torch.zeros((2, P0), dtype=torch.float16), torch.zeros((2, P0), dtype=torch.int64),
                np.zeros((2, P0), dtype=np.float64), np.zeros((2, P0), dtype=np.int32)):
        with pytest.raises(TypeError, match="float32"):  # (nothing is cast)
            env.lookahead_policy(bad, 3)
    for bad in ([[0.0] * P0], None, 1.0):
        with pytest.raises(TypeError, match="tensor"):
            env.lookahead_policy(bad, 3)
    for shape in ((P0,), (2, P0 + 1), (2, P0 - 1), (2, P7), (2, 1, P0), (P0, 2)):
        with pytest.raises(ValueError, match=rf"P = {P0} for hidden = 0"):
            env.lookahead_policy(torch.zeros(shape, dtype=torch.float32), 3)
    with pytest.raises(ValueError, match=rf"P = {P7} for hidden = 7"):
        env.lookahead_policy(torch.zeros((2, P0), dtype=torch.float32), 3, hidden=7)
    with pytest.raises(ValueError, match="K >= 1"):
        env.lookahead_policy(torch.zeros((0, P0), dtype=torch.float32), 3)
    for ok in (torch.zeros((2, P0)), np.zeros((3, P0), dtype=np.float32)):
        with pytest.raises(error.Error, match=NEEDS_ENGINE):
            env.lookahead_policy(ok, 3)
    with pytest.raises(error.Error, match=NEEDS_ENGINE):
        env.lookahead_policy(torch.zeros((2, P7)), 3, hidden=7)
    env.close()


def test_hidden_and_horizon_are_validated(oracle_factory):
    env = make("CartPole-v1", oracle_factory)
    env.reset(seed=0)
    p = good_params(env)
    for bad in (-1, 257, 1000):
        with pytest.raises(ValueError, match=r"hidden must be in \[0, 256\]"):
            env.lookahead_policy(p, 3, hidden=bad)
    for bad in (1.0, "1", None, True):
        with pytest.raises(TypeError, match="hidden"):
            env.lookahead_policy(p, 3, hidden=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="horizon must be >= 1"):
            env.lookahead_policy(p, bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError, match="horizon"):
            env.lookahead_policy(p, bad)
    for hidden in (1, 256):
        with pytest.raises(error.Error, match=NEEDS_ENGINE):
            env.lookahead_policy(good_params(env, 2, hidden), np.int64(1), hidden=hidden)
    env.close()


# -- the helper itself ----------------------------------------------------------------------------------------------------------------------------
def test_helper_equals_a_scalar_loop_on_cartpole(oracle_factory):
    """expected_lookahead_policy() for N = 3, K = 2, H = 5 and a linear policy against one single-sub-environment env per candidate, stepped until it
    is done, with the action written out in scalar float32 arithmetic."""
    N, K, H, gamma, cap = 3, 2, 5, 0.9, 12
    state = cartpole_near_thresholds(N, 3)
    elapsed = np.array([0, 9, 10], dtype=np.int32)  # (row 1 is truncated by its third step, row 2 by its second)
    flags = np.zeros(N, dtype=np.uint8)
    params = random_params("CartPole-v1", 0, K, 7)
    W, b = params[:, :8].reshape(K, 2, 4), params[:, 8:]

    def make_env(n):
        return gymnasium_amd.make_vec("CartPole-v1", num_envs=n, max_episode_steps=cap, _engine_factory=oracle_factory)

    one = make_env(1)
    one.reset(seed=0)
    present = state.astype(np.float32)  # cartpole.py:214: the observation is the state in float32
    got = expected_lookahead_policy(make_env, state, elapsed, flags, present, params, 0, H, gamma)
    ended, seen = 0, set()
    for k in range(K):
        for i in range(N):
            one.set_state(state[i:i + 1], elapsed[i:i + 1], flags[i:i + 1])
            G, disc, steps, te, tr, obs = 0.0, 1.0, 0, False, False, present[i]
            for t in range(H):
                y = [b[k, o] for o in range(2)]
                for o in range(2):
                    for j in range(4):
                        y[o] = np.float32(y[o] + np.float32(W[k, o, j] * obs[j]))
                a = 1 if y[1] > y[0] else 0
                seen.add(a)
                assert got["actions"][t, k, i] == a and got["took"][t, k, i]
                o_, r, te_, tr_, _ = one.step(np.array([a], dtype=np.int64))
                G = G + disc * float(r[0])
                disc = disc * gamma
                steps, te, tr, obs = steps + 1, bool(te_[0]), bool(tr_[0]), o_[0].copy()
                if te or tr:
                    break
            ended += te or tr
            assert not got["took"][steps:, k, i].any()
            assert got["returns"][k, i] == G and got["steps"][k, i] == steps, (k, i)
            assert got["terminated"][k, i] == te and got["truncated"][k, i] == tr, (k, i)
            assert np.array_equal(got["final_obs"][k, i], obs), (k, i)
    assert 0 < ended < K * N and got["truncated"].any() and seen == {0, 1}  # (both kinds of candidate and both actions were in the comparison)
    assert got["returns"].dtype == np.float64 and got["steps"].dtype == np.int32 and got["final_obs"].dtype == np.float32
    one.close()


def test_helper_leaves_lanes_that_wait_for_a_reset_alone(oracle_factory):
    N, K, H = 3, 2, 4
    state = cartpole_near_thresholds(N, 5) * 0.1  # (far from the thresholds: nobody ends inside the horizon)
    flags = np.array([0, 1, 0], dtype=np.uint8)
    present = state.astype(np.float32)
    make_env = lambda n: gymnasium_amd.make_vec("CartPole-v1", num_envs=n, _engine_factory=oracle_factory)
    got = expected_lookahead_policy(make_env, state, np.zeros(N, np.int32), flags, present, random_params("CartPole-v1", 3, K, 1), 3, H, 1.0)
    assert (got["steps"][:, 1] == 0).all() and (got["returns"][:, 1] == 0).all() and not got["terminated"][:, 1].any() and not got["truncated"][:, 1].any()
    assert np.array_equal(got["final_obs"][:, 1], np.stack([present[1]] * K)) and not got["took"][:, :, 1].any()
    assert (got["steps"][:, [0, 2]] == H).all() and (got["returns"][:, [0, 2]] == H).all()


@pytest.mark.parametrize("hidden", [0, 1, 7, 64])
@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_helper_network_against_float64(env_id, hidden):
    """The float32 loops against the same network in float64 matrix form (guards the layout: a transposed W2, a misplaced bias).  The bound: every
    float32 operation adds a relative 2^-24 of its result, and a logit is a sum of at most (hidden or 1) * (OBS + 2) + 1 such results whose magnitudes
    are bounded by the same sum taken over absolute values -- so |y32 - y64| <= ops * 2^-24 * S_abs with ops the depth of the longest chain, doubled
    for the rounding of the intermediate z's feeding the second layer."""
    K, n = 5, 6
    rng = np.random.default_rng(11)
    obs = rng.standard_normal((K * n, OBS_DIM[env_id])).astype(np.float32)
    params = random_params(env_id, hidden, K, 13)
    y = policy_logits(env_id, params, hidden, obs)
    parts = [np.repeat(p.astype(np.float64), n, axis=0) for p in split_params(env_id, params, hidden)]
    x = obs.astype(np.float64)
    if hidden == 0:
        W, b = parts
        want = b + np.einsum("laj,lj->la", W, x)
        mag = np.abs(b) + np.einsum("laj,lj->la", np.abs(W), np.abs(x))
        ops = OBS_DIM[env_id] + 1
    else:
        W1, b1, W2, b2 = parts
        z = b1 + np.einsum("luj,lj->lu", W1, x)
        zmag = np.abs(b1) + np.einsum("luj,lj->lu", np.abs(W1), np.abs(x))
        want = b2 + np.einsum("lau,lu->la", W2, np.maximum(z, 0.0))
        mag = np.abs(b2) + np.einsum("lau,lu->la", np.abs(W2), zmag)
        ops = 2 * (OBS_DIM[env_id] + 1 + hidden + 1)
    assert y.dtype == np.float32 and y.shape == want.shape == (K * n, n_outputs(env_id))
    assert (np.abs(y - want) <= ops * 2.0 ** -24 * mag).all(), np.abs(y - want).max()
    assert (np.abs(y - want) > 0).any()  # (float32 it is)
    a = policy_actions(env_id, params, hidden, obs)
    if env_id in DISCRETE_ACTIONS:
        clear = np.sort(want, axis=1)[:, -1] - np.sort(want, axis=1)[:, -2] > 2 * ops * 2.0 ** -24 * mag.max(axis=1)
        assert clear.mean() > 0.8 and np.array_equal(a[clear], want.argmax(axis=1)[clear]) and a.dtype == np.int64
    else:
        assert a.dtype == np.float32 and a.shape == (K * n, 1) and np.array_equal(a[:, 0], y[:, 0])


def test_helper_scan_is_strict_and_no_comparison_with_a_nan_holds():
    """Equal logits: the first wins.  A comparison with a NaN is false: a NaN y[o], o >= 1, is never chosen and a NaN y[0] is never displaced -- NOT
    np.argmax, which returns the first NaN."""
    p = np.zeros((4, 21), np.float32)  # Acrobot, hidden = 0: W [3, 6] then b [3]
    p[0, 18:] = [1.0, 1.0, 0.5]          # tie of 0 and 1
    p[1, 18:] = [0.5, 2.0, 2.0]          # tie of 1 and 2
    p[2, 18:] = [np.nan, 1.0, 3.0]       # y[0] NaN: nothing is > NaN, so `best` stays 0
    p[3, 18:] = [1.0, np.nan, 0.5]
    obs = np.ones((4, 6), np.float32)
    y = policy_logits("Acrobot-v1", p, 0, obs)
    a = policy_actions("Acrobot-v1", p, 0, obs)
    assert a.tolist() == [0, 1, 0, 0]
    assert np.argmax(y, axis=1).tolist() == [0, 1, 0, 1]  # (np.argmax lets the NaN of row 3 win)
