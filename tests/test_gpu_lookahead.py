"""-m gpu: HipVectorEnv.lookahead() (mi_lookahead, gymnasium_amd/csrc/lookahead.hip) against its definition by composition
(tests/lookahead_cases.py expected_lookahead): K * N sub-environments of the ORACLE put into the tiled state, stepped H times and reduced in NumPy --
every output array_equal, the float64 returns included.  Where the oracle has no counterpart (per-sub-environment attributes) the same composition
runs on the device engine's step(), which the parity suites pin to the oracle."""
import functools

import numpy as np
import pytest
import torch

from lookahead_cases import (CLASSIC_IDS, KEYS, NEEDS_RESET, acrobot_near_height, assert_equal, cartpole_near_thresholds, composed_on_device, device_env,
                             expected_lookahead, host, mountaincar_near_goal, oracle_env, random_actions)

pytestmark = pytest.mark.gpu

SHAPES = [(130, 3, 9, 1.0), (1, 1, 1, 1.0), (64, 1, 2, 1.0), (77, 5, 9, 0.97)]  # (N, K, H, gamma): 390 lanes are neither a wavefront nor a workgroup multiple


def reached_state(env_id, N, seed, warm, **kw):
    """The oracle's state after reset(seed) and `warm` random steps (NEXT_STEP), with no row waiting for its reset (the flag is cleared: a row that
    finished in the last step goes on from its final state -- rows that wait are test_rows_that_wait_for_their_reset's subject)."""
    env = oracle_env(env_id, **kw)(N)
    env.reset(seed=seed)
    env.action_space.seed(seed)
    for _ in range(warm):
        env.step(env.action_space.sample())
    state, elapsed, flags = env.get_state()
    env.close()
    return state, elapsed, flags & ~np.uint8(NEEDS_RESET)


@functools.lru_cache(maxsize=None)
def plain_case(env_id, N, K, H, gamma):
    """From reset: what a planner starts from."""
    state, elapsed, flags = reached_state(env_id, N, 11, 3)
    actions = random_actions(env_id, H, K, N, 5)
    return state, elapsed, flags, actions, expected_lookahead(oracle_env(env_id), state, elapsed, flags, actions, gamma, present_obs=None)


@pytest.mark.parametrize("N,K,H,gamma", SHAPES)
@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_equals_the_composition_over_the_oracle(env_id, N, K, H, gamma):
    state, elapsed, flags, actions, want = plain_case(env_id, N, K, H, gamma)
    gpu = device_env(env_id, N)
    gpu.reset(seed=11)
    gpu.set_state(state, elapsed, flags)
    got = gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True)
    assert_equal(host(got), want, env_id)
    short = gpu.lookahead(torch.from_numpy(actions).cuda(), gamma)
    assert set(short) == set(KEYS) - {"final_obs"} and all(torch.equal(short[k], got[k]) for k in short)
    gpu.close()


@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_same_step_autoreset_mode(env_id):
    """The autoreset mode decides what step() does after an episode's end, which a candidate never reaches: SAME_STEP scores like the others."""
    state, elapsed, flags, actions, want = plain_case(env_id, 77, 5, 9, 0.97)
    gpu = device_env(env_id, 77, autoreset_mode="SameStep")
    gpu.reset(seed=11)
    gpu.set_state(state, elapsed, flags)
    assert_equal(host(gpu.lookahead(torch.from_numpy(actions).cuda(), 0.97, final_obs=True)), want, env_id)
    gpu.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("env_id", ["Pendulum-v1", "MountainCarContinuous-v0"])
def test_float32_and_float64_action_rows(env_id, dtype):
    """float64 rows go in un-rounded (as in step() and rollout()); a trailing act_dim of 1 may be omitted; a host or strided tensor is converted."""
    N, K, H, gamma = 130, 3, 9, 0.97
    state, elapsed, flags = reached_state(env_id, N, 2, 4)
    actions = random_actions(env_id, H, K, N, 9, dtype=dtype)
    if dtype is np.float64:
        assert (actions.astype(np.float32) != actions).any()
    want = expected_lookahead(oracle_env(env_id), state, elapsed, flags, actions, gamma)
    gpu = device_env(env_id, N)
    gpu.reset(seed=2)
    gpu.set_state(state, elapsed, flags)
    a = torch.from_numpy(actions)
    assert_equal(host(gpu.lookahead(a.cuda(), gamma, final_obs=True)), want, (env_id, "device rows"))
    assert_equal(host(gpu.lookahead(a[..., 0].cuda(), gamma, final_obs=True)), want, (env_id, "act_dim omitted"))
    assert_equal(host(gpu.lookahead(a, gamma, final_obs=True)), want, (env_id, "host tensor"))
    strided = torch.empty((H, K, N, 2), dtype=a.dtype).cuda()
    strided[..., :1] = a.cuda()
    assert not strided[..., :1].is_contiguous()
    assert_equal(host(gpu.lookahead(strided[..., :1], gamma, final_obs=True)), want, (env_id, "not contiguous"))
    gpu.close()


@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_truncation_falls_at_different_steps(env_id):
    """max_episode_steps = 7 after 0 .. 6 elapsed steps per row: candidates are truncated by their 7th .. 1st step, H = 9 covers all of them."""
    N, K, H, gamma, cap = 130, 3, 9, 0.97, 7
    state, _, flags = reached_state(env_id, N, 4, 2)
    elapsed = (np.arange(N) % cap).astype(np.int32)
    actions = random_actions(env_id, H, K, N, 13)
    want = expected_lookahead(oracle_env(env_id, max_episode_steps=cap), state, elapsed, flags, actions, gamma)
    assert want["truncated"].mean() > 0.5 and set(np.unique(want["steps"][want["truncated"]])) == set(range(1, cap + 1))
    gpu = device_env(env_id, N, max_episode_steps=cap)
    gpu.reset(seed=4)
    gpu.set_state(state, elapsed, flags)
    assert_equal(host(gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True)), want, env_id)
    gpu.close()


TERMINATION_CASES = {"CartPole-v1": (cartpole_near_thresholds, 1), "MountainCar-v0": (functools.partial(mountaincar_near_goal, goal=0.5), 1),
                     "MountainCarContinuous-v0": (functools.partial(mountaincar_near_goal, goal=0.45), 1), "Acrobot-v1": (acrobot_near_height, 1)}


@pytest.mark.parametrize("env_id", sorted(TERMINATION_CASES))
def test_termination_inside_the_horizon(env_id):
    """States placed near where the id's episodes end, under a cap of 40 steps that some rows are about to reach: at least a quarter of the candidates
    end inside the horizon and at least a quarter do not (on the oracle's result), and both kinds of end occur."""
    N, K, H, gamma, cap = 130, 3, 9, 0.97, 40
    states, seed = TERMINATION_CASES[env_id]
    state = states(N, seed)
    elapsed = np.where(np.arange(N) % 5 == 0, cap - 1 - np.arange(N) % 7, np.arange(N) % 11).astype(np.int32)
    flags = np.zeros(N, np.uint8)
    actions = random_actions(env_id, H, K, N, 21)
    want = expected_lookahead(oracle_env(env_id, max_episode_steps=cap), state, elapsed, flags, actions, gamma)
    ended = want["terminated"] | want["truncated"]
    assert 0.25 <= ended.mean() <= 0.75, ended.mean()
    assert want["terminated"].mean() >= 0.1 and want["truncated"].any() and (want["steps"][ended] < H).any()
    gpu = device_env(env_id, N, max_episode_steps=cap)
    gpu.reset(seed=0)
    gpu.set_state(state, elapsed, flags)
    assert_equal(host(gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True)), want, env_id)
    gpu.close()


@pytest.mark.parametrize("mode", ["NextStep", "Disabled"])
def test_rows_that_wait_for_their_reset(mode):
    """A row whose episode ended in the last step() waits for its reset (NEXT_STEP: the next step resets it; DISABLED: the caller must): zeros and its
    present observation -- the one that step() returned.  The other rows are scored as usual."""
    N, K, H, gamma, cap = 130, 3, 9, 0.97, 7
    gpu = device_env("CartPole-v1", N, max_episode_steps=cap, autoreset_mode=mode)
    gpu.reset(seed=3)
    gpu.set_state(cartpole_near_thresholds(N, 8), (np.arange(N) % cap).astype(np.int32), np.zeros(N, np.uint8))
    present = gpu.step(torch.from_numpy(random_actions("CartPole-v1", 1, 1, N, 2)[0, 0]).cuda())[0].cpu().numpy()
    state, elapsed, flags = gpu.get_state()
    pending = (flags & NEEDS_RESET) != 0
    assert 0.1 < pending.mean() < 0.9
    actions = random_actions("CartPole-v1", H, K, N, 17)
    want = expected_lookahead(oracle_env("CartPole-v1", max_episode_steps=cap), state, elapsed, flags, actions, gamma, present_obs=present)
    got = host(gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True))
    assert_equal(got, want, mode)
    assert (got["steps"][:, pending] == 0).all() and (got["returns"][:, pending] == 0).all() and (got["steps"][:, ~pending] > 0).all()
    assert not got["terminated"][:, pending].any() and not got["truncated"][:, pending].any()
    assert np.array_equal(got["final_obs"][:, pending], np.broadcast_to(present[pending], (K,) + present[pending].shape))
    after = gpu.get_state()
    assert all(np.array_equal(x, y) for x, y in zip((state, elapsed, flags), after))
    gpu.synchronize()  # (DISABLED: looking ahead from a finished row is no step of it -- no error word)
    gpu.close()


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1", "Acrobot-v1"])
def test_the_env_is_untouched(env_id):
    """State, generators, statistics and the action stream before and after; and whatever comes next equals a twin's that never looked ahead."""
    N, K, H = 130, 3, 9
    a, b = device_env(env_id, N, max_episode_steps=20), device_env(env_id, N, max_episode_steps=20)
    for env in (a, b):
        env.reset(seed=6)
        env.action_space.seed(6)
        env.rollout(5)
    before = a.get_state(), a.get_rng_state(), a.statistics()
    out = a.lookahead(torch.from_numpy(random_actions(env_id, H, K, N, 3)).cuda(), 0.9, final_obs=True)
    assert (out["steps"] > 0).any()
    after = a.get_state(), a.get_rng_state(), a.statistics()
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert np.array_equal(np.asarray(a.action_space.sample()), np.asarray(b.action_space.sample()))
    ra, rb = a.rollout(8), b.rollout(8)
    assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state())) and np.array_equal(a.get_rng_state(), b.get_rng_state())
    assert a.statistics() == b.statistics()
    a.close(), b.close()


@pytest.mark.parametrize("env_id,name,lo,hi", [("CartPole-v1", "length", 0.25, 1.0), ("Pendulum-v1", "g", 2.0, 12.0)])
def test_attributes_of_the_candidates_own_sub_environment(env_id, name, lo, hi):
    N, K, H, gamma = 77, 5, 9, 0.97
    values = np.random.default_rng(1).uniform(lo, hi, N).tolist()
    state, elapsed, flags = reached_state(env_id, N, 7, 2)
    actions = random_actions(env_id, H, K, N, 23)
    want = expected_lookahead(composed_on_device(env_id, {name: values}), state, elapsed, flags, actions, gamma)
    plain = expected_lookahead(oracle_env(env_id), state, elapsed, flags, actions, gamma)
    assert (want["final_obs"] != plain["final_obs"]).any(axis=-1).mean() > 0.5  # (the attribute matters to the result)
    gpu = device_env(env_id, N)
    gpu.reset(seed=7)
    gpu.set_attr(name, values)
    gpu.set_state(state, elapsed, flags)
    assert_equal(host(gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True)), want, (env_id, name))
    gpu.close()


def test_acrobot_torque_noise_comes_from_a_copy_of_the_generator():
    """Every candidate of sub-environment i draws what the env itself would draw next; the env's generator does not move."""
    N, K, H, gamma = 77, 5, 9, 0.97
    noise = np.where(np.arange(N) % 3 == 0, 0.0, np.random.default_rng(2).uniform(0.1, 0.5, N)).tolist()
    mass = np.random.default_rng(3).uniform(0.8, 1.2, N).tolist()
    gpu = device_env("Acrobot-v1", N)
    gpu.reset(seed=9)
    gpu.set_attr("torque_noise_max", noise), gpu.set_attr("LINK_MASS_2", mass)
    gpu.set_state(acrobot_near_height(N, 4), np.zeros(N, np.int32), np.zeros(N, np.uint8))
    gpu.action_space.seed(1)
    gpu.rollout(3)  # (generators moved by their own steps' draws, episodes in flight)
    state, elapsed, flags = gpu.get_state()
    words = gpu.get_rng_state()
    present = gpu._obs.cpu().numpy()
    actions = random_actions("Acrobot-v1", H, K, N, 29)
    make_env = composed_on_device("Acrobot-v1", {"torque_noise_max": noise, "LINK_MASS_2": mass}, words=words)
    want = expected_lookahead(make_env, state, elapsed, flags, actions, gamma, present_obs=present)
    got = host(gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True))
    assert_equal(got, want, "noise")
    quiet = expected_lookahead(composed_on_device("Acrobot-v1", {"torque_noise_max": [0.0] * N, "LINK_MASS_2": mass}, words=words), state, elapsed, flags,
                               actions, gamma, present_obs=present)
    assert (quiet["final_obs"] != want["final_obs"]).any()  # (the noise matters to the result)
    assert np.array_equal(gpu.get_rng_state(), words) and all(np.array_equal(x, y) for x, y in zip(gpu.get_state(), (state, elapsed, flags)))
    again = host(gpu.lookahead(torch.from_numpy(actions).cuda(), gamma, final_obs=True))
    assert_equal(again, got, "a second call draws the same noise")
    gpu.close()


def test_an_invalid_discrete_action_is_reported_at_synchronize():
    N, K, H = 130, 3, 9
    gpu = device_env("CartPole-v1", N)
    gpu.reset(seed=1)
    before = gpu.get_state()
    actions = torch.from_numpy(random_actions("CartPole-v1", H, K, N, 31)).cuda()
    actions[0, 2, 17] = 2
    gpu.lookahead(actions)  # enqueued; nothing raised yet
    with pytest.raises(Exception, match="action outside the action space"):
        gpu.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(before, gpu.get_state()))
    gpu.close()


def test_entry_points_refuse_with_their_exact_messages():
    """mi_lookahead and mi_lookahead_policy called through the binding, past HipVectorEnv's own validation: the checks the two entry points share
    (engine.hip) and those they keep, each with its status and its full text.  No call here launches a kernel."""
    from gymnasium_amd import _native

    INVALID, STATE = -1, -5  # MI_ERR_INVALID_ARGUMENT, MI_ERR_STATE (include/mi355env.h)

    def refused(call, code, text):
        with pytest.raises(_native.NativeError) as e:
            call()
        assert (e.value.code, e.value.message) == (code, text)

    gpu = device_env("CartPole-v1", 2)
    eng = gpu._engine
    ptr = torch.zeros(64, dtype=torch.int64, device="cuda:0").data_ptr()  # (never read)
    refused(lambda: eng.lookahead(ptr, 3, 2, 0.9), STATE, "lookahead before reset")
    refused(lambda: eng.lookahead_policy(ptr, 0, 3, 2, 0.9), STATE, "lookahead_policy before reset")
    gpu.reset(seed=0)
    before = gpu.get_state()
    for name, call in (("mi_lookahead", lambda H, K, gamma, p=ptr: eng.lookahead(p, H, K, gamma)),
                       ("mi_lookahead_policy", lambda H, K, gamma, p=ptr, hidden=0: eng.lookahead_policy(p, hidden, H, K, gamma))):
        refused(lambda: call(0, 2, 0.9), INVALID, f"{name}: horizon and candidates must be >= 1")
        refused(lambda: call(3, 0, 0.9), INVALID, f"{name}: horizon and candidates must be >= 1")
        refused(lambda: call(3, 2, 1.5), INVALID, f"{name}: gamma must be in [0, 1]")
        refused(lambda: call(3, 2, float("nan")), INVALID, f"{name}: gamma must be in [0, 1]")
        what = "actions" if name == "mi_lookahead" else "params"
        refused(lambda: call(3, 2, 0.9, p=None), INVALID, f"{name}: {what} must not be NULL")
        refused(lambda: call(3, 2 ** 30, 0.9), INVALID, f"{name}: candidates * num_envs must be < 2^31")
    refused(lambda: eng.lookahead_policy(ptr, 257, 3, 2, 0.9), INVALID, "mi_lookahead_policy: hidden must be in [0, 256]")
    refused(lambda: eng.lookahead_policy(ptr, 257, 0, 2, 0.9), INVALID, "mi_lookahead_policy: hidden must be in [0, 256]")  # (hidden is tested before the horizon)
    refused(lambda: eng.lookahead(None, 0, 2, 0.9), INVALID, "mi_lookahead: actions must not be NULL")  # (... and the pointer before both)
    assert all(np.array_equal(x, y) for x, y in zip(before, gpu.get_state()))
    gpu.close()
    box = device_env("Pendulum-v1", 2)
    box.reset(seed=0)
    refused(lambda: box._engine.lookahead(ptr, 3, 2, 0.9, actions_dtype=_native.MI_I64), INVALID, "actions_dtype must be MI_F32, MI_F64 or MI_F64_WEAK")
    refused(lambda: box._engine.lookahead(ptr, 3, 2, 1.5, actions_dtype=_native.MI_I64), INVALID, "mi_lookahead: gamma must be in [0, 1]")  # (gamma first)
    box.close()
