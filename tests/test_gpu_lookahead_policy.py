"""-m gpu: HipVectorEnv.lookahead_policy() (mi_lookahead_policy, gymnasium_amd/csrc/lookahead_policy.hip) against its definition by composition
(tests/lookahead_policy_cases.py expected_lookahead_policy): K * N sub-environments of the ORACLE put into the tiled state and stepped H times, the
action of every step computed in NumPy float32 from the observation the oracle last returned -- every output array_equal, no tolerance: every
operation on either side is a separately rounded IEEE float32 or float64 operation in a fixed order.  Where the oracle has no counterpart
(per-sub-environment attributes) the same composition runs on the device engine's step(), which the parity suites pin to the oracle.

The start of every case is a state the oracle REACHED by a step, so that the observation of it -- which decides the first action -- is the oracle's too."""
import functools

import numpy as np
import pytest
import torch

from lookahead_cases import (CLASSIC_IDS, DISCRETE_ACTIONS, KEYS, NEEDS_RESET, acrobot_near_height, assert_equal, cartpole_near_thresholds, composed_on_device,
                             device_env, host, mountaincar_near_goal, oracle_env)
from lookahead_policy_cases import (assert_case_is_not_trivial, expected_lookahead_policy, param_size, policy_actions, policy_logits,
                                    random_params)

pytestmark = pytest.mark.gpu

PATH_VAR = "MI355ENV_LOOKAHEAD_POLICY_PATH"
NEAR = {"CartPole-v1": cartpole_near_thresholds, "MountainCar-v0": functools.partial(mountaincar_near_goal, goal=0.5),
        "MountainCarContinuous-v0": functools.partial(mountaincar_near_goal, goal=0.45), "Acrobot-v1": acrobot_near_height}


def scale(env_id, hidden):
    """N(0, 1) weights times this, so that a Box id's actions fall on both sides of its bound.  Pendulum: |action| <= 2 against observations up to 8.
    MountainCarContinuous: |action| <= 1 against observations below 1 -- a linear policy's output is about its bias, a hidden layer's a sum over units."""
    if env_id == "MountainCarContinuous-v0":
        return 0.5 if hidden == 0 else 1.0
    return 2.0 if env_id == "Pendulum-v1" else 1.0


assert_equal = functools.partial(assert_equal, equal_nan=True)  # (test_ties_and_nan_logits makes NaN observations on both sides)


@functools.lru_cache(maxsize=None)
def start(env_id, N, cap, seed):
    """(state, elapsed, flags, present_obs): the oracle placed near where the id's episodes end (Pendulum: where reset put it), moved by two sampled
    steps; elapsed steps then spread over 0 .. cap - 1 so that truncation falls at every step of a horizon, no row waiting for its reset."""
    env = oracle_env(env_id, max_episode_steps=cap)(N)
    env.reset(seed=seed)
    if env_id in NEAR:
        env.set_state(NEAR[env_id](N, seed), np.zeros(N, np.int32), np.zeros(N, np.uint8))
    env.action_space.seed(seed)
    env.step(env.action_space.sample())
    env.set_state(None, None, np.zeros(N, np.uint8))  # (a row that ended in the first step goes on from its final state)
    obs = env.step(env.action_space.sample())[0]
    state, _, _ = env.get_state()
    env.close()
    elapsed = ((np.arange(N) * 7 + seed) % cap).astype(np.int32)
    return state, elapsed, np.zeros(N, np.uint8), np.array(obs, np.float32)


@functools.lru_cache(maxsize=None)
def case(env_id, N, K, H, hidden, gamma, cap=40, seed=5):
    state, elapsed, flags, present = start(env_id, N, cap, seed)
    params = random_params(env_id, hidden, K, seed + 100 + hidden, scale(env_id, hidden))
    want = expected_lookahead_policy(oracle_env(env_id, max_episode_steps=cap), state, elapsed, flags, present, params, hidden, H, gamma)
    return state, elapsed, flags, present, params, want


def placed(env_id, N, cap, state, elapsed, flags, **kw):
    gpu = device_env(env_id, N, max_episode_steps=cap, **kw)
    gpu.reset(seed=0)
    gpu.set_state(state, elapsed, flags)
    return gpu


def call(gpu, params, H, gamma, hidden, final_obs=True):
    return host(gpu.lookahead_policy(torch.from_numpy(params).cuda(), H, gamma, hidden=hidden, final_obs=final_obs))


# -- parity -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [0, 7])
@pytest.mark.parametrize("env_id", CLASSIC_IDS)
def test_equals_the_composition_over_the_oracle(env_id, hidden):
    """N = 300: a candidate's boundary falls inside a workgroup and inside a wavefront."""
    N, K, H, gamma, cap = 300, 3, 24, 0.97, 40
    state, elapsed, flags, _, params, want = case(env_id, N, K, H, hidden, gamma)
    assert_case_is_not_trivial(env_id, want)
    gpu = placed(env_id, N, cap, state, elapsed, flags)
    got = gpu.lookahead_policy(torch.from_numpy(params).cuda(), H, gamma, hidden=hidden, final_obs=True)
    assert_equal(host(got), want, (env_id, hidden))
    short = gpu.lookahead_policy(params, H, gamma, hidden=hidden)  # (a host array is moved, not cast)
    assert set(short) == set(KEYS) - {"final_obs"} and all(torch.equal(short[k], got[k]) for k in short)
    gpu.close()


def fits_lds(env_id, N, K, hidden):
    rows = min(K, (256 + N - 1) // N + 1)  # the candidates 256 consecutive lanes can span
    return rows * param_size(env_id, hidden) * 4 <= 32 * 1024


# (N, K, hidden, the path the host must choose)
PATH_SHAPES = [(256, 2, 64, "lds"),     # one candidate per workgroup: every lane of a wavefront reads one address
               (5, 120, 0, "lds"),      # ~53 candidates per workgroup
               (1, 300, 64, "global"),  # 256 rows of 64 units do not fit; the last workgroup partly empty
               (64, 2, 256, "lds"),     # the cap on hidden
               (130, 3, 1, "lds")]


@pytest.mark.parametrize("N,K,hidden,path", PATH_SHAPES)
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1"])
def test_parameter_paths_give_identical_bits(monkeypatch, env_id, N, K, hidden, path):
    """The path the host chooses, and each path forced (MI355ENV_LOOKAHEAD_POLICY_PATH), against the composition: identical bits.  Forcing `lds` where
    the rows do not fit is refused, which shows that the unforced call took the global path there."""
    H, gamma, cap = 12, 0.9, 20
    assert fits_lds(env_id, N, K, hidden) == (path == "lds")
    state, elapsed, flags, _, params, want = case(env_id, N, K, H, hidden, gamma, cap=cap)
    if env_id == "Pendulum-v1" and N == 1:
        # Pendulum's episodes end by truncation alone, which all candidates of ONE sub-environment share: the actions' half of the condition
        took = want["actions"][want["took"]]
        assert (np.abs(took) > 2.0).any() and not (np.abs(took) > 2.0).all()
    else:
        assert_case_is_not_trivial(env_id, want)
    gpu = placed(env_id, N, cap, state, elapsed, flags)
    monkeypatch.delenv(PATH_VAR, raising=False)
    assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, "chosen"))
    monkeypatch.setenv(PATH_VAR, "global")
    assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, "global"))
    monkeypatch.setenv(PATH_VAR, "lds")
    if path == "lds":
        assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, "lds"))
    else:
        with pytest.raises(Exception, match="exceed 32 KiB"):
            call(gpu, params, H, gamma, hidden)
    gpu.close()


@pytest.mark.parametrize("H,gamma", [(1, 0.9), (9, 0.0), (9, 0.9), (9, 1.0)])
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1", "Acrobot-v1"])
def test_horizon_one_and_the_discounts(env_id, H, gamma):
    N, K, hidden, cap = 130, 3, 3, 12
    state, elapsed, flags, _, params, want = case(env_id, N, K, H, hidden, gamma, cap=cap)
    assert_case_is_not_trivial(env_id, want)
    gpu = placed(env_id, N, cap, state, elapsed, flags)
    assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, H, gamma))
    gpu.close()


def test_outputs_that_are_not_requested_are_not_written():
    """Through the binding: every output is nullable, and an output that IS requested does not depend on which others are."""
    env_id, N, K, H, hidden, gamma = "CartPole-v1", 130, 3, 9, 3, 0.9
    state, elapsed, flags, _, params, want = case(env_id, N, K, H, hidden, gamma, cap=12)
    gpu = placed(env_id, N, 12, state, elapsed, flags)
    p = torch.from_numpy(params).cuda()
    gpu.lookahead_policy(p, H, gamma, hidden=hidden)  # (binds the stream)
    bufs = {"returns": torch.full((K, N), -7.0, dtype=torch.float64, device="cuda:0"), "steps": torch.full((K, N), -7, dtype=torch.int32, device="cuda:0"),
            "terminated": torch.full((K, N), 7, dtype=torch.uint8, device="cuda:0"), "truncated": torch.full((K, N), 7, dtype=torch.uint8, device="cuda:0"),
            "final_obs": torch.full((K, N, 4), -7.0, dtype=torch.float32, device="cuda:0")}
    for only in KEYS:
        for b in bufs.values():
            b.fill_(7 if b.dtype == torch.uint8 else -7)
        gpu._engine.lookahead_policy(p.data_ptr(), hidden, H, K, gamma, **{only: bufs[only].data_ptr()})
        gpu.synchronize()
        for k, b in bufs.items():
            x = b.cpu().numpy()
            if k == only:
                assert np.array_equal(x.astype(want[k].dtype), want[k]), (only, k)
            else:
                assert (x == (7 if b.dtype == torch.uint8 else -7)).all(), (only, k)
    gpu.close()


@pytest.mark.parametrize("mode", ["NextStep", "Disabled"])
def test_rows_that_wait_for_their_reset(mode):
    """A row whose episode ended in the last step() waits for its reset: zeros and its present observation -- the one that step() returned.  The other
    rows are scored as usual."""
    N, K, H, hidden, gamma, cap = 130, 3, 9, 3, 0.97, 7
    gpu = device_env("CartPole-v1", N, max_episode_steps=cap, autoreset_mode=mode)
    gpu.reset(seed=3)
    gpu.set_state(cartpole_near_thresholds(N, 8), (np.arange(N) % cap).astype(np.int32), np.zeros(N, np.uint8))
    present = gpu.step(torch.from_numpy(np.random.default_rng(2).integers(0, 2, N)).cuda())[0].cpu().numpy()
    state, elapsed, flags = gpu.get_state()
    pending = (flags & NEEDS_RESET) != 0
    assert 0.1 < pending.mean() < 0.9
    params = random_params("CartPole-v1", hidden, K, 17)
    want = expected_lookahead_policy(oracle_env("CartPole-v1", max_episode_steps=cap), state, elapsed, flags, present, params, hidden, H, gamma)
    got = call(gpu, params, H, gamma, hidden)
    assert_equal(got, want, mode)
    assert (got["steps"][:, pending] == 0).all() and (got["returns"][:, pending] == 0).all() and (got["steps"][:, ~pending] > 0).all()
    assert not got["terminated"][:, pending].any() and not got["truncated"][:, pending].any()
    assert np.array_equal(got["final_obs"][:, pending], np.broadcast_to(present[pending], (K,) + present[pending].shape))
    assert all(np.array_equal(x, y) for x, y in zip((state, elapsed, flags), gpu.get_state()))
    gpu.synchronize()  # (DISABLED: looking ahead from a finished row is no step of it -- no error word)
    gpu.close()


# -- rows that pin the arithmetic ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [0, 7])
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Acrobot-v1", "Pendulum-v1"])
def test_subnormal_products_are_kept(env_id, hidden):
    """Rows scaled by 1e-30 (the products of two such layers underflow), 1e-39 (the weights are subnormal themselves) and 1e-20 (the second layer's
    products are ~1e-40): NumPy keeps subnormals, so must the kernel -- flushed, a row's logits would all be zero and its action always the first."""
    N, K, H, gamma, cap = 130, 4, 9, 0.97, 12
    state, elapsed, flags, present = start(env_id, N, cap, 5)
    params = random_params(env_id, hidden, K, 41)
    params[0] *= np.float32(1e-30)
    params[1] *= np.float32(1e-39)
    params[2] *= np.float32(1e-20)
    if hidden:
        params[2, -DISCRETE_ACTIONS.get(env_id, 1):] = 0  # b2 = 0: row 2's logits are sums of ~1e-40 products
    tiny = np.finfo(np.float32).tiny
    assert (params[1] != 0).any() and (np.abs(params[1]) < tiny).all()
    y = policy_logits(env_id, params, hidden, np.tile(present, (K, 1))).reshape(K, N, -1)
    sub = (y != 0) & (np.abs(y) < tiny)
    assert sub[1].any() and (hidden == 0 or sub[2].any())  # (the expected logits themselves are subnormal)
    want = expected_lookahead_policy(oracle_env(env_id, max_episode_steps=cap), state, elapsed, flags, present, params, hidden, H, gamma)
    if env_id in DISCRETE_ACTIONS:
        k = 1 if hidden == 0 else 2  # (hidden: row 1's second-layer products underflow to zero in IEEE arithmetic too, its logits are its biases)
        assert len(np.unique(want["actions"][:, k][want["took"][:, k]])) >= 2, k  # decided among subnormal logits
    gpu = placed(env_id, N, cap, state, elapsed, flags)
    assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, hidden))
    gpu.close()


@pytest.mark.parametrize("hidden", [0, 5])
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Acrobot-v1", "MountainCar-v0"])
def test_ties_and_nan_logits(env_id, hidden):
    """Row 0: two equal output rows -- an exact tie at every step, the first maximum wins.  Row 1: the LAST two equal and larger than the first.  Rows 2 and
    3: an infinite weight -- inf - inf and 0 * inf make NaN logits; no comparison with a NaN holds (the first-layer NaN becomes 0 by the ReLU's
    z > 0 ? z : 0).  Row 4: ordinary."""
    N, K, H, gamma, cap = 130, 5, 9, 0.97, 12
    A, P = DISCRETE_ACTIONS[env_id], param_size(env_id, hidden)
    state, elapsed, flags, present = start(env_id, N, cap, 5)
    obs_dim = present.shape[1]
    params = random_params(env_id, hidden, K, 43)
    out_w = params[:, :A * obs_dim].reshape(K, A, obs_dim) if hidden == 0 else params[:, hidden * (obs_dim + 1):P - A].reshape(K, A, hidden)
    out_b = params[:, P - A:]
    out_w[0, 1], out_b[0, 1] = out_w[0, 0], out_b[0, 0]
    if hidden:
        out_w[0] = np.abs(out_w[0])  # (so that the tie is the maximum whenever a third output exists)
    out_w[1, A - 1], out_b[1, A - 1] = out_w[1, A - 2], out_b[1, A - 2]
    params[2, 0], params[2, 1] = np.inf, -np.inf  # first layer (hidden == 0: W[0][0], W[0][1])
    out_w[3, A - 1, 0], out_w[3, A - 1, 1] = np.inf, np.inf if hidden == 0 else -np.inf  # (observations of either sign, activations >= 0: one row makes NaN)
    y = policy_logits(env_id, params, hidden, np.tile(present, (K, 1))).reshape(K, N, A)
    assert np.array_equal(y[0, :, 0], y[0, :, 1]) and np.array_equal(y[1, :, A - 1], y[1, :, A - 2])
    assert np.isnan(y[2]).any() or np.isnan(y[3]).any()
    want = expected_lookahead_policy(oracle_env(env_id, max_episode_steps=cap), state, elapsed, flags, present, params, hidden, H, gamma)
    assert not (want["actions"][:, 0] == 1).any()  # (the tie never goes to the second)
    assert not (want["actions"][:, 1] == A - 1).any()
    gpu = placed(env_id, N, cap, state, elapsed, flags)
    assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, hidden))
    gpu.synchronize()  # (every action was inside the space: no error word)
    gpu.close()


# -- attributes, the generator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,name,lo,hi", [("CartPole-v1", "length", 0.25, 1.0), ("Pendulum-v1", "g", 2.0, 12.0), ("MountainCar-v0", "force", 0.0005, 0.002),
                                               ("MountainCarContinuous-v0", "power", 0.001, 0.002), ("Acrobot-v1", "LINK_MASS_2", 0.8, 1.2)])
def test_attributes_of_the_candidates_own_sub_environment(env_id, name, lo, hi):
    N, K, H, hidden, gamma, cap = 77, 5, 9, 4, 0.97, 12
    values = np.random.default_rng(1).uniform(lo, hi, N).tolist()
    state, elapsed, flags, _ = start(env_id, N, cap, 7)
    gpu = device_env(env_id, N, max_episode_steps=cap)
    gpu.reset(seed=7)
    gpu.set_attr(name, values)
    gpu.set_state(state, elapsed, flags)
    gpu.action_space.seed(3)
    present = gpu.step(torch.from_numpy(np.asarray(gpu.action_space.sample())).cuda())[0].cpu().numpy()  # the attribute types' own observation of where they went
    gpu.set_state(None, None, np.zeros(N, np.uint8))
    state, elapsed, flags = gpu.get_state()
    params = random_params(env_id, hidden, K, 23, scale(env_id, hidden))
    want = expected_lookahead_policy(composed_on_device(env_id, {name: values}, max_episode_steps=cap), state, elapsed, flags, present, params, hidden, H, gamma)
    plain = expected_lookahead_policy(oracle_env(env_id, max_episode_steps=cap), state, elapsed, flags, present, params, hidden, H, gamma)
    assert (want["final_obs"] != plain["final_obs"]).any(axis=-1).mean() > 0.5  # (the attribute matters to the result)
    assert_equal(call(gpu, params, H, gamma, hidden), want, (env_id, name))
    gpu.close()


def test_acrobot_torque_noise_comes_from_a_copy_of_the_generator():
    """Every candidate of sub-environment i draws what the env itself would draw next: candidates with equal parameters give equal results, and the
    env's generator does not move."""
    N, K, H, hidden, gamma = 77, 4, 9, 4, 0.97
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
    params = random_params("Acrobot-v1", hidden, K, 29)
    params[2] = params[0]  # two candidates with equal parameters
    make_env = composed_on_device("Acrobot-v1", {"torque_noise_max": noise, "LINK_MASS_2": mass}, words=words)
    want = expected_lookahead_policy(make_env, state, elapsed, flags, present, params, hidden, H, gamma)
    got = call(gpu, params, H, gamma, hidden)
    assert_equal(got, want, "noise")
    assert all(np.array_equal(got[k][0], got[k][2]) for k in KEYS) and (got["final_obs"][0] != got["final_obs"][1]).any()
    quiet = expected_lookahead_policy(composed_on_device("Acrobot-v1", {"torque_noise_max": [0.0] * N, "LINK_MASS_2": mass}, words=words), state, elapsed,
                                      flags, present, params, hidden, H, gamma)
    assert (quiet["final_obs"] != want["final_obs"]).any()  # (the noise matters to the result)
    assert np.array_equal(gpu.get_rng_state(), words) and all(np.array_equal(x, y) for x, y in zip(gpu.get_state(), (state, elapsed, flags)))
    assert_equal(call(gpu, params, H, gamma, hidden), got, "a second call draws the same noise")
    gpu.close()


# -- the env ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1", "Acrobot-v1"])
def test_the_env_is_untouched(env_id):
    """State, generators, statistics and the action stream before and after; and whatever comes next equals a twin's that never looked ahead."""
    N, K, H, hidden = 130, 3, 9, 4
    a, b = device_env(env_id, N, max_episode_steps=20), device_env(env_id, N, max_episode_steps=20)
    for env in (a, b):
        env.reset(seed=6)
        env.action_space.seed(6)
        env.rollout(5)
    before = a.get_state(), a.get_rng_state(), a.statistics()
    out = a.lookahead_policy(random_params(env_id, hidden, K, 3), H, 0.9, hidden=hidden, final_obs=True)
    assert (out["steps"] > 0).any()
    after = a.get_state(), a.get_rng_state(), a.statistics()
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    act = np.asarray(a.action_space.sample())
    assert np.array_equal(act, np.asarray(b.action_space.sample()))
    sa, sb = a.step(torch.from_numpy(act).cuda()), b.step(torch.from_numpy(act).cuda())  # a following step() equals the twin's
    assert all(torch.equal(x, y) for x, y in zip(sa[:4], sb[:4]))
    ra, rb = a.rollout(8), b.rollout(8)
    assert set(ra) == set(rb) and all(torch.equal(ra[k], rb[k]) for k in ra)
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state())) and np.array_equal(a.get_rng_state(), b.get_rng_state())
    assert a.statistics() == b.statistics()
    a.close(), b.close()


@pytest.mark.parametrize("env_id,hidden", [("CartPole-v1", 0), ("Pendulum-v1", 7)])
def test_one_call_inside_a_graph_capture_replays_to_the_same_result(env_id, hidden):
    """One launch on the env's stream, no synchronisation: capturable.  The replay reads the env as it then stands."""
    N, K, H, gamma, cap = 300, 3, 24, 0.97, 40
    state, elapsed, flags, _, params, want = case(env_id, N, K, H, hidden, gamma)
    gpu = placed(env_id, N, cap, state, elapsed, flags)
    p = torch.from_numpy(params).cuda()
    eager = gpu.lookahead_policy(p, H, gamma, hidden=hidden, final_obs=True)  # (kernels load on first use, which a capture must not trigger)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gpu.lookahead_policy(p, H, gamma, hidden=hidden, final_obs=True)
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert_equal(host(out), want, "replay")
    assert all(torch.equal(out[k], eager[k]) for k in KEYS)
    assert all(np.array_equal(x, y) for x, y in zip(gpu.get_state(), (state, elapsed, flags)))
    gpu.close()
