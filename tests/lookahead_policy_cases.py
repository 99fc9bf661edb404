"""What HipVectorEnv.lookahead_policy() must return, by composition of calls that existed before it (shared by tests/test_lookahead_policy_host.py and
tests/test_gpu_lookahead_policy.py; no tests here): tests/lookahead_cases.py's composition() -- K * N sub-environments put into the tiled state and stepped H
times -- with the action of every step computed from the observation the composed env last returned, by the network of include/mi355env.h
(mi_lookahead_policy) restated in NumPy float32.  Over the oracle backend that is the reference's semantics."""
import numpy as np

from lookahead_cases import BOX_BOUND, CLASSIC_IDS, DISCRETE_ACTIONS, composition

OBS_DIM = {"CartPole-v1": 4, "Pendulum-v1": 3, "Acrobot-v1": 6, "MountainCar-v0": 2, "MountainCarContinuous-v0": 2}
KIND_ID = {"cartpole": "CartPole-v1", "pendulum": "Pendulum-v1", "acrobot": "Acrobot-v1", "mountain_car": "MountainCar-v0",
           "mountain_car_continuous": "MountainCarContinuous-v0"}
assert set(OBS_DIM) == set(CLASSIC_IDS)


def n_outputs(env_id):
    return DISCRETE_ACTIONS.get(env_id, 1)


def param_size(env_id, hidden):
    obs, A = OBS_DIM[env_id], n_outputs(env_id)
    return A * (obs + 1) if hidden == 0 else hidden * (obs + 1) + A * (hidden + 1)


def split_params(env_id, params, hidden):
    """[K, P] -> the parts of every row: (W [K, A, OBS], b [K, A]) for hidden == 0, (W1 [K, h, OBS], b1 [K, h], W2 [K, A, h], b2 [K, A]) otherwise."""
    obs, A, h = OBS_DIM[env_id], n_outputs(env_id), hidden
    K = params.shape[0]
    assert params.dtype == np.float32 and params.shape == (K, param_size(env_id, hidden)), (params.dtype, params.shape)
    if h == 0:
        return params[:, :A * obs].reshape(K, A, obs), params[:, A * obs:]
    at = [h * obs, h * obs + h, h * obs + h + A * h]
    return params[:, :at[0]].reshape(K, h, obs), params[:, at[0]:at[1]], params[:, at[1]:at[2]].reshape(K, A, h), params[:, at[2]:]


def policy_logits(env_id, params, hidden, obs):
    """y [L, A] float32 for L = K * n lanes, lane l using row l // n of ``params`` [K, P]: explicit loops over j, u and o in the contract's order,
    vectorised over lanes only; every operand is float32, so every product and every sum rounds once."""
    params, obs = np.asarray(params), np.asarray(obs)
    assert obs.dtype == np.float32 and obs.ndim == 2 and obs.shape[1] == OBS_DIM[env_id] and obs.shape[0] % params.shape[0] == 0
    L, OBS, A = obs.shape[0], OBS_DIM[env_id], n_outputs(env_id)
    rep = L // params.shape[0]
    parts = [np.repeat(p, rep, axis=0) for p in split_params(env_id, params, hidden)]
    y = np.empty((L, A), np.float32)
    with np.errstate(all="ignore"):
        if hidden == 0:
            W, b = parts
            for o in range(A):
                y[:, o] = b[:, o]
                for j in range(OBS):
                    y[:, o] = y[:, o] + W[:, o, j] * obs[:, j]
        else:
            W1, b1, W2, b2 = parts
            for o in range(A):
                y[:, o] = b2[:, o]
            for u in range(hidden):
                z = b1[:, u].copy()
                for j in range(OBS):
                    z = z + W1[:, u, j] * obs[:, j]
                a = np.where(z > 0, z, np.float32(0))
                assert a.dtype == np.float32
                for o in range(A):
                    y[:, o] = y[:, o] + W2[:, o, u] * a
    return y


def policy_actions(env_id, params, hidden, obs):
    """The action of every lane: [L] int64 by the strict-greater scan (first maximum wins, a NaN never wins) for the Discrete ids, [L, 1] float32 (y[0],
    unclipped) for the Box ids."""
    y = policy_logits(env_id, params, hidden, obs)
    if env_id not in DISCRETE_ACTIONS:
        return y[:, :1].copy()
    best = np.zeros(y.shape[0], np.int64)
    rows = np.arange(y.shape[0])
    with np.errstate(invalid="ignore"):
        for o in range(1, y.shape[1]):
            best = np.where(y[:, o] > y[rows, best], o, best)
    return best


def expected_lookahead_policy(make_env, state, elapsed, flags, present_obs, params, hidden, H, gamma):
    """lookahead_cases.expected_lookahead with closed-loop actions.  ``present_obs`` [N, obs_dim] float32 is the observation of ``state`` (always
    needed here: it decides the first action); ``params`` [K, P] float32.  Beyond the five outputs the dict holds ``actions`` [H, K, N(, 1)] and ``took``
    [H, K, N] (the candidate took step t), for the conditions a test sets on its inputs."""
    params, present_obs = np.asarray(params), np.asarray(present_obs)
    assert present_obs.dtype == np.float32
    K, N = params.shape[0], np.asarray(state).shape[0]
    out, actions, took = composition(make_env, state, elapsed, flags, K, H, gamma,
                                     lambda t, obs, env: policy_actions(KIND_ID[env.KIND], params, hidden, obs), present_obs)
    actions = np.stack(actions)
    return dict(out, actions=actions.reshape((H, K, N) + actions.shape[2:]), took=np.stack(took).reshape(H, K, N))


def assert_case_is_not_trivial(env_id, want):
    """The condition every parametrised parity case sets on its EXPECTED arrays: finished and unfinished candidates, and actions that differ -- two
    distinct ones for a Discrete id, a clipped and an unclipped one for a Box id -- among the steps that were taken."""
    ended = want["terminated"] | want["truncated"]
    assert ended.any() and not ended.all(), (env_id, ended.mean())
    taken = want["actions"][want["took"]]
    assert taken.size
    if env_id in DISCRETE_ACTIONS:
        assert len(np.unique(taken)) >= 2, (env_id, np.unique(taken))
    else:
        clipped = np.abs(taken) > BOX_BOUND[env_id]
        assert clipped.any() and not clipped.all(), (env_id, clipped.mean())


def random_params(env_id, hidden, K, seed, scale=1.0):
    """[K, P] float32, N(0, 1) * scale from a seeded generator."""
    return (np.random.default_rng(seed).standard_normal((K, param_size(env_id, hidden))) * scale).astype(np.float32)
