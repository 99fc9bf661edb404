"""What HipVectorEnv.lookahead() must return, by composition of calls that existed before it (shared by tests/test_lookahead_host.py and
tests/test_gpu_lookahead.py; no tests here): K * N sub-environments put into the tiled state with set_state(), stepped H times, and reduced in NumPy.
Over the oracle backend that is the reference's semantics -- the oracle equals the reference bit for bit for the five classic-control ids."""
import numpy as np

NEEDS_RESET = 1  # _native.FLAG_NEEDS_RESET

CLASSIC_IDS = ("CartPole-v1", "Pendulum-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0")
DISCRETE_ACTIONS = {"CartPole-v1": 2, "Acrobot-v1": 3, "MountainCar-v0": 3}
BOX_BOUND = {"Pendulum-v1": 2.0, "MountainCarContinuous-v0": 1.0}


def expected_lookahead(make_env, state, elapsed, flags, actions, gamma, present_obs=None):
    """``make_env(num_envs)`` builds a NEXT_STEP env with NumPy output (and the max_episode_steps / attributes of the env under test; it may reset and
    seed it itself).  ``state`` [N, S], ``elapsed`` [N], ``flags`` [N] are the env under test's get_state(); ``actions`` is the [H, K, N(, act_dim)]
    array.  Lane k * N + i of the composed env is candidate k of sub-environment i.  Everything after a lane's first terminated | truncated is masked
    (the composed env autoresets there), and a lane whose flags say it waits for a reset takes no step at all.  ``present_obs`` [N, obs_dim]: the
    observation of ``state``, needed only where a lane takes no step -- no call of the composed env returns it."""
    actions = np.asarray(actions)
    state, elapsed, flags = np.asarray(state, np.float64), np.asarray(elapsed, np.int32), np.asarray(flags, np.uint8)
    H, K, N = actions.shape[:3]
    KN = K * N
    env = make_env(KN)
    if not env._has_reset:
        env.reset(seed=0)
    env.set_state(np.tile(state, (K, 1)), np.tile(elapsed, K), np.tile(flags, K))
    alive = (np.tile(flags, K) & NEEDS_RESET) == 0
    G, disc = np.zeros(KN, np.float64), np.ones(KN, np.float64)
    steps = np.zeros(KN, np.int32)
    te_last, tr_last = np.zeros(KN, np.bool_), np.zeros(KN, np.bool_)
    final = None
    for t in range(H):
        a = actions[t].reshape((KN,) + actions.shape[3:])
        if a.ndim == 1 and not np.issubdtype(a.dtype, np.integer):
            a = a.reshape(KN, 1)  # (a Box action row whose trailing axis of 1 was omitted)
        obs, rew, te, tr, _ = env.step(a)
        obs, rew, te, tr = np.array(obs), np.asarray(rew, np.float64), np.asarray(te, np.bool_), np.asarray(tr, np.bool_)
        if final is None:
            final = np.zeros_like(obs)
            if present_obs is not None:
                final[:] = np.tile(np.asarray(present_obs, obs.dtype), (K, 1))
        go = alive.copy()
        term = disc * rew  # rounded, then added: the kernel's order
        G = np.where(go, G + term, G)
        disc = np.where(go, disc * np.float64(gamma), disc)
        steps += go
        te_last, tr_last = np.where(go, te, te_last), np.where(go, tr, tr_last)
        final[go] = obs[go]
        alive &= ~(te | tr)
    env.close()
    if present_obs is None and (steps == 0).any():
        raise ValueError("a lane takes no step: its final_obs is the observation of `state`, pass present_obs")
    return {"returns": G.reshape(K, N), "steps": steps.reshape(K, N), "terminated": te_last.reshape(K, N), "truncated": tr_last.reshape(K, N),
            "final_obs": final.reshape((K, N) + final.shape[1:])}


def random_actions(env_id, H, K, N, seed, dtype=None):
    """[H, K, N] int64 for the Discrete ids, [H, K, N, 1] float32 (or ``dtype``) inside and a little outside the Box for the others."""
    rng = np.random.default_rng(seed)
    if env_id in DISCRETE_ACTIONS:
        return rng.integers(0, DISCRETE_ACTIONS[env_id], (H, K, N), dtype=np.int64)
    b = BOX_BOUND[env_id]
    a = rng.uniform(-1.25 * b, 1.25 * b, (H, K, N, 1))
    return a.astype(np.float32 if dtype is None else dtype)


# ---- states placed with set_state(), inside the domain set_state accepts, near where each id's episodes end ---------------------------------------------
def cartpole_near_thresholds(n, seed):
    """cartpole.py:206-211: |x| > 2.4 or |theta| > 12 degrees (0.2095) ends the episode; within a few steps of either, from both sides."""
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), np.float64)
    side = rng.choice([-1.0, 1.0], n)
    near_x = rng.integers(0, 2, n) == 0
    s[:, 0] = np.where(near_x, side * rng.uniform(2.25, 2.399, n), rng.uniform(-1.0, 1.0, n))
    s[:, 1] = np.where(near_x, rng.uniform(-1.5, 1.5, n), rng.uniform(-0.5, 0.5, n))
    s[:, 2] = np.where(near_x, rng.uniform(-0.05, 0.05, n), side * rng.uniform(0.15, 0.209, n))
    s[:, 3] = np.where(near_x, rng.uniform(-0.3, 0.3, n), rng.uniform(-1.0, 1.0, n))
    return s


def mountaincar_near_goal(n, seed, goal=0.5):
    """mountain_car.py:147 / continuous_mountain_car.py:170: position >= goal (0.5 / 0.45) with velocity >= 0 ends the episode."""
    rng = np.random.default_rng(seed)
    s = np.empty((n, 2), np.float64)
    s[:, 0] = goal - rng.uniform(0.0, 0.45, n)
    s[:, 1] = rng.uniform(0.0, 0.07, n)
    return s


def acrobot_near_height(n, seed):
    """acrobot.py:239-242: -cos(theta1) - cos(theta1 + theta2) > 1 ends the episode; the tip a little below that line, moving."""
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), np.float64)
    s[:, 0] = rng.choice([-1.0, 1.0], n) * rng.uniform(1.7, 2.05, n)
    s[:, 1] = rng.uniform(-0.3, 0.3, n)
    s[:, 2] = rng.uniform(-2.0, 2.0, n)
    s[:, 3] = rng.uniform(-2.0, 2.0, n)
    return s
