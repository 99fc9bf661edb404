"""What HipVectorEnv.lookahead() must return, by composition of calls that existed before it (shared by the host and GPU test files of lookahead()
and lookahead_policy(); no tests here): K * N sub-environments put into the tiled state with set_state(), stepped H times, and reduced in NumPy.
Over the oracle backend that is the reference's semantics -- the oracle equals the reference bit for bit for the five classic-control ids.  Below
that: what those four test files share -- how they make envs, call the two methods and compare outputs."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import gymnasium_amd

NEEDS_RESET = 1  # _native.FLAG_NEEDS_RESET

CLASSIC_IDS = ("CartPole-v1", "Pendulum-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0")
DISCRETE_ACTIONS = {"CartPole-v1": 2, "Acrobot-v1": 3, "MountainCar-v0": 3}
BOX_BOUND = {"Pendulum-v1": 2.0, "MountainCarContinuous-v0": 1.0}


def composition(make_env, state, elapsed, flags, K, H, gamma, action_of, present_obs=None):
    """The one composition behind expected_lookahead and lookahead_policy_cases.expected_lookahead_policy: ``make_env(K * N)`` put into the tiled state
    -- lane k * N + i is candidate k of sub-environment i -- and stepped H times with ``action_of(t, obs, env)``, ``obs`` being the [K * N, obs_dim]
    observation the composed env last returned (before the first step: the tiled ``present_obs``, or None without one).  Everything after a lane's
    first terminated | truncated is masked (the composed env autoresets there), and a lane whose flags say it waits for a reset takes no step at all.
    Returns the five outputs as [K, N(, obs_dim)] arrays, and the per-step actions [H][K * N ...] and ``took`` [H][K * N] masks."""
    state, elapsed, flags = np.asarray(state, np.float64), np.asarray(elapsed, np.int32), np.asarray(flags, np.uint8)
    N = state.shape[0]
    KN = K * N
    env = make_env(KN)
    if not env._has_reset:
        env.reset(seed=0)
    env.set_state(np.tile(state, (K, 1)), np.tile(elapsed, K), np.tile(flags, K))
    alive = (np.tile(flags, K) & NEEDS_RESET) == 0
    G, disc = np.zeros(KN, np.float64), np.ones(KN, np.float64)
    steps = np.zeros(KN, np.int32)
    te_last, tr_last = np.zeros(KN, np.bool_), np.zeros(KN, np.bool_)
    obs = None if present_obs is None else np.tile(np.asarray(present_obs), (K, 1))
    final = None
    actions, took = [], []
    for t in range(H):
        a = action_of(t, obs, env)
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
        actions.append(a), took.append(go)
        alive &= ~(te | tr)
    env.close()
    out = {"returns": G.reshape(K, N), "steps": steps.reshape(K, N), "terminated": te_last.reshape(K, N), "truncated": tr_last.reshape(K, N),
           "final_obs": final.reshape((K, N) + final.shape[1:])}
    return out, actions, took


def expected_lookahead(make_env, state, elapsed, flags, actions, gamma, present_obs=None):
    """``make_env(num_envs)`` builds a NEXT_STEP env with NumPy output (and the max_episode_steps / attributes of the env under test; it may reset and
    seed it itself).  ``state`` [N, S], ``elapsed`` [N], ``flags`` [N] are the env under test's get_state(); ``actions`` is the [H, K, N(, act_dim)]
    array.  ``present_obs`` [N, obs_dim]: the observation of ``state``, needed only where a lane takes no step -- no call of the composed env
    returns it."""
    actions = np.asarray(actions)
    H, K, N = actions.shape[:3]

    def action_of(t, _obs, _env):
        a = actions[t].reshape((K * N,) + actions.shape[3:])
        if a.ndim == 1 and not np.issubdtype(a.dtype, np.integer):
            a = a.reshape(K * N, 1)  # (a Box action row whose trailing axis of 1 was omitted)
        return a

    out, _, _ = composition(make_env, state, elapsed, flags, K, H, gamma, action_of, present_obs)
    if present_obs is None and (out["steps"] == 0).any():
        raise ValueError("a lane takes no step: its final_obs is the observation of `state`, pass present_obs")
    return out


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


# ---- shared by the GPU test files ------------------------------------------------------------------------------------------------------------------
KEYS = ("returns", "steps", "terminated", "truncated", "final_obs")


def oracle_env(env_id, **kw):
    from oracle import oracle

    return lambda n: gymnasium_amd.make_vec(env_id, num_envs=n, _engine_factory=oracle.engine_factory, **kw)


def device_env(env_id, n, **kw):
    return gymnasium_amd.make_vec(env_id, num_envs=n, device=0, output="torch", **kw)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal(got, want, what, equal_nan=False):
    """``equal_nan``: where a test's own inputs make NaN observations (lookahead_policy's infinite weights), a NaN equals a NaN."""
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = np.flatnonzero((got[k] != want[k]).reshape(got[k].shape[0] * got[k].shape[1], -1).any(axis=1))
        assert np.array_equal(got[k], want[k], equal_nan=equal_nan), (what, k, bad[:6], got[k].reshape(-1)[:4], want[k].reshape(-1)[:4])


def composed_on_device(env_id, attrs, words=None, **kw):
    """make_env of the composition on the device engine: the K * N sub-environments carry the tiled attributes (and, with `words`, every copy of
    row i carries row i's generator)."""
    def make_env(n):
        env = gymnasium_amd.make_vec(env_id, num_envs=n, device=0, **kw)
        env.reset(seed=0)
        reps = n // len(next(iter(attrs.values())))
        for name, values in attrs.items():
            env.set_attr(name, list(values) * reps)
        if words is not None:
            env._engine.seed(np.tile(words, (reps, 1)))
        return env
    return make_env


# ---- shared by the host test files -------------------------------------------------------------------------------------------------------------------
def make(env_id, factory, n=4, **kw):
    kw.setdefault("output", "torch")
    return gymnasium_amd.make_vec(env_id, num_envs=n, _engine_factory=factory, **kw)


def check_struct_layout(ct, c_name, header, tmp_path):
    """The ctypes mirror `ct` against gcc's sizeof / offsetof of `c_name` in `header`."""
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler to cross-check the offsets with")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {", f'printf("size %zu\\n", sizeof({c_name}));']
    for fname, _ in ct._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({c_name}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(ct)
    for fname, _ in ct._fields_:
        assert int(out[fname]) == getattr(ct, fname).offset, fname


def good_actions(env, H=3, K=2):
    import torch

    return torch.zeros((H, K, env.num_envs) + (() if env._discrete else (1,)), dtype=torch.int64 if env._discrete else torch.float32)


def good_params(env, K=2, hidden=0):
    import torch

    return torch.zeros((K, env.policy_param_layout(hidden)["size"]), dtype=torch.float32)


# method -> (a good input for an env, the call with it -- gamma is the first of `a` --, what the checker backend answers when nothing else stands in the way)
METHODS = {"lookahead": (good_actions, lambda env, x, *a, **kw: env.lookahead(x, *a, **kw), r"needs the device engine \(mi_lookahead\)"),
           "lookahead_policy": (good_params, lambda env, x, *a, **kw: env.lookahead_policy(x, 3, *a, **kw), r"needs the device engine \(mi_lookahead_policy\)")}
KINDS_AND_MODES_WITHOUT = [("HalfCheetah-v5", {}, "MuJoCo and ToyText"), ("FrozenLake-v1", {}, "MuJoCo and ToyText"), ("Blackjack-v1", {}, "MuJoCo and ToyText"),
                           ("CartPole-v1", {"rng": "shared"}, "rng='shared'"), ("Pendulum-v1", {"fast_math": True}, "fast_math")]
