"""Shared by tests/test_gpu_rollout_infos.py (GPU) and tests/test_rollout_infos.py (CPU): the cases of the comparison
``rollout(T, infos=True)`` == T x ``step()``, how a case's two sides are stepped, stacked and compared, and the guards that keep a comparison
from being vacuous.

Shapes (classic control): 300 sub-environments = more than one 256-thread workgroup with a ragged last one; T = 19 is odd, no multiple of the
refill period of 8, and Acrobot's loop is unrolled by two; max_episode_steps = 5 puts truncations on many steps and lets an autoreset step be
followed by another finish inside the window.  One CartPole case with max_episode_steps = 30, T = 64 has terminations AND truncations.
MuJoCo: 5 sub-environments (a ragged wavefront / cooperative group), T = 6, max_episode_steps = 3.

The seeds below were chosen -- seeds, not shapes -- so that the CPU checker's trajectories satisfy the guards; tests/test_rollout_infos.py
re-checks that on the CPU with the checker backend and T step() calls, the GPU tests assert the same guards on what they compared.
"""
import numpy as np

import gymnasium_amd

CLASSIC_IDS = ("CartPole-v1", "Pendulum-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0")
MODES = ("NextStep", "SameStep")
RESET_SEED, ACTION_SEED = 5, 9

# (env id, num_envs, T, max_episode_steps)
CLASSIC_CASES = [(env_id, 300, 19, 5) for env_id in CLASSIC_IDS]
CARTPOLE_LONG = ("CartPole-v1", 300, 64, 30)
# The share of (t, i) cells that must have finished an episode: a tenth -- except in the long CartPole case, where no seed can give that: a
# random-policy CartPole episode lasts ~22 steps (the shortest possible ~8), so at most one cell in ~23 finishes one.  What its shape does
# guarantee: an episode is over after 30 steps and the autoreset step, so every sub-environment finishes at least floor(64 / 31) = 2 in 64 steps.
MIN_DONE, MIN_DONE_LONG = 0.1, 2 / 64
MUJOCO_CASES = [("InvertedPendulum-v5", 5, 6, 3), ("Ant-v5", 5, 6, 3), ("Humanoid-v5", 5, 6, 3)]


def make_pair(env_id, n, max_episode_steps, mode, stats, factory=None, **kw):
    """Two envs of the same configuration with device tensors (the checker backend's "device" is the host)."""
    extra = {} if factory is None else {"_engine_factory": factory}
    common = dict(num_envs=n, max_episode_steps=max_episode_steps, autoreset_mode=mode, output="torch", record_episode_statistics=stats, **kw, **extra)
    a, b = gymnasium_amd.make_vec(env_id, **common), gymnasium_amd.make_vec(env_id, **common)
    a.reset(seed=RESET_SEED), b.reset(seed=RESET_SEED)
    a.action_space.seed(ACTION_SEED), b.action_space.seed(ACTION_SEED)
    return a, b


def caller_actions(env, T, seed=17):
    """T batches inside the action space from a generator of the test's own, as a tensor on the env's device."""
    import torch

    space, rng = env.single_action_space, np.random.default_rng(seed)
    if hasattr(space, "n"):
        acts = rng.integers(0, int(space.n), size=(T, env.num_envs), dtype=np.int64)
    else:
        lo, hi = np.asarray(space.low, dtype=np.float64), np.asarray(space.high, dtype=np.float64)
        acts = (lo + (hi - lo) * rng.random((T, env.num_envs) + space.shape)).astype(np.float32)
    return torch.from_numpy(acts).to(env._tdev)


def stack_steps(env, T, actions=None):
    """T step() calls: (obs, rewards, terminations, truncations, actions) stacked, and the T info dicts stacked key by key.
    actions None: ``step(action_space.sample())``, the policy a rollout without actions evaluates on the device."""
    import torch

    cols, infos = [[] for _ in range(5)], []
    for t in range(T):
        act = torch.from_numpy(env.action_space.sample()).to(env._tdev) if actions is None else actions[t]
        o, r, te, tr, info = env.step(act)
        for c, v in zip(cols, (o, r, te, tr, act)):
            c.append(v.clone())
        infos.append(info)
    return tuple(torch.stack(c) for c in cols), stack_infos(infos)


def stack_infos(infos):
    import torch

    out = {}
    for k in infos[0]:
        out[k] = stack_infos([i[k] for i in infos]) if isinstance(infos[0][k], dict) else torch.stack([i[k].clone() for i in infos])
    return out


def _host(x):
    return x.cpu().numpy()


def compare_infos(ref, got, zero_fill, path="infos", outer_mask=None, masks=None):
    """Every key of ``ref`` (stacked step() dicts) against ``got``: the masks array_equal everywhere, the values array_equal where the mask is
    true and -- ``zero_fill``: ``got`` is a rollout's -- exactly 0 elsewhere.  "t" (a wall-clock value) is not compared.  Collects the masks into
    ``masks`` ({path: array}) for the guards."""
    assert set(ref) == set(got), (path, sorted(ref), sorted(got))
    for k, v in ref.items():
        if k.startswith("_"):
            m = _host(v)
            assert m.dtype == np.bool_ and np.array_equal(m, _host(got[k])), f"{path}[{k!r}]: masks differ"
            if masks is not None:
                masks[f"{path}[{k!r}]"] = m
    for k, v in ref.items():
        if k.startswith("_") or k == "t":
            continue
        m = _host(ref["_" + k]) if "_" + k in ref else outer_mask
        assert m is not None, f"{path}[{k!r}] has no mask"
        if isinstance(v, dict):
            compare_infos(v, got[k], zero_fill, f"{path}[{k!r}]", m, masks)
            continue
        a, b = _host(v), _host(got[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (path, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a[m], b[m]), f"{path}[{k!r}]: values differ where the mask is true"
        if zero_fill:
            assert not b[~m].any(), f"{path}[{k!r}]: a rollout's rows without a value must be zero"


def assert_guards(env, dones, masks, terminations=None, truncations=None, both_flags=False):
    """No comparison may be vacuous: at least a tenth of the (t, i) cells finished an episode (the long CartPole case: MIN_DONE_LONG, see
    there, and both flags occur), every mask has true cells, and every mask has false cells too -- except the masks of the keys every
    sub-environment supplies at every step by construction (the entries of the scalar env's RESET info, reported by step and reset alike:
    HipVectorEnv._info_columns), which must be all true."""
    need = MIN_DONE_LONG if both_flags else MIN_DONE
    assert dones.mean() >= need, f"only {dones.mean():.3f} of the cells finished an episode, {need:.3f} needed"
    if both_flags:
        assert terminations.any() and truncations.any(), "the long CartPole case needs terminations and truncations"
    always = {f"infos['_{name}']" for name, _, _, in_reset in env.unwrapped._info_columns() if in_reset}
    for path, m in masks.items():
        assert m.any(), f"{path} has no true cell"
        if path in always:
            assert m.all(), f"{path}: a key of the reset info is supplied by every sub-environment at every step"
        else:
            assert not m.all(), f"{path} has no false cell"
