"""gymnasium.wrappers.vector.{NormalizeObservation, NormalizeReward, ClipReward} with the batch kept in HBM.

Same constructor arguments, attributes (`obs_rms`, `return_rms`, `epsilon`, `gamma`, `update_running_mean`) and errors as

  gymnasium/wrappers/vector/stateful_observation.py:27-160   NormalizeObservation
  gymnasium/wrappers/vector/stateful_reward.py:21-183        NormalizeReward
  gymnasium/wrappers/vector/vectorize_reward.py:115-151      ClipReward
  gymnasium/wrappers/utils.py:33-71                          RunningMeanStd

but the arithmetic runs in libmi355env.so on the GPU (the wrappers have no CPU implementation -- the NumPy restatement in
oracle/wrappers.py is test infrastructure), in one of two forms:

* FUSED (classic-control HipVectorEnv directly underneath, possibly through RecordEpisodeStatistics / NumpyToTorch): the wrapper registers
  itself with the env and its arithmetic becomes the output stage of the step kernel (mi_set_step_epilogue, csrc/classic_kernels.h): the batch
  statistics are gathered by the step kernel's workgroups, one small second launch normalises in place -- NumPy callers get the wrapped
  batch with the step's one device-to-host copy.  The fusion is SCOPED to the call: a ``step()`` entered through fused wrapper k runs the
  arithmetic of the fused wrappers up to k; stepping the env itself (``w.env.step``, ``w.unwrapped.step``) or an inner wrapper returns that
  object's own values -- raw for the env -- and leaves the outer wrappers' statistics alone, as in the reference.  Settings (``gamma``,
  ``epsilon``, ``min_reward``, ``max_reward``, ``update_running_mean``) are read at every step.
* STAND-ALONE (any other env of this package, or a wrapper order the epilogue cannot express): passes of csrc/wrappers.hip over the arrays
  the engine produced; with ``output="torch"`` nothing leaves the GPU, NumPy batches are staged through the device.

``rollout(T)`` of a wrapper returns what T consecutive ``step()`` calls through it would have returned, as the time-major device tensors
of ``HipVectorEnv.rollout``, and leaves its statistics, accumulators and previous-done flags as those calls would have: each wrapper takes the
trajectory the wrapper below returned and runs its pass over all T steps at once (mi_normalize_observation_steps, mi_normalize_reward_steps,
mi_clip_reward over T * N elements) -- a fixed number of launches, on the handles ``step()`` uses, so ``step()``, ``rollout()`` and ``reset()``
interleave like one long sequence of steps.  The scoping rule holds by construction: ``w.rollout`` applies the wrappers up to ``w``.

The ACTION wrappers (ClipAction, RescaleAction, TransformAction; gymnasium/wrappers/vector/vectorize_action.py) change what goes INTO the step:
device tensors are transformed by mi_transform_actions (csrc/action_wrappers.hip) in one launch per ``step()`` / per ``rollout()`` block, NumPy
batches by one NumPy expression on the host; both give the reference's row-by-row result bit for bit.  They are transparent to the fused unit.

The OBSERVATION and REWARD transforms (RescaleObservation, DtypeObservation, FlattenObservation, TransformObservation, TransformReward;
gymnasium/wrappers/vector/vectorize_observation.py, vectorize_reward.py) change what comes OUT of the step, statelessly: device tensors go through
mi_transform_observations / mi_one_hot (csrc/observation_wrappers.hip) in one launch per ``step()`` / ``reset()`` / ``rollout()`` trajectory, NumPy
batches through one NumPy expression.  They are neither transparent nor fused -- what sits above them sees transformed values -- and refuse
``capture_steps`` (docs/observation_wrappers.md).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native
from ..gym_api import AutoresetMode, batch_space, error, spaces


def _torch():
    import torch

    return torch


class RunningMeanStd:
    """Device-resident mean / var / count (wrappers/utils.py:33-71); `.mean`, `.var`, `.count` read them back as NumPy."""

    def __init__(self, epsilon=1e-4, shape=(), dtype=np.float64, device=0):
        self._lib = _native.load_library()
        self.shape = tuple(shape)
        self.dim = int(np.prod(self.shape)) if self.shape else 1
        self.dtype = np.dtype(dtype)
        self.device = int(device)
        self._h = C.c_void_p()
        code = _native.MI_F32 if self.dtype == np.float32 else _native.MI_F64
        self._lib.check(self._lib.rms_create(self.device, self.dim, code, float(epsilon), C.byref(self._h)))

    def _get(self):
        mean, var, count = np.zeros(self.dim), np.zeros(self.dim), np.zeros(1)
        self._lib.check(self._lib.rms_get(self._h, _stream(), mean.ctypes.data, var.ctypes.data, count.ctypes.data))
        return mean, var, float(count[0])

    @property
    def mean(self):
        return self._get()[0].reshape(self.shape)

    @property
    def var(self):
        return self._get()[1].reshape(self.shape)

    @property
    def count(self):
        return self._get()[2]

    def set(self, mean=None, var=None, count=None):
        arrs = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), self.shape or (1,)).reshape(-1))
                for a in (mean, var)]
        cnt = None if count is None else np.array([float(count)])
        self._lib.check(self._lib.rms_set(self._h, _stream(), *[None if a is None else a.ctypes.data for a in arrs],
                                          None if cnt is None else cnt.ctypes.data))

    def close(self):
        if self._h:
            self._lib.rms_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _base_env(env):
    while isinstance(env, VectorWrapper):
        env = env.env
    return env


def _fusion_base(env):
    """The HipVectorEnv under ``env`` if it fuses wrappers and everything in between passes observations and rewards through unchanged (or
    is itself part of the fused unit); None otherwise."""
    e = env
    while isinstance(e, VectorWrapper):
        if not (e._transparent or e._fused):
            return None
        e = e.env
    return e if getattr(e, "_can_fuse", None) is not None and e._can_fuse() else None


def _close_fusion(env):
    """A stand-alone wrapper now sits on top of ``env``: nothing above it may join the fused unit underneath."""
    base = _base_env(env)
    if getattr(base, "_fusion_state", None) is not None and getattr(base, "FUSES_WRAPPERS", False):
        base._fusion_state()["closed"] = True


class VectorWrapper:
    """Minimal gymnasium.vector.VectorWrapper: forwards everything to the wrapped vector env (vector_env.py:341-470)."""

    _transparent = False  # True: observations and rewards pass through unchanged (a fused unit may extend across this wrapper)
    _fused = False        # True: this wrapper's arithmetic runs inside the step kernel of the HipVectorEnv underneath

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self.env, name)

    @property
    def unwrapped(self):
        return self.env.unwrapped

    def reset(self, *, seed=None, options=None):
        return self.env.reset(seed=seed, options=options)

    def step(self, actions):
        return self.env.step(actions)

    def rollout(self, num_steps, actions=None, **kwargs):
        """``num_steps`` consecutive ``step()`` calls through this wrapper at once (HipVectorEnv.rollout): here, the wrapped env's own."""
        return self.env.rollout(num_steps, actions, **kwargs)

    def lookahead(self, actions, gamma=1.0, **kwargs):
        """Not through a wrapper: the engine scores candidates with the plain env's actions, rewards and observations, which are not this wrapper's."""
        raise error.Error(f"{type(self).__name__}: lookahead() is not offered through wrappers -- forwarding it would hand back the unwrapped env's rewards "
                          "and observations as if they were this wrapper's; call env.unwrapped.lookahead(...) if those are what you want")

    def lookahead_policy(self, params, horizon, gamma=1.0, **kwargs):
        """Not through a wrapper, for lookahead()'s reason: the candidates see, and are scored by, the plain env's observations and rewards."""
        raise error.Error(f"{type(self).__name__}: lookahead_policy() is not offered through wrappers -- the candidate policies would be fed the unwrapped "
                          "env's observations and scored by its rewards as if they were this wrapper's; call env.unwrapped.lookahead_policy(...) if those "
                          "are what you want")

    def _workspace(self, steps, rows, dim):
        """Scratch of the whole-trajectory passes: a tensor from the caching allocator, so that the library neither allocates nor synchronises."""
        lib = _native.load_library()
        size = lib.wrapper_steps_workspace(int(steps), int(rows), int(dim))
        if size < 0:  # MI_ERR_INVALID_ARGUMENT: more than 65535 steps, or a step of 2^31 elements
            lib.check(int(size))
        return _torch().empty(size, dtype=_torch().uint8, device=f"cuda:{self._dev()}"), size

    def _step_fused(self, actions):
        """step() of a fused wrapper: mark this call as entered through `self` (the outermost fused wrapper of a call wins) and run the
        chain underneath -- the engine's step applies the epilogue of the members up to the entry (HipVectorEnv._sync_epilogue)."""
        st = self._base._fusion_state()
        outermost = st["entry"] is None
        if outermost:
            st["entry"] = self
        try:
            return self.env.step(actions)
        finally:
            if outermost:
                st["entry"] = None

    def close(self, **kwargs):
        return self.env.close(**kwargs)

    # staging helpers: device tensors pass through, NumPy batches go to the device and back
    def _dev(self):
        return getattr(self.env, "_device_index", 0)

    def _to_device(self, x, dtype=None):
        torch = _torch()
        if isinstance(x, torch.Tensor):
            return x.contiguous(), True
        t = torch.from_numpy(np.ascontiguousarray(x if dtype is None else np.asarray(x, dtype=dtype))).to(f"cuda:{self._dev()}")
        return t, False

    @staticmethod
    def _back(t, was_tensor):
        return t if was_tensor else t.cpu().numpy()


class RecordEpisodeStatistics(VectorWrapper):
    """gymnasium.wrappers.vector.RecordEpisodeStatistics (wrappers/vector/common.py:22-235) on the engine's own accounting: the step
    kernels accumulate each sub-environment's return and length on the device (NEXT_STEP: the autoreset step does not count; SAME_STEP:
    every step counts) and hand out the rows of the episodes that just ended; this class adds the reference's bookkeeping around them --
    ``infos[stats_key] = {"r", "l", "t"}`` + ``infos["_" + stats_key]``, ``episode_count`` and the three bounded queues."""

    _transparent = True

    def __init__(self, env, buffer_length: int = 100, stats_key: str = "episode"):
        from collections import deque

        super().__init__(env)
        if not hasattr(env.unwrapped, "enable_episode_statistics"):
            raise TypeError("RecordEpisodeStatistics of gymnasium_amd wraps a HipVectorEnv (use gymnasium's own wrapper for other vector envs)")
        env.unwrapped.enable_episode_statistics()
        self._stats_key = stats_key
        self.time_queue, self.return_queue, self.length_queue = deque(maxlen=buffer_length), deque(maxlen=buffer_length), deque(maxlen=buffer_length)

    @property
    def episode_count(self):
        return self.env.unwrapped.episode_count

    def step(self, actions):
        obs, rewards, terminations, truncations, infos = self.env.step(actions)
        found = self._rename(infos)
        if found is not None:
            stats, dones = found
            # common.py:214-217: the queues take the finished episodes in sub-environment order.  Device-resident infos (output="torch"): the
            # queues live on the host, so this wrapper reads the done mask back every step (the env underneath does not synchronise by itself)
            self._extend_queues(stats, dones)
        return obs, rewards, terminations, truncations, infos

    def _rename(self, infos):
        """infos["episode"] / ["_episode"] under this wrapper's key (common.py:205-213); returns (stats, dones) or None when there are none."""
        if "_episode" not in infos:
            return None
        stats, dones = infos.pop("episode"), infos.pop("_episode")
        if self._stats_key in infos or f"_{self._stats_key}" in infos:
            raise ValueError(f"Attempted to add episode stats with key '{self._stats_key}' but this key already exists in info: {list(infos.keys())}")
        infos[self._stats_key], infos[f"_{self._stats_key}"] = stats, dones
        return stats, dones

    def _extend_queues(self, stats, dones):
        """The finished episodes of one step ([N] arrays) or of a rollout ([T, N]: row-major, i.e. step by step and within a step in
        sub-environment order -- the order T step() calls extend the queues in) onto the three queues."""
        host = (lambda x: x.cpu().numpy()) if hasattr(dones, "cpu") else (lambda x: np.asarray(x))
        idx = np.flatnonzero(host(dones).reshape(-1))
        if idx.size:
            self.time_queue.extend(host(stats["t"]).reshape(-1)[idx]), self.return_queue.extend(host(stats["r"]).reshape(-1)[idx])
            self.length_queue.extend(host(stats["l"]).reshape(-1)[idx])

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` through this wrapper: the wrapped rollout ALWAYS runs with ``infos=True`` (the kernels store every step's
        finished-episode rows), so ``episode_count`` and the three queues end as those ``step()`` calls leave them -- the queues extended with the
        finished episodes in the order the calls would have found them, ONE read-back per rollout where ``step()`` has one per step.  The
        returned dict has the keys the caller asked for: ``"infos"`` (with ``episode`` / ``_episode`` under the wrapper's key) with
        ``infos=True``, the bare trajectory otherwise, as before."""
        wanted = bool(kwargs.get("infos", False))
        kwargs["infos"] = True
        out = dict(self.env.rollout(num_steps, actions, **kwargs))
        infos = dict(out.pop("infos"))
        found = self._rename(infos)
        if found is not None:
            self._extend_queues(*found)
        if wanted:
            out["infos"] = infos
        return out


# -- the reference's per-sub-environment action wrappers (gymnasium/wrappers/stateful_action.py), run by the engine's step itself ---------------------
_InvalidProbability = getattr(error, "InvalidProbability", error.Error)
_InvalidBound = getattr(error, "InvalidBound", error.Error)


def _bare_env(env, what):
    """``env`` if it is a HipVectorEnv with nothing around it; error.Error otherwise."""
    if isinstance(env, VectorWrapper) or not hasattr(env, "set_step_wrappers"):
        raise error.Error(f"{what} wraps every SUB-environment, below the vector level: it goes directly over the HipVectorEnv "
                          f"(gymnasium_amd.make_vec(...) of a classic-control or MuJoCo id), and the vector wrappers go above it; got {type(env).__name__}")
    return env


class RepeatAction(VectorWrapper):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.RepeatAction(env, num_repeats)`` (stateful_action.py:145-220; the
    reference has no vector version): a ``step()`` runs up to ``num_repeats`` inner steps of every sub-environment with the same action IN ONE
    LAUNCH -- a sub-environment stops after the inner step that terminates or truncates it (TimeLimit counts inner steps) while its neighbours
    go on --, returns the last inner observation and ``0.0 + r1 + r2 ...``.  Episode statistics count what the vector level sees: one step
    per ``step()``.  The NEXT_STEP autoreset step repeats nothing.  Goes directly over the env of the five classic-control ids or the eleven
    MuJoCo v5 ids; ``StickyAction`` may go over it, every vector wrapper goes above both.  ``step``, ``step(None)``, ``rollout`` and ``capture_steps``
    all follow.  Over a MuJoCo id a ``step()`` is a series of launches on the env's stream instead of one -- an opening kernel, then ``num_repeats``
    trips of the plain step's launches, nothing synchronised in between (docs/mujoco_design.md) --, a finished sub-environment sits the remaining
    trips out, and the observation and the info entries (``x_position``, ``reward_ctrl``, ...; ``final_info`` under SAME_STEP) are the last executed
    inner step's."""

    def __init__(self, env, num_repeats: int):
        if not np.issubdtype(type(num_repeats), np.integer):
            raise TypeError(f"The num_repeats is expected to be an integer, actual type: {type(num_repeats)}")
        if num_repeats < 1:
            raise ValueError(f"The num_repeats value needs to be equal or greater than one, actual value: {num_repeats}")
        if isinstance(env, MaxAndSkipObservation):
            raise error.Error("RepeatAction over MaxAndSkipObservation: MaxAndSkipObservation repeats the action itself -- fold the repeat into its "
                              f"`skip` (MaxAndSkipObservation(env, {int(env.skip) * int(num_repeats)}) runs as many inner steps)")
        base = _bare_env(env, "RepeatAction")
        if base._step_wrappers != (0, 0.0, 0):
            raise error.Error("this env already runs RepeatAction / StickyAction: switch them off first (env.set_step_wrappers())")
        super().__init__(env)
        base.set_step_wrappers(int(num_repeats), 0.0, 0)
        _close_fusion(env)
        self.num_repeats = num_repeats


class MaxAndSkipObservation(VectorWrapper):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.MaxAndSkipObservation(env, skip)`` (stateful_observation.py:564-649;
    the reference has no vector version): a ``step()`` runs up to ``skip`` inner steps of every sub-environment with the same action IN ONE
    LAUNCH, as ``RepeatAction`` does (TimeLimit counts inner steps, the reward is ``0.0 + r0 + r1 ...``, episode statistics count one step per
    ``step()``), and returns the element-wise maximum of the sub-environment's two frames: frame 0 is written after inner step ``skip - 2``, frame 1
    after inner step ``skip - 1``.  The frames start as zeros and are NEVER cleared -- not by ``reset()``, a masked reset, an autoreset or
    ``set_state()`` -- so a step whose episode ended before it wrote a frame returns the maximum over what an earlier step, possibly of an earlier
    episode, left there (``env.max_and_skip_frames()`` shows them).  Which zero comes out of ``+0`` and ``-0`` is not pinned (NumPy's reduction
    does not promise one).  The NEXT_STEP autoreset step returns the plain reset observation; under SAME_STEP ``final_obs`` is the max frame.
    Goes directly over the env of the five classic-control ids; ``StickyAction`` may go over it, ``RepeatAction`` neither over nor under it (fold
    the repeat into ``skip``); the ``per_env`` wrappers, the Discretize wrappers and every vector wrapper go above.  ``step``, ``step(None)``,
    ``rollout`` and ``capture_steps`` all follow."""

    def __init__(self, env, skip: int = 4):
        if not np.issubdtype(type(skip), np.integer):
            raise TypeError(f"The skip is expected to be an integer, actual type: {type(skip)}")
        if skip < 2:
            raise ValueError(f"The skip value needs to be equal or greater than two, actual value: {skip}")
        if isinstance(env, RepeatAction):
            raise error.Error("MaxAndSkipObservation over RepeatAction: MaxAndSkipObservation repeats the action itself -- fold the repeat into "
                              f"`skip` (MaxAndSkipObservation(env, {int(skip) * int(env.num_repeats)}) over the bare env runs as many inner steps)")
        base = _bare_env(env, "MaxAndSkipObservation")
        if not hasattr(base, "set_max_and_skip"):
            raise error.Error(f"{type(base).__name__} has no MaxAndSkipObservation of the sub-environments (mi_set_max_and_skip)")
        if base._step_wrappers != (0, 0.0, 0) or base._max_and_skip:
            raise error.Error("this env already runs RepeatAction / StickyAction / MaxAndSkipObservation: switch them off first "
                              "(env.set_step_wrappers(), env.set_max_and_skip()); a repeat is folded into `skip`")
        super().__init__(env)
        base.set_max_and_skip(int(skip))
        _close_fusion(env)
        self.skip = skip


class StickyAction(VectorWrapper):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.StickyAction(env, repeat_action_probability,
    repeat_action_duration)`` (stateful_action.py:16-142, Machado et al. 2018; the reference has no vector version).  Before a step, a
    sub-environment that has a last action and is not inside a series draws ``np_random.uniform()`` from ITS OWN generator (the one its resets
    consume: ``get_rng_state()`` shows it) and with that probability repeats its last action for ``repeat_action_duration`` steps; every reset
    of a sub-environment clears its state.  Goes directly over the env of the five classic-control ids or over ``RepeatAction`` /
    ``MaxAndSkipObservation`` (one decision per outer step); every vector wrapper goes above.  Two deliberate differences: actions are validated as given (the reference never looks at an
    action that a sticky one replaces), and the element type of the action batch (float32 / float64 rows) must not change between steps.
    ``repeat_action_duration`` is an int: a (low, high) range is drawn by ``Generator.integers`` from PCG64's buffered 32-bit half, which the
    sub-environments' generators on the device do not carry -- refused, not approximated.
    Over the eleven MuJoCo v5 ids likewise (directly over the env or over ``RepeatAction``): the decision is taken by a small kernel that opens the
    step, before anything else the sub-environment's generator does in it; the MuJoCo kinds validate no action.  The engine keeps a COPY of every
    sub-environment's last action row; the reference keeps a view of the caller's batch, so overwriting that batch in place between steps changes the
    reference's sticky action and not this one's."""

    def __init__(self, env, repeat_action_probability: float, repeat_action_duration=1):
        if not 0 <= repeat_action_probability < 1:
            raise _InvalidProbability(f"`repeat_action_probability` should be in the interval [0,1). Received {repeat_action_probability}")
        rng = (repeat_action_duration, repeat_action_duration) if isinstance(repeat_action_duration, int) else repeat_action_duration
        if not isinstance(rng, tuple):
            raise ValueError(f"`repeat_action_duration` should be either an integer or a tuple. Received {rng}")
        if len(rng) != 2:
            raise ValueError(f"`repeat_action_duration` should be a tuple or a list of two integers. Received {rng}")
        if rng[0] > rng[1]:
            raise _InvalidBound(f"`repeat_action_duration` is not a valid bound. Received {rng}")
        if np.any(np.array(rng) < 1):
            raise ValueError(f"`repeat_action_duration` should be larger or equal than 1. Received {rng}")
        if rng[0] != rng[1]:
            raise error.Error(f"`repeat_action_duration` = {rng}: a range is drawn with Generator.integers, which takes PCG64's buffered 32-bit half; the "
                              "sub-environments' generators on the device do not carry that half, so only an int duration is supported")
        inner = env
        repeats = 0
        if isinstance(env, RepeatAction):
            inner, repeats = env.env, int(env.num_repeats)
        elif isinstance(env, MaxAndSkipObservation):  # (one decision per outer step, as over RepeatAction; the engine keeps the skip apart)
            inner = env.env
        base = _bare_env(inner, "StickyAction")
        if base._step_wrappers != (repeats, 0.0, 0):
            raise error.Error("this env already runs StickyAction (RepeatAction goes UNDER StickyAction, never over it): switch them off first "
                              "(env.set_step_wrappers())")
        super().__init__(env)
        base.set_step_wrappers(repeats, float(repeat_action_probability), int(rng[0]))
        _close_fusion(env)
        self.repeat_action_probability = repeat_action_probability
        self.repeat_action_duration_range = rng


class NumpyToTorch(VectorWrapper):
    """gymnasium.wrappers.vector.NumpyToTorch (wrappers/vector/numpy_to_torch.py:16-53) without the conversion: the wrapped HipVectorEnv is
    switched to ``output="torch"``, so observations, rewards and flags ARE torch tensors the engine wrote in HBM (zero copy; the reference
    wrapper converts NumPy batches with ``torch.from_numpy`` / DLPack after the fact) and actions may be device tensors.  ``device``: where
    the caller wants the tensors -- None or the env's own GPU costs nothing, anything else (e.g. "cpu") is one ``.to(device)`` per array.
    The arrays inside ``infos`` become tensors as well, like the reference's recursive conversion."""

    _transparent = True

    def __init__(self, env, device=None):
        super().__init__(env)
        if not hasattr(env.unwrapped, "set_output"):
            raise TypeError("NumpyToTorch of gymnasium_amd wraps a HipVectorEnv (use gymnasium's own wrapper for other vector envs)")
        env.unwrapped.set_output("torch")
        self.device = device

    def _move(self, x):
        torch = _torch()
        if isinstance(x, dict):
            return {k: self._move(v) for k, v in x.items()}
        if isinstance(x, np.ndarray):
            if x.dtype == object:  # final_obs under SAME_STEP: a ragged object array stays as it is
                return x
            x = torch.from_numpy(x)
            return x.to(self.device if self.device is not None else f"cuda:{self._dev()}")
        if isinstance(x, torch.Tensor) and self.device is not None and x.device != torch.device(self.device):
            return x.to(self.device)
        return x

    def reset(self, *, seed=None, options=None):
        obs, infos = self.env.reset(seed=seed, options=options)
        return self._move(obs), self._move(infos)

    def step(self, actions):
        obs, rewards, terminations, truncations, infos = self.env.step(actions)
        return self._move(obs), self._move(rewards), self._move(terminations), self._move(truncations), self._move(infos)

    def rollout(self, num_steps, actions=None, **kwargs):
        return self._move(self.env.rollout(num_steps, actions, **kwargs))


class NormalizeObservation(VectorWrapper):
    """stateful_observation.py:27-160."""

    def __init__(self, env, epsilon: float = 1e-8):
        if epsilon <= 0:
            raise error.InvalidBound(f"`epsilon` should be strictly positive. Received {epsilon}")
        super().__init__(env)
        if self.env.metadata.get("autoreset_mode", AutoresetMode.NEXT_STEP) not in {AutoresetMode.NEXT_STEP}:
            raise ValueError(f"Expected env.metadata['autoreset_mode'] to be AutoresetMode.NEXT_STEP, got {self.env.metadata['autoreset_mode']}")
        shape = self.env.single_observation_space.shape
        self.single_observation_space = spaces.Box(low=-np.inf, high=np.inf, shape=shape, dtype=np.float32)
        self.observation_space = batch_space(self.single_observation_space, self.env.num_envs)
        in_dtype = np.dtype(self.env.single_observation_space.dtype)
        if in_dtype not in (np.float32, np.float64):
            raise ValueError(f"NormalizeObservation needs float32 / float64 observations, got {in_dtype}")
        # RunningMeanStd(dtype=float32) in the reference; float64 observations promote the statistics to float64 on the first update
        self.obs_rms = RunningMeanStd(shape=shape, dtype=np.float32 if in_dtype == np.float32 else np.float64, device=self._dev())
        self._in_code = _native.MI_F32 if in_dtype == np.float32 else _native.MI_F64
        self.epsilon = epsilon
        self._update_running_mean = True
        base = _fusion_base(self.env)
        if base is not None and in_dtype == np.float32 and base._fusion_state()["obs"] is None:
            self._fused, self._base = True, base
            self._fuse_index = base._fuse(self, "obs")
        else:
            _close_fusion(self.env)

    @property
    def update_running_mean(self) -> bool:
        return self._update_running_mean

    @update_running_mean.setter
    def update_running_mean(self, setting: bool):
        self._update_running_mean = setting

    def observations(self, observations):
        torch = _torch()
        x, was_tensor = self._to_device(observations)
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        lib = self.obs_rms._lib
        lib.check(lib.normalize_observation(self.obs_rms._h, _stream(), C.c_void_p(x.data_ptr()), self._in_code, int(x.shape[0]),
                                            float(self.epsilon), int(self._update_running_mean), C.c_void_p(out.data_ptr())))
        return self._back(out, was_tensor)

    def reset(self, *, seed=None, options=None):
        if options is not None and "reset_mask" in options and not np.all(options["reset_mask"]):
            raise ValueError("NormalizeObservation does not support partial resets. The 'reset_mask' must contain all True values.")
        obs, info = self.env.reset(seed=seed, options=options)
        return self.observations(obs), info

    def step(self, actions):
        if self._fused:  # the step kernel's output stage normalises (and updates obs_rms)
            return self._step_fused(actions)
        obs, reward, terminated, truncated, info = self.env.step(actions)
        return self.observations(obs), reward, terminated, truncated, info

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()``: obs_rms is updated from step t's batch, then step t is normalised with it (stateful_observation.py:144-160), for
        all t in four launches.  float32 trajectories are normalised in place (the tensor is the rollout's own, nobody else holds it)."""
        torch = _torch()
        out = dict(self.env.rollout(num_steps, actions, **kwargs))
        x = out["obs"].contiguous()
        steps, rows = int(x.shape[0]), int(x.shape[1])
        res = x if x.dtype == torch.float32 else torch.empty(x.shape, dtype=torch.float32, device=x.device)
        ws, size = self._workspace(steps, rows, self.obs_rms.dim)
        lib = self.obs_rms._lib
        lib.check(lib.normalize_observation_steps(self.obs_rms._h, _stream(), C.c_void_p(x.data_ptr()), self._in_code, steps, rows, float(self.epsilon),
                                                  int(self._update_running_mean), C.c_void_p(res.data_ptr()), C.c_void_p(ws.data_ptr()), size))
        out["obs"] = res
        return out


class NormalizeReward(VectorWrapper):
    """stateful_reward.py:21-183."""

    def __init__(self, env, gamma: float = 0.99, epsilon: float = 1e-8):
        if not 0 <= gamma <= 1:
            raise error.InvalidBound(f"`gamma` should be in the interval [0, 1]. Received {gamma}")
        if epsilon <= 0:
            raise error.InvalidBound(f"`epsilon` should be strictly positive. Received {epsilon}")
        super().__init__(env)
        torch = _torch()
        dev = f"cuda:{self._dev()}"
        self.return_rms = RunningMeanStd(shape=(), device=self._dev())
        self._acc = torch.zeros(self.env.num_envs, dtype=torch.float32, device=dev)
        self._prev = torch.zeros(self.env.num_envs, dtype=torch.uint8, device=dev)
        self.gamma, self.epsilon = gamma, epsilon
        self._update_running_mean = True
        self._autoreset_mode = self.env.metadata.get("autoreset_mode", AutoresetMode.NEXT_STEP)
        base = _fusion_base(self.env)
        st = None if base is None else base._fusion_state()
        if st is not None and st["ret"] is None and st["clip_post"] is None:  # order inside the epilogue: clip_pre -> normalise -> clip_post
            self._fused, self._base = True, base
            self._fuse_index = base._fuse(self, "ret")
        else:
            _close_fusion(self.env)

    @property
    def accumulated_reward(self):
        return self._acc.cpu().numpy()

    @property
    def update_running_mean(self) -> bool:
        return self._update_running_mean

    @update_running_mean.setter
    def update_running_mean(self, setting: bool):
        self._update_running_mean = setting

    def reset(self, *, seed=None, options=None):
        self._acc.zero_(), self._prev.zero_()
        return self.env.reset(seed=seed, options=options)

    def step(self, actions):
        if self._fused:
            return self._step_fused(actions)
        torch = _torch()
        obs, reward, terminated, truncated, info = self.env.step(actions)
        r, was_tensor = self._to_device(reward, np.float64)
        te, _ = self._to_device(terminated)
        tr, _ = self._to_device(truncated)
        te8, tr8 = te.view(torch.uint8) if te.dtype == torch.bool else te, tr.view(torch.uint8) if tr.dtype == torch.bool else tr
        out = torch.empty_like(r)
        lib = self.return_rms._lib
        lib.check(lib.normalize_reward(self.return_rms._h, _stream(), C.c_void_p(self._acc.data_ptr()), C.c_void_p(self._prev.data_ptr()),
                                       C.c_void_p(r.data_ptr()), C.c_void_p(te8.data_ptr()), C.c_void_p(tr8.data_ptr()), int(r.shape[0]),
                                       float(self.gamma), float(self.epsilon), int(self._autoreset_mode == AutoresetMode.SAME_STEP),
                                       int(self._update_running_mean), C.c_void_p(out.data_ptr())))
        return obs, self._back(out, was_tensor), terminated, truncated, info

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` (stateful_reward.py:150-176): one walk over t per sub-environment for the discounted returns and the previous-done
        flags, return_rms updated step by step from them, every reward divided by the deviation after its own step.  In place."""
        torch = _torch()
        out = dict(self.env.rollout(num_steps, actions, **kwargs))
        r = out["rewards"].to(torch.float64).contiguous()
        te, tr = out["terminations"].contiguous(), out["truncations"].contiguous()
        te8, tr8 = te.view(torch.uint8) if te.dtype == torch.bool else te, tr.view(torch.uint8) if tr.dtype == torch.bool else tr
        steps, rows = int(r.shape[0]), int(r.shape[1])
        ws, size = self._workspace(steps, rows, 1)
        lib = self.return_rms._lib
        lib.check(lib.normalize_reward_steps(self.return_rms._h, _stream(), C.c_void_p(self._acc.data_ptr()), C.c_void_p(self._prev.data_ptr()),
                                             C.c_void_p(r.data_ptr()), C.c_void_p(te8.data_ptr()), C.c_void_p(tr8.data_ptr()), steps, rows,
                                             float(self.gamma), float(self.epsilon), int(self._autoreset_mode == AutoresetMode.SAME_STEP),
                                             int(self._update_running_mean), C.c_void_p(r.data_ptr()), C.c_void_p(ws.data_ptr()), size))
        out["rewards"] = r
        return out


class ClipReward(VectorWrapper):
    """vectorize_reward.py:115-151 (transform_reward.ClipReward: np.clip(reward, min_reward, max_reward))."""

    def __init__(self, env, min_reward=None, max_reward=None):
        if min_reward is None and max_reward is None:
            raise error.InvalidBound("Both `min_reward` and `max_reward` cannot be None")
        if min_reward is not None and max_reward is not None and np.any(max_reward - min_reward < 0):
            raise error.InvalidBound(f"Min reward ({min_reward}) must be smaller than max reward ({max_reward})")
        super().__init__(env)
        self.min_reward, self.max_reward = min_reward, max_reward
        self._lib = _native.load_library()
        base = _fusion_base(self.env)
        st = None if base is None else base._fusion_state()
        scalar = all(b is None or np.ndim(b) == 0 for b in (min_reward, max_reward))
        slot = None
        if st is not None and scalar:
            if st["ret"] is None and st["clip_pre"] is None and st["clip_post"] is None:
                slot = "clip_pre"
            elif st["clip_post"] is None:
                slot = "clip_post"
        if slot is not None:
            self._fused, self._base = True, base
            self._fuse_index = base._fuse(self, slot)
        else:
            _close_fusion(self.env)

    def step(self, actions):
        if self._fused:
            return self._step_fused(actions)
        torch = _torch()
        obs, reward, terminated, truncated, info = self.env.step(actions)
        r, was_tensor = self._to_device(reward, np.float64)
        out = torch.empty_like(r)
        lo = None if self.min_reward is None else C.c_double(float(self.min_reward))
        hi = None if self.max_reward is None else C.c_double(float(self.max_reward))
        self._lib.check(self._lib.clip_reward(self._dev(), _stream(), C.c_void_p(r.data_ptr()), int(r.shape[0]),
                                              None if lo is None else C.cast(C.byref(lo), C.c_void_p), None if hi is None else C.cast(C.byref(hi), C.c_void_p),
                                              C.c_void_p(out.data_ptr())))
        return obs, self._back(out, was_tensor), terminated, truncated, info

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()``: np.clip over the T * N rewards of the trajectory, in place."""
        torch = _torch()
        out = dict(self.env.rollout(num_steps, actions, **kwargs))
        r = out["rewards"].to(torch.float64).contiguous()
        lo = None if self.min_reward is None else C.c_double(float(self.min_reward))
        hi = None if self.max_reward is None else C.c_double(float(self.max_reward))
        self._lib.check(self._lib.clip_reward(self._dev(), _stream(), C.c_void_p(r.data_ptr()), int(r.numel()),
                                              None if lo is None else C.cast(C.byref(lo), C.c_void_p), None if hi is None else C.cast(C.byref(hi), C.c_void_p),
                                              C.c_void_p(r.data_ptr())))
        out["rewards"] = r
        return out


# -- action wrappers --------------------------------------------------------------------------------------------------------------------------
class VectorActionWrapper(VectorWrapper):
    """gymnasium.vector.VectorActionWrapper (vector_env.py:520-552): ``step(a)`` is ``env.step(self.actions(a))``.  Observations and rewards pass
    through unchanged, so a fused NormalizeObservation / NormalizeReward / ClipReward unit may extend across it.  ``rollout`` and
    ``capture_steps`` apply the same transform; everything else forwards, as in the reference."""

    _transparent = True

    def actions(self, actions):
        raise NotImplementedError

    def step(self, actions):
        return self.env.step(self.actions(actions))

    def _actions_of_steps(self, block, steps):
        """``actions()`` of every step of a ``[T, N, ...]`` block, stacked."""
        torch = _torch()
        rows = [self.actions(block[t]) for t in range(steps)]
        return torch.stack(rows) if isinstance(rows[0], torch.Tensor) else np.stack(rows)

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` through this wrapper.  ``actions`` (``[T, N, A]``) are transformed in one pass and handed to the wrapped ``rollout``;
        with ``actions=None`` the T batches are ``self.action_space.sample()`` -- host draws from the WRAPPER's space, stacked and uploaded -- so
        the result equals ``[w.step(w.action_space.sample()) for _ in range(T)]``.  ``"actions"`` of the returned dict holds the batches as this
        wrapper received or drew them (a device tensor, untransformed)."""
        torch = _torch()
        steps = int(num_steps)
        if steps < 1:
            return self.env.rollout(num_steps, actions, **kwargs)
        if actions is None:
            draws = [self.action_space.sample() for _ in range(steps)]
            actions = torch.stack(draws) if isinstance(draws[0], torch.Tensor) else np.stack(draws)
        sent = self._actions_of_steps(actions, steps)
        out = dict(self.env.rollout(num_steps, sent if isinstance(sent, torch.Tensor) else torch.from_numpy(sent), **kwargs))
        if "actions" in out:
            out["actions"] = (actions if isinstance(actions, torch.Tensor) else torch.from_numpy(np.asarray(actions))).to(out["obs"].device)
        return out

    def _before_capture(self):
        """Whatever must have run once before a graph capture opens (a capture must not load a kernel)."""

    def capture_steps(self, actions=None, steps: int = 1, policy=None):
        """HipVectorEnv.capture_steps with this wrapper's transform captured between the policy and the step: ``actions`` (a device tensor read at
        replay time) or a callable ``policy``.  ``policy="random"`` is refused: the wrapper's space is sampled on the host."""
        if isinstance(policy, str):
            raise error.Error(f"capture_steps(policy={policy!r}) through {type(self).__name__}: the wrapper's action space is not sampled on the device; "
                              "capture a callable policy, or the wrapped env's own steps")
        if (actions is None) == (policy is None):
            raise ValueError("capture_steps() takes either `actions` (a device tensor read at replay time) or `policy` (a callable)")
        if actions is not None and not (hasattr(actions, "is_cuda") and actions.is_cuda):
            raise ValueError("the captured steps read `actions` at replay time: pass a tensor on the env's device")
        self._before_capture()
        inner = (lambda obs: self.actions(actions)) if policy is None else (lambda obs: self.actions(policy(obs)))
        return self.env.capture_steps(steps=steps, policy=inner)


class TransformAction(VectorActionWrapper):
    """vectorize_action.py:30-110: ``func`` is applied to the batch as given -- a NumPy array or a device tensor goes in, the same kind must come
    out (a ``func`` of operators and ``torch`` / NumPy ufuncs serves both)."""

    def __init__(self, env, func, action_space=None, single_action_space=None):
        super().__init__(env)
        if action_space is None:
            if single_action_space is not None:
                self.single_action_space = single_action_space
                self.action_space = batch_space(single_action_space, self.num_envs)
        else:
            self.action_space = action_space
            if single_action_space is not None:
                self.single_action_space = single_action_space
        if self.action_space != batch_space(self.single_action_space, self.num_envs):
            from ..gym_api import logger

            logger.warn(f"For {env}, the action space and the batched single action space don't match as expected, action_space={env.action_space}, "
                        f"batched single_action_space={batch_space(self.single_action_space, self.num_envs)}")
        self.func = func

    def actions(self, actions):
        return self.func(actions)


def _rescale_box(box, new_min, new_max):
    """wrappers/utils.py:160-266 ``rescale_box``: (the rescaled Box, gradient, intercept), the two arrays in the box's dtype.  Every expression is
    the reference's own NumPy expression in its dtype -- the bound difference in np.float128 where the platform has it -- because the float32
    rounding of ``gradient`` and ``intercept`` is what the device then computes with."""
    if not isinstance(box, spaces.Box):
        raise TypeError(f"Expected box to be a Box space, got {type(box)}")
    bounds = []
    for name, b in (("new_min", new_min), ("new_max", new_max)):
        if not isinstance(b, np.ndarray):
            if not (np.issubdtype(type(b), np.integer) or np.issubdtype(type(b), np.floating)):
                raise TypeError(f"Expected {name} to be an integer, float, or numpy array, got {type(b)}")
            b = np.full(box.shape, b)
        if b.shape != box.shape:
            raise ValueError(f"Expected {name}.shape to be {box.shape}, got {b.shape}")
        bounds.append(b)
    new_min, new_max = bounds
    for new, old in ((new_min, box.low), (new_max, box.high)):
        if not np.all((new == old)[np.isinf(new) | np.isinf(old)]):
            raise ValueError("For unbounded components, the target bounds must match the original infinity bounds.")
    if not np.all(new_min <= new_max):
        raise ValueError(f"Expected new_min to be less than or equal to new_max, got {new_min} and {new_max}")
    if not np.all(box.low <= box.high):
        raise ValueError(f"Expected box.low to be less than or equal to box.high, got {box.low} and {box.high}")
    wide = getattr(np, "float128", np.float64)
    min_finite, max_finite = np.isfinite(new_min), np.isfinite(new_max)
    both = min_finite & max_finite
    gradient = np.ones_like(new_min, dtype=box.dtype)
    gradient[both] = (new_max[both] - new_min[both]) / (np.array(box.high[both], dtype=wide) - np.array(box.low[both], dtype=wide))
    intercept = np.zeros_like(new_min, dtype=box.dtype)
    intercept[max_finite] = new_max[max_finite] - box.high[max_finite]
    intercept[min_finite] = gradient[min_finite] * -box.low[min_finite] + new_min[min_finite]  # (where both are finite this one stands)
    return spaces.Box(low=new_min, high=new_max, shape=box.shape, dtype=box.dtype), gradient, intercept


class _BoxTransformAction(VectorActionWrapper):
    """What ClipAction and RescaleAction share (vectorize_action.py:114-213, VectorizeTransformAction): the reference applies the scalar wrapper's
    ``func`` row by row and stacks the rows into a float32 ``(N, A)`` array -- or, when the wrapper's batched space equals the env's
    (``same_out``), into the caller's own array, whose dtype the result then keeps.  Here the rows are transformed at once, in the dtype NumPy's
    promotion gives a row against the float32 parameters (float32 for float32 / float16 rows, float64 for float64 and integer rows), and
    rounded once to the dtype they are stored in:

    * NumPy arrays, lists, host tensors: one vectorised NumPy expression; the env receives a NumPy batch.
    * device tensors: mi_transform_actions (csrc/action_wrappers.hip), one launch over the N * A -- in ``rollout`` the T * N * A -- elements.

    DEVIATION from the reference: the caller's array or tensor is never modified (``same_out`` writes into it there); the result is always a
    new one."""

    _kind = None

    def _setup(self, single_space, p0, p1):
        self.single_action_space = single_space
        self.action_space = batch_space(single_space, self.num_envs)
        self.same_out = self.action_space == self.env.action_space
        self._shape = tuple(self.env.single_action_space.shape)
        self._p0, self._p1 = p0, p1
        self._q0 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1)
        self._q1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1)

    def _formula(self, a):
        raise NotImplementedError

    def actions(self, actions):
        return self._apply(actions, (self.num_envs,))

    def _actions_of_steps(self, block, steps):
        return self._apply(block, (steps, self.num_envs))

    def _apply(self, actions, lead):
        if hasattr(actions, "data_ptr"):
            if actions.is_cuda:
                return self._apply_device(actions, lead)
            actions = actions.numpy()
        if self.same_out and not isinstance(actions, np.ndarray):
            raise TypeError(f"{type(self).__name__}: its action space equals the env's, so the result keeps the dtype of the caller's array: pass a NumPy "
                            f"array, not {type(actions)}")
        if len(lead) == 1 and isinstance(actions, (list, tuple)) and len(actions) > 0 and all(type(x) in (float, int) for x in actions):
            a = np.asarray(actions, dtype=np.float32)  # a row that is one Python scalar is weak against the float32 parameters (NEP 50)
        else:
            a = np.asarray(actions)
        if a.ndim == 0:
            raise TypeError(f"Unable to iterate over the actions of the batched space, got {actions!r}")
        if a.ndim == len(lead):
            a = a[..., None]
        res = self._formula(a)
        if res.shape != lead + self._shape:
            raise ValueError(f"actions must give rows of shape {self._shape} for {lead}, got an array of shape {np.shape(actions)}")
        out_dtype = a.dtype if self.same_out else np.dtype(np.float32)
        if not np.can_cast(res.dtype, out_dtype, "same_kind"):
            raise TypeError(f"Cannot cast the transformed actions from {res.dtype} to {out_dtype} according to the rule 'same_kind'")
        return res.astype(out_dtype)

    def _apply_device(self, x, lead):
        torch = _torch()
        dim = int(np.prod(self._shape))
        if dim > _native.TRANSFORM_MAX_ACT_DIM:
            raise error.Error(f"{type(self).__name__} on device tensors takes up to {_native.TRANSFORM_MAX_ACT_DIM} action dimensions, the env has {dim}")
        kept = x.dtype
        if self.same_out and not kept.is_floating_point:
            raise TypeError(f"Cannot cast the transformed actions to {kept} according to the rule 'same_kind'")
        compute = torch.float64 if kept in (torch.float64, torch.int32, torch.int64) else torch.float32
        if x.dim() == len(lead):
            x = x.unsqueeze(-1)
        want = lead + self._shape
        if tuple(x.shape) != want:
            try:
                ok = tuple(torch.broadcast_shapes(tuple(x.shape), self._shape)) == want
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError(f"actions must give rows of shape {self._shape} for {lead}, got a tensor of shape {tuple(x.shape)}")
            x = x.expand(want)
        x = x.to(compute).contiguous()
        out = torch.empty(want, dtype=compute if self.same_out else torch.float32, device=x.device)
        lib = _native.load_library()
        code = {torch.float32: _native.MI_F32, torch.float64: _native.MI_F64}
        lib.check(lib.transform_actions(x.device.index, C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream), C.c_void_p(x.data_ptr()),
                                        code[x.dtype], C.c_void_p(out.data_ptr()), code[out.dtype], x.numel(), dim, self._kind,
                                        self._q0.ctypes.data, self._q1.ctypes.data))
        return out.to(kept) if self.same_out and out.dtype != kept else out

    def _before_capture(self):
        torch = _torch()
        for dtype in (torch.float32, torch.float64):
            self._apply_device(torch.zeros((1,) + self._shape, dtype=dtype, device=f"cuda:{self._dev()}"), (1,))


class ClipAction(_BoxTransformAction):
    """vectorize_action.py:216-240 (transform_action.py:79-127): ``np.clip(action, low, high)`` with the env's bounds; the wrapper's own space is
    unbounded.  NaN stays NaN; a float64 batch is clipped in float64 and then rounded to float32."""

    _kind = _native.TRANSFORM_CLIP

    def __init__(self, env):
        super().__init__(env)
        box = self.env.single_action_space
        if not isinstance(box, spaces.Box):
            raise TypeError(f"ClipAction requires a Box action space, got {type(box)}")
        self._setup(spaces.Box(-np.inf, np.inf, shape=box.shape, dtype=box.dtype), box.low, box.high)

    def _formula(self, a):
        # NOT np.clip over the batch: with the bounds broadcast NumPy takes its constant-bounds loop, `x < lo ? lo : x`, which keeps the -0.0 that
        # the loop a single row goes through, `x > lo ? x : lo`, turns into the bound +0.0.  The row loop is what the reference runs.
        c = np.result_type(a.dtype, self._p0.dtype)
        x, lo, hi = a.astype(c), self._p0.astype(c), self._p1.astype(c)
        t = np.where((x > lo) | np.isnan(x), x, lo)
        return np.where((t < hi) | np.isnan(t), t, hi)


class RescaleAction(_BoxTransformAction):
    """vectorize_action.py:243-296 (transform_action.py:130-198): the wrapper's space is ``[min_action, max_action]``, the env receives
    ``(action - intercept) / gradient``.  ``gradient`` and ``intercept`` are rescale_box's float32 arrays, computed on the host."""

    _kind = _native.TRANSFORM_AFFINE_INVERSE

    def __init__(self, env, min_action, max_action):
        super().__init__(env)
        box = self.env.single_action_space
        if not isinstance(box, spaces.Box):
            raise TypeError(f"RescaleAction requires a Box action space, got {type(box)}")
        space, self.gradient, self.intercept = _rescale_box(box, min_action, max_action)
        if np.any(space.low == space.high):
            raise error.InvalidBound(f"Min action ({min_action}) must be strictly smaller than max action ({max_action}), the rescaling has no inverse "
                                     "where they are equal")
        self._setup(space, self.intercept, self.gradient)

    def _formula(self, a):
        return (a - self.intercept) / self.gradient


# -- observation and reward transforms --------------------------------------------------------------------------------------------------------
def _refuse_capture(wrapper, what):
    raise error.Error(f"capture_steps() through {type(wrapper).__name__} is not supported: the captured steps return the wrapped env's own buffers, so a "
                      f"replay would hand out the untransformed {what}; capture the wrapped env's steps and apply the transform to what replay() returns")


def _stack(rows):
    torch = _torch()
    if isinstance(rows[0], tuple):
        return tuple(_stack([r[k] for r in rows]) for k in range(len(rows[0])))
    return torch.stack(rows) if isinstance(rows[0], torch.Tensor) else np.stack(rows)


class VectorObservationWrapper(VectorWrapper):
    """gymnasium.vector.VectorObservationWrapper (vector_env.py:520-575): ``reset`` and ``step`` return ``self.observations(obs)`` in place of
    ``obs``; everything else forwards.  SAME_STEP is refused as in the reference, so ``final_obs`` never needs transforming.  ``rollout`` transforms
    the trajectory's ``"obs"``; ``capture_steps`` is refused (the captured results would be the untransformed buffers).  Neither transparent nor fused:
    statistics wrappers stacked above run their stand-alone passes over the transformed observations."""

    def __init__(self, env):
        super().__init__(env)
        if "autoreset_mode" not in self.env.metadata:
            from ..gym_api import logger

            logger.warn(f"Vector environment ({env}) is missing `autoreset_mode` metadata key.")
        elif self.env.metadata["autoreset_mode"] not in (AutoresetMode.NEXT_STEP, AutoresetMode.DISABLED):
            raise ValueError(f"Expected autoreset_mode to be NEXT_STEP or DISABLED, got {self.env.metadata['autoreset_mode']}")
        _close_fusion(self.env)

    def observations(self, observations):
        raise NotImplementedError

    def reset(self, *, seed=None, options=None):
        obs, infos = self.env.reset(seed=seed, options=options)
        return self.observations(obs), infos

    def step(self, actions):
        obs, rewards, terminations, truncations, infos = self.env.step(actions)
        return self.observations(obs), rewards, terminations, truncations, infos

    def _observations_of_steps(self, block, steps):
        """``observations()`` of every step of a ``[T, N, ...]`` block, stacked."""
        return _stack([self.observations(block[t]) for t in range(steps)])

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` through this wrapper: the wrapped ``rollout`` with ``"obs"`` transformed; the other keys (``infos=True`` included) pass through."""
        out = dict(self.env.rollout(num_steps, actions, **kwargs))
        steps = len(out["obs"][0]) if isinstance(out["obs"], tuple) else int(out["obs"].shape[0])
        if steps > 0:
            out["obs"] = self._observations_of_steps(out["obs"], steps)
        return out

    def capture_steps(self, *args, **kwargs):
        _refuse_capture(self, "observations")


class TransformObservation(VectorObservationWrapper):
    """vectorize_observation.py:32-111: ``func`` is applied to the batch as given -- a NumPy array or a device tensor goes in, the same kind must come
    out.  ``rollout`` applies it step by step (a ``func`` may look at the batch's shape)."""

    def __init__(self, env, func, observation_space=None, single_observation_space=None):
        super().__init__(env)
        if observation_space is None:
            if single_observation_space is not None:
                self.single_observation_space = single_observation_space
                self.observation_space = batch_space(single_observation_space, self.num_envs)
        else:
            self.observation_space = observation_space
            if single_observation_space is not None:
                self.single_observation_space = single_observation_space
        if self.observation_space != batch_space(self.single_observation_space, self.num_envs):
            from ..gym_api import logger

            logger.warn(f"For {env}, the observation space and the batched single observation space don't match as expected, "
                        f"observation_space={env.observation_space}, batched single_observation_space={batch_space(self.single_observation_space, self.num_envs)}")
        self.func = func

    def observations(self, observations):
        return self.func(observations)


_TORCH_CODES = None


def _dtype_code(tensor_dtype):
    """mi_dtype of a torch dtype, or None."""
    global _TORCH_CODES
    if _TORCH_CODES is None:
        torch = _torch()
        _TORCH_CODES = {torch.float16: _native.MI_F16, torch.float32: _native.MI_F32, torch.float64: _native.MI_F64, torch.int32: _native.MI_I32,
                        torch.int64: _native.MI_I64, torch.uint8: _native.MI_U8}
    return _TORCH_CODES.get(tensor_dtype)


class _ArrayTransformObservation(VectorObservationWrapper):
    """What RescaleObservation, DtypeObservation and FlattenObservation share (vectorize_observation.py:114-257, VectorizeTransformObservation): the
    reference applies the scalar wrapper's ``func`` row by row and concatenates the rows into a new array of the wrapper's space.  Here the rows are
    transformed at once:

    * NumPy arrays (and host tensors, which come back as host tensors): one vectorised NumPy expression.
    * device tensors: one launch of csrc/observation_wrappers.hip on ``torch.cuda.current_stream()`` over the N -- in ``rollout`` the T * N -- rows; no
      synchronisation, no host copy.

    DEVIATION from the reference: the caller's array or tensor is never modified (``same_out`` writes into it there)."""

    def _setup(self, single_space):
        self.single_observation_space = single_space
        self.observation_space = batch_space(single_space, self.num_envs)
        self.same_out = self.observation_space == self.env.observation_space

    def observations(self, observations):
        return self._apply(observations, 1)

    def _observations_of_steps(self, block, steps):
        return self._apply(block, 2)

    def _apply(self, obs, lead):
        """``obs``: ``lead`` leading axes ((N,) or (T, N)), then the single space's shape; a tuple of such parts for a Tuple space."""
        torch = _torch()
        first = obs[0] if isinstance(obs, tuple) else obs
        if isinstance(first, torch.Tensor):
            if first.is_cuda:
                return self._device(obs, lead)
            host = tuple(p.numpy() for p in obs) if isinstance(obs, tuple) else obs.numpy()
            return torch.from_numpy(np.ascontiguousarray(self._numpy(host, lead)))
        return self._numpy(obs, lead)

    def _numpy(self, obs, lead):
        raise NotImplementedError

    def _device(self, obs, lead):
        raise NotImplementedError

    @staticmethod
    def _launch_transform(x, out, kind, dim=1, gradient=None, intercept=None):
        torch = _torch()
        lib = _native.load_library()
        lib.check(lib.transform_observations(x.device.index, C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream), C.c_void_p(x.data_ptr()),
                                             _dtype_code(x.dtype), C.c_void_p(out.data_ptr()), _dtype_code(out.dtype), x.numel(), int(dim), kind,
                                             None if gradient is None else C.c_void_p(gradient.data_ptr()),
                                             None if intercept is None else C.c_void_p(intercept.data_ptr())))
        return out


class RescaleObservation(_ArrayTransformObservation):
    """vectorize_observation.py:400-438 (transform_observation.py:515-565): the wrapper's space is ``[min_obs, max_obs]`` and an observation becomes
    ``gradient * obs + intercept`` with rescale_box's arrays, in the box's dtype: the product rounded once, then the sum rounded once (NumPy's two
    ufuncs; never an FMA).  Unbounded components have gradient 1 and intercept 0 and go through the same arithmetic: -0.0 comes out as +0.0, NaN and
    the infinities propagate."""

    def __init__(self, env, min_obs, max_obs):
        super().__init__(env)
        box = self.env.single_observation_space
        if not isinstance(box, spaces.Box):
            raise TypeError(f"RescaleObservation requires a Box observation space, got {type(box)}")
        space, self.gradient, self.intercept = _rescale_box(box, min_obs, max_obs)
        self._setup(space)
        self._on_device = {}  # device index -> (gradient, intercept) as tensors of the box's dtype

    def _numpy(self, obs, lead):
        with np.errstate(invalid="ignore", over="ignore"):  # (inf * 0 and the like: NaN, as IEEE says)
            res = self.gradient * np.asarray(obs) + self.intercept
        return res.astype(self.single_observation_space.dtype, copy=False)

    def _device(self, obs, lead):
        torch = _torch()
        dtype = getattr(torch, np.dtype(self.single_observation_space.dtype).name)
        if obs.dtype != dtype or _dtype_code(dtype) not in (_native.MI_F32, _native.MI_F64):
            raise TypeError(f"RescaleObservation on device tensors computes in the box's dtype, float32 or float64: the space is {dtype}, the tensor {obs.dtype}")
        dim = self.gradient.size
        if dim > _native.OBS_MAX_DIM:
            raise error.Error(f"RescaleObservation on device tensors takes up to {_native.OBS_MAX_DIM} observation components, the env has {dim}")
        if tuple(obs.shape[lead:]) != tuple(self.gradient.shape):
            raise ValueError(f"observations must end in the shape {self.gradient.shape} of the space, got a tensor of shape {tuple(obs.shape)}")
        params = self._on_device.get(obs.device.index)
        if params is None:  # made once per device (a wrapper built before any GPU is touched, over the CPU checker say, never makes them)
            params = self._on_device[obs.device.index] = tuple(torch.from_numpy(np.ascontiguousarray(p).reshape(-1)).to(obs.device)
                                                               for p in (self.gradient, self.intercept))
        x = obs.contiguous()
        return self._launch_transform(x, torch.empty_like(x), _native.OBS_AFFINE, dim, *params)


def _cast_box(box, dtype):
    """``Box(box.low, box.high, box.shape, dtype)`` with the bound handling of spaces/box.py:235-367 whichever Box class is in use: an infinite bound becomes
    the end of a signed integer range and is refused by an unsigned one; without infinite bounds, a bound outside the dtype's range is refused.  (On
    copies: the reference's Box writes the integer range into the ENV's own bounds.)"""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        ends = (float(np.finfo(dt).min), float(np.finfo(dt).max))
    else:
        ends = (0, 1) if dt.kind == "b" else (int(np.iinfo(dt).min), int(np.iinfo(dt).max))
    low, high = box.low.copy(), box.high.copy()
    for name, bound, infinite, end, spelled in (("low", low, np.isneginf(low), ends[0], "-np.inf"), ("high", high, np.isposinf(high), ends[1], "np.inf")):
        if infinite.any():
            if dt.kind == "i":
                bound[infinite] = end
            elif dt.kind in "ub":
                raise ValueError(f"Box unsigned int dtype don't support `{spelled}`, {name}={bound}")
        elif bound.dtype != dt:
            with np.errstate(over="ignore"):  # (the ends of float64 against float32 bounds: +-inf in the comparison)
                beyond = np.any(bound < end if name == "low" else end < bound)
            if beyond:
                raise ValueError(f"Box {name} is out of bounds of the dtype range, {name}={bound}, {'min' if name == 'low' else 'max'} dtype={end}")
    return spaces.Box(low=low, high=high, shape=box.shape, dtype=dtype)


class DtypeObservation(_ArrayTransformObservation):
    """vectorize_observation.py:441-465 (transform_observation.py:568-635): ``dtype(obs)``, NumPy's C cast, over Box and Discrete observation spaces
    (a Discrete space becomes ``Box(start, start + n, (), dtype)``).  Float -> float is rounded ONCE (float64 -> float16 does not pass through float32),
    float -> integer truncates; NaN and values outside the target's range are undefined there, as they are in NumPy.  Device tensors: float32, float64
    and int64 observations to float16, float32, float64, int32, int64 or uint8; the NumPy path takes whatever NumPy takes."""

    DEVICE_TARGETS = ("float16", "float32", "float64", "int32", "int64", "uint8")

    def __init__(self, env, dtype):
        super().__init__(env)
        space = self.env.single_observation_space
        if not isinstance(space, (spaces.Box, spaces.Discrete)):
            raise TypeError(f"DtypeObservation requires a Box, Discrete, MultiDiscrete, or MultiBinary space, got {type(space)}")
        self.dtype = dtype
        if isinstance(space, spaces.Box):
            new = _cast_box(space, dtype)
        else:
            low, high, dt = space.start, space.start + space.n, np.dtype(dtype)
            if dt.kind in "iu":  # (spaces/box.py:247-264, 314-331: the scalar bounds' range check)
                if low < np.iinfo(dt).min:
                    raise ValueError(f"Box low is out of bounds of the dtype range, low={low}, min dtype={int(np.iinfo(dt).min)}")
                if high > np.iinfo(dt).max:
                    raise ValueError(f"Box high is out of bounds of the dtype range, high={high}, max dtype={int(np.iinfo(dt).max)}")
            new = spaces.Box(low=low, high=high, shape=(), dtype=dtype)
        self._np_dtype = np.dtype(new.dtype)
        self._setup(new)

    def _numpy(self, obs, lead):
        with np.errstate(invalid="ignore", over="ignore"):
            return np.asarray(obs).astype(self._np_dtype)

    def _device(self, obs, lead):
        torch = _torch()
        target = getattr(torch, self._np_dtype.name, None) if self._np_dtype.name in self.DEVICE_TARGETS else None
        if target is None:
            raise error.Error(f"DtypeObservation on device tensors casts to {', '.join(self.DEVICE_TARGETS)}; {self._np_dtype.name} is not among them "
                              "(a NumPy batch takes any dtype)")
        if _dtype_code(obs.dtype) not in (_native.MI_F32, _native.MI_F64, _native.MI_I64):
            raise error.Error(f"DtypeObservation on device tensors casts float32, float64 and int64 observations, got {obs.dtype}")
        x = obs.contiguous()
        return self._launch_transform(x, torch.empty(x.shape, dtype=target, device=x.device), _native.OBS_CAST)


class FlattenObservation(_ArrayTransformObservation):
    """vectorize_observation.py:295-317 (spaces/utils.py ``flatten_space`` / ``flatten``).  Box: ``np.asarray(x, space.dtype).reshape(N, -1)`` -- for a
    device tensor a view, nothing is launched.  Discrete (FrozenLake, CliffWalking, Taxi): one-hot rows of the space's dtype, the space
    ``Box(0, 1, (n,), int64)``.  A Tuple of Discrete spaces (Blackjack): the one-hot segments concatenated, from the tuple of arrays the env returns (a
    rollout's ``[T, N, parts]`` block is taken apart by its last axis).  DEVIATION: a state outside its space gives a zero segment (the reference raises
    IndexError, or wraps a negative index)."""

    def __init__(self, env):
        super().__init__(env)
        space = self.env.single_observation_space
        self._parts = None
        if isinstance(space, spaces.Box):
            flat = spaces.Box(space.low.flatten(), space.high.flatten(), dtype=space.dtype)
        else:
            parts = space.spaces if isinstance(space, spaces.Tuple) else (space,)
            if not all(isinstance(p, spaces.Discrete) for p in parts) or not 1 <= len(parts) <= _native.ONE_HOT_MAX_PARTS:
                raise TypeError(f"FlattenObservation of gymnasium_amd flattens Box, Discrete and Tuple spaces of up to {_native.ONE_HOT_MAX_PARTS} Discrete "
                                f"spaces, got {space}")
            self._parts = [(int(p.start), int(p.n)) for p in parts]
            self._is_tuple = isinstance(space, spaces.Tuple)
            dtype = np.result_type(*[p.dtype for p in parts])
            if dtype != np.int64:
                raise TypeError(f"FlattenObservation of gymnasium_amd writes int64 one-hot rows, the space asks for {dtype}")
            width = sum(n for _, n in self._parts)
            flat = spaces.Box(np.zeros(width, dtype), np.ones(width, dtype), dtype=dtype)
        self._setup(flat)

    def _split(self, obs, lead):
        """The columns of the one-hot segments: the tuple as it is, a ``lead + (parts,)`` block by its last axis, a Discrete batch alone."""
        if isinstance(obs, tuple):
            cols = obs
        elif self._is_tuple:
            cols = tuple(obs[..., k] for k in range(len(self._parts)))
        else:
            cols = (obs,)
        if len(cols) != len(self._parts) or any(c.ndim != lead for c in cols):
            raise ValueError(f"observations must have {lead} leading axes and {len(self._parts)} parts, got shapes {[tuple(c.shape) for c in cols]}")
        return cols

    def _numpy(self, obs, lead):
        if self._parts is None:
            x = np.asarray(obs, dtype=self.single_observation_space.dtype)
            return x.reshape(x.shape[:lead] + (-1,))
        cols = self._split(tuple(np.asarray(p) for p in obs) if isinstance(obs, tuple) else np.asarray(obs), lead)
        return np.concatenate([(np.arange(n) == (np.asarray(c, np.int64) - start)[..., None]).astype(np.int64) for c, (start, n) in zip(cols, self._parts)],
                              axis=-1)

    def _device(self, obs, lead):
        torch = _torch()
        if self._parts is None:
            return obs.reshape(tuple(obs.shape[:lead]) + (-1,))
        cols = [c.contiguous() for c in self._split(obs, lead)]  # (Blackjack's parts are columns of one [N, 3] buffer: three small copies)
        if any(c.dtype != torch.int64 for c in cols):
            raise TypeError(f"FlattenObservation on device tensors takes int64 states, got {[c.dtype for c in cols]}")
        k, rows = len(cols), cols[0].numel()
        out = torch.empty(tuple(cols[0].shape) + (sum(n for _, n in self._parts),), dtype=torch.int64, device=cols[0].device)
        lib = _native.load_library()
        lib.check(lib.one_hot(out.device.index, C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream), (C.c_void_p * k)(*[c.data_ptr() for c in cols]), k,
                              (C.c_int64 * k)(*[s for s, _ in self._parts]), (C.c_int32 * k)(*[n for _, n in self._parts]), rows, C.c_void_p(out.data_ptr())))
        return out


class VectorRewardWrapper(VectorWrapper):
    """gymnasium.vector.VectorRewardWrapper (vector_env.py:602-625): ``step`` returns ``self.rewards(rewards)`` in place of the rewards.  Neither
    transparent nor fused; ``capture_steps`` is refused like an observation wrapper's."""

    def __init__(self, env):
        super().__init__(env)
        _close_fusion(self.env)

    def rewards(self, rewards):
        raise NotImplementedError

    def step(self, actions):
        obs, rewards, terminations, truncations, infos = self.env.step(actions)
        return obs, self.rewards(rewards), terminations, truncations, infos

    def _rewards_of_steps(self, block, steps):
        return _stack([self.rewards(block[t]) for t in range(steps)])

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` through this wrapper: the wrapped ``rollout`` with ``"rewards"`` transformed."""
        out = dict(self.env.rollout(num_steps, actions, **kwargs))
        if int(out["rewards"].shape[0]) > 0:
            out["rewards"] = self._rewards_of_steps(out["rewards"], int(out["rewards"].shape[0]))
        return out

    def capture_steps(self, *args, **kwargs):
        _refuse_capture(self, "rewards")


class TransformReward(VectorRewardWrapper):
    """vectorize_reward.py:32-70: ``func`` is applied to the reward batch as given (NumPy in, NumPy out; device tensor in, device tensor out); ``rollout``
    applies it to the ``[T, N]`` rewards at once."""

    def __init__(self, env, func):
        super().__init__(env)
        self.func = func

    def rewards(self, rewards):
        return self.func(rewards)

    def _rewards_of_steps(self, block, steps):
        return self.func(block)
