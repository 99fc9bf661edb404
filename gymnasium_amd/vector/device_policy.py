"""``action_space.sample()`` of a HipVectorEnv served by the engine's action stream.

The metric's own loop is ``env.step(env.action_space.sample())`` (gymnasium/utils/performance.py:82-97).  In the reference
``sample()`` is one NumPy call on the batched space's generator -- ``(np_random.random(nvec.shape) * nvec).astype(dtype)``
(spaces/multi_discrete.py:176-178) or ``np_random.uniform(low, high, size)`` (spaces/box.py:463-465) -- which at 65 536
sub-environments costs more host time than the step costs the GPU.  The engine restates that generator (PCG64 with skip-ahead,
``mi_action_seed`` / ``mi_action_sample``), so the batched action space of a HipVectorEnv hands out the SAME draws from the device:

* ``sample()`` returns the next batch of a block the engine drew ahead in one launch (``mi_action_sample``: ``K`` batches); with
  ``output="torch"`` the batch is a device tensor and the loop above enqueues nothing but step kernels, with ``output="numpy"`` it is a
  NumPy view of one pinned device-to-host copy per ``K`` steps.  A fresh block is allocated per refill, so a returned batch is never
  overwritten, exactly like the reference's fresh arrays.
* ``np_random`` is the space's NumPy generator, brought up to date WHEN THE PROPERTY IS READ: reading it first returns the draws that were made
  ahead but not handed out (``mi_action_skip``) and moves the generator to the stream's position (``mi_action_get``), so mixing ``sample()``,
  ``np_random.random()``, ``env.rollout()``, ``env.step(None)`` and replays of ``env.capture_steps(policy="random")`` consumes ONE stream in
  call order, as in the reference.  ``seed()`` behaves as always.  Not covered: a generator object the caller KEPT from an earlier read
  (``g = space.np_random; space.sample(); g.random()``) is not followed -- read the property again after the space has been used.
* a replayed graph of the random policy advances the stream on the device without the engine seeing it (``GraphedSteps._before_replay`` /
  ``_after_replay``): the space hands the position over first (``hip_hold_on_device``), counts what every replay draws (``hip_note_launch``)
  and remembers that it holds the account (``_hip_held``), so that back-to-back replays cost nothing on the host; every other consumer first
  hands the sum to the engine (``_hip_settle``: ``mi_action_skip``) and so continues after what the replays drew.
* ``sample(mask=...)`` / ``sample(probability=...)`` of the batched Discrete space are drawn by the engine too (``mi_action_sample_masked`` /
  ``mi_action_sample_weighted``: the reference's ``_apply_mask`` over all rows, spaces/multi_discrete.py:180-249, from the same stream).  Besides the
  reference's tuple of ``N`` rows they take ONE ``(N, A)`` array or torch tensor (``int8`` / ``float64``) -- what ``info["action_mask"]`` of a
  HipVectorEnv is -- and a device tensor stays on the device: the call only enqueues.  Host rows are validated on the host with the reference's
  exception types before anything is consumed; a device batch with an invalid row is refused as a whole and raised at the next synchronising
  call (``env.synchronize()``), like an action outside the space.  A masked draw consumes 32-bit halves of the generator's outputs and may
  leave one pending (``has_uint32`` / ``uinteger`` of ``bit_generator.state``): the half travels with the position in both directions.
  Rows wider than the engine covers (64 actions masked, 7 weighted -- where ``np.sum`` stops being the left-to-right sum) and backends without
  the entry points take the space's own NumPy path at the stream's position.
* spaces the sampler does not cover (unbounded Box, MultiDiscrete with a start) and detached spaces (pickled, deep-copied, the env closed) take
  the reference's NumPy path.

Bit-equality with the NumPy sampler is pinned by tests/test_device_policy.py (host) and tests/test_gpu_device_policy.py (GPU); the masked and
weighted draws by tests/test_masked_sampling.py and tests/test_gpu_masked_sampling.py; interleavings of every consumer with graph replays by
tests/test_stream_interleaving.py and tests/test_gpu_stream_interleaving.py.
"""
from __future__ import annotations

import weakref

import numpy as np

from .. import _native
from ..gym_api import spaces

RING_BYTES = 32 << 20  # draw-ahead per refill (at 65 536 CartPoles: 64 batches of 512 KB)
RING_MAX = 256
MAX_MASKED_ACTIONS, MAX_WEIGHTED_ACTIONS = 64, 7  # what mi_action_sample_masked / mi_action_sample_weighted cover (include/mi355env.h)


def check_rows(arg, weighted: bool, n: int, a: int) -> np.ndarray:
    """The masks (``int8``) or probabilities (``float64``) of ``n`` sub-spaces of ``a`` actions as ONE contiguous ``(n, a)`` array, from the
    reference's tuple of rows or from an ``(n, a)`` array -- with the reference's checks (spaces/multi_discrete.py:188-237: type, length, dtype,
    mask values 0 / 1, probabilities in [0, 1] summing to 1), all of them made before a single value is drawn."""
    name, want = ("probability", np.float64) if weighted else ("mask", np.int8)
    if isinstance(arg, np.ndarray) and arg.ndim == 2:
        assert arg.shape == (n, a), f"Expects a {name} batch of shape {(n, a)}, actual shape: {arg.shape}"
        assert arg.dtype == want, f"Expects the {name} dtype to be {np.dtype(want)}, actual dtype: {arg.dtype}"
        rows = np.ascontiguousarray(arg)
    else:
        assert isinstance(arg, tuple), f"Expects the {name} to be a tuple of {n} arrays or one {(n, a)} array, actual type: {type(arg)}"
        assert len(arg) == n, f"Expects one {name} per sub-space, {name} length: {len(arg)}, sub-spaces: {n}"
        for row in arg:
            assert isinstance(row, np.ndarray), f"Expects every {name} to be np.ndarray, actual type: {type(row)}"
            assert row.shape == (a,), f"Expects the {name} length to be equal to the number of actions, {name} shape: {row.shape}, actions: {a}"
            assert row.dtype == want, f"Expects the {name} dtype to be {np.dtype(want)}, actual dtype: {row.dtype}"
        rows = np.stack(arg)
    if weighted:
        assert np.all((rows == 0) | ((rows > 0) & (rows <= 1))), f"Expects all {name} values to be between 0 and 1, actual values: {rows}"
        # np.sum of a row: left to right up to 7 elements, pairwise beyond
        sums = np.add.accumulate(rows, axis=1)[:, -1] if a <= MAX_WEIGHTED_ACTIONS else np.array([np.sum(row) for row in rows])
        assert np.all(np.isclose(sums, 1)), f"Expects the sum of every {name} row to be 1, actual sums: {sums}"
    else:
        assert np.all((rows == 0) | (rows == 1)), f"Expects all {name} values to be 0 or 1, actual values: {rows}"
    return rows


class _DevicePolicyMixin:
    """Mixed into the batched MultiDiscrete / Box of a HipVectorEnv (``attach``)."""

    __slots__ = ()

    # -- which side holds the stream's position ------------------------------------------------------------
    def _hip_engine(self):
        ref = self.__dict__.get("_hip_env")
        env = ref() if ref is not None else None
        if env is None or getattr(env, "_engine", None) is None or not getattr(env, "_device_policy", False):
            return None, None
        return env, env._engine

    def _hip_drop_ahead(self, eng):
        """Give back the batches that were drawn ahead and not handed out."""
        left = len(self.__dict__.get("_hip_ring", ())) - self.__dict__.get("_hip_pos", 0)
        self._hip_ring, self._hip_pos = (), 0
        if left > 0 and eng is not None:
            eng.action_skip(-left * self._hip_batch_draws)

    def _hip_to_host(self):
        """The NumPy generator becomes the stream's position (no-op while it already is)."""
        if not self.__dict__.get("_hip_on_engine", False):
            return
        self._hip_on_engine = False
        _, eng = self._hip_engine()
        if eng is None:  # the env is gone: whatever the generator holds is all there is
            self._hip_ring, self._hip_pos = (), 0
            self._hip_held, self._hip_launched = False, 0
            return
        self._hip_settle(eng)
        self._hip_drop_ahead(eng)
        # the pending 32-bit half: from the engine where masked draws can change it, else the one handed over (64-bit draws leave it alone)
        half = eng.action_get_buffered() if hasattr(eng.lib, "action_get_buffered") else self.__dict__.get("_hip_half", (0, 0))
        _native.set_pcg_words(self._np_random, eng.action_get(), *half)

    def _hip_to_engine(self, eng):
        """The engine's action stream becomes the position (no-op while it already is)."""
        if self.__dict__.get("_hip_on_engine", False):
            return
        gen = super().np_random
        words = _native.pcg_words(gen)
        eng.action_seed(words)
        self._hip_inc = (int(words[2]), int(words[3]))  # (a captured graph holds the increment's jump: GraphedSteps compares)
        self._hip_half = _native.pcg_buffered(gen)
        if self._hip_half != (0, 0) and hasattr(eng.lib, "action_set_buffered"):
            eng.action_set_buffered(*self._hip_half)
        self._hip_on_engine = True

    def hip_use_stream(self):
        """For the env's own consumers of the stream (rollout(), step(None), capture): position on the engine, nothing drawn ahead.
        Returns the engine, or None when the space is detached."""
        _, eng = self._hip_engine()
        if eng is not None:
            self._hip_settle(eng)
            self._hip_to_engine(eng)
            self._hip_drop_ahead(eng)
        return eng

    # -- launches the engine does not see (GraphedSteps.replay) --------------------------------------------
    def _hip_settle(self, eng):
        """Tell the engine what the launches it did not see have drawn (``hip_note_launch``): its position moves past them
        (``mi_action_skip``, which also marks the per-lane states for re-initialisation).  No-op when there were none."""
        if self.__dict__.get("_hip_held", False):
            self._hip_held = False
            drawn, self._hip_launched = self.__dict__.get("_hip_launched", 0), 0
            if drawn:
                eng.action_skip(drawn)

    def hip_hold_on_device(self):
        """For a consumer whose launches the engine does not see -- the kernels of a replayed graph read and advance the per-lane states of the
        stream on the device: besides ``hip_use_stream()``, the engine's own copy becomes the position (``mi_action_get``: the capture, an eager
        ``step(None)`` or a masked draw may have left it with the lanes) and the lanes are (re-)initialised for it where a seed, a skip or a
        rollout left them behind (``mi_action_sample`` with T = 0, on the env's current stream).  From here on the space keeps the account:
        every such launch is noted (``hip_note_launch``), and the next consumer of any other kind first hands the sum to the engine
        (``_hip_settle``), so ``np_random``, ``sample()``, ``rollout()`` and ``step(None)`` continue after what the launches drew.  While
        ``_hip_held`` is set a further launch needs nothing from the host.  The ENGINE is not told: while ``_hip_held`` is set its own copy of
        the position is the one before the launches, so raw engine calls that read or move the stream (``env._engine.action_get()`` /
        ``action_skip()`` / ``rollout()`` / ``step_bound(None, ...)``) must not be made then -- go through the space or the env, which settle
        first.  Returns the engine, or None when the space is detached."""
        eng = self.hip_use_stream()
        if eng is not None:
            eng.action_get()
            eng.action_sample(0, None, _native.MI_DEVICE)
            self._hip_held, self._hip_launched = True, 0
        return eng

    def hip_note_launch(self, batches: int):
        """A launch the engine did not see has drawn ``batches`` batches from the lanes (no engine call: an addition on the host)."""
        self._hip_launched = self.__dict__.get("_hip_launched", 0) + int(batches) * self._hip_batch_draws

    # -- the Space interface ------------------------------------------------------------------------------------
    @property
    def np_random(self):
        self._hip_to_host()
        return super().np_random

    def seed(self, seed=None):
        self._hip_on_engine = self._hip_held = False  # (whatever was drawn ahead, or by launches since, belongs to the old stream)
        self._hip_launched = 0
        self._hip_ring, self._hip_pos = (), 0
        return super().seed(seed)

    def sample(self, mask=None, probability=None):
        d = self.__dict__
        if mask is None and probability is None:  # the common call: the next batch of the block drawn ahead (a non-empty block implies an attached engine)
            pos, ring = d.get("_hip_pos", 0), d.get("_hip_ring", ())
            if pos < len(ring):
                d["_hip_pos"] = pos + 1
                return ring[pos]
        if mask is not None or probability is not None:
            return self._hip_sample_with(mask, probability)
        env, eng = self._hip_engine()
        if eng is None:
            return super().sample(mask, probability)
        pos = self.__dict__.get("_hip_pos", 0)
        ring = self.__dict__.get("_hip_ring", ())
        if pos >= len(ring):
            self._hip_settle(eng)
            self._hip_to_engine(eng)
            ring = self._hip_ring = env._draw_action_batches(self._hip_ring_steps)
            pos = 0
        self._hip_pos = pos + 1
        return ring[pos]

    def _hip_sample_with(self, mask, probability):
        """sample(mask=...) / sample(probability=...): the space's own NumPy path (HipMultiDiscrete draws on the engine)."""
        return super().sample(mask, probability)

    def __getstate__(self):
        self._hip_to_host()
        return {k: v for k, v in self.__dict__.items() if not k.startswith("_hip_")}

    def __deepcopy__(self, memo):
        import copy

        self._hip_to_host()
        new = self.__class__.__new__(self.__class__)
        for k, v in self.__dict__.items():
            if not k.startswith("_hip_"):
                setattr(new, k, copy.deepcopy(v, memo))
        return new


class HipMultiDiscrete(_DevicePolicyMixin, spaces.MultiDiscrete):
    def _hip_sample_with(self, mask, probability):
        if mask is not None and probability is not None:
            raise ValueError(f"Only one of `mask` or `probability` can be provided, actual values: mask={mask}, probability={probability}")
        if self.nvec.ndim != 1:
            self._hip_to_host()
            return super()._hip_sample_with(mask, probability)
        weighted = probability is not None
        arg = probability if weighted else mask
        n, a = int(self.nvec.shape[0]), int(self.nvec.flat[0])
        env, eng = self._hip_engine()
        on_engine = (eng is not None and hasattr(eng.lib, "action_sample_masked")
                     and a <= (MAX_WEIGHTED_ACTIONS if weighted else MAX_MASKED_ACTIONS))
        if hasattr(arg, "data_ptr") and not isinstance(arg, np.ndarray):  # a torch tensor: what can be checked without reading it is checked here
            name, want = ("probability", "torch.float64") if weighted else ("mask", "torch.int8")
            assert tuple(arg.shape) == (n, a), f"Expects a {name} batch of shape {(n, a)}, actual shape: {tuple(arg.shape)}"
            assert str(arg.dtype) == want, f"Expects the {name} dtype to be {want}, actual dtype: {arg.dtype}"
            if on_engine and env.output == "torch" and arg.device == env._tdev:
                self.hip_use_stream()
                return env._sample_with_rows(arg, weighted, on_device=True)
            arg = arg.detach().cpu().numpy()
        rows = check_rows(arg, weighted, n, a)
        if on_engine:
            self.hip_use_stream()
            return env._sample_with_rows(rows, weighted, on_device=False)
        self._hip_to_host()
        rows = tuple(rows)
        out = spaces.MultiDiscrete.sample(self, mask=None if weighted else rows, probability=rows if weighted else None)
        return env._as_sample(out) if eng is not None else out


class HipBox(_DevicePolicyMixin, spaces.Box):
    pass


def attach(space, env, act_dim: int):
    """Turn the batched action space of ``env`` into its device-sampled subclass -- when the engine's sampler covers it: a MultiDiscrete of
    equal counts starting at 0 (a batched Discrete) or a fully bounded float32 Box (the classic and MuJoCo action spaces).  Returns the space."""
    if isinstance(space, spaces.MultiDiscrete):
        start = getattr(space, "start", None)
        ok = space.dtype == np.int64 and np.all(space.nvec == space.nvec.flat[0]) and (start is None or not np.any(start))
        cls = HipMultiDiscrete
    elif isinstance(space, spaces.Box):
        ok = space.dtype == np.float32 and bool(np.all(space.bounded_below) and np.all(space.bounded_above))
        cls = HipBox
    else:
        return space
    if not ok:
        return space
    new = cls.__new__(cls)  # the same space (nvec / bounds / dtype / generator) as an instance of the device-sampled subclass
    new.__dict__.update(space.__dict__)
    space = new
    space._hip_env = weakref.ref(env)
    space._hip_on_engine = space._hip_held = False
    space._hip_launched = 0
    space._hip_ring, space._hip_pos = (), 0
    space._hip_batch_draws = env.num_envs * act_dim
    bytes_per_batch = env.num_envs * act_dim * (8 if cls is HipMultiDiscrete else 4)
    space._hip_ring_steps = int(max(1, min(RING_MAX, RING_BYTES // bytes_per_batch)))
    return space
