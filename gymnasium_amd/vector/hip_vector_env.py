"""HipVectorEnv: a gymnasium.vector.VectorEnv whose sub-environments are lanes of an MI355X kernel.

Host-side mirror of the reference's vectoriser for this path.  It replaces, with ONE C-ABI call per method,

  gymnasium/vector/sync_vector_env.py:76-185   __init__  (spaces, metadata["autoreset_mode"], buffers)
  gymnasium/vector/sync_vector_env.py:187-264  reset     (seed fan-out seed+i, options["reset_mask"])
  gymnasium/vector/sync_vector_env.py:266-337  step      (NEXT_STEP / SAME_STEP / DISABLED autoreset)
  gymnasium/wrappers/common.py:116-150         TimeLimit (max_episode_steps, folded into the kernel)
  gymnasium/wrappers/vector/common.py:156-235  RecordEpisodeStatistics (optional, accumulated on device)

and is created through the reference's own plug-in boundary, ``make_vec(id, num_envs,
vectorization_mode="vector_entry_point", **kwargs)`` (envs/registration.py:933-963), which calls the subclass
as ``creator(num_envs=..., max_episode_steps=..., **kwargs)``.

Observations/rewards/terminations/truncations have the reference's shapes and dtypes ((N, obs_dim) float32,
(N,) float64, (N,) bool, (N,) bool).  With ``output="numpy"`` they are NumPy arrays (copies unless
``copy=False``, like SyncVectorEnv); with ``output="torch"`` they are tensors resident in HBM and nothing
crosses PCIe (VectorEnv is generic in its array type, vector_env.py:20,42).
"""
from __future__ import annotations

import time
from typing import Any

import numpy as np

from .. import _native
from ..gym_api import AutoresetMode, VectorEnv, batch_space, error, logger, seeding
from . import device_policy

_U64 = (1 << 64) - 1


def _verify_number_and_cast(x) -> float:
    """envs/classic_control/utils.py:9-15."""
    try:
        return float(x)
    except (ValueError, TypeError) as e:
        raise ValueError(f"An option ({x}) could not be converted to a float.") from e


def parse_low_high(options, default_low, default_high):
    """envs/classic_control/utils.py:17-46 maybe_parse_reset_bounds."""
    if options is None:
        return None
    low = _verify_number_and_cast(options.get("low") if "low" in options else default_low)
    high = _verify_number_and_cast(options.get("high") if "high" in options else default_high)
    if low > high:
        raise ValueError(f"Lower bound ({low}) must be lower than higher bound ({high}).")
    return (low, high)


def _pcg_words_for_seed(seed: int) -> np.ndarray:
    gen, _ = seeding.np_random(seed)
    return _native.pcg_words(gen)


class UnknownEnvAttributeError(error.Error, AttributeError):
    """get_attr / set_attr with a name that is no per-sub-environment attribute of the env's kind.  Both an AttributeError (what the name is) and
    an error.Error (what every other refusal of get_attr / set_attr raises), so that a caller may catch either."""


class HipVectorEnv(VectorEnv):
    """Base class; subclasses set KIND, spaces, default reset bounds and constructor params."""

    KIND: str = ""
    DEFAULT_MAX_EPISODE_STEPS: int | None = None
    INFO_KEYS: tuple = ()        # names of the engine's scalar info columns (MuJoCo envs); the first N_RESET_INFO_KEYS are also
    N_RESET_INFO_KEYS: int = 0   # what the scalar env's reset() reports (_get_reset_info), i.e. valid on autoreset steps
    INFO_VECTOR_KEYS: tuple = () # (name, width) array-valued info entries stored after the scalar columns; reported by step AND reset
    INFO_DTYPES: dict = {}       # info key -> dtype of the reference's entry where it is not float64 (e.g. reward_ctrl of a float32 action: np.float32)
    HOST_INFOS = False           # True: the infos need host-side table look-ups (ToyText): built on the host also with output="torch"
    metadata: dict[str, Any] = {"render_modes": [], "autoreset_mode": AutoresetMode.NEXT_STEP}

    # -- to be provided by subclasses ------------------------------------------------------------------
    def _single_spaces(self):
        raise NotImplementedError

    def _engine_params(self) -> tuple:
        return ()

    def _engine_options(self) -> int:
        """MI_CFG_* option bits of mi_config.reserved[0]."""
        return 0

    # -- wrappers fused into the step kernel (gymnasium_amd/wrappers/vector.py, mi_set_step_epilogue) ----------------------------------
    FUSES_WRAPPERS = False  # classic control: NormalizeObservation / NormalizeReward / ClipReward run as the step kernel's output stage

    def _fusion_state(self):
        st = self.__dict__.get("_fused")
        if st is None:
            # chain: the fused wrappers in wrapping order (innermost first); entry: the OUTERMOST fused wrapper the running step() call came
            # through (None: the env is being stepped directly); attached: signature of the epilogue the engine currently holds
            st = self._fused = {"obs": None, "ret": None, "clip_pre": None, "clip_post": None, "closed": False, "chain": [], "entry": None, "attached": None}
        return st

    def _can_fuse(self) -> bool:
        return (self.FUSES_WRAPPERS and self._engine_factory is None and hasattr(self._engine.lib, "set_step_epilogue")
                and not self._fusion_state()["closed"] and self._step_wrappers == (0, 0.0, 0) and self._max_and_skip == 0)

    def _fuse(self, wrapper, slot: str) -> int:
        """Register ``wrapper`` as the next member of the fused unit; returns its position in the chain."""
        st = self._fusion_state()
        st[slot] = wrapper
        st["chain"].append((slot, wrapper))
        return len(st["chain"]) - 1

    def _sync_epilogue(self):
        """Attach exactly the epilogue of the step() call in progress.  The wrapped values belong to the WRAPPER they come out of
        (the reference's contract: the inner env returns raw values): a step entered through fused wrapper k runs the arithmetic of the
        chain's members 0..k as the step kernel's output stage, a step of the env itself -- or of a wrapper below k -- runs none / fewer.
        Settings are read from the wrappers at every step (a tuple compare), so a later ``w.gamma = ...`` / ``w.min_reward = ...`` /
        ``w.update_running_mean = False`` takes effect like in the reference; the engine is only re-configured when something changed."""
        st = self.__dict__.get("_fused")
        if st is None or not st["chain"]:
            return
        entry = st["entry"]
        level = -1 if entry is None else entry._fuse_index
        members = st["chain"][:level + 1]
        sig = [level]
        for slot, w in members:
            # (the statistics HANDLES and accumulator addresses are part of the signature: replacing `w.obs_rms` / `w.return_rms`, e.g. when a
            # checkpoint is restored, must re-attach the epilogue to the new object)
            if slot == "obs":
                sig += [float(w.epsilon), bool(w.update_running_mean), w.obs_rms._h.value]
            elif slot == "ret":
                sig += [float(w.gamma), float(w.epsilon), bool(w.update_running_mean),
                        w.return_rms._h.value, w._acc.data_ptr(), w._prev.data_ptr()]
            else:
                sig += [None if w.min_reward is None else float(w.min_reward), None if w.max_reward is None else float(w.max_reward)]
        sig = tuple(sig)
        if sig == st["attached"]:
            return
        if not members:
            self._epilogue_struct = None
            self._engine.set_step_epilogue(None)
        else:
            e = _native.MiStepEpilogue()
            for slot, w in members:
                if slot == "obs":
                    e.obs_rms, e.obs_epsilon, e.obs_update = w.obs_rms._h, float(w.epsilon), int(w.update_running_mean)
                elif slot == "ret":
                    e.return_rms, e.accumulated, e.prev_done = w.return_rms._h, w._acc.data_ptr(), w._prev.data_ptr()
                    e.gamma, e.reward_epsilon, e.reward_update = float(w.gamma), float(w.epsilon), int(w.update_running_mean)
                else:
                    lo, hi = w.min_reward, w.max_reward
                    setattr(e, slot, (1 if lo is not None else 0) | (2 if hi is not None else 0))
                    setattr(e, slot + "_min", 0.0 if lo is None else float(lo)), setattr(e, slot + "_max", 0.0 if hi is None else float(hi))
            self._epilogue_struct = e  # keep the ctypes object alive
            self._engine.set_step_epilogue(e)
        st["attached"] = sig

    def _parse_reset_options(self, options):
        """Return the env-specific (b0, b1) reset bounds or None for defaults; raise ValueError like the reference."""
        return None

    def _short_step_allowed(self) -> bool:
        """May step() take its short path (device tensor in, the env's own output tensors out)?  Subclasses whose step() post-processes say no."""
        return True

    # --------------------------------------------------------------------------------------------------
    def __init__(self, num_envs: int = 1, max_episode_steps: int | None = None, autoreset_mode=AutoresetMode.NEXT_STEP,
                 render_mode: str | None = None, device=None, output: str = "numpy", copy: bool = True,
                 env_index_offset: int = 0, record_episode_statistics: bool = False, strict_actions: bool = False, sample_output: str | None = None,
                 _engine_factory=None):
        if render_mode is not None:
            raise error.Error("gymnasium_amd sub-environments live on the GPU and cannot render; use render_mode=None")
        if output not in ("numpy", "torch"):
            raise ValueError(f"output must be 'numpy' or 'torch', got {output!r}")
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1, got {num_envs}")
        self.autoreset_mode = autoreset_mode if isinstance(autoreset_mode, AutoresetMode) else AutoresetMode(autoreset_mode)
        self.metadata = dict(type(self).metadata)
        self.metadata["autoreset_mode"] = self.autoreset_mode
        self.render_mode = None
        self.copy = bool(copy)
        # output="torch": the engine runs asynchronously on torch's stream, so what the reference raises at once -- the AssertionError for an
        # action outside the space (cartpole.py:165-167), stepping a finished sub-environment under DISABLED autoreset -- is DEFERRED: the
        # kernel records a sticky error word in page-locked memory (the sub-environment with the invalid action is left untouched) and a later `step()` -- the first
        # one that finds the word set, usually the next -- or any synchronising call (`synchronize()`, `statistics()`) raises it.  strict_actions=True synchronises after every step and raises there, at the cost
        # of the asynchrony (debugging aid).  NumPy input is always validated on the host before anything is mutated.
        self.strict_actions = bool(strict_actions)
        self.output = output
        # What `action_space.sample()` hands out (vector/device_policy.py).  Either way the batch is drawn by the engine from the space's own
        # stream, bit-equal to the NumPy sampler.  "numpy" (default): NumPy arrays like the reference's, whatever `output` is -- scripts that
        # treat a sample as an ndarray keep working.  "torch" (needs output="torch"): device tensors, so that the metric's own loop
        # `env.step(env.action_space.sample())` (utils/performance.py:82-97) enqueues nothing but step kernels.
        sample_output = "numpy" if sample_output is None else sample_output
        if sample_output not in ("numpy", "torch") or (sample_output == "torch" and output != "torch"):
            raise ValueError(f"sample_output must be 'numpy' or (with output='torch') 'torch', got {sample_output!r} with output={output!r}")
        self.sample_output = sample_output
        self.max_episode_steps = self.DEFAULT_MAX_EPISODE_STEPS if max_episode_steps is None else max_episode_steps
        self.env_index_offset = int(env_index_offset)
        self.record_episode_statistics = bool(record_episode_statistics)

        self.single_observation_space, self.single_action_space = self._single_spaces()
        self.observation_space = batch_space(self.single_observation_space, self.num_envs)
        self.action_space = batch_space(self.single_action_space, self.num_envs)

        self._device_index = _resolve_device(device)
        self._engine_factory = _engine_factory
        if _engine_factory is None:
            lib = _native.load_library()  # raises ImportError if the HIP library was not built
            self._engine = _native.Engine(lib, self.KIND, self.num_envs, self.max_episode_steps, self.autoreset_mode.value,
                                          self._engine_params(), self._device_index, options=self._engine_options())
        else:  # test seam: tests drive this host class against a checker backend; never used by the package itself
            self._engine = _engine_factory(self.KIND, self.num_envs, self.max_episode_steps, self.autoreset_mode.value,
                                           self._engine_params(), self._device_index, options=self._engine_options())
        eng = self._engine
        self._discrete = eng.act_dtype is np.int64
        self._act_shape = (self.num_envs,) if self._discrete else (self.num_envs, eng.act_dim)
        # action_space.sample() from the engine's action stream (vector/device_policy.py): same draws as the NumPy sampler, no host sampling
        self._device_policy = hasattr(getattr(eng, "lib", None), "action_sample") and not getattr(self, "_host_policy_only", False)
        self.action_space = device_policy.attach(self.action_space, self, eng.act_dim)
        self.last_sampled_actions = None  # step(None): the batch the on-device policy drew in the last such step
        self._seeded = False
        self._has_reset = False
        self._async_pending = None
        self._was_done = np.zeros(self.num_envs, dtype=np.bool_)  # mirror of the device's needs-reset flags (SyncVectorEnv._autoreset_envs)
        self._alloc_buffers()
        if self.record_episode_statistics:
            self._episode_count = 0
            self._episode_start = np.zeros(self.num_envs)
            self._prev_dones = np.zeros(self.num_envs, dtype=np.bool_)

    @property
    def episode_count(self) -> int:
        """Episodes finished so far (RecordEpisodeStatistics.episode_count); with device-resident infos the count lives on the device and
        reading it synchronises."""
        dev = self.__dict__.get("_episode_count_t")
        return getattr(self, "_episode_count", 0) + (int(dev.item()) if dev is not None else 0)

    def set_output(self, output: str):
        """Switch between NumPy batches ("numpy": the engine's pinned host block, one H2D + one D2H per step) and device tensors ("torch": the engine writes
        straight into torch tensors in HBM, nothing crosses PCIe) after construction -- what wrappers.vector.NumpyToTorch(env) does.
        Call before reset()."""
        if output not in ("numpy", "torch"):
            raise ValueError(f"output must be 'numpy' or 'torch', got {output!r}")
        if output != self.output:
            if hasattr(self.action_space, "_hip_to_host"):
                self.action_space._hip_to_host()  # (batches drawn ahead have the old mode's array type)
            if output == "numpy":
                self.sample_output = "numpy"
            self.output = output
            self._alloc_buffers()
            self._has_reset = False

    def enable_episode_statistics(self):
        """Switch on the on-device episode accounting after construction (what wrappers.vector.RecordEpisodeStatistics(env) does):
        the step kernels start writing the finished episodes' return / length rows.  Call before reset()."""
        if not self.record_episode_statistics:
            self.record_episode_statistics = True
            self._episode_count = 0
            self._episode_start = np.zeros(self.num_envs)
            self._prev_dones = np.zeros(self.num_envs, dtype=np.bool_)
            self._alloc_buffers()
            self._has_reset = False

    # -- buffers ---------------------------------------------------------------------------------------
    def _alloc_buffers(self):
        N, eng = self.num_envs, self._engine
        old_count = self.__dict__.pop("_episode_count_t", None)
        if old_count is not None:  # episodes counted on the device so far survive a re-allocation / a switch of the output mode
            self._episode_count = getattr(self, "_episode_count", 0) + int(old_count.item())
        if self.output == "torch":
            import torch

            self._torch = torch
            # (the test seam's checker backend computes on the host: its "device" tensors are host tensors, same code path otherwise)
            dev = torch.device("cuda", self._device_index) if self._engine_factory is None else torch.device("cpu")
            self._tdev = dev
            self._obs_tdtype = {np.float64: torch.float64, np.float32: torch.float32, np.int64: torch.int64}[eng.obs_dtype]
            self._obs_shape = (N,) if (eng.obs_dtype is np.int64 and eng.obs_dim == 1) else (N, eng.obs_dim)  # Discrete states batch to MultiDiscrete: (N,)
            self._obs = torch.zeros(self._obs_shape, dtype=self._obs_tdtype, device=dev)
            self._rew = torch.zeros((N,), dtype=torch.float64, device=dev)
            self._term = torch.zeros((N,), dtype=torch.bool, device=dev)
            self._trunc = torch.zeros((N,), dtype=torch.bool, device=dev)
            self._final = torch.zeros(self._obs_shape, dtype=self._obs_tdtype, device=dev) if self.autoreset_mode == AutoresetMode.SAME_STEP else None
            self._info = torch.zeros((N, eng.info_dim), dtype=torch.float64, device=dev) if eng.info_dim else None
            self._final_info = torch.zeros((N, eng.info_dim), dtype=torch.float64, device=dev) if (eng.info_dim and self._final is not None) else None
            self._ep_r = torch.zeros((N,), dtype=torch.float64, device=dev) if self.record_episode_statistics else None
            self._ep_l = torch.zeros((N,), dtype=torch.int32, device=dev) if self.record_episode_statistics else None
            self._loc = _native.MI_DEVICE
            # device-resident infos (no read-back per step): the pending-autoreset set and the episode clocks live on the device too
            self._device_infos = not self.HOST_INFOS
            self._was_done_t = torch.zeros((N,), dtype=torch.bool, device=dev)
            self._all_true_t = torch.ones((N,), dtype=torch.bool, device=dev)
            if self.record_episode_statistics:
                self._episode_start_t = torch.zeros((N,), dtype=torch.float64, device=dev)
                self._prev_dones_t = torch.zeros((N,), dtype=torch.bool, device=dev)
                self._episode_count_t = torch.zeros((), dtype=torch.int64, device=dev)
            # the addresses step() writes to never change between two allocations: hand them to the binding once (Engine.bind_step)
            eng.bind_step(self._p(self._obs), self._p(self._rew), self._p(self._term), self._p(self._trunc), self._p(self._final), self._p(self._ep_r),
                          self._p(self._ep_l), self._loc, self._p(self._info), self._p(self._final_info))
            self._raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) if self._engine_factory is None else None
            self._stream_bound = None
            # step()'s short path (device tensors in, device tensors out, nothing for the host to assemble): see step()
            self._act_tdtype = torch.int64 if self._discrete else torch.float32
            self._short_step = (not self.INFO_KEYS and self.autoreset_mode != AutoresetMode.SAME_STEP and not self.record_episode_statistics
                                and not self.strict_actions and type(self).step in _SHORT_STEP_OWNERS and self._short_step_allowed())
        else:
            self._obs_shape = (N,) if (eng.obs_dtype is np.int64 and eng.obs_dim == 1) else (N, eng.obs_dim)
            same = self.autoreset_mode == AutoresetMode.SAME_STEP
            # The engine's own PINNED host arrays (mi_host_buffers): the step's single D2H lands directly in what step() returns
            # (copy=False) or copies from (copy=True, like SyncVectorEnv's deepcopy).  A backend without them (the checker): plain arrays.
            hb = eng.host_buffers() if hasattr(eng, "host_buffers") else None
            self._pinned = hb is not None
            self.action_buffer = hb["actions"] if hb else None  # sample / write actions here to skip the staging memcpy of step()
            self._obs = hb["obs"] if hb else np.zeros(self._obs_shape, dtype=eng.obs_dtype)
            self._rew = hb["reward"] if hb else np.zeros((N,), dtype=np.float64)
            self._term = hb["terminated"] if hb else np.zeros((N,), dtype=np.bool_)
            self._trunc = hb["truncated"] if hb else np.zeros((N,), dtype=np.bool_)
            self._final = (hb["final_obs"] if hb else np.zeros(self._obs_shape, dtype=eng.obs_dtype)) if same else None
            self._info = (hb["info"] if hb else np.zeros((N, eng.info_dim), dtype=np.float64)) if eng.info_dim else None
            self._final_info = (hb["final_info"] if hb else np.zeros((N, eng.info_dim), dtype=np.float64)) if (eng.info_dim and same) else None
            self._ep_r = (hb["episode_return"] if hb else np.zeros((N,), dtype=np.float64)) if self.record_episode_statistics else None
            self._ep_l = (hb["episode_length"] if hb else np.zeros((N,), dtype=np.int32)) if self.record_episode_statistics else None
            self._loc = _native.MI_HOST
            self._device_infos = False

    def _p(self, buf):
        if buf is None:
            return None
        return buf.data_ptr() if self.output == "torch" else buf

    def _out(self, buf):
        if not self.copy:
            return buf
        return buf.clone() if self.output == "torch" else buf.copy()

    def _bind_stream(self):
        """The engine enqueues on torch's CURRENT stream of its device (asked at every step; the engine is told only when it changed)."""
        if self.output == "torch" and self._engine_factory is None:
            raw = self._raw_stream
            st = raw(self._device_index) if raw is not None else self._torch.cuda.current_stream(self._tdev).cuda_stream
            if st != self._stream_bound:
                self._engine.set_stream(st)
                self._stream_bound = st

    # -- seeding ---------------------------------------------------------------------------------------
    def _seed_engines(self, seed, mask):
        """SyncVectorEnv seed fan-out (sync_vector_env.py:204-212): int -> seed+i, list -> per env, None -> keep."""
        N, off = self.num_envs, self.env_index_offset
        if seed is None:
            if not self._seeded:  # like Env.np_random's lazy OS-entropy seeding (core.py:227-236)
                base = int(np.random.SeedSequence().generate_state(1, np.uint64)[0]) >> 1
                self._engine.seed_sequence(base, off, None)
                self._seeded = True
            return
        if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
            seed = int(seed)
            if seed < 0:
                raise error.Error(f"Seed must be greater or equal to zero, actual value: {seed}")
            if seed + off + N - 1 <= _U64:
                self._engine.seed_sequence(seed, off, mask)  # SeedSequence + PCG64 seeding evaluated on device
            else:  # beyond 64 bits: NumPy on the host
                words = np.stack([_pcg_words_for_seed(seed + off + i) for i in range(N)])
                self._engine.seed(words, mask)
            self._seeded = True
            return
        seeds = list(seed)
        if len(seeds) != N:
            raise ValueError(f"If seeds are passed as a list the length must match num_envs={N} but got length={len(seeds)}.")
        words = np.zeros((N, 4), dtype=np.uint64)
        smask = np.zeros(N, dtype=np.uint8)
        for i, s in enumerate(seeds):
            if s is None:
                continue
            words[i] = _pcg_words_for_seed(s)
            smask[i] = 1
        if not self._seeded and not smask.all():
            base = int(np.random.SeedSequence().generate_state(1, np.uint64)[0]) >> 1
            self._engine.seed_sequence(base, off, None)
        if mask is not None:
            smask &= np.asarray(mask, dtype=np.uint8)
        if smask.any():
            self._engine.seed(words, smask)
        self._seeded = True

    # -- API -------------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        """Reset the sub-environments (all, or options["reset_mask"]) and return (observations, infos)."""
        self._check_open()
        self._check_not_pending("reset")
        if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
            super().reset(seed=int(seed))
        mask = None
        if options is not None and "reset_mask" in options:
            options = dict(options)
            reset_mask = options.pop("reset_mask")
            if not isinstance(reset_mask, np.ndarray):
                raise TypeError(f"`options['reset_mask']` must be a numpy array, got {type(reset_mask)}")
            if reset_mask.shape != (self.num_envs,):
                raise ValueError(f"`options['reset_mask']` must have shape `({self.num_envs},)`, got {reset_mask.shape}")
            if reset_mask.dtype != np.bool_:
                raise TypeError(f"`options['reset_mask']` must have `dtype=np.bool_`, got {reset_mask.dtype}")
            if not np.any(reset_mask):
                raise ValueError(f"`options['reset_mask']` must contain a boolean array with at least one True value, got reset_mask={reset_mask}")
            mask = np.ascontiguousarray(reset_mask).view(np.uint8)
        bounds = self._parse_reset_options(options if options else None)
        self._seed_engines(seed, mask)
        self._bind_stream()
        if self.output == "torch":
            dmask = None
            if mask is not None:
                dmask = self._torch.from_numpy(mask.copy()).to(self._tdev)
            self._engine.reset(None if dmask is None else dmask.data_ptr(), bounds, self._obs.data_ptr(), _native.MI_DEVICE)
        else:
            self._engine.reset(mask, bounds, self._obs, _native.MI_HOST)
        self._has_reset = True
        if mask is None:
            self._was_done[:] = False
        else:  # sync_vector_env.py:232-234: only the reset sub-envs leave the pending-autoreset set
            self._was_done[mask.view(np.bool_)] = False
        if self.record_episode_statistics:
            now = time.perf_counter()
            if mask is None:
                self._episode_start[:] = now
                self._prev_dones[:] = False
            else:
                self._episode_start[mask.view(np.bool_)] = now
                self._prev_dones[mask.view(np.bool_)] = False
        if self._device_infos:
            keep = None if mask is None else ~dmask.view(self._torch.bool)
            # (every update of the device-side bookkeeping is IN PLACE: a HIP graph captured around step() keeps reading and writing these tensors)
            self._was_done_t.logical_and_(keep) if keep is not None else self._was_done_t.zero_()
            if self.record_episode_statistics:
                if keep is None:
                    self._episode_start_t.fill_(now), self._prev_dones_t.zero_()
                else:
                    self._episode_start_t.copy_(self._torch.where(keep, self._episode_start_t, now))
                    self._prev_dones_t.logical_and_(keep)
        return self._out(self._obs), self._reset_infos(mask)

    def _reset_infos(self, mask) -> dict:
        """The scalar envs' reset info (``_get_reset_info`` / ``{"prob": 1}``) batched like VectorEnv._add_info does."""
        return {}

    def _coerce_actions(self, actions):
        """The action batch as the engine reads it: (object to keep alive, pointer, mi_dtype of a Box row).

        Box action spaces: the reference hands every sub-environment its row of the caller's array AS IT IS (sync_vector_env.py:274 iterate();
        pendulum.py:127-134, continuous_mountain_car.py:153, mujoco_env.py:148 `data.ctrl[:] = ctrl`) -- a float64 array is not rounded to the
        space's float32, and NumPy's promotion rules then make parts of the step float64 arithmetic.  So float64 rows (and integer arrays:
        exact in float64) go to the engine un-rounded with actions_dtype = MI_F64; float32 rows take the float32 path, which is also the
        on-device sampler's type.  A list of Python lists reaches the scalar envs as Python lists: `action[0]` is then a Python float, which
        NumPy 2 treats as WEAK (np.float32 + float stays float32) -- MI_F64_WEAK; only MountainCarContinuous tells it from MI_F64.  A row of
        NumPy scalars (`[[np.float64(x)], ...]`) is STRONG, like an ndarray row: only exact Python floats / ints are weak.
        NOT reproduced: float16 / bfloat16 rows.  The reference would then compute parts of the step in half precision; the engine widens
        them to float32 (one warning per env), so those trajectories are within tolerance of, not bit-equal to, the reference's."""
        eng = self._engine
        if self.output == "torch" and hasattr(actions, "data_ptr"):
            t = self._torch
            if self._discrete:
                want = t.int64
            else:
                want = t.float32 if actions.dtype in (t.float32, t.float16, t.bfloat16) else t.float64
                if actions.dtype in (t.float16, t.bfloat16):
                    self._warn_half_precision(actions.dtype)
            if actions.device != self._tdev or actions.dtype != want or not actions.is_contiguous():
                actions = actions.to(device=self._tdev, dtype=want).contiguous()
            if actions.numel() != self.num_envs * eng.act_dim:
                raise ValueError(f"actions must have {self.num_envs * eng.act_dim} elements, got shape {tuple(actions.shape)}")
            return actions, actions.data_ptr(), (_native.MI_F64 if want is t.float64 else _native.MI_F32)
        a = np.asarray(actions)
        dtype = _native.MI_F32
        if self._discrete:
            if not np.issubdtype(a.dtype, np.integer):
                raise AssertionError(f"{actions!r} ({type(actions)}) invalid")
            a = np.ascontiguousarray(a, dtype=np.int64)
        elif a.dtype in (np.float32, np.float16):
            if a.dtype == np.float16:
                self._warn_half_precision(a.dtype)
            a = np.ascontiguousarray(a, dtype=np.float32)
        else:
            # weak = every leaf is an exact Python float / int (NEP 50); np.generic scalars inside the lists are strong like an ndarray's elements
            weak = (isinstance(actions, (list, tuple)) and len(actions) > 0
                    and all(isinstance(r, (list, tuple)) and all(type(x) in (float, int) for x in r) for r in actions))
            a, dtype = np.ascontiguousarray(a, dtype=np.float64), (_native.MI_F64_WEAK if weak else _native.MI_F64)
        if a.size != self.num_envs * eng.act_dim:
            raise ValueError(f"actions must have shape {self._act_shape}, got {a.shape}")
        if self.output == "torch":
            ta = self._torch.from_numpy(a).to(self._tdev)
            return ta, ta.data_ptr(), dtype
        return a, a, dtype

    def _warn_half_precision(self, dtype):
        if not getattr(self, "_warned_half", False):
            self._warned_half = True
            logger.warn(f"{dtype} action rows are widened to float32: the reference computes parts of the step in half precision for such rows, "
                        "so this trajectory is within tolerance of the reference's, not bit-equal to it")

    def step(self, actions):
        """One lockstep step of every sub-environment: (obs, rewards, terminations, truncations, infos)."""
        if self.output == "torch" and self._short_step and self._has_reset and self._async_pending is None and not self.closed \
                and actions.__class__ is self._torch.Tensor and actions.dtype is self._act_tdtype and actions.device == self._tdev \
                and actions.is_contiguous() and actions.numel() == self.num_envs * self._engine.act_dim and not self.__dict__.get("_fused"):
            # The metric's loop (utils/performance.py:82-97) with device tensors is host-bound: the step kernel of 65 536 CartPoles runs 5 us, and the
            # general path below -- coercion of whatever the caller passed, the wrappers' epilogue, the infos -- costs about as much in Python.
            # An action tensor that already is what the engine reads, on an env with nothing to assemble on the host, goes straight to mi_step.
            self._bind_stream()
            self._act_f64 = False
            try:
                self._engine.step_bound(actions.data_ptr(), _native.MI_F32)
            except _native.NativeError as e:
                if e.code in (-1, -5):
                    raise AssertionError(e.message) from e
                if e.code == -4:  # MI_ERR_UNSUPPORTED: StickyAction is on and the element type of the action rows changed
                    raise error.Error(e.message) from e
                raise
            if self.copy:
                return self._obs.clone(), self._rew.clone(), self._term.clone(), self._trunc.clone(), {}
            return self._obs, self._rew, self._term, self._trunc, {}
        self._check_open()
        self._check_not_pending("step")
        if not self._has_reset:
            raise AssertionError("Call reset before using step method.")
        aout = None
        if actions is None:
            # the on-device policy: `step(action_space.sample())` in ONE launch -- the step kernel draws the batch from the action stream itself
            # (mi_step with actions == NULL).  Device tensors only; with NumPy batches it is the two calls it stands for.
            eng_stream = self.action_space.hip_use_stream() if (self.output == "torch" and hasattr(self.action_space, "hip_use_stream")) else None
            if eng_stream is None:
                # (not `self.step(...)`: a subclass that reshapes what step() returns -- Blackjack's tuple of columns -- is already on the stack)
                actions = self.action_space.sample()
        if actions is None:
            if self.last_sampled_actions is None:
                t = self._torch
                self.last_sampled_actions = t.zeros(self._act_shape, dtype=t.int64 if self._discrete else t.float32, device=self._tdev)
            keep, aptr, adt, aout = None, None, _native.MI_F32, self.last_sampled_actions.data_ptr()
        else:
            keep, aptr, adt = self._coerce_actions(actions)
        self._act_f64 = adt != _native.MI_F32
        self._bind_stream()
        self._sync_epilogue()
        try:
            if self.output == "torch":
                self._engine.step_bound(aptr, adt, aout)
                if self.strict_actions:
                    self._engine.synchronize()  # raises the device error word of this very step
            else:
                self._engine.step(aptr, self._obs, self._rew, self._term, self._trunc, self._final, self._ep_r, self._ep_l, self._loc, self._info,
                                  self._final_info, actions_dtype=adt)
        except _native.NativeError as e:
            if e.code == -1:  # MI_ERR_INVALID_ARGUMENT: action outside the space (cartpole.py:165-167 asserts)
                raise AssertionError(e.message) from e
            if e.code == -5:
                raise AssertionError(e.message) from e
            if e.code == -4:  # MI_ERR_UNSUPPORTED: StickyAction is on and the element type of the action rows changed
                raise error.Error(e.message) from e
            raise
        del keep
        infos = self._build_infos()
        return self._out(self._obs), self._out(self._rew), self._out(self._term), self._out(self._trunc), infos

    def _info_columns(self):
        """[(name, first column, width, in_reset_info)] of the engine's info row."""
        cols = [(name, k, 0, k < self.N_RESET_INFO_KEYS) for k, name in enumerate(self.INFO_KEYS)]
        start = len(self.INFO_KEYS)
        for name, width in self.INFO_VECTOR_KEYS:
            cols.append((name, start, width, True))
            start += width
        return cols

    def _info_dict(self, rows, supplied, reset_rows) -> dict:
        """VectorEnv._add_info (vector_env.py:277-338) over an info matrix: one array per key plus the `_key` mask of the
        sub-envs that supplied it.  `supplied`: rows that have an info at all; `reset_rows`: rows whose info is the scalar
        env's RESET info, which carries only the reset keys.  A key no sub-env supplied does not appear."""
        out: dict[str, Any] = {}
        for name, start, width, in_reset in self._info_columns():
            mask = supplied if in_reset else (supplied & ~reset_rows)
            if not mask.any():
                continue
            col = rows[:, start] if width == 0 else rows[:, start:start + width]
            val = np.where(mask if width == 0 else mask[:, None], col, 0.0)
            dt = self._info_dtype(name)
            if dt is not None:  # (the engine's info row is float64; such entries hold float32 / integer values exactly)
                val = val.astype(dt)
            out[name], out["_" + name] = val, mask.copy()
        return out

    def _info_dtype(self, name):
        """dtype of the reference's info entry where it is not float64.  An np.float32 entry is one computed from the action row
        (`reward_ctrl`): float32 for a float32 row, float64 for a float64 row (see _coerce_actions)."""
        dt = self.INFO_DTYPES.get(name)
        if dt is np.float32 and getattr(self, "_act_f64", False):
            return None
        return dt

    def _host(self, buf):
        return buf.cpu().numpy() if self.output == "torch" else buf

    # -- asynchronous stepping (AsyncVectorEnv.step_async / step_wait, vector/async_vector_env.py:440-521) ----------------------------
    def step_async(self, actions):
        """Enqueue one step (actions H2D, kernel, one D2H into the pinned block) and return at once; ``step_wait()`` collects it.
        With device tensors (``output="torch"``) every step is already asynchronous: this is then ``step()`` with the result parked."""
        self._check_open()
        if not self._has_reset:
            raise AssertionError("Call reset before using step method.")
        self._check_not_pending("step_async")
        if self.output == "torch" or not self._pinned:
            self._async_pending = ("done", self.step(actions))
            return
        keep, aptr, adt = self._coerce_actions(actions)
        self._act_f64 = adt != _native.MI_F32
        self._bind_stream()
        self._sync_epilogue()
        try:
            self._engine.step_async(aptr, self._obs, self._rew, self._term, self._trunc, self._final, self._ep_r, self._ep_l, self._info, self._final_info,
                                    actions_dtype=adt)
        except _native.NativeError as e:
            if e.code in (-1, -5):
                raise AssertionError(e.message) from e
            raise
        self._async_pending = ("engine", keep)

    def step_wait(self, timeout=None):
        pending = getattr(self, "_async_pending", None)
        if pending is None:
            raise error.NoAsyncCallError("Calling `step_wait` without any prior call to `step_async`.", "step")  # async_vector_env.py:477-481
        self._async_pending = None
        if pending[0] == "done":
            return pending[1]
        try:
            self._engine.step_wait()
        except _native.NativeError as e:
            if e.code in (-1, -5):
                raise AssertionError(e.message) from e
            raise
        infos = self._build_infos()
        return self._out(self._obs), self._out(self._rew), self._out(self._term), self._out(self._trunc), infos

    def _info_dict_device(self, rows, supplied, reset_rows) -> dict:
        """_info_dict over a device info matrix without reading anything back.  supplied / reset_rows: device bool masks or None (= every
        sub-env / none).  The KEY SET IS STATIC: a key no sub-env supplied in this step is still present (its `_key` mask is all False) --
        deciding otherwise would need the masks on the host, i.e. a synchronisation per step."""
        t, out = self._torch, {}
        for name, start, width, in_reset in self._info_columns():  # (`...`: a rollout's matrices have a leading time axis, and so have its masks)
            col = rows[..., start] if width == 0 else rows[..., start:start + width]
            mask = supplied if (in_reset or reset_rows is None) else (~reset_rows if supplied is None else supplied & ~reset_rows)
            if mask is None:
                val, mask = (col.clone() if self.copy else col), self._all_true_t
            else:
                val = t.where(mask if width == 0 else mask[..., None], col, 0.0)
            dt = self._info_dtype(name)
            if dt is not None:  # same dtypes as the NumPy infos (_info_dict)
                val = val.to({np.float32: t.float32, np.int64: t.int64, np.int32: t.int32, np.bool_: t.bool}[dt])
            out[name], out["_" + name] = val, (mask.clone() if (self.copy and mask is self._all_true_t) else mask)
        return out

    def _build_infos_device(self) -> dict:
        """The infos of a step as DEVICE tensors (output="torch"): nothing is copied to the host and nothing synchronises -- the step stays
        asynchronous for the MuJoCo kinds (whose infos carry x_position, reward terms, ...), under SAME_STEP autoreset and with episode
        statistics.  Differences from the NumPy dict, all forced by not looking at the flags on the host: the key set is static (see
        _info_dict_device); under SAME_STEP `final_obs` is the batched tensor of final observations (rows valid where `_final_obs`), not an
        object array; `episode` is present every step with its `_episode` mask."""
        t, N = self._torch, self.num_envs
        infos: dict[str, Any] = {}
        same_step = self.autoreset_mode == AutoresetMode.SAME_STEP
        dones = self._term | self._trunc
        if self.INFO_KEYS and self._info is not None:
            reset_rows = self._was_done_t if self.autoreset_mode == AutoresetMode.NEXT_STEP else (dones if same_step else None)
            infos.update(self._info_dict_device(self._info, None, reset_rows))
        if same_step:
            infos["final_obs"], infos["_final_obs"] = self._out(self._final), dones
            finfo = self._info_dict_device(self._final_info, dones, None) if (self.INFO_KEYS and self._final_info is not None) else {}
            infos["final_info"], infos["_final_info"] = finfo, dones
        # (private copies: `dones` itself is handed to the caller as the `_episode` / `_final_obs` / `_final_info` masks, and an in-place edit of
        # those must not reach the next step's autoreset bookkeeping -- the NumPy path returns copies as well)
        self._was_done_t.copy_(dones) if not same_step else self._was_done_t.zero_()
        if self.record_episode_statistics:
            now = time.perf_counter()
            if not same_step:
                self._episode_start_t.copy_(t.where(self._prev_dones_t, now, self._episode_start_t))
            self._prev_dones_t.copy_(dones)
            infos["episode"] = {"r": self._out(self._ep_r), "l": self._ep_l.to(t.int64),
                                "t": t.where(dones, t.round((now - self._episode_start_t) * 1e6) / 1e6, 0.0)}
            infos["_episode"] = dones
            self._episode_count_t.add_(dones.sum())
            if same_step:
                self._episode_start_t.copy_(t.where(dones, now, self._episode_start_t))
        return infos

    def _build_infos(self) -> dict:
        infos: dict[str, Any] = {}
        N = self.num_envs
        same_step = self.autoreset_mode == AutoresetMode.SAME_STEP
        if not (self.INFO_KEYS or same_step or self.record_episode_statistics):
            return infos  # nothing to report: with device tensors the step stays asynchronous (no read-back of the flags)
        if self._device_infos:
            return self._build_infos_device()
        dones = np.logical_or(self._host(self._term), self._host(self._trunc))
        every = np.ones(N, dtype=np.bool_)
        if self.INFO_KEYS and self._info is not None:
            # an env in its NEXT_STEP autoreset step supplies only its reset info (sync_vector_env.py:279-284); under SAME_STEP a
            # finished env's top-level entries are its reset info and the finishing step's info goes to "final_info" (:309-319)
            if self.autoreset_mode == AutoresetMode.NEXT_STEP:
                reset_rows = self._was_done
            elif same_step:
                reset_rows = dones
            else:
                reset_rows = np.zeros(N, dtype=np.bool_)
            infos.update(self._info_dict(self._host(self._info), every, reset_rows))
        if same_step and dones.any():
            # sync_vector_env.py:309-317 via VectorEnv._add_info: object array of per-env observations + nested final_info
            final = self._host(self._final)
            arr = np.full(N, None, dtype=object)
            scalar_obs = final.ndim == 1  # Discrete observations: the scalar env returns a Python int (frozen_lake.py:343 `int(s)`)
            for i in np.flatnonzero(dones):
                arr[i] = int(final[i]) if scalar_obs else final[i].copy()
            infos["final_obs"], infos["_final_obs"] = arr, dones.copy()
            finfo = {}
            if self.INFO_KEYS and self._final_info is not None:
                finfo = self._info_dict(self._host(self._final_info), dones, np.zeros(N, dtype=np.bool_))
            infos["final_info"], infos["_final_info"] = finfo, dones.copy()
        self._was_done = dones if self.autoreset_mode != AutoresetMode.SAME_STEP else np.zeros(N, dtype=np.bool_)
        if self.record_episode_statistics:
            now = time.perf_counter()
            any_done = bool(dones.any())
            if self.autoreset_mode != AutoresetMode.SAME_STEP:
                self._episode_start[self._prev_dones] = now
            self._prev_dones = dones
            if any_done:
                r = self._ep_r.cpu().numpy() if self.output == "torch" else self._ep_r.copy()
                ln = self._ep_l.cpu().numpy() if self.output == "torch" else self._ep_l.copy()
                infos["episode"] = {"r": r, "l": ln.astype(np.int64),
                                    "t": np.where(dones, np.round(now - self._episode_start, 6), 0.0)}
                infos["_episode"] = dones.copy()
                self._episode_count += int(dones.sum())
                if self.autoreset_mode == AutoresetMode.SAME_STEP:
                    self._episode_start[dones] = now
        return infos

    # -- the policy `action_space.sample()` on the engine's action stream (vector/device_policy.py) -----------------------------------
    def _draw_action_batches(self, K: int):
        """The next K batches of ``action_space.sample()`` in one engine call (mi_action_sample); a tuple of K arrays / device tensors,
        views of ONE freshly allocated block (nothing a caller holds is ever overwritten)."""
        eng = self._engine
        if self.sample_output == "torch" and self.output == "torch":
            t = self._torch
            self._bind_stream()
            block = t.empty((K,) + self._act_shape, dtype=t.int64 if self._discrete else t.float32, device=self._tdev)
            eng.action_sample(K, block.data_ptr(), _native.MI_DEVICE)
            return block.unbind(0)
        dtype = np.int64 if self._discrete else np.float32
        block = None
        if self._engine_factory is None:  # page-locked, so that the device-to-host copy of the block runs at PCIe speed
            try:
                import torch

                block = torch.empty((K,) + self._act_shape, dtype=torch.int64 if self._discrete else torch.float32, pin_memory=True).numpy()
            except Exception:
                block = None
        if block is None:
            block = np.empty((K,) + self._act_shape, dtype=dtype)
        self._bind_stream()
        eng.action_sample(K, block, _native.MI_HOST)
        return tuple(block)

    def _as_sample(self, batch: np.ndarray):
        """A batch of actions drawn on the host as what ``action_space.sample()`` of this env returns (``sample_output``)."""
        if self.sample_output == "torch" and self.output == "torch":
            return self._torch.from_numpy(batch).to(self._tdev)
        return batch

    def _sample_with_rows(self, rows, weighted: bool, on_device: bool):
        """One batch of ``action_space.sample(mask=rows)`` / ``sample(probability=rows)`` from the engine's action stream
        (mi_action_sample_masked / mi_action_sample_weighted).  ``rows``: the ``(N, A)`` masks (int8) or probabilities (float64), a NumPy array or
        -- ``on_device`` -- a tensor on the env's device, in which case the call only enqueues and an invalid row surfaces at the next
        synchronising call."""
        eng = self._engine
        fn = eng.action_sample_weighted if weighted else eng.action_sample_masked

        def draw(*args):
            try:
                fn(*args)
            except _native.NativeError as e:
                if e.code == -1:  # MI_ERR_INVALID_ARGUMENT: an invalid row, here or in an earlier enqueued batch (the reference asserts)
                    raise AssertionError(e.message) from e
                raise

        self._bind_stream()
        if on_device:
            t = self._torch
            rows = rows.contiguous()
            out = t.empty((self.num_envs,), dtype=t.int64, device=self._tdev)
            draw(rows.data_ptr(), out.data_ptr(), _native.MI_DEVICE)
            return out if self.sample_output == "torch" else out.cpu().numpy()
        out = np.empty((self.num_envs,), dtype=np.int64)
        draw(rows, out, _native.MI_HOST)
        return self._as_sample(out)

    # -- fused rollouts ---------------------------------------------------------------------------------
    def rollout(self, num_steps: int, actions=None, *, return_actions: bool = True, infos: bool = False):
        """``num_steps`` consecutive ``step()`` calls in ONE kernel launch; trajectories are time-major tensors in HBM.

        With ``actions=None`` the random policy ``action_space.sample()`` (spaces/multi_discrete.py:176-178,
        spaces/box.py:463-465) is evaluated on device from the action space's own PCG64 stream, which is then
        advanced on the host by the number of draws consumed -- so
        ``rollout(T)`` == ``[step(action_space.sample()) for _ in range(T)]`` bit for bit.
        Requires ``output="torch"``.  Returns dict(obs, rewards, terminations, truncations[, actions]).

        ``infos=True`` adds the key ``"infos"``: the fifth element of those ``step()`` calls, as ONE dict with the static key set of the
        device-resident infos (_build_infos_device) whose tensors have a leading time axis -- the engine's info entries with their ``_key``
        masks, under SAME_STEP ``final_obs`` / ``_final_obs`` and ``final_info`` / ``_final_info``, with episode statistics ``episode`` =
        {"r", "l", "t"} and ``_episode`` (mi_rollout_infos: the kernels store these rows per step).  It equals ``torch.stack`` over the
        ``step()`` calls' dicts wherever the mask is true and is ZERO elsewhere (``final_obs`` included, whose unfinished rows ``step()``
        leaves stale).  ``"t"`` is a host wall-clock value: ONE ``time.perf_counter()`` reading per rollout call serves all its steps.
        The env's bookkeeping (pending autoresets, episode clocks and count, the current final_obs / info / episode rows) ends as those
        ``step()`` calls leave it; nothing synchronises for the kinds whose ``step()`` infos are device-resident.
        """
        self._check_open()
        if self.output != "torch":
            raise error.Error("rollout() returns device tensors; create the env with output='torch'")
        if not self._has_reset:
            raise AssertionError("Call reset before using rollout.")
        t, eng, N, T = self._torch, self._engine, self.num_envs, int(num_steps)
        dev = self._tdev
        if infos:
            if not hasattr(getattr(eng, "lib", None), "rollout_infos"):
                raise error.Error("rollout(infos=True): the engine behind this env does not store a rollout's infos (mi_rollout_infos)")
            if T < 1:
                raise ValueError(f"rollout(infos=True) needs num_steps >= 1, got {num_steps}")
        self._bind_stream()
        act_dtype = t.int64 if self._discrete else t.float32
        act_shape = (T, N) if self._discrete else (T, N, eng.act_dim)
        a_in = a_out = None
        in_dtype = _native.MI_F32
        if actions is not None:
            if not self._discrete and actions.dtype == t.float64:  # float64 rows are taken un-rounded, like step() does (_coerce_actions)
                a_in, in_dtype = actions.to(device=dev).contiguous(), _native.MI_F64
            else:
                a_in = actions.to(device=dev, dtype=act_dtype).contiguous()
            if tuple(a_in.shape) != act_shape:
                raise ValueError(f"actions must have shape {act_shape}, got {tuple(a_in.shape)}")
        else:
            on_stream = self.action_space.hip_use_stream() if hasattr(self.action_space, "hip_use_stream") else None
            if on_stream is None:  # a space without the device sampler: its NumPy generator is the position
                eng.action_seed(_native.pcg_words(self.action_space.np_random))
            if return_actions:
                a_out = t.empty(act_shape, dtype=act_dtype, device=dev)
        obs = t.empty((T,) + tuple(self._obs_shape), dtype=self._obs_tdtype, device=dev)
        rew = t.empty((T, N), dtype=t.float64, device=dev)
        term = t.empty((T, N), dtype=t.bool, device=dev)
        trunc = t.empty((T, N), dtype=t.bool, device=dev)
        extra = self._rollout_extra_buffers(T) if infos else {}
        if extra:
            eng.rollout(T, None if a_in is None else a_in.data_ptr(), None if a_out is None else a_out.data_ptr(), obs.data_ptr(), rew.data_ptr(),
                        term.data_ptr(), trunc.data_ptr(), actions_in_dtype=in_dtype, extra={k: v.data_ptr() for k, v in extra.items()})
        else:
            eng.rollout(T, None if a_in is None else a_in.data_ptr(), None if a_out is None else a_out.data_ptr(),
                        obs.data_ptr(), rew.data_ptr(), term.data_ptr(), trunc.data_ptr(), actions_in_dtype=in_dtype)
        self._act_f64 = in_dtype == _native.MI_F64
        if actions is None and on_stream is None:
            self.action_space.np_random.bit_generator.advance(T * N * eng.act_dim)
        out = {"obs": obs, "rewards": rew, "terminations": term, "truncations": trunc}
        if a_out is not None:
            out["actions"] = a_out
        elif a_in is not None and return_actions:
            out["actions"] = a_in
        if infos:  # (before the pending-autoreset set moves on: the first step's reset rows come from it)
            out["infos"] = self._rollout_infos(extra, obs, term | trunc)
        # the vector env's "current" buffers follow the last step, as after T step() calls
        self._obs.copy_(obs[-1]); self._rew.copy_(rew[-1]); self._term.copy_(term[-1]); self._trunc.copy_(trunc[-1])
        if self.autoreset_mode == AutoresetMode.NEXT_STEP:  # the sub-envs that finished in the last step reset in the next one
            if self._device_infos:
                self._was_done_t.copy_(term[-1] | trunc[-1])
            else:
                self._was_done = (term[-1] | trunc[-1]).cpu().numpy()
        return out

    def _rollout_extra_buffers(self, T: int) -> dict:
        """The [T, N, ...] device tensors mi_rollout_infos fills for this configuration (keys: the members of mi_rollout_extra)."""
        t, eng, N, dev = self._torch, self._engine, self.num_envs, self._tdev
        same = self.autoreset_mode == AutoresetMode.SAME_STEP
        x = {}
        if same:
            x["final_obs"] = t.empty((T,) + tuple(self._obs_shape), dtype=self._obs_tdtype, device=dev)
        if self.record_episode_statistics:
            x["episode_return"] = t.empty((T, N), dtype=t.float64, device=dev)
            x["episode_length"] = t.empty((T, N), dtype=t.int32, device=dev)
        if eng.info_dim:
            x["info"] = t.empty((T, N, eng.info_dim), dtype=t.float64, device=dev)
            if same:
                x["final_info"] = t.empty((T, N, eng.info_dim), dtype=t.float64, device=dev)
        return x

    def _rollout_infos(self, x: dict, obs, dones) -> dict:
        """The infos of the T steps of a rollout from the arrays the engine stored (``x``, _rollout_extra_buffers): _build_infos_device with a
        leading time axis, including what it does to the env's bookkeeping.  ``dones``: terminations | truncations, [T, N]."""
        t, N, T = self._torch, self.num_envs, int(dones.shape[0])
        same = self.autoreset_mode == AutoresetMode.SAME_STEP
        host_side = not self._device_infos  # (the kinds whose step() infos are assembled on the host keep their bookkeeping there)
        infos: dict[str, Any] = {}
        if self.INFO_KEYS and "info" in x:
            if same:
                reset_rows = dones
            else:  # the rows in their autoreset step: the pending set before the call, then every step's finished rows
                was = t.from_numpy(self._was_done.copy()).to(self._tdev) if host_side else self._was_done_t
                reset_rows = t.cat([was[None], dones[:-1]])
            infos.update(self._info_dict_device(x["info"], t.ones_like(dones), reset_rows))
            self._info.copy_(x["info"][-1])
        if same:
            infos["final_obs"], infos["_final_obs"] = x["final_obs"], dones
            has_finfo = bool(self.INFO_KEYS) and "final_info" in x
            infos["final_info"], infos["_final_info"] = (self._info_dict_device(x["final_info"], dones, None) if has_finfo else {}), dones
            # step() leaves the rows of sub-environments that finished nothing untouched: the current buffers end with each row's LAST finish
            last = (dones * t.arange(1, T + 1, device=dones.device)[:, None]).amax(0)  # 0: never finished in this window
            pick, cols = (last - 1).clamp_min(0), t.arange(N, device=dones.device)
            for cur, arr in ((self._final, x["final_obs"]), (self._final_info, x["final_info"] if has_finfo else None)):
                if cur is not None and arr is not None:
                    got = arr[pick, cols]
                    cur.copy_(t.where((last > 0).reshape((N,) + (1,) * (got.dim() - 1)), got, cur))
        if self.record_episode_statistics:
            now = time.perf_counter()  # ONE reading for all T steps
            start = t.from_numpy(self._episode_start.copy()).to(self._tdev) if host_side else self._episode_start_t
            prev = t.from_numpy(self._prev_dones.copy()).to(self._tdev) if host_side else self._prev_dones_t
            # restarted[t]: the episode clock of the row was set to `now` by one of the steps before t (NEXT_STEP: in its autoreset step, i.e. the step
            # after a finish -- the first one from the flags the call found; SAME_STEP: right after the finishing step)
            first = t.zeros_like(prev) if same else prev
            restarted = t.cat([first[None], dones[:-1]]).to(t.int32).cumsum(0) > 0
            started = t.where(restarted, now, start[None])
            infos["episode"] = {"r": x["episode_return"], "l": x["episode_length"].to(t.int64),
                                "t": t.where(dones, t.round((now - started) * 1e6) / 1e6, 0.0)}
            infos["_episode"] = dones
            moved = (restarted[-1] | dones[-1]) if same else restarted[-1]
            self._ep_r.copy_(x["episode_return"][-1]), self._ep_l.copy_(x["episode_length"][-1])
            if host_side:
                self._episode_start = t.where(moved, now, start).cpu().numpy()
                self._prev_dones = dones[-1].cpu().numpy()
                self._episode_count += int(dones.sum().item())
            else:
                self._episode_start_t.copy_(t.where(moved, now, start))
                self._prev_dones_t.copy_(dones[-1])
                self._episode_count_t.add_(dones.sum())
        return infos

    # -- lookahead: candidate action sequences scored from the present state (mi_lookahead) --------------------------------------------------
    _CLASSIC_KINDS = ("cartpole", "pendulum", "acrobot", "mountain_car", "mountain_car_continuous")

    def _lookahead_refusal(self) -> str | None:
        if self.output != "torch":
            return "lookahead() takes and returns device tensors; create the env with output='torch'"
        if self.KIND not in self._CLASSIC_KINDS:
            return (f"{type(self).__name__}: lookahead exists for CartPole-v1, Pendulum-v1, Acrobot-v1, MountainCar-v0 and MountainCarContinuous-v0 "
                    "only (the MuJoCo and ToyText kernels have no such loop)")
        if getattr(self, "_shared_rng", False):
            return "rng='shared' is the reference's NumPy CartPoleVectorEnv: it has no sub-environment generators that a candidate could copy"
        if getattr(self, "fast_math", False):
            return "lookahead runs the exact kernels only: not with fast_math=True"
        if self._step_wrappers != (0, 0.0, 0):
            return "this env runs RepeatAction / StickyAction inside its step (set_step_wrappers): lookahead steps the plain env"
        if self._max_and_skip:
            return "this env runs MaxAndSkipObservation inside its step (set_max_and_skip): lookahead steps the plain env"
        st = self.__dict__.get("_fused")
        if st is not None and st["chain"]:
            return "vector wrappers are fused into this env's step kernel: lookahead returns the plain env's rewards and observations"
        return None

    def _lookahead_begin(self, name: str, gamma) -> float:
        """What ``lookahead()`` and ``lookahead_policy()`` (``name``) check before they look at their own arguments; returns gamma as a float."""
        self._check_open()
        self._check_not_pending(name)
        refusal = self._lookahead_refusal()
        if refusal:
            raise error.Error(refusal)
        if not self._has_reset:
            raise AssertionError(f"Call reset before using {name}.")
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)):
            raise TypeError(f"gamma must be a number, got {type(gamma).__name__}")
        gamma = float(gamma)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {gamma}")
        return gamma

    def _lookahead_outputs(self, name: str, K: int, final_obs: bool) -> dict:
        """What both (``name``) do once their own arguments are valid and K >= 1: K against the lane index, the engine's entry point ``mi_<name>``,
        torch's stream bound, the output tensors allocated."""
        t, N = self._torch, self.num_envs
        if K * N >= 2 ** 31:
            raise ValueError(f"{name} needs K * N < 2**31, got K = {K}, N = {N}")
        if not hasattr(getattr(self._engine, "lib", None), name):
            raise error.Error(f"{name} needs the device engine (mi_{name}): the engine behind this env has no such entry point")
        self._bind_stream()
        dev = self._tdev
        out = {"returns": t.empty((K, N), dtype=t.float64, device=dev), "steps": t.empty((K, N), dtype=t.int32, device=dev),
               "terminated": t.empty((K, N), dtype=t.bool, device=dev), "truncated": t.empty((K, N), dtype=t.bool, device=dev)}
        if final_obs:
            out["final_obs"] = t.empty((K, N) + tuple(self._obs_shape[1:]), dtype=self._obs_tdtype, device=dev)
        return out

    def lookahead(self, actions, gamma: float = 1.0, *, final_obs: bool = False) -> dict:
        """Score ``K`` candidate action sequences of length ``H`` for every sub-environment from its PRESENT state, in one kernel launch, without
        touching the env: what a sampling planner (random shooting, CEM, MPPI) asks of a model.

        ``actions``: ``[H, K, N]`` int64 for the Discrete ids, ``[H, K, N, act_dim]`` float32 or float64 for the Box ids (a trailing
        ``act_dim`` of 1 may be omitted; float64 rows go in un-rounded, as in ``step()``).  Candidate ``k`` of sub-environment ``i`` steps a private
        copy of that sub-environment -- state, elapsed steps, ``set_attr`` values, generator -- with ``actions[t, k, i]`` for ``t = 0 .. H - 1`` and stops
        after the first step that terminates or truncates (``max_episode_steps`` counts from the sub-environment's elapsed steps).

        Returns a dict of device tensors: ``returns`` ``[K, N]`` float64 (``G = 0; disc = 1``; per step ``G = G + disc * r; disc = disc * gamma``,
        in float64 in that order), ``steps`` ``[K, N]`` int32 (steps taken), ``terminated`` / ``truncated`` ``[K, N]`` bool (of the last step
        taken) and, with ``final_obs=True``, ``final_obs`` ``[K, N, obs_dim]`` float32 (the observation after the last step taken).  A
        sub-environment that waits for its autoreset gives return 0, 0 steps, both flags False and its present observation.

        Nothing synchronises.  An action outside a Discrete space is reported like ``step()``'s with device tensors: by a later synchronising call.
        """
        gamma = self._lookahead_begin("lookahead", gamma)
        t, eng, N = self._torch, self._engine, self.num_envs
        if isinstance(actions, np.ndarray):
            actions = t.from_numpy(actions)
        if not isinstance(actions, t.Tensor):
            raise TypeError(f"actions must be a tensor, got {type(actions).__name__}")
        if self._discrete:
            if actions.dtype != t.int64:
                raise TypeError(f"actions of {type(self).__name__} must be int64, got {actions.dtype}")
            want = "[H, K, N]"
            ok = actions.dim() == 3
        else:
            if actions.dtype not in (t.float32, t.float64):
                raise TypeError(f"actions of {type(self).__name__} must be float32 or float64, got {actions.dtype}")
            want = f"[H, K, N, {eng.act_dim}]" + (" or [H, K, N]" if eng.act_dim == 1 else "")
            ok = (actions.dim() == 4 and actions.shape[3] == eng.act_dim) or (actions.dim() == 3 and eng.act_dim == 1)
        if not ok or actions.shape[2] != N:
            raise ValueError(f"actions must have shape {want} with N = {N}, got {tuple(actions.shape)}")
        H, K = int(actions.shape[0]), int(actions.shape[1])
        if H < 1 or K < 1:
            raise ValueError(f"lookahead needs H >= 1 and K >= 1, got H = {H}, K = {K}")
        out = self._lookahead_outputs("lookahead", K, final_obs)
        in_dtype = _native.MI_F64 if actions.dtype == t.float64 else _native.MI_F32
        a = actions.to(device=self._tdev).contiguous()
        eng.lookahead(a.data_ptr(), H, K, gamma, out["returns"].data_ptr(), out["steps"].data_ptr(), out["terminated"].data_ptr(),
                      out["truncated"].data_ptr(), out["final_obs"].data_ptr() if final_obs else None, actions_dtype=in_dtype)
        return out  # (a converted copy `a` is the caching allocator's on torch's stream, which the launch is on: reused in stream order)

    # -- lookahead over policies: candidate parameter vectors scored from the present state (mi_lookahead_policy) ------------------------------
    def policy_param_layout(self, hidden: int = 0) -> dict:
        """Where the parts of one candidate's parameter vector lie for ``lookahead_policy(..., hidden=hidden)``: ``{"W": (slice, shape), "b": ...,
        "size": P}`` for ``hidden == 0``, ``{"W1": ..., "b1": ..., "W2": ..., "b2": ..., "size": P}`` otherwise (row-major; ``W`` / ``W2`` have one row per
        action of a Discrete space or per component of a Box action, ``W`` / ``W1`` one column per observation component):
        ``row[sl].reshape(shape)`` reads a part, ``row[sl] = part.ravel()`` writes it."""
        if self.KIND not in self._CLASSIC_KINDS:
            raise error.Error(f"{type(self).__name__}: lookahead_policy exists for CartPole-v1, Pendulum-v1, Acrobot-v1, MountainCar-v0 and "
                              "MountainCarContinuous-v0 only")
        if isinstance(hidden, bool) or not isinstance(hidden, (int, np.integer)):
            raise TypeError(f"hidden must be an int, got {type(hidden).__name__}")
        hidden = int(hidden)
        if not 0 <= hidden <= 256:
            raise ValueError(f"hidden must be in [0, 256], got {hidden}")
        obs = int(self._engine.obs_dim)
        A = int(self.single_action_space.n) if self._discrete else int(self._engine.act_dim)
        parts = [("W", (A, obs)), ("b", (A,))] if hidden == 0 else [("W1", (hidden, obs)), ("b1", (hidden,)), ("W2", (A, hidden)), ("b2", (A,))]
        out, at = {}, 0
        for name, shape in parts:
            n = int(np.prod(shape))
            out[name] = (slice(at, at + n), shape)
            at += n
        out["size"] = at
        return out

    def lookahead_policy(self, params, horizon: int, gamma: float = 1.0, *, hidden: int = 0, final_obs: bool = False) -> dict:
        """Score ``K`` candidate POLICIES for every sub-environment from its PRESENT state, closed loop, in one kernel launch, without touching the
        env: what evolution strategies, ARS, CEM over parameters and population-based search ask of a model.  ``lookahead()`` with the action of every
        step computed on the device from the observation the candidate's private copy would have returned.

        ``params``: ``[K, P]`` float32 (tensor or ndarray; nothing is cast), candidate ``k`` using row ``k`` for all ``N`` sub-environments;
        ``policy_param_layout(hidden)`` gives ``P`` and the parts.  ``hidden == 0``: ``y = b + W @ obs``.  ``1 <= hidden <= 256``:
        ``y = b2 + W2 @ relu(b1 + W1 @ obs)``.  All in float32, every product and every sum rounded on its own, accumulated in ascending index order
        (``include/mi355env.h`` states the order operation by operation; NumPy reproduces it bit for bit).  Discrete ids take the first largest
        ``y[o]`` by a strict ``>`` scan from ``o = 0`` -- no comparison with a NaN holds, which is NOT ``np.argmax``'s rule --; Box ids take ``y[0]`` as the float32
        action, clipped by the env as every action is.  There is no tanh or sigmoid.

        ``horizon``, ``gamma``, ``final_obs`` and the returned dict of device tensors are ``lookahead()``'s.  Nothing synchronises."""
        gamma = self._lookahead_begin("lookahead_policy", gamma)
        t, eng = self._torch, self._engine
        P = self.policy_param_layout(hidden)["size"]
        hidden = int(hidden)
        if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)):
            raise TypeError(f"horizon must be an int, got {type(horizon).__name__}")
        H = int(horizon)
        if H < 1:
            raise ValueError(f"horizon must be >= 1, got {H}")
        if isinstance(params, np.ndarray):
            if params.dtype != np.float32:
                raise TypeError(f"params must be float32, got {params.dtype}")
            params = t.from_numpy(params)
        if not isinstance(params, t.Tensor):
            raise TypeError(f"params must be a tensor, got {type(params).__name__}")
        if params.dtype != t.float32:
            raise TypeError(f"params must be float32, got {params.dtype}")
        if params.dim() != 2 or params.shape[1] != P:
            raise ValueError(f"params must have shape [K, P] with P = {P} for hidden = {hidden}, got {tuple(params.shape)}")
        K = int(params.shape[0])
        if K < 1:
            raise ValueError(f"lookahead_policy needs K >= 1, got K = {K}")
        out = self._lookahead_outputs("lookahead_policy", K, final_obs)
        p = params.to(device=self._tdev).contiguous()
        eng.lookahead_policy(p.data_ptr(), hidden, H, K, gamma, out["returns"].data_ptr(), out["steps"].data_ptr(), out["terminated"].data_ptr(),
                             out["truncated"].data_ptr(), out["final_obs"].data_ptr() if final_obs else None)
        return out  # (a converted copy `p`: lookahead()'s note)

    # -- HIP graphs ------------------------------------------------------------------------------------
    def capture_steps(self, actions=None, steps: int = 1, policy=None):
        """Capture ``steps`` consecutive ``step()`` calls -- and, with ``policy``, the policy between them -- into ONE HIP graph
        (``torch.cuda.CUDAGraph``, which on ROCm is a hipGraph) and return a :class:`GraphedSteps` whose ``replay()`` runs them with a
        single launch.  At 65 536 CartPoles a step kernel runs ~3 us and its launch from Python costs more than that: the per-step API is
        launch-bound, and a replayed graph takes the host out of the loop.

        ``actions``: a device tensor the captured steps READ at replay time (write the next actions into it with ``copy_`` before
        ``replay()``); or ``policy``: a callable ``obs -> actions`` of torch ops, captured with the steps (its first input is the current
        observation buffer), or the string ``"random"``: every captured step is ``step(action_space.sample())`` with the batch drawn inside the
        step kernel from the action stream, whose position lives on the device and moves with every replay (``step(None)``).  Capturing executes nothing: the sub-environments advance only when the graph is replayed.  What a replay does not
        do: the host-side checks of step() (an invalid action raises at the next eager call or ``synchronize()``), and the wall-clock ``t`` of
        the episode statistics (a host value, frozen at capture).  Requires output="torch" and one eager step()/reset() before (kernels load
        on first use, which a capture must not trigger).  The reference has no counterpart: its step is a Python loop (sync_vector_env.py:253-323)."""
        self._check_open()
        self._check_not_pending("capture_steps")
        if self.output != "torch" or self._engine_factory is not None:
            raise error.Error("capture_steps() needs device tensors on a GPU: create the env with output='torch'")
        if not self._has_reset:
            raise AssertionError("Call reset before using capture_steps.")
        if self.strict_actions:
            raise error.Error("strict_actions=True synchronises after every step, which a graph capture cannot contain")
        if (self.INFO_KEYS or self.autoreset_mode == AutoresetMode.SAME_STEP or self.record_episode_statistics) and not self._device_infos:
            raise error.Error("this environment assembles its infos on the host: its step() cannot be captured")
        st = self.__dict__.get("_fused")
        if st is not None and st["chain"]:
            raise error.Error("vector wrappers are fused into this env's step kernel (their running statistics double-buffer on the host side): "
                              "its step() cannot be captured")
        if (actions is None) == (policy is None):
            raise ValueError("capture_steps() takes either `actions` (a device tensor read at replay time) or `policy` (a callable, or \"random\")")
        if policy == "random" and not hasattr(self.action_space, "hip_use_stream"):
            raise error.Error("policy=\"random\" needs the device-sampled action space")
        return GraphedSteps(self, actions, int(steps), policy)

    # -- per-sub-environment attributes: SyncVectorEnv.get_attr / set_attr (vector/sync_vector_env.py:365-398) ---------------------------
    # ENV_ATTRS: the attributes the reference's step() reads, in the engine's id order (include/mi355env.h MI_ATTR_*), as (name, default, whether
    # an np.float64 value is accepted); a default of None is the constructor's value (_env_attr_ctor).  None: no per-lane physics.  Unlike the
    # reference, set_attr does not create attributes: an unknown name raises UnknownEnvAttributeError (an AttributeError and an error.Error).
    ENV_ATTRS: tuple | None = None
    # the string-valued ones: name -> (string, row value of that string, row value of anything else, strings only).  The engine keeps a number.
    ENV_ATTR_STRINGS: dict = {}
    _env_attr_mask = 0  # bit k: attribute k was set (the engine runs the per-lane kernels once any is)

    def _env_attr_refusal(self) -> str | None:
        if self.ENV_ATTRS is None:
            return (f"{type(self).__name__}: per-sub-environment attributes (get_attr / set_attr) exist for CartPole-v1, Pendulum-v1, Acrobot-v1, "
                    "MountainCar-v0 and MountainCarContinuous-v0 only (the MuJoCo v5 classes have model fields of their own: gravity, actuator_gear, "
                    "dof_damping, geom_friction)")
        return None

    def _env_attr_id(self, name: str) -> int:
        refusal = self._env_attr_refusal()
        if refusal:
            raise error.Error(refusal)
        names = [a[0] for a in self.ENV_ATTRS]
        if name not in names:
            raise UnknownEnvAttributeError(f"{type(self).__name__} has no per-sub-environment attribute {name!r}; the supported names are "
                                           f"{', '.join(names)} (the attributes the reference's step() reads: set_attr does not create new ones)")
        return names.index(name)

    def _env_attr_validate(self, name: str, values) -> None:
        """A kind's own limits on an attribute's values (a list of Python numbers, or a 1-D device tensor): raises ValueError.  None here."""

    def _env_attr_default(self, k: int):
        name, default, _ = self.ENV_ATTRS[k]
        return self._env_attr_ctor[name] if default is None else default

    def get_attr(self, name: str) -> tuple:
        """The attribute of every sub-environment, as set_attr stored it (Python types kept); before any set_attr the reference's defaults."""
        self._check_open()
        self._check_not_pending("get_attr")
        k = self._env_attr_id(name)
        vals = self.__dict__.get("_env_attr_values", {}).get(name)
        if vals is None:
            return (self._env_attr_default(k),) * self.num_envs
        if isinstance(vals, str):  # "device": set from a device tensor, read back
            return tuple(self._engine.get_env_attr(k).tolist())
        return tuple(vals)

    def set_attr(self, name: str, values) -> None:
        """Set an attribute of the sub-environments (SyncVectorEnv.set_attr): a list or tuple gives one value per sub-environment, anything else
        one value for all; a 1-D ndarray or tensor of num_envs entries is per sub-environment too (as ``values.tolist()``; a CUDA tensor is copied
        on the device, without synchronising).  Takes effect from the next step(); reset() does not undo it.  Python numbers behave as in the
        reference; NumPy scalars are refused where NumPy 2 would round the reference's arithmetic differently for them (TypeError)."""
        self._check_open()
        self._check_not_pending("set_attr")
        k = self._env_attr_id(name)
        _, _, f64_ok = self.ENV_ATTRS[k]
        N = self.num_envs
        strings = self.ENV_ATTR_STRINGS.get(name)

        def wrong_length(n):
            return ValueError("Values must be a list or tuple with length equal to the number of environments. "
                              f"Got `{n}` values for {N} environments.")

        dev = None
        if type(values).__module__.split(".")[0] == "torch" and hasattr(values, "dim"):
            if values.dim() != 1 or values.shape[0] != N:
                raise wrong_length(values.shape[0] if values.dim() else 1)
            if values.device.type == "cuda":
                if strings is not None:
                    raise TypeError(f"set_attr({name!r}) takes strings, not a tensor")
                dev = values
            else:
                values = values.tolist()
        elif isinstance(values, np.ndarray):
            if values.ndim != 1 or values.shape[0] != N:
                raise wrong_length(values.shape[0] if values.ndim else 1)
            values = values.tolist()
        elif not isinstance(values, (list, tuple)):
            values = [values for _ in range(N)]
        if dev is None:
            if len(values) != N:
                raise wrong_length(len(values))
            if strings is not None:
                word, hit, miss, strings_only = strings
                if strings_only:
                    for v in values:
                        if not isinstance(v, str):
                            raise TypeError(f"set_attr({name!r}) takes strings, got {type(v).__name__}")
                row = np.array([hit if (isinstance(v, str) and v == word) else miss for v in values])
            else:
                for v in values:
                    if isinstance(v, np.generic):
                        if not (f64_ok and type(v) is np.float64):
                            why = ("NumPy 2 would round the reference's float32 arithmetic differently for it" if not f64_ok else
                                   "of the NumPy scalars only np.float64 is accepted here")
                            raise TypeError(f"set_attr({name!r}): a {type(v).__name__} value -- {why}; pass float(v)")
                    elif not isinstance(v, (bool, int, float)):
                        raise TypeError(f"set_attr({name!r}) takes numbers, got {type(v).__name__}")
                row = np.array([float(v) for v in values], dtype=np.float64)
        if strings is None:
            self._env_attr_validate(name, values if dev is None else dev)
        if not hasattr(self._engine.lib, "set_env_attr"):
            raise error.Error(f"set_attr({name!r}): the engine behind this env has no per-sub-environment attributes (mi_set_env_attr)")
        if dev is not None:
            t = self._torch if "_torch" in self.__dict__ else __import__("torch")
            d = dev.to(dtype=t.float64).contiguous()
            if self.output == "torch":
                self._bind_stream()  # the copy is ordered after what produced the tensor on torch's stream
            else:
                t.cuda.current_stream(d.device).synchronize()
            self._engine.set_env_attr(k, d.data_ptr(), on_device=True)
            if self.output != "torch" or d is not dev:
                self._engine.synchronize()  # (the engine's stream is not the allocator's: keep `d` alive until the copy ran)
            stored = "device"
        else:
            self._engine.set_env_attr(k, row)
            stored = list(values)
        self.__dict__.setdefault("_env_attr_values", {})[name] = stored
        self._env_attr_mask = self._env_attr_mask | (1 << k)

    # -- RepeatAction / StickyAction of the sub-environments (gymnasium_amd.wrappers.RepeatAction / StickyAction; mi_set_step_wrappers) ------
    _step_wrappers = (0, 0.0, 0)  # (num_repeats, sticky probability, sticky duration) the engine runs; 0 = no such wrapper

    _MUJOCO_KINDS = ("half_cheetah", "ant", "humanoid", "humanoid_standup", "hopper", "walker2d", "inverted_pendulum", "inverted_double_pendulum",
                     "reacher", "pusher", "swimmer")

    def _step_wrappers_refusal(self) -> str | None:
        # the eleven MuJoCo ids: trips of the plain step's launches, in the product engine (a backend without the entry point has no such step)
        has_entry = hasattr(getattr(self._engine, "lib", None), "set_step_wrappers")
        mujoco = self.KIND in self._MUJOCO_KINDS and has_entry
        if not mujoco and self.KIND not in ("cartpole", "pendulum", "acrobot", "mountain_car", "mountain_car_continuous"):
            if has_entry:
                return (f"{type(self).__name__}: RepeatAction / StickyAction of the sub-environments exist for the five classic-control ids and the "
                        "eleven MuJoCo v5 ids only (the ToyText kernels have no such step)")
            return (f"{type(self).__name__}: RepeatAction / StickyAction of the sub-environments exist for CartPole-v1, Pendulum-v1, Acrobot-v1, "
                    "MountainCar-v0 and MountainCarContinuous-v0 only (the MuJoCo and ToyText kernels have no such step)")
        if getattr(self, "_shared_rng", False):
            return "rng='shared' is the reference's NumPy CartPoleVectorEnv: it has no sub-environments that a scalar wrapper could wrap"
        if getattr(self, "fast_math", False):
            return "RepeatAction / StickyAction of the sub-environments run the exact kernels only: not with fast_math=True"
        st = self.__dict__.get("_fused")
        if st is not None and st["chain"]:
            return "vector wrappers are already fused into this env's step kernel: RepeatAction / StickyAction go directly over the env, the vector wrappers above them"
        if not hasattr(getattr(self._engine, "lib", None), "set_step_wrappers"):
            return "the engine behind this env has no per-sub-environment action wrappers (mi_set_step_wrappers)"
        return None

    def set_step_wrappers(self, num_repeats: int = 0, sticky_probability: float = 0.0, sticky_duration: int = 0) -> None:
        """What ``wrappers.RepeatAction`` / ``wrappers.StickyAction`` switch on: every sub-environment steps as if it were wrapped in
        ``RepeatAction(env, num_repeats)`` and, outside it, ``StickyAction(env, sticky_probability, sticky_duration)`` (0: no such wrapper; all
        three 0: the plain step again).  Each call constructs the wrappers anew: no sub-environment has a last action."""
        self._check_open()
        self._check_not_pending("set_step_wrappers")
        refusal = self._step_wrappers_refusal()
        if refusal:
            raise error.Error(refusal)
        if num_repeats and self._max_and_skip:
            raise error.Error("this env runs MaxAndSkipObservation, which repeats the action itself: fold the repeat into its `skip` "
                              "(env.set_max_and_skip() switches it off)")
        self._engine.set_step_wrappers(num_repeats, sticky_probability, sticky_duration)
        self._step_wrappers = (int(num_repeats), float(sticky_probability), int(sticky_duration))

    # -- MaxAndSkipObservation of the sub-environments (gymnasium_amd.wrappers.MaxAndSkipObservation; mi_set_max_and_skip) ------------------------
    _max_and_skip = 0  # the skip the engine runs; 0 = no such wrapper

    def _max_and_skip_refusal(self) -> str | None:
        if self.KIND not in ("cartpole", "pendulum", "acrobot", "mountain_car", "mountain_car_continuous"):
            return (f"{type(self).__name__}: MaxAndSkipObservation of the sub-environments exists for CartPole-v1, Pendulum-v1, Acrobot-v1, "
                    "MountainCar-v0 and MountainCarContinuous-v0 only (the MuJoCo and ToyText kernels have no inner-step loop)")
        if getattr(self, "_shared_rng", False):
            return "rng='shared' is the reference's NumPy CartPoleVectorEnv: it has no sub-environments that a scalar wrapper could wrap"
        if getattr(self, "fast_math", False):
            return "MaxAndSkipObservation of the sub-environments runs the exact kernels only: not with fast_math=True"
        st = self.__dict__.get("_fused")
        if st is not None and st["chain"]:
            return "vector wrappers are already fused into this env's step kernel: MaxAndSkipObservation goes directly over the env, the vector wrappers above it"
        if not hasattr(getattr(self._engine, "lib", None), "set_max_and_skip"):
            return "the engine behind this env has no MaxAndSkipObservation of the sub-environments (mi_set_max_and_skip)"
        return None

    def set_max_and_skip(self, skip: int = 0) -> None:
        """What ``wrappers.MaxAndSkipObservation`` switches on: every sub-environment steps as if it were wrapped in
        ``MaxAndSkipObservation(env, skip)`` (0: the plain step again).  Each call constructs the wrapper anew: all frames are zeros.  Not together
        with ``RepeatAction`` (fold the repeat into ``skip``); ``StickyAction`` goes over it."""
        self._check_open()
        self._check_not_pending("set_max_and_skip")
        refusal = self._max_and_skip_refusal()
        if refusal:
            raise error.Error(refusal)
        if skip and self._step_wrappers[0] > 0:
            raise error.Error("this env runs RepeatAction: MaxAndSkipObservation repeats the action itself, fold the repeat into `skip` "
                              "(env.set_step_wrappers() switches RepeatAction off)")
        self._engine.set_max_and_skip(skip)
        self._max_and_skip = int(skip)

    def max_and_skip_frames(self) -> np.ndarray:
        """The sub-environments' ``_obs_buffer``: float32 ``[2, num_envs, *obs_shape]`` (tests, checkpoints).  Nothing but ``set_max_and_skip``
        ever clears it: ``reset()``, a masked reset and ``set_state()`` leave it as it is."""
        self._check_open()
        self._check_not_pending("max_and_skip_frames")
        if not self._max_and_skip:
            raise error.Error("MaxAndSkipObservation is not on (set_max_and_skip)")
        dim = int(np.prod(self.single_observation_space.shape))
        return self._engine.get_max_and_skip_frames(dim).reshape((2, self.num_envs) + tuple(self.single_observation_space.shape))

    # -- bookkeeping -----------------------------------------------------------------------------------
    def statistics(self) -> dict:
        """Running totals kept on device: env_steps, reset_steps, episodes, return_sum, length_sum."""
        return self._engine.stats()

    def reset_statistics(self):
        self._engine.reset_stats()

    def get_state(self):
        """(state[N, state_dim] float64, elapsed_steps[N] int32, flags[N] uint8) -- checkpoint of the sub-environments."""
        return self._engine.get_state()

    def set_state(self, state=None, elapsed_steps=None, flags=None):
        self._engine.set_state(state, elapsed_steps, flags)
        self._has_reset = True
        if flags is not None:  # keep the host mirror of the pending-autoreset set in step with the device flags
            self._was_done = (np.asarray(flags, dtype=np.uint8) & _native.FLAG_NEEDS_RESET) != 0
            if self._device_infos:
                self._was_done_t.copy_(self._torch.from_numpy(self._was_done.copy()))

    def get_rng_state(self) -> np.ndarray:
        """Per-env PCG64 words [N, 4] = {state_hi, state_lo, inc_hi, inc_lo}."""
        return self._engine.get_rng()

    def synchronize(self):
        self._engine.synchronize()

    def _check_not_pending(self, what: str):
        """AsyncVectorEnv's state machine (vector/async_vector_env.py:340-344, 440-452): one outstanding call at a time."""
        if getattr(self, "_async_pending", None) is not None:
            raise error.AlreadyPendingCallError(f"Calling `{what}` while waiting for a pending call to `step_async` to complete.", "step")

    def _check_open(self):
        if self.closed:
            raise error.ClosedEnvironmentError(f"Trying to operate on `{type(self).__name__}`, after a call to `close()`.")

    def close_extras(self, **kwargs):
        eng = getattr(self, "_engine", None)
        if eng is not None:
            if hasattr(self.action_space, "_hip_to_host"):  # the action space outlives the env: its NumPy generator takes the stream's position back
                try:
                    self.action_space._hip_to_host()
                except Exception:
                    pass
            if getattr(self, "_async_pending", None) is not None and self._async_pending[0] == "engine":
                try:  # a step is in flight on the pinned block: collect it before the block goes away
                    eng.step_wait()
                except Exception:
                    pass
                self._async_pending = None
            if self.output == "numpy" and getattr(self, "_pinned", False):
                # The NumPy arrays handed out with copy=False (and `action_buffer`) are VIEWS of the engine's page-locked block, which
                # mi_destroy frees: replace this object's references by ordinary copies so that reading `env._obs` / the last returned
                # batch's base after close() is not a use-after-free.  (Views a caller still holds are the caller's: documented in README.)
                for name in ("_obs", "_rew", "_term", "_trunc", "_final", "_info", "_final_info", "_ep_r", "_ep_l", "action_buffer"):
                    v = getattr(self, name, None)
                    if isinstance(v, np.ndarray):
                        setattr(self, name, v.copy())
                self._pinned = False
            eng.close()
            self._engine = None


_SHORT_STEP_OWNERS = {HipVectorEnv.step}  # step() implementations that add nothing to HipVectorEnv.step's result (subclasses register theirs)


class GraphedSteps:
    """``steps`` step() calls of a :class:`HipVectorEnv` (plus the policy between them) as one HIP graph; see ``HipVectorEnv.capture_steps``.

    ``results``: the (obs, rewards, terminations, truncations, infos) tuple of every captured step -- static device tensors that each
    ``replay()`` overwrites (with ``copy=False`` the observation / reward / flag tensors of all steps are the env's own buffers, i.e. they hold
    the LAST step's values; with ``copy=True`` every step has its own).  HAZARD: a graph of ``policy="random"`` captures its steps again in the
    first ``replay()`` after an ``action_space.seed()`` that changed the generator's increment (_before_replay); ``results`` is then a NEW list of
    new tensors, and tuples kept from earlier replays are written by no launch any more -- silently.  Use what ``replay()`` returns, or read
    ``graph.results`` afresh after every replay, wherever the action space may be re-seeded."""

    def __init__(self, env: "HipVectorEnv", actions, steps: int, policy):
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if actions is not None:
            keep, _, _ = env._coerce_actions(actions)
            if keep is not actions:
                raise ValueError("the captured steps read `actions` in place at replay time: pass a contiguous tensor on the env's device with "
                                 "the action space's dtype (int64, or float32 / float64 rows for Box spaces)")
        self.env, self.steps, self.actions, self.policy = env, steps, actions, policy
        self.attr_mask = env._env_attr_mask  # which kernels the graph holds (per-lane attributes: set_attr)
        self.step_wrappers = env._step_wrappers  # ... and whose parameters they carry (RepeatAction / StickyAction: set_step_wrappers)
        self.max_and_skip = env._max_and_skip  # (MaxAndSkipObservation: set_max_and_skip)
        self._capture()

    def _prepare_capture(self):
        """What must hold before the capture opens.  policy="random": the action stream's position is on the engine with nothing drawn ahead, its
        per-lane states exist on the device (a capture cannot create them) and hold the position; the captured kernels carry the jump of the
        generator's increment, which is remembered here."""
        if self.policy == "random":
            self.env._bind_stream()
            self.env.action_space.hip_hold_on_device()
            self._inc = self.env.action_space._hip_inc

    def _capture(self):
        env, actions, policy = self.env, self.actions, self.policy
        t = env._torch
        self.graph = t.cuda.CUDAGraph()
        self.results = []
        self._prepare_capture()
        env.synchronize()
        try:
            with t.cuda.graph(self.graph):
                obs = env._obs
                for _ in range(self.steps):
                    out = env.step(actions if policy is None else (None if policy == "random" else policy(obs)))
                    obs = out[0]
                    self.results.append(out)
        finally:
            env._stream_bound = None  # (the capture bound the engine to the capture stream)
            env._bind_stream()

    def _before_replay(self):
        """The host's part of a replay before the launch.  A graph of the random policy is one more consumer of the action stream
        (vector/device_policy.py), and one the engine does not see: its kernels read and advance the per-lane states on the device.  So, unless
        the last consumer was such a replay -- then NOTHING is left to do, no engine call and no synchronisation: back-to-back replays stay
        launch-bound --, the space hands the stream over first (``hip_hold_on_device``: the NumPy generator's draws and its pending 32-bit half
        taken over, batches drawn ahead given back, the lanes re-initialised on the replay's stream where ``action_space.seed()``, a skip or a
        rollout left them behind; from then on the space keeps the account of what the launches draw).  The captured kernels carry the jump of the generator's
        INCREMENT: after a seed() that changed it the steps are captured again (``results`` are then new tensors; ``replay()`` returns them)."""
        env = self.env
        env._check_open()
        env._check_not_pending("replay")
        if env._env_attr_mask != self.attr_mask:
            raise error.Error("set_attr() has made the env read per-sub-environment attributes since this graph was captured; its kernels do not "
                              "read them: capture the steps again")
        if env._step_wrappers != getattr(self, "step_wrappers", env._step_wrappers):
            raise error.Error("RepeatAction / StickyAction of the sub-environments were switched since this graph was captured; its kernels carry the "
                              "old setting: capture the steps again")
        if env._max_and_skip != getattr(self, "max_and_skip", env._max_and_skip):
            raise error.Error("MaxAndSkipObservation of the sub-environments was switched since this graph was captured; its kernels carry the old "
                              "setting: capture the steps again")
        env._bind_stream()  # statistics() / synchronize() wait on the engine's stream: keep it the one the replay runs on
        if self.policy == "random":
            space = env.action_space
            if not space.__dict__.get("_hip_held", False):
                space.hip_use_stream()  # (the engine is seeded from the generator where a seed() is pending: `_hip_inc` is current after it)
            if space._hip_inc != self._inc:  # on EVERY replay (a tuple compare): another graph of this env may have taken the stream over since the seed()
                self._capture()
            if not space.__dict__.get("_hip_held", False):
                space.hip_hold_on_device()

    def _after_replay(self):
        """The host's part of a replay after the launch: the space notes what the launch draws (an addition, no engine call), so that the next
        consumer of another kind -- ``np_random``, ``sample()``, ``rollout()``, ``step(None)``, ``mi_action_get`` through them -- continues after it."""
        if self.policy == "random":
            self.env.action_space.hip_note_launch(self.steps)
        return self.results[-1]

    def replay(self):
        """Run the captured steps (one graph launch on torch's current stream, asynchronous like step() with device tensors); returns the
        last step's tuple."""
        self._before_replay()
        self.graph.replay()
        return self._after_replay()


def _resolve_device(device) -> int:
    """None -> LOCAL_RANK (one process per GPU) or 0; 'cuda:3' / 3 / torch.device -> index."""
    import os

    if device is None:
        return int(os.environ.get("LOCAL_RANK", "0"))
    if isinstance(device, (int, np.integer)):
        return int(device)
    s = str(device)
    if ":" in s:
        return int(s.split(":")[1])
    if s in ("cuda", "hip"):
        return 0
    return int(s)
