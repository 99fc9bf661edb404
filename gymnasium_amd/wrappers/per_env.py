"""gymnasium.wrappers.{NormalizeObservation, NormalizeReward} around every SUB-environment, with the batch kept in HBM.

The reference's scalar wrappers, placed around each scalar env before vectorising -- the standard PPO ``make_env`` stack -- keep ONE set of running
statistics PER sub-environment, each updated from a batch of one:

  gymnasium/wrappers/stateful_observation.py:464-561   NormalizeObservation
  gymnasium/wrappers/stateful_reward.py:20-142         NormalizeReward
  gymnasium/wrappers/utils.py:33-71                    RunningMeanStd
  gymnasium/vector/sync_vector_env.py:266-337          SyncVectorEnv.step: which rows step, which reset, final_obs

The classes here are ``SyncVectorEnv([lambda: NormalizeReward(NormalizeObservation(make(id)), gamma)] * N)`` bit for bit -- no batch reduction, every
lane runs the reference's float32 / float64 recurrence (csrc/per_env_normalize.hip) -- where ``gymnasium_amd.wrappers.NormalizeObservation`` /
``NormalizeReward`` are the VECTOR wrappers (one set of statistics over the batch).  The split is gymnasium's ``wrappers`` / ``wrappers.vector`` in
reverse: in this package the default namespace is the vector one.

Placement: directly over a ``HipVectorEnv`` or over ``RepeatAction`` / ``StickyAction`` (normalisation then sees the outer steps, as in the reference);
one may sit on the other, in either order, with identical results; every vector wrapper (``ClipReward``, ``TransformObservation``,
``RecordEpisodeStatistics``, ``ClipAction`` ...) goes above.  A ``step()`` of the pair is ONE launch behind the env's own; ``rollout(T)`` is one launch
behind the rollout's.  Device tensors pass straight through; NumPy batches are staged through the device (a correctness path).

  * ``reset``: every row that resets updates its statistics from its reset observation; with ``options={"reset_mask": m}`` the rows outside the mask
    keep their statistics and return the normalised observation they returned last.  The wrapper keeps a reference to the last batch it handed out
    for that purpose (device tensors are not copied: do not modify a returned observation tensor in place if masked resets follow).
  * ``step``: NEXT_STEP, SAME_STEP (the final observation of a row that ends updates the statistics and is normalised -- ``infos["final_obs"]`` --
    then its reset observation: two updates in one call) and DISABLED.  Under NEXT_STEP a row in its autoreset step gets reward 0.0 and its return
    statistics and accumulator are left alone.  The accumulator is cleared by ``terminated`` only, never by a reset or a truncation.
  * ``rollout``: NEXT_STEP and DISABLED.  REFUSED under SAME_STEP (``error.Error``): the final observations update the statistics between two steps.
    The engine has no rollout launch for a DISABLED env (a finished row waits for the caller's reset), so there the trajectory is collected from T
    ``step()`` calls of the wrapped env and the statistics pass is still the one launch over all T steps.
  * ``capture_steps``: refused, like the other observation / reward wrappers.

Statistics: ``w.obs_rms`` / ``w.return_rms`` have ``.mean``, ``.var``, ``.count`` with a leading ``num_envs`` axis (float32 ``[N, D]`` for float32
observations, float64 for float64 ones; ``count`` float64 ``[N]``), readable (a device-to-host copy) and assignable (checkpointing);
``NormalizeReward.discounted_reward`` (``[N]`` float64) and ``.pending_autoreset`` (``[N]`` bool: the rows that finished in the last step) complete
a checkpoint.  ``update_running_mean`` is one bool for the whole batch.  float64 observations: the reference's statistics are float32 arrays until
their first update, which makes that update's ``var * count`` a float32 product; reproduced per row, and assigning ``obs_rms`` statistics ends that
state for all rows.  Normalising float64 observations with ``update_running_mean = False`` BEFORE any update computes ``var + epsilon`` in float64
(the reference: in float32) -- outside the tested domain.

There is no CPU implementation: over a backend without the device engine the constructors validate their arguments and then raise ``error.Error``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native
from ..gym_api import AutoresetMode, batch_space, error, spaces
from .vector import RepeatAction, StickyAction, VectorWrapper, _base_env, _close_fusion, _refuse_capture, _torch

_MODES = {AutoresetMode.NEXT_STEP: 0, AutoresetMode.SAME_STEP: 1, AutoresetMode.DISABLED: 2}


def _require_device_engine(base, what):
    if getattr(base, "_engine_factory", None) is not None or not hasattr(getattr(base._engine, "lib", None), "per_env_normalize_step"):
        raise error.Error(f"{what} of gymnasium_amd.wrappers.per_env needs the device engine (mi_per_env_normalize_step): the statistics live in HBM and "
                          "there is no CPU implementation")


class PerEnvRunningMeanStd:
    """``mean`` / ``var`` / ``count`` of every sub-environment's RunningMeanStd, read from and written to the device arrays of the wrapper."""

    def __init__(self, get, put):
        self._get, self._put = get, put

    mean = property(lambda self: self._get("mean"), lambda self, v: self._put("mean", v))
    var = property(lambda self: self._get("var"), lambda self, v: self._put("var", v))
    count = property(lambda self: self._get("count"), lambda self, v: self._put("count", v))


class _PerEnvWrapper(VectorWrapper):
    """What the two classes share: placement, the state struct of the pair, and reset / step / rollout of the pair in one launch each."""

    _what = None  # "observations" / "rewards"

    def __init__(self, env):
        name = type(self).__name__
        partner, inner = None, env
        if isinstance(inner, _PerEnvWrapper):
            if type(inner) is type(self):
                raise error.Error(f"the sub-environments are already wrapped in per_env.{name}: at most one of each")
            partner, inner = inner, inner.env
        e = inner
        if isinstance(e, _PerEnvWrapper):
            raise error.Error(f"the sub-environments are already wrapped in per_env.NormalizeObservation and per_env.NormalizeReward: at most one of each")
        while isinstance(e, (RepeatAction, StickyAction)):
            e = e.env
        if isinstance(e, VectorWrapper) or not hasattr(e, "_engine"):
            raise error.Error(f"per_env.{name} wraps every SUB-environment, below the vector level: it goes directly over a HipVectorEnv "
                              f"(gymnasium_amd.make_vec(...)), RepeatAction / StickyAction or the other per_env wrapper, and the vector wrappers go above it; "
                              f"got {type(e).__name__}")
        super().__init__(env)
        self._partner, self._inner, self._base = partner, inner, e
        self._update_running_mean = True
        self._struct = None
        self._allocated = False

    @property
    def update_running_mean(self) -> bool:
        return self._update_running_mean

    @update_running_mean.setter
    def update_running_mean(self, setting: bool):
        self._update_running_mean = setting

    # -- the pair -------------------------------------------------------------------------------------------------------------------------
    def _pair(self):
        """(the NormalizeObservation, the NormalizeReward) a call entered through this wrapper runs; either may be None."""
        both = (self, self._partner)
        on = next((w for w in both if isinstance(w, NormalizeObservation)), None)
        rn = next((w for w in both if isinstance(w, NormalizeReward)), None)
        return on, rn

    def _device(self):
        return _torch().device("cuda", getattr(self._base, "_device_index", 0))

    def _state(self, on, rn):
        """The mi_per_env_state of the pair with this call's settings."""
        s = self._struct
        if s is None:
            s = self._struct = _native.MiPerEnvState()
            s.autoreset_mode = _MODES[self._base.autoreset_mode]
        if on is not None and not s.obs_mean:  # (the arrays never move once allocated: their addresses are filled in once)
            on._allocate()
            s.obs_mean, s.obs_var, s.obs_count, s.obs_first = on._mean.data_ptr(), on._var.data_ptr(), on._count.data_ptr(), on._first.data_ptr()
            s.obs_dtype, s.obs_dim = on._code, on._dim
        if rn is not None and not s.ret_mean:
            rn._allocate()
            s.acc, s.ret_mean, s.ret_var, s.ret_count = rn._acc.data_ptr(), rn._mean.data_ptr(), rn._var.data_ptr(), rn._count.data_ptr()
            s.was_done = rn._was_done.data_ptr()
        if on is not None:
            s.obs_phase, s.obs_update, s.obs_epsilon = on._phase, int(bool(on._update_running_mean)), float(on.epsilon)
        if rn is not None:
            s.gamma, s.reward_epsilon, s.reward_update = float(rn.gamma), float(rn.epsilon), int(bool(rn._update_running_mean))
        return s

    def _stage_obs(self, on, obs):
        torch = _torch()
        x, was_tensor = self._to_device(obs)
        if x.dtype != on._tdtype or x.numel() != self.num_envs * on._dim:
            raise ValueError(f"per_env.NormalizeObservation: expected {on._tdtype} observations of {self.num_envs} x {on._dim} elements, got {x.dtype} "
                             f"{tuple(x.shape)}")
        if x.device != self._device():
            x = x.to(self._device())
        return x, was_tensor, torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)

    @staticmethod
    def _u8(t):
        torch = _torch()
        return t.view(torch.uint8) if t.dtype == torch.bool else t

    def _launch_step(self, on, rn, x=None, out=None, row_mask=None, prev=None, fin=None, fin_out=None, fin_mask=None, r=None, te=None, tr=None, r_out=None):
        torch = _torch()
        dev = self._device()
        lib = _native.load_library()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        lib.check(lib.per_env_normalize_step(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(self._state(on, rn)), self.num_envs,
                                             p(x), p(out), p(row_mask), p(prev), p(fin), p(fin_out), p(fin_mask), p(r), p(te), p(tr), p(r_out)))
        if x is not None:
            on._phase ^= 1
            on._last = out

    # -- API ------------------------------------------------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        torch = _torch()
        on, rn = self._pair()
        obs, infos = self._inner.reset(seed=seed, options=options)
        mask = options.get("reset_mask") if options is not None else None
        mask_t = None
        if mask is not None:
            mask_t = torch.from_numpy(np.ascontiguousarray(mask).view(np.uint8).copy()).to(self._device())
        if rn is not None:  # sync_vector_env.py:233-250: the rows that reset leave the pending-autoreset set
            rn._allocate()
            rn._was_done.zero_() if mask_t is None else rn._was_done.mul_(1 - mask_t)
        if on is None:
            return obs, infos
        x, was_tensor, out = self._stage_obs(on, obs)
        prev = None
        if mask_t is not None:
            prev = on._last
            if prev is None:  # (a masked reset as the very first call: the rows outside the mask have returned nothing yet)
                out.zero_()
        self._launch_step(on, None, x=x, out=out, row_mask=mask_t, prev=prev)
        return self._back(out, was_tensor), infos

    def step(self, actions):
        torch = _torch()
        on, rn = self._pair()
        obs, reward, terminated, truncated, infos = self._inner.step(actions)
        kw = {}
        obs_tensor = rew_tensor = True
        if on is not None:
            x, obs_tensor, out = self._stage_obs(on, obs)
            kw.update(x=x, out=out)
            if self._base.autoreset_mode == AutoresetMode.SAME_STEP and "final_obs" in infos:
                fmask = infos["_final_obs"]
                if obs_tensor:
                    fin, fm = infos["final_obs"].contiguous(), self._u8(fmask.contiguous())
                else:  # the NumPy infos hold an object array of the finished rows' observations
                    rows = np.zeros((self.num_envs, on._dim), dtype=on._np_dtype)
                    for i in np.flatnonzero(fmask):
                        rows[i] = np.asarray(infos["final_obs"][i]).reshape(-1)
                    fin, fm = self._to_device(rows)[0], self._to_device(np.asarray(fmask).view(np.uint8))[0]
                kw.update(fin=fin, fin_mask=fm, fin_out=torch.empty((self.num_envs, on._dim), dtype=torch.float32, device=x.device))
        if rn is not None:
            r, rew_tensor = self._to_device(reward, np.float64)
            te, tr = self._u8(self._to_device(terminated)[0]), self._u8(self._to_device(truncated)[0])
            if r.dtype != torch.float64:
                r = r.to(torch.float64)
            dev = self._device()
            r, te, tr = (t if t.device == dev else t.to(dev) for t in (r, te, tr))
            kw.update(r=r, te=te, tr=tr, r_out=torch.empty_like(r))
        self._launch_step(on, rn, **kw)
        if on is not None:
            obs = self._back(kw["out"], obs_tensor)
            if "fin_out" in kw:
                infos = dict(infos)
                if obs_tensor:
                    infos["final_obs"] = kw["fin_out"].reshape(infos["final_obs"].shape)
                else:
                    host, arr = kw["fin_out"].cpu().numpy(), np.full(self.num_envs, None, dtype=object)
                    for i in np.flatnonzero(infos["_final_obs"]):
                        arr[i] = host[i].reshape(self._base.single_observation_space.shape).copy()
                    infos["final_obs"] = arr
        if rn is not None:
            reward = self._back(kw["r_out"], rew_tensor)
        return obs, reward, terminated, truncated, infos

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` through the pair: the wrapped ``rollout``, then ONE launch in which every (row, column) walks the T steps with its statistics
        in registers (mi_per_env_normalize_steps).  float32 observations and the rewards are normalised in place (the tensors are the rollout's own)."""
        torch = _torch()
        on, rn = self._pair()
        if self._base.autoreset_mode == AutoresetMode.SAME_STEP:
            raise error.Error(f"rollout() through per_env.{type(self).__name__} under SAME_STEP is not supported: the final observation of a row that ends "
                              "updates its statistics between two steps; use step(), or NEXT_STEP / DISABLED")
        if self._base.autoreset_mode == AutoresetMode.DISABLED:
            out = self._rollout_by_steps(int(num_steps), actions, **kwargs)
        else:
            out = dict(self._inner.rollout(num_steps, actions, **kwargs))
        steps = int(out["rewards"].shape[0])
        if steps < 1:
            return out
        x = res = r = te = tr = None
        if on is not None:
            x = out["obs"].contiguous()
            if x.dtype != on._tdtype or x.numel() != steps * self.num_envs * on._dim:
                raise ValueError(f"per_env.NormalizeObservation: expected a {on._tdtype} trajectory of {steps} x {self.num_envs} x {on._dim} elements, got "
                                 f"{x.dtype} {tuple(x.shape)}")
            res = x if x.dtype == torch.float32 else torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
        if rn is not None:
            r = out["rewards"].to(torch.float64).contiguous()
            te, tr = self._u8(out["terminations"].contiguous()), self._u8(out["truncations"].contiguous())
        dev = self._device()
        lib = _native.load_library()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        lib.check(lib.per_env_normalize_steps(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(self._state(on, rn)), steps,
                                              self.num_envs, p(x), p(res), p(r), p(te), p(tr), p(r)))
        if on is not None:
            on._phase ^= 1
            on._last = res[-1].clone()  # (not a view: it would keep the whole trajectory alive)
            out["obs"] = res
        if rn is not None:
            out["rewards"] = r
        return out

    def _rollout_by_steps(self, steps, actions, return_actions=True, infos=False):
        """The trajectory of a DISABLED env, whose engine has no rollout launch (a finished row must be reset by the caller): ``steps`` of the wrapped
        env's own ``step()`` collected into time-major device tensors, as ``HipVectorEnv.rollout`` lays them out."""
        torch = _torch()
        base = self._base
        if base.output != "torch":
            raise error.Error("rollout() returns device tensors; create the env with output='torch'")
        if infos:
            raise error.Error(f"rollout(infos=True) through per_env.{type(self).__name__} under DISABLED autoreset is not supported")
        if steps < 1:
            raise ValueError(f"rollout() under DISABLED autoreset needs num_steps >= 1, got {steps}")
        if actions is not None and len(actions) != steps:
            raise ValueError(f"actions must hold {steps} batches, got {len(actions)}")
        out, taken = None, []
        for t in range(steps):
            a = self.action_space.sample() if actions is None else actions[t]
            o, r, te, tr, _ = self._inner.step(a)
            if out is None:
                out = {k: torch.empty((steps,) + tuple(v.shape), dtype=v.dtype, device=v.device)
                       for k, v in (("obs", o), ("rewards", r), ("terminations", te), ("truncations", tr))}
            out["obs"][t].copy_(o), out["rewards"][t].copy_(r), out["terminations"][t].copy_(te), out["truncations"][t].copy_(tr)
            taken.append(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)))
        if return_actions:
            out["actions"] = torch.stack(taken).to(out["obs"].device)
        return out

    def capture_steps(self, *args, **kwargs):
        _refuse_capture(self, self._what)

    # -- device arrays <-> NumPy --------------------------------------------------------------------------------------------------------------
    def _read(self, tensor):
        return tensor.cpu().numpy()

    def _write(self, tensor, value, np_dtype):
        torch = _torch()
        host = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np_dtype), tuple(tensor.shape)))
        tensor.copy_(torch.from_numpy(host.copy()))


class NormalizeObservation(_PerEnvWrapper):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.NormalizeObservation(env, epsilon)`` (stateful_observation.py:464-561):
    per-sub-environment ``obs_rms``, updated from every observation the sub-environment's ``reset()`` or ``step()`` returns, output float32.  Box
    observations in float32 (classic control) or float64 (MuJoCo)."""

    _what = "observations"

    def __init__(self, env, epsilon: float = 1e-8):
        if epsilon <= 0:
            raise error.InvalidBound(f"`epsilon` should be strictly positive. Received {epsilon}")
        super().__init__(env)
        space = self.env.single_observation_space
        if not isinstance(space, spaces.Box) or np.dtype(space.dtype) not in (np.float32, np.float64):
            raise error.Error(f"per_env.NormalizeObservation normalises float32 / float64 Box observations, the sub-environments have {space}: put "
                              "FlattenObservation between them (one-hot rows) and use the vector NormalizeObservation above it")
        _require_device_engine(self._base, "NormalizeObservation")
        self.epsilon = epsilon
        self._np_dtype = np.dtype(space.dtype)
        self._dim = int(np.prod(space.shape)) if space.shape else 1
        self._shape = tuple(space.shape)
        self._code = _native.MI_F32 if self._np_dtype == np.float32 else _native.MI_F64
        self.single_observation_space = spaces.Box(low=-np.inf, high=np.inf, shape=space.shape, dtype=np.float32)
        self.observation_space = batch_space(self.single_observation_space, self.env.num_envs)
        self._phase, self._last = 0, None
        self.obs_rms = PerEnvRunningMeanStd(self._get_stat, self._put_stat)
        _close_fusion(self.env)

    @property
    def _tdtype(self):
        torch = _torch()
        return torch.float32 if self._np_dtype == np.float32 else torch.float64

    def _allocate(self):
        if not self._allocated:
            torch, dev, n = _torch(), self._device(), self.env.num_envs
            self._mean = torch.zeros((n, self._dim), dtype=self._tdtype, device=dev)
            self._var = torch.ones((n, self._dim), dtype=self._tdtype, device=dev)
            self._count = torch.full((2, n), 1e-4, dtype=torch.float64, device=dev)  # double-buffered: half `_phase` is current
            self._first = torch.ones((2, n), dtype=torch.uint8, device=dev)
            self._allocated = True

    def _get_stat(self, name):
        self._allocate()
        if name == "count":
            return self._read(self._count[self._phase])
        return self._read(self._mean if name == "mean" else self._var).reshape((self.env.num_envs,) + self._shape)

    def _put_stat(self, name, value):
        self._allocate()
        if name == "count":
            self._write(self._count[self._phase], value, np.float64)
        else:
            value = np.asarray(value, dtype=self._np_dtype)
            if value.shape == (self.env.num_envs,) + self._shape:
                value = value.reshape(self.env.num_envs, self._dim)
            self._write(self._mean if name == "mean" else self._var, value, self._np_dtype)
        self._first.zero_()  # assigned statistics are arrays of the observations' dtype: the float32 first update is over


class NormalizeReward(_PerEnvWrapper):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.NormalizeReward(env, gamma, epsilon)`` (stateful_reward.py:20-142):
    per-sub-environment discounted return and ``return_rms``, all float64; works for every env id."""

    _what = "rewards"

    def __init__(self, env, gamma: float = 0.99, epsilon: float = 1e-8):
        if not 0 <= gamma <= 1:
            raise error.InvalidBound(f"`gamma` should be in the interval [0, 1]. Received {gamma}")
        if epsilon <= 0:
            raise error.InvalidBound(f"`epsilon` should be strictly positive. Received {epsilon}")
        super().__init__(env)
        _require_device_engine(self._base, "NormalizeReward")
        self.gamma, self.epsilon = gamma, epsilon
        self.return_rms = PerEnvRunningMeanStd(self._get_stat, self._put_stat)
        _close_fusion(self.env)

    def _allocate(self):
        if not self._allocated:
            torch, dev, n = _torch(), self._device(), self.env.num_envs
            self._acc = torch.zeros((n,), dtype=torch.float64, device=dev)
            self._mean = torch.zeros((n,), dtype=torch.float64, device=dev)
            self._var = torch.ones((n,), dtype=torch.float64, device=dev)
            self._count = torch.full((n,), 1e-4, dtype=torch.float64, device=dev)
            self._was_done = torch.zeros((n,), dtype=torch.uint8, device=dev)
            self._allocated = True

    def _get_stat(self, name):
        self._allocate()
        return self._read({"mean": self._mean, "var": self._var, "count": self._count}[name])

    def _put_stat(self, name, value):
        self._allocate()
        self._write({"mean": self._mean, "var": self._var, "count": self._count}[name], value, np.float64)

    @property
    def discounted_reward(self):
        """Every sub-environment's ``discounted_reward`` (stateful_reward.py:112), ``[N]`` float64."""
        self._allocate()
        return self._read(self._acc)

    @discounted_reward.setter
    def discounted_reward(self, value):
        self._allocate()
        self._write(self._acc, value, np.float64)

    @property
    def pending_autoreset(self):
        """The rows that finished in the last step (``[N]`` bool): under NEXT_STEP their next step is the autoreset step, which this wrapper skips."""
        self._allocate()
        return self._read(self._was_done).astype(np.bool_)

    @pending_autoreset.setter
    def pending_autoreset(self, value):
        self._allocate()
        self._write(self._was_done, np.asarray(value, dtype=np.bool_), np.uint8)
