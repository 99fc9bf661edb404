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

Placement: directly over a ``HipVectorEnv`` or over ``RepeatAction`` / ``MaxAndSkipObservation`` / ``StickyAction`` (normalisation then sees the outer steps, as in the reference);
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

``FrameStackObservation``, ``DelayObservation`` and ``TimeAwareObservation`` (stateful_observation.py:304-461, 35-103, 106-301) are the same kind of
wrapper -- scalar, around every sub-environment, state in HBM (csrc/stateful_observation.hip) -- as layers of their own that go over the env, the
action wrappers, the two normalisers above and one another: see ``_StatefulObservation`` below.  They build their spaces on any backend and ask for
the device engine at the first call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _native
from ..gym_api import AutoresetMode, batch_space, error, spaces
from .vector import MaxAndSkipObservation, RepeatAction, StickyAction, VectorWrapper, _base_env, _close_fusion, _refuse_capture, _torch

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
        while isinstance(e, (RepeatAction, StickyAction, MaxAndSkipObservation)):
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


# -- FrameStackObservation / DelayObservation / TimeAwareObservation around every sub-environment ------------------------------------------------------
_PADDING = {"reset": 0, "zero": 1, "_custom": 2}


class _StatefulObservation(VectorWrapper):
    """What the three stateful observation wrappers of gymnasium/wrappers/stateful_observation.py:35-461 share: placement below the vector level,
    device state per sub-environment, and reset / step / rollout as ONE launch each behind the wrapped env's own (csrc/stateful_observation.hip).

    Each wrapper is its own layer: it goes over a ``HipVectorEnv`` with float32 / float64 Box observations, ``RepeatAction`` / ``StickyAction``,
    ``per_env.NormalizeObservation`` / ``NormalizeReward`` or another wrapper of this family, in any order; every vector wrapper goes above.  The
    ``per_env`` normalisers do NOT go over this family (their placement check refuses it).  It keeps its own record of the rows that finished in the
    last step (under NEXT_STEP their next step is the autoreset step: the scalar wrapper's ``reset()``).

      * ``reset``: rows outside ``options["reset_mask"]`` keep their state and return what they returned last (the wrapper keeps a reference to the
        last batch it handed out: do not modify a returned tensor in place if masked resets follow).
      * ``step``: NEXT_STEP, SAME_STEP (``infos["final_obs"]`` is the wrapper's output for the final observation, the returned observation its output
        for the reset observation) and DISABLED.
      * ``rollout``: NEXT_STEP and DISABLED, equal to T x ``step()`` in values and in the state left behind, with the state carried in from before
        (frames of the running episode, a part-filled queue, a running counter, a pending autoreset); refused under SAME_STEP.  Directly over a
        DISABLED env the trajectory is collected from T ``step()`` calls, as the normalisers do.
      * ``capture_steps``: refused.

    There is no CPU implementation: over a backend without the device engine the constructors validate their arguments and build their spaces --
    which can be inspected --, and the first ``reset`` / ``step`` / ``rollout`` raises ``error.Error``.
    ``MaxAndSkipObservation`` is an inner-step wrapper and lives in the step kernel next to ``RepeatAction`` (``wrappers.MaxAndSkipObservation``): these
    wrappers go over it as they go over ``RepeatAction``.  Out of scope: fusing these passes into
    the step / rollout kernels, rollouts under SAME_STEP, ToyText observations, the normalisers above these wrappers."""

    _what = "observations"
    _kind = None

    def __init__(self, env):
        name = type(self).__name__
        e = env
        while isinstance(e, (_StatefulObservation, _PerEnvWrapper, RepeatAction, StickyAction, MaxAndSkipObservation)):
            e = e.env
        if isinstance(e, VectorWrapper) or not hasattr(e, "_engine"):
            raise error.Error(f"per_env.{name} wraps every SUB-environment, below the vector level: it goes over a HipVectorEnv (gymnasium_amd.make_vec(...)), "
                              f"RepeatAction / StickyAction or other per_env wrappers, and the vector wrappers go above it; got {type(e).__name__}")
        space = env.single_observation_space
        if not isinstance(space, spaces.Box) or np.dtype(space.dtype) not in (np.float32, np.float64):
            raise error.Error(f"per_env.{name} takes float32 / float64 Box observations, the sub-environments have {space}")
        super().__init__(env)
        self._base, self._inner = e, env
        self._np_dtype = np.dtype(space.dtype)
        self._in_shape = tuple(space.shape)
        self._dim = int(np.prod(space.shape)) if space.shape else 1
        self._code = _native.MI_F32 if self._np_dtype == np.float32 else _native.MI_F64
        self._struct, self._allocated, self._last = None, False, None
        _close_fusion(env)

    # -- device state ---------------------------------------------------------------------------------------------------------------------
    def _dev(self):
        return getattr(self._base, "_device_index", 0)

    def _device(self):
        return _torch().device("cuda", self._dev())

    @staticmethod
    def _tdtype_of(np_dtype):
        torch = _torch()
        return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32}[np.dtype(np_dtype)]

    def _require(self):
        base = self._base
        if getattr(base, "_engine_factory", None) is not None or not hasattr(getattr(base._engine, "lib", None), "stateful_observation_step"):
            raise error.Error(f"per_env.{type(self).__name__} needs the device engine (mi_stateful_observation_step): its state lives in HBM and there is "
                              "no CPU implementation")

    def _allocate(self):
        """The state arrays, twice each: a launch reads one set and writes the other."""
        if self._allocated:
            return
        self._require()
        torch, dev, n = _torch(), self._device(), self.num_envs
        self._pending = [torch.zeros((n,), dtype=torch.uint8, device=dev) for _ in range(2)]
        self._count = [torch.zeros((n,), dtype=torch.int32, device=dev) for _ in range(2)]
        self._carried = self._carried_arrays(torch, dev, n)
        self._last = torch.zeros((n,) + self._out_row, dtype=self._tdtype_of(self._out_np_dtype), device=dev)
        s = self._struct = _native.MiStatefulObservationState()
        s.kind, s.in_dtype, s.dim, s.autoreset_mode = self._kind, self._code, self._dim, _MODES[self._base.autoreset_mode]
        s.out_dtype = {np.dtype(np.float32): _native.MI_F32, np.dtype(np.float64): _native.MI_F64, np.dtype(np.int32): _native.MI_I32}[self._out_np_dtype]
        self._configure(s)
        self._allocated = True

    def _carried_arrays(self, torch, dev, n):
        return None

    def _configure(self, s):
        pass

    def _state(self):
        self._allocate()
        s = self._struct
        s.pending_in, s.pending_out = self._pending[0].data_ptr(), self._pending[1].data_ptr()
        s.count_in, s.count_out = self._count[0].data_ptr(), self._count[1].data_ptr()
        if self._carried is not None:
            s.carried_in, s.carried_out = self._carried[0].data_ptr(), self._carried[1].data_ptr()
        return s

    def _launched(self, last):
        """After a launch: what was written is the state now."""
        self._pending.reverse(), self._count.reverse()
        if self._carried is not None:
            self._carried.reverse()
        self._last = last

    @property
    def pending_autoreset(self):
        """The rows that finished in the last step (``[N]`` bool): under NEXT_STEP their next step resets them."""
        self._allocate()
        return self._pending[0].cpu().numpy().astype(np.bool_)

    # -- staging ----------------------------------------------------------------------------------------------------------------------------
    def _stage(self, obs, steps=None):
        x, was_tensor = self._to_device(obs)
        lead = self.num_envs if steps is None else steps * self.num_envs
        if x.dtype != self._tdtype_of(self._np_dtype) or x.numel() != lead * self._dim:
            raise ValueError(f"per_env.{type(self).__name__}: expected {self._np_dtype} observations of {lead} x {self._dim} elements, got {x.dtype} "
                             f"{tuple(x.shape)}")
        if x.device != self._device():
            x = x.to(self._device())
        return x, was_tensor

    def _new_out(self, steps=None):
        lead = (self.num_envs,) if steps is None else (steps, self.num_envs)
        return _torch().empty(lead + self._out_row, dtype=self._tdtype_of(self._out_np_dtype), device=self._device())

    def _launch_step(self, is_reset, x, out, row_mask=None, fin=None, fin_out=None, fin_mask=None, te=None, tr=None):
        torch = _torch()
        dev = self._device()
        lib = _native.load_library()
        state = self._state()
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        lib.check(lib.stateful_observation_step(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(state), self.num_envs,
                                                int(is_reset), p(x), p(out), p(row_mask), p(self._last) if row_mask is not None else None, p(fin), p(fin_out),
                                                p(fin_mask), p(te), p(tr)))
        self._launched(out)

    # what the wrapper hands out for an input batch and its own output (TimeAwareObservation(flatten=False) returns a dict)
    def _wrap(self, given, out, was_tensor):
        return self._back(out, was_tensor)

    def _wrap_row(self, given_row, out_row):
        return out_row

    # -- API --------------------------------------------------------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        torch = _torch()
        self._require()
        mask = options.get("reset_mask") if options is not None else None
        mask = None if mask is None else np.ascontiguousarray(mask).view(np.uint8).copy()
        obs, infos = self.env.reset(seed=seed, options=options)
        mask_t = None if mask is None else torch.from_numpy(mask).to(self._device())
        x, was_tensor = self._stage(obs)
        out = self._new_out()
        self._launch_step(True, x, out, row_mask=mask_t)
        return self._wrap(obs, out, was_tensor), infos

    def step(self, actions):
        torch = _torch()
        self._require()
        obs, reward, terminated, truncated, infos = self.env.step(actions)
        x, was_tensor = self._stage(obs)
        out = self._new_out()
        dev = self._device()
        kw = {}
        same = self._base.autoreset_mode == AutoresetMode.SAME_STEP
        if same and "final_obs" in infos:
            fmask = infos["_final_obs"]
            if was_tensor:
                fin, fm = infos["final_obs"].contiguous(), _PerEnvWrapper._u8(fmask.contiguous())
            else:  # the NumPy infos hold an object array of the finished rows' observations
                rows = np.zeros((self.num_envs, self._dim), dtype=self._np_dtype)
                for i in np.flatnonzero(fmask):
                    rows[i] = np.asarray(infos["final_obs"][i]).reshape(-1)
                fin, fm = self._to_device(rows)[0], self._to_device(np.asarray(fmask).view(np.uint8))[0]
            kw.update(fin=fin.to(dev), fin_mask=fm.to(dev), fin_out=self._new_out())
        if not same:
            te, tr = (_PerEnvWrapper._u8(self._to_device(f)[0]) for f in (terminated, truncated))
            kw.update(te=te.to(dev), tr=tr.to(dev))
        self._launch_step(False, x, out, **kw)
        if "fin_out" in kw:
            infos = dict(infos)
            if was_tensor:
                infos["final_obs"] = self._wrap(infos["final_obs"], kw["fin_out"], True)
            else:
                host, arr = kw["fin_out"].cpu().numpy(), np.full(self.num_envs, None, dtype=object)
                for i in np.flatnonzero(infos["_final_obs"]):
                    arr[i] = self._wrap_row(infos["final_obs"][i], host[i].copy())
                infos["final_obs"] = arr
        return self._wrap(obs, out, was_tensor), reward, terminated, truncated, infos

    def rollout(self, num_steps, actions=None, **kwargs):
        """T x ``step()`` through the wrapper: the wrapped ``rollout``, then ONE launch over the whole trajectory (mi_stateful_observation_steps)."""
        torch = _torch()
        self._require()
        if self._base.autoreset_mode == AutoresetMode.SAME_STEP:
            raise error.Error(f"rollout() through per_env.{type(self).__name__} under SAME_STEP is not supported: a row that ends returns its final and its "
                              "reset observation in one step; use step(), or NEXT_STEP / DISABLED")
        if self._base.autoreset_mode == AutoresetMode.DISABLED and not isinstance(self.env, (_StatefulObservation, _PerEnvWrapper)):
            out = _PerEnvWrapper._rollout_by_steps(self, int(num_steps), actions, **kwargs)
        else:
            out = dict(self.env.rollout(num_steps, actions, **kwargs))
        steps = int(out["rewards"].shape[0])
        if steps < 1:
            return out
        x, _ = self._stage(out["obs"], steps)
        res = self._new_out(steps)
        dev = self._device()
        te, tr = (_PerEnvWrapper._u8(out[k].contiguous()) for k in ("terminations", "truncations"))
        lib = _native.load_library()
        lib.check(lib.stateful_observation_steps(dev.index, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(self._state()), steps,
                                                 self.num_envs, C.c_void_p(x.data_ptr()), C.c_void_p(res.data_ptr()), C.c_void_p(te.data_ptr()),
                                                 C.c_void_p(tr.data_ptr())))
        self._launched(res[-1].clone())  # (not a view: it would keep the whole trajectory alive)
        out["obs"] = self._wrap(out["obs"], res, True)
        return out

    def capture_steps(self, *args, **kwargs):
        _refuse_capture(self, self._what)


class FrameStackObservation(_StatefulObservation):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.FrameStackObservation(env, stack_size, padding_type=...)``
    (stateful_observation.py:304-461): observations ``[N, stack_size, ...]`` in the observations' dtype, the newest frame last.  Every reset of a row
    (``reset()``, a masked reset, the NEXT_STEP autoreset step, the SAME_STEP reset) fills ``stack_size - 1`` slots with the padding -- the reset
    observation itself (``"reset"``), zeros (``"zero"``) or a custom observation -- and the last slot with the reset observation."""

    _kind = _native.SO_FRAME_STACK

    def __init__(self, env, stack_size: int, *, padding_type="reset"):
        if not np.issubdtype(type(stack_size), np.integer):
            raise TypeError(f"The stack_size is expected to be an integer, actual type: {type(stack_size)}")
        if not 0 < stack_size:
            raise ValueError(f"The stack_size needs to be greater than zero, actual value: {stack_size}")
        super().__init__(env)
        space = env.single_observation_space
        self._padding_value = None
        if isinstance(padding_type, str) and (padding_type == "reset" or padding_type == "zero"):
            pass
        elif padding_type in space:
            self._padding_value = np.ascontiguousarray(np.asarray(padding_type, dtype=self._np_dtype).reshape(-1))
            padding_type = "_custom"
        elif isinstance(padding_type, str):
            raise ValueError(f"Unexpected `padding_type`, expected 'reset', 'zero' or a custom observation space, actual value: {padding_type!r}")
        else:
            raise ValueError(f"Unexpected `padding_type`, expected 'reset', 'zero' or a custom observation space, actual value: {padding_type!r} not an "
                             f"instance of env observation ({space})")
        self.stack_size, self.padding_type = int(stack_size), padding_type
        self._out_np_dtype, self._out_row = self._np_dtype, (self.stack_size,) + self._in_shape
        self.single_observation_space = batch_space(space, self.stack_size)
        self.observation_space = batch_space(self.single_observation_space, self.env.num_envs)

    def _configure(self, s):
        s.depth, s.padding = self.stack_size, _PADDING[self.padding_type]
        if self._padding_value is not None:
            self._padding_t = _torch().from_numpy(self._padding_value.copy()).to(self._device())
            s.padding_value = self._padding_t.data_ptr()

    def _state(self):
        s = super()._state()
        s.carried_in = self._last.data_ptr()  # the stack returned last IS the state
        return s


class DelayObservation(_StatefulObservation):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.DelayObservation(env, delay)`` (stateful_observation.py:35-103): a row's
    queue empties at every reset of the row; until it holds more than ``delay`` observations the row returns zeros, then the observation from
    ``delay`` steps earlier.  ``delay = 0`` passes the observations through."""

    _kind = _native.SO_DELAY

    def __init__(self, env, delay: int):
        if not np.issubdtype(type(delay), np.integer):
            raise TypeError(f"The delay is expected to be an integer, actual type: {type(delay)}")
        if not 0 <= delay:
            raise ValueError(f"The delay needs to be greater than zero, actual value: {delay}")
        super().__init__(env)
        self.delay = int(delay)
        self._out_np_dtype, self._out_row = self._np_dtype, self._in_shape
        self.single_observation_space = env.single_observation_space
        self.observation_space = env.observation_space

    def _carried_arrays(self, torch, dev, n):
        if self.delay == 0:
            return None
        return [torch.zeros((n, self.delay, self._dim), dtype=self._tdtype_of(self._np_dtype), device=dev) for _ in range(2)]

    def _configure(self, s):
        s.depth = self.delay


class TimeAwareObservation(_StatefulObservation):
    """``SyncVectorEnv`` over scalar envs each wrapped in ``gymnasium.wrappers.TimeAwareObservation(env, flatten, normalize_time)``
    (stateful_observation.py:106-301): every row keeps a counter that every reset of the row zeroes and every ``step()`` of the wrapper increments
    (over ``RepeatAction``: outer steps); ``max_timesteps`` is the TimeLimit the engine runs with.  ``flatten=True``: ``[N, D + 1]`` with the time in
    the last column -- int32 time makes the flattened Box float64 (exact), the normalised time ``float32(t / max_timesteps)`` keeps the observations'
    dtype.  ``flatten=False``: ``{"obs": [N, ...], "time": [N, 1]}`` in a ``Dict`` space.  ``dict_time_key`` is accepted for signature parity (no
    environment here has a Dict observation)."""

    _kind = _native.SO_TIME_AWARE

    def __init__(self, env, flatten: bool = True, normalize_time: bool = False, *, dict_time_key: str = "time"):
        super().__init__(env)
        self.flatten, self.normalize_time = flatten, normalize_time
        limit = getattr(self._base, "max_episode_steps", None)
        if not limit:
            raise ValueError("The environment must be wrapped by a TimeLimit wrapper or the spec specify a `max_episode_steps`.")
        self.max_timesteps = int(limit)
        space = env.single_observation_space
        time_space = spaces.Box(0.0, 1.0) if normalize_time else spaces.Box(0, self.max_timesteps, dtype=np.int32)
        if flatten:  # spaces/utils.py flatten_space of Dict(obs=..., time=...): the flattened bounds side by side in the common dtype
            self._out_np_dtype = np.dtype(np.result_type(space.dtype, time_space.dtype))
            self._out_row = (self._dim + 1,)
            self.single_observation_space = spaces.Box(low=np.concatenate([space.low.flatten(), time_space.low.flatten()]),
                                                       high=np.concatenate([space.high.flatten(), time_space.high.flatten()]), dtype=self._out_np_dtype)
        else:
            self._out_np_dtype, self._out_row = np.dtype(time_space.dtype), (1,)
            self.single_observation_space = spaces.Dict(obs=space, time=time_space)
        self.observation_space = batch_space(self.single_observation_space, self.env.num_envs)

    def _configure(self, s):
        s.normalize_time, s.max_timesteps = int(bool(self.normalize_time)), self.max_timesteps
        if not self.flatten:  # the launch writes the time column alone; the observations pass through untouched
            s.dim, s.in_dtype = 0, _native.MI_F32

    def _launch_step(self, is_reset, x, out, fin=None, **kw):
        if not self.flatten:
            x, fin = None, None
        super()._launch_step(is_reset, x, out, fin=fin, **kw)

    def _wrap(self, given, out, was_tensor):
        if self.flatten:
            return self._back(out, was_tensor)
        return {"obs": given, "time": self._back(out, was_tensor)}

    def _wrap_row(self, given_row, out_row):
        return out_row if self.flatten else {"obs": given_row, "time": out_row}

    @property
    def timesteps(self):
        """Every sub-environment's ``timesteps`` (stateful_observation.py:216), ``[N]`` int32."""
        self._allocate()
        return self._count[0].cpu().numpy()
