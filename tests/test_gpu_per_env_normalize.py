"""-m gpu: wrappers.per_env.NormalizeObservation / NormalizeReward -- one set of running statistics per sub-environment, csrc/per_env_normalize.hip --
against the reference's SyncVectorEnv over scalar envs each wrapped in gymnasium.wrappers.NormalizeReward(NormalizeObservation(env)), bit for bit.

The fixtures per_env_normalize_<id>_<mode>.npz were recorded from the reference (tests/golden/make_golden_per_env_normalize.py): 70 sub-environments
(a wavefront and a partial one), 80 steps, CartPole / Pendulum / MountainCarContinuous with short episodes, the three autoreset modes, and a float64
stream through the scalar wrappers that shows the first-update quirk.  Where no fixture exists the NumPy restatement (tests/per_env_normalize_cases.py,
pinned to the fixtures by tests/test_per_env_normalize_host.py) is applied to the raw outputs of an unwrapped env with the same seeds and actions.
Every comparison is array_equal: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import error
from gymnasium_amd.wrappers import per_env

import per_env_normalize_cases as cases

pytestmark = pytest.mark.gpu

N, T, GAMMA, SEED = cases.N, cases.T, cases.GAMMA, cases.SEED
MODES = {"next": "NextStep", "same": "SameStep", "disabled": "Disabled"}
KEYS = [(k, m) for k in cases.IDS for m in cases.MODES]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def pair(env, order="obs_inside", gamma=GAMMA):
    if order == "obs_inside":
        return per_env.NormalizeReward(per_env.NormalizeObservation(env), gamma=gamma)
    return per_env.NormalizeObservation(per_env.NormalizeReward(env, gamma=gamma))


def build(key, mode, output="torch", order="obs_inside", **kw):
    kw.setdefault("max_episode_steps", cases.LIMITS[key])
    return pair(gymnasium_amd.make_vec(cases.IDS[key], num_envs=N, output=output, autoreset_mode=MODES[mode], **kw), order)


def actions_of(fix, t, output):
    a = fix["actions"][t]
    if output == "torch":
        import torch

        return torch.from_numpy(a).cuda()
    return a


def check_statistics(w, fix):
    assert w.obs_rms.mean.dtype == fix["obs_mean"].dtype and w.obs_rms.count.dtype == np.float64
    for name, have in (("obs_mean", w.obs_rms.mean), ("obs_var", w.obs_rms.var), ("obs_count", w.obs_rms.count), ("ret_mean", w.return_rms.mean),
                       ("ret_var", w.return_rms.var), ("ret_count", w.return_rms.count), ("acc", w.discounted_reward)):
        assert np.array_equal(have, fix[name]), name


def check_final_obs(infos, fix, t):
    fm = fix["final_mask"][t]
    if not fm.any() and "_final_obs" not in infos:  # (the NumPy infos carry the key only in a step that finished an episode)
        return
    assert np.array_equal(host(infos["_final_obs"]).astype(bool), fm), ("final mask", t)
    for i in np.flatnonzero(fm):
        got = host(infos["final_obs"][i])
        assert got.dtype == np.float32 and np.array_equal(got, fix["final_obs"][t][i]), ("final_obs", t, i)


def run_against_fixture(w, fix, mode, output):
    obs0, _ = w.reset(seed=SEED)
    assert host(obs0).dtype == np.float32 and np.array_equal(host(obs0), fix["obs0"])
    for t in range(T):
        o, r, te, tr, infos = w.step(actions_of(fix, t, output))
        assert np.array_equal(host(te), fix["term"][t]) and np.array_equal(host(tr), fix["trunc"][t]), ("flags", t)
        assert host(o).dtype == np.float32 and np.array_equal(host(o), fix["obs"][t]), ("obs", t)
        assert host(r).dtype == np.float64 and np.array_equal(host(r), fix["reward"][t]), ("reward", t)
        if mode == "same":
            check_final_obs(infos, fix, t)
        if mode == "disabled" and fix["reset_mask"][t].any():
            ro, _ = w.reset(options={"reset_mask": fix["reset_mask"][t].copy()})
            assert np.array_equal(host(ro), fix["reset_obs"][t]), ("masked reset", t)
    check_statistics(w, fix)


# -- 1. golden parity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,mode", KEYS)
def test_golden_parity_device_tensors(key, mode):
    fix = cases.fixture(f"{key}_{mode}")
    w = build(key, mode)
    run_against_fixture(w, fix, mode, "torch")
    w.close()


# -- 2. stacking order, NumPy batches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["obs_inside", "reward_inside"])
@pytest.mark.parametrize("key,mode", [("cartpole", "same"), ("pendulum", "next"), ("mountaincar_continuous", "disabled")])
def test_stacking_order_numpy_batches(key, mode, order):
    fix = cases.fixture(f"{key}_{mode}")
    w = build(key, mode, output="numpy", order=order)
    run_against_fixture(w, fix, mode, "numpy")
    w.close()


# -- 3. rollouts --------------------------------------------------------------------------------------------------------------------------------------
def check_rollout(out, fix, a, b):
    assert out["obs"].dtype.is_floating_point and host(out["obs"]).dtype == np.float32
    assert np.array_equal(host(out["terminations"]), fix["term"][a:b]) and np.array_equal(host(out["truncations"]), fix["trunc"][a:b])
    assert np.array_equal(host(out["obs"]), fix["obs"][a:b]), ("rollout obs", a, b)
    assert np.array_equal(host(out["rewards"]), fix["reward"][a:b]), ("rollout rewards", a, b)


@pytest.mark.parametrize("key", list(cases.IDS))
def test_rollout_equals_the_fixture_next_step(key):
    import torch

    fix = cases.fixture(f"{key}_next")
    w = build(key, "next")
    obs0, _ = w.reset(seed=SEED)
    assert np.array_equal(host(obs0), fix["obs0"])
    check_rollout(w.rollout(T, torch.from_numpy(fix["actions"]).cuda()), fix, 0, T)
    check_statistics(w, fix)
    w.close()


@pytest.mark.parametrize("key", list(cases.IDS))
def test_rollout_equals_the_fixture_disabled(key):
    """DISABLED: the caller resets the rows that ended, so the fixture is a sequence of rollouts between its masked resets."""
    import torch

    fix = cases.fixture(f"{key}_disabled")
    w = build(key, "disabled")
    obs0, _ = w.reset(seed=SEED)
    assert np.array_equal(host(obs0), fix["obs0"])
    acts = torch.from_numpy(fix["actions"]).cuda()
    a, longest = 0, 0
    for t in range(T):
        if fix["reset_mask"][t].any() or t == T - 1:
            check_rollout(w.rollout(t + 1 - a, acts[a:t + 1]), fix, a, t + 1)
            longest, a = max(longest, t + 1 - a), t + 1
            if fix["reset_mask"][t].any():
                ro, _ = w.reset(options={"reset_mask": fix["reset_mask"][t].copy()})
                assert np.array_equal(host(ro), fix["reset_obs"][t]), ("masked reset", t)
    assert longest >= (7 if key == "pendulum" else 1)
    check_statistics(w, fix)
    w.close()


@pytest.mark.parametrize("key,mode,limit,CUT", [("cartpole", "next", 30, 40), ("pendulum", "next", 7, 40), ("pendulum", "next", 7, 39),
                                                ("pendulum", "disabled", None, 40)])
def test_two_rollouts_equal_the_steps(key, mode, limit, CUT):
    """rollout(40) twice against 80 step() calls on a second env with the same seeds: values, statistics, accumulator and the carried flags.  Also
    cut after 39 steps: Pendulum's rows (limit 7 under NEXT_STEP: a cycle of 8) all truncate in step 39, so the second rollout starts with their
    autoreset step.  DISABLED at the id's own limit: nothing finishes within 80 steps."""
    import torch

    fix = cases.fixture(f"{key}_next")
    kw = {"max_episode_steps": limit} if limit else {"max_episode_steps": None}
    a_env, b_env = build(key, mode, **kw), build(key, mode, **kw)
    acts = torch.from_numpy(fix["actions"]).cuda()
    oa, _ = a_env.reset(seed=SEED)
    ob, _ = b_env.reset(seed=SEED)
    assert np.array_equal(host(oa), host(ob))
    first, second = a_env.rollout(CUT, acts[:CUT]), a_env.rollout(T - CUT, acts[CUT:])
    if CUT == 39:  # the first rollout ends on a step that finishes rows
        assert (host(first["terminations"][-1]) | host(first["truncations"][-1])).any()
    for t in range(T):
        o, r, te, tr, _ = b_env.step(acts[t])
        src, k = (first, t) if t < CUT else (second, t - CUT)
        assert np.array_equal(host(src["obs"][k]), host(o)) and np.array_equal(host(src["rewards"][k]), host(r)), t
        assert np.array_equal(host(src["terminations"][k]), host(te)) and np.array_equal(host(src["truncations"][k]), host(tr)), t
    for name in ("mean", "var", "count"):
        assert np.array_equal(getattr(a_env.obs_rms, name), getattr(b_env.obs_rms, name)), name
        assert np.array_equal(getattr(a_env.return_rms, name), getattr(b_env.return_rms, name)), name
    assert np.array_equal(a_env.discounted_reward, b_env.discounted_reward) and np.array_equal(a_env.pending_autoreset, b_env.pending_autoreset)
    # ... and the two go on alike
    o1, r1 = a_env.step(acts[0])[:2]
    o2, r2 = b_env.step(acts[0])[:2]
    assert np.array_equal(host(o1), host(o2)) and np.array_equal(host(r1), host(r2))
    a_env.close(), b_env.close()


def test_same_step_rollout_is_refused():
    w = build("cartpole", "same")
    w.reset(seed=SEED)
    with pytest.raises(error.Error, match="SAME_STEP"):
        w.rollout(4)
    w.close()


# -- 4. the float64 stream straight through the two ABI calls -----------------------------------------------------------------------------------------
class DeviceState:
    """mi_per_env_state over torch tensors, as wrappers/per_env.py lays it out."""

    def __init__(self, n, dim, dtype, mode, gamma=GAMMA, epsilon=1e-8):
        import torch

        self.torch, self.lib, self.n, self.dim = torch, _native.load_library(), n, dim
        self.tdtype = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
        z = lambda *shape, **kw: torch.zeros(shape, device="cuda", **kw)  # noqa: E731
        self.mean, self.var = z(n, dim, dtype=self.tdtype), z(n, dim, dtype=self.tdtype) + 1
        self.count, self.first = z(2, n, dtype=torch.float64) + 1e-4, z(2, n, dtype=torch.uint8) + 1
        self.acc, self.rmean, self.rvar, self.rcount = (z(n, dtype=torch.float64) + v for v in (0.0, 0.0, 1.0, 1e-4))
        self.was_done = z(n, dtype=torch.uint8)
        s = self.s = _native.MiPerEnvState()
        s.obs_mean, s.obs_var, s.obs_count, s.obs_first = (t.data_ptr() for t in (self.mean, self.var, self.count, self.first))
        s.obs_phase, s.obs_dtype, s.obs_dim, s.obs_update, s.obs_epsilon = 0, (_native.MI_F32 if self.tdtype == torch.float32 else _native.MI_F64), dim, 1, epsilon
        s.acc, s.ret_mean, s.ret_var, s.ret_count, s.was_done = (t.data_ptr() for t in (self.acc, self.rmean, self.rvar, self.rcount, self.was_done))
        s.gamma, s.reward_epsilon, s.reward_update, s.autoreset_mode = gamma, epsilon, 1, _native.AUTORESET[MODES[mode]]
        self.last = None

    def dev(self, a, dtype=None):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8) if a.dtype == np.bool_ else a).cuda()

    @staticmethod
    def p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def step(self, x, mask=None, reward=None, term=None, trunc=None):
        torch = self.torch
        x = self.dev(x)
        out = torch.zeros((self.n, self.dim), dtype=torch.float32, device="cuda")
        m = None if mask is None else self.dev(mask)
        r = te = tr = r_out = None
        if reward is not None:
            r, te, tr = self.dev(reward), self.dev(term), self.dev(trunc)
            r_out = torch.empty_like(r)
        self.lib.check(self.lib.per_env_normalize_step(0, self.stream(), C.byref(self.s), self.n, self.p(x), self.p(out), self.p(m),
                                                       self.p(self.last if m is not None else None), None, None, None, self.p(r), self.p(te), self.p(tr),
                                                       self.p(r_out)))
        self.s.obs_phase ^= 1
        self.last = out
        return host(out), (None if r_out is None else host(r_out))

    def steps(self, x, reward, term, trunc):
        torch = self.torch
        x, r, te, tr = self.dev(x), self.dev(reward), self.dev(term), self.dev(trunc)
        out = torch.empty(tuple(x.shape), dtype=torch.float32, device="cuda")
        self.lib.check(self.lib.per_env_normalize_steps(0, self.stream(), C.byref(self.s), int(x.shape[0]), self.n, self.p(x), self.p(out), self.p(r),
                                                        self.p(te), self.p(tr), self.p(r)))
        self.s.obs_phase ^= 1
        self.last = out[-1].clone()
        return host(out), host(r)

    def statistics(self):
        return dict(obs_mean=host(self.mean), obs_var=host(self.var), obs_count=host(self.count[self.s.obs_phase]), ret_mean=host(self.rmean),
                    ret_var=host(self.rvar), ret_count=host(self.rcount), acc=host(self.acc))


@pytest.mark.parametrize("how", ["per_step", "trajectory"])
def test_float64_replay_through_the_abi(how):
    fix = cases.fixture("float64_replay")
    steps, n, dim = fix["raw_obs"].shape
    st = DeviceState(n, dim, np.float64, "disabled")
    o0, _ = st.step(fix["raw_obs0"])
    assert np.array_equal(o0, fix["obs0"])
    a = 0
    for t in range(steps):
        resets = fix["reset_mask"][t].any()
        if how == "per_step":
            o, r = st.step(fix["raw_obs"][t], None, fix["raw_reward"][t], fix["term"][t], fix["trunc"][t])
            assert np.array_equal(o, fix["obs"][t]) and np.array_equal(r, fix["reward"][t]), t
        elif resets or t == steps - 1:
            o, r = st.steps(fix["raw_obs"][a:t + 1], fix["raw_reward"][a:t + 1], fix["term"][a:t + 1], fix["trunc"][a:t + 1])
            assert np.array_equal(o, fix["obs"][a:t + 1]) and np.array_equal(r, fix["reward"][a:t + 1]), (a, t)
            a = t + 1
        if resets:
            ro, _ = st.step(fix["raw_reset_obs"][t], fix["reset_mask"][t])
            assert np.array_equal(ro, fix["reset_obs"][t]), ("masked reset", t)
    for name, have in st.statistics().items():
        assert have.dtype == fix[name].dtype and np.array_equal(have, fix[name]), name


def test_abi_rejects_bad_arguments():
    st = DeviceState(4, 3, np.float32, "same")
    x = st.dev(np.zeros((2, 4, 3), np.float32))
    r = st.dev(np.zeros((2, 4)))
    f = st.dev(np.zeros((2, 4), bool))
    rc = st.lib.per_env_normalize_steps(0, st.stream(), C.byref(st.s), 2, 4, st.p(x), st.p(x), st.p(r), st.p(f), st.p(f), st.p(r))
    assert rc == -4  # MI_ERR_UNSUPPORTED: SAME_STEP trajectories need the final observations
    assert st.lib.per_env_normalize_step(0, st.stream(), C.byref(st.s), 4, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert st.lib.per_env_normalize_step(0, st.stream(), C.byref(st.s), 4, st.p(x), None, None, None, None, None, None, None, None, None, None) == -1


# -- 5. the restatement on the raw outputs of an unwrapped env ----------------------------------------------------------------------------------------
def collect(raw, w, steps, mode, numpy_actions=True):
    """Step ``raw`` and ``w`` with the same actions; the raw stream as a fixture-like dict, and what ``w`` returned."""
    o_raw, _ = raw.reset(seed=SEED)
    o_w, _ = w.reset(seed=SEED)
    raw.action_space.seed(cases.ASEED)
    fix = {"raw_obs0": host(o_raw), "raw_obs": [], "raw_reward": [], "term": [], "trunc": [], "raw_final_obs": [], "final_mask": []}
    got = {"obs0": host(o_w), "obs": [], "reward": [], "final_obs": []}
    for t in range(steps):
        a = raw.action_space.sample()
        o, r, te, tr, infos = raw.step(a)
        o2, r2, te2, tr2, infos2 = w.step(a)
        assert np.array_equal(host(te), host(te2)) and np.array_equal(host(tr), host(tr2)), t
        fix["raw_obs"].append(host(o)), fix["raw_reward"].append(host(r)), fix["term"].append(host(te)), fix["trunc"].append(host(tr))
        got["obs"].append(host(o2)), got["reward"].append(host(r2))
        if mode == "same":
            fm = host(infos["_final_obs"]).astype(bool)
            fix["final_mask"].append(fm), fix["raw_final_obs"].append(np.where(fm[:, None], host(infos["final_obs"]), 0))
            got["final_obs"].append(np.where(fm[:, None], host(infos2["final_obs"]), 0).astype(np.float32))
            assert np.array_equal(host(infos2["_final_obs"]).astype(bool), fm)
    return {k: (np.stack(v) if isinstance(v, list) and v else v) for k, v in fix.items()}, {k: (np.stack(v) if isinstance(v, list) and v else v) for k, v in got.items()}


@pytest.mark.parametrize("env_id,mode,dtype,steps,kw,inner", [
    ("Acrobot-v1", "next", np.float32, 40, {"max_episode_steps": 9}, None),
    ("Acrobot-v1", "same", np.float32, 40, {"max_episode_steps": 9}, None),
    ("InvertedPendulum-v5", "next", np.float64, 30, {"max_episode_steps": 9}, None),
    ("CartPole-v1", "next", np.float32, 40, {"max_episode_steps": 12}, lambda e: wrappers.StickyAction(wrappers.RepeatAction(e, 4), 0.25)),
])
def test_restatement_on_raw_outputs(env_id, mode, dtype, steps, kw, inner):
    make = lambda: gymnasium_amd.make_vec(env_id, num_envs=N, output="torch", autoreset_mode=MODES[mode], **kw)  # noqa: E731
    raw, wrapped = make(), make()
    if inner is not None:
        raw, wrapped = inner(raw), inner(wrapped)
    w = pair(wrapped)
    fix, got = collect(raw, w, steps, mode)
    assert fix["raw_obs"].dtype == dtype and (fix["term"] | fix["trunc"]).sum() >= N
    want = cases.replay(fix, mode, dtype)
    assert got["obs"].dtype == np.float32 and np.array_equal(got["obs0"], want["obs0"]) and np.array_equal(got["obs"], want["obs"])
    assert np.array_equal(got["reward"], want["reward"])
    if mode == "same":
        assert np.array_equal(got["final_obs"], want["final_obs"])
    on, rn = want["on"], want["rn"]
    assert w.obs_rms.mean.dtype == dtype and np.array_equal(w.obs_rms.mean, on.mean) and np.array_equal(w.obs_rms.var, on.var)
    assert np.array_equal(w.obs_rms.count, on.count) and np.array_equal(w.return_rms.var, rn.var) and np.array_equal(w.discounted_reward, rn.acc)
    raw.close(), w.close()


def test_normalize_reward_alone_over_discrete_observations():
    make = lambda: gymnasium_amd.make_vec("FrozenLake-v1", num_envs=N, output="torch")  # noqa: E731
    raw, w = make(), per_env.NormalizeReward(make(), gamma=0.9)
    with pytest.raises(error.Error, match="FlattenObservation"):
        per_env.NormalizeObservation(w)
    o1, _ = raw.reset(seed=SEED)
    o2, _ = w.reset(seed=SEED)
    assert np.array_equal(host(o1), host(o2))
    raw.action_space.seed(cases.ASEED)
    rn = cases.RewardNormalizer(N, 0.9, 1e-8, "next")
    rewarded = 0
    for t in range(60):
        a = raw.action_space.sample()
        o, r, te, tr, _ = raw.step(a)
        o2, r2, te2, tr2, _ = w.step(a)
        assert np.array_equal(host(o), host(o2)) and np.array_equal(host(te), host(te2))
        assert np.array_equal(host(r2), rn.step(host(r), host(te), host(tr))), t
        rewarded += int((host(r) != 0).sum())
    assert rewarded > 0 and np.array_equal(w.return_rms.count, rn.count) and np.array_equal(w.return_rms.mean, rn.mean)
    raw.close(), w.close()


# -- 6. masked reset --------------------------------------------------------------------------------------------------------------------------------
def test_masked_reset_updates_the_masked_rows_only():
    fix = cases.fixture("cartpole_next")
    w = build("cartpole", "next")
    raw = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, output="torch", max_episode_steps=cases.LIMITS["cartpole"])
    w.reset(seed=SEED), raw.reset(seed=SEED)
    for t in range(5):
        last = w.step(actions_of(fix, t, "torch"))[0]
        raw.step(actions_of(fix, t, "torch"))
    last = host(last).copy()
    mean, var, count = w.obs_rms.mean, w.obs_rms.var, w.obs_rms.count
    mask = np.zeros(N, dtype=bool)
    mask[[0, 5, 63, 64, 69]] = True
    ro, _ = w.reset(options={"reset_mask": mask.copy()})
    raw_ro, _ = raw.reset(options={"reset_mask": mask.copy()})
    ro, raw_ro = host(ro), host(raw_ro)
    assert np.array_equal(ro[~mask], last[~mask])
    assert np.array_equal(w.obs_rms.count[~mask], count[~mask]) and np.array_equal(w.obs_rms.count[mask], count[mask] + 1.0)
    assert np.array_equal(w.obs_rms.mean[~mask], mean[~mask]) and np.array_equal(w.obs_rms.var[~mask], var[~mask])
    on = cases.ObsNormalizer(N, 4, np.float32)
    on.mean, on.var, on.count, on.last = mean.copy(), var.copy(), count.copy(), last
    want = on.observe(raw_ro, mask)
    assert np.array_equal(ro, want) and np.array_equal(w.obs_rms.mean, on.mean) and np.array_equal(w.obs_rms.var, on.var)
    w.close(), raw.close()


# -- 7. frozen statistics -------------------------------------------------------------------------------------------------------------------------------
def test_update_running_mean_false_freezes_the_statistics_not_the_accumulator():
    fix = cases.fixture("pendulum_next")
    w = build("pendulum", "next")
    w.reset(seed=SEED)
    for t in range(10):
        w.step(actions_of(fix, t, "torch"))
    w.update_running_mean = False       # NormalizeReward (the outer wrapper)
    w.env.update_running_mean = False   # NormalizeObservation
    obs_before = (w.obs_rms.mean, w.obs_rms.var, w.obs_rms.count)
    ret_before = (w.return_rms.mean, w.return_rms.var, w.return_rms.count)
    on, rn = cases.ObsNormalizer(N, 3, np.float32), cases.RewardNormalizer(N, GAMMA, 1e-8, "next")
    on.mean, on.var, on.count = (a.copy() for a in obs_before)
    rn.mean, rn.var, rn.count = (a.copy() for a in ret_before)
    rn.acc, rn.was_done = w.discounted_reward.copy(), w.pending_autoreset.copy()
    on.update_running_mean = rn.update_running_mean = False
    acc0 = rn.acc.copy()
    for t in range(10, 20):
        o, r, te, tr, _ = w.step(actions_of(fix, t, "torch"))
        assert np.array_equal(host(o), on.observe(fix["raw_obs"][t])), t
        assert np.array_equal(host(r), rn.step(fix["raw_reward"][t], fix["term"][t], fix["trunc"][t])), t
    for have, want in zip((w.obs_rms.mean, w.obs_rms.var, w.obs_rms.count, w.return_rms.mean, w.return_rms.var, w.return_rms.count), obs_before + ret_before):
        assert np.array_equal(have, want)
    assert np.array_equal(w.discounted_reward, rn.acc) and not np.array_equal(rn.acc, acc0)
    w.close()


# -- 8. checkpoint round trip ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip():
    fix = cases.fixture("cartpole_next")
    a_env = build("cartpole", "next")
    a_env.reset(seed=SEED)
    for t in range(25):
        a_env.step(actions_of(fix, t, "torch"))
    base = a_env.unwrapped
    state, rng = base.get_state(), base.get_rng_state()
    saved = {(r, n): getattr(getattr(a_env, r), n) for r in ("obs_rms", "return_rms") for n in ("mean", "var", "count")}
    acc, pending = a_env.discounted_reward, a_env.pending_autoreset
    b_env = build("cartpole", "next")
    b_env.reset(seed=99)
    b_base = b_env.unwrapped
    b_base.set_state(*state)
    b_base._engine.seed(rng)
    for (r, n), v in saved.items():
        setattr(getattr(b_env, r), n, v)
    b_env.discounted_reward, b_env.pending_autoreset = acc, pending
    for t in range(25, 35):
        got = b_env.step(actions_of(fix, t, "torch"))
        want = a_env.step(actions_of(fix, t, "torch"))
        for x, y, f in zip(got[:4], want[:4], (fix["obs"][t], fix["reward"][t], fix["term"][t], fix["trunc"][t])):
            assert np.array_equal(host(x), host(y)) and np.array_equal(host(x), f), t
    a_env.close(), b_env.close()


# -- 9. composition with the vector wrappers --------------------------------------------------------------------------------------------------------------
def test_clip_reward_and_episode_statistics_above_the_pair():
    fix = cases.fixture("cartpole_next")
    w = wrappers.RecordEpisodeStatistics(wrappers.ClipReward(build("cartpole", "next"), -0.5, 0.5))
    obs0, _ = w.reset(seed=SEED)
    assert np.array_equal(host(obs0), fix["obs0"])
    returns, lengths, finished = np.zeros(N), np.zeros(N, np.int64), 0
    pending = np.zeros(N, dtype=bool)
    for t in range(T):
        o, r, te, tr, infos = w.step(actions_of(fix, t, "torch"))
        assert np.array_equal(host(o), fix["obs"][t]) and np.array_equal(host(r), np.clip(fix["reward"][t], -0.5, 0.5)), t
        returns[pending], lengths[pending] = 0.0, 0  # (NEXT_STEP: the autoreset step does not count)
        returns[~pending] += fix["raw_reward"][t][~pending]
        lengths[~pending] += 1
        done = fix["term"][t] | fix["trunc"][t]
        assert np.array_equal(host(infos["_episode"]).astype(bool), done)
        assert np.array_equal(host(infos["episode"]["r"])[done], returns[done]) and np.array_equal(host(infos["episode"]["l"])[done], lengths[done]), t
        finished += int(done.sum())
        pending = done
    assert finished >= 50 and (np.abs(fix["reward"]) > 0.5).any() and w.episode_count == finished
    w.close()


# -- step(None) and per-row seeds -----------------------------------------------------------------------------------------------------------------------
def test_step_none_and_a_list_of_seeds():
    """``reset(seed=[...])`` is the int seed's fan-out, and ``step(None)`` -- the on-device policy -- goes through the wrappers like any other step."""
    fix = cases.fixture("cartpole_next")
    raw = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, output="torch", max_episode_steps=cases.LIMITS["cartpole"])
    w = build("cartpole", "next")
    seeds = [SEED + i for i in range(N)]
    o_raw, _ = raw.reset(seed=seeds)
    o_w, _ = w.reset(seed=seeds)
    assert np.array_equal(host(o_w), fix["obs0"])
    raw.action_space.seed(5), w.action_space.seed(5)
    on, rn = cases.ObsNormalizer(N, 4, np.float32), cases.RewardNormalizer(N, GAMMA, 1e-8, "next")
    assert np.array_equal(on.observe(host(o_raw)), host(o_w))
    finished = 0
    for t in range(40):
        o, r, te, tr, _ = raw.step(None)
        o2, r2, te2, tr2, _ = w.step(None)
        assert np.array_equal(host(raw.unwrapped.last_sampled_actions), host(w.unwrapped.last_sampled_actions)), t
        assert np.array_equal(host(te), host(te2)) and np.array_equal(host(tr), host(tr2)), t
        assert np.array_equal(host(o2), on.observe(host(o))) and np.array_equal(host(r2), rn.step(host(r), host(te), host(tr))), t
        finished += int((host(te) | host(tr)).sum())
    assert finished >= N
    raw.close(), w.close()
