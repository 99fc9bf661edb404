"""-m gpu: ``rollout(T, infos=True)`` (mi_rollout_infos: the rollout kernels store per step what ``step()`` returns besides the trajectory)
against the reference's recordings and against T ``step()`` calls on the device.

Everything here is bit equality: the classic-control and ToyText kernels reproduce the reference bit for bit (tests/test_gpu_parity.py), and a
rollout and a sequence of steps run the same arithmetic on the same device (tests/test_gpu_mujoco.py::test_fused_rollout_equals_stepping
asserts ``torch.equal`` for the MuJoCo kinds too).  Shapes, seeds and guards: tests/rollout_infos_cases.py.
"""
import os

import numpy as np
import pytest

import gymnasium_amd
import rollout_infos_cases as cases
from gymnasium_amd import _native
from gymnasium_amd import wrappers as gw
from gymnasium_amd.gym_api import error

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAIN_KEYS = {"obs", "rewards", "terminations", "truncations", "actions"}


def _np(x):
    return x.cpu().numpy()


# -- against the reference's recordings -------------------------------------------------------------------------------------------------------
def test_same_step_final_observations_vs_reference_recording():
    import torch

    g = np.load(os.path.join(GOLD, "modes_cartpole.npz"))
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=6, autoreset_mode="SameStep", output="torch")
    obs0, _ = env.reset(seed=3)
    assert np.array_equal(_np(obs0), g["SameStep_obs0"])
    out = env.rollout(300, actions=torch.from_numpy(g["SameStep_actions"]).cuda(), infos=True)
    for name, rec in (("obs", "obs"), ("rewards", "reward"), ("terminations", "term"), ("truncations", "trunc")):
        assert np.array_equal(_np(out[name]), g[f"SameStep_{rec}"]), name
    infos = out["infos"]
    assert set(infos) == {"final_obs", "_final_obs", "final_info", "_final_info"} and infos["final_info"] == {}
    assert np.array_equal(_np(infos["_final_obs"]), g["SameStep_final_mask"]) and np.array_equal(_np(infos["_final_info"]), g["SameStep_final_mask"])
    assert g["SameStep_final_mask"].any() and not g["SameStep_final_mask"].all()
    # (the fixture holds zeros in the rows that finished nothing: the zero-fill contract of mi_rollout_extra)
    assert infos["final_obs"].dtype == torch.float32 and np.array_equal(_np(infos["final_obs"]), g["SameStep_final_obs"])
    env.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
def test_record_episode_statistics_rollout_vs_reference_recording(mode):
    """``infos=True`` here: without the keyword the wrapper returns the bare trajectory (tests/test_gpu_wrapped_rollout.py pins that key set) and
    only fills its queues and count -- which the second env below checks."""
    g = np.load(os.path.join(GOLD, "episode_stats.npz"))
    for kw, tag in ((dict(), ""), (dict(buffer_length=7, stats_key="ep"), "short_")):
        env = gw.RecordEpisodeStatistics(gymnasium_amd.make_vec("CartPole-v1", num_envs=6, autoreset_mode=mode, output="torch"), **kw)
        key = kw.get("stats_key", "episode")
        env.action_space.seed(5)
        env.reset(seed=3)
        out = env.rollout(300, infos=True)
        assert set(out) == PLAIN_KEYS | {"infos"}
        infos = out["infos"]
        assert key in infos and (key == "episode" or ("episode" not in infos and "_episode" not in infos))
        assert np.array_equal(_np(infos["_" + key]), g[f"{mode}_mask"])
        r, ln, tt = _np(infos[key]["r"]), _np(infos[key]["l"]), _np(infos[key]["t"])
        assert r.dtype == np.float64 and np.array_equal(r, g[f"{mode}_r"]), "episode returns, bit for bit (zeros where no episode ended)"
        assert ln.dtype == np.int64 and np.array_equal(ln, g[f"{mode}_l"])
        assert (tt[~g[f"{mode}_mask"]] == 0).all() and (tt[g[f"{mode}_mask"]] >= 0).all()
        assert env.episode_count == int(g[f"{mode}_episode_count"])
        assert np.array_equal(np.array(env.return_queue), g[f"{mode}_{tag}return_queue"])
        assert np.array_equal(np.array(env.length_queue), g[f"{mode}_{tag}length_queue"])
        assert len(env.time_queue) == len(env.return_queue) and min(env.time_queue) >= 0
        env.close()
    quiet = gw.RecordEpisodeStatistics(gymnasium_amd.make_vec("CartPole-v1", num_envs=6, autoreset_mode=mode, output="torch"))
    quiet.action_space.seed(5)
    quiet.reset(seed=3)
    assert set(quiet.rollout(172)) == PLAIN_KEYS and set(quiet.rollout(128)) == PLAIN_KEYS  # two calls: the bookkeeping carries across them
    assert quiet.episode_count == int(g[f"{mode}_episode_count"])
    assert np.array_equal(np.array(quiet.return_queue), g[f"{mode}_return_queue"]) and np.array_equal(np.array(quiet.length_queue), g[f"{mode}_length_queue"])
    quiet.close()


@pytest.mark.parametrize("key,env_id", [("frozenlake", "FrozenLake-v1"), ("taxi", "Taxi-v4")])
def test_toytext_same_step_infos_vs_reference_recording(key, env_id):
    """The recorded actions through ONE SAME_STEP rollout.  ``prob``: the reference types a step's "prob" array after the first sub-environment
    that supplies it, so in the steps where that is a reset info ({"prob": 1}, an int -- ``prob_is_int``) its recording holds the values
    truncated to integers (tests/parity_suite.py check_same_step_infos); a rollout's tensor has one dtype, float64, so those steps are compared
    after the same truncation and every other step as it is."""
    import torch

    g = np.load(os.path.join(GOLD, f"infos_same_step_{key}.npz"))
    T, n = g["actions"].shape
    env = gymnasium_amd.make_vec(env_id, num_envs=n, autoreset_mode="SameStep", output="torch")
    obs0, _ = env.reset(seed=13)
    assert np.array_equal(_np(obs0), g["obs0"])
    out = env.rollout(T, actions=torch.from_numpy(g["actions"]).cuda(), infos=True)
    for name, rec in (("obs", "obs"), ("rewards", "reward"), ("terminations", "term"), ("truncations", "trunc")):
        assert np.array_equal(_np(out[name]), g[rec]), name
    infos, fm = out["infos"], g["final_mask"]
    assert fm.any() and not fm.all()
    prob = _np(infos["prob"])
    assert prob.dtype == np.float64 and np.array_equal(_np(infos["_prob"]), g["prob_mask"])
    assert np.array_equal(np.where(g["prob_is_int"][:, None], np.trunc(prob), prob), g["prob"])
    assert np.array_equal(_np(infos["_final_obs"]), fm) and np.array_equal(_np(infos["_final_info"]), fm)
    fo = _np(infos["final_obs"])
    assert fo.dtype == np.int64 and np.array_equal(fo[fm], g["final_obs"][fm]) and not fo[~fm].any()
    fi = infos["final_info"]
    assert np.array_equal(_np(fi["_prob"]), g["final_prob_mask"]) and np.array_equal(_np(fi["prob"]), g["final_prob"]) and _np(fi["prob"]).dtype == np.float64
    if "action_mask" in g.files:
        assert np.array_equal(_np(infos["action_mask"]), g["action_mask"]) and _np(infos["_action_mask"]).all()
        assert np.array_equal(_np(fi["action_mask"]), g["final_action_mask"]) and np.array_equal(_np(fi["_action_mask"]), g["final_action_mask_mask"])
        assert _np(fi["action_mask"]).dtype == g["final_action_mask"].dtype
    env.close()


# -- rollout == T x step on the device ---------------------------------------------------------------------------------------------------------
def _rollout_equals_steps(env_id, n, T, mes, mode, caller, stats, both_flags=False, **kw):
    import torch

    a, b = cases.make_pair(env_id, n, mes, mode, stats, **kw)
    acts = cases.caller_actions(a, T) if caller else None
    (obs, rew, te, tr, act), ref = cases.stack_steps(b, T, acts)
    out = a.rollout(T, actions=acts, infos=True)
    assert set(out) == PLAIN_KEYS | {"infos"}
    assert torch.equal(out["obs"], obs) and torch.equal(out["rewards"], rew.to(out["rewards"].dtype)), "trajectory"
    assert torch.equal(out["terminations"], te) and torch.equal(out["truncations"], tr)
    assert torch.equal(out["actions"].reshape(act.shape), act), "actions"
    masks = {}
    cases.compare_infos(ref, out["infos"], True, masks=masks)
    cases.assert_guards(a, _np(te | tr), masks, _np(te), _np(tr), both_flags)
    # one further step on both: the bookkeeping the rollout left (pending autoresets, episode clocks and counts, current buffers, action stream)
    nxt = cases.caller_actions(a, 1, seed=23)[0] if caller else None
    sa = a.step(torch.from_numpy(a.action_space.sample()).cuda() if nxt is None else nxt)
    sb = b.step(torch.from_numpy(b.action_space.sample()).cuda() if nxt is None else nxt)
    for x, y in zip(sa[:4], sb[:4]):
        assert torch.equal(x, y), "the step after"
    cases.compare_infos(sb[4], sa[4], False)
    if stats:
        assert a.episode_count == b.episode_count > 0
        for name in ("_ep_r", "_ep_l", "_prev_dones_t"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("_was_done_t", "_final", "_info", "_final_info"):
        if getattr(b, name, None) is not None:
            assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state())) and np.array_equal(a.get_rng_state(), b.get_rng_state())
    a.close(), b.close()


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("caller", [True, False], ids=["caller_actions", "device_policy"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.CLASSIC_CASES, ids=lambda c: c[0])
def test_classic_rollout_infos_equal_stacked_steps(case, mode, caller, stats):
    _rollout_equals_steps(*case, mode, caller, stats)


@pytest.mark.parametrize("mode", cases.MODES)
def test_cartpole_rollout_infos_with_terminations_and_truncations(mode):
    _rollout_equals_steps(*cases.CARTPOLE_LONG, mode, False, True, both_flags=True)


def test_shared_generator_cartpole_rollout_infos_equal_stacked_steps():
    """rng="shared" (CartPoleVectorEnv's one generator): the rollout is T step launches that write row t of the caller's arrays."""
    _rollout_equals_steps("CartPole-v1", 300, 19, 5, "NextStep", True, True, rng="shared")


@pytest.mark.parametrize("caller", [True, False], ids=["caller_actions", "device_policy"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.MUJOCO_CASES, ids=lambda c: c[0])
def test_mujoco_rollout_infos_equal_stacked_steps(case, mode, caller):
    _rollout_equals_steps(*case, mode, caller, True)


@pytest.mark.parametrize("mode", cases.MODES)
def test_one_lane_simulator_rollout_infos_equal_stacked_steps(mode, monkeypatch):
    """MI355ENV_MJ_SERIAL=1: the fused one-lane rollout kernel of a kind that otherwise runs the cooperative path (HalfCheetah)."""
    monkeypatch.setenv("MI355ENV_MJ_SERIAL", "1")
    _rollout_equals_steps("HalfCheetah-v5", 5, 6, 3, mode, False, True)


# -- mi_rollout_infos == T x mi_step on the test's own device buffers ---------------------------------------------------------------------------
def _raw_rollout_equals_raw_steps(env_id, mode, sample, extras, T, n=300, max_episode_steps=2, **kw):
    """One mi_rollout_infos on one env against T mi_step calls on a second, below the Python env: the trajectory and the rows of `extras`
    (a rollout writes zeros where a step leaves the row alone, so the steps' arrays start as zeros), then state, generators and statistics.  300
    sub-environments: two workgroups, the second partial; max_episode_steps = 2: a truncation and an autoreset inside three steps."""
    import torch

    a, b = (gymnasium_amd.make_vec(env_id, num_envs=n, max_episode_steps=max_episode_steps, autoreset_mode=mode, output="torch", **kw) for _ in range(2))
    a.reset(seed=cases.RESET_SEED), b.reset(seed=cases.RESET_SEED)
    ea, eb = a._engine, b._engine
    discrete = ea.act_dtype is np.int64
    acts = None if sample else cases.caller_actions(a, T)
    if sample:
        words = _native.pcg_words(np.random.default_rng(cases.ACTION_SEED))
        ea.action_seed(words), eb.action_seed(words)

    def buffers():
        def z(shape, dtype):
            return torch.zeros((T,) + tuple(shape), dtype=dtype, device="cuda")

        info = (n, max(ea.info_dim, 1))
        traj = {"obs": z(a._obs_shape, a._obs_tdtype), "reward": z((n,), torch.float64), "terminated": z((n,), torch.bool), "truncated": z((n,), torch.bool),
                "actions_out": z((n,) if discrete else (n, ea.act_dim), torch.int64 if discrete else torch.float32)}
        ex = {"final_obs": z(a._obs_shape, a._obs_tdtype), "episode_return": z((n,), torch.float64), "episode_length": z((n,), torch.int32),
              "info": z(info, torch.float64), "final_info": z(info, torch.float64)}
        return traj, {k: ex[k] for k in extras}

    (ta, xa), (tb, xb) = buffers(), buffers()
    a._bind_stream(), b._bind_stream()
    ea.rollout(T, None if sample else acts.data_ptr(), ta["actions_out"].data_ptr() if sample else None, ta["obs"].data_ptr(), ta["reward"].data_ptr(),
               ta["terminated"].data_ptr(), ta["truncated"].data_ptr(), extra={k: v.data_ptr() for k, v in xa.items()})
    info_row = torch.zeros((n, max(ea.info_dim, 1)), dtype=torch.float64, device="cuda")
    for t in range(T):
        row = {k: v[t].data_ptr() for k, v in xb.items()}
        if "final_info" in row:  # (a step's final_info is its info row of the finishing transition: a step that asks for one has an info row)
            row.setdefault("info", info_row.data_ptr())
        eb.step(None if sample else acts[t].data_ptr(), tb["obs"][t].data_ptr(), tb["reward"][t].data_ptr(), tb["terminated"][t].data_ptr(),
                tb["truncated"][t].data_ptr(), loc=_native.MI_DEVICE, actions_out=tb["actions_out"][t].data_ptr() if sample else None, **row)
    a.synchronize(), b.synchronize()
    for name in ta:
        assert torch.equal(ta[name], tb[name]), name
    for name in xa:
        assert torch.equal(xa[name], xb[name]), name
    done = _np(ta["terminated"] | ta["truncated"])
    assert done.any() and not done.all()
    if "final_obs" in xa or "final_info" in xa:
        assert any(xa[k].any() for k in ("final_obs", "final_info") if k in xa), "no finished episode left a final row"
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), b.get_state())) and np.array_equal(a.get_rng_state(), b.get_rng_state())
    assert a.statistics() == b.statistics()
    a.close(), b.close()


# the five forms of tab_rollout_kernel (tabular.hip mi_tabular::rollout): Blackjack; the fickle Taxi and a plain table, each read from HBM (T < 8) and from LDS
TABULAR_FORMS = [("Blackjack-v1", {}, 3), ("Taxi-v4", {"fickle_passenger": True}, 3), ("Taxi-v4", {"fickle_passenger": True}, 8), ("FrozenLake-v1", {}, 3),
                 ("FrozenLake-v1", {}, 8)]


@pytest.mark.parametrize("sample", [False, True], ids=["caller_actions", "device_policy"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("form", TABULAR_FORMS, ids=["blackjack", "fickle", "fickle_lds", "plain", "plain_lds"])
def test_toytext_rollout_extras_equal_stacked_steps(form, mode, sample):
    env_id, kw, T = form
    extras = ["episode_return", "episode_length"] + ([] if env_id.startswith("Blackjack") else ["info"])  # (Blackjack has no info columns)
    if mode == "SameStep":
        extras += ["final_obs"] + ([] if env_id.startswith("Blackjack") else ["final_info"])
    _raw_rollout_equals_raw_steps(env_id, mode, sample, extras, T, **kw)


def test_cooperative_rollout_with_final_info_but_no_info_array():
    """The T-launch rollout of the cooperative robots (mujoco.hip launch_mj_rollout_coop): the finishing step's info reaches final_info through the env's own
    staging row when the caller keeps no info array."""
    _raw_rollout_equals_raw_steps("Ant-v5", "SameStep", False, ["final_info"], 3)


# -- scoping ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cases.MODES)
def test_default_rollout_is_unchanged_also_after_a_rollout_with_infos(mode):
    import torch

    a, b = cases.make_pair("CartPole-v1", 300, 5, mode, True)
    first = a.rollout(19)
    assert set(first) == PLAIN_KEYS
    ref = b.rollout(19)
    assert all(torch.equal(first[k], ref[k]) for k in PLAIN_KEYS)
    with_infos, ref = a.rollout(19, infos=True), b.rollout(19)
    assert all(torch.equal(with_infos[k], ref[k]) for k in PLAIN_KEYS)
    after, ref = a.rollout(19), b.rollout(19)
    assert set(after) == PLAIN_KEYS and all(torch.equal(after[k], ref[k]) for k in PLAIN_KEYS)
    a.close(), b.close()


def _raw_rollout(env, T, **extra):
    import torch

    N, eng = env.num_envs, env._engine
    acts = torch.zeros((T, N), dtype=torch.int64, device="cuda")
    obs = torch.empty((T, N, eng.obs_dim), dtype=torch.float32, device="cuda")
    bufs = {k: torch.empty((T, N, eng.obs_dim), dtype=torch.float32, device="cuda") for k in extra}
    env._bind_stream()
    eng.rollout(T, acts.data_ptr(), None, obs.data_ptr(), None, None, None, extra={k: v.data_ptr() for k, v in bufs.items()})
    env.synchronize()


def test_abi_refusals():
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=8, output="torch")
    env.reset(seed=0)
    with pytest.raises(_native.NativeError) as e:
        _raw_rollout(env, 4, final_obs=True)
    assert e.value.code == -1 and "SAME_STEP" in e.value.message, "final_obs under NEXT_STEP: MI_ERR_INVALID_ARGUMENT"
    with pytest.raises(_native.NativeError) as e:
        _raw_rollout(env, 4, info=True)
    assert e.value.code == -1, "a kind without info columns"
    env.close()
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=8, output="torch", autoreset_mode="Disabled")
    env.reset(seed=0)
    with pytest.raises(_native.NativeError) as plain:
        env.rollout(4)
    with pytest.raises(_native.NativeError) as with_infos:
        env.rollout(4, infos=True)
    with pytest.raises(_native.NativeError) as raw:
        _raw_rollout(env, 4, episode_return=True)
    assert plain.value.code == with_infos.value.code == raw.value.code and plain.value.message == raw.value.message
    env.close()


def test_infos_with_numpy_output_is_refused():
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=8)
    env.reset(seed=0)
    with pytest.raises(error.Error, match="output='torch'") as plain:
        env.rollout(4)
    with pytest.raises(error.Error, match="output='torch'") as with_infos:
        env.rollout(4, infos=True)
    assert str(plain.value) == str(with_infos.value)
    env.close()
