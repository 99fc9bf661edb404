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
