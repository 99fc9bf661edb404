"""-m gpu: RepeatAction / StickyAction of the sub-environments inside the engine's step (gymnasium_amd.wrappers.RepeatAction / StickyAction,
mi_set_step_wrappers) against the reference's own SyncVectorEnv over scalar envs wrapped in gymnasium.wrappers.RepeatAction / StickyAction, bit for bit.

The fixtures step_wrappers_<key>.npz were recorded from the reference (tests/golden/make_golden_step_wrappers.py, which asserts their coverage:
truncations and terminations INSIDE a repeat, sticky draws that trigger and that do not, series cut short by a reset): 96 sub-environments,
RepeatAction(4) / StickyAction(0.5, 2) / both, max_episode_steps = 11 and the id's default, all three autoreset modes, teacher-forced rows that end an
episode inside a repeat, Acrobot's torque noise under StickyAction.  Every comparison is array_equal, with ONE exception that the fixtures themselves mark (same_obs): the cos / sin of an Acrobot
observation right after a reset, where the reference's value depends on NumPy's float32 SIMD kernels.  Measured on the MI355X against the recordings:
in the eight Acrobot runs 3 / 5 / 3 / 3 / 2 / 2 / 0 / 0 elements differ, each by 1 float32 ulp, all in rows that just reset, all marked by the
generator from the reference's own state; rewards, flags, every other observation and the generators' positions are equal."""
import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import wrappers
from gymnasium_amd.gym_api import error
from conftest import ENV_IDS, golden

pytestmark = pytest.mark.gpu

N, K, P, D, SEED, ASEED = 96, 4, 0.5, 2, 4242, 77
MODES = {"next": "NextStep", "same": "SameStep", "disabled": "Disabled"}
RUNS = [f"{c}_11_{m}" for c in ("repeat", "sticky", "both") for m in ("next", "same")] + ["both_default_next", "both_default_same"]
INTEGER_REWARDS = ("cartpole", "acrobot", "mountaincar")  # (their episode returns add up exactly in any order)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same_obs(got, g, name, t=None):
    """array_equal with the recording -- but for the elements the generator marked `<name>_inexact` (Acrobot only): cos / sin of a reset observation
    where NumPy's float32 SIMD kernel, on the machine that recorded, did not return the correctly rounded value (the project's one stated parity
    exception, csrc/envs_classic.h; the engine returns the correctly rounded one).  Those -- 2 to 5 of the 23 040 elements of a run -- are held to the
    1 float32 ulp that separates the two; the mask is a property of the reference's recording, made without the engine."""
    got, ref = host(got), g[name] if t is None else g[name][t]
    if f"{name}_inexact" not in g.files:
        return np.array_equal(got, ref)
    m = g[f"{name}_inexact"] if t is None else g[f"{name}_inexact"][t]
    ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    return got.shape == ref.shape and np.array_equal(got[~m], ref[~m]) and bool((ulps[m] <= 1).all())


def wrap(env, config):
    if config in ("repeat", "both"):
        env = wrappers.RepeatAction(env, K)
    if config in ("sticky", "both", "noise"):
        env = wrappers.StickyAction(env, P, D)
    return env


def build(key, run, output, statistics=True, **kw):
    config, limit, mode = run.split("_")
    if limit != "default":
        kw["max_episode_steps"] = int(limit)
    env = wrap(gymnasium_amd.make_vec(ENV_IDS[key], num_envs=N, output=output, autoreset_mode=MODES[mode], **kw), config)
    return wrappers.RecordEpisodeStatistics(env) if statistics else env


def episode_rows(infos):
    if "_episode" not in infos:
        return np.zeros(N), np.zeros(N, np.int64), np.zeros(N, bool)
    m = host(infos["_episode"]).astype(bool)
    return np.where(m, host(infos["episode"]["r"]), 0.0), np.where(m, host(infos["episode"]["l"]), 0).astype(np.int64), m


def check_step(g, run, t, out, what):
    o, r, te, tr, infos = out
    assert same_obs(o, g, f"{run}_obs", t), (what, run, "obs", t)
    assert np.array_equal(host(r), g[f"{run}_reward"][t]), (what, run, "reward", t)
    assert np.array_equal(host(te), g[f"{run}_term"][t]) and np.array_equal(host(tr), g[f"{run}_trunc"][t]), (what, run, "flags", t)
    if f"{run}_ep_mask" in g.files:
        er, el, em = episode_rows(infos)
        assert np.array_equal(em, g[f"{run}_ep_mask"][t]) and np.array_equal(el, g[f"{run}_ep_l"][t]), (what, run, "episode length", t)
        assert np.array_equal(er, g[f"{run}_ep_r"][t]), (what, run, "episode return", t)
    if f"{run}_final_mask" in g.files:
        fm = g[f"{run}_final_mask"][t]
        if fm.any():
            assert np.array_equal(host(infos["_final_obs"]).astype(bool), fm), (what, run, "final mask", t)
            got = infos["final_obs"]
            for i in np.flatnonzero(fm):
                assert np.array_equal(host(got[i]), g[f"{run}_final_obs"][t][i]), (what, run, "final_obs", t, i)


def check_end(key, g, run, env, mode):
    """the sub-environments' generators and the engine's running totals after the run"""
    assert np.array_equal(env.get_rng_state(), g[f"{run}_rng"]), (run, "generators")
    done = g[f"{run}_term"] | g[f"{run}_trunc"]
    T = done.shape[0]
    resets = int(done[:-1].sum()) if mode == "next" else 0
    st = env.statistics()
    assert st["reset_steps"] == resets and st["env_steps"] == T * N - resets, (run, st)  # OUTER steps (utils/performance.py:88-90)
    assert st["episodes"] == int(done.sum()) and st["length_sum"] == int(g[f"{run}_ep_l"].sum()), (run, st)
    if key in INTEGER_REWARDS:
        assert st["return_sum"] == float(g[f"{run}_ep_r"].sum()), (run, st)


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("how", ["numpy", "torch", "sampled"])
def test_step_equals_the_reference(key, how):
    import torch

    g = golden(f"step_wrappers_{key}.npz")
    for run in RUNS:
        env = build(key, run, "numpy" if how == "numpy" else "torch")
        obs0, _ = env.reset(seed=SEED)
        assert same_obs(obs0, g, f"{run}_obs0"), (run, "reset")
        env.action_space.seed(ASEED)
        for t, a in enumerate(g[f"{run}_actions"]):
            if how == "sampled":
                out = env.step(None)
                assert np.array_equal(host(env.last_sampled_actions), a), (run, "sampled actions", t)
            else:
                out = env.step(torch.from_numpy(a).cuda() if how == "torch" else a)
            check_step(g, run, t, out, how)
        check_end(key, g, run, env, run.split("_")[2])
        env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("how", ["rollout", "rollout_actions", "rollout_infos"])
def test_rollout_equals_the_reference(key, how):
    import torch

    g = golden(f"step_wrappers_{key}.npz")
    for run in RUNS:
        acts = g[f"{run}_actions"]
        T = acts.shape[0]
        env = build(key, run, "torch", statistics=how == "rollout_infos")
        env.reset(seed=SEED)
        env.action_space.seed(ASEED)
        if how == "rollout_actions":
            out = env.rollout(T, torch.from_numpy(acts).cuda())
        else:
            out = env.rollout(T, infos=how == "rollout_infos")
            assert np.array_equal(host(out["actions"]), acts), (run, "the policy's actions, not the effective ones")
        assert same_obs(out["obs"], g, f"{run}_obs") and np.array_equal(host(out["rewards"]), g[f"{run}_reward"]), (how, run)
        assert np.array_equal(host(out["terminations"]), g[f"{run}_term"]) and np.array_equal(host(out["truncations"]), g[f"{run}_trunc"]), (how, run)
        if how == "rollout_infos":
            infos = out["infos"]
            em = host(infos["_episode"]).astype(bool)
            assert np.array_equal(em, g[f"{run}_ep_mask"]), (run, "episode mask")
            assert np.array_equal(host(infos["episode"]["r"]), g[f"{run}_ep_r"]) and np.array_equal(host(infos["episode"]["l"]), g[f"{run}_ep_l"]), run
            if run.endswith("_same"):
                assert np.array_equal(host(infos["_final_obs"]).astype(bool), g[f"{run}_final_mask"]), (run, "final mask")
                assert np.array_equal(host(infos["final_obs"]), g[f"{run}_final_obs"]), (run, "final_obs: the last INNER observation")
        check_end(key, g, run, env, run.split("_")[2])
        env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_disabled_run_with_masked_resets(key, output):
    import torch

    g, run = golden(f"step_wrappers_{key}.npz"), "both_11_disabled"
    env = build(key, run, output, statistics=False)
    obs0, _ = env.reset(seed=SEED)
    assert same_obs(obs0, g, f"{run}_obs0")
    for t, a in enumerate(g[f"{run}_actions"]):
        check_step(g, run, t, env.step(torch.from_numpy(a).cuda() if output == "torch" else a), output)
        mask = g[f"{run}_reset_mask"][t]
        if mask.any():  # the rows that reset forget their last action and leave a running series
            o, _ = env.reset(options={"reset_mask": mask.copy()})
            assert same_obs(o, g, f"{run}_reset_obs", t), (key, "masked reset", t)
    assert np.array_equal(env.get_rng_state(), g[f"{run}_rng"])
    env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
def test_teacher_forced_rows_end_inside_the_repeat(key):
    g = golden(f"step_wrappers_{key}.npz")
    s, a = g["teacher_state"], g["teacher_action"]
    M = s.shape[0]
    assert key == "pendulum" or int((g["teacher_term"] & (g["teacher_inner"] < K)).sum()) == 48
    env = wrappers.RepeatAction(gymnasium_amd.make_vec(ENV_IDS[key], num_envs=M), K)
    env.reset(seed=0)
    flags = np.full(M, 2 if key == "mountaincar_continuous" else 0, np.uint8)  # (MountainCarContinuous: the state is a float32 array)
    env.set_state(s, np.zeros(M, np.int32), flags)
    o, r, te, tr, _ = env.step(a.reshape(M, 1) if a.dtype == np.float32 else a)
    assert np.array_equal(o, g["teacher_obs"]) and np.array_equal(r, g["teacher_reward"]), key
    assert np.array_equal(te, g["teacher_term"]) and np.array_equal(tr, g["teacher_trunc"]), key
    state, elapsed, _ = env.get_state()
    assert np.array_equal(state, g["teacher_next_state"]) and np.array_equal(elapsed, g["teacher_inner"]), (key, "TimeLimit counts inner steps")
    env.close()


@pytest.mark.parametrize("how", ["numpy", "sampled", "rollout"])
def test_acrobot_sticky_draw_precedes_the_noise_draw(how):
    g, run = golden("step_wrappers_acrobot.npz"), "noise_11_next"
    env = build("acrobot", run, "numpy" if how == "numpy" else "torch", statistics=how != "rollout")
    obs0, _ = env.reset(seed=SEED)
    assert same_obs(obs0, g, f"{run}_obs0")
    env.set_attr("torque_noise_max", g[f"{run}_noise"].tolist())
    env.action_space.seed(ASEED)
    acts = g[f"{run}_actions"]
    if how == "rollout":
        out = env.rollout(acts.shape[0])
        assert same_obs(out["obs"], g, f"{run}_obs") and np.array_equal(host(out["rewards"]), g[f"{run}_reward"])
        assert np.array_equal(host(out["terminations"]), g[f"{run}_term"]) and np.array_equal(host(out["truncations"]), g[f"{run}_trunc"])
    else:
        for t, a in enumerate(acts):
            check_step(g, run, t, env.step(None if how == "sampled" else a), how)
    assert np.array_equal(env.get_rng_state(), g[f"{run}_rng"])
    env.close()


def test_graph_replay_of_eight_steps_equals_eight_eager_steps():
    common = dict(num_envs=N, output="torch", max_episode_steps=11, copy=True)
    a, b = (wrap(gymnasium_amd.make_vec("CartPole-v1", **common), "both") for _ in range(2))
    for e in (a, b):
        e.reset(seed=SEED)
        e.action_space.seed(ASEED)
        e.step(None)  # kernels load on first use, which a capture must not trigger
    graph = b.capture_steps(policy="random", steps=8)
    for rep in range(3):  # all wrapper state is on the device: nothing on the host moves between replays
        eager = [a.step(None) for _ in range(8)]
        graph.replay()
        for k in range(8):
            for x, y in zip(eager[k][:4], graph.results[k][:4]):
                assert np.array_equal(host(x), host(y)), (rep, k)
    assert np.array_equal(a.get_rng_state(), b.get_rng_state()) and a.statistics() == b.statistics() and a.statistics()["episodes"] > 0
    a.close(), b.close()


@pytest.mark.parametrize("key", ["cartpole", "pendulum"])
def test_switched_off_the_plain_trajectory_returns(key):
    g = golden(f"rollout_{key}.npz")
    n = g["obs0"].shape[0]
    env = gymnasium_amd.make_vec(ENV_IDS[key], num_envs=n)
    w = wrap(env, "both")
    w.reset(seed=3)
    for _ in range(5):
        w.step(env.action_space.sample())
    env.set_step_wrappers()  # (0, 0.0, 0): the plain step again, on the one-role kernels the env now stays on
    obs, _ = env.reset(seed=7)
    assert np.array_equal(obs, g["obs0"])
    for t in range(120):
        o, r, te, tr, _ = env.step(g["actions"][t])
        assert np.array_equal(o, g["obs"][t]) and np.array_equal(r, g["reward"][t]), (key, t)
        assert np.array_equal(te, g["term"][t]) and np.array_equal(tr, g["trunc"][t]), (key, t)
    env.close()


def test_sticky_refuses_a_changed_action_dtype():
    env = wrappers.StickyAction(gymnasium_amd.make_vec("Pendulum-v1", num_envs=8), 0.25)
    env.reset(seed=0)
    env.step(np.zeros((8, 1), np.float32))
    with pytest.raises(error.Error, match="element type"):
        env.step(np.zeros((8, 1), np.float64))
    env.step(np.ones((8, 1), np.float32))
    env.close()
