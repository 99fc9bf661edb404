"""-m gpu: MaxAndSkipObservation of the sub-environments inside the engine's step (gymnasium_amd.wrappers.MaxAndSkipObservation, mi_set_max_and_skip)
against the reference's own SyncVectorEnv over scalar envs wrapped in gymnasium.wrappers.MaxAndSkipObservation, bit for bit.

The fixtures max_and_skip_<key>.npz were recorded from the reference (tests/golden/make_golden_max_and_skip.py, which asserts their coverage: steps that
return frames a step of an earlier episode -- or the constructor -- left behind, in one slot and in both): 96 sub-environments, skip 4 and 2,
max_episode_steps 11 / 9 / 5 / 3 and CartPole's default, all three autoreset modes, StickyAction and FrameStackObservation over the wrapper,
teacher-forced rows that end an episode before a slot is written.  Every comparison is array_equal, with ONE exception that the fixtures themselves
mark (same_obs): the cos / sin of an Acrobot observation right after a reset, where the reference's value depends on NumPy's float32 SIMD kernels.
The frame slots hold step observations only, which have no such exception: max_and_skip_frames() is held to equality everywhere."""
import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import wrappers
from gymnasium_amd.gym_api import error
from gymnasium_amd.wrappers import per_env
from conftest import ENV_IDS, golden

pytestmark = pytest.mark.gpu

N, K, P, D, STACK, SEED, ASEED = 96, 4, 0.5, 2, 4, 4242, 77
MODES = {"next": "NextStep", "same": "SameStep", "disabled": "Disabled"}
# run -> (config, skip, limit, mode)
RUNS = {"s4_11_next": ("plain", 4, 11, "next"), "s4_11_same": ("plain", 4, 11, "same"), "s4_9_next": ("plain", 4, 9, "next"),
        "s4_9_same": ("plain", 4, 9, "same"), "s2_5_next": ("plain", 2, 5, "next"), "s4_3_next": ("plain", 4, 3, "next"),
        "sticky_s4_11_next": ("sticky", 4, 11, "next"), "stack_s4_11_next": ("stack", 4, 11, "next")}
CARTPOLE_RUNS = {"s4_default_next": ("plain", 4, None, "next")}
DISABLED_RUN = ("plain", 4, 11, "disabled")
INTEGER_REWARDS = ("cartpole", "acrobot", "mountaincar")  # (their episode returns add up exactly in any order)


def runs_of(key, configs=("plain", "sticky", "stack")):
    runs = dict(RUNS, **(CARTPOLE_RUNS if key == "cartpole" else {}))
    return {r: c for r, c in runs.items() if c[0] in configs}


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same_obs(got, g, name, t=None):
    """array_equal with the recording -- but for the elements the generator marked `<name>_inexact` (Acrobot only): cos / sin of a RESET observation
    where NumPy's float32 SIMD kernel, on the machine that recorded, did not return the correctly rounded value (the project's one stated parity
    exception, csrc/envs_classic.h; the engine returns the correctly rounded one).  Those are held to the 1 float32 ulp that separates the two; the
    mask is a property of the reference's recording, made without the engine."""
    got, ref = host(got), g[name] if t is None else g[name][t]
    if f"{name}_inexact" not in g.files:
        return np.array_equal(got, ref)
    m = g[f"{name}_inexact"] if t is None else g[f"{name}_inexact"][t]
    ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    return got.shape == ref.shape and np.array_equal(got[~m], ref[~m]) and bool((ulps[m] <= 1).all())


def build(key, conf, output, statistics=True, **kw):
    config, skip, limit, mode = conf
    if limit is not None:
        kw["max_episode_steps"] = limit
    base = gymnasium_amd.make_vec(ENV_IDS[key], num_envs=N, output=output, autoreset_mode=MODES[mode], **kw)
    env = wrappers.MaxAndSkipObservation(base, skip)
    if config == "sticky":
        env = wrappers.StickyAction(env, P, D)
    if config == "stack":
        env = per_env.FrameStackObservation(env, STACK)
    return base, (wrappers.RecordEpisodeStatistics(env) if statistics else env)


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
                assert np.array_equal(host(got[i]), g[f"{run}_final_obs"][t][i]), (what, run, "final_obs: the max frame", t, i)


def check_end(key, g, run, base, mode):
    """the frame slots, the sub-environments' generators and the engine's running totals after the run"""
    assert np.array_equal(base.max_and_skip_frames(), g[f"{run}_frames"]), (run, "frames")
    assert np.array_equal(base.get_rng_state(), g[f"{run}_rng"]), (run, "generators")
    if mode == "disabled":
        return
    done = g[f"{run}_term"] | g[f"{run}_trunc"]
    T = done.shape[0]
    resets = int(done[:-1].sum()) if mode == "next" else 0
    st = base.statistics()
    assert st["reset_steps"] == resets and st["env_steps"] == T * N - resets, (run, st)  # OUTER steps, as under RepeatAction
    assert st["episodes"] == int(done.sum()) and st["length_sum"] == int(g[f"{run}_ep_l"].sum()), (run, st)
    if key in INTEGER_REWARDS:
        assert st["return_sum"] == float(g[f"{run}_ep_r"].sum()), (run, st)


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("how", ["numpy", "torch", "sampled"])
def test_step_equals_the_reference(key, how):
    import torch

    g = golden(f"max_and_skip_{key}.npz")
    for run, conf in runs_of(key).items():
        base, env = build(key, conf, "numpy" if how == "numpy" else "torch")
        obs0, _ = env.reset(seed=SEED)
        assert same_obs(obs0, g, f"{run}_obs0"), (run, "reset")
        env.action_space.seed(ASEED)
        for t, a in enumerate(g[f"{run}_actions"]):
            if how == "sampled":
                out = env.step(None)
                assert np.array_equal(host(base.last_sampled_actions), a), (run, "sampled actions", t)
            else:
                out = env.step(torch.from_numpy(a).cuda() if how == "torch" else a)
            check_step(g, run, t, out, how)
        check_end(key, g, run, base, conf[3])
        env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("output", ["numpy", "torch"])
def test_disabled_run_with_masked_resets(key, output):
    import torch

    g, run = golden(f"max_and_skip_{key}.npz"), "s4_11_disabled"
    base, env = build(key, DISABLED_RUN, output, statistics=False)
    obs0, _ = env.reset(seed=SEED)
    assert same_obs(obs0, g, f"{run}_obs0")
    for t, a in enumerate(g[f"{run}_actions"]):
        check_step(g, run, t, env.step(torch.from_numpy(a).cuda() if output == "torch" else a), output)
        mask = g[f"{run}_reset_mask"][t]
        if mask.any():  # the rows that reset keep their frames
            before = base.max_and_skip_frames()
            o, _ = env.reset(options={"reset_mask": mask.copy()})
            assert same_obs(o, g, f"{run}_reset_obs", t), (key, "masked reset", t)
            assert np.array_equal(base.max_and_skip_frames(), before), (key, "a masked reset touched the frames", t)
    check_end(key, g, run, base, "disabled")
    env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("how", ["rollout_actions", "rollout_infos"])
def test_rollout_equals_the_reference(key, how):
    """rollout(T, actions) as rollout(13) + rollout(27): the frames cross a launch boundary in HBM.  rollout(T, infos=True): the random policy on the
    device, and under SAME_STEP final_obs rows that are max frames."""
    import torch

    g = golden(f"max_and_skip_{key}.npz")
    for run, conf in runs_of(key, ("plain", "sticky")).items():
        acts = g[f"{run}_actions"]
        T = acts.shape[0]
        base, env = build(key, conf, "torch", statistics=how == "rollout_infos")
        env.reset(seed=SEED)
        env.action_space.seed(ASEED)
        if how == "rollout_actions":
            cut = 13 if T > 13 else 5
            parts = [env.rollout(cut, torch.from_numpy(acts[:cut]).cuda()), env.rollout(T - cut, torch.from_numpy(acts[cut:]).cuda())]
            out = {k: torch.cat([p[k] for p in parts]) for k in ("obs", "rewards", "terminations", "truncations")}
        else:
            out = env.rollout(T, infos=True)
            assert np.array_equal(host(out["actions"]), acts), (run, "the policy's actions")
        assert same_obs(out["obs"], g, f"{run}_obs") and np.array_equal(host(out["rewards"]), g[f"{run}_reward"]), (how, run)
        assert np.array_equal(host(out["terminations"]), g[f"{run}_term"]) and np.array_equal(host(out["truncations"]), g[f"{run}_trunc"]), (how, run)
        if how == "rollout_infos":
            infos = out["infos"]
            assert np.array_equal(host(infos["_episode"]).astype(bool), g[f"{run}_ep_mask"]), (run, "episode mask")
            assert np.array_equal(host(infos["episode"]["r"]), g[f"{run}_ep_r"]) and np.array_equal(host(infos["episode"]["l"]), g[f"{run}_ep_l"]), run
            if conf[3] == "same":
                assert np.array_equal(host(infos["_final_obs"]).astype(bool), g[f"{run}_final_mask"]), (run, "final mask")
                assert np.array_equal(host(infos["final_obs"]), g[f"{run}_final_obs"]), (run, "final_obs: the max frame")
        check_end(key, g, run, base, conf[3])
        env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("mode", ["next", "same"])
def test_random_policy_rollout_equals_sampled_steps(key, mode):
    T = 24
    envs = [build(key, ("plain", 4, 9, mode), "torch", statistics=False) for _ in range(2)]
    for base, env in envs:
        env.reset(seed=SEED)
        env.action_space.seed(ASEED)
    (base_a, a), (base_b, b) = envs
    out = a.rollout(T)
    for t in range(T):
        o, r, te, tr, _ = b.step(None)
        assert np.array_equal(host(out["obs"][t]), host(o)) and np.array_equal(host(out["rewards"][t]), host(r)), (key, mode, t)
        assert np.array_equal(host(out["terminations"][t]), host(te)) and np.array_equal(host(out["truncations"][t]), host(tr)), (key, mode, t)
        assert np.array_equal(host(out["actions"][t]), host(base_b.last_sampled_actions)), (key, mode, t)
    assert np.array_equal(base_a.max_and_skip_frames(), base_b.max_and_skip_frames()) and base_a.max_and_skip_frames().any()
    assert np.array_equal(base_a.get_rng_state(), base_b.get_rng_state()) and base_a.statistics() == base_b.statistics()
    a.close(), b.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
def test_teacher_forced_rows_from_fresh_wrappers(key):
    g = golden(f"max_and_skip_{key}.npz")
    s, a = g["teacher_state"], g["teacher_action"]
    M = s.shape[0]
    assert key == "pendulum" or int((g["teacher_term"] & (g["teacher_inner"] < K)).sum()) == 48
    env = gymnasium_amd.make_vec(ENV_IDS[key], num_envs=M)
    env.reset(seed=0)
    env.set_max_and_skip(K)  # zeroed frames
    flags = np.full(M, 2 if key == "mountaincar_continuous" else 0, np.uint8)  # (MountainCarContinuous: the state is a float32 array)
    env.set_state(s, np.zeros(M, np.int32), flags)
    assert not env.max_and_skip_frames().any()
    o, r, te, tr, _ = env.step(a.reshape(M, 1) if a.dtype == np.float32 else a)
    assert np.array_equal(o, g["teacher_obs"]) and np.array_equal(r, g["teacher_reward"]), key
    assert np.array_equal(te, g["teacher_term"]) and np.array_equal(tr, g["teacher_trunc"]), key
    assert np.array_equal(env.max_and_skip_frames(), g["teacher_frames"]), key
    state, elapsed, _ = env.get_state()
    assert np.array_equal(state, g["teacher_next_state"]) and np.array_equal(elapsed, g["teacher_inner"]), (key, "TimeLimit counts inner steps")
    env.close()


@pytest.mark.parametrize("key", list(ENV_IDS))
@pytest.mark.parametrize("mode", ["next", "same"])
def test_everything_but_the_observation_is_repeat_action(key, mode):
    """needs no fixture: MaxAndSkipObservation(env, 4) and RepeatAction(env, 4) from the same seeds and actions"""
    common = dict(num_envs=N, max_episode_steps=11, autoreset_mode=MODES[mode])
    m_base, r_base = gymnasium_amd.make_vec(ENV_IDS[key], **common), gymnasium_amd.make_vec(ENV_IDS[key], **common)
    m, r = wrappers.MaxAndSkipObservation(m_base, K), wrappers.RepeatAction(r_base, K)
    om, _ = m.reset(seed=SEED)
    orr, _ = r.reset(seed=SEED)
    assert np.array_equal(om, orr)
    m_base.action_space.seed(ASEED)
    prev_done, differed = np.zeros(N, bool), 0
    for t in range(30):
        a = m_base.action_space.sample()
        o1, r1, te1, tr1, _ = m.step(a)
        o2, r2, te2, tr2, _ = r.step(a)
        assert np.array_equal(r1, r2) and np.array_equal(te1, te2) and np.array_equal(tr1, tr2), (key, mode, t)
        for x, y in zip(m_base.get_state(), r_base.get_state()):
            assert np.array_equal(x, y), (key, mode, t, "state")
        assert np.array_equal(m_base.get_rng_state(), r_base.get_rng_state()), (key, mode, t)
        resets = prev_done if mode == "next" else (te1 | tr1)  # the rows whose observation is a reset's
        assert np.array_equal(o1[resets], o2[resets]), (key, mode, t, "reset observations")
        differed += int((o1 != o2).any())
        prev_done = te1 | tr1
    assert differed > 0 and m_base.statistics() == r_base.statistics()
    m.close(), r.close()


def test_frames_survive_every_state_change():
    base = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, max_episode_steps=11)
    plain = gymnasium_amd.make_vec("CartPole-v1", num_envs=N, max_episode_steps=11)
    with pytest.raises(error.Error):
        base.max_and_skip_frames()
    env = wrappers.MaxAndSkipObservation(base, K)
    env.reset(seed=SEED)
    assert not base.max_and_skip_frames().any()
    base.action_space.seed(ASEED)
    for _ in range(5):
        env.step(base.action_space.sample())
    frames = base.max_and_skip_frames()
    assert frames.shape == (2, N, 4) and frames.dtype == np.float32 and frames[0].any() and frames[1].any()
    env.reset(seed=1)
    assert np.array_equal(base.max_and_skip_frames(), frames), "reset()"
    mask = np.arange(N) % 3 == 0
    env.reset(options={"reset_mask": mask})
    assert np.array_equal(base.max_and_skip_frames(), frames), "a masked reset"
    state, elapsed, flags = base.get_state()
    base.set_state(state * 0.5, elapsed, flags)
    assert np.array_equal(base.max_and_skip_frames(), frames), "set_state()"
    with pytest.raises(error.Error, match="fold the repeat"):
        base.set_step_wrappers(2, 0.0, 0)
    base.set_max_and_skip(K)  # a new wrapper
    assert not base.max_and_skip_frames().any()
    base.set_max_and_skip(0)  # the plain step again
    with pytest.raises(error.Error):
        base.max_and_skip_frames()
    o1, _ = base.reset(seed=7)
    o2, _ = plain.reset(seed=7)
    assert np.array_equal(o1, o2)
    for t in range(30):
        a = plain.action_space.sample()
        for x, y in zip(base.step(a)[:4], plain.step(a)[:4]):
            assert np.array_equal(x, y), t
    base.close(), plain.close()


def test_graph_replay_of_eight_steps_equals_eight_eager_steps():
    common = dict(num_envs=N, output="torch", max_episode_steps=11, copy=True)
    bases = [gymnasium_amd.make_vec("CartPole-v1", **common) for _ in range(2)]
    a, b = (wrappers.StickyAction(wrappers.MaxAndSkipObservation(e, K), P, D) for e in bases)
    for e in (a, b):
        e.reset(seed=SEED)
        e.action_space.seed(ASEED)
        e.step(None)  # kernels load on first use, which a capture must not trigger
    graph = b.capture_steps(policy="random", steps=8)
    eager = [a.step(None) for _ in range(8)]
    graph.replay()
    for k in range(8):
        for x, y in zip(eager[k][:4], graph.results[k][:4]):
            assert np.array_equal(host(x), host(y)), k
    assert np.array_equal(bases[0].max_and_skip_frames(), bases[1].max_and_skip_frames()) and bases[0].max_and_skip_frames().any()
    assert np.array_equal(a.get_rng_state(), b.get_rng_state()) and a.statistics() == b.statistics() and a.statistics()["episodes"] > 0
    a.close(), b.close()
