"""-m gpu: Acrobot's per-sub-environment physics (set_attr), torque noise and "nips" dynamics on the HIP engine against the reference's own
SyncVectorEnv, bit for bit.

The fixture env_attrs_acrobot.npz was recorded from the reference (tests/golden/make_golden_acrobot_attrs.py): 96 sub-environments (a full
wavefront and a half one), max_episode_steps = 25, 96 random-policy steps with every attribute set per sub-environment after the reset and
changed half-way -- noisy and noise-free sub-environments, "book" and "nips", Python ints and floats, four sub-environments at the defaults --
in NEXT_STEP and SAME_STEP mode, the sub-environments' generator states after the NEXT_STEP run, and teacher-forced single steps.  The
generator script asserts that the runs hold truncations, terminations of noisy sub-environments and autoresets between noisy steps.
Every comparison is array_equal."""
import numpy as np
import pytest

import gymnasium_amd
import rollout_infos_cases as cases
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    z = golden("env_attrs_acrobot.npz")
    return {k: z[k] for k in z.files}  # (decompressed once)


def names(env):
    return [a[0] for a in env.ENV_ATTRS]


def values(env, rows, ints, reps=1):
    """{name: per-sub-environment Python values} from the fixture's [A][n] rows (ints: the values that were Python ints)."""
    out = {}
    for k, name in enumerate(names(env)):
        if name == "book_or_nips":
            vals = ["nips" if v == 1.0 else "book" for v in rows[k]]
        else:
            vals = [int(v) if i else float(v) for v, i in zip(rows[k], ints[k])]
        out[name] = vals * reps
    return out


def set_all(env, vals):
    for name, v in vals.items():
        env.set_attr(name, v)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def make(g, tag, **kw):
    env = gymnasium_amd.make_vec("Acrobot-v1", num_envs=g[f"{tag}_actions"].shape[1], max_episode_steps=int(g[f"{tag}_max_steps"]), **kw)
    obs0, _ = env.reset(seed=[int(s) for s in g[f"{tag}_seeds"]])
    assert np.array_equal(host(obs0), g[f"{tag}_obs0"])
    set_all(env, values(env, g[f"{tag}_attr0"], g[f"{tag}_attr0_int"]))
    env.action_space.seed(int(g[f"{tag}_aseed"]))
    return env


@pytest.mark.parametrize("how", ["numpy", "torch", "sampled", "rollout", "rollout_actions"])
def test_random_policy_run_equals_the_reference(g, how):
    """... and leaves every sub-environment's generator where the reference's is: a noisy sub-environment took exactly one draw per step it
    made, none in its autoreset steps, and the resets' four draws in between."""
    import torch

    T, sw = g["run_actions"].shape[0], int(g["run_switch"])
    env = make(g, "run", output="numpy" if how == "numpy" else "torch")

    def check(t0, obs, rew, term, trunc):
        for t in range(obs.shape[0]):
            assert np.array_equal(obs[t], g["run_obs"][t0 + t]), (how, "obs", t0 + t)
            assert np.array_equal(rew[t], g["run_reward"][t0 + t]), (how, "reward", t0 + t)
            assert np.array_equal(term[t], g["run_term"][t0 + t]) and np.array_equal(trunc[t], g["run_trunc"][t0 + t]), (how, t0 + t)

    for t0, t1 in ((0, sw), (sw, T)):
        if t0 == sw:
            set_all(env, values(env, g["run_attr1"], g["run_attr1_int"]))
        if how.startswith("rollout"):
            acts = torch.from_numpy(g["run_actions"][t0:t1]).cuda() if how == "rollout_actions" else None
            out = env.rollout(t1 - t0, actions=acts)
            if how == "rollout":
                assert np.array_equal(host(out["actions"]), g["run_actions"][t0:t1])
            check(t0, host(out["obs"]), host(out["rewards"]), host(out["terminations"]), host(out["truncations"]))
            continue
        for t in range(t0, t1):
            if how == "sampled":
                o, r, te, tr, _ = env.step(None)
                assert np.array_equal(host(env.last_sampled_actions), g["run_actions"][t])
            else:
                a = g["run_actions"][t]
                o, r, te, tr, _ = env.step(torch.from_numpy(a).cuda() if how == "torch" else a)
            check(t, host(o)[None], host(r)[None], host(te)[None], host(tr)[None])
    assert np.array_equal(env._engine.get_rng(), g["run_rng"]), (how, "the sub-environments' generators after the run")
    env.close()


@pytest.mark.parametrize("how", ["step", "rollout"])
def test_same_step_run_equals_the_reference(g, how):
    import torch

    env = make(g, "same", autoreset_mode="SameStep", output="torch")
    T, sw = g["same_actions"].shape[0], int(g["same_switch"])
    fm = g["same_final_mask"]
    assert fm.any() and not fm.all()
    for t0, t1 in ((0, sw), (sw, T)):
        if t0 == sw:
            set_all(env, values(env, g["same_attr1"], g["same_attr1_int"]))
        if how == "rollout":
            out = env.rollout(t1 - t0, actions=torch.from_numpy(g["same_actions"][t0:t1]).cuda(), infos=True)
            for name, fx in (("obs", "same_obs"), ("rewards", "same_reward"), ("terminations", "same_term"), ("truncations", "same_trunc")):
                assert np.array_equal(host(out[name]), g[fx][t0:t1]), (name, t0)
            assert np.array_equal(host(out["infos"]["_final_obs"]), fm[t0:t1])
            assert np.array_equal(host(out["infos"]["final_obs"]), g["same_final_obs"][t0:t1])  # (zeros in the rows that finished nothing, in both)
            continue
        for t in range(t0, t1):
            o, r, te, tr, info = env.step(torch.from_numpy(g["same_actions"][t]).cuda())
            assert np.array_equal(host(o), g["same_obs"][t]) and np.array_equal(host(r), g["same_reward"][t]), t
            assert np.array_equal(host(te), g["same_term"][t]) and np.array_equal(host(tr), g["same_trunc"][t]), t
            if fm[t].any():
                assert np.array_equal(host(info["_final_obs"]), fm[t])
                assert np.array_equal(host(info["final_obs"])[fm[t]], g["same_final_obs"][t][fm[t]]), t
    assert np.array_equal(env._engine.get_rng(), g["same_rng"])
    env.close()


def test_teacher_forced_steps_equal_the_reference(g):
    s = g["teacher_state"]
    M = s.shape[0]
    env = gymnasium_amd.make_vec("Acrobot-v1", num_envs=M, max_episode_steps=1000)
    env.reset(seed=0)
    env.set_state(s, np.zeros(M, np.int32), np.zeros(M, np.uint8))
    set_all(env, values(env, g["teacher_attr"], g["teacher_attr_int"]))
    o, r, te, _, _ = env.step(g["teacher_action"])
    assert np.array_equal(o, g["teacher_obs"])
    assert np.array_equal(r, g["teacher_reward"]) and np.array_equal(te, g["teacher_term"])
    assert np.array_equal(env.get_state()[0], g["teacher_next_state"])
    env.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
def test_rollout_infos_equal_the_step_loop(g, mode):
    """rollout(T, infos=True) == T x step() with noisy per-lane physics; T = 19 is odd (the loop is unrolled by two), max_episode_steps = 5
    puts an episode end on many steps."""
    N, T = 96, 19
    a, b = cases.make_pair("Acrobot-v1", N, 5, mode, True)
    for e in (a, b):
        set_all(e, values(e, g["run_attr0"], g["run_attr0_int"]))
    acts = cases.caller_actions(a, T)
    (obs, rew, term, trunc, _), ref_infos = cases.stack_steps(a, T, acts)
    out = b.rollout(T, actions=acts, infos=True)
    for name, want in (("obs", obs), ("rewards", rew), ("terminations", term), ("truncations", trunc)):
        assert np.array_equal(host(out[name]), host(want)), (mode, name)
    masks = {}
    cases.compare_infos(ref_infos, out["infos"], True, masks=masks)
    dones = host(term) | host(trunc)
    assert dones.mean() >= cases.MIN_DONE and all(m.any() for m in masks.values())
    assert np.array_equal(a._engine.get_rng(), b._engine.get_rng())
    assert np.array_equal(a.get_state()[0], b.get_state()[0])
    a.close(), b.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep", "Disabled"])
def test_defaults_set_explicitly_equal_the_uniform_kernel(mode):
    """Every attribute set per sub-environment to its default: the per-lane kernels give the uniform kernels' results, 64 envs x 64 steps."""
    import torch

    N, T = 64, 64
    kw = dict(num_envs=N, output="torch", autoreset_mode=mode, max_episode_steps=20)
    a, b = gymnasium_amd.make_vec("Acrobot-v1", **kw), gymnasium_amd.make_vec("Acrobot-v1", **kw)
    for e in (a, b):
        e.reset(seed=5)
        e.action_space.seed(9)
    for name in names(b):
        b.set_attr(name, list(b.get_attr(name)))
    if mode != "Disabled":
        ra, rb = a.rollout(T), b.rollout(T)
        for k in ("obs", "rewards", "terminations", "truncations", "actions"):
            assert torch.equal(ra[k], rb[k]), (mode, k)
        assert ra["truncations"].any()
    for t in range(T if mode != "Disabled" else 19):  # (DISABLED: no sub-environment may finish)
        x = torch.from_numpy(a.action_space.sample()).cuda()
        sa, sb = a.step(x), b.step(x)
        for u, v in zip(sa[:4], sb[:4]):
            assert torch.equal(u, v), (mode, t)
    assert np.array_equal(a.get_state()[0], b.get_state()[0])
    assert np.array_equal(a._engine.get_rng(), b._engine.get_rng())
    a.close(), b.close()


def test_device_tensor_equals_the_list(g):
    import torch

    N = g["run_attr0"].shape[1]
    a, b = (gymnasium_amd.make_vec("Acrobot-v1", num_envs=N, output="torch", max_episode_steps=25) for _ in range(2))
    vals = values(a, g["run_attr0"], g["run_attr0_int"])
    for name, v in vals.items():
        if name == "book_or_nips":
            a.set_attr(name, v), b.set_attr(name, v)
            continue
        t = torch.tensor([float(x) for x in v], dtype=torch.float64, device="cuda")
        a.set_attr(name, t), b.set_attr(name, [float(x) for x in v])
        assert a.get_attr(name) == b.get_attr(name) == tuple(float(x) for x in v)
    with pytest.raises(TypeError):
        a.set_attr("book_or_nips", torch.zeros(N, device="cuda"))
    with pytest.raises(ValueError, match="ACROBOT_ATTR_RANGES"):
        a.set_attr("dt", torch.full((N,), 0.5, dtype=torch.float64, device="cuda"))
    for e in (a, b):
        e.reset(seed=1)
        e.action_space.seed(7)
    ra, rb = a.rollout(64), b.rollout(64)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    assert np.array_equal(a._engine.get_rng(), b._engine.get_rng())
    a.close(), b.close()


def test_disabled_mode_steps_equal_the_reference_until_the_first_episode_end(g):
    """DISABLED autoreset runs the same per-lane step, noise draws included: the recorded NEXT_STEP run up to and including the first step in
    which a sub-environment finishes (after it the two modes part)."""
    done = g["run_term"] | g["run_trunc"]
    t_end = int(np.flatnonzero(done.any(axis=1))[0])
    # (several steps in a row, so that a noisy lane's generator is read, moved and stored by more than one launch)
    assert 2 <= t_end < int(g["run_switch"]) and (g["run_attr0"][9] > 0).any()
    env = make(g, "run", autoreset_mode="Disabled")
    for t in range(t_end + 1):
        o, r, te, tr, _ = env.step(g["run_actions"][t])
        assert np.array_equal(o, g["run_obs"][t]) and np.array_equal(r, g["run_reward"][t]), t
        assert np.array_equal(te, g["run_term"][t]) and np.array_equal(tr, g["run_trunc"][t]), t
    env.close()


def test_fused_normalize_wrappers_see_the_same_steps(g):
    """The step kernel with the wrappers' epilogue: noisy per-lane physics under NormalizeObservation / NormalizeReward against the same env
    normalised by the wrappers' stand-alone passes (FUSES_WRAPPERS = False)."""
    from gymnasium_amd import wrappers

    N = g["run_attr0"].shape[1]
    envs = [gymnasium_amd.make_vec("Acrobot-v1", num_envs=N, max_episode_steps=25) for _ in range(2)]
    envs[1].FUSES_WRAPPERS = False
    for e in envs:
        set_all(e, values(e, g["run_attr0"], g["run_attr0_int"]))
    ws = [wrappers.NormalizeReward(wrappers.NormalizeObservation(e), gamma=0.99) for e in envs]
    for w in ws:
        w.reset(seed=3)
    for t in range(40):
        sa, sb = ws[0].step(g["run_actions"][t]), ws[1].step(g["run_actions"][t])
        for u, v in zip(sa[:4], sb[:4]):
            assert np.array_equal(u, v), t
    assert np.array_equal(envs[0]._engine.get_rng(), envs[1]._engine.get_rng())
    for e in envs:
        e.close()
