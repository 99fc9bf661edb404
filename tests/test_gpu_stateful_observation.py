"""-m gpu: wrappers.per_env.FrameStackObservation / DelayObservation / TimeAwareObservation (csrc/stateful_observation.hip) against the reference's
SyncVectorEnv over scalar envs each wrapped in the gymnasium.wrappers classes of the same names, bit for bit.

The fixtures stateful_observation_<id>_<mode>.npz were recorded from the reference (tests/golden/make_golden_stateful_observation.py): 70
sub-environments (a wavefront and a partial one), 40 steps, CartPole / Pendulum / MountainCar (D = 4, 3, 2) with short episodes, the three autoreset
modes, every configuration of tests/stateful_observation_cases.py CONFIGS.  Where no fixture exists the NumPy restatement (the same module, pinned to
the fixtures by tests/test_stateful_observation_host.py) is applied to the raw outputs of an unwrapped twin env with the same seeds and actions.  The
wrappers only move data (and divide once, exactly): every comparison is array_equal."""
import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import wrappers
from gymnasium_amd.gym_api import error
from gymnasium_amd.wrappers import per_env

import stateful_observation_cases as cases

pytestmark = pytest.mark.gpu

N, T, SEED = cases.N, cases.T, cases.SEED
MODES = {"next": "NextStep", "same": "SameStep", "disabled": "Disabled"}
KEYS = [(k, m) for k in cases.IDS for m in cases.MODES]
# the configurations the rollout tests walk: every kind, the deepest stack and queue, both chains
ROLLOUT_CONFIGS = ["stack1_reset", "stack3_custom", "stack4_reset", "stack4_zero", "delay0", "delay1", "delay3", "time_int", "time_normalized", "time_dict",
                   "chain_stack_time_delay", "chain_stack_normalize"]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def base(key, mode, output="torch", num_envs=N, **kw):
    kw.setdefault("max_episode_steps", cases.LIMITS[key])
    return gymnasium_amd.make_vec(cases.IDS[key], num_envs=num_envs, output=output, autoreset_mode=MODES[mode], **kw)


def build(key, mode, name, output="torch", **kw):
    return cases.wrap(base(key, mode, output, **kw), key, cases.CONFIGS[name])


def actions_of(fix, a, b, output="torch"):
    acts = fix["actions"][a:b]
    if output == "torch":
        import torch

        return torch.from_numpy(np.array(acts)).cuda()  # (a copy: the fixtures are read-only)
    return acts


def same(got, want, raw, what):
    """One returned batch (or trajectory, or row) against the recorded one; a Dict (flatten=False) is its "time" against the recording and its "obs"
    against the unwrapped observations."""
    if isinstance(got, dict):
        assert sorted(got) == ["obs", "time"], what
        g = host(got["obs"])
        assert g.dtype == raw.dtype and np.array_equal(g, raw), (what, "obs")
        got = got["time"]
    g = host(got)
    assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), what


def check_final_obs(infos, fix, name, t):
    fm = fix["final_mask"][t]
    if not fm.any() and "_final_obs" not in infos:  # (the NumPy infos carry the key only in a step that finished an episode)
        return
    assert np.array_equal(host(infos["_final_obs"]).astype(bool), fm), ("final mask", name, t)
    final = infos["final_obs"]
    for i in np.flatnonzero(fm):
        row = {k: v[i] for k, v in final.items()} if isinstance(final, dict) else final[i]
        same(row, fix[f"{name}__final_obs"][t][i], fix["final_obs"][t][i], ("final_obs", name, t, i))


def run_against_fixture(w, fix, name, mode, output):
    obs0, _ = w.reset(seed=SEED)
    same(obs0, fix[f"{name}__obs0"], fix["obs0"], ("obs0", name))
    for t in range(T):
        o, r, te, tr, infos = w.step(actions_of(fix, t, t + 1, output)[0])
        assert np.array_equal(host(te), fix["term"][t]) and np.array_equal(host(tr), fix["trunc"][t]), ("flags", name, t)
        same(o, fix[f"{name}__obs"][t], fix["obs"][t], ("obs", name, t))
        if mode == "same":
            check_final_obs(infos, fix, name, t)
        if mode == "disabled" and fix["reset_mask"][t].any():
            ro, _ = w.reset(options={"reset_mask": fix["reset_mask"][t].copy()})
            same(ro, fix[f"{name}__reset_obs"][t], fix["reset_obs"][t], ("masked reset", name, t))


# -- 1. step() against the fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,mode", KEYS)
def test_steps_equal_the_fixtures_device_tensors(key, mode):
    fix = cases.fixture(f"{key}_{mode}")
    for name in cases.CONFIGS:
        w = build(key, mode, name)
        run_against_fixture(w, fix, name, mode, "torch")
        w.close()


@pytest.mark.parametrize("key,mode", [("cartpole", "same"), ("pendulum", "next"), ("mountaincar", "disabled"), ("pendulum", "same")])
def test_steps_equal_the_fixtures_numpy_batches(key, mode):
    fix = cases.fixture(f"{key}_{mode}")
    for name in ROLLOUT_CONFIGS:
        w = build(key, mode, name, output="numpy")
        run_against_fixture(w, fix, name, mode, "numpy")
        w.close()


# -- 2. rollouts ----------------------------------------------------------------------------------------------------------------------------------------
def check_rollout(out, fix, name, a, b):
    assert np.array_equal(host(out["terminations"]), fix["term"][a:b]) and np.array_equal(host(out["truncations"]), fix["trunc"][a:b]), (name, a, b)
    same(out["obs"], fix[f"{name}__obs"][a:b], fix["obs"][a:b], ("rollout", name, a, b))


@pytest.mark.parametrize("key", list(cases.IDS))
def test_rollouts_equal_the_fixture_next_step(key):
    """rollout(40), and rollout(7) followed by rollout(33): the second carries frames, a part-filled queue, counters and pending rows in."""
    fix = cases.fixture(f"{key}_next")
    for name in ROLLOUT_CONFIGS:
        for cuts in ((0, T), (0, 7, T)):
            w = build(key, "next", name)
            obs0, _ = w.reset(seed=SEED)
            same(obs0, fix[f"{name}__obs0"], fix["obs0"], ("obs0", name))
            for a, b in zip(cuts[:-1], cuts[1:]):
                check_rollout(w.rollout(b - a, actions_of(fix, a, b)), fix, name, a, b)
            w.close()


@pytest.mark.parametrize("key", list(cases.IDS))
def test_step_rollout_step(key):
    """step() calls, a rollout, step() calls: the pieces of one recorded run.  Two steps first: with Pendulum's limit of 2 EVERY row is pending its
    autoreset when the rollout starts."""
    fix = cases.fixture(f"{key}_next")
    pending = fix["term"][1] | fix["trunc"][1]
    assert pending.all() if key == "pendulum" else True
    for name in ROLLOUT_CONFIGS:
        w = build(key, "next", name)
        w.reset(seed=SEED)
        for t in (0, 1):
            o, *_ = w.step(actions_of(fix, t, t + 1)[0])
            same(o, fix[f"{name}__obs"][t], fix["obs"][t], ("step", name, t))
        assert np.array_equal(w.pending_autoreset, pending), name
        check_rollout(w.rollout(11, actions_of(fix, 2, 13)), fix, name, 2, 13)
        assert np.array_equal(w.pending_autoreset, fix["term"][12] | fix["trunc"][12]), name
        for t in range(13, 13 + cases.KMAX + 1):
            o, *_ = w.step(actions_of(fix, t, t + 1)[0])
            same(o, fix[f"{name}__obs"][t], fix["obs"][t], ("step after the rollout", name, t))
        w.close()


@pytest.mark.parametrize("key", list(cases.IDS))
def test_rollouts_equal_the_fixture_disabled(key):
    """DISABLED: the caller resets the rows that ended, so the fixture is a sequence of rollouts between its masked resets (each collected from steps,
    one launch per wrapper over the piece)."""
    fix = cases.fixture(f"{key}_disabled")
    for name in ("stack4_reset", "delay1", "time_normalized", "chain_stack_time_delay"):
        w = build(key, "disabled", name)
        w.reset(seed=SEED)
        a = 0
        for t in range(T):
            if fix["reset_mask"][t].any() or t == T - 1:
                check_rollout(w.rollout(t + 1 - a, actions_of(fix, a, t + 1)), fix, name, a, t + 1)
                a = t + 1
                if fix["reset_mask"][t].any():
                    ro, _ = w.reset(options={"reset_mask": fix["reset_mask"][t].copy()})
                    same(ro, fix[f"{name}__reset_obs"][t], fix["reset_obs"][t], ("masked reset", name, t))
        w.close()


def twin_run(make_base, key, name, steps, pieces, dtype=np.float32, limit=None):
    """An unwrapped env stepped ``steps`` times and the restatement applied to what it returned; a twin through the wrappers with the same seeds and
    actions, as the rollouts / steps of ``pieces`` (("rollout", n) / ("step", n)).  Returns nothing: asserts."""
    import torch

    raw, w = make_base(), cases.wrap(make_base(), key, cases.CONFIGS[name])
    o_raw, _ = raw.reset(seed=SEED)
    raw.action_space.seed(cases.ASEED)
    acts, obs, term, trunc = [], [], [], []
    for t in range(steps):
        a = raw.action_space.sample()
        o, r, te, tr, _ = raw.step(a)
        acts.append(np.asarray(a)), obs.append(host(o)), term.append(host(te)), trunc.append(host(tr))
    obs, term, trunc = np.stack(obs), np.stack(term), np.stack(trunc)
    assert obs.dtype == dtype and (term | trunc).any()
    n = obs.shape[1]
    layers = cases.build(cases.CONFIGS[name], n, obs.shape[2:], dtype, limit if limit is not None else raw.max_episode_steps, cases.CUSTOM.get(key))
    stack = cases.Stack(layers, "next")
    want0, want = stack.reset(host(o_raw)), cases.rollout(stack, obs, term, trunc)
    got0, _ = w.reset(seed=SEED)
    same(got0, want0, host(o_raw), ("obs0", name))
    actions = torch.from_numpy(np.stack(acts)).cuda()
    at = 0
    for kind, count in pieces:
        if kind == "rollout":
            out = w.rollout(count, actions[at:at + count])
            assert np.array_equal(host(out["terminations"]), term[at:at + count]) and np.array_equal(host(out["truncations"]), trunc[at:at + count])
            same(out["obs"], want[at:at + count], obs[at:at + count], ("rollout", name, at, count))
        else:
            for t in range(at, at + count):
                o, *_ = w.step(actions[t])
                same(o, want[t], obs[t], ("step", name, t))
        at += count
    assert at == steps
    raw.close(), w.close()


@pytest.mark.parametrize("name,k", [("stack4_custom", 4), ("stack3_reset", 3), ("delay3", 4), ("time_int", 4), ("chain_stack_time_delay", 3)])
@pytest.mark.parametrize("steps", ["1", "k-1", "k", "40"])
def test_rollout_equals_steps_on_a_twin(name, k, steps):
    """rollout(T) == T x step(), and the same state afterwards: both are followed by step() calls that look back through the whole rollout."""
    count = {"1": 1, "k-1": k - 1, "k": k, "40": 40}[steps]
    twin_run(lambda: base("pendulum", "next", max_episode_steps=5), "pendulum", name, 3 + count + 6, (("step", 3), ("rollout", count), ("step", 6)))


@pytest.mark.parametrize("num_envs", [1, 63, 65, 257])
def test_batch_sizes(num_envs):
    for key, name in (("cartpole", "stack4_reset"), ("pendulum", "stack3_zero"), ("pendulum", "delay3"), ("mountaincar", "time_normalized"),
                      ("pendulum", "chain_stack_time_delay")):
        twin_run(lambda: base(key, "next", num_envs=num_envs, max_episode_steps=4), key, name, 21, (("rollout", 6), ("step", 2), ("rollout", 13)))


# -- 3. float64 observations, RepeatAction underneath ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,dim", [("InvertedPendulum-v5", 4), ("HalfCheetah-v5", 17)])
def test_float64_observations(env_id, dim):
    make = lambda: gymnasium_amd.make_vec(env_id, num_envs=33, output="torch", max_episode_steps=5)  # noqa: E731
    assert make().single_observation_space.shape == (dim,)
    for name in ("stack3_reset", "stack4_zero", "delay1", "time_int", "time_normalized", "time_dict", "chain_stack_time_delay"):
        twin_run(make, None, name, 16, (("step", 2), ("rollout", 9), ("step", 5)), dtype=np.float64)


def test_over_repeat_action():
    """The wrappers see the OUTER steps: TimeAware counts one per step() while the TimeLimit underneath counts inner steps."""
    make = lambda: wrappers.RepeatAction(base("cartpole", "next", max_episode_steps=9), 2)  # noqa: E731
    for name in ("stack3_reset", "delay1", "time_int", "time_normalized"):
        twin_run(make, "cartpole", name, 20, (("step", 3), ("rollout", 12), ("step", 5)), limit=9)


# -- 4. vector wrappers above, refusals -----------------------------------------------------------------------------------------------------------------
def test_vector_wrappers_above_a_frame_stack():
    fix = cases.fixture("cartpole_next")
    name = "stack4_reset"
    w = wrappers.RecordEpisodeStatistics(wrappers.TransformReward(build("cartpole", "next", name), lambda r: 2.0 * r))
    obs0, _ = w.reset(seed=SEED)
    same(obs0, fix[f"{name}__obs0"], fix["obs0"], "obs0")
    episodes = 0
    for t in range(10):
        o, r, te, tr, infos = w.step(actions_of(fix, t, t + 1)[0])
        same(o, fix[f"{name}__obs"][t], fix["obs"][t], ("obs", t))
        pending = fix["term"][t - 1] | fix["trunc"][t - 1] if t else np.zeros(N, dtype=bool)
        assert np.array_equal(host(r), np.where(pending, 0.0, 2.0)), t  # CartPole's reward is 1.0 per step; 0.0 in the autoreset step
        episodes += int((fix["term"][t] | fix["trunc"][t]).sum())
        assert np.array_equal(host(infos["_episode"]).astype(bool), fix["term"][t] | fix["trunc"][t])
    out = w.rollout(T - 10, actions_of(fix, 10, T))
    check_rollout(out, fix, name, 10, T)
    assert int(w.episode_count) == int((fix["term"] | fix["trunc"]).sum()) > episodes
    w.close()


def test_refusals_on_the_device():
    w = build("cartpole", "same", "stack3_reset")
    w.reset(seed=SEED)
    with pytest.raises(error.Error, match="SAME_STEP"):
        w.rollout(4)
    with pytest.raises(error.Error, match="capture_steps"):
        w.capture_steps(steps=2, policy="random")
    with pytest.raises(error.Error, match="directly over"):
        per_env.NormalizeObservation(w)
    w.close()
