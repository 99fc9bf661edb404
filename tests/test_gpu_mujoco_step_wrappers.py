"""-m gpu: RepeatAction / StickyAction of the sub-environments for the eleven MuJoCo v5 ids (mi_set_step_wrappers over the MuJoCo kinds: an outer step is k
trips of the plain step's launches, csrc/mj_wrapped_kernels.h) against the hand composition of tests/mujoco_step_wrapper_cases.py over the PLAIN oracle
env -- which tests/test_mujoco_step_wrappers_host.py pins on the reference's own SyncVectorEnv over StickyAction(RepeatAction(env, 3), 0.5, 2).

Shape: 96 sub-environments (one full wavefront plus a partial one; cooperative groups of 16 and 32 lanes both end inside a wavefront), k = 3, p = 0.5,
d = 2, max_episode_steps = 7 (a truncation falls inside a repeat: 3 + 3 + 1), 12 outer steps (8 for the two humanoids), re-synchronised to the oracle's
state every 4 outer steps as test_gpu_mujoco.py does.  Exact: flags, episode lengths, engine totals, the generators' words after every outer step.
Observations, rewards, final rows at atol 1e-8 and the info entries at 1e-7: the tolerances test_gpu_mujoco.py::test_reset_bit_exact_and_windowed_parity
asserts (this project's measured HIP-vs-oracle regime).  Episode returns at 1e-7: a sum of at most 7 inner rewards, each within 1e-8.

Worst differences seen on one MI355X over all runs (docs/results_log.md, "MuJoCo step wrappers"): observations 5.7e-11 (HumanoidStandup; HalfCheetah
3.8e-11, every other robot <= 3.0e-12), rewards 3.0e-13, info entries 3.0e-13, episode returns 4.4e-13, final_obs 4.1e-12.
"""
import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import wrappers
from gymnasium_amd.gym_api import error
from mujoco_step_wrapper_cases import Composition, coverage
import model_attrs_cases as mac

pytestmark = pytest.mark.gpu

IDS = {"half_cheetah": "HalfCheetah-v5", "ant": "Ant-v5", "humanoid": "Humanoid-v5", "hopper": "Hopper-v5", "walker2d": "Walker2d-v5",
       "inverted_pendulum": "InvertedPendulum-v5", "inverted_double_pendulum": "InvertedDoublePendulum-v5", "reacher": "Reacher-v5",
       "humanoid_standup": "HumanoidStandup-v5", "swimmer": "Swimmer-v5", "pusher": "Pusher-v5"}
FIRST_INFO = {"pusher": ("reward_dist", "reward_ctrl", "reward_near"), "humanoid_standup": ("x_position", "reward_linup", "reward_quadctrl", "reward_impact"),
              "reacher": ("reward_dist", "reward_ctrl"), "inverted_pendulum": ("reward_survive",),
              "inverted_double_pendulum": ("reward_survive", "distance_penalty", "velocity_penalty")}
N, K, P, D, LIMIT, WINDOW, SEED, ASEED = 96, 3, 0.5, 2, 7, 4, 11, 2
MODES = {"next": "NextStep", "same": "SameStep", "disabled": "Disabled"}
CONFIGS = {"repeat": (K, 0.0, 0), "sticky": (0, P, D), "both": (K, P, D)}
# the default-limit runs: the outer step count for which the ORACLE ALONE shows a termination at an inner step below k in at least one row in eight
# (counted on the oracle, seed 11 / action seed 2: 60 / 77 / 80 of the 96 rows at these counts)
DEFAULT_LIMIT_STEPS = {"hopper": 8, "inverted_pendulum": 8, "inverted_double_pendulum": 4}
_WORST = {}


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def outer_steps(name):
    return 8 if name.startswith("humanoid") else 12


def wrap(env, config):
    k, p, d = CONFIGS[config]
    if k:
        env = wrappers.RepeatAction(env, k)
    if d:
        env = wrappers.StickyAction(env, p, d)
    return env


def gpu_env(name, config, mode, limit=LIMIT, output="numpy", statistics=True, **kw):
    if limit is not None:
        kw["max_episode_steps"] = limit
    env = wrap(gymnasium_amd.make_vec(IDS[name], num_envs=N, autoreset_mode=MODES[mode], output=output, **kw), config)
    return wrappers.RecordEpisodeStatistics(env) if statistics else env


def oracle_composition(name, config, mode, factory, limit=LIMIT, **kw):
    if limit is not None:
        kw["max_episode_steps"] = limit
    plain = gymnasium_amd.make_vec(IDS[name], num_envs=N, autoreset_mode="Disabled", _engine_factory=factory, **kw)
    return Composition(plain, *CONFIGS[config], MODES[mode])


def note(name, what, diff):
    key = (name, what)
    _WORST[key] = max(_WORST.get(key, 0.0), float(diff))


def check_infos(name, got, want, where):
    assert set(got) == set(want), (where, "info keys", sorted(got), sorted(want))
    for k in FIRST_INFO.get(name, ("x_position", "x_velocity", "reward_forward", "reward_ctrl")):
        if k not in want:
            continue
        assert np.array_equal(host(got["_" + k]), want["_" + k]), (where, "_" + k)
        diff = np.abs(host(got[k]).astype(np.float64) - want[k].astype(np.float64))
        note(name, "info", diff.max())
        assert diff.max() <= 1e-7, (where, k, diff.max())


def check_step(name, out, rec, where, lanes=None):
    """one outer step of the wrapped GPU env against the composition's record; `lanes`: the rows to compare (all)"""
    o, r, te, tr, infos = out
    sel = np.ones(N, dtype=bool) if lanes is None else lanes
    assert np.array_equal(host(te)[sel], rec["terminated"][sel]) and np.array_equal(host(tr)[sel], rec["truncated"][sel]), (where, "flags")
    d_obs, d_rew = np.abs(host(o) - rec["obs"])[sel].max(), np.abs(host(r) - rec["reward"])[sel].max()
    note(name, "obs", d_obs), note(name, "reward", d_rew)
    print(f"{where}: max |obs diff| {d_obs:.3e}, max |reward diff| {d_rew:.3e}")
    assert d_obs <= 1e-8, (where, "obs", d_obs)
    assert d_rew <= 1e-8, (where, "reward", d_rew)
    done = rec["terminated"] | rec["truncated"]
    if lanes is None:
        check_infos(name, {k: v for k, v in infos.items() if k not in ("episode", "_episode", "final_obs", "_final_obs", "final_info", "_final_info")},
                    {k: v for k, v in rec["infos"].items() if k not in ("final_obs", "_final_obs", "final_info", "_final_info")}, where)
    if (done & sel).any() and "episode" in infos:
        assert np.array_equal(host(infos["_episode"])[sel], done[sel]), (where, "episode mask")
        assert np.array_equal(host(infos["episode"]["l"])[sel], rec["ep_l"][sel]), (where, "episode lengths")
        d_ep = np.abs(host(infos["episode"]["r"]) - rec["ep_r"])[sel].max()
        note(name, "episode return", d_ep)
        assert d_ep <= 1e-7, (where, "episode returns", d_ep)
    if "final_obs" in rec["infos"]:
        assert np.array_equal(host(infos["_final_obs"])[sel], done[sel]), (where, "final mask")
        for i in np.flatnonzero(done & sel):
            d_f = np.abs(host(infos["final_obs"][i]) - rec["final_obs"][i]).max()
            note(name, "final_obs", d_f)
            assert d_f <= 1e-8, (where, "final_obs", i, d_f)
        if lanes is None:
            check_infos(name, infos["final_info"], rec["infos"]["final_info"], where + " final_info")


def run_against_the_oracle(name, config, mode, factory, T, limit=LIMIT):
    comp = oracle_composition(name, config, mode, factory, limit)
    gpu = gpu_env(name, config, mode, limit)
    og, _ = gpu.reset(seed=SEED)
    oc, _ = comp.reset(seed=SEED)
    assert np.array_equal(gpu.get_rng_state(), comp.env.get_rng_state())
    gpu.set_state(*comp.env.get_state())  # (the Humanoids' reset observation shows computed quantities: start from the oracle's state, as every window does)
    gpu.action_space.seed(ASEED)
    records = []
    for t in range(T):
        a = gpu.action_space.sample()
        rec = comp.step(a)
        records.append(rec)
        check_step(name, gpu.step(a), rec, f"{name} {config} {mode} t={t}")
        assert np.array_equal(gpu.get_rng_state(), rec["rng"]), (name, config, mode, t, "generator words")
        if mode == "disabled":
            done = rec["terminated"] | rec["truncated"]
            if done.any():  # masked resets: the rows that reset forget their last action and leave a running series
                o1, _ = gpu.reset(options={"reset_mask": done.copy()})
                o2, _, _ = comp.reset_rows(done)
                assert np.abs(host(o1) - o2)[done].max() <= 1e-8 and np.array_equal(gpu.get_rng_state(), comp.env.get_rng_state())
        if (t + 1) % WINDOW == 0:
            gpu.set_state(*comp.env.get_state())
    st = gpu.statistics()
    assert all(st[k] == comp.totals[k] for k in ("env_steps", "reset_steps", "episodes", "length_sum")), (st, comp.totals)
    assert abs(st["return_sum"] - comp.totals["return_sum"]) <= 1e-7 * max(1, comp.totals["episodes"])
    gpu.close(), comp.env.close()
    return records


def check_coverage(records, config, where):
    """a condition on the inputs, from the oracle's records alone"""
    k, _, d = CONFIGS[config]
    c = coverage(records, k, d)
    if k:
        assert c["trunc_inside"] > 0, (where, "no truncation at an inner step below k", c)
    if d:
        assert c["triggered"] > 0 and c["not_triggered"] > 0 and c["cut"] > 0, (where, "sticky coverage", c)
    return c


# -- 1 + 2: against the oracle composition, with the coverage of every run ----------------------------------------------------------------------------
CASES = [(name, "both", "next") for name in IDS]
CASES += [(name, config, mode) for name in ("hopper", "ant", "humanoid") for config, mode in
          (("repeat", "next"), ("sticky", "next"), ("both", "same"), ("repeat", "same"), ("sticky", "same"))]
CASES += [("hopper", "both", "disabled")]


@pytest.mark.parametrize("name,config,mode", CASES)
def test_wrapped_step_equals_the_oracle_composition(name, config, mode, oracle_factory):
    records = run_against_the_oracle(name, config, mode, oracle_factory, outer_steps(name))
    check_coverage(records, config, (name, config, mode))
    print({k: f"{v:.3e}" for k, v in _WORST.items() if k[0] == name})


@pytest.mark.parametrize("name", list(DEFAULT_LIMIT_STEPS))
def test_terminations_inside_a_repeat_at_the_default_limit(name, oracle_factory):
    records = run_against_the_oracle(name, "both", "next", oracle_factory, DEFAULT_LIMIT_STEPS[name], limit=None)
    c = coverage(records, K, D)
    assert c["term_inside_rows"] * 8 >= N, (name, "rows with a termination at an inner step below k", c)


# -- 3: rollout equals step() --------------------------------------------------------------------------------------------------------------------------
def _stack_infos(per_step):
    out = {}
    for k in per_step[0]:
        if isinstance(per_step[0][k], dict):
            out[k] = _stack_infos([s[k] for s in per_step])
        else:
            out[k] = np.stack([host(s[k]) for s in per_step])
    return out


def _same_where_masked(a, b, where):
    """rollout infos == stacked step infos wherever the key's mask is true (rollout(): zero elsewhere, step(): stale)"""
    assert set(a) == set(b), (where, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], dict):
            parent = host(b["_" + k]).astype(bool)
            for kk in a[k]:
                m = host(a[k]["_" + kk]).astype(bool) if ("_" + kk) in a[k] else parent
                x, y = host(a[k][kk]), host(b[k][kk])
                if kk == "t":
                    continue  # (a wall-clock value)
                assert np.array_equal(x[m], y[m]), (where, k, kk)
        elif k.startswith("_"):
            assert np.array_equal(host(a[k]), host(b[k])), (where, k)
        else:
            m = host(a["_" + k]).astype(bool)
            assert np.array_equal(host(a[k])[m], host(b[k])[m]), (where, k)


@pytest.mark.parametrize("name", ["hopper", "ant"])
@pytest.mark.parametrize("mode", ["next", "same"])
@pytest.mark.parametrize("how", ["sampled", "actions"])
def test_rollout_equals_steps_bit_for_bit(name, mode, how):
    import torch

    T = 6
    a, b = (gpu_env(name, "both", mode, output="torch", copy=True) for _ in range(2))
    for e in (a, b):
        e.reset(seed=SEED)
        e.action_space.seed(ASEED)
    acts = torch.stack([torch.as_tensor(host(a.action_space.sample())) for _ in range(T)]).cuda() if how == "actions" else None
    if how == "actions":
        b.action_space.seed(ASEED)
        for _ in range(T):
            b.action_space.sample()
    steps = [a.step(None if how == "sampled" else acts[t]) for t in range(T)]
    out = b.rollout(T, acts, infos=True)
    for k, key in enumerate(("obs", "rewards", "terminations", "truncations")):
        assert np.array_equal(np.stack([host(s[k]) for s in steps]), host(out[key])), (name, mode, how, key)
    _same_where_masked(out["infos"], _stack_infos([s[4] for s in steps]), (name, mode, how))
    assert np.array_equal(a.get_rng_state(), b.get_rng_state()) and a.statistics() == b.statistics() and a.statistics()["episodes"] > 0
    assert np.array_equal(host(a.action_space.sample()), host(b.action_space.sample())), "the action stream's position"
    for k in range(4):  # ... and the state the two leave behind: the next step is the same step
        assert np.array_equal(host(a.step(None)[k]), host(b.step(None)[k])), (name, mode, how, "next step", k)
    a.close(), b.close()


# -- 4: capture_steps ----------------------------------------------------------------------------------------------------------------------------------
def test_two_graph_replays_equal_six_eager_steps():
    import torch

    a, b = (gpu_env("half_cheetah", "both", "next", output="torch", statistics=False, copy=True) for _ in range(2))
    for e in (a, b):
        e.reset(seed=SEED)
        e.action_space.seed(ASEED)
        e.step(e.action_space.sample())  # kernels load on first use, which a capture must not trigger
    buf = torch.zeros((N, 6), dtype=torch.float32, device="cuda")
    graph = b.capture_steps(actions=buf, steps=3)
    for rep in range(2):
        act = a.action_space.sample()
        b.action_space.sample()
        buf.copy_(torch.as_tensor(host(act)).cuda())
        eager = [a.step(act) for _ in range(3)]
        graph.replay()
        for k in range(3):
            for x, y in zip(eager[k][:4], graph.results[k][:4]):
                assert np.array_equal(host(x), host(y)), (rep, k)
    assert np.array_equal(a.get_rng_state(), b.get_rng_state()) and a.statistics() == b.statistics() and a.statistics()["episodes"] > 0
    a.close(), b.close()


# -- 5: with per-sub-environment model fields -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["wrappers_first", "attribute_first"])
def test_repeat_action_over_per_lane_gravity(order, oracle_factory):
    name, T = "hopper", 8
    values = mac.lane_values(name, ("gravity",), N)
    sets = mac.param_sets(name)
    env = gymnasium_amd.make_vec(IDS[name], num_envs=N, max_episode_steps=LIMIT)
    if order == "attribute_first":
        env.set_attr("gravity", values["gravity"])
    gpu = wrappers.RepeatAction(env, K)
    if order == "wrappers_first":
        env.set_attr("gravity", values["gravity"])
    gpu.reset(seed=SEED)
    gpu.action_space.seed(ASEED)
    actions = [gpu.action_space.sample() for _ in range(T)]
    runs = []
    for s in range(3):  # one uniform oracle per parameter set: lane i runs set i % 3
        with mac.oracle_model(name, {"gravity": sets[s]["gravity"]}):
            comp = oracle_composition(name, "repeat", "next", oracle_factory)
            comp.reset(seed=SEED)
            recs, states = [], {}
            for t in range(T):
                recs.append(comp.step(actions[t]))
                if (t + 1) % WINDOW == 0:
                    states[t] = tuple(np.array(x) for x in comp.env.get_state())
            check_coverage(recs, "repeat", (name, "gravity set", s))
            runs.append((recs, states))
            comp.env.close()
    lanes = [np.arange(N) % 3 == s for s in range(3)]
    assert all(not np.array_equal(runs[0][0][1]["obs"], runs[s][0][1]["obs"]) for s in (1, 2)), "the sets must differ (the second step is no reset step)"
    for t in range(T):
        out = gpu.step(actions[t])
        for s in range(3):
            check_step(name, out, runs[s][0][t], f"{name} gravity {order} set {s} t={t}", lanes=lanes[s])
        if (t + 1) % WINDOW == 0:
            mixed = [np.where(lanes[0].reshape((N,) + (1,) * (runs[0][1][t][j].ndim - 1)), runs[0][1][t][j],
                              np.where(lanes[1].reshape((N,) + (1,) * (runs[0][1][t][j].ndim - 1)), runs[1][1][t][j], runs[2][1][t][j])) for j in range(3)]
            gpu.set_state(*mixed)
    gpu.close()


# -- 6: switching the wrappers off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hopper", "ant"])
def test_switched_off_the_plain_kernels_return(name):
    env = gymnasium_amd.make_vec(IDS[name], num_envs=N, max_episode_steps=LIMIT)
    twin = gymnasium_amd.make_vec(IDS[name], num_envs=N, max_episode_steps=LIMIT)
    w = wrap(env, "both")
    w.reset(seed=3)
    for _ in range(4):
        w.step(env.action_space.sample())
    env.set_step_wrappers()
    o1, _ = env.reset(seed=7)
    o2, _ = twin.reset(seed=7)
    assert np.array_equal(o1, o2)
    twin.action_space.seed(5)
    for t in range(10):
        a = twin.action_space.sample()
        for x, y in zip(env.step(a)[:4], twin.step(a)[:4]):
            assert np.array_equal(x, y), (name, t)
    assert np.array_equal(env.get_rng_state(), twin.get_rng_state())
    env.close(), twin.close()


# -- 7: the per_env stack ------------------------------------------------------------------------------------------------------------------------------------
def test_the_documented_per_env_stack_steps_and_rolls_out():
    from gymnasium_amd.wrappers import per_env

    def stack(wrapped):
        env = gymnasium_amd.make_vec("HalfCheetah-v5", num_envs=N, output="torch")
        if wrapped:
            env = wrappers.StickyAction(wrappers.RepeatAction(env, K), P, D)
        return per_env.NormalizeReward(per_env.NormalizeObservation(env))

    a, plain = stack(True), stack(False)
    for e in (a, plain):
        e.reset(seed=SEED)
        e.action_space.seed(ASEED)
    for _ in range(3):
        act = a.action_space.sample()
        o, r, te, tr, _ = a.step(act)
        plain.step(act)
        assert np.isfinite(host(o)).all() and np.isfinite(host(r)).all()
    out = a.rollout(4)
    plain.rollout(4)
    assert np.isfinite(host(out["obs"])).all() and host(out["obs"]).shape[0] == 4
    # the statistics count what the vector level sees: one observation and one reward per step(), not one per inner step
    assert np.array_equal(host(a.env.obs_rms.count), host(plain.env.obs_rms.count)) and np.array_equal(host(a.return_rms.count), host(plain.return_rms.count))
    _, elapsed, _ = a.unwrapped.get_state()
    assert (elapsed == 7 * K).all(), "TimeLimit counts inner steps"
    a.close(), plain.close()


def test_the_constructors_no_longer_refuse_and_sticky_keeps_its_element_type():
    env = wrappers.StickyAction(gymnasium_amd.make_vec("InvertedPendulum-v5", num_envs=8), 0.25)
    env.reset(seed=0)
    env.step(np.zeros((8, 1), np.float32))
    with pytest.raises(error.Error, match="element type"):
        env.step(np.zeros((8, 1), np.float64))
    env.step(np.ones((8, 1), np.float32))
    with pytest.raises(error.Error, match="MaxAndSkipObservation of the sub-environments exists for"):
        env.unwrapped.set_max_and_skip(4)
    env.close()
