"""-m gpu: per-sub-environment model fields of the MuJoCo robots (set_attr("gravity" | "actuator_gear" | "dof_damping" | "geom_friction"); the
one-lane simulator over mjx::LaneModel, csrc/mjx_model.hip) against the CPU oracle, which takes the same fields as data (tests/model_attrs_cases.py).
PARITY UNPINNED against `mujoco`, like all MuJoCo physics of this project: "HIP == oracle" is the pin.

Shapes: 96 sub-environments = less than one 256-thread workgroup but a full wavefront plus a partial one, lane i on parameter set i % 3, so the
three sets -- and, with the all-zero damping of set 1, both branches of the Euler integrator -- meet inside every wavefront; 40 steps (20 for the
two humanoids), the regime and the tolerances of tests/test_gpu_mujoco.py::test_reset_bit_exact_and_windowed_parity.

Measured on one MI355X, test 1 (55 cases): worst |GPU - oracle| 1.17e-9 on observations (HalfCheetah, dof_damping; every other robot <= 2.8e-10),
1.8e-11 on rewards; test 2: <= 7.5e-11, bit-identical for Walker2d and InvertedDoublePendulum (docs/results_log.md)."""
import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd.gym_api import error

from model_attrs_cases import FIELDS, ROBOTS, lane_values, next_step_counts, param_sets, record_oracle, stock
from rollout_infos_cases import caller_actions, compare_infos, make_pair, stack_steps

pytestmark = pytest.mark.gpu
N = 96
NSTATE = {"half_cheetah": 17, "ant": 27, "humanoid": 45, "hopper": 11, "walker2d": 17, "inverted_pendulum": 4, "inverted_double_pendulum": 0, "reacher": 0,
          "humanoid_standup": 45, "swimmer": 8, "pusher": 14}  # the part of the reset observation that is pure generator arithmetic (test_gpu_mujoco.py)
CASES = [(f,) for f in FIELDS] + [FIELDS]
_RECORDED = {}


def _shape(name):
    return (20, 5) if name.startswith("humanoid") else (40, 10)


_ACTIONS = {}


def _actions(name, T):
    """T batches of the env's own action space, seeded; computed once per robot."""
    if (name, T) not in _ACTIONS:
        env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N)
        env.action_space.seed(2)
        _ACTIONS[name, T] = [env.action_space.sample() for _ in range(T)]
        env.close()
    return _ACTIONS[name, T]


def _oracle(name, fields, s, oracle_factory, actions):
    """The recorded oracle run of set s restricted to `fields` (the other fields stock); set 0 is the stock model whatever the fields.  Computed once."""
    key = (name, fields if s else (), s)
    if key not in _RECORDED:
        T, window = _shape(name)
        values = {f: param_sets(name)[s][f] for f in fields} if s else {}
        _RECORDED[key] = record_oracle(name, values, N, T, window, 11, actions, oracle_factory)
    return _RECORDED[key]


def _select(per_set):
    """Lane i from the array of set i % 3."""
    return np.stack(per_set)[np.arange(N) % 3, np.arange(N)]


def _set_lanes(env, name, fields):
    for f, vals in lane_values(name, fields, N).items():
        env.set_attr(f, vals)


@pytest.mark.parametrize("fields", CASES, ids=lambda f: "+".join(f) if len(f) < 4 else "all")
@pytest.mark.parametrize("name", list(ROBOTS))
def test_per_lane_physics_equals_the_oracle(name, fields, oracle_factory):
    T, window = _shape(name)
    actions = _actions(name, T)
    recs = [_oracle(name, fields, s, oracle_factory, actions) for s in range(3)]
    for r in recs:  # the flag bookkeeping of this test, pinned on the oracle's own counts over all its lanes
        assert all(r["stats"][k] == v for k, v in next_step_counts(r["te"], r["tr"]).items())
    # values that are ignored cannot pass: the sets' trajectories differ
    m = stock(name)
    for f in fields:
        apart = max(float(np.abs(a - b).max()) for s in (1, 2) for a, b in zip(recs[0]["obs"], _oracle(name, (f,), s, oracle_factory, actions)["obs"]))
        print(f"{name} {f}: oracle trajectories of the sets differ by up to {apart:.3e}")
        if f == "geom_friction" and (len(m.pair_geom1) == 0 or m.pair_condim.max() <= 1):
            # No frictional contact can occur: a robot without contact pairs, or whose pairs are all condim 1 (pusher.xml: frictionless contacts, the
            # solver never reads their friction) -- read off the compiled model, so a model that gains a frictional pair is held to the assertion.
            assert apart == 0.0, f"{name}: friction changed a trajectory although no pair of the model is frictional"
            continue
        assert apart > 1e-3, f"{name}: the sets of {f} give the same oracle trajectory"
    gpu = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N)
    _set_lanes(gpu, name, fields)
    og, _ = gpu.reset(seed=11)
    oc = _select([r["reset_obs"] for r in recs])
    ns = NSTATE[name]
    assert og.dtype == np.float64 and np.array_equal(og[:, :ns], oc[:, :ns]), "reset state must be bit-exact"
    np.testing.assert_allclose(og[:, ns:], oc[:, ns:], rtol=1e-9, atol=1e-9)
    assert np.array_equal(gpu.get_rng_state(), _select([r["reset_rng"] for r in recs]))
    worst = worst_r = 0.0
    for t in range(T):
        og, rg, teg, trg, _ = gpu.step(actions[t])
        oc, rc = _select([r["obs"][t] for r in recs]), _select([r["rew"][t] for r in recs])
        assert np.array_equal(teg, _select([r["te"][t] for r in recs])) and np.array_equal(trg, _select([r["tr"][t] for r in recs])), f"{name} flags t={t}"
        worst, worst_r = max(worst, float(np.abs(og - oc).max())), max(worst_r, float(np.abs(rg - rc).max()))
        np.testing.assert_allclose(og, oc, rtol=0, atol=1e-8, err_msg=f"{name} obs t={t}")
        np.testing.assert_allclose(rg, rc, rtol=0, atol=1e-8, err_msg=f"{name} reward t={t}")
        if (t + 1) % window == 0:
            gpu.set_state(*(_select([r["states"][t][k] for r in recs]) for k in range(3)))
    print(f"{name} {'+'.join(fields)}: max |obs diff| {worst:.3e}, max |reward diff| {worst_r:.3e} over {T} steps x {N} envs (resync every {window})")
    assert np.array_equal(gpu.get_rng_state(), _select([r["rng"] for r in recs]))
    want = next_step_counts([_select([r["te"][t] for r in recs]) for t in range(T)], [_select([r["tr"][t] for r in recs]) for t in range(T)])
    got = gpu.statistics()
    assert all(got[k] == v for k, v in want.items()), (got, want)
    for f in fields:  # resets and steps did not undo the fields
        assert all(np.array_equal(a, b) for a, b in zip(gpu.get_attr(f), lane_values(name, (f,), N)[f]))
    gpu.close()


SERIAL_ROBOTS = ["half_cheetah", "ant", "humanoid", "hopper", "walker2d", "inverted_double_pendulum"]  # test_gpu_mujoco.py COOP_ROBOTS and one small robot


def _per_lane_defaults(name, **kw):
    env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N, **kw)
    env.set_attr("gravity", stock(name).gravity)
    return env


@pytest.mark.parametrize("name", SERIAL_ROBOTS)
def test_defaults_through_the_per_lane_kernels_equal_the_stock_one_lane_kernel(name, monkeypatch):
    """The regime of test_gpu_mujoco.py::test_cooperative_kernel_equals_one_lane_simulator: two HIP builds of the same physics, atol 1e-8 per 5-step window."""
    T, window = (30, 5) if name != "humanoid" else (20, 5)
    monkeypatch.setenv("MI355ENV_MJ_SERIAL", "1")
    ser = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N)
    monkeypatch.delenv("MI355ENV_MJ_SERIAL")
    monkeypatch.setenv("MI355ENV_MJ_COOP", "1")  # (does not bring the cooperative kernel back once a field is set)
    lane = _per_lane_defaults(name)
    monkeypatch.delenv("MI355ENV_MJ_COOP")
    o1, _ = ser.reset(seed=21)
    o2, _ = lane.reset(seed=21)
    assert np.array_equal(o1, o2)
    ser.action_space.seed(4)
    worst, same = 0.0, True
    for t in range(T):
        a = ser.action_space.sample()
        o1, r1, te1, tr1, _ = ser.step(a)
        o2, r2, te2, tr2, _ = lane.step(a)
        assert np.array_equal(te1, te2) and np.array_equal(tr1, tr2)
        worst, same = max(worst, float(np.abs(o1 - o2).max())), same and np.array_equal(o1, o2) and np.array_equal(r1, r2)
        np.testing.assert_allclose(o2, o1, rtol=0, atol=1e-8, err_msg=f"{name} obs t={t}")
        np.testing.assert_allclose(r2, r1, rtol=0, atol=1e-8, err_msg=f"{name} reward t={t}")
        if (t + 1) % window == 0:
            lane.set_state(*ser.get_state())
    assert np.array_equal(ser.get_rng_state(), lane.get_rng_state())
    print(f"{name}: per-lane kernel at default values vs stock one-lane kernel: max |obs diff| {worst:.3e}, bit-identical: {same}")
    ser.close(), lane.close()


def _set_pair(a, b, name):
    for env in (a, b):
        _set_lanes(env, name, FIELDS)


@pytest.mark.parametrize("policy", ["device", "caller"])
@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("name", ["hopper", "inverted_pendulum"])
def test_rollout_equals_steps_with_all_fields_set(name, mode, policy):
    """max_episode_steps = 7: short episodes, many resets inside the window -- which must not undo the fields."""
    import torch

    T = 19
    a, b = make_pair(ROBOTS[name], N, 7, mode, False)
    _set_pair(a, b, name)
    acts = caller_actions(a, T) if policy == "caller" else None
    out = a.rollout(T, actions=acts, infos=True)
    (obs, rew, te, tr, act), infos = stack_steps(b, T, actions=acts)
    assert torch.equal(out["obs"], obs) and torch.equal(out["rewards"], rew) and torch.equal(out["terminations"], te) and torch.equal(out["truncations"], tr)
    assert torch.equal(out["actions"], act)
    compare_infos(infos, out["infos"], zero_fill=True)
    dones = (te | tr).cpu().numpy()
    assert dones.sum() >= 2 * N, "every sub-environment must have finished (and reset) at least twice"
    assert np.array_equal(a.get_rng_state(), b.get_rng_state()) and np.array_equal(a.get_state()[0], b.get_state()[0])
    out2 = a.rollout(5, infos=False)  # ... and without the extras (the other rollout entry point)
    (obs2, rew2, _, _, _), _ = stack_steps(b, 5)
    assert torch.equal(out2["obs"], obs2) and torch.equal(out2["rewards"], rew2)
    # the fields made a difference, and survived
    c = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N, max_episode_steps=7, autoreset_mode=mode, output="torch")
    c.reset(seed=5), c.action_space.seed(9)
    plain = c.rollout(T, actions=acts)
    assert not torch.equal(plain["obs"], out["obs"])
    sel = torch.arange(N, device=obs.device) % 3 == 0  # lanes on set 0 run the stock model (another instantiation of the same code: test 2's tolerance)
    assert float((plain["obs"][0][sel] - out["obs"][0][sel]).abs().max()) <= 1e-8
    a.close(), b.close(), c.close()


def test_rollout_equals_steps_ant_next_step():
    import torch

    a, b = make_pair("Ant-v5", N, 7, "NextStep", False)
    _set_pair(a, b, "ant")
    out = a.rollout(12, infos=True)
    (obs, rew, te, tr, act), infos = stack_steps(b, 12)
    assert torch.equal(out["obs"], obs) and torch.equal(out["rewards"], rew) and torch.equal(out["terminations"], te) and torch.equal(out["truncations"], tr)
    compare_infos(infos, out["infos"], zero_fill=True)
    a.close(), b.close()


def test_disabled_autoreset_steps_with_fields_set():
    """The engine has no rollout launch for a DISABLED env; its per-lane step kernel equals the NEXT_STEP one until the first episode ends."""
    kw = dict(num_envs=N, max_episode_steps=7)
    a = gymnasium_amd.make_vec("Hopper-v5", autoreset_mode="Disabled", **kw)
    b = gymnasium_amd.make_vec("Hopper-v5", autoreset_mode="NextStep", **kw)
    _set_pair(a, b, "hopper")
    a.reset(seed=5), b.reset(seed=5)
    b.action_space.seed(3)
    steps = 0
    while True:
        act = b.action_space.sample()
        ra, rb = a.step(act), b.step(act)
        assert all(np.array_equal(x, y) for x, y in zip(ra[:4], rb[:4]))
        steps += 1
        if (ra[2] | ra[3]).any():
            break
    assert 2 <= steps <= 7
    a.close(), b.close()


def _run(env, actions):
    out = []
    for a in actions:
        o, r, te, tr, _ = env.step(a)
        out.append((o.copy(), r.copy(), te.copy(), tr.copy()))
    return out


def _same(x, y):
    return all(np.array_equal(a, b) for sx, sy in zip(x, y) for a, b in zip(sx, sy))


def test_set_semantics():
    import torch

    name, T = "walker2d", 8
    m = stock(name)
    actions = _actions(name, 2 * T)
    vals = lane_values(name, FIELDS, N)
    # a set between two steps takes effect at the next step and not before
    plain, late = (gymnasium_amd.make_vec(ROBOTS[name], num_envs=N) for _ in range(2))
    plain.reset(seed=1), late.reset(seed=1)
    first = _run(plain, actions[:T]), _run(late, actions[:T])
    assert _same(*first)
    for f in FIELDS:
        late.set_attr(f, vals[f])
    second = _run(plain, actions[T:T + 1]), _run(late, actions[T:T + 1])
    sel = np.arange(N) % 3 == 0
    np.testing.assert_allclose(second[1][0][0][sel], second[0][0][0][sel], rtol=0, atol=1e-8)  # set 0 is the stock model (test 2's tolerance)
    assert float(np.abs(second[0][0][0][~sel] - second[1][0][0][~sel]).max()) > 1e-6
    # host list, host broadcast array and device tensor give bit-identical trajectories; the get_attr round trip is exact
    envs = {k: gymnasium_amd.make_vec(ROBOTS[name], num_envs=N, output="torch" if k == "tensor" else "numpy") for k in ("list", "tensor")}
    for f in FIELDS:
        envs["list"].set_attr(f, vals[f])
        envs["tensor"].set_attr(f, torch.from_numpy(np.stack(vals[f])).cuda())
    for k, env in envs.items():
        for f in FIELDS:
            got = env.get_attr(f)
            assert len(got) == N and all(g.dtype == np.float64 and np.array_equal(g, v) for g, v in zip(got, vals[f])), (k, f)
    for env in envs.values():
        env.reset(seed=1)
    ref = _run(envs["list"], actions)
    for t, a in enumerate(actions):
        o, r, te, tr, _ = envs["tensor"].step(torch.from_numpy(a).cuda())
        assert np.array_equal(o.cpu().numpy(), ref[t][0]) and np.array_equal(r.cpu().numpy(), ref[t][1]) and np.array_equal(te.cpu().numpy(), ref[t][2])
    uniform = {f: param_sets(name)[2][f] for f in FIELDS}
    b1, b2 = (gymnasium_amd.make_vec(ROBOTS[name], num_envs=N) for _ in range(2))
    for f in FIELDS:
        b1.set_attr(f, uniform[f])  # anything but a list or tuple: the same array for all
        b2.set_attr(f, [uniform[f]] * N)
    b1.reset(seed=1), b2.reset(seed=1)
    assert _same(_run(b1, actions), _run(b2, actions))
    # the stock values after a non-stock set: the trajectories of the per-lane-defaults env, bit for bit
    back, dflt = envs["list"], _per_lane_defaults(name)
    stock_vals = {"gravity": m.gravity, "actuator_gear": m.actuator_gear, "dof_damping": m.dof_damping, "geom_friction": m.geom_friction[:, 0]}
    for i, f in enumerate(FIELDS):
        back.set_attr(f, None if i % 2 else stock_vals[f])  # (None restores the compiled model's values)
        assert all(np.array_equal(g, stock_vals[f]) for g in back.get_attr(f))
    back.reset(seed=1), dflt.reset(seed=1)
    assert _same(_run(back, actions), _run(dflt, actions))
    # the engine refuses what the host class would have refused (a binding of its own meets these)
    eng = back._engine
    for fid, bad in ((0, np.nan), (2, -1.0), (3, 0.5e-5)):
        rows = eng.get_model_field(fid)
        rows[N - 1, -1] = bad
        with pytest.raises(Exception, match="mi_set_model_field"):
            eng.set_model_field(fid, rows)
    for env in (plain, late, b1, b2, dflt, *envs.values()):
        env.close()
    cart = gymnasium_amd.make_vec("CartPole-v1", num_envs=4)
    assert cart._engine.model_field_width(0) < 0
    with pytest.raises(Exception, match="MuJoCo kinds only"):
        cart._engine.set_model_field(0, None)
    cart.close()


def test_swimmer_accepts_geom_friction_and_it_changes_nothing():
    a, b = (gymnasium_amd.make_vec("Swimmer-v5", num_envs=N) for _ in range(2))
    a.set_attr("geom_friction", lane_values("swimmer", ("geom_friction",), N)["geom_friction"])
    b.set_attr("gravity", stock("swimmer").gravity)
    a.reset(seed=2), b.reset(seed=2)
    actions = _actions("swimmer", 6)
    assert _same(_run(a, actions), _run(b, actions))
    a.close(), b.close()


def test_newton_humanoid_honours_the_fields(oracle_factory):
    """One window against the oracle with the same option, at the agreement test_gpu_mujoco.py::test_humanoid_solver_choice asserts for it."""
    name, T = "humanoid", 5
    actions = _actions(name, T)
    recs = [record_oracle(name, param_sets(name)[s] if s else {}, N, T, T, 8, actions, oracle_factory, solver="Newton") for s in range(3)]
    gpu = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N, solver="Newton")
    _set_lanes(gpu, name, FIELDS)
    gpu.reset(seed=8)
    apart = 0.0
    for t in range(T):
        og, rg, teg, _, _ = gpu.step(actions[t])
        np.testing.assert_allclose(og, _select([r["obs"][t] for r in recs]), rtol=0, atol=1e-7, err_msg=f"obs t={t}")
        np.testing.assert_allclose(rg, _select([r["rew"][t] for r in recs]), rtol=1e-9, atol=1e-7, err_msg=f"reward t={t}")
        assert np.array_equal(teg, _select([r["te"][t] for r in recs]))
        apart = max(apart, float(np.abs(recs[0]["obs"][t] - recs[1]["obs"][t]).max()))
    assert apart > 1e-3
    gpu.close()


def test_graphs():
    import torch

    name = "hopper"
    a, b = make_pair(ROBOTS[name], N, 7, "NextStep", False)
    a.step(torch.from_numpy(a.action_space.sample()).cuda()), b.step(torch.from_numpy(b.action_space.sample()).cuda())
    early = a.capture_steps(policy="random", steps=4)  # before the first set: holds the stock kernels
    _set_pair(a, b, name)
    with pytest.raises(error.Error, match="capture the steps again"):
        early.replay()
    graph = a.capture_steps(policy="random", steps=4)  # straight after the first set: the set has loaded the per-lane kernels

    def replay_equals_four_steps():
        got = graph.replay()
        for _ in range(4):
            o, r, te, tr, _ = b.step(None)
        assert torch.equal(got[0], o) and torch.equal(got[1], r) and torch.equal(got[2], te) and torch.equal(got[3], tr)
        assert np.array_equal(a.get_state()[0], b.get_state()[0]) and np.array_equal(a.get_rng_state(), b.get_rng_state())

    for _ in range(3):  # 12 steps with max_episode_steps = 7: resets inside the replays
        replay_equals_four_steps()
    # the rows live in device memory updated in place: a graph captured after the switch sees a later set
    g2 = param_sets(name)[2]["gravity"]
    a.set_attr("gravity", g2), b.set_attr("gravity", g2)
    replay_equals_four_steps()
    with pytest.raises(error.Error, match="capture the steps again"):
        early.replay()
    a.close(), b.close()


def test_seeding_without_a_reset_leaves_the_state_alone():
    """mi_seed / mi_seed_sequence are calls of their own in the C ABI.  Their kernels read the tabular table's first integer (the Blackjack marker)
    for every kind: the model rows' pointer must not share its bytes, or a re-seed in the middle of an episode zeroes qpos[1] of the seeded lanes
    whenever bit 31 of the address is set."""
    for name in ("hopper", "ant"):
        env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N)
        _set_lanes(env, name, FIELDS)
        env.reset(seed=3)
        for a in _actions(name, _shape(name)[0])[:3]:
            env.step(a)
        before = [np.array(x) for x in env.get_state()]
        assert np.abs(before[0][:, 1]).min() > 0.0, "qpos[1] must be non-zero for the check to see anything"
        rng0 = env.get_rng_state().copy()
        env._engine.seed_sequence(77, 0)
        mid = [np.array(x) for x in env.get_state()]
        words = env.get_rng_state().copy()
        env._engine.seed(words[::-1].copy())
        after = [np.array(x) for x in env.get_state()]
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(before, mid, after)), name
        assert not np.array_equal(rng0, words) and np.array_equal(env.get_rng_state(), words[::-1])
        env.close()
