"""-m gpu: per-sub-environment body mass scale of the MuJoCo robots (set_attr("body_mass_scale"); the constants derived from it on the device by
mj_model_constants_kernel, csrc/mjx_mass_model.hip, and the one-lane simulator reading them through mjx::MassLaneModel) against compiler.scaled and against
the CPU oracle running compiler.scaled's model as data (tests/body_mass_cases.py).
PARITY UNPINNED against `mujoco`, like all MuJoCo physics of this project: "HIP == oracle" is the pin.

Shapes: the regime of tests/test_gpu_model_attrs.py -- 96 sub-environments (a full wavefront plus a partial one), lane i on set i % 3, 40 steps (20 for
the two humanoids), resynchronised every 10 (5), atol 1e-8 (tests/test_gpu_mujoco.py's own); the derived constants also with 1 and 65 sub-environments.

Measured on one MI355X (59 tests in 25 s): device-derived constants within 3.7e-14 relative of compiler.scaled (Humanoid, set 2; every robot within 1.4
times the host build's figure); worst |GPU - oracle| 5.5e-9 on observations (HalfCheetah, the mass scale alone; every other robot <= 1.7e-10), 1.3e-10
on rewards; Newton Humanoid 1.0e-11 (docs/results_log.md)."""
import numpy as np
import pytest

import gymnasium_amd

from body_mass_cases import DERIVED, compare_derived, lane_scales, record_oracle, scale_sets
from model_attrs_cases import FIELDS, ROBOTS, lane_values, param_sets, stock
from rollout_infos_cases import compare_infos, make_pair, stack_steps

pytestmark = pytest.mark.gpu
N = 96
FIELD = "body_mass_scale"
NSTATE = {"half_cheetah": 17, "ant": 27, "humanoid": 45, "hopper": 11, "walker2d": 17, "inverted_pendulum": 4, "inverted_double_pendulum": 0, "reacher": 0,
          "humanoid_standup": 45, "swimmer": 8, "pusher": 14}  # the part of the reset observation that is pure generator arithmetic (test_gpu_mujoco.py)
_RECORDED, _ACTIONS = {}, {}


def _shape(name):
    return (20, 5) if name.startswith("humanoid") else (40, 10)


def _actions(name, T):
    """T batches of the env's own action space, seeded; computed once per robot."""
    if (name, T) not in _ACTIONS:
        env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N)
        env.action_space.seed(2)
        _ACTIONS[name, T] = [env.action_space.sample() for _ in range(T)]
        env.close()
    return _ACTIONS[name, T]


def _select(per_set, n=N):
    """Lane i from the array of set i % 3."""
    return np.stack(per_set)[np.arange(n) % 3, np.arange(n)]


@pytest.mark.parametrize("n", [1, 65, 96])
@pytest.mark.parametrize("name", list(ROBOTS))
def test_derived_constants_equal_compiler_scaled(name, n):
    m, sets = stock(name), scale_sets(name)
    env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=n)
    for k in DERIVED:  # before any set: the compiled model's values
        assert all(np.array_equal(r, np.asarray(getattr(m, k))) for r in env.get_attr(k))
    env.set_attr(FIELD, lane_scales(name, n))
    got = {k: env.get_attr(k) for k in DERIVED}
    assert all(len(v) == n for v in got.values())
    worst = [0.0, 0.0, 0.0]
    for i in range(n):
        worst[i % 3] = max(worst[i % 3], compare_derived(name, {k: got[k][i] for k in DERIVED}, sets[i % 3]))
    print(f"{name} N={n}: worst relative difference of the device-derived constants from compiler.scaled, per set: " + ", ".join(f"{w:.3e}" for w in worst))
    assert all(np.array_equal(a, b) for a, b in zip(env.get_attr(FIELD), lane_scales(name, n)))  # get_attr returns what was given
    if n > 3:  # lanes of one set hold the same values bit for bit, and the sets differ
        for k in DERIVED:
            assert all(np.array_equal(got[k][i], got[k][i % 3]) for i in range(n))
        assert not np.array_equal(got["dof_invweight0"][0], got["dof_invweight0"][1]) and not np.array_equal(got["meaninertia"][0], got["meaninertia"][2])
    env.set_attr(FIELD, None)  # the compiled constants again, copied and not derived
    for k in DERIVED:
        assert all(np.array_equal(r, np.asarray(getattr(m, k))) for r in env.get_attr(k)), k
    assert all(np.array_equal(r, np.ones(m.nbody)) for r in env.get_attr(FIELD))
    env.close()


def _oracle(name, case, s, oracle_factory, actions, **kw):
    """The recorded oracle run of set s: the mass scale alone ("mass") or together with the other four fields ("all"); set 0 is the stock model."""
    key = (name, case if s else "stock", s, tuple(sorted(kw.items())))
    if key not in _RECORDED:
        T, window = _shape(name)
        values = param_sets(name)[s] if (case == "all" and s) else {}
        _RECORDED[key] = record_oracle(name, scale_sets(name)[s], values, N, T, window, 11, actions, oracle_factory, **kw)
    return _RECORDED[key]


def _set_lanes(env, name, case):
    env.set_attr(FIELD, lane_scales(name, N))
    if case == "all":
        for f, vals in lane_values(name, FIELDS, N).items():
            env.set_attr(f, vals)


@pytest.mark.parametrize("case", ["mass", "all"])
@pytest.mark.parametrize("name", list(ROBOTS))
def test_trajectories_equal_the_oracle(name, case, oracle_factory):
    T, window = _shape(name)
    actions = _actions(name, T)
    recs = [_oracle(name, case, s, oracle_factory, actions) for s in range(3)]
    assert all(np.isfinite(np.stack(r["obs"])).all() for r in recs), f"{name}: the oracle itself diverges on one of the sets (body_mass_cases.FLOOR_BODY)"
    # a scale that is ignored cannot pass: the oracle's runs of set 0 and set 1 differ
    apart = max(float(np.abs(a - b).max()) for a, b in zip(recs[0]["obs"], _oracle(name, "mass", 1, oracle_factory, actions)["obs"]))
    print(f"{name}: oracle trajectories of mass set 0 and set 1 differ by up to {apart:.3e}")
    assert apart > 1e-3, f"{name}: the mass sets give the same oracle trajectory"
    gpu = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N)
    _set_lanes(gpu, name, case)
    og, _ = gpu.reset(seed=11)
    oc = _select([r["reset_obs"] for r in recs])
    ns = NSTATE[name]
    assert og.dtype == np.float64 and np.array_equal(og[:, :ns], oc[:, :ns]), "reset state must be bit-exact"
    np.testing.assert_allclose(og[:, ns:], oc[:, ns:], rtol=1e-9, atol=1e-9)  # (the Humanoids' cinert reads the lane's masses)
    assert np.array_equal(gpu.get_rng_state(), _select([r["reset_rng"] for r in recs]))
    worst = worst_r = 0.0
    for t in range(T):
        og, rg, teg, trg, _ = gpu.step(actions[t])
        oc, rc = _select([r["obs"][t] for r in recs]), _select([r["rew"][t] for r in recs])
        assert np.array_equal(teg, _select([r["te"][t] for r in recs])) and np.array_equal(trg, _select([r["tr"][t] for r in recs])), f"{name} flags t={t}"
        worst, worst_r = max(worst, float(np.abs(og - oc).max())), max(worst_r, float(np.abs(rg - rc).max()))
        print(f"{name} {case} t={t}: max |obs diff| {float(np.abs(og - oc).max()):.3e}, max |reward diff| {float(np.abs(rg - rc).max()):.3e}")
        np.testing.assert_allclose(og, oc, rtol=0, atol=1e-8, err_msg=f"{name} obs t={t}")
        np.testing.assert_allclose(rg, rc, rtol=0, atol=1e-8, err_msg=f"{name} reward t={t}")
        if (t + 1) % window == 0:
            gpu.set_state(*(_select([r["states"][t][k] for r in recs]) for k in range(3)))
    print(f"{name} {case}: max |obs diff| {worst:.3e}, max |reward diff| {worst_r:.3e} over {T} steps x {N} envs (resync every {window})")
    assert np.array_equal(gpu.get_rng_state(), _select([r["rng"] for r in recs]))
    assert all(np.array_equal(a, b) for a, b in zip(gpu.get_attr(FIELD), lane_scales(name, N)))  # resets and steps did not undo the field
    gpu.close()


def test_newton_humanoid_honours_the_mass_scale(oracle_factory):
    """One window against the oracle with the same option, at the agreement test_gpu_mujoco.py::test_humanoid_solver_choice asserts for it."""
    name, T = "humanoid", 5
    actions = _actions(name, T)
    recs = [record_oracle(name, scale_sets(name)[s], {}, N, T, T, 8, actions, oracle_factory, solver="Newton") for s in range(3)]
    gpu = gymnasium_amd.make_vec(ROBOTS[name], num_envs=N, solver="Newton")
    gpu.set_attr(FIELD, lane_scales(name, N))
    gpu.reset(seed=8)
    apart = worst = 0.0
    for t in range(T):
        og, rg, teg, _, _ = gpu.step(actions[t])
        worst = max(worst, float(np.abs(og - _select([r["obs"][t] for r in recs])).max()))
        np.testing.assert_allclose(og, _select([r["obs"][t] for r in recs]), rtol=0, atol=1e-7, err_msg=f"obs t={t}")
        np.testing.assert_allclose(rg, _select([r["rew"][t] for r in recs]), rtol=1e-9, atol=1e-7, err_msg=f"reward t={t}")
        assert np.array_equal(teg, _select([r["te"][t] for r in recs]))
        apart = max(apart, float(np.abs(recs[0]["obs"][t] - recs[1]["obs"][t]).max()))
    print(f"humanoid Newton: max |obs diff| {worst:.3e}; sets 0 and 1 apart by {apart:.3e}")
    assert apart > 1e-3
    gpu.close()


@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
def test_rollout_equals_steps_with_the_mass_scale_set(mode):
    """max_episode_steps = 7: short episodes, many resets inside the window -- which must not undo the field."""
    import torch

    T = 19
    a, b = make_pair("Hopper-v5", N, 7, mode, False)
    for env in (a, b):
        env.set_attr(FIELD, lane_scales("hopper", N))
    out = a.rollout(T, infos=True)
    (obs, rew, te, tr, act), infos = stack_steps(b, T)
    compare_infos(infos, out["infos"], zero_fill=True)
    assert torch.equal(out["obs"], obs) and torch.equal(out["rewards"], rew) and torch.equal(out["terminations"], te) and torch.equal(out["truncations"], tr)
    assert torch.equal(out["actions"], act)
    assert int((te | tr).sum()) >= 2 * N, "every sub-environment must have finished (and reset) at least twice"
    assert np.array_equal(a.get_rng_state(), b.get_rng_state()) and np.array_equal(a.get_state()[0], b.get_state()[0])
    c = gymnasium_amd.make_vec("Hopper-v5", num_envs=N, max_episode_steps=7, autoreset_mode=mode, output="torch")  # the field made a difference
    c.reset(seed=5), c.action_space.seed(9)
    assert not torch.equal(c.rollout(T, actions=out["actions"])["obs"], out["obs"])
    a.close(), b.close(), c.close()


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
    actions = _actions(name, 40)[:2 * T]
    scales = lane_scales(name, N)
    # a set between two steps, without a reset: the state stays bit-identical and the next step runs the new masses
    plain, late = (gymnasium_amd.make_vec(ROBOTS[name], num_envs=N) for _ in range(2))
    plain.reset(seed=1), late.reset(seed=1)
    assert _same(_run(plain, actions[:T]), _run(late, actions[:T]))
    late.set_attr(FIELD, scales)
    assert all(np.array_equal(x, y) for x, y in zip(plain.get_state(), late.get_state())) and np.array_equal(plain.get_rng_state(), late.get_rng_state())
    second = _run(plain, actions[T:T + 1]), _run(late, actions[T:T + 1])
    sel = np.arange(N) % 3 == 0
    np.testing.assert_allclose(second[1][0][0][sel], second[0][0][0][sel], rtol=0, atol=1e-8)  # set 0 is the stock model (another instantiation of the same code)
    assert float(np.abs(second[0][0][0][~sel] - second[1][0][0][~sel]).max()) > 1e-6
    # host list, host broadcast array and device tensor give bit-identical trajectories; the get_attr round trip is exact
    envs = {k: gymnasium_amd.make_vec(ROBOTS[name], num_envs=N, output="torch" if k == "tensor" else "numpy") for k in ("list", "tensor")}
    envs["list"].set_attr(FIELD, scales)
    envs["tensor"].set_attr(FIELD, torch.from_numpy(np.stack(scales)).cuda())
    for k, env in envs.items():
        got = env.get_attr(FIELD)
        assert len(got) == N and all(g.dtype == np.float64 and np.array_equal(g, v) for g, v in zip(got, scales)), k
        for d in DERIVED:  # the same kernel derived the same constants from both
            assert all(np.array_equal(x, y) for x, y in zip(env.get_attr(d), envs["list"].get_attr(d)))
    for env in envs.values():
        env.reset(seed=1)
    ref = _run(envs["list"], actions)
    for t, a in enumerate(actions):
        o, r, te, tr, _ = envs["tensor"].step(torch.from_numpy(a).cuda())
        assert np.array_equal(o.cpu().numpy(), ref[t][0]) and np.array_equal(r.cpu().numpy(), ref[t][1]) and np.array_equal(te.cpu().numpy(), ref[t][2])
    uniform = scale_sets(name)[2]
    b1, b2 = (gymnasium_amd.make_vec(ROBOTS[name], num_envs=N) for _ in range(2))
    b1.set_attr(FIELD, uniform)  # anything but a list or tuple: the same array for all
    b2.set_attr(FIELD, [uniform] * N)
    b1.reset(seed=1), b2.reset(seed=1)
    assert _same(_run(b1, actions), _run(b2, actions))
    # an env that sets only gravity, and one that sets gravity and then body_mass_scale = None: bit for bit the same trajectory
    g = param_sets(name)[2]["gravity"]
    only, both = (gymnasium_amd.make_vec(ROBOTS[name], num_envs=N) for _ in range(2))
    only.set_attr("gravity", g)
    both.set_attr("gravity", g), both.set_attr(FIELD, None)
    only.reset(seed=1), both.reset(seed=1)
    assert _same(_run(only, actions), _run(both, actions))
    # ... and after a non-stock scale, None brings that trajectory back as well
    both.set_attr(FIELD, scales), both.set_attr(FIELD, None)
    only.reset(seed=2), both.reset(seed=2)
    assert _same(_run(only, actions[:T]), _run(both, actions[:T]))
    # the engine refuses what the host class would have refused (a binding of its own meets these)
    eng = both._engine
    for bad in (np.nan, 0.5e-3):
        rows = eng.get_model_field(4)
        assert rows.shape == (N, m.nbody)
        rows[N - 1, -1] = bad
        with pytest.raises(Exception, match="mi_set_model_field"):
            eng.set_model_field(4, rows)
    assert all(np.array_equal(r, np.ones(m.nbody)) for r in both.get_attr(FIELD))  # nothing was stored
    for env in (plain, late, b1, b2, only, both, *envs.values()):
        env.close()
