"""Shared by tests/test_body_mass_host.py and tests/test_gpu_body_mass.py: the sets of the per-sub-environment body mass scale
(set_attr("body_mass_scale")), the oracle side of them and the tolerance of the derived constants.  The oracle takes its model as data
(model_attrs_cases.py): compiler.scaled(stock, scale) registered in place of the stock model IS the robot with heavier links, derived constants
included.  PARITY UNPINNED against `mujoco`, like all MuJoCo physics of this project: the oracle is the reference for this field."""
import contextlib

import numpy as np

from gymnasium_amd.envs.mujoco import compiler

from model_attrs_cases import ROBOTS, _register, patched, stock

MINVAL = compiler.MINVAL
DERIVED = ("dof_invweight0", "body_invweight0", "meaninertia")
# Worst relative difference between the simulator's derivation routine built for the host (mjx_core.h derive_mass_constants, g++ -O1, no contraction) and
# compiler.scaled over the three sets below, per robot, as recorded in docs/results_log.md.  The routine factorises the mass matrix the step kernels build
# (composite rigid body, packed Cholesky); the compiler sums m Jp'Jp + Jr' I Jr and calls LAPACK's inverse: two formulations in float64 whose difference
# scales with the condition number of M (8 .. 3e3 for the stock robots).  The assertion is at TEN times the recorded figure -- the margin
# for the device contracting other products into FMAs than the host build -- and never looser than 1e-9, beyond which the 1e-8 trajectory test
# could not hold.
RECORDED_WORST = {"half_cheetah": 1.060e-15, "ant": 4.472e-16, "humanoid": 3.291e-14, "hopper": 3.986e-15, "walker2d": 3.037e-14, "inverted_pendulum": 4.944e-16,
                  "inverted_double_pendulum": 1.123e-15, "reacher": 5.563e-16, "humanoid_standup": 2.714e-14, "swimmer": 1.253e-14, "pusher": 2.328e-15}


def tolerance(name):
    tol = 10.0 * RECORDED_WORST[name]
    assert tol <= 1e-9, f"{name}: a derived-constant tolerance looser than 1e-9 means a bug, not noise"
    return tol


# The body of set 2 that sits on the floor value: the last one (a leaf of every robot), except where a leaf a thousand times lighter than its neighbours
# makes the explicit RK4 integration diverge in the ORACLE itself within the 40 steps of the trajectory tests (InvertedPendulum's pole: the joint damping
# over the pole's inertia times the step leaves RK4's stability region; Swimmer's end links: the same with the quadratic fluid drag) -- a reference of
# NaNs compares with nothing.  There the floor value goes to a body the oracle stays finite with: the cart, the middle link.
FLOOR_BODY = {"inverted_pendulum": 1, "swimmer": 2}


def scale_sets(name):
    """Three body mass scales [nbody]; lane i of a GPU env uses set i % 3.  Set 0 is the stock model; set 1 alternates 0.6 / 1.5 from body to body;
    set 2 is a uniform 2.0 with the floor value 1e-3 on one body (FLOOR_BODY, by default the last)."""
    nb = stock(name).nbody
    s2 = np.full(nb, 2.0)
    s2[FLOOR_BODY.get(name, nb - 1)] = 1e-3
    return [np.ones(nb), np.where(np.arange(nb) % 2 == 0, 0.6, 1.5), s2]


def lane_scales(name, n):
    sets = scale_sets(name)
    return [sets[i % 3] for i in range(n)]


def relative_difference(got, want):
    """Worst |got - want| / |want| over the entries of `want` that are not on the MINVAL floor (or zero: the world body); those must be equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    floor = (want == MINVAL) | (want == 0.0)
    assert np.array_equal(got[floor], want[floor]), "entries on the MINVAL floor (and the world body's zeros) must be equal"
    if floor.all():
        return 0.0
    return float((np.abs(got[~floor] - want[~floor]) / np.abs(want[~floor])).max())


_SCALED = {}


def compare_derived(name, got, scale):
    """got = {"dof_invweight0": [nv], "body_invweight0": [nbody, 2], "meaninertia": ()} against compiler.scaled(stock, scale); returns the worst
    relative difference after asserting it within tolerance(name)."""
    key = (name, np.asarray(scale, dtype=np.float64).tobytes())
    if key not in _SCALED:  # (computed once per set, shared by the tests, left unchanged)
        _SCALED[key] = compiler.scaled(stock(name), scale)
    want = _SCALED[key]
    worst = max(relative_difference(got[k], getattr(want, k)) for k in DERIVED)
    assert worst <= tolerance(name), f"{name}: derived constants differ from compiler.scaled by {worst:.3e} relative (tolerance {tolerance(name):.1e})"
    return worst


@contextlib.contextmanager
def oracle_model(name, scale, values=None):
    """The oracle runs `name` with every body's mass and inertia scaled (and, with `values`, the other four fields patched) inside the block; the stock
    model is registered again on the way out, whatever happened."""
    try:
        _register(name, compiler.scaled(patched(name, values or {}), scale))
        yield
    finally:
        _register(name, stock(name))


def record_oracle(name, scale, values, n, T, window, seed, actions, factory, **kw):
    """model_attrs_cases.record_oracle on the scaled model: what reset and T steps return, the state at the end of every window, the generator states."""
    import gymnasium_amd

    with oracle_model(name, scale, values):
        env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=n, _engine_factory=factory, **kw)
        rec = {"reset_obs": env.reset(seed=seed)[0].copy(), "reset_rng": env.get_rng_state().copy(), "obs": [], "rew": [], "te": [], "tr": [], "states": {}}
        for t in range(T):
            o, r, te, tr, _ = env.step(actions[t])
            rec["obs"].append(o.copy()), rec["rew"].append(r.copy()), rec["te"].append(te.copy()), rec["tr"].append(tr.copy())
            if (t + 1) % window == 0:
                rec["states"][t] = tuple(np.array(x) for x in env.get_state())
        rec["rng"] = env.get_rng_state().copy()
        env.close()
    return rec


def densities_scaled(name, scale):
    """models.MODELS[name]() with every geom density of body b multiplied by scale[b] (bodies in the compiler's depth-first order): the independent
    way to compile the robot with heavier links."""
    from gymnasium_amd.envs.mujoco import models

    d = models.MODELS[name]()
    gdef = dict(compiler.GEOM_DEFAULTS, **d.get("geom_default", {}))
    index = [0]

    def visit(b):
        index[0] += 1
        s = float(scale[index[0]])
        for g in b["geoms"]:
            g["density"] = float(g.get("density", gdef["density"])) * s
        for c in b["children"]:
            visit(c)

    for b in d["bodies"]:
        visit(b)
    assert index[0] == len(scale) - 1
    return d
