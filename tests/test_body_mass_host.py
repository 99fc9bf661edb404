"""Per-sub-environment body mass scale of the MuJoCo classes, host side (no GPU): compiler.scaled against an independent compile of the robot with
denser links, its closed form, the simulator's derivation routine built for the host against compiler.scaled, and the names, shapes and refusals of
set_attr / get_attr("body_mass_scale" | "dof_invweight0" | "body_invweight0" | "meaninertia") on the oracle backend.
PARITY UNPINNED against `mujoco`, like all MuJoCo physics of this project: the oracle -- which takes compiler.scaled's model as data -- is the reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd.envs.mujoco import compiler, models
from gymnasium_amd.gym_api import error
from gymnasium_amd.vector.hip_vector_env import UnknownEnvAttributeError

from body_mass_cases import DERIVED, MINVAL, compare_derived, densities_scaled, scale_sets
from model_attrs_cases import FIELDS, ORDER, ROBOTS, stock

HERE = os.path.dirname(os.path.abspath(__file__))
N = 5
NO_TOTALMASS = [n for n in ROBOTS if n != "half_cheetah"]  # (settotalmass rescales the masses after the densities: the density path cannot see a per-body factor)


def _fields_differing(a, b):
    assert set(vars(a)) == set(vars(b))
    out = []
    for key in vars(a):
        x, y = getattr(a, key), getattr(b, key)
        if isinstance(x, np.ndarray):
            same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        else:
            same = x == y
        if not same:
            out.append(key)
    return out


@pytest.mark.parametrize("name", NO_TOTALMASS)
def test_scaled_is_the_compile_of_the_denser_robot(name):
    """Per-body factors from {0.5, 1, 2, 4} (powers of two: s rho V is exact): compiler.scaled(stock, s) is, byte for byte in EVERY field of the
    CompiledModel, the compile of the description whose geoms of body b are s_b times as dense -- body_ipos, body_fluidbox and body_imat included,
    which is the claim that a density change moves neither the centre of mass, nor the principal axes, nor the fluid box."""
    m = stock(name)
    assert not models.MODELS[name]().get("settotalmass")
    rng = np.random.default_rng(ORDER.index(name))
    s = rng.choice([0.5, 1.0, 2.0, 4.0], size=m.nbody)
    s[1] = 4.0 if s[1] == 1.0 else s[1]  # (never the identity)
    a, b = compiler.scaled(m, s), compiler.compile_model(densities_scaled(name, s))
    assert _fields_differing(a, b) == [], f"{name}: scaled() and the density compile differ in {_fields_differing(a, b)}"
    assert np.array_equal(a.body_mass, m.body_mass * s) and not np.array_equal(a.body_mass, m.body_mass)
    assert np.array_equal(a.body_fluidbox, m.body_fluidbox) and np.array_equal(a.body_imat, m.body_imat) and np.array_equal(a.body_ipos, m.body_ipos)
    assert compiler.scaled(m, np.ones(m.nbody)).__dict__.keys() == m.__dict__.keys() and _fields_differing(compiler.scaled(m, np.ones(m.nbody)), m) == []


def test_scaled_refuses_a_wrong_width():
    with pytest.raises(ValueError, match="one factor per body"):
        compiler.scaled(stock("hopper"), np.ones(stock("hopper").nbody - 1))


@pytest.mark.parametrize("name", ["inverted_pendulum", "inverted_double_pendulum"])
def test_closed_form_of_a_uniform_scale(name):
    """Without armature M is linear in the masses: a uniform 2.0 halves M^-1 and doubles mean(diag M), exactly (a power of two)."""
    m = stock(name)
    assert not m.dof_armature.any()
    d = compiler.scaled(m, np.full(m.nbody, 2.0))
    assert np.array_equal(d.dof_invweight0, m.dof_invweight0 / 2)
    floor = m.body_invweight0 == MINVAL
    assert floor.any() and np.array_equal(d.body_invweight0[floor], m.body_invweight0[floor])
    assert np.array_equal(d.body_invweight0[~floor], m.body_invweight0[~floor] / 2)
    assert d.meaninertia == 2 * m.meaninertia and d.total_mass == 2 * m.total_mass


_LIB = []


def _derive_lib():
    """mjx_core.h's derive_mass_constants compiled for the host (tests/body_mass_emu/derive.cpp), as tests/test_coop_emu.py builds the simulator."""
    if not _LIB:
        emu = os.path.join(HERE, "body_mass_emu")
        so, src = os.path.join(emu, "libbody_mass_emu.so"), os.path.join(emu, "derive.cpp")
        csrc = os.path.join(HERE, "..", "gymnasium_amd", "csrc")
        deps = [src, __file__, os.path.join(csrc, "mjx_core.h"), os.path.join(csrc, "generated", "mjx_models.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            from gymnasium_amd.envs.mujoco import codegen

            codegen.generate()
            subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden", "-Wno-unknown-pragmas", "-o", so, src],
                           check=True, cwd=emu)
        lib = C.CDLL(so)
        lib.body_mass_derive.restype, lib.body_mass_derive.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_void_p]
        _LIB.append(lib)
    return _LIB[0]


def host_derived(name, scale):
    m = stock(name)
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    out = np.zeros(m.nv + 2 * m.nbody + 1)
    assert _derive_lib().body_mass_derive(ORDER.index(name), scale.ctypes.data, out.ctypes.data) == out.size
    return {"dof_invweight0": out[:m.nv], "body_invweight0": out[m.nv:m.nv + 2 * m.nbody].reshape(m.nbody, 2), "meaninertia": out[-1]}


@pytest.mark.parametrize("name", list(ROBOTS))
def test_host_build_of_the_derivation_equals_compiler_scaled(name):
    """The routine mj_model_constants_kernel runs, over the three sets: within ten times the recorded worst relative difference (body_mass_cases.py
    RECORDED_WORST, docs/results_log.md), entries on the MINVAL floor equal."""
    worst = 0.0
    for k, scale in enumerate(scale_sets(name)):
        w = compare_derived(name, host_derived(name, scale), scale)
        print(f"{name} set {k}: worst relative difference of the host-built derivation from compiler.scaled {w:.3e}")
        worst = max(worst, w)
    print(f"{name}: worst over the sets {worst:.3e}")
    sets = scale_sets(name)
    assert not np.array_equal(host_derived(name, sets[1])["dof_invweight0"], host_derived(name, sets[0])["dof_invweight0"])


@pytest.fixture()
def ant(oracle_factory):
    env = gymnasium_amd.make_vec("Ant-v5", num_envs=N, _engine_factory=oracle_factory)
    yield env
    env.close()


@pytest.mark.parametrize("name", list(ROBOTS))
def test_get_attr_defaults_of_all_fields(name, oracle_factory):
    env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=3, _engine_factory=oracle_factory)
    m = stock(name)
    want = {"gravity": m.gravity, "actuator_gear": m.actuator_gear, "dof_damping": m.dof_damping, "geom_friction": m.geom_friction[:, 0],
            "body_mass_scale": np.ones(m.nbody)}
    assert [f[0] for f in env.MODEL_FIELDS] == list(FIELDS) + ["body_mass_scale"]
    for field, value in want.items():
        got = env.get_attr(field)
        assert isinstance(got, tuple) and len(got) == 3
        for row in got:
            assert isinstance(row, np.ndarray) and row.dtype == np.float64 and row.shape == value.shape and np.array_equal(row, value)
    for field in DERIVED:  # before any set: the compiled model's values
        got = env.get_attr(field)
        assert isinstance(got, tuple) and len(got) == 3
        for row in got:
            assert row.dtype == np.float64 and np.array_equal(row, np.asarray(getattr(m, field)))
    assert env.get_attr("body_invweight0")[0].shape == (m.nbody, 2) and env.get_attr("dof_invweight0")[0].shape == (m.nv,) and env.get_attr("meaninertia")[0].shape == ()
    env.close()


def test_refusals_by_name(ant):
    field, m = "body_mass_scale", stock("ant")
    w = m.nbody
    ok = np.asarray(ant.get_attr(field)[0])
    for bad in (np.nan, np.inf, -np.inf):
        v = ok.copy()
        v[-1] = bad
        with pytest.raises(ValueError, match=f"{field}.*finite"):
            ant.set_attr(field, v)
        with pytest.raises(ValueError, match=f"{field}.*finite"):
            ant.set_attr(field, [ok] * (N - 1) + [v])
    for low in (0.99e-3, 0.0, -1.0):
        v = ok.copy()
        v[3] = low
        with pytest.raises(ValueError, match=f"{field}.*>= 0.001"):
            ant.set_attr(field, v)
        with pytest.raises(ValueError, match=f"{field}.*>= 0.001"):
            ant.set_attr(field, [v] + [ok] * (N - 1))
    with pytest.raises(ValueError, match=f"{field}.*shape \\({w},\\)"):
        ant.set_attr(field, np.ones(w + 1))
    with pytest.raises(ValueError, match=f"{field}.*shape \\({w},\\)"):
        ant.set_attr(field, np.ones(w - 1))  # (nbody - 1: the world body's column is part of the width)
    with pytest.raises(ValueError, match=f"{field}.*shape \\({w},\\)"):
        ant.set_attr(field, 2.0)  # a scalar is not broadcast over the bodies
    with pytest.raises(ValueError, match=f"`{N - 1}` values for {N} environments"):
        ant.set_attr(field, [ok] * (N - 1))
    with pytest.raises(TypeError, match=field):
        ant.set_attr(field, "heavy")
    with pytest.raises(TypeError, match=field):
        ant.set_attr(field, ["heavy"] * N)
    # valid values (the floor itself, and anything in the world body's column that is >= the floor) pass every check and then meet the backend
    v = np.full(w, 1e-3)
    for values in (v, [v] * N, np.full(w, 3.0)):
        with pytest.raises(error.Error, match="the engine behind this env has no per-sub-environment model fields"):
            ant.set_attr(field, values)
    assert all(np.array_equal(r, np.ones(w)) for r in ant.get_attr(field))  # nothing was stored
    # the derived constants are read-only, and the name the existing tests pin as unknown stays unknown
    for name in DERIVED:
        with pytest.raises(AttributeError, match="read-only"):
            ant.set_attr(name, ant.get_attr(name))
        with pytest.raises(AttributeError, match="read-only"):
            ant.set_attr(name, None)
    with pytest.raises(UnknownEnvAttributeError, match="gravity, actuator_gear, dof_damping, geom_friction, body_mass_scale"):
        ant.get_attr("body_mass")
    with pytest.raises(UnknownEnvAttributeError):
        ant.set_attr("body_inertia", np.ones(w))


def test_tensor_refusals(ant):
    torch = pytest.importorskip("torch")
    w = stock("ant").nbody
    with pytest.raises(ValueError, match=f"body_mass_scale.*shape \\({N}, {w}\\)"):
        ant.set_attr("body_mass_scale", torch.ones((N, w - 1), dtype=torch.float64))
    with pytest.raises(ValueError, match=f"body_mass_scale.*shape \\({N}, {w}\\)"):
        ant.set_attr("body_mass_scale", torch.ones((w,), dtype=torch.float64))
    with pytest.raises(TypeError, match="body_mass_scale.*float64"):
        ant.set_attr("body_mass_scale", torch.ones((N, w), dtype=torch.float32))
    with pytest.raises(ValueError, match="body_mass_scale.*device"):  # a host tensor is on the wrong device: host values travel as lists / arrays
        ant.set_attr("body_mass_scale", torch.ones((N, w), dtype=torch.float64))
    with pytest.raises(AttributeError, match="read-only"):
        ant.set_attr("meaninertia", torch.ones((N, 1), dtype=torch.float64))
