"""Shared by tests/test_model_attrs_host.py and tests/test_gpu_model_attrs.py: the parameter sets of the per-sub-environment model fields and the
oracle side of them.  The oracle takes its models as data (oracle/oracle.py _register_mujoco_models): a patched CompiledModel registered in place of
the stock one makes the whole oracle vector engine -- physics, glue, resets, PGS warm start -- run that model.  oracle/mujoco_envs.c keeps ONE
model per robot (g_models[which], overwritten in place by a registration) and its envs point at it without copying (only a solver="Newton" env copies,
at creation), so no two oracle envs with different models are alive at the same time here and the stock model is always put back.
PARITY UNPINNED against `mujoco`, like all MuJoCo physics of this project: the oracle is the reference for these fields."""
import contextlib
import copy
import ctypes

import numpy as np

from gymnasium_amd.envs.mujoco import compiler, models

ROBOTS = {"half_cheetah": "HalfCheetah-v5", "ant": "Ant-v5", "humanoid": "Humanoid-v5", "hopper": "Hopper-v5", "walker2d": "Walker2d-v5",
          "inverted_pendulum": "InvertedPendulum-v5", "inverted_double_pendulum": "InvertedDoublePendulum-v5", "reacher": "Reacher-v5",
          "humanoid_standup": "HumanoidStandup-v5", "swimmer": "Swimmer-v5", "pusher": "Pusher-v5"}
ORDER = list(ROBOTS)  # the oracle's model numbers (oracle/oracle.py)
FIELDS = ("gravity", "actuator_gear", "dof_damping", "geom_friction")
_STOCK = {}


def stock(name):
    if name not in _STOCK:
        _STOCK[name] = compiler.compile_model(name)
    return _STOCK[name]


def mix_pairs(m, geom_friction):
    """The compiler's rule for the sliding friction of a contact pair (compiler.py: element-wise maximum of the two geoms)."""
    g = np.asarray(geom_friction, dtype=np.float64)
    return np.maximum(g[..., m.pair_geom1], g[..., m.pair_geom2])


def param_sets(name):
    """Three sets of the four fields; lane i of a GPU env uses set i % 3.  Set 0 is the stock model; one set has a small x component of gravity;
    set 1 has ALL-ZERO damping where the stock damping is not (every robot but the undamped Swimmer, whose sets 1 and 2 are damped instead): the
    implicit-damping branch of the Euler integrator then differs between lanes of one wavefront."""
    m = stock(name)
    gz = (-9.81, -6.0, -12.0)
    out = []
    for s in range(3):
        damping = m.dof_damping * (1.0, 0.5, 2.0)[s]
        if s == 1 and m.dof_damping.max() > 0:
            damping = np.zeros_like(m.dof_damping)
        if m.dof_damping.max() == 0:  # an undamped robot (Swimmer): factors of zero would test nothing -- absolute values; the stock lanes stay undamped
            damping = np.full_like(m.dof_damping, (0.0, 0.1, 0.4)[s])
        gravity = m.gravity.copy()  # (set 0 IS the stock model: InvertedDoublePendulum's MJCF has gravity x = 1e-5)
        if s:
            gravity[2] = gz[s]
        if s == 2:
            gravity[0] = 0.3
        out.append({"gravity": gravity, "actuator_gear": m.actuator_gear * (1.0, 0.6, 1.4)[s],
                    "dof_damping": damping, "geom_friction": m.geom_friction[:, 0] * (1.0, 0.5, 1.5)[s]})
    return out


def patched(name, values):
    """The stock CompiledModel with the given fields replaced (what is licensed by test_no_compiled_quantity_is_derived_from_the_fields)."""
    m = copy.deepcopy(stock(name))
    if "gravity" in values:
        m.gravity = np.array(values["gravity"], dtype=np.float64)
    if "actuator_gear" in values:
        m.actuator_gear = np.array(values["actuator_gear"], dtype=np.float64)
    if "dof_damping" in values:
        m.dof_damping = np.array(values["dof_damping"], dtype=np.float64)
    if "geom_friction" in values and len(m.pair_geom1):
        m.pair_friction = m.pair_friction.copy()
        m.pair_friction[:, 0] = mix_pairs(m, values["geom_friction"])
    return m


def _register(name, model):
    from oracle import mujoco as omj
    from oracle import oracle

    lib = oracle.load()
    fn = lib.dll.orc_mj_register_model
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    blob = omj.model_blob(model)
    rc = fn(ORDER.index(name), blob.ctypes.data, len(blob))
    assert rc == 0, f"oracle rejected the {name} model blob (rc={rc})"


@contextlib.contextmanager
def oracle_model(name, values):
    """The oracle runs `name` with the patched fields inside the block; the stock model is registered again on the way out, whatever happened."""
    try:
        _register(name, patched(name, values))
        yield
    finally:
        _register(name, stock(name))


def altered_description(name):
    """models.MODELS[name]() with gravity, every actuator's gear, every joint's damping and every geom's sliding friction changed."""
    d = models.MODELS[name]()
    d["option"] = dict(d["option"], gravity=(0.25, -0.5, -7.0))
    d["actuators"] = [(a[0], a[1] * 1.7 + 3.0) + tuple(a[2:]) for a in d["actuators"]]
    jdef = dict(compiler.JOINT_DEFAULTS, **d.get("joint_default", {}))
    gdef = dict(compiler.GEOM_DEFAULTS, **d.get("geom_default", {}))
    count = [0]

    def fr(f):
        count[0] += 1
        return (f[0] * 0.5 + 0.01 * count[0],) + tuple(f[1:])

    def visit(b):
        for j in b["joints"]:
            j["damping"] = float(j.get("damping", jdef["damping"])) * 1.3 + 0.07
        for g in b["geoms"]:
            g["friction"] = fr(tuple(g.get("friction", gdef["friction"])))
        for c in b["children"]:
            visit(c)

    for b in d["bodies"]:
        visit(b)
    if d["floor"] is not None:
        d["floor"] = dict(d["floor"], friction=fr(tuple(d["floor"].get("friction", gdef["friction"]))))
    return d


def lane_values(name, fields, n):
    """{field: [value of lane 0, ...]} with lane i on set i % 3, for the given fields; the other fields stay stock."""
    sets = param_sets(name)
    return {f: [sets[i % 3][f] for i in range(n)] for f in fields}


def record_oracle(name, values, n, T, window, seed, actions, factory, **kw):
    """One uniform oracle env on the model patched with `values`: what reset and T steps return, the state at the end of every window, the
    generator states and the counts.  The env is closed and the stock model registered again before this returns."""
    import gymnasium_amd

    with oracle_model(name, values):
        env = gymnasium_amd.make_vec(ROBOTS[name], num_envs=n, _engine_factory=factory, **kw)
        rec = {"reset_obs": env.reset(seed=seed)[0].copy(), "reset_rng": env.get_rng_state().copy(), "obs": [], "rew": [], "te": [], "tr": [], "states": {}}
        for t in range(T):
            o, r, te, tr, _ = env.step(actions[t])
            rec["obs"].append(o.copy()), rec["rew"].append(r.copy()), rec["te"].append(te.copy()), rec["tr"].append(tr.copy())
            if (t + 1) % window == 0:
                rec["states"][t] = tuple(np.array(x) for x in env.get_state())
        rec["rng"], rec["stats"] = env.get_rng_state().copy(), dict(env.statistics())
        env.close()
    return rec


def next_step_counts(te, tr):
    """env_steps, reset_steps, episodes, length_sum of the NEXT_STEP state machine from the flags [T][lanes] of a recorded trajectory (a lane that
    finished resets in its next step, which counts as a reset step and starts a new episode)."""
    T, n = len(te), len(te[0])
    out = {"env_steps": 0, "reset_steps": 0, "episodes": 0, "length_sum": 0}
    for i in range(n):
        pending, length = False, 0
        for t in range(T):
            if pending:
                out["reset_steps"] += 1
                pending, length = False, 0
                continue
            out["env_steps"] += 1
            length += 1
            if te[t][i] or tr[t][i]:
                out["episodes"] += 1
                out["length_sum"] += length
                pending = True
    return out
