#!/usr/bin/env python3
"""Fixtures of per-sub-environment physics (SyncVectorEnv.set_attr), recorded FROM THE REFERENCE ITSELF.

Run in the build container only (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_env_attrs.py

It imports gymnasium from the reference tree (GYM_REFERENCE, default /root/reference; NumPy >= 2: NEP 50 promotion) and writes, per id,
env_attrs_<key>.npz with

  run_*       gym.make_vec(id, 64, "sync"), reset(seed=[...]), attributes set per sub-environment right after the reset and a second set
              half-way, random policy from action_space.seed(ASEED): actions, observations, rewards, flags, and the attributes (attr0 / attr1:
              [A][64] float64 as the engine stores them, *_int: which values were Python ints)
  teacher_*   single steps of the scalar env from (state, attributes, action) rows, for Pendulum and MountainCarContinuous with float32 rows,
              float64 rows and Python-float rows (teacher_*0 / 1 / 2)
  same_*      CartPole and MountainCarContinuous: the same kind of run under AutoresetMode.SAME_STEP, with final_obs

The attribute values reach every branch an attribute moves: both CartPole integrators, terminations by x and by theta, thresholds beyond the
short sin / cos range (|theta| < 0.855), stale polemass_length / total_mass, Python ints, an active torque clip, hits on the left wall, both
object kinds out of MountainCarContinuous' min / max.  The script also checks, on the teacher rows, that the attributes the engine accepts as
np.float64 (gymnasium_amd/envs/classic_control.py ENV_ATTRS) are type-blind: np.float64 values step exactly like Python floats.
Everything is a function of the fixed seeds below: a second run rewrites every file byte for byte.
"""
import os
import sys

REF = os.environ.get("GYM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import gymnasium as gym  # noqa: E402
from gymnasium.vector import AutoresetMode  # noqa: E402

assert int(np.__version__.split(".")[0]) >= 2, "the fixtures must be generated with NumPy >= 2"
OUT = os.path.dirname(os.path.abspath(__file__))
N, T, T_SWITCH, M = 64, 200, 100, 1024
SEEDS = [1000 + 7 * i for i in range(N)]
ASEED = 31

# (name, accepted as np.float64) in the engine's id order (include/mi355env.h MI_ATTR_*)
ATTRS = {
    "cartpole": ("CartPole-v1", [("gravity", True), ("masscart", True), ("masspole", True), ("total_mass", True), ("length", True),
                                 ("polemass_length", True), ("force_mag", True), ("tau", True), ("kinematics_integrator", True),
                                 ("theta_threshold_radians", True), ("x_threshold", True)]),
    "pendulum": ("Pendulum-v1", [("g", True), ("m", False), ("l", False), ("dt", True), ("max_speed", True), ("max_torque", False)]),
    "mountaincar": ("MountainCar-v0", [("force", True), ("gravity", True), ("max_speed", True), ("min_position", True), ("max_position", True),
                                       ("goal_position", True), ("goal_velocity", True)]),
    "mountaincar_continuous": ("MountainCarContinuous-v0", [("min_action", False), ("max_action", False), ("power", False), ("max_speed", False),
                                                            ("min_position", False), ("max_position", False), ("goal_position", False),
                                                            ("goal_velocity", False)]),
}


def r4(x):
    return float(np.round(x, 4))


def draw(key, rng, n):
    """n sets of attribute values as the Python objects a user would pass: {name: [value] * n}."""
    u = lambda lo, hi: [r4(v) for v in rng.uniform(lo, hi, n)]  # noqa: E731
    ints = rng.random(n) < 0.15
    if key == "cartpole":
        mc, mp, ln = u(0.5, 2.0), u(0.05, 0.5), u(0.3, 0.8)
        stale = rng.random(n) < 0.5  # total_mass / polemass_length left at what __init__ computed
        wide = rng.random(n) < 0.3
        return {"gravity": [10 if ints[i] else v for i, v in enumerate(u(5.0, 15.0))], "masscart": mc, "masspole": mp,
                "total_mass": [1.1 if stale[i] else mp[i] + mc[i] for i in range(n)], "length": ln,
                "polemass_length": [0.05 if stale[i] else mp[i] * ln[i] for i in range(n)],
                "force_mag": [10 if ints[i] else v for i, v in enumerate(u(5.0, 15.0))], "tau": u(0.01, 0.03),
                "kinematics_integrator": ["euler" if k else "semi-implicit" for k in rng.random(n) < 0.5],
                "theta_threshold_radians": [float(rng.choice([1.0, 2.0, 4.0])) if wide[i] else v for i, v in enumerate(u(0.12, 0.3))],
                "x_threshold": [2 if ints[i] else v for i, v in enumerate(u(0.8, 3.0))]}
    if key == "pendulum":
        return {"g": [10 if ints[i] else v for i, v in enumerate(u(5.0, 15.0))], "m": [1 if ints[i] else v for i, v in enumerate(u(0.5, 2.0))],
                "l": u(0.5, 1.5), "dt": u(0.03, 0.07), "max_speed": [8 if ints[i] else v for i, v in enumerate(u(3.0, 12.0))],
                "max_torque": u(0.5, 3.0)}
    if key == "mountaincar":
        return {"force": u(0.0005, 0.003), "gravity": u(0.001, 0.0035), "max_speed": u(0.03, 0.1),
                "min_position": [r4(v) for v in rng.choice([-1.2, -0.75, -0.7, -0.65], n) + rng.uniform(0, 0.01, n)],
                "max_position": u(0.4, 0.8), "goal_position": u(-0.3, 0.55),
                "goal_velocity": [0 if ints[i] or k else v for i, (v, k) in enumerate(zip(u(0.0, 0.02), rng.random(n) < 0.5))]}
    return {"min_action": u(-1.3, -0.3), "max_action": u(0.3, 1.3), "power": u(0.001, 0.005), "max_speed": u(0.03, 0.1),
            "min_position": [r4(v) for v in rng.choice([-1.2, -0.75, -0.7, -0.65], n) + rng.uniform(0, 0.01, n)],
            "max_position": u(0.3, 0.7), "goal_position": u(-0.3, 0.5),
            "goal_velocity": [0 if ints[i] or k else v for i, (v, k) in enumerate(zip(u(0.0, 0.02), rng.random(n) < 0.5))]}


def as_rows(key, vals):
    """[A][n] float64 as the engine stores them, and [A][n] bool: the value was a Python int."""
    names = [a for a, _ in ATTRS[key][1]]
    rows = np.array([[(0.0 if v == "euler" else 1.0) if isinstance(v, str) else float(v) for v in vals[a]] for a in names], dtype=np.float64)
    ints = np.array([[type(v) is int for v in vals[a]] for a in names], dtype=bool)
    return rows, ints


def run(key, mode, T_run, seed_rng):
    env_id = ATTRS[key][0]
    vec = gym.make_vec(env_id, num_envs=N, vectorization_mode="sync", vector_kwargs={"autoreset_mode": mode})
    obs0, _ = vec.reset(seed=SEEDS)
    v0, v1 = draw(key, seed_rng, N), draw(key, seed_rng, N)
    for name, vals in v0.items():
        vec.set_attr(name, vals)
        assert list(vec.get_attr(name)) == vals
    vec.action_space.seed(ASEED)
    A, O, R, TE, TR, FO, FM = [], [], [], [], [], [], []
    for t in range(T_run):
        if t == T_SWITCH:
            for name, vals in v1.items():
                vec.set_attr(name, vals)
        a = vec.action_space.sample()
        o, r, te, tr, info = vec.step(a)
        fo, fm = np.zeros_like(o), np.zeros(N, dtype=bool)
        if "final_obs" in info:
            fm = info["_final_obs"].copy()
            for i in np.where(fm)[0]:
                fo[i] = info["final_obs"][i]
        A.append(a), O.append(o), R.append(r), TE.append(te), TR.append(tr), FO.append(fo), FM.append(fm)
    vec.close()
    a0, i0 = as_rows(key, v0)
    a1, i1 = as_rows(key, v1)
    out = dict(seeds=np.array(SEEDS, dtype=np.int64), aseed=np.int64(ASEED), switch=np.int64(T_SWITCH), obs0=obs0, actions=np.stack(A),
               obs=np.stack(O), reward=np.stack(R), term=np.stack(TE), trunc=np.stack(TR), attr0=a0, attr1=a1, attr0_int=i0, attr1_int=i1)
    if mode == AutoresetMode.SAME_STEP:
        out.update(final_obs=np.stack(FO), final_mask=np.stack(FM))
    return out


def teacher(key, rng):
    env_id, spec = ATTRS[key]
    names = [a for a, _ in spec]
    vals = draw(key, rng, M)
    if key == "cartpole":
        s = np.stack([rng.uniform(-3, 3, M), rng.uniform(-3, 3, M), rng.uniform(-4.5, 4.5, M), rng.uniform(-4, 4, M)], 1)
        s[: M // 8, 2] = rng.uniform(-0.3, 0.3, M // 8)
        acts = [rng.integers(0, 2, M)]
    elif key == "pendulum":
        s = np.stack([rng.uniform(-20, 20, M), rng.uniform(-10, 10, M)], 1)
        a = rng.uniform(-3.5, 3.5, M)
        acts = [a.astype(np.float32), a, a]
    elif key == "mountaincar":
        s = np.stack([rng.uniform(-1.25, 0.65, M), rng.uniform(-0.1, 0.1, M)], 1)
        acts = [rng.integers(0, 3, M)]
    else:
        s = np.stack([rng.uniform(-1.25, 0.65, M), rng.uniform(-0.1, 0.1, M)], 1)
        a = rng.uniform(-1.4, 1.4, M)
        a[: M // 8] = rng.choice([-1.0, 1.0, -0.5, 0.5], M // 8)
        acts = [a.astype(np.float32), a, a]
    f32 = rng.random(M) < 0.6 if key == "mountaincar_continuous" else np.zeros(M, dtype=bool)
    s[f32] = s[f32].astype(np.float32).astype(np.float64)

    def step_all(vals, kind, a):
        env = gym.make(env_id).unwrapped
        env.reset(seed=0)
        ns, ob, rw, te = [], [], [], []
        for k in range(M):
            for name in names:
                setattr(env, name, vals[name][k])
            if key == "mountaincar":
                env.state = (np.float64(s[k, 0]), np.float64(s[k, 1]))
            else:
                env.state = np.array(s[k], dtype=np.float32 if f32[k] else np.float64)
            if hasattr(env, "steps_beyond_terminated"):
                env.steps_beyond_terminated = None
            if key in ("cartpole", "mountaincar"):
                act = a[k]
            else:
                act = [np.float32(a[k]), np.float64(a[k]), float(a[k])][kind]
                act = np.array([act]) if kind < 2 else [act]
            o, r, t, _, _ = env.step(act)
            ns.append(np.asarray(env.state, dtype=np.float64).ravel()), ob.append(o), rw.append(r), te.append(t)
        return np.stack(ns), np.stack(ob), np.array(rw, dtype=np.float64), np.array(te, dtype=bool)

    out = {"teacher_state": s, "teacher_f32": f32}
    out["teacher_attr"], out["teacher_attr_int"] = as_rows(key, vals)
    strong = {name: [np.float64(v) if (ok and not isinstance(v, str)) else v for v in vals[name]] for name, ok in spec}
    for kind, a in enumerate(acts):
        ns, ob, rw, te = step_all(vals, kind, a)
        # the attributes accepted as np.float64 are type-blind: the same steps with np.float64 values
        for x, y in zip((ns, ob, rw, te), step_all(strong, kind, a)):
            assert np.array_equal(x, y), f"{key}: an np.float64 attribute changed the reference's result (action kind {kind})"
        out[f"teacher_action{kind}"] = a
        out[f"teacher_next_state{kind}"], out[f"teacher_obs{kind}"], out[f"teacher_reward{kind}"], out[f"teacher_term{kind}"] = ns, ob, rw, te
    out["teacher_kinds"] = np.int64(len(acts))
    return out


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrs)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    for n, key in enumerate(ATTRS):
        arrs = {}
        for k, v in run(key, AutoresetMode.NEXT_STEP, T, np.random.default_rng(100 + n)).items():
            arrs["run_" + k] = v
        arrs.update(teacher(key, np.random.default_rng(200 + n)))
        if key in ("cartpole", "mountaincar_continuous"):
            for k, v in run(key, AutoresetMode.SAME_STEP, 100, np.random.default_rng(300 + n)).items():
                arrs["same_" + k] = v
        save(f"env_attrs_{key}.npz", **arrs)


if __name__ == "__main__":
    main()
