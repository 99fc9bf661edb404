#!/usr/bin/env python3
"""Fixture of Acrobot's per-sub-environment physics (SyncVectorEnv.set_attr), recorded FROM THE REFERENCE ITSELF.

Run where the reference gymnasium imports (GYM_REFERENCE names its tree; NumPy >= 2), never on the GPU box:

    GYM_REFERENCE=/path/to/gymnasium-tree PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_acrobot_attrs.py

It writes env_attrs_acrobot.npz with

  run_*      gym.make_vec("Acrobot-v1", 96, "sync", max_episode_steps=25), reset(seed=[...]), every attribute set per sub-environment right
             after the reset and a second set half-way, 96 steps of a random policy from action_space.seed(ASEED): actions, observations,
             rewards, flags, the attributes (attr0 / attr1: [A][96] float64 as the engine stores them, *_int: which were Python ints) and
             run_rng: every sub-environment's PCG64 words {state_hi, state_lo, inc_hi, inc_lo} after the last step -- the NUMBER of draws a
             noisy sub-environment took is pinned, not only their values
  same_*     the same configuration under AutoresetMode.SAME_STEP, with final_obs
  teacher_*  single steps of the scalar env from (state, attributes, action) rows without noise; the second half of the rows is the first
             half with book_or_nips swapped

The batch mixes torque_noise_max = 0 and > 0, "book" and "nips", Python ints and floats, and sub-environments 0..3 keep every default.  The
script asserts on its own output that the fixture is not vacuous (counts below).  Everything is a function of the fixed seeds: a second run
rewrites the file byte for byte.
"""
import math
import os
import sys

if os.environ.get("GYM_REFERENCE"):
    sys.path.insert(0, os.environ["GYM_REFERENCE"])
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import gymnasium as gym  # noqa: E402
from gymnasium.vector import AutoresetMode  # noqa: E402

assert int(np.__version__.split(".")[0]) >= 2, "the fixture must be generated with NumPy >= 2"
OUT = os.path.dirname(os.path.abspath(__file__))
N, T, T_SWITCH, M, MAX_STEPS = 96, 96, 48, 256, 25
N_DEFAULT = 4  # sub-environments 0..3 keep every attribute at its default
SEEDS = [2000 + 11 * i for i in range(N)]
ASEED = 47

# the engine's id order (include/mi355env.h MI_ATTR_ACROBOT_*) and the reference's defaults
NAMES = ["LINK_LENGTH_1", "LINK_MASS_1", "LINK_MASS_2", "LINK_COM_POS_1", "LINK_COM_POS_2", "LINK_MOI", "MAX_VEL_1", "MAX_VEL_2", "dt",
         "torque_noise_max", "book_or_nips"]
DEFAULTS = [1.0, 1.0, 1.0, 0.5, 0.5, 1.0, 4 * math.pi, 9 * math.pi, 0.2, 0.0, "book"]


def r4(x):
    return float(np.round(x, 4))


def draw(rng, n, noise=True, n_default=0):
    """n sets of attribute values as the Python objects a user would pass: {name: [value] * n}; light links and a generous torque, so that
    episodes of 25 steps terminate."""
    u = lambda lo, hi: [r4(v) for v in rng.uniform(lo, hi, n)]  # noqa: E731
    ints = rng.random(n) < 0.2
    noisy = rng.random(n) < 0.6
    light = rng.random(n) < 0.5  # links light enough for the torque (1 + noise) to swing them over the bar within an episode
    vals = {
        "LINK_LENGTH_1": [1 if ints[i] else v for i, v in enumerate(u(0.6, 1.4))],
        "LINK_MASS_1": [1 if ints[i] else (w if light[i] else v) for i, (v, w) in enumerate(zip(u(0.2, 1.2), u(0.01, 0.12)))],
        "LINK_MASS_2": [1 if (ints[i] and i % 2) else (w if light[i] else v) for i, (v, w) in enumerate(zip(u(0.2, 1.2), u(0.01, 0.12)))],
        "LINK_COM_POS_1": u(0.3, 0.9),
        "LINK_COM_POS_2": u(0.3, 0.9),
        "LINK_MOI": [1 if (ints[i] and i % 3 == 0) else v for i, v in enumerate(u(0.5, 1.5))],
        "MAX_VEL_1": [8 if ints[i] else v for i, v in enumerate(u(2.0, 14.0))],
        "MAX_VEL_2": [20 if ints[i] else v for i, v in enumerate(u(4.0, 30.0))],
        "dt": u(0.1, 0.25),
        "torque_noise_max": [(2 if ints[i] else v) if (noisy[i] and noise) else (0 if ints[i] else 0.0) for i, v in enumerate(u(1.0, 4.0))],
        "book_or_nips": ["nips" if k else "book" for k in rng.random(n) < 0.5],
    }
    for name, d in zip(NAMES, DEFAULTS):
        vals[name][:n_default] = [d] * n_default
    return vals


def as_rows(vals):
    rows = np.array([[(1.0 if v == "nips" else 0.0) if isinstance(v, str) else float(v) for v in vals[a]] for a in NAMES], dtype=np.float64)
    ints = np.array([[type(v) is int for v in vals[a]] for a in NAMES], dtype=bool)
    return rows, ints


def pcg_words(gen):
    st = gen.bit_generator.state
    assert st["bit_generator"] == "PCG64" and st["has_uint32"] == 0
    s, i, m = st["state"]["state"], st["state"]["inc"], (1 << 64) - 1
    return [s >> 64, s & m, i >> 64, i & m]


def run(mode, seed_rng):
    vec = gym.make_vec("Acrobot-v1", num_envs=N, vectorization_mode="sync", max_episode_steps=MAX_STEPS, vector_kwargs={"autoreset_mode": mode})
    obs0, _ = vec.reset(seed=SEEDS)
    v0, v1 = draw(seed_rng, N, n_default=N_DEFAULT), draw(seed_rng, N, n_default=N_DEFAULT)
    for name, vals in v0.items():
        vec.set_attr(name, vals)
        assert list(vec.get_attr(name)) == vals
    vec.action_space.seed(ASEED)
    A, O, R, TE, TR, FO, FM = [], [], [], [], [], [], []
    for t in range(T):
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
    rng_words = np.array([pcg_words(e.unwrapped.np_random) for e in vec.envs], dtype=np.uint64)
    vec.close()
    a0, i0 = as_rows(v0)
    a1, i1 = as_rows(v1)
    out = dict(seeds=np.array(SEEDS, dtype=np.int64), aseed=np.int64(ASEED), switch=np.int64(T_SWITCH), max_steps=np.int64(MAX_STEPS), obs0=obs0,
               actions=np.stack(A), obs=np.stack(O), reward=np.stack(R), term=np.stack(TE), trunc=np.stack(TR), attr0=a0, attr1=a1, attr0_int=i0,
               attr1_int=i1, rng=rng_words)
    if mode == AutoresetMode.SAME_STEP:
        out.update(final_obs=np.stack(FO), final_mask=np.stack(FM))
    return out


def check_run(out):
    """The NEXT_STEP run exercises what it is there for."""
    term, trunc = out["term"], out["trunc"]
    noisy = [(out["attr0"][9] > 0), (out["attr1"][9] > 0)]
    sw = int(out["switch"])
    assert trunc.sum() >= 20, f"only {trunc.sum()} truncations"
    noisy_terms = int(term[:sw][:, noisy[0]].sum() + term[sw:][:, noisy[1]].sum())
    assert noisy_terms >= 3, f"only {noisy_terms} terminations among the noisy sub-environments"
    # an autoreset of a noisy sub-environment followed by further noisy steps: the episode ends at t, t + 1 is the reset step, t + 2 steps again
    followed = 0
    for t, i in zip(*np.nonzero(term | trunc)):
        ph = 0 if t + 2 < sw else 1
        if t + 2 < term.shape[0] and noisy[ph][i] and not (t + 1 < sw <= t + 2):
            followed += 1
    assert followed >= 1, "no autoreset of a noisy sub-environment is followed by noisy steps"
    for ph in (0, 1):
        a = out[f"attr{ph}"]
        assert (a[9] > 0).any() and (a[9] == 0).any() and (a[10] == 1).any() and (a[10] == 0).any()
        assert out[f"attr{ph}_int"][:6].any(), "no Python int among the masses and lengths"
        assert all(a[k][0] == (0.0 if isinstance(d, str) else d) for k, d in enumerate(DEFAULTS)), "sub-environment 0 is not all defaults"
    print(f"run: {int(trunc.sum())} truncations, {int(term.sum())} terminations ({noisy_terms} noisy), {followed} noisy autoresets followed by noisy steps")


def teacher(rng):
    half = M // 2
    vals = draw(rng, half, noise=False)
    vals = {k: v + v for k, v in vals.items()}
    vals["book_or_nips"] = vals["book_or_nips"][:half] + ["book" if v == "nips" else "nips" for v in vals["book_or_nips"][:half]]
    mv1, mv2 = np.array([float(v) for v in vals["MAX_VEL_1"][:half]]), np.array([float(v) for v in vals["MAX_VEL_2"][:half]])
    s = np.stack([rng.uniform(-math.pi, math.pi, half), rng.uniform(-math.pi, math.pi, half), rng.uniform(-1, 1, half) * mv1,
                  rng.uniform(-1, 1, half) * mv2], 1)
    q = half // 4  # a quarter of the rows starts next to an end of the angle range and moves across it; another at a velocity limit
    sign = np.where(rng.random(q) < 0.5, -1.0, 1.0)
    s[:q, 0] = sign * (math.pi - rng.uniform(0, 0.2, q))
    s[:q, 2] = sign * rng.uniform(0.5, 1.0, q) * mv1[:q]
    sign = np.where(rng.random(q) < 0.5, -1.0, 1.0)
    s[q:2 * q, 1] = sign * (math.pi - rng.uniform(0, 0.2, q))
    s[q:2 * q, 3] = sign * rng.uniform(0.5, 1.0, q) * mv2[q:2 * q]
    s[2 * q:3 * q, 2] = np.where(rng.random(q) < 0.5, -1.0, 1.0) * mv1[2 * q:3 * q]
    s[2 * q:3 * q, 3] = np.where(rng.random(q) < 0.5, -1.0, 1.0) * mv2[2 * q:3 * q]
    s = np.concatenate([s, s])
    act = rng.integers(0, 3, half)
    act = np.concatenate([act, act])

    def step_all(vals):
        env = gym.make("Acrobot-v1").unwrapped
        env.reset(seed=0)
        ns, ob, rw, te = [], [], [], []
        for k in range(M):
            for name in NAMES:
                setattr(env, name, vals[name][k])
            env.state = np.array(s[k], dtype=np.float64)
            o, r, t, _, _ = env.step(int(act[k]))
            ns.append(np.asarray(env.state, dtype=np.float64)), ob.append(o), rw.append(r), te.append(t)
        return np.stack(ns), np.stack(ob), np.array(rw, dtype=np.float64), np.array(te, dtype=bool)

    ns, ob, rw, te = step_all(vals)
    # every numeric attribute is accepted as np.float64 (classic_control.py ENV_ATTRS): the same steps with np.float64 values
    strong = {name: [v if isinstance(v, str) else np.float64(v) for v in vals[name]] for name in NAMES}
    for x, y in zip((ns, ob, rw, te), step_all(strong)):
        assert np.array_equal(x, y), "an np.float64 attribute changed the reference's result"
    rows, ints = as_rows(vals)
    differ = int((ns[:half] != ns[half:]).any(axis=1).sum())
    assert differ >= half // 2, f"book and nips differ in only {differ} of {half} rows"
    assert (ns[:, 2] == rows[6]).any() and (ns[:, 2] == -rows[6]).any() and (ns[:, 3] == rows[7]).any() and (ns[:, 3] == -rows[7]).any(), "a velocity clip is not reached"
    for c in (0, 1):
        jump = ns[:, c] - s[:, c]
        assert (jump < -math.pi).any() and (jump > math.pi).any(), f"theta{c + 1} does not wrap both ways"
    print(f"teacher: {differ}/{half} book/nips pairs differ; clips and wraps reached; {int(te.sum())} terminal rows")
    return dict(teacher_state=s, teacher_attr=rows, teacher_attr_int=ints, teacher_action=act.astype(np.int64), teacher_next_state=ns, teacher_obs=ob,
                teacher_reward=rw, teacher_term=te)


def main():
    arrs = {}
    out = run(AutoresetMode.NEXT_STEP, np.random.default_rng(104))
    check_run(out)
    for k, v in out.items():
        arrs["run_" + k] = v
    for k, v in run(AutoresetMode.SAME_STEP, np.random.default_rng(104)).items():
        arrs["same_" + k] = v
    assert arrs["same_final_mask"].sum() >= 20
    arrs.update(teacher(np.random.default_rng(204)))
    path = os.path.join(OUT, "env_attrs_acrobot.npz")
    np.savez_compressed(path, **arrs)
    print(f"env_attrs_acrobot.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
