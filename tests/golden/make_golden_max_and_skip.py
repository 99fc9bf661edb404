#!/usr/bin/env python3
"""Fixtures of MaxAndSkipObservation around every sub-environment, recorded FROM THE REFERENCE ITSELF.

Run in the build container only (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_max_and_skip.py [output directory]

It imports gymnasium from the reference tree (GYM_REFERENCE, default /root/reference; NumPy >= 2) and writes, per id, max_and_skip_<key>.npz and
max_and_skip_<key>_inner.npz (the *_inner_obs arrays alone: one file would pass the size limit of a committed file).
Every run is gym.make_vec(id, 96, "sync", wrappers=(Probe, lambda e: MaxAndSkipObservation(e, skip)), max_episode_steps=limit) under the vector
RecordEpisodeStatistics (not under DISABLED), reset(seed=SEED), random policy from action_space.seed(ASEED); 96 = one full wavefront and a partial one.

  run                          skip  limit    mode       steps  what it pins
  s4_11_next, s4_11_same       4     11       NEXT/SAME  40     truncation at inner step skip - 2: slot 0 fresh, slot 1 stale
  s4_9_next, s4_9_same         4     9        NEXT/SAME  40     truncation at inner step 0: both slots stale
  s2_5_next                    2     5        NEXT       40     the smallest skip
  s4_3_next                    4     3        NEXT       12     slot 1 is the constructor's zeros forever
  s4_default_next (CartPole)   4     default  NEXT       40     terminations at every inner step, stale frames from an earlier episode
  s4_11_disabled               4     11       DISABLED   12     masked reset after every step that finished rows
  sticky_s4_11_next            4     11       NEXT       40     StickyAction(MaxAndSkipObservation(e, 4), 0.5, 2)
  stack_s4_11_next             4     11       NEXT       24     FrameStackObservation(MaxAndSkipObservation(e, 4), 4)

Per step: actions, obs, reward, term, trunc, final_obs / final_mask (SAME_STEP), ep_r / ep_l / ep_mask (the vector RecordEpisodeStatistics' "r" / "l" /
"_episode"), and what the Probe between TimeLimit and the wrapper saw: inner (the number of inner steps; 0 in a NEXT_STEP autoreset step) and
inner_obs[.., 0 / 1, :] (the observations after inner steps skip - 2 and skip - 1, zeros where the step ended before).  At the end: frames (the 96
wrappers' _obs_buffer as [2][96][OBS]) and rng (the sub-environments' generators, [96][4] words).  The stack run's obs are [T][96][4][OBS]; its inner
observations are not kept (the buffer rule is pinned by the other runs).  Acrobot also *_inexact: the elements of RESET observations where NumPy's
float32 SIMD cos / sin is not the correctly rounded value; the frame slots hold step observations, which have no such exception.

  teacher_*   64 (state, action) rows, each stepped ONCE through a fresh MaxAndSkipObservation(gym.make(id), 4) (all-zero frames) from
              env.unwrapped.state: where the id can terminate at all, 48 of them terminate after 1 .. 3 inner steps.

The script ASSERTS the coverage the fixtures exist for and fails otherwise:
  (a) each *_9_* run holds steps where both slots were stale;
  (b) each *_11_* and s2_5 run holds steps where exactly one slot was stale;
  (c) in each run of (b) at least one returned frame differs from the last inner observation;
  (d) in each run of (b) at least one returned frame differs from the maximum over the slots written in that step alone: a stale element decided;
  (e) s4_3_next starts every row from all-zero slots (and slot 1 is still all zeros at the end);
  (f) CartPole's default-limit run holds a termination at an inner step below skip - 2.
Everything is a function of the fixed seeds below: a second run writes the same bytes.
"""
import os
import sys

REF = os.environ.get("GYM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import gymnasium as gym  # noqa: E402
from gymnasium.vector import AutoresetMode  # noqa: E402
from gymnasium.wrappers import FrameStackObservation, MaxAndSkipObservation, StickyAction  # noqa: E402
from gymnasium.wrappers.vector import RecordEpisodeStatistics  # noqa: E402

assert int(np.__version__.split(".")[0]) >= 2, "the fixtures must be generated with NumPy >= 2"
OUT = os.path.dirname(os.path.abspath(__file__))
N, M = 96, 64
K, P, D, STACK = 4, 0.5, 2, 4
SEED, ASEED = 4242, 77
IDS = {"cartpole": "CartPole-v1", "pendulum": "Pendulum-v1", "acrobot": "Acrobot-v1", "mountaincar": "MountainCar-v0",
       "mountaincar_continuous": "MountainCarContinuous-v0"}
MODES = {"next": AutoresetMode.NEXT_STEP, "same": AutoresetMode.SAME_STEP, "disabled": AutoresetMode.DISABLED}
# (name, config, skip, limit, mode, steps)
PLAN = [("s4_11_next", "plain", 4, 11, "next", 40), ("s4_11_same", "plain", 4, 11, "same", 40), ("s4_9_next", "plain", 4, 9, "next", 40),
        ("s4_9_same", "plain", 4, 9, "same", 40), ("s2_5_next", "plain", 2, 5, "next", 40), ("s4_3_next", "plain", 4, 3, "next", 12),
        ("s4_11_disabled", "plain", 4, 11, "disabled", 12), ("sticky_s4_11_next", "sticky", 4, 11, "next", 40),
        ("stack_s4_11_next", "stack", 4, 11, "next", 24)]
CARTPOLE_PLAN = [("s4_default_next", "plain", 4, None, "next", 40)]


class Probe(gym.Wrapper):
    """Between TimeLimit and the wrapper under test: keeps the inner steps of the outer step in progress.  Changes nothing."""

    def __init__(self, env):
        super().__init__(env)
        self.seen, self.ended = [], None

    def step(self, action):
        out = self.env.step(action)
        self.seen.append(np.array(out[0], copy=True))
        if out[2] or out[3]:
            self.ended = ("term" if out[2] else "trunc", len(self.seen))
        return out


def wrappers_of(config, skip):
    if config == "sticky":
        return (Probe, lambda e: MaxAndSkipObservation(e, skip), lambda e: StickyAction(e, P, D))
    if config == "stack":
        return (Probe, lambda e: MaxAndSkipObservation(e, skip), lambda e: FrameStackObservation(e, STACK))
    return (Probe, lambda e: MaxAndSkipObservation(e, skip))


def find(env, cls):
    while not isinstance(env, cls):
        env = env.env
    return env


def rng_words(vec):
    rows = []
    for e in vec.envs:
        st = e.unwrapped.np_random.bit_generator.state
        assert st["has_uint32"] == 0, "a classic lane carries no buffered 32-bit half"
        s, i, m = st["state"]["state"], st["state"]["inc"], (1 << 64) - 1
        rows.append([s >> 64, s & m, i >> 64, i & m])
    return np.array(rows, dtype=np.uint64)


def inexact_reset_obs(sync, obs, rows):
    """Acrobot only.  Right after a reset the state is a float32 array and NumPy evaluates cos / sin of it with its own float32 SIMD kernels, whose
    result depends on the CPU's features and is not always the correctly rounded one (<= 1 float32 ulp: the project's one stated parity exception;
    the engine returns the correctly rounded value).  Marks the elements of the rows that just reset where THIS machine's recording is not the
    correctly rounded value -- from the reference's state alone --; asserts that they are within 1 ulp of it.  `obs` may carry a stack axis: every
    frame of a row that just reset is the reset observation."""
    mask = np.zeros(obs.shape, dtype=bool)
    for i in np.flatnonzero(rows):
        s = sync.envs[i].unwrapped.state
        assert s.dtype == np.float32
        t1, t2 = float(s[0]), float(s[1])
        exact = np.array([np.cos(t1), np.sin(t1), np.cos(t2), np.sin(t2)]).astype(np.float32)
        got = obs[i].reshape(-1, obs.shape[-1])[-1]
        m = got[:4] != exact
        mask[i].reshape(-1, obs.shape[-1])[:, :4] = m  # (FrameStackObservation pads with the reset observation: every frame of the row is a copy of it)
        assert (obs[i].reshape(-1, obs.shape[-1]) == got).all()
        ulps = np.abs(got[:4].view(np.int32).astype(np.int64) - exact.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (i, got, exact)
    return mask


def run(env_id, config, skip, limit, mode_name, steps):
    mode = MODES[mode_name]
    acrobot = env_id.startswith("Acrobot")
    kw = {} if limit is None else {"max_episode_steps": limit}
    vec = gym.make_vec(env_id, num_envs=N, vectorization_mode="sync", wrappers=wrappers_of(config, skip), vector_kwargs={"autoreset_mode": mode}, **kw)
    sync = vec
    if mode != AutoresetMode.DISABLED:
        vec = RecordEpisodeStatistics(vec)
    obs0, _ = vec.reset(seed=SEED)
    obs0_inexact = inexact_reset_obs(sync, obs0, np.ones(N, dtype=bool)) if acrobot else None
    vec.action_space.seed(ASEED)
    ms = [find(e, MaxAndSkipObservation) for e in sync.envs]
    probes = [find(e, Probe) for e in sync.envs]
    dim = ms[0]._obs_buffer.shape[1]
    start_zero = all(not m._obs_buffer.any() for m in ms)
    cover = {"both_stale": 0, "one_stale": 0, "differs_from_last": 0, "stale_decides": 0, "term_below": 0, "start_zero": int(start_zero)}
    IX, RIX, prev_done = [], [], np.zeros(N, dtype=bool)
    A, O, R, TE, TR, FO, FM, ER, EL, EM, RM, RO, IN, IO = [], [], [], [], [], [], [], [], [], [], [], [], [], []
    for t in range(steps):
        a = vec.action_space.sample()
        for p in probes:
            p.seen, p.ended = [], None
        o, r, te, tr, info = vec.step(a)
        fo, fm = np.zeros_like(o), np.zeros(N, dtype=bool)
        if "final_obs" in info:
            fm = info["_final_obs"].copy()
            for i in np.where(fm)[0]:
                fo[i] = info["final_obs"][i]
        inner, inner_obs = np.zeros(N, dtype=np.int8), np.zeros((N, 2, dim), dtype=np.float32)
        for i, p in enumerate(probes):
            n = len(p.seen)
            inner[i] = n
            if n == 0:
                continue
            if n >= skip - 1:
                inner_obs[i, 0] = p.seen[skip - 2]
            if n >= skip:
                inner_obs[i, 1] = p.seen[skip - 1]
            if config != "stack":
                frame = fo[i] if (mode == AutoresetMode.SAME_STEP and fm[i]) else o[i]
                written = [p.seen[k] for k in (skip - 2, skip - 1) if k < n]
                cover["both_stale"] += len(written) == 0
                cover["one_stale"] += len(written) == 1
                cover["differs_from_last"] += not np.array_equal(frame, p.seen[-1])
                cover["stale_decides"] += len(written) == 0 or not np.array_equal(frame, np.max(np.stack(written), axis=0))
                cover["term_below"] += p.ended is not None and p.ended[0] == "term" and p.ended[1] - 1 < skip - 2
        er, el, em = np.zeros(N), np.zeros(N, dtype=np.int64), np.zeros(N, dtype=bool)
        if "_episode" in info:
            er, el, em = info["episode"]["r"].copy(), info["episode"]["l"].astype(np.int64), info["_episode"].copy()
        A.append(a), O.append(o.copy()), R.append(r.copy()), TE.append(te.copy()), TR.append(tr.copy()), FO.append(fo), FM.append(fm)
        ER.append(er), EL.append(el), EM.append(em), IN.append(inner), IO.append(inner_obs)
        if acrobot:  # (the rows whose observation is a reset's: NEXT_STEP the autoreset step, SAME_STEP the step that finished the episode)
            rows = prev_done if mode == AutoresetMode.NEXT_STEP else ((te | tr) if mode == AutoresetMode.SAME_STEP else np.zeros(N, dtype=bool))
            fresh = inexact_reset_obs(sync, o, rows)
            if config == "stack":  # a marked reset observation stays in the row's stack until it is shifted out or the row resets again
                prev = IX[-1] if IX else obs0_inexact
                moved = np.zeros_like(prev)
                moved[:, :-1] = prev[:, 1:]
                moved[rows] = fresh[rows]
                fresh = moved
            IX.append(fresh)
            prev_done = te | tr
        if mode == AutoresetMode.DISABLED:
            done = te | tr
            ro = np.zeros_like(o)
            if done.any():
                ro, _ = vec.reset(options={"reset_mask": done.copy()})
                ro = ro.copy()
            if acrobot:
                RIX.append(inexact_reset_obs(sync, ro, done))
            RM.append(done.copy()), RO.append(ro)
    frames = np.stack([m._obs_buffer for m in ms], axis=1)
    assert frames.shape == (2, N, dim) and frames.dtype == np.float32
    out = dict(obs0=obs0, actions=np.stack(A), obs=np.stack(O), reward=np.stack(R), term=np.stack(TE), trunc=np.stack(TR), rng=rng_words(sync),
               frames=frames, inner=np.stack(IN))
    if config != "stack":
        out["inner_obs"] = np.stack(IO)
    if mode == AutoresetMode.SAME_STEP:
        out.update(final_obs=np.stack(FO), final_mask=np.stack(FM))
    if mode == AutoresetMode.DISABLED:
        out.update(reset_mask=np.stack(RM), reset_obs=np.stack(RO))
    else:
        out.update(ep_r=np.stack(ER), ep_l=np.stack(EL), ep_mask=np.stack(EM))
    if acrobot:
        out.update(obs0_inexact=obs0_inexact, obs_inexact=np.stack(IX))
        if RIX:
            out["reset_obs_inexact"] = np.stack(RIX)
        resets = int((out["term"] | out["trunc"]).sum())
        marked = int(out["obs_inexact"].sum())
        # a rare event: a few elements per run of ~1000 resets; under the stack an element is counted while it stays in the row's stack (4 + 3 + 2 + 1 times)
        assert marked <= max(2, resets // 50) * (10 if config == "stack" else 1), (marked, resets)
        print(f"    reset observations where NumPy's float32 cos / sin is not the correctly rounded value: {marked} elements in {resets} resets")
    cover["slot1_zero_at_end"] = int(not frames[1].any())
    vec.close()
    return out, cover


def check_cover(key, name, config, cover):
    want = []
    if config != "stack":
        if "_9_" in name:
            want += ["both_stale"]  # (a)
        if "_11_" in name or name.startswith("s2_5"):
            want += ["one_stale", "differs_from_last", "stale_decides"]  # (b) (c) (d)
        if name == "s4_3_next":
            want += ["start_zero", "slot1_zero_at_end"]  # (e)
        if name == "s4_default_next":
            want += ["term_below", "both_stale"]  # (f)
    for w in want:
        assert cover[w] > 0, f"{key} {name}: the run does not contain `{w}` ({cover})"
    print(f"  {name}: " + ", ".join(f"{w}={cover[w]}" for w in want))


# ---- teacher-forced rows ---------------------------------------------------------------------------------------------------------------------
def candidates(key, rng, n):
    """n (state, action) rows near where the id's episodes terminate."""
    sign = lambda k: rng.choice([-1.0, 1.0], k)  # noqa: E731
    if key == "cartpole":
        h = n // 2  # half near the angle limit (12 degrees = 0.2094), half near x_threshold
        angle = np.stack([rng.uniform(-1, 1, h), rng.uniform(-1, 1, h), rng.uniform(0.17, 0.209, h) * sign(h), rng.uniform(-2, 2, h)], 1)
        edge = np.stack([rng.uniform(2.2, 2.4, n - h) * sign(n - h), rng.uniform(-2, 2, n - h), rng.uniform(-0.05, 0.05, n - h), rng.uniform(-1, 1, n - h)], 1)
        return np.concatenate([angle, edge]), rng.integers(0, 2, n)
    if key == "pendulum":
        return np.stack([rng.uniform(-4, 4, n), rng.uniform(-8, 8, n)], 1), rng.uniform(-2.5, 2.5, n).astype(np.float32)
    if key == "acrobot":
        return np.stack([rng.uniform(1.6, 3.1, n) * sign(n), rng.uniform(-1.0, 1.0, n), rng.uniform(-8, 8, n), rng.uniform(-12, 12, n)], 1), rng.integers(0, 3, n)
    if key == "mountaincar":
        return np.stack([rng.uniform(0.4, 0.4999, n), rng.uniform(0.0, 0.07, n)], 1), rng.integers(0, 3, n)
    s = np.stack([rng.uniform(0.35, 0.4499, n), rng.uniform(0.0, 0.07, n)], 1).astype(np.float32).astype(np.float64)
    return s, rng.uniform(-1.2, 1.2, n).astype(np.float32)


def teacher(key, env_id, rng):
    env = MaxAndSkipObservation(Probe(gym.make(env_id)), K)
    env.reset(seed=0)
    probe, limit, raw = find(env, Probe), find(env, gym.wrappers.TimeLimit), env.unwrapped

    def step_row(s, a):
        if key == "mountaincar":
            raw.state = (np.float64(s[0]), np.float64(s[1]))
        else:
            raw.state = np.array(s, dtype=np.float32 if key == "mountaincar_continuous" else np.float64)
        if hasattr(raw, "steps_beyond_terminated"):
            raw.steps_beyond_terminated = None
        limit._elapsed_steps, probe.seen, probe.ended = 0, [], None
        env._obs_buffer[:] = 0  # a FRESH wrapper for every row
        act = a if key in ("cartpole", "acrobot", "mountaincar") else np.array([a], dtype=np.float32)
        o, r, te, tr, _ = env.step(act)
        return np.asarray(raw.state, dtype=np.float64).ravel(), o.copy(), float(r), bool(te), bool(tr), len(probe.seen), env._obs_buffer.copy()

    inside, other = [], []
    want_inside = 0 if key == "pendulum" else 48
    while len(inside) < want_inside or len(other) < M - want_inside:
        S, Aa = candidates(key, rng, 256)
        for s, a in zip(S, Aa):
            ns, o, r, te, tr, inner, fr = step_row(s, a)
            row = (s, a, ns, o, r, te, tr, inner, fr)
            if te and inner < K and len(inside) < want_inside:
                inside.append(row)
            elif not (te and inner < K) and len(other) < M - want_inside:
                other.append(row)
    rows = inside + other
    assert key == "pendulum" or all(x[5] and 1 <= x[7] < K for x in inside), key
    env.close()
    out = dict(teacher_state=np.stack([x[0] for x in rows]), teacher_action=np.array([x[1] for x in rows]),
               teacher_next_state=np.stack([x[2] for x in rows]), teacher_obs=np.stack([x[3] for x in rows]),
               teacher_reward=np.array([x[4] for x in rows], dtype=np.float64), teacher_term=np.array([x[5] for x in rows], dtype=bool),
               teacher_trunc=np.array([x[6] for x in rows], dtype=bool), teacher_inner=np.array([x[7] for x in rows], dtype=np.int64),
               teacher_frames=np.stack([x[8] for x in rows], axis=1))
    print(f"  teacher: {len(inside)} rows terminate inside the skip, inner steps {np.bincount(out['teacher_inner'], minlength=K + 1).tolist()}")
    return out


def save(out_dir, name, **arrs):
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size < 1 << 20, f"{name}: {size} bytes"
    print(f"{name}: {size / 1024:.1f} KiB")


def main(out_dir=OUT):
    for n, (key, env_id) in enumerate(IDS.items()):
        print(key)
        arrs, inner = {}, {}
        for name, config, skip, limit, mode, steps in PLAN + (CARTPOLE_PLAN if key == "cartpole" else []):
            out, cover = run(env_id, config, skip, limit, mode, steps)
            check_cover(key, name, config, cover)
            if "inner_obs" in out:  # (a file of their own: with them an id's fixtures would pass the size limit of a committed file)
                inner[f"{name}_inner_obs"] = out.pop("inner_obs")
            arrs.update({f"{name}_{k}": v for k, v in out.items()})
        arrs.update(teacher(key, env_id, np.random.default_rng(700 + n)))
        save(out_dir, f"max_and_skip_{key}.npz", **arrs)
        save(out_dir, f"max_and_skip_{key}_inner.npz", **inner)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
