#!/usr/bin/env python3
"""Fixtures of NormalizeObservation / NormalizeReward around every SCALAR env of a vector env, recorded FROM THE REFERENCE ITSELF.

Run in the build container only (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_per_env_normalize.py [output directory]

It imports gymnasium from the reference tree (GYM_REFERENCE, default /root/reference; NumPy >= 2) and writes per_env_normalize_<id>_<mode>.npz for
CartPole-v1 (max_episode_steps=30), Pendulum-v1 (7: truncation never clears the accumulator) and MountainCarContinuous-v0 (25) under NEXT_STEP,
SAME_STEP and DISABLED: SyncVectorEnv over 70 x NormalizeReward(NormalizeObservation(Probe(gym.make(id))), gamma=0.99) -- 70 = one wavefront and a
partial one --, reset(seed=3), 80 steps of action_space.sample() from action_space.seed(1); DISABLED with a masked reset of the rows that ended after
every step that ended some.  Probe sits under the two wrappers, changes nothing and records what they were given, so that every file holds the raw
stream next to the normalised one:

  obs0 / raw_obs0 [N, D]; actions [T, N(, A)]; obs / raw_obs [T, N, D]; reward / raw_reward [T, N]; term / trunc [T, N];
  SAME_STEP: final_obs / raw_final_obs [T, N, D] (zero outside final_mask [T, N]); DISABLED: reset_mask [T, N], reset_obs (the FULL batch reset()
  returned: rows outside the mask keep what they returned last) / raw_reset_obs [T, N, D];
  after the last step: obs_mean / obs_var [N, D], obs_count [N], ret_mean / ret_var / ret_count / acc [N].

per_env_normalize_float64_replay.npz: the float64 path (the MuJoCo ids' observations; mujoco is not importable here).  The SCALAR wrappers over a
replay env -- float64 Box(3,), columns scaled 1, 1e3 and 1e-3 --, 5 streams as the 5 rows, 40 steps, a reset after every termination: the same arrays
as a DISABLED file.

The script ASSERTS the coverage the fixtures exist for: CartPole holds at least 50 terminations, 10 truncations without termination and rows that
reset at least twice; the float64 file holds an output that differs from the recurrence without the first-update quirk (the reference's statistics
are float32 arrays until the first update) and a stream that terminates.  Everything is a function of the fixed seeds: a second run writes the same
arrays bit for bit.
"""
import os
import sys

REF = os.environ.get("GYM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import gymnasium as gym  # noqa: E402
from gymnasium.vector import AutoresetMode, SyncVectorEnv  # noqa: E402
from gymnasium.wrappers import NormalizeObservation, NormalizeReward  # noqa: E402

import per_env_normalize_cases as cases  # noqa: E402

assert int(np.__version__.split(".")[0]) >= 2, "the fixtures must be generated with NumPy >= 2"
OUT = os.path.dirname(os.path.abspath(__file__))
N, T, GAMMA, SEED, ASEED = cases.N, cases.T, cases.GAMMA, cases.SEED, cases.ASEED
MODES = {"next": AutoresetMode.NEXT_STEP, "same": AutoresetMode.SAME_STEP, "disabled": AutoresetMode.DISABLED}
STREAMS, REPLAY_STEPS = 5, 40


class Probe(gym.Wrapper):
    """Under the wrappers being recorded: keeps what the env returned in the vector call in progress.  Changes nothing."""

    def __init__(self, env):
        super().__init__(env)
        self.clear()

    def clear(self):
        self.step_obs = self.step_reward = self.reset_obs = None

    def reset(self, **kwargs):
        obs, info = self.env.reset(**kwargs)
        self.reset_obs = np.array(obs, copy=True)
        return obs, info

    def step(self, action):
        out = self.env.step(action)
        self.step_obs, self.step_reward = np.array(out[0], copy=True), float(out[1])
        return out


def find(env, cls):
    while not isinstance(env, cls):
        env = env.env
    return env


def final_statistics(envs):
    on, rn = [find(e, NormalizeObservation) for e in envs], [find(e, NormalizeReward) for e in envs]
    return dict(obs_mean=np.stack([w.obs_rms.mean for w in on]), obs_var=np.stack([w.obs_rms.var for w in on]),
                obs_count=np.array([w.obs_rms.count for w in on], dtype=np.float64),
                ret_mean=np.array([float(w.return_rms.mean) for w in rn]), ret_var=np.array([float(w.return_rms.var) for w in rn]),
                ret_count=np.array([w.return_rms.count for w in rn], dtype=np.float64),
                acc=np.array([float(w.discounted_reward[0]) for w in rn]))


def run(env_id, limit, mode_name):
    mode = MODES[mode_name]
    vec = SyncVectorEnv([lambda: NormalizeReward(NormalizeObservation(Probe(gym.make(env_id, max_episode_steps=limit))), gamma=GAMMA)] * N,
                        autoreset_mode=mode)
    probes = [find(e, Probe) for e in vec.envs]
    obs0, _ = vec.reset(seed=SEED)
    raw_obs0 = np.stack([p.reset_obs for p in probes])
    vec.action_space.seed(ASEED)
    A, O, RO, R, RR, TE, TR, FO, RFO, FM, RM, RSO, RRSO = ([] for _ in range(13))
    resets = np.zeros(N, dtype=np.int64)
    for t in range(T):
        for p in probes:
            p.clear()
        pending = vec._autoreset_envs.copy()
        a = vec.action_space.sample()
        o, r, te, tr, info = vec.step(a)
        done = te | tr
        raw_o, raw_r = np.zeros_like(raw_obs0), np.zeros(N)
        fo, raw_fo, fm = np.zeros_like(o), np.zeros_like(raw_obs0), np.zeros(N, dtype=bool)
        for i, p in enumerate(probes):
            if mode == AutoresetMode.NEXT_STEP and pending[i]:
                assert p.step_obs is None and r[i] == 0.0
                raw_o[i] = p.reset_obs
            else:
                raw_r[i] = p.step_reward
                if mode == AutoresetMode.SAME_STEP and done[i]:
                    raw_fo[i], raw_o[i], fm[i], fo[i] = p.step_obs, p.reset_obs, True, info["final_obs"][i]
                else:
                    raw_o[i] = p.step_obs
        if mode == AutoresetMode.SAME_STEP:
            assert np.array_equal(fm, info.get("_final_obs", np.zeros(N, dtype=bool)))
            resets += done
        if mode == AutoresetMode.NEXT_STEP:
            resets += pending
        A.append(a), O.append(o.copy()), RO.append(raw_o), R.append(r.copy()), RR.append(raw_r), TE.append(te.copy()), TR.append(tr.copy())
        FO.append(fo), RFO.append(raw_fo), FM.append(fm)
        if mode == AutoresetMode.DISABLED:
            rso, raw_rso = np.zeros_like(o), np.zeros_like(raw_obs0)
            if done.any():
                for p in probes:
                    p.clear()
                rso, _ = vec.reset(options={"reset_mask": done.copy()})
                rso = rso.copy()
                for i in np.flatnonzero(done):
                    raw_rso[i] = probes[i].reset_obs
                assert all(probes[i].reset_obs is None for i in np.flatnonzero(~done))
                assert np.array_equal(rso[~done], o[~done]), "rows outside the mask keep the observation they returned last"
                resets += done
            RM.append(done.copy()), RSO.append(rso), RRSO.append(raw_rso)
    out = dict(obs0=obs0, raw_obs0=raw_obs0, actions=np.stack(A), obs=np.stack(O), raw_obs=np.stack(RO), reward=np.stack(R), raw_reward=np.stack(RR),
               term=np.stack(TE), trunc=np.stack(TR), **final_statistics(vec.envs))
    if mode == AutoresetMode.SAME_STEP:
        out.update(final_obs=np.stack(FO), raw_final_obs=np.stack(RFO), final_mask=np.stack(FM))
    if mode == AutoresetMode.DISABLED:
        out.update(reset_mask=np.stack(RM), reset_obs=np.stack(RSO), raw_reset_obs=np.stack(RRSO))
    assert out["obs"].dtype == np.float32 and out["raw_obs"].dtype == np.float32 and out["reward"].dtype == np.float64
    vec.close()
    cover = dict(terminations=int(out["term"].sum()), truncations=int((out["trunc"] & ~out["term"]).sum()), reset_twice=int((resets >= 2).sum()))
    return out, cover


class Replay(gym.Env):
    """Plays back a float64 stream: reset() and step() return its next row."""

    def __init__(self, obs, reward, terminated):
        self.observation_space = gym.spaces.Box(-np.inf, np.inf, (3,), np.float64)
        self.action_space = gym.spaces.Discrete(2)
        self._obs, self._reward, self._terminated, self._k = obs, reward, terminated, 0

    def _next(self):
        self._k += 1
        return self._obs[self._k - 1].copy()

    def reset(self, *, seed=None, options=None):
        return self._next(), {}

    def step(self, action):
        j = self._k
        return self._next(), float(self._reward[j]), bool(self._terminated[j]), False, {}


def float64_replay():
    rng = np.random.default_rng(20250)
    scale = np.array([1.0, 1e3, 1e-3])
    raw_obs0 = np.zeros((STREAMS, 3))
    raw_obs, raw_reset = np.zeros((REPLAY_STEPS, STREAMS, 3)), np.zeros((REPLAY_STEPS, STREAMS, 3))
    obs0 = np.zeros((STREAMS, 3), np.float32)
    obs, reset_obs = np.zeros((REPLAY_STEPS, STREAMS, 3), np.float32), np.zeros((REPLAY_STEPS, STREAMS, 3), np.float32)
    raw_reward, reward = np.zeros((REPLAY_STEPS, STREAMS)), np.zeros((REPLAY_STEPS, STREAMS))
    term = np.zeros((REPLAY_STEPS, STREAMS), dtype=bool)
    envs = []
    for s in range(STREAMS):
        te = rng.random(REPLAY_STEPS) < (0.0 if s == 0 else 0.12)
        rows = (rng.normal(size=(1 + REPLAY_STEPS + int(te.sum()), 3)) * (1.0 + s) + s) * scale
        rew = rng.normal(size=1 + REPLAY_STEPS + int(te.sum())) * 3.0 - 1.0
        # the env's stream is indexed by its own counter: lay the rewards / terminations out along it
        k, r_at, t_at = 1, np.zeros(len(rows)), np.zeros(len(rows), dtype=bool)
        for t in range(REPLAY_STEPS):
            r_at[k], t_at[k] = rew[k], te[t]
            k += 2 if te[t] else 1
        env = NormalizeReward(NormalizeObservation(Replay(rows, r_at, t_at)), gamma=GAMMA)
        envs.append(env)
        k = 0
        o, _ = env.reset()
        assert o.dtype == np.float32
        raw_obs0[s], obs0[s], k = rows[k], o, k + 1
        last = o
        for t in range(REPLAY_STEPS):
            o, r, terminated, truncated, _ = env.step(0)
            raw_obs[t, s], obs[t, s], raw_reward[t, s], reward[t, s], term[t, s], k = rows[k], o, r_at[k], r, terminated, k + 1
            last = o
            if terminated:
                o, _ = env.reset()
                raw_reset[t, s], last, k = rows[k], o, k + 1
            reset_obs[t, s] = last
        assert k == len(rows)
    # (reset_obs: as a vector env's masked reset returns it -- the full batch; rows of a step without any reset are zero, like the DISABLED files')
    reset_obs[~term.any(axis=1)] = 0.0
    out = dict(obs0=obs0, raw_obs0=raw_obs0, obs=obs, raw_obs=raw_obs, reward=reward, raw_reward=raw_reward, term=term, trunc=np.zeros_like(term),
               reset_mask=term.copy(), reset_obs=reset_obs, raw_reset_obs=raw_reset, **final_statistics(envs))
    assert out["obs_mean"].dtype == np.float64 and term.sum() >= 5 and not term[:, 0].any()
    # the quirk must show: the same stream through the restatement with and without it
    with_quirk = cases.replay(out, "disabled", np.float64)
    assert np.array_equal(with_quirk["obs"], obs) and np.array_equal(with_quirk["obs0"], obs0), "the restatement does not reproduce the float64 stream"

    class NoQuirk(cases.ObsNormalizer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.first[:] = False

    without = cases.replay(out, "disabled", np.float64, obs_cls=NoQuirk)
    differing = int((without["obs"] != obs).sum() + (without["obs0"] != obs0).sum())
    assert differing >= 1, "no recorded output shows the first-update quirk"
    print(f"  float64 replay: {int(term.sum())} terminations, {differing} outputs differ from the recurrence without the first-update quirk")
    return out


def save(out_dir, name, **arrs):
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size < 500_000, f"{name}: {size} bytes"
    print(f"{name}: {size / 1024:.1f} KiB")


def main(out_dir=OUT):
    for key, env_id in cases.IDS.items():
        for mode in cases.MODES:
            out, cover = run(env_id, cases.LIMITS[key], mode)
            print(f"  {key} {mode}: {cover}")
            if key == "cartpole":
                assert cover["terminations"] >= 50 and cover["truncations"] >= 10 and cover["reset_twice"] >= 1, cover
            if key == "pendulum":
                assert cover["terminations"] == 0 and cover["truncations"] >= N, cover
            save(out_dir, f"per_env_normalize_{key}_{mode}.npz", **out)
    save(out_dir, "per_env_normalize_float64_replay.npz", **float64_replay())


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
