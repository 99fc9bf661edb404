"""Record discretize.npz FROM THE REFERENCE: gymnasium.wrappers.DiscretizeObservation / DiscretizeAction (wrappers/transform_observation.py:755-907,
wrappers/transform_action.py:201-345), scalar wrappers that SyncVectorEnv runs around every sub-environment (the reference has no vector form).

    GYM_REFERENCE=/path/to/reference python tests/golden/make_golden_discretize.py      # rewrites tests/golden/discretize.npz

The inputs come from tests/discretize_cases.py.  Keys:

o/<case>/...   DiscretizeObservation over a Box of discretize_cases.BOXES: x (the crafted observations), y (``observation(x[i])``, int64: [rows] flat or
               [rows, D] multidiscrete), edges (``bin_edges`` concatenated), hi_clip (``high - 1e-8``), single ([n] or nvec of the wrapper's space), batched
               (the space SyncVectorEnv of N such envs has: nvec, or [low, high] of its Box), revert ([2, k, D]: ``revert_observation(y[i])`` of the first rows)
a/<case>/...   DiscretizeAction likewise: x (indices), y (``action(x[i])``, the Box's dtype), centers (``bin_centers`` concatenated), single, batched,
               revert (``revert_action(y[i])`` of the first rows)
t/<name>/<mode>/...  SyncVectorEnv of N envs wrapped by discretize_cases.wrap, max_episode_steps = LIMIT: obs0 = reset(seed=SEED); T steps of
               ``action_space.sample()`` after ``action_space.seed(ASEED)``: actions, obs, rewards, term, trunc; final_obs / final_mask (SAME_STEP; zero where
               nothing finished); reset_mask / reset_obs [T, ...]: the masked reset after step t (DISABLED: the finished rows; every mode: MASK after step
               MASK_AT), zero in a step without one
s/<name>       SAMPLE_BATCHES batches of ``action_space.sample()`` of SAMPLE_N wrapped envs after ``action_space.seed(SAMPLE_SEED)``
errors         "ctor/<name>=ExceptionType" of every refused constructor call (discretize_cases.REFUSED)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if "GYM_REFERENCE" in os.environ:  # (otherwise: an installed gymnasium)
    sys.path.insert(0, os.environ["GYM_REFERENCE"])
sys.dont_write_bytecode = True

import discretize_cases as dc  # noqa: E402

REVERT_ROWS = 12


def main():
    import gymnasium as gym
    from gymnasium import spaces
    from gymnasium import wrappers as ref
    from gymnasium.vector import AutoresetMode, SyncVectorEnv
    from gymnasium.vector.utils import batch_space

    assert int(np.__version__.split(".")[0]) >= 2, "the fixture must be generated with NumPy >= 2"

    class SpacesOnly(gym.Env):
        def __init__(self, observation_space, action_space):
            self.observation_space, self.action_space = observation_space, action_space

    def box_of(name):
        low, high = dc.box_arrays(name)
        return spaces.Box(low, high, dtype=low.dtype)

    def space_arrays(space):
        single = np.array([space.n]) if isinstance(space, spaces.Discrete) else np.array(space.nvec)
        b = batch_space(space, dc.N)
        return single, (np.array(b.nvec) if isinstance(b, spaces.MultiDiscrete) else np.stack([b.low, b.high]))

    out, errors = {}, {}
    for case, (name, bins, multi) in dc.OBS_CASES.items():
        w = ref.DiscretizeObservation(SpacesOnly(box_of(name), spaces.Discrete(2)), bins, multidiscrete=multi)
        x = dc.obs_inputs(name, bins)
        y = np.array([w.observation(row) for row in x], dtype=np.int64)
        k = f"o/{case}"
        out[f"{k}/x"], out[f"{k}/y"] = x, y
        out[f"{k}/edges"] = np.concatenate(w.bin_edges) if len(w.bin_edges) else np.zeros(0)
        assert out[f"{k}/edges"].dtype == x.dtype or out[f"{k}/edges"].size == 0, (case, out[f"{k}/edges"].dtype)
        out[f"{k}/hi_clip"] = w.high - 1e-8
        out[f"{k}/single"], out[f"{k}/batched"] = space_arrays(w.observation_space)
        valid = [r for r in y[:REVERT_ROWS]]
        rev = [w.revert_observation(r if multi else int(r)) for r in valid]
        out[f"{k}/revert"] = np.stack([np.stack([lo for lo, _ in rev]), np.stack([hi for _, hi in rev])])
    for case, (name, bins, multi) in dc.ACT_CASES.items():
        w = ref.DiscretizeAction(SpacesOnly(spaces.Discrete(2), box_of(name)), bins, multidiscrete=multi)
        x = dc.act_inputs(name, bins, multi)
        y = np.stack([w.action(row if multi else int(row)) for row in x])
        k = f"a/{case}"
        out[f"{k}/x"], out[f"{k}/y"] = x, y
        out[f"{k}/centers"] = np.concatenate(w.bin_centers)
        out[f"{k}/single"], out[f"{k}/batched"] = space_arrays(w.action_space)
        out[f"{k}/revert"] = np.array([w.revert_action(r) for r in y[:REVERT_ROWS]], dtype=np.int64)
    # refused constructor calls
    for case, (which, env_id, bins) in dc.REFUSED.items():
        try:
            env = gym.make(env_id)
        except Exception:  # noqa: BLE001 -- no MuJoCo here: the id's spaces (mujoco/half_cheetah_v5.py) stand in for the env
            assert env_id == "HalfCheetah-v5", env_id
            env = SpacesOnly(spaces.Box(-np.inf, np.inf, (17,), np.float64), spaces.Box(-1.0, 1.0, (6,), np.float32))
        try:
            (ref.DiscretizeObservation if which == "obs" else ref.DiscretizeAction)(env, bins)
            raise SystemExit(f"the reference accepted {case}")
        except Exception as e:  # noqa: BLE001 -- the TYPE is what is recorded
            errors[f"ctor/{case}"] = type(e).__name__
    # trajectories
    modes = {"next": AutoresetMode.NEXT_STEP, "same": AutoresetMode.SAME_STEP, "disabled": AutoresetMode.DISABLED}
    for name, (env_id, *_rest) in dc.TRAJ.items():
        for mode_name, mode in modes.items():
            vec = SyncVectorEnv([lambda: dc.wrap(ref, gym.make(env_id, max_episode_steps=dc.LIMIT), name)] * dc.N, autoreset_mode=mode)
            obs0, _ = vec.reset(seed=dc.SEED)
            vec.action_space.seed(dc.ASEED)
            rec = {k: [] for k in ("actions", "obs", "rewards", "term", "trunc", "final_obs", "final_mask", "reset_mask", "reset_obs")}
            for t in range(dc.T):
                a = vec.action_space.sample()
                o, r, te, tr, info = vec.step(a)
                done = te | tr
                for k, v in zip(("actions", "obs", "rewards", "term", "trunc"), (a, o, r, te, tr)):
                    rec[k].append(np.array(v))
                if mode_name == "same":
                    fo, fm = np.zeros_like(o), np.zeros(dc.N, dtype=bool)
                    if "final_obs" in info:
                        fm = info["_final_obs"].copy()
                        for i in np.flatnonzero(fm):
                            fo[i] = info["final_obs"][i]
                    assert np.array_equal(fm, done)
                    rec["final_obs"].append(fo), rec["final_mask"].append(fm)
                mask = done.copy() if mode_name == "disabled" else np.zeros(dc.N, dtype=bool)
                if t == dc.MASK_AT:
                    mask |= dc.MASK
                ro = np.zeros_like(o)
                if mask.any():
                    ro = np.array(vec.reset(options={"reset_mask": mask.copy()})[0])
                rec["reset_mask"].append(mask), rec["reset_obs"].append(ro)
            k = f"t/{name}/{mode_name}"
            out[f"{k}/obs0"] = np.array(obs0)
            for key, v in rec.items():
                if v:
                    out[f"{k}/{key}"] = np.stack(v)
            assert (out[f"{k}/term"] | out[f"{k}/trunc"]).sum() >= dc.N, "episodes must end inside the recording"
            vec.close()
    # seeded samples of the wrapper's batched action space
    for name, (env_id, bins, multi) in dc.SAMPLE_CASES.items():
        vec = SyncVectorEnv([lambda: ref.DiscretizeAction(gym.make(env_id), bins, multidiscrete=multi)] * dc.SAMPLE_N)
        vec.action_space.seed(dc.SAMPLE_SEED)
        out[f"s/{name}"] = np.stack([vec.action_space.sample() for _ in range(dc.SAMPLE_BATCHES)])
        vec.close()
    out["errors"] = np.array(sorted(f"{k}={v}" for k, v in errors.items()))
    np.savez_compressed(dc.GOLDEN, **out)
    print(dc.GOLDEN, os.path.getsize(dc.GOLDEN), "bytes,", len(out), "arrays")
    print(*out["errors"], sep="\n")


if __name__ == "__main__":
    main()
