"""Record observation_wrappers.npz FROM THE REFERENCE: gymnasium.wrappers.vector.{RescaleObservation, DtypeObservation, FlattenObservation,
TransformObservation, TransformReward} (wrappers/vector/vectorize_observation.py, vectorize_reward.py, wrappers/transform_observation.py,
wrappers/utils.py rescale_box, spaces/utils.py flatten).

    GYM_REFERENCE=/path/to/reference python tests/golden/make_golden_observation_wrappers.py      # rewrites tests/golden/observation_wrappers.npz

The inputs come from tests/observation_wrapper_cases.py, so the tests need nothing but this file and NumPy.  Keys:

(a) over a vector env that has only spaces (observation_wrapper_cases.SpacesOnlyEnv), ``observations(batch)`` of
      r/B/S      RescaleObservation over box B with target S (RESCALE_TARGETS), batch: crafted(B)       /out /space [low, high] /params [gradient, intercept]
                                                                                                         /meta [same_out]
      d/B/T      DtypeObservation over box B to dtype T (DTYPE_TARGETS), batch: dtype_batch(B, T)       /out /space
      d/E/T      ... over the Discrete space E (DISCRETE), batch: discrete_batch(n)                     /out /space
      f/E        FlattenObservation over the Discrete space E and "blackjack", batch: discrete_batch(n) / blackjack_batch()     /out /space
      f/pendulum ... over a Box                                                                         /out /space
    errors          "key=ExceptionType" of every refused constructor call (the keys above, and ctor/<case>)
    error_messages  "key=message" of the same
(b) t/K/M/obs ([1 + T, N, ...]: the reset observation, then every step's), /rewards ([T, N]), /flags ([terminations, truncations]) and, for M =
    DISABLED, /post ([T, N, ...]: the observations after the masked reset that follows a step with finished sub-environments; the step's own where
    there was none): SyncVectorEnv of TRAJ_N envs in autoreset mode M (TRAJ_MODES) under the wrapper of TRAJECTORIES[K], reset(seed=TRAJ_SEED),
    TRAJ_T steps of observation_wrapper_cases.trajectory_actions
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("GYM_REFERENCE", "/root/reference"))
sys.dont_write_bytecode = True

import observation_wrapper_cases as oc  # noqa: E402


def closure_arrays(func):
    """gradient / intercept out of rescale_box's ``forward`` closure."""
    cells = dict(zip(func.__code__.co_freevars, (c.cell_contents for c in func.__closure__)))
    return cells["gradient"], cells["intercept"]


def constructor_cases(spaces):
    """name -> (single observation space, autoreset mode's name, callable(wrappers, env)) of constructor calls the reference refuses."""
    box = oc.make_box(spaces, "pendulum")
    half = oc.make_box(spaces, "cartpole")
    return {
        "rescale_discrete": (spaces.Discrete(16), "NEXT_STEP", lambda w, e: w.RescaleObservation(e, -1.0, 1.0)),
        "rescale_tuple": (oc.blackjack_space(spaces), "NEXT_STEP", lambda w, e: w.RescaleObservation(e, -1.0, 1.0)),
        "dtype_tuple": (oc.blackjack_space(spaces), "NEXT_STEP", lambda w, e: w.DtypeObservation(e, np.float32)),
        "rescale_bound_is_a_list": (box, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, [0.0] * 3, 1.0)),
        "rescale_bound_is_a_string": (box, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, 0.0, "1")),
        "rescale_wrong_shape": (box, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, np.zeros(2), np.ones(2))),
        "rescale_max_wrong_shape": (box, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, 0.0, np.ones((3, 1)))),
        "rescale_min_above_max": (box, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, 1.0, 0.0)),
        "rescale_infinite_target_finite_box": (box, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, -np.inf, 1.0)),
        "rescale_finite_target_infinite_box": (half, "NEXT_STEP", lambda w, e: w.RescaleObservation(e, -1.0, 1.0)),
        "same_step_rescale": (box, "SAME_STEP", lambda w, e: w.RescaleObservation(e, -1.0, 1.0)),
        "same_step_dtype": (box, "SAME_STEP", lambda w, e: w.DtypeObservation(e, np.float64)),
        "same_step_flatten": (box, "SAME_STEP", lambda w, e: w.FlattenObservation(e)),
        "same_step_transform": (box, "SAME_STEP", lambda w, e: w.TransformObservation(e, oc.transform_func)),
    }


def main():
    import gymnasium as gym
    from gymnasium import spaces
    from gymnasium.vector import AutoresetMode, SyncVectorEnv
    from gymnasium.vector.utils import batch_space
    from gymnasium.wrappers import vector as ref

    warnings.simplefilter("ignore")  # (Box: "precision lowered by casting")
    spaces_only = type("SpacesOnlyVectorEnv", (oc.SpacesOnlyEnv, gym.vector.VectorEnv), {})  # (the reference's wrappers insist on a VectorEnv)
    out, errors, messages = {}, {}, {}

    def stand_in(space, rows, mode="NEXT_STEP"):
        return spaces_only(spaces, batch_space, space, rows, AutoresetMode[mode])

    def record(key, space, batch, make):
        rows = len(batch[0]) if isinstance(batch, tuple) else len(batch)
        try:
            w = make(stand_in(space, rows))
        except Exception as e:  # noqa: BLE001 -- type and message are what is recorded
            errors[key], messages[key] = type(e).__name__, str(e)
            return None
        sp = w.single_observation_space
        out[f"{key}/space"] = np.stack([sp.low, sp.high])
        given = tuple(p.copy() for p in batch) if isinstance(batch, tuple) else batch.copy()
        with np.errstate(all="ignore"):
            out[f"{key}/out"] = np.array(w.observations(given))
        return w

    # (a)
    for name in oc.RESCALE_BOXES:
        for target in oc.RESCALE_TARGETS:
            w = record(f"r/{name}/{target}", oc.make_box(spaces, name), oc.crafted(name), lambda e: oc.build(ref, e, "rescale", target, name))
            if w is not None:
                out[f"r/{name}/{target}/params"] = np.stack(closure_arrays(w.wrapper.func))
                out[f"r/{name}/{target}/meta"] = np.array([int(w.same_out)])
    for name in oc.BOXES:
        for target in oc.DTYPE_TARGETS:
            record(f"d/{name}/{target}", oc.make_box(spaces, name), oc.dtype_batch(name, target), lambda e: oc.build(ref, e, "dtype", target))
    for name, n in oc.DISCRETE.items():
        for target in oc.DTYPE_TARGETS:
            record(f"d/{name}/{target}", spaces.Discrete(n), oc.discrete_batch(n), lambda e: oc.build(ref, e, "dtype", target))
        record(f"f/{name}", spaces.Discrete(n), oc.discrete_batch(n), lambda e: ref.FlattenObservation(e))
    record("f/blackjack", oc.blackjack_space(spaces), oc.blackjack_batch(), lambda e: ref.FlattenObservation(e))
    record("f/pendulum", oc.make_box(spaces, "pendulum"), oc.crafted("pendulum"), lambda e: ref.FlattenObservation(e))
    for case, (space, mode, call) in constructor_cases(spaces).items():
        try:
            call(ref, stand_in(space, 3, mode))
            raise SystemExit(f"the reference accepted {case}")
        except Exception as e:  # noqa: BLE001
            errors[f"ctor/{case}"], messages[f"ctor/{case}"] = type(e).__name__, str(e)
    # (b)
    for key, (env_id, kind, arg) in oc.TRAJECTORIES.items():
        for mode in oc.TRAJ_MODES:
            vec = SyncVectorEnv([lambda: gym.make(env_id) for _ in range(oc.TRAJ_N)], autoreset_mode=AutoresetMode[mode])
            w = oc.build(ref, vec, kind, arg, oc.BOX_OF_ENV.get(env_id))
            obs, _ = w.reset(seed=oc.TRAJ_SEED)
            rec = {k: [] for k in ("obs", "rewards", "terminations", "truncations", "post")}
            rec["obs"].append(np.array(obs))
            for a in oc.trajectory_actions(env_id):
                o, r, te, tr, _ = w.step(a.copy())
                for k, v in zip(rec, (o, r, te, tr)):
                    rec[k].append(np.array(v))
                done = np.logical_or(te, tr)
                if mode == "DISABLED" and done.any():
                    o, _ = w.reset(options={"reset_mask": done})
                rec["post"].append(np.array(o))
            base = f"t/{key}/{mode}"
            out[f"{base}/obs"], out[f"{base}/rewards"] = np.stack(rec["obs"]), np.stack(rec["rewards"])
            out[f"{base}/flags"] = np.stack([np.stack(rec["terminations"]), np.stack(rec["truncations"])])
            if mode == "DISABLED":
                out[f"{base}/post"] = np.stack(rec["post"])
            w.close()
    out["errors"] = np.array(sorted(f"{k}={v}" for k, v in errors.items()))
    out["error_messages"] = np.array(sorted(f"{k}={v}" for k, v in messages.items()))
    path = os.path.join(HERE, "observation_wrappers.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    print(*out["errors"], sep="\n")


if __name__ == "__main__":
    main()
