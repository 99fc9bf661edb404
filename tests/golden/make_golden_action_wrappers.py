"""Record action_wrappers.npz FROM THE REFERENCE: gymnasium.wrappers.vector.{ClipAction, RescaleAction} (wrappers/vector/vectorize_action.py,
wrappers/transform_action.py, wrappers/utils.py rescale_box).

    GYM_REFERENCE=/path/to/reference python tests/golden/make_golden_action_wrappers.py      # rewrites tests/golden/action_wrappers.npz

The inputs come from tests/action_wrapper_cases.py, so the tests need nothing but this file and NumPy.  Keys:

(a) per box B, wrapper stack S (action_wrapper_cases.TRANSFORMS) over a vector env that has only spaces:
      a/B/S/space        [low, high] of the wrapper's single action space (its dtype: the array's)
      a/B/S/meta         [same_out (whether the batched space equals the env's), *shape of the batched space]
      a/B/S/params       [gradient, intercept]: the two arrays inside rescale_box's inverse function (RescaleAction stacks)
      a/B/S/I            what ``actions()`` returns for input I (action_wrapper_cases.INPUTS): the forwarded batch, dtype included
    errors               "key=ExceptionType" of every refused input (key a/B/S/I) and refused constructor call (key ctor/<case>)
(b) per env E, wrapper stack W, dtype D: b/E/W/D/obs ([1 + T, N, obs]: the reset observation, then every step's), /rewards ([T, N]) and /flags
    ([terminations, truncations]): SyncVectorEnv of TRAJ_N envs under W, reset(seed=TRAJ_SEED), TRAJ_T steps of
    action_wrapper_cases.trajectory_actions(E, D)
(c) c/B/S/samples: SAMPLE_BATCHES batches of ``action_space.sample()`` after ``action_space.seed(SAMPLE_SEED)``, SAMPLE_N envs
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("GYM_REFERENCE", "/root/reference"))
sys.dont_write_bytecode = True

import action_wrapper_cases as ac  # noqa: E402


def closure_arrays(func):
    """gradient / intercept out of rescale_box's ``backward`` closure."""
    cells = dict(zip(func.__code__.co_freevars, (c.cell_contents for c in func.__closure__)))
    return cells["gradient"], cells["intercept"]


def constructor_cases(spaces):
    """name -> (single space, callable(wrappers, env)) of constructor calls the reference refuses."""
    box = ac.make_box(spaces, "ant")
    half = spaces.Box(np.array([-1.0, -np.inf], np.float32), np.array([1.0, np.inf], np.float32), dtype=np.float32)
    return {
        "clip_discrete": (spaces.Discrete(2), lambda w, e: w.ClipAction(e)),
        "rescale_discrete": (spaces.Discrete(2), lambda w, e: w.RescaleAction(e, -1.0, 1.0)),
        "rescale_min_equals_max": (box, lambda w, e: w.RescaleAction(e, 0.5, 0.5)),
        "rescale_min_equals_max_one_component": (box, lambda w, e: w.RescaleAction(e, np.zeros(8), np.r_[0.0, np.ones(7)])),
        "rescale_bound_is_a_list": (box, lambda w, e: w.RescaleAction(e, [0.0] * 8, 1.0)),
        "rescale_bound_is_a_string": (box, lambda w, e: w.RescaleAction(e, 0.0, "1")),
        "rescale_wrong_shape": (box, lambda w, e: w.RescaleAction(e, np.zeros(7), np.ones(7))),
        "rescale_max_wrong_shape": (box, lambda w, e: w.RescaleAction(e, 0.0, np.ones((8, 1)))),
        "rescale_min_above_max": (box, lambda w, e: w.RescaleAction(e, 1.0, 0.0)),
        "rescale_infinite_target_finite_box": (box, lambda w, e: w.RescaleAction(e, -np.inf, 1.0)),
        "rescale_finite_target_infinite_box": (half, lambda w, e: w.RescaleAction(e, -1.0, 1.0)),
    }


def main():
    import gymnasium as gym
    from gymnasium import spaces
    from gymnasium.vector import SyncVectorEnv
    from gymnasium.vector.utils import batch_space
    from gymnasium.wrappers import vector as ref

    spaces_only = type("SpacesOnlyVectorEnv", (ac.SpacesOnlyEnv, gym.vector.VectorEnv), {})  # (the reference's wrappers insist on a VectorEnv)
    out, errors = {}, {}
    # (a)
    for name in ac.BOXES:
        batches = ac.inputs(name)
        rows = len(batches["f64"])
        for tr in ac.TRANSFORMS:
            env = spaces_only(spaces, batch_space, ac.make_box(spaces, name), rows)
            w = ac.build(ref, env, tr)
            key = f"a/{name}/{tr}"
            out[f"{key}/space"] = np.stack([w.single_action_space.low, w.single_action_space.high])
            out[f"{key}/meta"] = np.array([int(w.same_out), *w.action_space.shape])
            assert bool(w.same_out) == ac.is_same_out(tr, name), (name, tr)
            if tr.startswith("rescale"):
                out[f"{key}/params"] = np.stack(closure_arrays(w.wrapper.func))
            for inp in ac.INPUTS:
                x = batches[inp]
                given = x.copy() if isinstance(x, np.ndarray) else [list(r) for r in x]
                try:
                    with np.errstate(all="ignore"):
                        got = w.actions(given)
                    out[f"{key}/{inp}"] = np.array(got)
                except Exception as e:  # noqa: BLE001 -- the TYPE is what is recorded
                    errors[f"{key}/{inp}"] = type(e).__name__
    for case, (space, call) in constructor_cases(spaces).items():
        env = spaces_only(spaces, batch_space, space, 3)
        try:
            call(ref, env)
            raise SystemExit(f"the reference accepted {case}")
        except Exception as e:  # noqa: BLE001
            errors[f"ctor/{case}"] = type(e).__name__
    # (b)
    for env_name, env_id in ac.TRAJ_ENVS.items():
        for tr in ac.TRAJ_WRAPPERS:
            for dtype in (np.float32, np.float64):
                vec = SyncVectorEnv([lambda: gym.make(env_id) for _ in range(ac.TRAJ_N)])
                w = ac.build(ref, vec, tr)
                key = f"b/{env_name}/{tr}/{np.dtype(dtype).name}"
                obs, _ = w.reset(seed=ac.TRAJ_SEED)
                rec = {k: [] for k in ("obs", "rewards", "terminations", "truncations")}
                rec["obs"].append(obs.copy())
                for a in ac.trajectory_actions(env_name, dtype):
                    o, r, te, tr_, _ = w.step(a.copy())
                    for k, v in zip(rec, (o, r, te, tr_)):
                        rec[k].append(np.array(v))
                out[f"{key}/obs"], out[f"{key}/rewards"] = np.stack(rec["obs"]), np.stack(rec["rewards"])
                out[f"{key}/flags"] = np.stack([np.stack(rec["terminations"]), np.stack(rec["truncations"])])
                w.close()
    # (c)
    for name in ac.SAMPLE_BOXES:
        for tr in ("clip", "rescale01"):
            env = spaces_only(spaces, batch_space, ac.make_box(spaces, name), ac.SAMPLE_N)
            w = ac.build(ref, env, tr)
            w.action_space.seed(ac.SAMPLE_SEED)
            out[f"c/{name}/{tr}/samples"] = np.stack([w.action_space.sample() for _ in range(ac.SAMPLE_BATCHES)])
    out["errors"] = np.array(sorted(f"{k}={v}" for k, v in errors.items()))
    path = os.path.join(HERE, "action_wrappers.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    print(*out["errors"], sep="\n")


if __name__ == "__main__":
    main()
