#!/usr/bin/env python3
"""Fixtures of FrameStackObservation / DelayObservation / TimeAwareObservation around every SCALAR env of a vector env, recorded FROM THE REFERENCE
ITSELF.

Run in the build container only (the reference does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stateful_observation.py [output directory [<id>_<mode> ...]]

It imports gymnasium from the reference tree (GYM_REFERENCE, default /root/reference; NumPy >= 2) and writes stateful_observation_<id>_<mode>.npz for
CartPole-v1 (D = 4), Pendulum-v1 (3) and MountainCar-v0 (2) under NEXT_STEP, SAME_STEP and DISABLED: SyncVectorEnv over 70 scalar envs -- a wavefront
and a partial one --, reset(seed=3), 40 steps of action_space.sample() from action_space.seed(1); DISABLED with a masked reset of the rows that ended
after every step that ended some.  Every file holds the UNWRAPPED run once

  obs0 [N, D]; actions [T, N]; obs [T, N, D]; term / trunc [T, N]; SAME_STEP: final_obs [T, N, D] (zero outside final_mask [T, N]);
  DISABLED: reset_mask [T, N], reset_obs [T, N, D] (the FULL batch reset() returned; zero in a step without a reset)

and, for every configuration C of tests/stateful_observation_cases.py CONFIGS (the same seeds give the same trajectory, which the script checks), what
the wrapped envs returned: C__obs0, C__obs, C__final_obs, C__reset_obs, and the single observation space as C__low / C__high (their dtype and shape
are the space's).  The Dict configuration (flatten=False) stores its "time" entries as C__obs0 ... and the two spaces as C__low / C__high ("obs") and
C__time_low / C__time_high; its "obs" entries are asserted to equal the unwrapped ones.

max_episode_steps (cases.LIMITS) keeps resets dense, and the script ASSERTS what the fixtures exist for:
  * pendulum (limit 2), every mode: episodes with fewer observations than the largest stack (4) holds -- the reset observation and two steps -- so
    every stack of 4 looks across a reset; under SAME_STEP and DISABLED two resets of a row lie 2 steps apart, under NEXT_STEP (whose reset takes a
    step of its own) 3;
  * mountaincar (limit 3), every mode: episodes of exactly 4 observations;
  * cartpole (limit 14), every mode: terminations that are not truncations, and truncations.
  One limit per vector env cannot give both short episodes and terminations: Pendulum never terminates, MountainCar cannot reach its goal within 40
  steps, and a CartPole does not fall within 2.
Everything is a function of the fixed seeds: a second run writes the same arrays bit for bit.
"""
import os
import sys
import zipfile

REF = os.environ.get("GYM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

import gymnasium as gym  # noqa: E402
from gymnasium.vector import AutoresetMode, SyncVectorEnv  # noqa: E402
from gymnasium.wrappers import DelayObservation, FrameStackObservation, NormalizeObservation, TimeAwareObservation  # noqa: E402

import stateful_observation_cases as cases  # noqa: E402

assert int(np.__version__.split(".")[0]) >= 2, "the fixtures must be generated with NumPy >= 2"
OUT = os.path.dirname(os.path.abspath(__file__))
N, T, SEED, ASEED = cases.N, cases.T, cases.SEED, cases.ASEED
MODES = {"next": AutoresetMode.NEXT_STEP, "same": AutoresetMode.SAME_STEP, "disabled": AutoresetMode.DISABLED}
LIMIT_BYTES = 280_766  # the largest per_env_normalize_*.npz


def wrap(env, key, layers):
    for kind, kw in layers:
        if kind == "stack":
            padding = cases.CUSTOM[key] if kw["padding"] == "custom" else kw["padding"]
            env = FrameStackObservation(env, kw["k"], padding_type=padding)
        elif kind == "delay":
            env = DelayObservation(env, kw["delay"])
        elif kind == "time":
            env = TimeAwareObservation(env, flatten=kw["flatten"], normalize_time=kw["normalize_time"])
        else:
            env = NormalizeObservation(env)
    return env


def run(key, mode_name, layers):
    """One run of the vector env; layers = [] is the unwrapped one."""
    mode = MODES[mode_name]
    env_id, limit = cases.IDS[key], cases.LIMITS[key]
    vec = SyncVectorEnv([lambda: wrap(gym.make(env_id, max_episode_steps=limit), key, layers)] * N, autoreset_mode=mode)
    is_dict = isinstance(vec.single_observation_space, gym.spaces.Dict)
    part = (lambda o: o["time"]) if is_dict else (lambda o: o)
    obs0, _ = vec.reset(seed=SEED)
    vec.action_space.seed(ASEED)
    out = dict(obs0=part(obs0).copy(), actions=[], obs=[], term=[], trunc=[], final_obs=[], final_mask=[], reset_mask=[], reset_obs=[])
    inner = dict(obs0=obs0["obs"].copy(), obs=[], final_obs=[], reset_obs=[]) if is_dict else None
    for t in range(T):
        a = vec.action_space.sample()
        o, r, te, tr, info = vec.step(a)
        done = te | tr
        out["actions"].append(a), out["obs"].append(part(o).copy()), out["term"].append(te.copy()), out["trunc"].append(tr.copy())
        if is_dict:
            inner["obs"].append(o["obs"].copy())
        if mode == AutoresetMode.SAME_STEP:
            fo, fm = np.zeros_like(part(o)), np.zeros(N, dtype=bool)
            fo_inner = np.zeros_like(o["obs"]) if is_dict else None
            if "final_obs" in info:
                fm = info["_final_obs"].copy()
                for i in np.flatnonzero(fm):
                    fo[i] = part(info["final_obs"][i])
                    if is_dict:
                        fo_inner[i] = info["final_obs"][i]["obs"]
            assert np.array_equal(fm, done)
            out["final_obs"].append(fo), out["final_mask"].append(fm)
            if is_dict:
                inner["final_obs"].append(fo_inner)
        if mode == AutoresetMode.DISABLED:
            rso = np.zeros_like(part(o))
            rso_inner = np.zeros_like(o["obs"]) if is_dict else None
            if done.any():
                ro, _ = vec.reset(options={"reset_mask": done.copy()})
                rso = part(ro).copy()
                assert np.array_equal(rso[~done], part(o)[~done]), "rows outside the mask keep the observation they returned last"
                if is_dict:
                    rso_inner = ro["obs"].copy()
            out["reset_mask"].append(done.copy()), out["reset_obs"].append(rso)
            if is_dict:
                inner["reset_obs"].append(rso_inner)
    space = vec.single_observation_space
    vec.close()
    for d in (out, inner):
        for k in list(d or ()):
            if isinstance(d[k], list):
                if d[k]:
                    d[k] = np.stack(d[k])
                else:
                    del d[k]
    return out, inner, space


def episode_lengths(term, trunc, mode):
    """The lengths (in env steps) of the episodes that began and ended inside the recording, all rows."""
    done, lengths = term | trunc, []
    for n in range(N):
        length = 0  # (every row starts an episode with reset(seed=...))
        for t in range(T):
            if mode == "next" and t > 0 and done[t - 1, n]:
                length = 0  # the autoreset step: no env step
                continue
            length += 1
            if done[t, n]:
                lengths.append(length)
                length = 0
    return np.array(lengths)


def save(out_dir, name, **arrs):
    """One .npz with ONE LZMA-compressed member beside its directory (cases.pack): the ~25 outputs of a file are shifted, padded and widened copies of
    one trajectory, which a compressor sees only when they share a stream and its dictionary spans them (deflate's 32 KiB window does not span one
    array; member by member the files would be 0.4 - 1.2 MiB)."""
    path = os.path.join(out_dir, name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for member, arr in cases.pack(arrs).items():
            with z.open(member + ".npy", "w", force_zip64=True) as f:
                np.lib.format.write_array(f, arr, allow_pickle=False)
    back = cases.load(path)
    assert list(back) == list(arrs) and all(back[k].dtype == v.dtype and back[k].shape == v.shape and back[k].tobytes() == v.tobytes() for k, v in arrs.items())
    size = os.path.getsize(path)
    assert size <= LIMIT_BYTES, f"{name}: {size} bytes"
    print(f"{name}: {size / 1024:.1f} KiB")


def main(out_dir=OUT, only=()):
    for key in cases.IDS:
        for mode in cases.MODES:
            if only and f"{key}_{mode}" not in only:
                continue
            raw, _, raw_space = run(key, mode, [])
            lengths = episode_lengths(raw["term"], raw["trunc"], mode)
            cover = dict(terminations=int((raw["term"] & ~raw["trunc"]).sum()), truncations=int(raw["trunc"].sum()), shortest=int(lengths.min()),
                         longest=int(lengths.max()))
            print(f"  {key} {mode}: {cover}")
            if key == "pendulum":
                assert cover["longest"] + 1 < cases.KMAX and len(lengths) >= 5 * N, cover
            if key == "mountaincar":
                assert cover["shortest"] + 1 == cases.KMAX == cover["longest"] + 1, cover
            if key == "cartpole":
                assert cover["terminations"] >= 1 and cover["truncations"] >= 1, cover
            assert raw["obs"].dtype == np.float32 and raw["obs"].shape == (T, N) + raw_space.shape
            arrs = dict(raw)
            for name, layers in cases.CONFIGS.items():
                got, inner, space = run(key, mode, layers)
                for k in ("actions", "term", "trunc"):
                    assert np.array_equal(got[k], raw[k]), (name, k)
                for k in ("obs0", "obs", "final_obs", "reset_obs"):
                    if k in got:
                        arrs[f"{name}__{k}"] = got[k]
                        if inner is not None:
                            assert np.array_equal(inner[k], raw[k]), (name, k, "the Dict's obs entries are the unwrapped observations")
                if inner is not None:
                    arrs[f"{name}__low"], arrs[f"{name}__high"] = space["obs"].low, space["obs"].high
                    arrs[f"{name}__time_low"], arrs[f"{name}__time_high"] = space["time"].low, space["time"].high
                else:
                    arrs[f"{name}__low"], arrs[f"{name}__high"] = space.low, space.high
                    assert got["obs"].dtype == space.dtype and got["obs"].shape == (T, N) + space.shape, (name, got["obs"].dtype, got["obs"].shape, space)
            save(out_dir, f"stateful_observation_{key}_{mode}.npz", **arrs)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT, sys.argv[2:])
