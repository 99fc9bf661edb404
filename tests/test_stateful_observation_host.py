"""CPU side of wrappers.per_env.FrameStackObservation / DelayObservation / TimeAwareObservation: the NumPy restatement reproduces the fixtures recorded
from the reference bit for bit; the index arithmetic of the kernels (csrc/stateful_observation_internal.h), compiled for the host into a stand-alone
program, takes the restatement's decisions on the fixtures' flag patterns; the constructors validate like the reference, build the reference's spaces
and refuse what is documented; the fixture generator reproduces its files.  What the kernels compute is a GPU matter
(tests/test_gpu_stateful_observation.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import AutoresetMode, error, spaces
from gymnasium_amd.wrappers import per_env
from conftest import GOLDEN, REFERENCE, ROOT

import stateful_observation_cases as cases

KEYS = [f"{k}_{m}" for k in cases.IDS for m in cases.MODES]
FILES = sorted(f"stateful_observation_{k}.npz" for k in KEYS)
LARGEST_NORMALIZE_FIXTURE = 280_766  # bytes: the size the new files stay within


def layers_of(key, name, dim):
    return cases.build(cases.CONFIGS[name], cases.N, (dim,), np.float32, cases.LIMITS[key], cases.CUSTOM[key])


# -- 1. the restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
def test_restatement_reproduces_the_reference(key):
    fix = cases.fixture(key)
    env_key, mode = key.rsplit("_", 1)
    assert fix["obs"].shape[:2] == (cases.T, cases.N) and fix["obs"].dtype == np.float32
    for name in cases.CONFIGS:
        got = cases.replay(fix, mode, layers_of(env_key, name, fix["obs"].shape[-1]))
        compared = 0
        for k in ("obs0", "obs", "final_obs", "reset_obs"):
            if f"{name}__{k}" in fix:
                want = fix[f"{name}__{k}"]
                assert got[k].dtype == want.dtype and got[k].shape == want.shape and np.array_equal(got[k], want), (name, k)
                compared += 1
        assert compared == (2 if mode == "next" else 3), name


def test_fixture_coverage():
    for key in KEYS:
        fix, (env_key, mode) = cases.fixture(key), key.rsplit("_", 1)
        assert os.path.getsize(os.path.join(GOLDEN, f"stateful_observation_{key}.npz")) <= LARGEST_NORMALIZE_FIXTURE, key
        done = fix["term"] | fix["trunc"]
        if env_key == "cartpole":
            assert (fix["term"] & ~fix["trunc"]).any() and fix["trunc"].any()
        if env_key == "pendulum":  # 3 observations per episode: every stack of 4 looks across a reset
            assert done.sum() >= 5 * cases.N and cases.LIMITS[env_key] + 1 < cases.KMAX
        if mode == "same":
            assert np.array_equal(fix["final_mask"], done)
        if mode == "disabled":
            assert np.array_equal(fix["reset_mask"], done)
    # a stack that holds an episode's frames, the padding of its reset AND a frame of the episode before never occurs; one that holds two
    # resets' paddings cannot either (a reset overwrites the whole stack) -- but a window of 4 steps with two resets in it does: pendulum, NEXT_STEP
    done = cases.fixture("pendulum_next")["term"] | cases.fixture("pendulum_next")["trunc"]
    assert (done[:-3] & done[3:]).any()


# -- 2. the index arithmetic on the host ------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "stateful_observation_internal.h"
using namespace mi_stateful;

static int code(Slot s) {
    switch (s.source) {
    case SRC_TRAJECTORY: case SRC_RESET_OBS: return s.index + 1;
    case SRC_CARRIED: return -(s.index + 1);
    case SRC_CUSTOM: return 1000000;
    default: return 0;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) return 3;
    int T, N, k, delay, padding, next_step, max_timesteps;
    if (fscanf(in, "%d %d %d %d %d %d %d", &T, &N, &k, &delay, &padding, &next_step, &max_timesteps) != 7) return 4;
    std::vector<int> pending(N), count(N), time(N), done((size_t)T * N);
    for (auto *v : {&pending, &count, &time, &done})
        for (auto &x : *v)
            if (fscanf(in, "%d", &x) != 1) return 5;
    for (int n = 0; n < N; n++) {
        auto fin = [&](int s) { return done[(size_t)s * N + n] != 0; };
        for (int t = 0; t < T; t++) {  // FrameStack: T * k codes
            const int r = latest_reset(t - (k - 1), t, next_step != 0, pending[n] != 0, fin);
            for (int j = 0; j < k; j++) fprintf(out, "%d ", code(frame_stack_slot(k, padding, t, j, r)));
        }
        for (int t = 0; t < T; t++)  // Delay: T codes, then the new history and count
            fprintf(out, "%d ", code(delay_slot(delay, t, latest_reset(t - delay + 1, t, next_step != 0, pending[n] != 0, fin), count[n])));
        for (int j = 0; j < delay; j++) fprintf(out, "%d ", code(delay_history_slot(delay, T, j)));
        fprintf(out, "%d ", delay_count(delay, T, latest_reset(T - delay + 1, T - 1, next_step != 0, pending[n] != 0, fin), count[n]));
        int tm = time[n];
        bool p = pending[n] != 0;
        for (int t = 0; t < T; t++) {  // TimeAware: T times and the bits of T normalised times
            tm = time_after(tm, next_step && p);
            p = fin(t);
            const float f = time_normalized(tm, max_timesteps);
            uint32_t bits;
            memcpy(&bits, &f, 4);
            fprintf(out, "%d %u ", tm, bits);
        }
        fprintf(out, "\n");
    }
    fclose(out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_program(tmp_path_factory):
    cxx = shutil.which("g++") or (os.environ.get("HIPCC", "/opt/rocm/bin/hipcc") if os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) else None)
    if cxx is None:
        pytest.skip("no C++ compiler to build the index arithmetic for the host with")
    d = tmp_path_factory.mktemp("stateful_observation_header")
    src = d / "program.cpp"
    src.write_text(PROGRAM)
    cmd = [cxx] + ([] if cxx.endswith("g++") else ["-x", "c++"]) + ["-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "gymnasium_amd", "csrc"), "-o",
                                                                   str(d / "program"), str(src)]
    subprocess.run(cmd, check=True)
    return str(d / "program"), d


def restated_decisions(done, next_step, pending, count, time, k, delay, padding, max_timesteps):
    """The same rollout through the restatement, fed observations whose VALUE names their source: step s is s + 1, slot i of the carried state is
    -(i + 1), the custom padding is 1e6."""
    steps, n = done.shape
    mode = "next" if next_step else "disabled"
    obs = np.broadcast_to(np.arange(1, steps + 1, dtype=np.float64)[:, None, None], (steps, n, 1))
    nothing = np.zeros_like(done)
    out = {}
    stack = cases.FrameStack(n, (1,), np.float64, k, ("reset", "zero", "custom")[padding], custom=[1e6])
    stack.stack[:] = -np.arange(1, k + 1, dtype=np.float64)[None, :, None]
    s = cases.Stack([stack], mode)
    s.pending = pending.copy()
    out["stack"] = cases.rollout(s, obs, done, nothing)[..., 0].transpose(1, 0, 2).astype(np.int64)  # [N, T, k]
    queue = cases.Delay(n, (1,), np.float64, delay)
    queue.queue[:, 1:] = -np.arange(1, delay + 1, dtype=np.float64)[None, :, None]
    queue.length[:] = count
    s = cases.Stack([queue], mode)
    s.pending = pending.copy()
    out["delay"] = cases.rollout(s, obs, done, nothing)[..., 0].T.astype(np.int64)  # [N, T]
    out["history"], out["count"] = queue.queue[:, 1:, 0].astype(np.int64), queue.length.copy()
    for normalize in (False, True):
        clock = cases.TimeAware(n, (1,), np.float32, max_timesteps, True, normalize)
        clock.timesteps[:] = time
        s = cases.Stack([clock], mode)
        s.pending = pending.copy()
        got = cases.rollout(s, obs.astype(np.float32), done, nothing)[..., -1].T
        out["normalized" if normalize else "time"] = got.astype(np.float32).view(np.uint32).astype(np.int64) if normalize else got.astype(np.int64)
    return out


@pytest.mark.parametrize("key", [f"{k}_{m}" for k in cases.IDS for m in ("next", "disabled")])
@pytest.mark.parametrize("k,delay,padding", [(1, 0, 0), (3, 1, 1), (4, 3, 2), (4, 5, 0)])
def test_header_decisions_equal_the_restatement(header_program, key, k, delay, padding):
    program, d = header_program
    fix = cases.fixture(key)
    env_key, mode = key.rsplit("_", 1)
    done = fix["term"] | fix["trunc"]
    steps, n = done.shape
    rng = np.random.default_rng(k * 100 + delay)
    next_step = mode == "next"
    pending = rng.random(n) < 0.3 if next_step else np.zeros(n, dtype=bool)
    count, time = rng.integers(0, delay + 1, n), rng.integers(0, 50, n)
    max_timesteps = cases.LIMITS[env_key] + 5  # (a denominator that does not divide most counters)
    want = restated_decisions(done, next_step, pending, count, time, k, delay, padding, max_timesteps)
    path_in, path_out = d / f"{key}_{k}_{delay}.in", d / f"{key}_{k}_{delay}.out"
    with open(path_in, "w") as f:
        f.write(f"{steps} {n} {k} {delay} {padding} {int(next_step)} {max_timesteps}\n")
        for v in (pending.astype(int), count, time, done.astype(int).reshape(-1)):
            f.write(" ".join(map(str, v.tolist())) + "\n")
    subprocess.run([program, str(path_in), str(path_out)], check=True)
    rows = np.loadtxt(path_out, dtype=np.int64, ndmin=2)
    assert rows.shape == (n, steps * k + steps + delay + 1 + 2 * steps)
    at = 0
    got_stack, at = rows[:, at:at + steps * k].reshape(n, steps, k), at + steps * k
    got_delay, at = rows[:, at:at + steps], at + steps
    got_history, at = rows[:, at:at + delay], at + delay
    got_count, at = rows[:, at], at + 1
    clock = rows[:, at:].reshape(n, steps, 2)
    assert np.array_equal(got_stack, want["stack"])
    assert np.array_equal(got_delay, want["delay"])
    assert np.array_equal(got_count, want["count"])
    valid = np.arange(delay)[None, :] >= delay - got_count[:, None]  # the queue is the LAST count slots; the others are never read
    assert np.array_equal(got_history[valid], want["history"][valid])
    assert np.array_equal(clock[..., 0], want["time"]) and np.array_equal(clock[..., 1], want["normalized"])
    if next_step and k > 1:
        pad = got_stack[:, k:, 0] == got_stack[:, k:, -1] if padding == 0 else got_stack[:, k:, 0] == (0, 1000000)[padding - 1]
        assert (got_stack < 0).any() and pad.any()  # carried slots and paddings both occur


# -- 3. validation, spaces, refusals ------------------------------------------------------------------------------------------------------------------
def make(env_id, factory, **kw):
    return gymnasium_amd.make_vec(env_id, num_envs=4, _engine_factory=factory, **kw)


def test_constructors_validate_like_the_reference(oracle_factory):
    assert {"stateful_observation_step", "stateful_observation_steps"} <= set(_native.WRAPPER_SYMBOLS)
    assert not {"stateful_observation_step", "stateful_observation_steps"} & set(_native.SYMBOLS)
    env = make("CartPole-v1", oracle_factory)
    for bad in (2.0, "3", None):
        with pytest.raises(TypeError, match="The stack_size is expected to be an integer"):
            per_env.FrameStackObservation(env, bad)
        with pytest.raises(TypeError, match="The delay is expected to be an integer"):
            per_env.DelayObservation(env, bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="The stack_size needs to be greater than zero"):
            per_env.FrameStackObservation(env, bad)
    with pytest.raises(ValueError, match="The delay needs to be greater than zero"):
        per_env.DelayObservation(env, -1)
    with pytest.raises(ValueError, match="Unexpected `padding_type`, expected 'reset', 'zero' or a custom observation space, actual value: 'resett'"):
        per_env.FrameStackObservation(env, 2, padding_type="resett")
    for bad in (np.zeros(3, np.float32), np.array([9.0, 0.0, 0.0, 0.0], np.float32)):  # the wrong shape, outside the bounds
        with pytest.raises(ValueError, match="not an instance of env observation"):
            per_env.FrameStackObservation(env, 2, padding_type=bad)
    assert per_env.FrameStackObservation(env, np.int64(2)).stack_size == 2 and per_env.DelayObservation(env, np.int32(0)).delay == 0
    w = per_env.FrameStackObservation(env, 2, padding_type=np.array([1.0, -1.0, 0.0, 2.0], np.float32))
    assert w.padding_type == "_custom"
    env.close()


def test_time_aware_needs_a_time_limit(oracle_factory):
    env = make("CartPole-v1", oracle_factory)
    assert per_env.TimeAwareObservation(env).max_timesteps == 500
    env.max_episode_steps = None
    with pytest.raises(ValueError, match="The environment must be wrapped by a TimeLimit wrapper or the spec specify a `max_episode_steps`."):
        per_env.TimeAwareObservation(env)
    env.close()
    env = make("CartPole-v1", oracle_factory, max_episode_steps=7)
    assert per_env.TimeAwareObservation(env, dict_time_key="clock").max_timesteps == 7
    env.close()


def wrapped(env, key, layers):
    for kind, kw in layers:
        if kind == "stack":
            env = per_env.FrameStackObservation(env, kw["k"], padding_type=cases.CUSTOM[key] if kw["padding"] == "custom" else kw["padding"])
        elif kind == "delay":
            env = per_env.DelayObservation(env, kw["delay"])
        elif kind == "time":
            env = per_env.TimeAwareObservation(env, flatten=kw["flatten"], normalize_time=kw["normalize_time"])
        else:
            env = per_env.NormalizeObservation(env)
    return env


def same_box(space, low, high):
    return (isinstance(space, spaces.Box) and space.dtype == low.dtype and space.shape == low.shape and np.array_equal(space.low, low)
            and np.array_equal(space.high, high))


@pytest.mark.parametrize("key", list(cases.IDS))
def test_spaces_equal_the_recorded_ones(oracle_factory, monkeypatch, key):
    monkeypatch.setattr(per_env, "_require_device_engine", lambda base, what: None)  # (the normaliser under a stack: nothing here reaches its statistics)
    fix = cases.fixture(f"{key}_next")
    for name, layers in cases.CONFIGS.items():
        env = make(cases.IDS[key], oracle_factory, max_episode_steps=cases.LIMITS[key])
        w = wrapped(env, key, layers)
        single, batched = w.single_observation_space, w.observation_space
        if name == "time_dict":
            assert isinstance(single, spaces.Dict) and list(single.keys()) == ["obs", "time"]
            assert same_box(single["obs"], fix[f"{name}__low"], fix[f"{name}__high"]) and single["obs"] == env.single_observation_space
            assert same_box(single["time"], fix[f"{name}__time_low"], fix[f"{name}__time_high"])
            assert batched["time"].shape == (4, 1) and batched["time"].dtype == np.int32 and batched["obs"].shape == (4,) + single["obs"].shape
        else:
            low, high = fix[f"{name}__low"], fix[f"{name}__high"]
            assert same_box(single, low, high), name
            assert same_box(batched, np.broadcast_to(low, (4,) + low.shape), np.broadcast_to(high, (4,) + high.shape)), name
            assert fix[f"{name}__obs"].dtype == single.dtype and fix[f"{name}__obs"].shape[2:] == single.shape, name
        env.close()
    # the two the issue names: TimeAware over CartPole is a float64 Box of 5, FrameStack(2) over it (2, 5) float64
    if key == "cartpole":
        env = make("CartPole-v1", oracle_factory)
        t = per_env.TimeAwareObservation(env)
        s = per_env.FrameStackObservation(t, 2)
        assert (t.single_observation_space.shape, t.single_observation_space.dtype) == ((5,), np.float64) and t.single_observation_space.high[-1] == 500
        assert (s.single_observation_space.shape, s.single_observation_space.dtype) == ((2, 5), np.float64) and s.observation_space.shape == (4, 2, 5)
        n = per_env.TimeAwareObservation(make("CartPole-v1", oracle_factory), normalize_time=True)
        assert n.single_observation_space.dtype == np.float32 and n.single_observation_space.high[-1] == 1.0
        env.close()


@pytest.mark.parametrize("env_id", ["FrozenLake-v1", "Blackjack-v1"])
def test_discrete_and_tuple_observations_are_refused(oracle_factory, env_id):
    env = make(env_id, oracle_factory)
    for build in (lambda: per_env.FrameStackObservation(env, 2), lambda: per_env.DelayObservation(env, 1), lambda: per_env.TimeAwareObservation(env)):
        with pytest.raises(error.Error, match="float32 / float64 Box observations"):
            build()
    env.close()


def test_placement(oracle_factory, monkeypatch):
    monkeypatch.setattr(per_env, "_require_device_engine", lambda base, what: None)
    env = make("CartPole-v1", oracle_factory)
    # a Dict from flatten=False goes under neither FrameStack nor Delay
    d = per_env.TimeAwareObservation(env, flatten=False)
    for build in (lambda: per_env.FrameStackObservation(d, 2), lambda: per_env.DelayObservation(d, 1)):
        with pytest.raises(error.Error, match="float32 / float64 Box observations"):
            build()
    # over one another in any order, over the normalisers; every vector wrapper goes ABOVE them ...
    a = per_env.FrameStackObservation(per_env.TimeAwareObservation(per_env.DelayObservation(env, 1)), 3)
    b = per_env.DelayObservation(per_env.FrameStackObservation(per_env.NormalizeReward(per_env.NormalizeObservation(env)), 2), 2)
    assert a._base is env and b._base is env and b.single_observation_space.shape == (2, 4) and b.single_observation_space.dtype == np.float32
    top = wrappers.RecordEpisodeStatistics(wrappers.TransformReward(a, lambda r: r))
    assert top.unwrapped is env and not env._can_fuse()
    # ... never below
    for inner in (wrappers.RecordEpisodeStatistics(make("CartPole-v1", oracle_factory)), wrappers.ClipAction(make("Pendulum-v1", oracle_factory))):
        for build in (lambda: per_env.FrameStackObservation(inner, 2), lambda: per_env.DelayObservation(inner, 1), lambda: per_env.TimeAwareObservation(inner)):
            with pytest.raises(error.Error, match="below the vector level"):
                build()
    # the normalisers stay BELOW this family: their own placement check refuses the other order
    for cls in (per_env.NormalizeObservation, per_env.NormalizeReward):
        with pytest.raises(error.Error, match="directly over"):
            cls(per_env.DelayObservation(make("CartPole-v1", oracle_factory), 1))
    # RepeatAction / StickyAction are sub-environment wrappers too
    env3 = make("CartPole-v1", oracle_factory)
    monkeypatch.setattr(env3._engine.lib, "set_step_wrappers", True, raising=False)
    monkeypatch.setattr(env3._engine, "set_step_wrappers", lambda *a: None)
    assert per_env.TimeAwareObservation(wrappers.StickyAction(wrappers.RepeatAction(env3, 2), 0.25))._base is env3
    env.close(), env3.close()


def test_no_cpu_implementation_capture_and_same_step_rollouts(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory, autoreset_mode=AutoresetMode.SAME_STEP)
    for w in (per_env.FrameStackObservation(env, 2), per_env.DelayObservation(env, 1), per_env.TimeAwareObservation(env)):
        with pytest.raises(error.Error, match="capture_steps"):
            w.capture_steps(steps=2, policy="random")
        # the spaces above were built; the first call says that the state lives on the device
        for call in (lambda: w.reset(seed=1), lambda: w.step(np.zeros(4, np.int64)), lambda: w.rollout(3)):
            with pytest.raises(error.Error, match="needs the device engine"):
                call()
        monkeypatch.setattr(w, "_require", lambda: None)
        with pytest.raises(error.Error, match="SAME_STEP"):
            w.rollout(4)
    env.close()


# -- 4. the fixtures --------------------------------------------------------------------------------------------------------------------------------
def test_generator_regenerates_its_files_bit_for_bit(tmp_path):
    if not os.path.isdir(os.path.join(REFERENCE, "gymnasium")):
        pytest.skip("the reference tree is not on this machine: the fixtures were recorded where it is")
    script = os.path.join(GOLDEN, "make_golden_stateful_observation.py")
    env = dict(os.environ, GYM_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    some = ["cartpole_same", "pendulum_next", "mountaincar_disabled"]  # (every id and every mode once: the whole set takes half a minute)
    subprocess.run([sys.executable, script, str(tmp_path)] + some, check=True, cwd=ROOT, env=env, capture_output=True)
    names = sorted(f"stateful_observation_{k}.npz" for k in some)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz")) == names and set(names) <= set(FILES)
    for name in names:
        new, old = cases.load(tmp_path / name), cases.load(os.path.join(GOLDEN, name))
        assert list(new) == list(old), name
        for k in new:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)
