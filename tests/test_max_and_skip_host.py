"""CPU side of wrappers.MaxAndSkipObservation: the reference's constructor validation, the placement rules and refusals, what the class hands to the
engine, the layers above accepting it, and the fixtures -- their coverage claims re-checked from the files alone, the buffer rule restated in NumPy
over the recorded inner observations, and (where the reference tree exists) the generator reproducing its files.  What the wrapper computes is a GPU
matter (tests/test_gpu_max_and_skip.py): the checker backend has no mi_set_max_and_skip, and these tests pin that the host class says so instead of
stepping unwrapped."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import error
from gymnasium_amd.wrappers import per_env
from conftest import GOLDEN, REFERENCE, ROOT, golden

KEYS = ("cartpole", "pendulum", "acrobot", "mountaincar", "mountaincar_continuous")
IDS = ("CartPole-v1", "Pendulum-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0")
# run -> skip, of the runs that keep their inner observations (the FrameStack run does not)
PLAIN_RUNS = {"s4_11_next": 4, "s4_11_same": 4, "s4_9_next": 4, "s4_9_same": 4, "s2_5_next": 2, "s4_3_next": 4, "s4_11_disabled": 4,
              "sticky_s4_11_next": 4}


def make(env_id, factory, **kw):
    return gymnasium_amd.make_vec(env_id, num_envs=4, _engine_factory=factory, **kw)


class _Switch:
    """Stands in for the engine's entry points: records what the host classes hand to mi_set_max_and_skip / mi_set_step_wrappers."""

    def __init__(self, monkeypatch, env):
        self.skips, self.calls = [], []
        monkeypatch.setattr(env._engine.lib, "set_max_and_skip", True, raising=False)
        monkeypatch.setattr(env._engine, "set_max_and_skip", lambda *a: self.skips.append(a), raising=False)
        monkeypatch.setattr(env._engine.lib, "set_step_wrappers", True, raising=False)
        monkeypatch.setattr(env._engine, "set_step_wrappers", lambda *a: self.calls.append(a), raising=False)


# -- constructor validation: the reference's exception types and messages (stateful_observation.py:607-614) -----------------------------------------
def test_validates_like_the_reference(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    sw = _Switch(monkeypatch, env)
    for bad in (4.0, "4", None):
        with pytest.raises(TypeError, match="The skip is expected to be an integer, actual type"):
            wrappers.MaxAndSkipObservation(env, bad)
    for bad in (1, 0, -3, np.int64(1)):
        with pytest.raises(ValueError, match="The skip value needs to be equal or greater than two, actual value"):
            wrappers.MaxAndSkipObservation(env, bad)
    assert sw.skips == [] and env._max_and_skip == 0
    env.close()


def test_hands_the_skip_to_the_engine_and_leaves_the_step_wrappers_alone(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    sw = _Switch(monkeypatch, env)
    space = env.single_observation_space
    w = wrappers.MaxAndSkipObservation(env)  # the reference's default
    assert w.skip == 4 and sw.skips == [(4,)] and env._max_and_skip == 4
    assert env._step_wrappers == (0, 0.0, 0) and sw.calls == []
    assert w.single_observation_space == space and w.unwrapped is env and not env._can_fuse()
    env.set_max_and_skip()
    assert sw.skips[-1] == (0,) and env._max_and_skip == 0
    w = wrappers.MaxAndSkipObservation(env, np.int64(2))
    assert sw.skips[-1] == (2,) and env._max_and_skip == 2 and env._step_wrappers == (0, 0.0, 0)
    env.close()


# -- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_an_engine_without_the_entry_point_is_refused(oracle_factory):
    for name in ("set_max_and_skip", "get_max_and_skip_frames"):
        assert name in _native.HOST_SYMBOLS and name not in _native.SYMBOLS  # (the checker library does not have them)
    for env_id in IDS:
        env = make(env_id, oracle_factory)
        with pytest.raises(TypeError):  # the arguments are validated first
            wrappers.MaxAndSkipObservation(env, 2.5)
        with pytest.raises(error.Error, match="mi_set_max_and_skip"):
            wrappers.MaxAndSkipObservation(env, 4)
        with pytest.raises(error.Error, match="mi_set_max_and_skip"):
            env.set_max_and_skip(4)
        with pytest.raises(error.Error):
            env.max_and_skip_frames()
        assert env._max_and_skip == 0 and env._step_wrappers == (0, 0.0, 0)
        env.close()


@pytest.mark.parametrize("env_id,kw,why", [("HalfCheetah-v5", {}, "MuJoCo and ToyText"), ("FrozenLake-v1", {}, "MuJoCo and ToyText"),
                                           ("Blackjack-v1", {}, "MuJoCo and ToyText"), ("CartPole-v1", {"rng": "shared"}, "rng='shared'"),
                                           ("Pendulum-v1", {"fast_math": True}, "fast_math")])
def test_kinds_and_modes_without_the_wrapper(oracle_factory, env_id, kw, why):
    env = make(env_id, oracle_factory, **kw)
    for build in (lambda: wrappers.MaxAndSkipObservation(env, 4), lambda: env.set_max_and_skip(4)):
        with pytest.raises(error.Error, match=why):
            build()
    assert env._max_and_skip == 0
    env.close()


# -- placement ------------------------------------------------------------------------------------------------------------------------------------
def test_repeat_action_neither_over_nor_under_it(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    sw = _Switch(monkeypatch, env)
    m = wrappers.MaxAndSkipObservation(env, 4)
    with pytest.raises(error.Error, match="fold the repeat into"):
        wrappers.RepeatAction(m, 2)
    with pytest.raises(error.Error, match="fold the repeat into"):
        env.set_step_wrappers(2, 0.0, 0)
    with pytest.raises(error.Error):  # a second one
        wrappers.MaxAndSkipObservation(m, 2)
    assert sw.calls == [] and sw.skips == [(4,)]
    env.set_max_and_skip()
    r = wrappers.RepeatAction(env, 3)
    with pytest.raises(error.Error, match="fold the repeat into"):
        wrappers.MaxAndSkipObservation(r, 4)
    with pytest.raises(error.Error, match="fold the repeat into"):
        env.set_max_and_skip(4)
    assert env._max_and_skip == 0 and env._step_wrappers == (3, 0.0, 0)
    env.close()


def test_sticky_action_goes_over_it_not_under(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    sw = _Switch(monkeypatch, env)
    m = wrappers.MaxAndSkipObservation(env, 4)
    s = wrappers.StickyAction(m, 0.25, 3)  # one decision per outer step: no repeat is handed over, the skip stays
    assert sw.calls == [(0, 0.25, 3)] and env._step_wrappers == (0, 0.25, 3) and env._max_and_skip == 4 and s.unwrapped is env
    with pytest.raises(error.Error, match="fold the repeat into"):
        wrappers.RepeatAction(m, 2)
    env.close()
    env = make("CartPole-v1", oracle_factory)
    _Switch(monkeypatch, env)
    with pytest.raises(error.Error, match="directly over"):
        wrappers.MaxAndSkipObservation(wrappers.StickyAction(env, 0.25), 4)
    env.close()


def test_not_over_another_wrapper(oracle_factory, monkeypatch):
    env = make("Pendulum-v1", oracle_factory)
    _Switch(monkeypatch, env)
    for over in (wrappers.ClipAction(env), wrappers.RecordEpisodeStatistics(env)):
        with pytest.raises(error.Error, match="directly over"):
            wrappers.MaxAndSkipObservation(over, 4)
    assert env._max_and_skip == 0
    env.close()


def test_the_layers_above_accept_it(oracle_factory, monkeypatch):
    # (lets the per_env normalisers be constructed over the checker backend: nothing here reaches their statistics)
    monkeypatch.setattr(per_env, "_require_device_engine", lambda base, what: None)

    def base(env_id="Pendulum-v1"):
        env = make(env_id, oracle_factory)
        _Switch(monkeypatch, env)
        return env, wrappers.MaxAndSkipObservation(env, 4)

    for build in (lambda m: per_env.NormalizeObservation(m), lambda m: per_env.NormalizeReward(m), lambda m: per_env.FrameStackObservation(m, 4),
                  lambda m: per_env.DelayObservation(m, 2), lambda m: per_env.TimeAwareObservation(m),
                  lambda m: per_env.NormalizeReward(per_env.NormalizeObservation(wrappers.StickyAction(m, 0.5))),
                  lambda m: per_env.FrameStackObservation(per_env.NormalizeObservation(m), 4),
                  lambda m: wrappers.DiscretizeObservation(m, 5), lambda m: wrappers.DiscretizeAction(m, 5),
                  lambda m: wrappers.ClipAction(m), lambda m: wrappers.RecordEpisodeStatistics(m), lambda m: wrappers.ClipReward(m, -1.0, 1.0),
                  lambda m: wrappers.RecordEpisodeStatistics(wrappers.ClipAction(per_env.TimeAwareObservation(m)))):
        env, m = base()
        top = build(m)
        assert top.unwrapped is env and env._max_and_skip == 4
        env.close()


# -- the fixtures ---------------------------------------------------------------------------------------------------------------------------------
def _frames_of(g, gi, run, skip):
    """The buffer rule restated (stateful_observation.py:638-647) over the recorded inner observations of one run: yields, per step, the rows that
    stepped, how many slots each wrote and what the wrapper returns for them; returns nothing else -- the caller reads `frames` from the state."""
    inner, seen = g[f"{run}_inner"].astype(np.int64), gi[f"{run}_inner_obs"]
    frames = np.zeros((2,) + seen.shape[1:2] + seen.shape[3:], np.float32)  # np.zeros((2, *shape)) per sub-environment, never cleared
    for t in range(inner.shape[0]):
        w0, w1 = inner[t] >= skip - 1, inner[t] >= skip  # inner step skip - 2 / skip - 1 was reached
        frames[0][w0], frames[1][w1] = seen[t, :, 0][w0], seen[t, :, 1][w1]
        yield t, inner[t] > 0, w0.astype(np.int64) + w1, np.max(frames, axis=0), frames


@pytest.mark.parametrize("key", KEYS)
def test_the_buffer_rule_restated_reproduces_the_recorded_observations(key):
    g, gi = golden(f"max_and_skip_{key}.npz"), golden(f"max_and_skip_{key}_inner.npz")
    runs = dict(PLAIN_RUNS, **({"s4_default_next": 4} if key == "cartpole" else {}))
    for run, skip in runs.items():
        frames = None
        for t, stepped, _, mx, frames in _frames_of(g, gi, run, skip):
            returned = g[f"{run}_obs"][t].copy()
            if f"{run}_final_mask" in g.files:  # SAME_STEP: the row that finished returns the max frame as final_obs
                fm = g[f"{run}_final_mask"][t]
                returned[fm] = g[f"{run}_final_obs"][t][fm]
            assert np.array_equal(returned[stepped], mx[stepped]), (key, run, t)
        assert np.array_equal(frames, g[f"{run}_frames"]), (key, run, "the wrappers' _obs_buffer at the end")


@pytest.mark.parametrize("key", KEYS)
def test_the_fixtures_hold_the_coverage_they_exist_for(key):
    g, gi = golden(f"max_and_skip_{key}.npz"), golden(f"max_and_skip_{key}_inner.npz")
    runs = dict(PLAIN_RUNS, **({"s4_default_next": 4} if key == "cartpole" else {}))
    for run, skip in runs.items():
        both_stale = one_stale = differs_from_last = stale_decides = 0
        inner, seen = g[f"{run}_inner"].astype(np.int64), gi[f"{run}_inner_obs"]
        assert g[f"{run}_obs"].shape[1] == 96 and g[f"{run}_frames"].shape == (2, 96, seen.shape[-1]) and g[f"{run}_frames"].dtype == np.float32
        for t, stepped, wrote, mx, _ in _frames_of(g, gi, run, skip):
            both_stale += int((stepped & (wrote == 0)).sum())
            one_stale += int((stepped & (wrote == 1)).sum())
            last = np.where((wrote == 2)[:, None], seen[t, :, 1], seen[t, :, 0])  # the last inner observation, where the step wrote a slot
            differs_from_last += int((stepped & (wrote > 0) & (mx != last).any(axis=1)).sum())
            alone = np.where((wrote == 2)[:, None], np.maximum(seen[t, :, 0], seen[t, :, 1]), seen[t, :, 0])
            stale_decides += int((stepped & ((wrote == 0) | (mx != alone).any(axis=1))).sum())
        if "_9_" in run:
            assert both_stale > 0, (key, run, "(a)")
        if "_11_" in run or run.startswith("s2_5"):
            assert one_stale > 0 and differs_from_last > 0 and stale_decides > 0, (key, run, "(b) (c) (d)", one_stale, differs_from_last, stale_decides)
        if run == "s4_3_next":  # (e) no step ever reaches inner step skip - 1: slot 1 is the constructor's zeros, from the first step to the last
            assert int(inner.max()) == 3 and not g[f"{run}_frames"][1].any() and g[f"{run}_frames"][0].any(), (key, "(e)")
        if run == "s4_default_next":  # (f)
            assert int((g[f"{run}_term"] & (inner >= 1) & (inner - 1 < skip - 2)).sum()) > 0, (key, "(f)")
    # teacher rows: fresh wrappers, and where the id can terminate 48 rows that end after 1 .. 3 inner steps
    assert g["teacher_state"].shape[0] == 64 and g["teacher_frames"].shape[:2] == (2, 64)
    assert key == "pendulum" or int((g["teacher_term"] & (g["teacher_inner"] < 4)).sum()) == 48
    early = g["teacher_inner"] < 3
    assert not g["teacher_frames"][:, early].any() and not g["teacher_obs"][early].any(), (key, "no slot written: the constructor's zeros come back")
    # the FrameStack run keeps its stack axis
    assert g["stack_s4_11_next_obs"].shape[1:3] == (96, 4)


def test_generator_regenerates_its_files_bit_for_bit(tmp_path):
    if not os.path.isdir(os.path.join(REFERENCE, "gymnasium")):
        pytest.skip("the reference tree is not on this machine: the fixtures were recorded where it is")
    script = os.path.join(GOLDEN, "make_golden_max_and_skip.py")
    env = dict(os.environ, GYM_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, script, str(tmp_path)], check=True, cwd=ROOT, env=env, capture_output=True)
    names = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert names == sorted([f"max_and_skip_{k}.npz" for k in KEYS] + [f"max_and_skip_{k}_inner.npz" for k in KEYS])
    for name in names:
        assert os.path.getsize(tmp_path / name) < 1 << 20
        with open(tmp_path / name, "rb") as a, open(os.path.join(GOLDEN, name), "rb") as b:
            assert a.read() == b.read(), name
