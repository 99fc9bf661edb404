"""CPU side of wrappers.RepeatAction / wrappers.StickyAction: the reference's constructor validation, the refusals, the stacking rules, and the fixture
generator reproducing its files.  What the wrappers compute is a GPU matter (tests/test_gpu_step_wrappers.py): the checker backend has no
mi_set_step_wrappers, and these tests pin that the host class says so instead of stepping unwrapped."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import error
from conftest import GOLDEN, REFERENCE, ROOT


def make(env_id, factory, **kw):
    return gymnasium_amd.make_vec(env_id, num_envs=4, _engine_factory=factory, **kw)


class _Switch:
    """Stands in for the engine's entry point: records what the host classes hand to mi_set_step_wrappers."""

    def __init__(self, monkeypatch, env):
        self.calls = []
        monkeypatch.setattr(env._engine.lib, "set_step_wrappers", True, raising=False)
        monkeypatch.setattr(env._engine, "set_step_wrappers", lambda *a: self.calls.append(a))


# -- constructor validation: the reference's exception types (stateful_action.py:47-106, 176-195) -------------------------------------------------
def test_repeat_action_validates_like_the_reference(oracle_factory):
    env = make("CartPole-v1", oracle_factory)
    for bad in (2.0, "4"):
        with pytest.raises(TypeError, match="expected to be an integer"):
            wrappers.RepeatAction(env, bad)
    for bad in (0, -3, np.int64(0)):
        with pytest.raises(ValueError, match="equal or greater than one"):
            wrappers.RepeatAction(env, bad)
    env.close()


def test_sticky_action_validates_like_the_reference(oracle_factory):
    env = make("CartPole-v1", oracle_factory)
    invalid_probability = getattr(error, "InvalidProbability")
    for bad in (1, 1.5, -0.1):
        with pytest.raises(invalid_probability):
            wrappers.StickyAction(env, bad)
    with pytest.raises(ValueError, match="either an integer or a tuple"):
        wrappers.StickyAction(env, 0.5, [1, 2])
    with pytest.raises(ValueError, match="two integers"):
        wrappers.StickyAction(env, 0.5, (1, 2, 3))
    with pytest.raises(error.InvalidBound):
        wrappers.StickyAction(env, 0.5, (3, 2))
    for bad in (0, (0, 2), -1):
        with pytest.raises(ValueError, match="larger or equal than 1"):
            wrappers.StickyAction(env, 0.5, bad)
    env.close()


def test_a_duration_range_is_refused_with_the_reason(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    sw = _Switch(monkeypatch, env)
    with pytest.raises(error.Error, match="32-bit half"):
        wrappers.StickyAction(env, 0.5, (1, 3))
    assert sw.calls == []
    w = wrappers.StickyAction(env, 0.5, (2, 2))  # not a range: Generator.integers(2, 3) consumes nothing
    assert sw.calls == [(0, 0.5, 2)] and w.repeat_action_duration_range == (2, 2)
    env.close()


def test_generator_integers_of_one_value_consumes_nothing():
    g = np.random.default_rng(5)
    before = g.bit_generator.state
    assert g.integers(3, 4) == 3 and g.bit_generator.state == before


# -- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_an_engine_without_the_entry_point_is_refused(oracle_factory):
    assert "set_step_wrappers" in _native.HOST_SYMBOLS and "set_step_wrappers" not in _native.SYMBOLS  # (the checker library does not have it)
    for env_id in ("CartPole-v1", "Pendulum-v1", "Acrobot-v1", "MountainCar-v0", "MountainCarContinuous-v0"):
        env = make(env_id, oracle_factory)
        with pytest.raises(error.Error, match="mi_set_step_wrappers"):
            wrappers.RepeatAction(env, 4)
        with pytest.raises(error.Error, match="mi_set_step_wrappers"):
            wrappers.StickyAction(env, 0.25)
        assert env._step_wrappers == (0, 0.0, 0)
        env.close()


@pytest.mark.parametrize("env_id,kw,why", [("HalfCheetah-v5", {}, "MuJoCo and ToyText"), ("FrozenLake-v1", {}, "MuJoCo and ToyText"),
                                           ("Blackjack-v1", {}, "MuJoCo and ToyText"), ("CartPole-v1", {"rng": "shared"}, "rng='shared'"),
                                           ("Pendulum-v1", {"fast_math": True}, "fast_math")])
def test_kinds_and_modes_without_the_wrappers(oracle_factory, env_id, kw, why):
    env = make(env_id, oracle_factory, **kw)
    for build in (lambda: wrappers.RepeatAction(env, 2), lambda: wrappers.StickyAction(env, 0.25, 1), lambda: env.set_step_wrappers(2, 0.0, 0)):
        with pytest.raises(error.Error, match=why):
            build()
    env.close()


# -- stacking rules -------------------------------------------------------------------------------------------------------------------------------
def test_stacking_rules(oracle_factory, monkeypatch):
    env = make("CartPole-v1", oracle_factory)
    sw = _Switch(monkeypatch, env)
    r = wrappers.RepeatAction(env, 4)
    assert r.num_repeats == 4 and sw.calls == [(4, 0.0, 0)]
    with pytest.raises(error.Error):  # a second RepeatAction
        wrappers.RepeatAction(r, 2)
    s = wrappers.StickyAction(r, 0.25, 3)  # sticky OUTSIDE repeat: one decision per outer step
    assert sw.calls[-1] == (4, 0.25, 3) and env._step_wrappers == (4, 0.25, 3) and s.repeat_action_probability == 0.25
    with pytest.raises(error.Error, match="directly over"):  # RepeatAction over StickyAction
        wrappers.RepeatAction(s, 2)
    with pytest.raises(error.Error):  # StickyAction twice
        wrappers.StickyAction(s, 0.5)
    # vector wrappers stack above them as before, and stay stand-alone (the step epilogue does not reach below the sub-environment wrappers)
    top = wrappers.RecordEpisodeStatistics(s)
    assert top.unwrapped is env and env.record_episode_statistics and not env._can_fuse()
    env.set_step_wrappers()
    assert sw.calls[-1] == (0, 0.0, 0) and env._step_wrappers == (0, 0.0, 0)
    env.close()


def test_not_over_another_wrapper(oracle_factory, monkeypatch):
    env = make("Pendulum-v1", oracle_factory)
    _Switch(monkeypatch, env)
    clipped = wrappers.ClipAction(env)
    for build in (lambda: wrappers.RepeatAction(clipped, 2), lambda: wrappers.StickyAction(clipped, 0.5)):
        with pytest.raises(error.Error, match="directly over"):
            build()
    wrappers.ClipAction(wrappers.StickyAction(wrappers.RepeatAction(env, 2), 0.5))  # ... but above them
    env.close()


# -- the fixtures ---------------------------------------------------------------------------------------------------------------------------------
def test_generator_regenerates_its_files_bit_for_bit(tmp_path):
    if not os.path.isdir(os.path.join(REFERENCE, "gymnasium")):
        pytest.skip("the reference tree is not on this machine: the fixtures were recorded where it is")
    script = os.path.join(GOLDEN, "make_golden_step_wrappers.py")
    env = dict(os.environ, GYM_REFERENCE=REFERENCE, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, script, str(tmp_path)], check=True, cwd=ROOT, env=env, capture_output=True)
    names = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert names == sorted(f"step_wrappers_{k}.npz" for k in ("cartpole", "pendulum", "acrobot", "mountaincar", "mountaincar_continuous"))
    for name in names:
        new, old = np.load(tmp_path / name), np.load(os.path.join(GOLDEN, name))
        assert os.path.getsize(tmp_path / name) < 1 << 20
        assert new.files == old.files, name
        for k in new.files:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)
