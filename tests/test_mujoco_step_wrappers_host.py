"""CPU side of RepeatAction / StickyAction over the MuJoCo ids.

Where the reference tree exists, the hand composition of tests/mujoco_step_wrapper_cases.py -- what the GPU test compares the engine with -- is pinned on
the reference's own SyncVectorEnv over StickyAction(RepeatAction(<id>Env, 3), 0.5, 2), run through tests/fake_mujoco (the reference's env classes over
this repo's CPU oracle, as in test_mujoco_fixture_pipeline.py): observations, rewards, flags and the whole infos dict under the reference's strict
data_equivalence, the generators' words, and the wrappers' own sticky state, exactly.  Always: the refusal over the checker backend, which has no
mi_set_step_wrappers, and the constructors' validation over a MuJoCo id."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import wrappers
from gymnasium_amd.gym_api import error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("GYM_REFERENCE", "/root/reference")
FAKE = os.path.join(ROOT, "tests", "fake_mujoco")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "gymnasium")), reason="needs the reference tree (its env classes and wrappers)")

CHECK = r'''
TESTS_DIR, ENV_ID, MODE = %r, %r, %r
import sys
import numpy as np
import mujoco, gymnasium as gym
from gymnasium.wrappers import RepeatAction, StickyAction
from gymnasium.utils.env_checker import data_equivalence
import gymnasium_amd
from oracle import oracle
assert getattr(mujoco, "IS_ORACLE_SHIM", False)
sys.path.insert(0, TESTS_DIR)
from mujoco_step_wrapper_cases import Composition, coverage
N, K, P, D, LIMIT, T = 8, 3, 0.5, 2, 7, 30
ref = gym.make_vec(ENV_ID, num_envs=N, vectorization_mode="sync", vector_kwargs={"autoreset_mode": MODE}, max_episode_steps=LIMIT,
                   wrappers=(lambda e: StickyAction(RepeatAction(e, K), P, D),))
plain = gym.make_vec("MI355X/" + ENV_ID, num_envs=N, autoreset_mode="Disabled", max_episode_steps=LIMIT, _engine_factory=oracle.engine_factory)
comp = Composition(plain, K, P, D, MODE)
assert data_equivalence(comp.reset(seed=5), ref.reset(seed=5), exact=True), "reset"
def sticky(e):
    while not isinstance(e, StickyAction):
        e = e.env
    return e
def words(e):
    s = e.unwrapped.np_random.bit_generator.state["state"]
    m = (1 << 64) - 1
    return [s["state"] >> 64, s["state"] & m, s["inc"] >> 64, s["inc"] & m]
ref.action_space.seed(2)
records = []
for t in range(T):
    a = ref.action_space.sample()
    rec = comp.step(a)
    s2 = ref.step(a.copy())
    records.append(rec)
    for key, got in zip(("obs", "reward", "terminated", "truncated"), s2):
        assert data_equivalence(rec[key], got, exact=True), (t, key, rec[key], got)
    assert data_equivalence(dict(rec["infos"]), dict(s2[4]), exact=True), (t, "infos", sorted(rec["infos"]), sorted(s2[4]))
    assert np.array_equal(rec["rng"], np.array([words(e) for e in ref.envs], dtype=np.uint64)), (t, "generator words")
    st = [sticky(e) for e in ref.envs]
    assert np.array_equal(rec["sticky_taken"], [s.repeats_taken for s in st]), (t, "repeats_taken")
    assert np.array_equal(rec["sticky_has_last"], [s.last_action is not None for s in st]), (t, "last_action is None")
    for i, s in enumerate(st):
        if s.last_action is not None:
            assert np.array_equal(comp.last[i], s.last_action), (t, i, "last_action")
c = coverage(records, K, D)
assert c["trunc_inside"] > 0 and c["triggered"] > 0 and c["not_triggered"] > 0 and c["cut"] > 0, c
print("COMPOSITION_OK", c)
'''


def _env():
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([FAKE, REFERENCE, ROOT]), PYTHONDONTWRITEBYTECODE="1", GYM_REFERENCE=REFERENCE)
    e.pop("GYMNASIUM_AMD_FORCE_MIRROR", None)
    return e


@needs_reference
@pytest.mark.parametrize("mode", ["NextStep", "SameStep"])
@pytest.mark.parametrize("env_id", ["HalfCheetah-v5", "Hopper-v5", "InvertedPendulum-v5"])
def test_the_hand_composition_equals_the_reference(env_id, mode):
    p = subprocess.run([sys.executable, "-c", CHECK % (os.path.join(ROOT, "tests"), env_id, mode)], env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "COMPOSITION_OK" in p.stdout, p.stdout[-2500:] + p.stderr[-3500:]


@pytest.mark.parametrize("env_id", ["HalfCheetah-v5", "Humanoid-v5", "InvertedPendulum-v5"])
def test_the_checker_backend_still_refuses_the_mujoco_ids(oracle_factory, env_id):
    env = gymnasium_amd.make_vec(env_id, num_envs=4, _engine_factory=oracle_factory)
    assert not hasattr(env._engine.lib, "set_step_wrappers")
    for build in (lambda: wrappers.RepeatAction(env, 2), lambda: wrappers.StickyAction(env, 0.25, 1), lambda: env.set_step_wrappers(2, 0.0, 0)):
        with pytest.raises(error.Error, match="the MuJoCo and ToyText kernels have no such step"):
            build()
    assert env._step_wrappers == (0, 0.0, 0)
    env.close()


def test_an_engine_with_the_entry_point_lets_the_mujoco_ids_through(oracle_factory, monkeypatch):
    env = gymnasium_amd.make_vec("Hopper-v5", num_envs=4, _engine_factory=oracle_factory)
    calls = []
    monkeypatch.setattr(env._engine.lib, "set_step_wrappers", True, raising=False)
    monkeypatch.setattr(env._engine, "set_step_wrappers", lambda *a: calls.append(a), raising=False)
    s = wrappers.StickyAction(wrappers.RepeatAction(env, 3), 0.5, 2)
    assert calls == [(3, 0.0, 0), (3, 0.5, 2)] and env._step_wrappers == (3, 0.5, 2) and s.unwrapped is env
    with pytest.raises(error.Error, match="MaxAndSkipObservation of the sub-environments exists for"):  # stays classic-only
        env.set_max_and_skip(4)
    env.set_step_wrappers()
    assert calls[-1] == (0, 0, 0) or calls[-1] == (0, 0.0, 0)
    env.close()
    tab = gymnasium_amd.make_vec("FrozenLake-v1", num_envs=4, _engine_factory=oracle_factory)
    monkeypatch.setattr(tab._engine.lib, "set_step_wrappers", True, raising=False)
    with pytest.raises(error.Error, match="ToyText kernels have no such step"):
        wrappers.RepeatAction(tab, 2)
    tab.close()


def test_constructor_validation_over_a_mujoco_id(oracle_factory, monkeypatch):
    env = gymnasium_amd.make_vec("HalfCheetah-v5", num_envs=4, _engine_factory=oracle_factory)
    monkeypatch.setattr(env._engine.lib, "set_step_wrappers", True, raising=False)
    monkeypatch.setattr(env._engine, "set_step_wrappers", lambda *a: None, raising=False)
    for bad in (2.0, "4"):
        with pytest.raises(TypeError, match="expected to be an integer"):
            wrappers.RepeatAction(env, bad)
    for bad in (0, -3, np.int64(0)):
        with pytest.raises(ValueError, match="equal or greater than one"):
            wrappers.RepeatAction(env, bad)
    for bad in (1, 1.5, -0.1):
        with pytest.raises(getattr(error, "InvalidProbability")):
            wrappers.StickyAction(env, bad)
    with pytest.raises(ValueError, match="larger or equal than 1"):
        wrappers.StickyAction(env, 0.5, 0)
    with pytest.raises(error.Error, match="32-bit half"):  # the range form stays refused
        wrappers.StickyAction(env, 0.5, (1, 3))
    with pytest.raises(error.Error, match="directly over"):
        wrappers.RepeatAction(wrappers.ClipAction(env), 2)
    env.close()
