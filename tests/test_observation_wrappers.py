"""RescaleObservation / DtypeObservation / FlattenObservation / TransformObservation / TransformReward on the CPU: the NumPy path of
gymnasium_amd.wrappers and the restatement the GPU tests lean on, against what the REFERENCE's wrappers returned
(tests/golden/observation_wrappers.npz, recorded by tests/golden/make_golden_observation_wrappers.py).  Everything is compared bit for bit
(integer views, NaN by position); the trajectories run on the oracle engine.  (Stacking with NormalizeObservation needs the device -- the statistics
wrappers have no CPU implementation -- and is in tests/test_gpu_observation_wrappers.py.)"""
import os
import re
import sys
import warnings

import numpy as np
import pytest

import observation_wrapper_cases as oc
import gymnasium_amd
from conftest import golden
from gymnasium_amd import wrappers as gw
from gymnasium_amd.gym_api import AutoresetMode, batch_space, error, spaces

EXCEPTIONS = {"TypeError": TypeError, "ValueError": ValueError}
MODES = {"NEXT_STEP": "NextStep", "DISABLED": "Disabled"}
RESCALE_CASES = [(name, target) for name in oc.RESCALE_BOXES for target in oc.RESCALE_TARGETS]
DTYPE_CASES = [(name, target) for name in list(oc.BOXES) + list(oc.DISCRETE) for target in oc.DTYPE_TARGETS]


@pytest.fixture(scope="module")
def gold():
    return golden("observation_wrappers.npz")


@pytest.fixture(scope="module")
def errors(gold):
    return dict(str(e).split("=", 1) for e in gold["errors"])


@pytest.fixture(scope="module")
def messages(gold):
    return dict(str(e).split("=", 1) for e in gold["error_messages"])


def stand_in(space, rows, mode="NEXT_STEP"):
    return oc.SpacesOnlyEnv(spaces, batch_space, space, rows, AutoresetMode[mode])


def same_message(got, want):
    """Equal up to how a class is spelled (``<class 'gymnasium.spaces...'>``: the package may run on its own mirror of the spaces)."""
    strip = lambda s: re.sub(r"<class '[^']*\.(\w+)'>", r"<class \1>", s)  # noqa: E731
    return strip(str(got)) == strip(want)


def source_space(name):
    return spaces.Discrete(oc.DISCRETE[name]) if name in oc.DISCRETE else oc.make_box(spaces, name)


def source_batch(name, target):
    return oc.discrete_batch(oc.DISCRETE[name]) if name in oc.DISCRETE else oc.dtype_batch(name, target)


def test_the_fixture_covers_what_it_should(gold, errors):
    """The recording itself: every stated condition occurs in it."""
    for name in oc.RESCALE_BOXES:
        x = oc.crafted(name)
        low, high, dtype = oc.BOXES[name]
        assert x.dtype == dtype and x.shape[1] == low.size
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any(), "both zeros"
        assert ((np.abs(x) > 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any(), "float32 denormals"
        lo, hi = low.astype(dtype), high.astype(dtype)
        for bound in (lo, hi):
            at, below, above = (x == bound).any(0), (x == np.nextafter(bound, np.array(-np.inf, dtype))).any(0), (x == np.nextafter(bound, np.array(np.inf, dtype))).any(0)
            assert at.all() and below[np.isfinite(bound)].all() and above[np.isfinite(bound)].all(), "both bounds and their neighbours"
        # at least one element whose twice-rounded gradient * x + intercept is not what an FMA gives
        differing = 0
        for target in oc.RESCALE_TARGETS:
            key = f"r/{name}/{target}"
            if key in errors:
                continue
            g, c = gold[f"{key}/params"]
            differing += int(oc.differs_from_fused(g, x[-24:], c).sum())
        assert differing > 0, name
    assert {"r/cartpole/pm1", "r/cartpole/unit", "r/wide64/pm1", "r/wide64/unit"} == {k for k in errors if k.startswith("r/")}
    assert int(gold["r/pendulum/same/meta"][0]) == 1 and int(gold["r/pendulum/pm1/meta"][0]) == 0 and int(gold["r/mountaincar/pm1/meta"][0]) == 0
    # float64 values whose float16 cast differs when taken through float32
    for name in ("wide64", "level64"):
        x = oc.crafted(name)
        with np.errstate(all="ignore"):
            direct, through = x.astype(np.float16), x.astype(np.float32).astype(np.float16)
        assert (oc.bits(direct) != oc.bits(through))[~np.isnan(x)].any(), name
        oc.assert_same_bits(gold[f"d/{name}/float16/out"], direct, name)
    assert np.float16(oc.F16_DIRECT[0]) == np.float16(1.001) and np.float16(np.float32(oc.F16_DIRECT[0])) == np.float16(1.0)
    # every supported pair is recorded, or refused by the reference's Box (an unsigned target under a box that reaches below zero, Taxi's 500 states)
    for name, target in DTYPE_CASES:
        key = f"d/{name}/{target}"
        assert (key in errors) != (f"{key}/out" in gold), key
        if key in errors:
            assert target == "uint8"
        elif np.dtype(target).kind in "iu" and name in oc.BOXES:
            x = oc.integer_batch(name, target)
            assert np.isfinite(x).all() and x.min() >= np.iinfo(target).min and x.max() <= np.iinfo(target).max
    assert {"d/level32/uint8/out", "d/level64/uint8/out", "d/frozenlake/uint8/out", "d/cliffwalking/uint8/out"} <= set(gold.files)
    assert gold["f/blackjack/out"].shape == (64, 45) and gold["f/taxi/out"].shape == (500, 500) and gold["f/frozenlake/out"].dtype == np.int64


@pytest.mark.parametrize("name,target", RESCALE_CASES)
def test_rescale_equals_the_reference(gold, errors, messages, name, target):
    key = f"r/{name}/{target}"
    x = oc.crafted(name)
    if key in errors:
        with pytest.raises(EXCEPTIONS[errors[key]]) as e:
            oc.build(gw, stand_in(oc.make_box(spaces, name), len(x)), "rescale", target, name)
        assert same_message(e.value, messages[key])
        return
    w = oc.build(gw, stand_in(oc.make_box(spaces, name), len(x)), "rescale", target, name)
    low, high = gold[f"{key}/space"]
    sp = w.single_observation_space
    assert sp.dtype == low.dtype and np.array_equal(sp.low, low) and np.array_equal(sp.high, high) and w.observation_space == batch_space(sp, len(x))
    assert w.same_out == bool(gold[f"{key}/meta"][0])
    g, c = gold[f"{key}/params"]
    oc.assert_same_bits(w.gradient, g, "gradient"), oc.assert_same_bits(w.intercept, c, "intercept")
    box = oc.make_box(spaces, name)
    pg, pc = oc.rescale_parameters(box.low, box.high, *oc.rescale_target(name, target))
    oc.assert_same_bits(pg, g, "restated gradient"), oc.assert_same_bits(pc, c, "restated intercept")
    oc.assert_same_bits(oc.affine(x, g, c), gold[f"{key}/out"], key + " restatement")
    given = x.copy()
    got = w.observations(given)
    oc.assert_same_bits(got, gold[f"{key}/out"], key)
    assert not np.shares_memory(got, given)
    oc.assert_same_bits(given, x, "the caller's array")
    zeros = gold[f"{key}/out"][1]  # the row of -0.0
    assert not np.signbit(zeros[(g == 1) & (c == 0)]).any(), "-0.0 goes through the arithmetic: +0.0"


@pytest.mark.parametrize("name,target", DTYPE_CASES)
def test_dtype_equals_the_reference(gold, errors, messages, name, target):
    key = f"d/{name}/{target}"
    x = source_batch(name, target)
    if key in errors:
        with pytest.raises(EXCEPTIONS[errors[key]]) as e:
            oc.build(gw, stand_in(source_space(name), len(x)), "dtype", target)
        assert same_message(e.value, messages[key])
        return
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (gymnasium's Box: "precision lowered by casting")
        w = oc.build(gw, stand_in(source_space(name), len(x)), "dtype", target)
    low, high = gold[f"{key}/space"]
    sp = w.single_observation_space
    assert isinstance(sp, spaces.Box) and sp.dtype == np.dtype(target) == low.dtype and sp.shape == low.shape
    assert np.array_equal(sp.low, low) and np.array_equal(sp.high, high)
    oc.assert_same_bits(oc.cast(x, target), gold[f"{key}/out"], key + " restatement")
    given = x.copy()
    got = w.observations(given)
    oc.assert_same_bits(got, gold[f"{key}/out"], key)
    assert not np.shares_memory(got, given)
    oc.assert_same_bits(given, x, "the caller's array")


@pytest.mark.parametrize("name", list(oc.DISCRETE) + ["blackjack", "pendulum"])
def test_flatten_equals_the_reference(gold, name):
    if name == "pendulum":
        space, x = oc.make_box(spaces, name), oc.crafted(name)
        want = x.reshape(len(x), -1)
    elif name == "blackjack":
        space, x = oc.blackjack_space(spaces), oc.blackjack_batch()
        want = oc.one_hot(x, oc.BLACKJACK)
    else:
        space, x = spaces.Discrete(oc.DISCRETE[name]), oc.discrete_batch(oc.DISCRETE[name])
        want = oc.one_hot((x,), (oc.DISCRETE[name],))
    rows = len(x[0]) if isinstance(x, tuple) else len(x)
    oc.assert_same_bits(want, gold[f"f/{name}/out"], name + " restatement")
    w = gw.FlattenObservation(stand_in(space, rows))
    low, high = gold[f"f/{name}/space"]
    sp = w.single_observation_space
    assert isinstance(sp, spaces.Box) and sp.dtype == low.dtype and np.array_equal(sp.low, low) and np.array_equal(sp.high, high)
    given = tuple(p.copy() for p in x) if isinstance(x, tuple) else x.copy()
    oc.assert_same_bits(w.observations(given), gold[f"f/{name}/out"], name)
    for a, b in zip(given if isinstance(x, tuple) else (given,), x if isinstance(x, tuple) else (x,)):
        oc.assert_same_bits(a, b, "the caller's array")


def test_one_hot_of_a_state_outside_its_space_is_zero():
    w = gw.FlattenObservation(stand_in(oc.blackjack_space(spaces), 3))
    got = w.observations((np.array([31, 32, -1]), np.array([0, 11, 5]), np.array([1, 0, 2])))
    assert got.shape == (3, 45) and list(got.sum(1)) == [3, 1, 1] and got[1, 43] == 1 and got[2, 37] == 1


def test_constructor_errors_equal_the_reference(errors, messages):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        from make_golden_observation_wrappers import constructor_cases
    finally:
        sys.path.pop(0)
    cases = constructor_cases(spaces)
    assert {f"ctor/{c}" for c in cases} == {k for k in errors if k.startswith("ctor/")}
    for case, (space, mode, call) in cases.items():
        with pytest.raises(EXCEPTIONS[errors[f"ctor/{case}"]]) as e:
            call(gw, stand_in(space, 3, mode))
        assert same_message(e.value, messages[f"ctor/{case}"]), case


def test_transform_observation_spaces_and_function():
    env = stand_in(oc.make_box(spaces, "pendulum"), 3)
    w = gw.TransformObservation(env, oc.transform_func)
    assert w.observation_space is env.observation_space and w.single_observation_space is env.single_observation_space
    a = np.ones((3, 3), np.float32)
    assert np.array_equal(w.observations(a), a * 0.5 - 0.25)
    single = spaces.Box(-2.0, 2.0, shape=(3,), dtype=np.float32)
    w = gw.TransformObservation(env, oc.transform_func, single_observation_space=single)
    assert w.single_observation_space == single and w.observation_space == batch_space(single, 3)
    w = gw.TransformObservation(env, oc.transform_func, observation_space=batch_space(single, 3), single_observation_space=single)
    assert w.observation_space == batch_space(single, 3)
    with pytest.warns(UserWarning, match="don't match"):
        gw.TransformObservation(env, oc.transform_func, observation_space=batch_space(single, 3))


def make_env(env_id, mode, oracle_factory, n=oc.TRAJ_N):
    return gymnasium_amd.make_vec(env_id, num_envs=n, autoreset_mode=MODES[mode], _engine_factory=oracle_factory)


def stacked(obs):
    """A Tuple observation as its [..., parts] block."""
    return np.stack(obs, axis=-1) if isinstance(obs, tuple) else np.asarray(obs)


@pytest.mark.parametrize("mode", oc.TRAJ_MODES)
@pytest.mark.parametrize("key", list(oc.TRAJECTORIES))
def test_trajectories_through_the_numpy_path(gold, oracle_factory, key, mode):
    env_id, kind, arg = oc.TRAJECTORIES[key]
    w = oc.build(gw, make_env(env_id, mode, oracle_factory), kind, arg, oc.BOX_OF_ENV.get(env_id))
    base = f"t/{key}/{mode}"
    obs, _ = w.reset(seed=oc.TRAJ_SEED)
    oc.assert_same_bits(obs, gold[f"{base}/obs"][0], "reset")
    for t, a in enumerate(oc.trajectory_actions(env_id)):
        o, r, te, tr, _ = w.step(a.copy())
        oc.assert_same_bits(o, gold[f"{base}/obs"][t + 1], f"obs t={t}")
        assert np.array_equal(np.asarray(r, np.float64), gold[f"{base}/rewards"][t]), f"rewards t={t}"
        assert np.array_equal(te, gold[f"{base}/flags"][0, t]) and np.array_equal(tr, gold[f"{base}/flags"][1, t])
        if mode == "DISABLED":
            done = np.logical_or(te, tr)
            if done.any():
                o, _ = w.reset(options={"reset_mask": done})
            oc.assert_same_bits(o, gold[f"{base}/post"][t], f"after the masked reset t={t}")
    w.close()


class SteppingRollout:
    """An env whose ``rollout`` is T ``step()`` calls stacked into host tensors: the shape of HipVectorEnv.rollout's result (a Tuple observation as
    one [T, N, parts] block) without a device."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def rollout(self, num_steps, actions=None, **kwargs):
        import torch

        steps = [self.env.step(actions[t]) for t in range(num_steps)]
        out = {k: torch.from_numpy(np.stack([stacked(s[i]) for s in steps])) for i, k in enumerate(("obs", "rewards", "terminations", "truncations"))}
        out["extra"] = kwargs
        return out


@pytest.mark.parametrize("key", list(oc.TRAJECTORIES))
def test_rollout_equals_steps(oracle_factory, key):
    env_id, kind, arg = oc.TRAJECTORIES[key]
    a = oc.build(gw, make_env(env_id, "NEXT_STEP", oracle_factory), kind, arg, oc.BOX_OF_ENV.get(env_id))
    b = oc.build(gw, SteppingRollout(make_env(env_id, "NEXT_STEP", oracle_factory)), kind, arg, oc.BOX_OF_ENV.get(env_id))
    a.reset(seed=3), b.reset(seed=3)
    actions = oc.trajectory_actions(env_id)[:8]
    steps = [a.step(x) for x in actions]
    traj = b.rollout(8, actions, infos=True)
    assert traj["extra"] == {"infos": True}, "the keywords pass through"
    for i, k in enumerate(("obs", "rewards", "terminations", "truncations")):
        oc.assert_same_bits(traj[k].numpy(), np.stack([np.asarray(s[i]) for s in steps]), f"{key} {k}")
    a.close(), b.close()


def test_wrappers_refuse_what_they_must(oracle_factory):
    env = make_env("Pendulum-v1", "NEXT_STEP", oracle_factory)
    for w in (gw.RescaleObservation(env, -1.0, 1.0), gw.DtypeObservation(env, np.float64), gw.FlattenObservation(env),
              gw.TransformObservation(env, oc.transform_func), gw.TransformReward(env, oc.reward_func)):
        assert not w._transparent and not w._fused and w.unwrapped is env and w.num_envs == oc.TRAJ_N
        with pytest.raises(error.Error, match="untransformed"):
            w.capture_steps(policy=lambda obs: obs, steps=2)
    env.close()
    same = gymnasium_amd.make_vec("Pendulum-v1", num_envs=3, autoreset_mode="SameStep", _engine_factory=oracle_factory)
    for make in (lambda: gw.RescaleObservation(same, -1.0, 1.0), lambda: gw.DtypeObservation(same, np.float64), lambda: gw.FlattenObservation(same),
                 lambda: gw.TransformObservation(same, oc.transform_func)):
        with pytest.raises(ValueError, match="Expected autoreset_mode to be NEXT_STEP or DISABLED"):
            make()
    gw.TransformReward(same, oc.reward_func)  # (a reward wrapper has no such condition, as in the reference)
    same.close()
    black = make_env("Blackjack-v1", "NEXT_STEP", oracle_factory)
    with pytest.raises(TypeError):
        gw.DtypeObservation(black, np.float32)
    with pytest.raises(TypeError):
        gw.RescaleObservation(black, -1.0, 1.0)
    black.close()


def test_device_only_targets_are_named():
    """Any dtype NumPy takes passes on the NumPy path."""
    w = gw.DtypeObservation(stand_in(oc.make_box(spaces, "level32"), 2), np.uint16)
    got = w.observations(np.array([[1.5, 2, 3, 4, 250]] * 2, np.float32))
    assert got.dtype == np.uint16 and list(got[0]) == [1, 2, 3, 4, 250]
