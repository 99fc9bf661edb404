"""get_attr / set_attr of AcrobotVectorEnv on the oracle-backed host class (which has no per-lane physics: set_attr reaches its engine check
last): defaults and their types, the string attribute book_or_nips, the unknown-name exception, the refusals, the admitted ranges and the bound
behind them, and -- where the reference imports -- round trips against the reference's SyncVectorEnv.  The trajectories are pinned on the GPU
(tests/test_gpu_acrobot_attrs.py)."""
import math

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd.envs import classic_control
from gymnasium_amd.gym_api import error
from gymnasium_amd.vector.hip_vector_env import UnknownEnvAttributeError

try:
    import gymnasium as gym

    HAVE_REF = hasattr(gym.vector, "SyncVectorEnv")
except ImportError:
    gym, HAVE_REF = None, False

DEFAULTS = {"LINK_LENGTH_1": 1.0, "LINK_MASS_1": 1.0, "LINK_MASS_2": 1.0, "LINK_COM_POS_1": 0.5, "LINK_COM_POS_2": 0.5, "LINK_MOI": 1.0,
            "MAX_VEL_1": 4 * math.pi, "MAX_VEL_2": 9 * math.pi, "dt": 0.2, "torque_noise_max": 0.0, "book_or_nips": "book"}
ENGINE_MISSING = "mi_set_env_attr"  # validation passed: only the oracle engine itself has no per-lane physics


def make(oracle_factory, env_id="Acrobot-v1", n=4, **kw):
    return gymnasium_amd.make_vec(env_id, num_envs=n, _engine_factory=oracle_factory, **kw)


def test_get_attr_defaults_and_their_types(oracle_factory):
    env = make(oracle_factory)
    assert [a[0] for a in env.ENV_ATTRS] == list(DEFAULTS) and all(a[2] for a in env.ENV_ATTRS)
    for name, want in DEFAULTS.items():
        got = env.get_attr(name)
        assert len(got) == 4 and all(v == want and type(v) is type(want) for v in got), (name, got)
    env.close()


@pytest.mark.skipif(not HAVE_REF, reason="the reference gymnasium is not importable")
def test_defaults_and_round_trips_equal_the_reference(oracle_factory):
    ref = gym.make_vec("Acrobot-v1", num_envs=3, vectorization_mode="sync")
    env = make(oracle_factory, n=3)
    for name in DEFAULTS:
        a, b = env.get_attr(name), ref.get_attr(name)
        assert a == b and [type(x) for x in a] == [type(x) for x in b], (name, a, b)
    ref.close(), env.close()


def test_book_or_nips_takes_strings_only(oracle_factory):
    env = make(oracle_factory)
    for bad in (1, 1.0, True, np.float64(1.0), [1, 0, 1, 0], ["nips", 1, "book", "book"], np.ones(4)):
        with pytest.raises(TypeError, match="book_or_nips"):
            env.set_attr("book_or_nips", bad)
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="book_or_nips"):
        env.set_attr("book_or_nips", torch.ones(4, dtype=torch.float64))
    for good in ("nips", ["nips", "book", "nips", "book"], ("book",) * 4, np.array(["nips", "book", "book", "nips"])):
        with pytest.raises(error.Error, match=ENGINE_MISSING):
            env.set_attr("book_or_nips", good)
    with pytest.raises(ValueError, match="length equal to the number of environments"):
        env.set_attr("book_or_nips", ["nips", "book"])
    env.close()


def test_kinematics_integrator_keeps_its_behaviour(oracle_factory):
    """The general string path serves CartPole's attribute as before: anything but "euler" is the other integrator, tensors are refused."""
    env = make(oracle_factory, "CartPole-v1")
    for good in ("euler", ["euler", "semi-implicit", "x", "euler"]):
        with pytest.raises(error.Error, match=ENGINE_MISSING):
            env.set_attr("kinematics_integrator", good)
    env.close()


@pytest.mark.parametrize("env_id,name", [("Acrobot-v1", "gravity"), ("Acrobot-v1", "LINK_LENGTH_2"), ("Acrobot-v1", "AVAIL_TORQUE"),
                                         ("CartPole-v1", "lenght"), ("Pendulum-v1", "gravity"), ("MountainCar-v0", "g"),
                                         ("MountainCarContinuous-v0", "force")])
def test_unknown_names_raise_one_class_that_is_both(env_id, name, oracle_factory):
    env = make(oracle_factory, env_id)
    for call in (lambda: env.get_attr(name), lambda: env.set_attr(name, 1.0)):
        for caught in (AttributeError, error.Error, UnknownEnvAttributeError):
            with pytest.raises(caught) as e:
                call()
            assert type(e.value) is UnknownEnvAttributeError and name in str(e.value) and env.ENV_ATTRS[0][0] in str(e.value)
    assert issubclass(UnknownEnvAttributeError, AttributeError) and issubclass(UnknownEnvAttributeError, error.Error)
    env.close()


def test_fast_math_is_refused(oracle_factory):
    env = make(oracle_factory, fast_math=True)
    for call in (lambda: env.get_attr("dt"), lambda: env.set_attr("dt", 0.1), lambda: env.set_attr("book_or_nips", "nips")):
        with pytest.raises(error.Error, match="fast_math") as e:
            call()
        assert not isinstance(e.value, AttributeError)
    env.close()


def test_numpy_scalars_and_python_numbers(oracle_factory):
    env = make(oracle_factory)
    for name in DEFAULTS:
        if name == "book_or_nips":
            continue
        for bad in (np.float32(1.0), np.int64(1)):
            with pytest.raises(TypeError, match="float\\(v\\)"):
                env.set_attr(name, bad)
        with pytest.raises(TypeError):
            env.set_attr(name, "1.0")
        d = DEFAULTS[name]
        lo, hi = classic_control.ACROBOT_ATTR_RANGES[name]
        goods = [np.float64(d), d, [d, np.float64(d), d, d], np.full(4, d)]
        if (lo is None or lo <= 1) and 1 <= hi:
            goods += [1, True, [1, 1.0, np.float64(1.0), True]]
        for good in goods:
            with pytest.raises(error.Error, match=ENGINE_MISSING):  # set_attr reaches the engine check last
                env.set_attr(name, good)
    env.close()


def test_values_outside_the_admitted_ranges_are_refused_by_name(oracle_factory):
    env = make(oracle_factory)
    for name, (lo, hi) in classic_control.ACROBOT_ATTR_RANGES.items():
        with pytest.raises(ValueError, match=f"{name}.*{hi:g}"):
            env.set_attr(name, [1.0, 1.0, math.nextafter(hi, math.inf), 1.0])
        with pytest.raises(error.Error, match=ENGINE_MISSING):
            env.set_attr(name, hi)
        if lo is not None:
            with pytest.raises(ValueError, match=name):
                env.set_attr(name, math.nextafter(lo, -math.inf))
            with pytest.raises(ValueError, match="NaN"):
                env.set_attr(name, math.nan)
            with pytest.raises(error.Error, match=ENGINE_MISSING):
                env.set_attr(name, lo)
    for quiet in (math.nan, -1.0, -math.inf, 0):  # no noise, like the reference's `if self.torque_noise_max > 0`
        with pytest.raises(error.Error, match=ENGINE_MISSING):
            env.set_attr("torque_noise_max", quiet)
    assert set(classic_control.ACROBOT_ATTR_RANGES) == set(DEFAULTS) - {"book_or_nips"}
    env.close()


def test_the_admitted_ranges_keep_every_stage_angle_inside_the_exact_trig_range():
    """The reasoning behind ACROBOT_ATTR_RANGES, evaluated: the bound holds for the box, with the defaults well inside, and it is not idle --
    a box twice as generous in the lengths no longer passes."""
    limit = classic_control.AcrobotVectorEnv.EXACT_TRIG_RANGE
    assert classic_control.acrobot_stage_angle_bound() < limit
    for name, (lo, hi) in classic_control.ACROBOT_ATTR_RANGES.items():
        d = DEFAULTS[name]
        assert (lo is None or lo <= d) and d <= hi, name
    wider = dict(classic_control.ACROBOT_ATTR_RANGES, LINK_LENGTH_1=(0.0, 3.0), LINK_COM_POS_2=(0.0, 3.0))
    assert classic_control.acrobot_stage_angle_bound(wider) > limit


def test_wide_state_velocities_and_attributes_exclude_each_other(oracle_factory):
    env = make(oracle_factory)
    env.reset(seed=0)
    s = np.zeros((4, 4))
    s[1, 3] = 50.0  # accepted by set_state (|velocity| <= 100) but beyond MAX_VEL_2's limit of 32
    env.set_state(s)
    with pytest.raises(ValueError, match="set_state"):
        env.set_attr("dt", 0.1)
    s[1, 3] = 30.0
    env.set_state(s)
    with pytest.raises(error.Error, match=ENGINE_MISSING):
        env.set_attr("dt", 0.1)
    env.close()


def test_pending_and_closed(oracle_factory):
    env = make(oracle_factory)
    env.reset(seed=0)
    env.step_async(np.zeros(4, dtype=np.int64))
    with pytest.raises(error.AlreadyPendingCallError):
        env.set_attr("dt", 0.1)
    env.step_wait()
    env.close()
    with pytest.raises(error.ClosedEnvironmentError):
        env.get_attr("dt")
