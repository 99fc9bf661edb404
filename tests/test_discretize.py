"""CPU side of wrappers.DiscretizeObservation / DiscretizeAction: spaces, tables, errors, the NumPy path and ``revert_*`` equal what was recorded from the
reference (tests/golden/discretize.npz); whole trajectories through make_vec(..., _engine_factory=oracle_factory) plus the wrappers equal the SyncVectorEnv
recordings in the three autoreset modes, final_obs, masked resets and FlattenObservation's one-hot rows included; the header declares the two entry points
and _native lists them.  What the kernels compute is a GPU matter (tests/test_gpu_discretize.py)."""
import os
import re

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native, wrappers
from gymnasium_amd.gym_api import AutoresetMode, batch_space, spaces
from conftest import REFERENCE, ROOT

import discretize_cases as dc

FIX = dc.fixture()
MODES = {"next": AutoresetMode.NEXT_STEP, "same": AutoresetMode.SAME_STEP, "disabled": AutoresetMode.DISABLED}


SpacesOnlyEnv, box_of, obs_wrapper, act_wrapper = dc.SpacesOnlyEnv, dc.box_of, dc.obs_wrapper, dc.act_wrapper


def same(got, want, what):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True), what


def check_spaces(single, batched, k):
    if isinstance(single, spaces.Discrete):
        assert np.array_equal([single.n], FIX[f"{k}/single"]) and isinstance(batched, spaces.MultiDiscrete)
        assert np.array_equal(batched.nvec, FIX[f"{k}/batched"]) and batched.dtype == np.int64
    else:
        assert isinstance(single, spaces.MultiDiscrete) and np.array_equal(single.nvec, FIX[f"{k}/single"])
        assert isinstance(batched, spaces.Box) and batched.dtype == FIX[f"{k}/batched"].dtype == np.int64
        assert np.array_equal(np.stack([batched.low, batched.high]), FIX[f"{k}/batched"])


# -- 1. spaces, tables, the NumPy path, revert_* ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(dc.OBS_CASES))
def test_observation_wrapper_equals_the_recording(case):
    k = f"o/{case}"
    x, y = FIX[f"{k}/x"], FIX[f"{k}/y"]
    w = obs_wrapper(case, rows=len(x))
    check_spaces(w.single_observation_space, batch_space(w.single_observation_space, dc.N), k)
    edges = np.concatenate(w.bin_edges)
    if edges.size:
        same(edges, FIX[f"{k}/edges"], "bin_edges")
    assert FIX[f"{k}/edges"].size == edges.size == int(np.sum(w.bins - 1))
    same(w._hi_clip, FIX[f"{k}/hi_clip"], "the clip bound")
    assert w.n_dims == x.shape[1] and w.multidiscrete == dc.OBS_CASES[case][2] and np.array_equal(w.low, box_of(dc.OBS_CASES[case][0]).low)
    same(w.observations(x), y, "observations()")
    same(w._apply(np.stack([x, x[::-1]]), 2), np.stack([y, y[::-1]]), "a [T, N, D] block")
    lows, highs = zip(*[w.revert_observation(r if w.multidiscrete else int(r)) for r in y[:len(FIX[f"{k}/revert"][0])]])
    same(np.stack([np.stack(lows), np.stack(highs)]), FIX[f"{k}/revert"], "revert_observation")


def test_observation_quirks_are_in_the_recording():
    """What the issue lists, read off the recording itself: NaN in the last bin, bins=1 gives 0, the float32 clip bound equals high for 0.6 and not for 0.07."""
    x, y = FIX["o/pendulum_345_multi/x"], FIX["o/pendulum_345_multi/y"]
    nan_rows = np.isnan(x)
    assert nan_rows.any() and np.array_equal(y[nan_rows], (np.array([3, 4, 5]) - 1)[np.nonzero(nan_rows)[1]])
    assert not FIX["o/pendulum_1/y"].any() and FIX["o/pendulum_1/edges"].size == 0
    hi = FIX["o/mountaincar_2/hi_clip"]
    assert hi.dtype == np.float32 and hi[0] == np.float32(0.6) and hi[1] != np.float32(0.07)
    assert FIX["o/pendulum_345/edges"].dtype == np.float32 and FIX["a/hopper_345/centers"].dtype == np.float32
    assert FIX["o/wide64_345/edges"].dtype == np.float64 and FIX["a/act64_345/y"].dtype == np.float64
    assert FIX["o/one_cap/edges"].size == _native.DISCRETIZE_MAX_TABLE == dc.MAX_TABLE


@pytest.mark.parametrize("case", list(dc.ACT_CASES))
def test_action_wrapper_equals_the_recording(case):
    k = f"a/{case}"
    x, y = FIX[f"{k}/x"], FIX[f"{k}/y"]
    w = act_wrapper(case, rows=len(x))
    check_spaces(w.single_action_space, batch_space(w.single_action_space, dc.N), k)
    same(np.concatenate(w.bin_centers), FIX[f"{k}/centers"], "bin_centers")
    same(w.actions(x), y, "actions()")
    same(w.actions(x.tolist()), y, "actions() of a list")
    same(w._actions_of_steps(np.stack([x, x[::-1]]), 2), np.stack([y, y[::-1]]), "a [T, N] block")
    small = np.abs(x) < 2 ** 31
    if small.all(axis=None if x.ndim == 1 else 1).any():
        rows = small if x.ndim == 1 else small.all(axis=1)
        w32 = act_wrapper(case, rows=int(rows.sum()))
        same(w32.actions(x[rows].astype(np.int32)), y[rows], "int32 indices")
    same(np.array([w.revert_action(r) for r in y[:len(FIX[f"{k}/revert"])]], dtype=np.int64), FIX[f"{k}/revert"], "revert_action")


def test_flat_indices_wrap_and_multidiscrete_indices_clamp():
    w = act_wrapper("one_7", rows=2)
    centers = w.bin_centers[0]
    assert np.array_equal(w.actions(np.array([-1, 100])), centers[[6, 2]][:, None])
    wm = act_wrapper("one_7_multi", rows=2)
    assert np.array_equal(wm.actions(np.array([[-1], [100]])), centers[[0, 6]][:, None])


def test_non_integer_indices_are_refused():
    for case, bad in (("one_7", np.array([0.0, 1.0, 2.0])), ("one_7_multi", np.array([[0.5], [1.0], [2.0]])), ("one_7", np.array([True, False, True]))):
        with pytest.raises(TypeError):
            act_wrapper(case).actions(bad)
    with pytest.raises(ValueError):
        act_wrapper("one_7").actions(np.zeros((3, 1), dtype=np.int64))


# -- 2. refused constructor calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(dc.REFUSED))
def test_refused_constructor_calls(case, oracle_factory):
    import builtins

    which, env_id, bins = dc.REFUSED[case]
    kw = {} if env_id.startswith("FrozenLake") else {"_engine_factory": oracle_factory}
    try:
        env = gymnasium_amd.make_vec(env_id, num_envs=2, **kw)
    except Exception:  # noqa: BLE001 -- (an id this backend cannot build here: its spaces stand in for it)
        env = SpacesOnlyEnv(spaces.Discrete(16) if env_id.startswith("FrozenLake") else spaces.Box(-np.inf, np.inf, (17,), np.float64),
                            spaces.Discrete(4) if env_id.startswith("FrozenLake") else spaces.Box(-1.0, 1.0, (6,), np.float32), 2)
    want = getattr(builtins, dc.errors()[f"ctor/{case}"])
    with pytest.raises(want):
        (wrappers.DiscretizeObservation if which == "obs" else wrappers.DiscretizeAction)(env, bins)


def test_stated_deviations_are_refused():
    two_d = spaces.Box(-np.ones((2, 2), np.float32), np.ones((2, 2), np.float32), dtype=np.float32)
    with pytest.raises(ValueError, match="1-D"):
        wrappers.DiscretizeObservation(SpacesOnlyEnv(two_d, spaces.Discrete(2), 2), 3)
    with pytest.raises(ValueError, match="1-D"):
        wrappers.DiscretizeAction(SpacesOnlyEnv(spaces.Discrete(2), two_d, 2), 3)
    with pytest.raises(ValueError, match="2\\^62"):
        wrappers.DiscretizeAction(SpacesOnlyEnv(spaces.Discrete(2), box_of("humanoid"), 2), 13)  # 13^17 > 2^62
    wrappers.DiscretizeAction(SpacesOnlyEnv(spaces.Discrete(2), box_of("humanoid"), 2), 13, multidiscrete=True)
    # the LDS cap: a table at it is taken (one_cap above), one entry more is refused
    with pytest.raises(ValueError, match="LDS"):
        wrappers.DiscretizeObservation(SpacesOnlyEnv(box_of("one"), spaces.Discrete(2), 2), dc.MAX_TABLE + 2)
    wrappers.DiscretizeAction(SpacesOnlyEnv(spaces.Discrete(2), box_of("one"), 2), dc.MAX_TABLE)
    with pytest.raises(ValueError, match="LDS"):
        wrappers.DiscretizeAction(SpacesOnlyEnv(spaces.Discrete(2), box_of("one"), 2), dc.MAX_TABLE + 1)


# -- 3. trajectories through the CPU checker ------------------------------------------------------------------------------------------------------------
def final_rows(infos, like):
    """(rows, mask) of a NumPy infos dict's final_obs object array."""
    fo, fm = np.zeros_like(like), np.zeros(len(like), dtype=bool)
    if "final_obs" in infos:
        fm = np.asarray(infos["_final_obs"]).copy()
        for i in np.flatnonzero(fm):
            assert isinstance(infos["final_obs"][i], int) == (like.ndim == 1)
            fo[i] = infos["final_obs"][i]
        assert all(infos["final_obs"][i] is None for i in np.flatnonzero(~fm))
    return fo, fm


@pytest.mark.parametrize("name,mode", dc.TRAJ_KEYS)
def test_trajectories_equal_the_sync_vector_env_recordings(name, mode, oracle_factory):
    k = f"t/{name}/{mode}"
    env = gymnasium_amd.make_vec(dc.TRAJ[name][0], num_envs=dc.N, max_episode_steps=dc.LIMIT, autoreset_mode=MODES[mode], _engine_factory=oracle_factory)
    w = dc.wrap(wrappers, env, name)
    obs0, _ = w.reset(seed=dc.SEED)
    same(obs0, FIX[f"{k}/obs0"], "obs0")
    for t in range(dc.T):
        o, r, te, tr, infos = w.step(FIX[f"{k}/actions"][t].copy())
        same(o, FIX[f"{k}/obs"][t], ("obs", t)), same(r, FIX[f"{k}/rewards"][t], ("rewards", t))
        same(te, FIX[f"{k}/term"][t], ("term", t)), same(tr, FIX[f"{k}/trunc"][t], ("trunc", t))
        if mode == "same":
            fo, fm = final_rows(infos, o)
            same(fm, FIX[f"{k}/final_mask"][t], ("final mask", t)), same(fo, FIX[f"{k}/final_obs"][t], ("final_obs", t))
        mask = FIX[f"{k}/reset_mask"][t]
        if mask.any():
            ro, _ = w.reset(options={"reset_mask": mask.copy()})
            same(ro, FIX[f"{k}/reset_obs"][t], ("masked reset", t))
    w.close()


def test_recorded_trajectories_cover_what_they_should():
    for name in dc.TRAJ:
        for mode in dc.MODES:
            k = f"t/{name}/{mode}"
            done = FIX[f"{k}/term"] | FIX[f"{k}/trunc"]
            assert done.sum() >= dc.N and FIX[f"{k}/reset_mask"][dc.MASK_AT].any()
            assert (mode == "same") == (f"{k}/final_obs" in FIX)
    assert FIX["t/mountaincar_onehot/same/obs"].shape[-1] == 16 and set(np.unique(FIX["t/mountaincar_onehot/same/obs"])) == {0, 1}
    assert FIX["t/pendulum_flat/same/final_obs"].ndim == 2 and FIX["t/pendulum_multi/same/final_obs"].ndim == 3
    assert FIX["t/pendulum_flat/next/rewards"].dtype == np.float64


@pytest.mark.parametrize("name", list(dc.SAMPLE_CASES))
def test_seeded_samples_of_the_wrappers_action_space(name, oracle_factory):
    env_id, bins, multi = dc.SAMPLE_CASES[name]
    w = wrappers.DiscretizeAction(gymnasium_amd.make_vec(env_id, num_envs=dc.SAMPLE_N, _engine_factory=oracle_factory), bins, multidiscrete=multi)
    w.action_space.seed(dc.SAMPLE_SEED)
    same(np.stack([w.action_space.sample() for _ in range(dc.SAMPLE_BATCHES)]), FIX[f"s/{name}"], "samples")
    with pytest.raises(gymnasium_amd.gym_api.error.Error):
        w.capture_steps(policy="random")


def test_placement(oracle_factory):
    env = gymnasium_amd.make_vec("Pendulum-v1", num_envs=2, _engine_factory=oracle_factory)
    w = wrappers.DiscretizeObservation(wrappers.DiscretizeAction(wrappers.RescaleAction(env, np.float32(0.0), np.float32(1.0)), 3), 4)
    assert np.array_equal(w.actions(np.array([0, 1])), np.array([[1 / 6], [0.5]], dtype=np.float32))  # (bin centres of [0, 1]: RescaleAction maps them on)
    with pytest.raises(ValueError):  # ClipAction's own space is unbounded, as in the reference
        wrappers.DiscretizeAction(wrappers.ClipAction(env), 3)
    assert w.single_observation_space == spaces.Discrete(64) and w.single_action_space == spaces.Discrete(3)
    assert wrappers.FlattenObservation(w).single_observation_space.shape == (64,)
    with pytest.raises(ValueError):  # the normalisers' spaces are unbounded, as in the reference
        wrappers.DiscretizeObservation(SpacesOnlyEnv(spaces.Box(-np.inf, np.inf, (3,), np.float32), spaces.Discrete(2), 2), 4)
    with pytest.raises(gymnasium_amd.gym_api.error.Error):
        w.capture_steps(steps=1)
    assert wrappers.DiscretizeAction._transparent and not wrappers.DiscretizeObservation._transparent
    assert issubclass(wrappers.DiscretizeAction, wrappers.VectorActionWrapper)


# -- 4. the ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_native_lists_them():
    with open(os.path.join(ROOT, "include", "mi355env.h")) as f:
        header = f.read()
    for symbol in ("discretize_observations", "discretize_actions"):
        assert re.search(rf"^int mi_{symbol}\(", header, re.M) and symbol in _native.WRAPPER_SYMBOLS and symbol not in _native.SYMBOLS
    assert int(re.search(r"#define MI_DISCRETIZE_MAX_TABLE (\d+)", header).group(1)) == _native.DISCRETIZE_MAX_TABLE
    assert int(re.search(r"#define MI_DISCRETIZE_MAX_DIM (\d+)", header).group(1)) == _native.DISCRETIZE_MAX_DIM
    assert "discretize.hip" in __import__("gymnasium_amd.csrc.build", fromlist=["SOURCES"]).SOURCES and _native.ABI_VERSION == 10


# -- 5. live against the reference --------------------------------------------------------------------------------------------------------------------
def test_live_against_the_reference(oracle_factory):
    if not os.path.isdir(os.path.join(REFERENCE, "gymnasium")):
        pytest.skip("the reference tree is not here")
    gym = pytest.importorskip("gymnasium")
    if not hasattr(gym.wrappers, "DiscretizeObservation"):
        pytest.skip("this gymnasium has no Discretize wrappers")
    for mode_name, mode in (("next", gym.vector.AutoresetMode.NEXT_STEP), ("same", gym.vector.AutoresetMode.SAME_STEP)):
        ref = gym.vector.SyncVectorEnv([lambda: dc.wrap(gym.wrappers, gym.make("Pendulum-v1", max_episode_steps=3), "pendulum_flat")] * 4, autoreset_mode=mode)
        ours = dc.wrap(wrappers, gymnasium_amd.make_vec("Pendulum-v1", num_envs=4, max_episode_steps=3, autoreset_mode=MODES[mode_name],
                                                        _engine_factory=oracle_factory), "pendulum_flat")
        assert ours.observation_space == ref.observation_space and ours.action_space == ref.action_space
        o1, o2 = ours.reset(seed=21)[0], ref.reset(seed=21)[0]
        same(o1, o2, "reset")
        ref.action_space.seed(2)
        for t in range(9):
            a = ref.action_space.sample() - (t % 3)  # (some indices below zero: they wrap)
            s1, s2 = ours.step(a.copy()), ref.step(a.copy())
            for g, want in zip(s1[:4], s2[:4]):
                same(g, want, (mode_name, t))
            if mode_name == "same" and "final_obs" in s2[4]:
                same(s1[4]["_final_obs"], s2[4]["_final_obs"], "final mask")
                assert list(s1[4]["final_obs"]) == list(s2[4]["final_obs"])
        ref.close(), ours.close()
