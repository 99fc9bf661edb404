"""CPU side of the crafted generator states (tests/golden/normal_sampler.npz, written by tests/golden/make_golden_normal_sampler.py): lanes whose reset
draws one of the rare branches of NumPy's ziggurat -- the tail beyond R, whose VALUE is made of libm's log1p, and the wedge, whose exp only decides --
at a chosen velocity index.  Here: the file is what the script writes, its conditions hold, the running NumPy reproduces it, and the oracle engine,
seeded with the words through the C ABI, resets to the recorded state.  tests/test_gpu_normal_sampler.py holds the HIP engine to the same rows.
"""
import importlib.util
import os

import numpy as np
import pytest

import gymnasium_amd
from gymnasium_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = {"half_cheetah": "HalfCheetah-v5", "ant": "Ant-v5", "inverted_double_pendulum": "InvertedDoublePendulum-v5"}


def sampler_module():
    spec = importlib.util.spec_from_file_location("make_golden_normal_sampler", os.path.join(HERE, "golden", "make_golden_normal_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MK = sampler_module()


@pytest.fixture(scope="module")
def rows():
    return MK.load()


def category(rows, name, *cats):
    return np.isin(rows[f"{name}_category"], [MK.CATEGORIES.index(c) for c in cats])


def neighbour_words(words):
    """the states one raw word later (Generator.bit_generator.advance(1))"""
    g = np.random.Generator(np.random.PCG64(0))
    out = np.empty_like(words)
    for i, w in enumerate(words):
        _native.set_pcg_words(g, w)
        g.bit_generator.advance(1)
        out[i] = _native.pcg_words(g)
    return out


def test_fixture_regenerates_byte_for_byte():
    if not MK.expected_libm():
        pytest.skip("host libm is not glibc 2.35's: the log1p / exp columns cannot be regenerated here")
    with open(MK.PATH, "rb") as f:
        committed = f.read()
    fresh = MK.generate()
    with np.load(MK.PATH, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(fresh)
        for name in z.files:
            assert z[name].dtype == fresh[name].dtype and np.array_equal(z[name], fresh[name]), name
    assert MK.npz_bytes(fresh) == committed
    assert len(committed) <= 640 * 1024  # well inside the limit for a committed file


def test_conditions_of_the_fixture(rows):
    from gymnasium_amd.envs.mujoco import compiler

    for name, (nq, nv, qpos0) in MK.ROBOTS.items():
        m = compiler.compile_model(name)
        assert (m.nq, m.nv) == (nq, nv) and np.array_equal(m.qpos0, qpos0)
        cat, k = rows[f"{name}_category"], rows[f"{name}_k"]
        assert cat.shape == (MK.N,) and MK.N == 1024
        assert {c: int((cat == t).sum()) for t, c in enumerate(MK.CATEGORIES)} == {"tail": 512, "tail_retry": 128, "wedge_accept": 128, "wedge_reject": 128, "plain": 128}
        assert np.array_equal(k, np.arange(MK.N) % nv)
        special = rows[f"{name}_qvel"][np.arange(MK.N), k] / MK.SCALE
        tails = category(rows, name, "tail", "tail_retry")
        assert (np.abs(special[tails]) > MK.R).all() and (np.abs(special[~tails]) < MK.R).all()
        earlier = np.arange(nv)[None, :] < k[:, None]
        assert (np.abs(rows[f"{name}_qvel"] / MK.SCALE)[earlier] < MK.R).all()
        for c in MK.CATEGORIES:  # every velocity index meets every category, and every wavefront mixes them
            assert set(k[category(rows, name, c)]) == set(range(nv)), (name, c)
        for w in range(MK.N // 64):
            assert len(set(cat[64 * w:64 * w + 64])) == len(MK.CATEGORIES), (name, w)
        assert len({tuple(r) for r in rows[f"{name}_words"]}) == MK.N
    lx, lr = rows["log1p_x"].view(np.float64), rows["log1p_r"].view(np.float64)
    assert lx.size >= 3 * (512 * 2 + 128 * 4) * 3 // 4 and ((lx <= 0) & (lx > -1)).all() and (np.diff(lx) > 0).all()
    ex = rows["exp_x"].view(np.float64)
    assert ex.size >= 3 * 256 * 2 // 3 and ((ex <= 0) & (ex >= -0.5 * MK.R * MK.R)).all()


def test_running_numpy_and_libm_reproduce_the_rows(rows):
    import math

    if not MK.expected_libm():
        pytest.skip("host libm is not glibc 2.35's: NumPy's tail draws here are another libm's, nothing to compare the rows with")
    for name, (nq, nv, qpos0) in MK.ROBOTS.items():
        g = np.random.Generator(np.random.PCG64(0))
        for i in range(MK.N):
            _native.set_pcg_words(g, rows[f"{name}_words"][i])
            qpos = qpos0 + g.uniform(low=-MK.SCALE, high=MK.SCALE, size=nq)
            qvel = MK.SCALE * g.standard_normal(nv)
            assert np.array_equal(qpos, rows[f"{name}_qpos"][i]) and np.array_equal(qvel, rows[f"{name}_qvel"][i]), (name, i)
            assert np.array_equal(_native.pcg_words(g), rows[f"{name}_words_after"][i]), (name, i)
    lx, ex = rows["log1p_x"].view(np.float64), rows["exp_x"].view(np.float64)
    assert np.array_equal(np.array([math.log1p(v) for v in lx.tolist()]).view(np.uint64), rows["log1p_r"])
    assert np.array_equal(np.array([math.exp(v) for v in ex.tolist()]).view(np.uint64), rows["exp_r"])


def reset_from(env, words):
    """the engine at `words`, reset: (qpos | qvel rows, generator words afterwards)"""
    env._engine.seed(words)
    env.reset()
    return np.array(env.get_state()[0]), env.get_rng_state().copy()


def expected_state(rows, name):
    return np.concatenate([rows[f"{name}_qpos"], rows[f"{name}_qvel"]], axis=1)


@pytest.mark.parametrize("name", list(IDS))
def test_oracle_engine_reproduces_the_rows(name, rows, oracle_factory):
    if not MK.expected_libm():
        pytest.skip("host libm is not glibc 2.35's: the oracle's tail draws are this machine's log1p")
    nq, nv, _ = MK.ROBOTS[name]
    env = gymnasium_amd.make_vec(IDS[name], num_envs=MK.N, _engine_factory=oracle_factory)
    env.reset(seed=0)
    state, after = reset_from(env, rows[f"{name}_words"])
    assert np.array_equal(state[:, :nq + nv], expected_state(rows, name))
    assert np.array_equal(after, rows[f"{name}_words_after"])
    # the guard: one word later the special draw is gone -- exactly the lanes moved there differ
    tails = category(rows, name, "tail", "tail_retry")
    words = rows[f"{name}_words"].copy()
    words[tails] = neighbour_words(words[tails])
    twin, _ = reset_from(env, words)
    differs = (twin[:, :nq + nv] != expected_state(rows, name)).any(axis=1)
    assert np.array_equal(differs, tails)
    env.close()
