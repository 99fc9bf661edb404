"""-m gpu: the HIP engine's mjx::standard_normal (csrc/mjx_kernels.h) against tests/golden/normal_sampler.npz, through the C ABI.

The fixture holds 1 024 crafted generator states per robot whose reset draws the ziggurat's tail (512 lanes, 128 more that go round the tail's rejection
loop), its wedge (128 accepted, 128 rejected) or the fast path (128) at velocity index lane % nv -- what NumPy, on glibc's log1p and exp, makes of them
(tests/golden/make_golden_normal_sampler.py; tests/test_normal_sampler.py holds the oracle engine and the running NumPy to the same rows).  The tail's
value R + (-1/R) log1p(-u) goes into qvel bit for bit, so the device's log1p has to be glibc's, not merely accurate; the words afterwards pin the number
of draws each branch consumed, hence every accept / reject decision.

Every comparison is array_equal on get_state() rows and get_rng_state(): no tolerances.  Each test is a handful of launches on 1 024 lanes; each
instantiation of MjEnv::reset is met: reset(), the autoreset inside step() and rollout() in both modes, the cooperative default (whose glue kernel
resets) and the per-lane-model kernels of csrc/mjx_model.hip.

Measured on one MI355X with the device library's log1p in the tail (before csrc/log1p_exact.h): 2 / 3 / 3 of the 640 tail lanes of HalfCheetah / Ant /
InvertedDoublePendulum differed from NumPy in the last bit of their special velocity, the same lanes in every instantiation; no lane differed in the
words afterwards, none in the wedge or on the fast path.  With the restated routine: none anywhere (docs/results_log.md).
"""
import numpy as np
import pytest

import gymnasium_amd

from test_normal_sampler import IDS, MK, category, expected_state, neighbour_words

pytestmark = pytest.mark.gpu
N = MK.N
_SECOND = {}


@pytest.fixture(scope="module")
def rows():
    return MK.load()


def report(label, name, rows, state, after, want_state=None, want_after=None):
    """Print the mismatching lanes by category and velocity index; return (values agree, words agree)."""
    nq, nv, _ = MK.ROBOTS[name]
    want_state = expected_state(rows, name) if want_state is None else want_state
    want_after = rows[f"{name}_words_after"] if want_after is None else want_after
    bad_v = (state[:, :nq + nv] != want_state).any(axis=1)
    bad_w = (after != want_after).any(axis=1)
    k = rows[f"{name}_k"]
    parts = []
    for c in MK.CATEGORIES:
        sel = category(rows, name, c)
        at = sorted(set(k[sel & bad_v].tolist()))
        parts.append(f"{c} {int((sel & bad_v).sum())}/{int(sel.sum())} values" + (f" (velocity index {at})" if at else "") + f", {int((sel & bad_w).sum())} words")
    special = state[np.arange(N), nq + k] != want_state[np.arange(N), nq + k]
    print(f"normal sampler, {name}, {label}: lanes that differ from NumPy -- " + "; ".join(parts) + f"; {int((bad_v & ~special).sum())} lanes differ away from their special draw")
    return not bad_v.any(), not bad_w.any()


def make(name, model="stock", **kw):
    env = gymnasium_amd.make_vec(IDS[name], num_envs=N, **kw)
    if model == "per_lane":  # any set_attr of a model field moves the env to the per-lane-model kernels; the stock values keep the physics
        from gymnasium_amd.envs.mujoco import compiler

        env.set_attr("gravity", compiler.compile_model(name).gravity)
    return env


def state_of(env):
    return np.array(env.get_state()[0]), env.get_rng_state().copy()


def check(label, name, rows, env, **want):
    values, words = report(label, name, rows, *state_of(env), **want)
    assert words, f"{name}, {label}: a branch of the sampler consumed another number of draws than NumPy's"
    assert values, f"{name}, {label}: reset state differs from NumPy's"


@pytest.mark.parametrize("name,model", [(n, "stock") for n in IDS] + [("half_cheetah", "per_lane")])
def test_reset_reproduces_the_rows(name, model, rows):
    env = make(name, model)
    env.reset(seed=0)
    env._engine.seed(rows[f"{name}_words"])
    env.reset()
    check(f"reset() [{model}]", name, rows, env)
    env.close()


def second_reset(name, rows):
    """What NumPy draws for the reset that follows the recorded one: (state rows, words afterwards).  Computed once per robot."""
    if name not in _SECOND:
        from gymnasium_amd import _native

        nq, nv, qpos0 = MK.ROBOTS[name]
        g = np.random.Generator(np.random.PCG64(0))
        state, after = np.empty((N, nq + nv)), np.empty((N, 4), dtype=np.uint64)
        for i in range(N):
            _native.set_pcg_words(g, rows[f"{name}_words_after"][i])
            state[i, :nq] = qpos0 + g.uniform(low=-MK.SCALE, high=MK.SCALE, size=nq)
            state[i, nq:] = MK.SCALE * g.standard_normal(nv)
            after[i] = _native.pcg_words(g)
        _SECOND[name] = (state, after)
    return _SECOND[name]


AUTORESET = [("half_cheetah", model, mode, api) for model in ("stock", "per_lane") for mode in ("NextStep", "SameStep") for api in ("step", "rollout")]
AUTORESET += [("ant", "stock", "NextStep", api) for api in ("step", "rollout")]


@pytest.mark.parametrize("name,model,mode,api", AUTORESET)
def test_autoreset_reproduces_the_rows(name, model, mode, api, rows):
    """max_episode_steps = 1: every step truncates every lane.  NEXT_STEP: the second step resets; SAME_STEP: the first one does (and the second one
    again, from the words the first left: rollout(2) then shows the recorded reset in its first observation row and ends on NumPy's next reset)."""
    nq, nv, _ = MK.ROBOTS[name]
    kw = dict(max_episode_steps=1, autoreset_mode=mode)
    label = f"{api} {mode} [{model}]"
    if api == "step":
        env = make(name, model, **kw)
        env.reset(seed=0)
        env._engine.seed(rows[f"{name}_words"])
        zero = np.zeros((N, env.single_action_space.shape[0]), dtype=np.float32)
        for _ in range(2 if mode == "NextStep" else 1):
            _, _, _, truncated, _ = env.step(zero)
        assert truncated.all() == (mode == "SameStep") and truncated.any() == (mode == "SameStep")
        check(label, name, rows, env)
    else:
        import torch

        env = make(name, model, output="torch", exclude_current_positions_from_observation=False, **kw)
        env.reset(seed=0)
        env._engine.seed(rows[f"{name}_words"])
        out = env.rollout(2, actions=torch.zeros((2, N, env.single_action_space.shape[0]), dtype=torch.float32, device="cuda"))
        if mode == "NextStep":
            assert out["truncations"][0].all() and not out["truncations"][1].any()
            check(label, name, rows, env)
        else:
            assert out["truncations"].all()
            first = out["obs"][0].cpu().numpy()[:, :nq + nv]  # the SAME_STEP observation of a finished lane is its reset observation: qpos | qvel
            bad = (first != expected_state(rows, name)).any(axis=1)
            print(f"normal sampler, {name}, {label}: first observation row differs from NumPy on {int(bad.sum())} lanes, by category "
                  f"{ {c: int((bad & category(rows, name, c)).sum()) for c in MK.CATEGORIES} }")
            state2, after2 = second_reset(name, rows)
            values, words = report(label + ", second reset", name, rows, *state_of(env), want_state=state2, want_after=after2)
            assert words and not bad.any() and values
    env.close()


@pytest.mark.parametrize("name", list(IDS))
def test_the_fixture_reaches_the_branches(name, rows):
    """A twin run whose tail lanes start one raw word later differs on exactly those lanes: the special word is the one consumed at index k.  (Compared
    with the first run, not with the fixture: this holds whatever the device's log1p returns.)"""
    nq, nv, _ = MK.ROBOTS[name]
    env = make(name)
    env.reset(seed=0)
    env._engine.seed(rows[f"{name}_words"])
    env.reset()
    first, _ = state_of(env)
    tails = category(rows, name, "tail", "tail_retry")
    words = rows[f"{name}_words"].copy()
    words[tails] = neighbour_words(words[tails])
    env._engine.seed(words)
    env.reset()
    twin, _ = state_of(env)
    assert np.array_equal((twin[:, :nq + nv] != first[:, :nq + nv]).any(axis=1), tails)
    k = rows[f"{name}_k"]
    assert (np.abs(first[np.arange(N), nq + k][tails]) > MK.SCALE * MK.R).all() and (np.abs(twin[np.arange(N), nq + k][tails]) < MK.SCALE * MK.R).sum() >= tails.sum() * 9 // 10
    env.close()
