"""CPU side of ``rollout(T, infos=True)`` (the GPU side: tests/test_gpu_rollout_infos.py): the refusals, the keyword's way through the wrapper
stack, the queue logic of ``RecordEpisodeStatistics.rollout`` on a hand-made infos dict, the ABI declaration, and that the seeds of
tests/rollout_infos_cases.py satisfy the guards of the GPU comparison on the checker backend (T ``step()`` calls; the checker has no fused
rollout with infos, which is what the refusal test pins)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import gymnasium_amd
import rollout_infos_cases as cases
from conftest import ROOT
from gymnasium_amd import wrappers as gw
from gymnasium_amd.gym_api import error


# -- refusals and plumbing -------------------------------------------------------------------------------------------------------------------
def test_infos_with_numpy_output_is_refused_like_rollout_itself(oracle_factory):
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=4, _engine_factory=oracle_factory)
    env.reset(seed=0)
    with pytest.raises(error.Error, match="output='torch'") as plain:
        env.rollout(3)
    with pytest.raises(error.Error, match="output='torch'") as with_infos:
        env.rollout(3, infos=True)
    assert str(plain.value) == str(with_infos.value)
    env.close()


def test_a_backend_without_the_entry_point_refuses_and_stays_untouched(oracle_factory):
    """No quiet fall-back to T step() calls: a backend without mi_rollout_infos says so, before anything moved."""
    a = gymnasium_amd.make_vec("CartPole-v1", num_envs=4, output="torch", autoreset_mode="SameStep", _engine_factory=oracle_factory)
    b = gymnasium_amd.make_vec("CartPole-v1", num_envs=4, output="torch", autoreset_mode="SameStep", _engine_factory=oracle_factory)
    a.reset(seed=1), b.reset(seed=1)
    a.action_space.seed(2), b.action_space.seed(2)
    with pytest.raises(error.Error, match="mi_rollout_infos"):
        a.rollout(5, infos=True)
    oa, ob = a.rollout(5), b.rollout(5)  # the refused call consumed nothing: neither env state nor action stream
    assert set(oa) == {"obs", "rewards", "terminations", "truncations", "actions"}, "the default returns exactly the keys it always returned"
    for k in oa:
        assert np.array_equal(oa[k].numpy(), ob[k].numpy()), k
    a.close(), b.close()


def test_the_keyword_reaches_the_env_through_the_wrapper_stack(oracle_factory):
    """RecordEpisodeStatistics.rollout asks the env for the infos whatever the caller passed; the wrappers above hand keywords down unchanged."""
    env = gymnasium_amd.make_vec("CartPole-v1", num_envs=4, _engine_factory=oracle_factory)
    stack = gw.ClipReward(gw.NumpyToTorch(gw.RecordEpisodeStatistics(env), device="cpu"), min_reward=0.0, max_reward=0.5)
    stack.reset(seed=0)
    for kw in ({}, {"infos": False}, {"infos": True}, {"return_actions": False}):
        with pytest.raises(error.Error, match="mi_rollout_infos"):
            stack.rollout(4, **kw)
    with pytest.raises(error.Error, match="mi_rollout_infos"):
        gw.NumpyToTorch(env, device="cpu").rollout(4, infos=True)
    assert set(gw.NumpyToTorch(env, device="cpu").rollout(4)) == {"obs", "rewards", "terminations", "truncations", "actions"}
    env.close()


# -- RecordEpisodeStatistics.rollout on a hand-made infos dict --------------------------------------------------------------------------------
class _StubEnv:
    """What RecordEpisodeStatistics needs of the env underneath, with a rollout that returns a prepared dict and records its keywords."""

    num_envs = 3

    def __init__(self, infos):
        self.infos, self.calls = infos, []

    @property
    def unwrapped(self):
        return self

    def enable_episode_statistics(self):
        pass

    def rollout(self, num_steps, actions=None, **kwargs):
        self.calls.append((num_steps, actions, dict(kwargs)))
        out = {"obs": np.zeros((num_steps, 3, 1)), "rewards": np.zeros((num_steps, 3))}
        if kwargs.get("infos"):
            out["infos"] = self.infos
        return out


def _handmade():
    mask = np.array([[0, 0, 1], [1, 0, 1], [0, 0, 0], [1, 1, 1]], dtype=bool)  # [T = 4, N = 3]
    r = np.arange(12, dtype=np.float64).reshape(4, 3) + 100.0
    ln = np.arange(12, dtype=np.int64).reshape(4, 3) + 1
    tt = np.arange(12, dtype=np.float64).reshape(4, 3) / 8.0
    ep = {"r": np.where(mask, r, 0.0), "l": np.where(mask, ln, 0), "t": np.where(mask, tt, 0.0)}
    return {"episode": ep, "_episode": mask, "x_position": np.ones((4, 3)), "_x_position": np.ones((4, 3), dtype=bool)}, mask, r, ln, tt


def test_queues_take_the_finished_episodes_step_by_step_then_by_sub_environment():
    infos, mask, r, ln, tt = _handmade()
    stub = _StubEnv(infos)
    w = gw.RecordEpisodeStatistics(stub)
    assert "infos" not in w.rollout(4, None, infos=False, return_actions=False), "the bare trajectory unless the caller asks"
    assert stub.calls == [(4, None, {"infos": True, "return_actions": False})], "the env underneath is always asked for the infos"
    w.return_queue.clear(), w.length_queue.clear(), w.time_queue.clear()
    out = w.rollout(4, infos=True)
    order = [(t, i) for t in range(4) for i in range(3) if mask[t, i]]  # the order T step() calls find them in
    assert order == [(0, 2), (1, 0), (1, 2), (3, 0), (3, 1), (3, 2)]
    assert list(w.return_queue) == [r[c] for c in order] and list(w.length_queue) == [ln[c] for c in order] and list(w.time_queue) == [tt[c] for c in order]
    assert set(out["infos"]) == {"episode", "_episode", "x_position", "_x_position"} and out["infos"]["episode"] is infos["episode"]
    assert "episode" in infos, "the dict the env returned is not edited in place"
    w.rollout(4)  # a further call appends, also without the keyword
    assert len(w.return_queue) == 12 and list(w.return_queue)[6:] == [r[c] for c in order]


def test_short_queues_and_a_stats_key_of_the_callers():
    infos, mask, r, ln, _ = _handmade()
    w = gw.RecordEpisodeStatistics(_StubEnv(infos), buffer_length=4, stats_key="ep")
    out = w.rollout(4, infos=True)
    order = [(t, i) for t in range(4) for i in range(3) if mask[t, i]][-4:]
    assert list(w.return_queue) == [r[c] for c in order] and list(w.length_queue) == [ln[c] for c in order] and len(w.time_queue) == 4
    assert "episode" not in out["infos"] and "_episode" not in out["infos"]
    assert out["infos"]["ep"] is infos["episode"] and np.array_equal(out["infos"]["_ep"], mask)


def test_a_key_clash_raises_like_step():
    infos, *_ = _handmade()
    w = gw.RecordEpisodeStatistics(_StubEnv(infos), stats_key="x_position")
    with pytest.raises(ValueError, match="Attempted to add episode stats with key 'x_position'"):
        w.rollout(4)
    assert len(w.return_queue) == 0


def test_a_rollout_without_finished_episodes_leaves_the_queues_alone():
    infos, mask, *_ = _handmade()
    infos["_episode"] = np.zeros_like(mask)
    w = gw.RecordEpisodeStatistics(_StubEnv(infos))
    out = w.rollout(4, infos=True)
    assert len(w.return_queue) == len(w.length_queue) == len(w.time_queue) == 0 and "_episode" in out["infos"]


# -- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_rollout_extra_struct_matches_the_header(tmp_path):
    from gymnasium_amd import _native as n

    assert n.ABI_VERSION == 10 and "rollout_infos" in n.HOST_SYMBOLS and "rollout_infos" not in n.SYMBOLS  # (the checker library does not have it)
    assert ctypes.sizeof(n.MiRolloutExtra) == 5 * 8
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler to cross-check the offsets with")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "mi355env.h")}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(mi_rollout_extra));']
    lines += [f'printf("{name} %zu\\n", offsetof(mi_rollout_extra, {name}));' for name, _ in n.MiRolloutExtra._fields_]
    lines.append("int (*f)(mi_vecenv *, int, const mi_rollout_io *, const mi_rollout_extra *) = mi_rollout_infos; (void)f; return 0; }")
    (tmp_path / "extra.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-c", "-o", str(tmp_path / "extra.o"), str(tmp_path / "extra.c")], check=True)  # (the prototype has the declared type)
    lines[-1] = "return 0; }"
    (tmp_path / "extra.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-o", str(tmp_path / "extra"), str(tmp_path / "extra.c")], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path / "extra")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(n.MiRolloutExtra)
    for name, _ in n.MiRolloutExtra._fields_:
        assert int(out[name]) == getattr(n.MiRolloutExtra, name).offset, name


# -- the seeds of the GPU comparison satisfy its guards (checker backend, T step() calls) -------------------------------------------------------
def _guards_on_the_checker(factory, env_id, n, T, mes, mode, caller, both_flags=False):
    a, b = cases.make_pair(env_id, n, mes, mode, True, factory)
    (obs, rew, te, tr, act), infos = cases.stack_steps(a, T, cases.caller_actions(a, T) if caller else None)
    masks = {}
    cases.compare_infos(infos, infos, False, masks=masks)
    cases.assert_guards(a, (te | tr).numpy(), masks, te.numpy(), tr.numpy(), both_flags)
    a.close(), b.close()


@pytest.mark.parametrize("caller", [True, False], ids=["caller_actions", "device_policy"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.CLASSIC_CASES + [cases.CARTPOLE_LONG], ids=lambda c: f"{c[0]}-T{c[2]}")
def test_classic_seeds_satisfy_the_guards(case, mode, caller, oracle_factory):
    _guards_on_the_checker(oracle_factory, *case, mode, caller, both_flags=case is cases.CARTPOLE_LONG)


@pytest.mark.parametrize("caller", [True, False], ids=["caller_actions", "device_policy"])
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("case", cases.MUJOCO_CASES, ids=lambda c: c[0])
def test_mujoco_seeds_satisfy_the_guards(case, mode, caller, oracle_factory):
    _guards_on_the_checker(oracle_factory, *case, mode, caller)
