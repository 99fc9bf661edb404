"""-m gpu: the on-device policy's per-lane states kept across launches.

The classic kinds' sampling rollouts (rollout_kernel, rollout_duo_kernel) start from the per-lane states of the action stream when they are
current and leave them current for the next launch (engine_types.h ActionStream::lane; mi_action_seed prepares them); the first launch after
mi_action_skip or after a captured launch, and one inside a stream capture, skips ahead from the host copy instead.  Every sequence below mixes the consumers of the one stream -- rollout(),
sample(), step(None), np_random, seed(), a skip, a captured launch -- and is checked bit for bit against the oracle stepped with the NumPy
sampler of the same seeded space."""
import numpy as np
import pytest

import gymnasium_amd
import policy_suite as ps

pytestmark = pytest.mark.gpu

DUO = ["CartPole-v1", "Pendulum-v1", "MountainCar-v0", "MountainCarContinuous-v0"]


class Pair:
    """The GPU env (output="torch") and the oracle, reset alike, with the reference sampler of the GPU env's seeded space."""

    def __init__(self, env_id, n, oracle_factory, **kw):
        self.gpu = gymnasium_amd.make_vec(env_id, num_envs=n, device=0, output="torch", sample_output="torch", **kw)
        self.cpu = gymnasium_amd.make_vec(env_id, num_envs=n, _engine_factory=oracle_factory, **kw)
        og, _ = self.gpu.reset(seed=5)
        oc, _ = self.cpu.reset(seed=5)
        assert np.array_equal(ps._np(og), oc)
        self.gpu.action_space.seed(3)
        self.ref = ps.reference_space(self.gpu, 3)
        self.env_id = env_id

    def expect_step(self, g, act, what):
        c = self.cpu.step(act)
        for k in range(4):
            assert np.array_equal(ps._np(g[k]), c[k]), (self.env_id, what, k)

    def rollout(self, T, what):
        out = self.gpu.rollout(T)
        acts = ps._np(out["actions"])
        for t in range(T):
            act = self.ref.sample()
            assert np.array_equal(acts[t].reshape(act.shape), act), (self.env_id, what, t)
            c = self.cpu.step(act)
            for k, name in enumerate(("obs", "rewards", "terminations", "truncations")):
                assert np.array_equal(ps._np(out[name][t]), c[k]), (self.env_id, what, name, t)

    def step_sample(self, what):
        act = self.gpu.action_space.sample()
        want = self.ref.sample()
        assert np.array_equal(ps._np(act).reshape(want.shape), want), (self.env_id, what)
        self.expect_step(self.gpu.step(act), want, what)

    def step_none(self, what):
        g = self.gpu.step(None)
        want = self.ref.sample()
        assert np.array_equal(ps._np(self.gpu.last_sampled_actions).reshape(want.shape), want), (self.env_id, what)
        self.expect_step(g, want, what)

    def finish(self):
        st_g, st_c = self.gpu.get_state(), self.cpu.get_state()
        for x, y in zip(st_g[:2], st_c[:2]):  # (the state words and the TimeLimit counters)
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert np.array_equal(ps._np(self.gpu.action_space.sample()), self.ref.sample())
        self.gpu.close(), self.cpu.close()


@pytest.mark.parametrize("env_id", DUO + ["Acrobot-v1"])
def test_rollout_rollout_sample_step_rollout(env_id, oracle_factory):
    p = Pair(env_id, 1000, oracle_factory)
    p.rollout(16, "first (lanes from the seed)")
    p.rollout(16, "second (lanes)")
    p.step_sample("step(sample())")  # sample() draws batches ahead; the next rollout gives them back (mi_action_skip)
    p.rollout(16, "after sample")
    p.step_none("step(None) 1")  # the position moves to the device ...
    p.step_none("step(None) 2")
    p.rollout(16, "after step(None)")  # ... and the rollout starts from the lanes without reading it back
    p.rollout(8, "last")
    p.finish()


@pytest.mark.parametrize("env_id", ["CartPole-v1", "MountainCarContinuous-v0"])
def test_rollout_np_random_sample(env_id, oracle_factory):
    p = Pair(env_id, 1000, oracle_factory)
    p.rollout(16, "first")
    p.rollout(16, "second")
    assert np.array_equal(p.gpu.action_space.np_random.random(5), p.ref.np_random.random(5))
    p.step_sample("sample after np_random")
    p.rollout(16, "after np_random")
    p.finish()


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Pendulum-v1"])
def test_seed_then_rollout(env_id, oracle_factory):
    p = Pair(env_id, 1000, oracle_factory)
    p.rollout(16, "first")
    p.gpu.action_space.seed(99), p.ref.seed(99)
    p.rollout(16, "after seed")
    p.rollout(16, "after seed, lanes")
    p.gpu.action_space.seed(99), p.ref.seed(99)  # the same seed again (same increment: the seed keeps its jump table, re-prepares the lanes)
    p.rollout(8, "same seed again")
    p.finish()


@pytest.mark.parametrize("env_id", ["CartPole-v1", "MountainCar-v0"])
def test_action_skip_between_rollouts(env_id, oracle_factory):
    p = Pair(env_id, 1000, oracle_factory)
    p.rollout(16, "first")
    p.rollout(16, "second")
    eng = p.gpu.action_space.hip_use_stream()
    for k in (1, 3 * 1000 + 17):
        eng.action_skip(k)
        p.ref.np_random.bit_generator.advance(k)
        p.rollout(16, f"after skip {k}")
        p.rollout(8, f"after skip {k}, lanes")
    p.finish()


def test_chunk_does_not_divide_T(oracle_factory):
    """T = 13: the one-role kernel, which keeps the lanes as well -- mixed with two-role launches in both orders."""
    p = Pair("CartPole-v1", 1000, oracle_factory)
    p.rollout(13, "one role (lanes from the seed)")
    p.rollout(13, "one role (lanes)")
    p.rollout(16, "two roles after one role")
    p.rollout(5, "one role after two roles")
    p.finish()


@pytest.mark.parametrize("n", [1, 63, 300, 4097])
def test_batches_that_are_not_whole_workgroups(n, oracle_factory):
    p = Pair("CartPole-v1", n, oracle_factory, max_episode_steps=9)
    for r in range(3):
        p.rollout(8, f"launch {r}")
    p.finish()


def test_rollout_captured_in_a_graph(oracle_factory):
    """A rollout enqueued inside a stream capture keeps the old contract: it skips ahead from the host copy baked into the graph and leaves
    the lanes alone (they are stale from then on).  Eager launches before and after it, one replay in between."""
    import torch

    from gymnasium_amd import _native

    n, T = 1000, 16
    p = Pair("CartPole-v1", n, oracle_factory)
    p.rollout(T, "eager (lanes from the seed)")
    p.rollout(T, "eager (lanes)")
    gpu = p.gpu
    eng = gpu.action_space.hip_use_stream()
    acts = torch.empty((T, n), dtype=torch.int64, device="cuda:0")
    obs = torch.empty((T, n, 4), dtype=torch.float32, device="cuda:0")
    rew = torch.empty((T, n), dtype=torch.float64, device="cuda:0")
    te = torch.empty((T, n), dtype=torch.bool, device="cuda:0")
    tr = torch.empty((T, n), dtype=torch.bool, device="cuda:0")
    gpu.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            gpu._stream_bound = None
            gpu._bind_stream()
            eng.rollout(T, None, acts.data_ptr(), obs.data_ptr(), rew.data_ptr(), te.data_ptr(), tr.data_ptr(), actions_in_dtype=_native.MI_F32)
    finally:
        gpu._stream_bound = None
        gpu._bind_stream()
    graph.replay()
    torch.cuda.synchronize()
    for t in range(T):
        act = p.ref.sample()
        assert np.array_equal(acts[t].cpu().numpy(), act), t
        c = p.cpu.step(act)
        for k, x in enumerate((obs, rew, te, tr)):
            assert np.array_equal(x[t].cpu().numpy(), c[k]), (k, t)
    # (the engine's own step state moved by T steps in the replay; the Python env's "current" buffers did not -- not used below)
    p.rollout(T, "eager after the captured launch (skip-ahead)")
    p.rollout(T, "eager after that (lanes)")
    p.finish()
