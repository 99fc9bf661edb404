"""Backend-agnostic interleavings of every consumer of the action stream (gymnasium_amd/vector/device_policy.py) with replays of a graph of the
random policy (HipVectorEnv.capture_steps(policy="random")): ``sample()``, ``sample(mask=...)``, ``sample(probability=...)``, ``np_random``, ``rollout()``,
``step(None)``, ``step(sample())``, ``seed()``, ``reset(seed=...)``, copies of the space and ``GraphedSteps.replay()`` consume ONE PCG64 stream in call order.

Known answers, neither of them the code under test:

* values and position: the NumPy sampler of ``policy_suite.reference_space(env, seed)`` -- every operation below is modelled as "what it consumes from
  the reference space" (``sample()`` / ``sample(mask=...)`` / ``sample(probability=...)`` for values, ``np_random.random(k)`` for host draws,
  ``np_random.bit_generator.state`` for the position including the pending 32-bit half ``has_uint32`` / ``uinteger``);
* trajectories: a twin env on the ORACLE engine stepped with the reference space's batches -- ``array_equal`` for classic control, within the MuJoCo
  kinds' stated 1e-8 per window for Ant, the twin re-synchronised to the env's state after every operation (``set_state(*get_state())``).

``make_graph(env, steps)`` returns the object whose ``replay()`` runs ``steps`` sampled steps: on the GPU ``env.capture_steps(policy="random", steps=...)``,
on the CPU ``StandInGraph`` -- the product's own host hand-over (``GraphedSteps._prepare_capture`` / ``_before_replay`` / ``_after_replay``) around
engine-side ``step(None)`` calls that, like a graph launch, tell the space nothing.  ``make_graph=None`` removes the capture and replay operations from
every sequence.

Shapes (the smallest at which the lanes' skip-ahead can go wrong): CartPole-v1 (the draw fused into the step kernel, Discrete) and Pendulum-v1 (fused, Box)
at 300 sub-environments -- no multiple of 64, five wavefronts --, Ant-v5 at 129 (the stand-alone sampler, 8 draws per row, a partial group of 16-lane
robots); graphs of 3 steps and ``max_episode_steps=25``, so that autoresets fall inside replays.
"""
import copy
import pickle

import numpy as np

import gymnasium_amd
import policy_suite as ps
from gymnasium_amd import _native
from gymnasium_amd.vector.hip_vector_env import GraphedSteps

NUM_ENVS = {"CartPole-v1": 300, "Pendulum-v1": 300, "Ant-v5": 129}
G = 3
MAX_EPISODE_STEPS = 25
MJ_TOL = 1e-8  # the MuJoCo kinds' stated agreement with the oracle per re-synchronised window (tests/test_gpu_mujoco.py, tests/test_gpu_device_policy.py)


class CountingEngine:
    """An engine that notes the name of every method called on it (the hand-over's cost is counted in calls, not timed)."""

    def __init__(self, engine):
        object.__setattr__(self, "_e", engine)
        object.__setattr__(self, "calls", [])

    def __getattr__(self, name):
        value = getattr(self._e, name)
        if not callable(value) or name == "lib":
            return value

        def counted(*args, **kwargs):
            self.calls.append(name)
            return value(*args, **kwargs)

        return counted

    def __setattr__(self, name, value):
        setattr(self._e, name, value)


class StandInGraph(GraphedSteps):
    """GraphedSteps without a GPU: whatever the product does on the host around a capture and around ``graph.replay()`` is the product's own code;
    the launch itself is ``steps`` engine-side ``step(None)`` calls, which -- like the kernels of a replayed graph -- bypass the space."""

    def __init__(self, env, steps):
        self.env, self.steps, self.actions, self.policy = env, int(steps), None, "random"
        self.attr_mask = env._env_attr_mask
        self._capture()

    def _capture(self):
        env = self.env
        self.results = []
        self._prepare_capture()
        env._standin_ahead = 0
        if env.last_sampled_actions is None:
            t = env._torch
            env.last_sampled_actions = t.zeros(env._act_shape, dtype=t.int64 if env._discrete else t.float32, device=env._tdev)
        for _ in range(self.steps):  # the host side of the captured `env.step(None)` calls (nothing executes during a capture)
            env.action_space.hip_use_stream()

    def replay(self):
        env = self.env
        # The stand-in's OWN account of where the simulated lanes stand: ahead of the engine's copy by what the stand-in launches of this env drew
        # since the last hand-over.  A hand-over is due exactly when the space does not hold the account on entry (the one flag read here).
        held = env.action_space.__dict__.get("_hip_held", False)
        self._before_replay()
        ahead = env.__dict__.get("_standin_ahead", 0) if held else 0  # (a capture in between hands over too: _capture zeroes the account)
        raw = getattr(env._engine, "_e", env._engine)  # (a launch is not a call of the engine)
        self.results = []
        # A graph's kernels read and advance the per-lane states on the device and leave the engine's own copy of the position behind.  The oracle
        # has one position and no lanes: it stands in for the lanes during the launch and is moved back afterwards, so that, as on the device,
        # the engine has not seen any of the launches.
        raw.action_skip(ahead)
        for _ in range(self.steps):
            raw.step_bound(None, _native.MI_F32, env.last_sampled_actions.data_ptr())
            infos = env._build_infos()
            self.results.append((env._obs.clone(), env._rew.clone(), env._term.clone(), env._trunc.clone(), infos))
        ahead += self.steps * env.action_space._hip_batch_draws
        raw.action_skip(-ahead)
        env._standin_ahead = ahead
        return self._after_replay()


def gpu_graph(env, steps):
    return env.capture_steps(policy="random", steps=steps)


class Harness:
    """The env under test, the reference space and the oracle twin, and one method per operation: each performs the operation on the env, takes what it
    consumes from the reference space and compares."""

    def __init__(self, env_id, factory, oracle_factory, make_graph, seed=7, sample_output="torch", **kw):
        self.env_id, self.mj, self.make_graph = env_id, env_id.endswith("-v5"), make_graph
        n = NUM_ENVS[env_id]
        where = {"device": 0} if factory is None else {"_engine_factory": factory}
        self.env = gymnasium_amd.make_vec(env_id, num_envs=n, max_episode_steps=MAX_EPISODE_STEPS, output="torch", sample_output=sample_output, **where, **kw)
        self.twin = gymnasium_amd.make_vec(env_id, num_envs=n, max_episode_steps=MAX_EPISODE_STEPS, _engine_factory=oracle_factory, **kw)
        self.space = self.env.action_space
        self.discrete = self.env._discrete
        self.log = []
        self.inputs = np.random.default_rng(2024)  # the harness's own inputs: masks, probabilities, given actions
        self.reset(1)
        self.space.seed(seed)
        self.ref = ps.reference_space(self.env, seed)
        for _ in range(2):  # kernels load on first use, which a capture must not trigger
            self.step_none()
        self.log.clear()

    def close(self):
        if not self.env.closed:
            self.env.close()
        self.twin.close()

    # -- comparisons -----------------------------------------------------------------------------------------------------------------------
    def _same_values(self, got, want, what):
        got = ps._np(got)
        assert got.dtype == want.dtype and got.reshape(want.shape).shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
        assert np.array_equal(got.reshape(want.shape), want), f"{self.env_id}: {what} differs from the NumPy sampler"

    def _twin_step(self, got, act, what):
        """The twin steps with the reference's batch; ``got``: (obs, rewards, terminations, truncations) of the env for the same step."""
        c = self.twin.step(act)
        obs, rew = ps._np(got[0]), ps._np(got[1])
        if self.mj:
            np.testing.assert_allclose(obs, c[0], rtol=0, atol=MJ_TOL, err_msg=f"{self.env_id}: observations of {what}")
            np.testing.assert_allclose(rew, c[1], rtol=0, atol=MJ_TOL, err_msg=f"{self.env_id}: rewards of {what}")
        else:
            assert np.array_equal(obs, c[0]), f"{self.env_id}: observations of {what} differ from the oracle stepped with the NumPy sampler's batch"
            assert np.array_equal(rew, c[1]), f"{self.env_id}: rewards of {what} differ from the oracle stepped with the NumPy sampler's batch"
        assert np.array_equal(ps._np(got[2]), c[2]) and np.array_equal(ps._np(got[3]), c[3]), f"{self.env_id}: flags of {what}"

    def _resync(self):
        if self.mj:  # windowed comparison: chaotic dynamics amplify the last bits
            self.twin.set_state(*self.env.get_state())

    def check_position(self):
        """``np_random.bit_generator.state`` of the space == the reference's: the position and the pending 32-bit half."""
        got, want = self.space.np_random.bit_generator.state, self.ref.np_random.bit_generator.state
        assert got == want, f"{self.env_id}: the space's generator is not at the reference's position\n got {got}\nwant {want}"

    # -- the operations --------------------------------------------------------------------------------------------------------------------
    def sample(self):
        self.log.append("sample()")
        self._same_values(self.space.sample(), self.ref.sample(), "sample()")

    def _rows(self, weighted):
        n, a = self.env.num_envs, int(self.space.nvec.flat[0])
        if weighted:
            p = self.inputs.integers(0, 4, size=(n, a)).astype(np.float64)
            p[p.sum(1) == 0, 0] = 1.0
            return p / p.sum(1, keepdims=True)  # quarters, thirds, halves: rows that sum to 1 (np.isclose) with zeros among them
        return self.inputs.integers(0, 2, size=(n, a)).astype(np.int8)  # rows with no, one and two valid actions

    def sample_mask(self, device=False):
        self.log.append(f"sample(mask, device={device})")
        rows = self._rows(False)
        arg = self.env._torch.from_numpy(rows).to(self.env._tdev) if device else tuple(rows)
        self._same_values(self.space.sample(mask=arg), self.ref.sample(mask=tuple(rows)), "sample(mask=...)")

    def sample_probability(self):
        self.log.append("sample(probability)")
        rows = self._rows(True)
        self._same_values(self.space.sample(probability=rows), self.ref.sample(probability=tuple(rows)), "sample(probability=...)")

    def np_random(self, k=5):
        self.log.append(f"np_random.random({k})")
        got, want = self.space.np_random.random(k), self.ref.np_random.random(k)
        assert np.array_equal(got, want), f"{self.env_id}: np_random.random({k}) = {got}, the reference's {want}"
        self.check_position()

    def rollout(self, T=6):
        self.log.append(f"rollout({T})")
        out = self.env.rollout(T)
        for t in range(T):
            act = self.ref.sample()
            self._same_values(out["actions"][t], act, f"rollout({T}) actions[{t}]")
            self._twin_step((out["obs"][t], out["rewards"][t], out["terminations"][t], out["truncations"][t]), act, f"rollout({T}) step {t}")
        self._resync()

    def rollout_given(self, T=6):
        """rollout(T, actions): consumes nothing from the stream."""
        self.log.append(f"rollout({T}, actions)")
        n = self.env.num_envs
        if self.discrete:
            acts = self.inputs.integers(0, int(self.space.nvec.flat[0]), size=(T, n)).astype(np.int64)
        else:
            lo, hi = self.space.low, self.space.high
            acts = (lo + (hi - lo) * self.inputs.random((T,) + lo.shape)).astype(np.float32)
        out = self.env.rollout(T, self.env._torch.from_numpy(acts).to(self.env._tdev))
        for t in range(T):
            self._twin_step((out["obs"][t], out["rewards"][t], out["terminations"][t], out["truncations"][t]), acts[t], f"rollout({T}, actions) step {t}")
        self._resync()

    def step_none(self):
        self.log.append("step(None)")
        got = self.env.step(None)
        act = self.ref.sample()
        self._same_values(self.env.last_sampled_actions, act, "the batch step(None) drew")
        self._twin_step(got, act, "step(None)")
        self._resync()

    def step_sample(self):
        self.log.append("step(sample())")
        a, act = self.space.sample(), self.ref.sample()
        self._same_values(a, act, "sample() for step()")
        self._twin_step(self.env.step(a), act, "step(sample())")
        self._resync()

    def seed(self, s):
        self.log.append(f"seed({s})")
        self.space.seed(s), self.ref.seed(s)

    def reset(self, s):
        """env.reset(seed=...): the sub-environments' generators, not the action stream."""
        self.log.append(f"reset(seed={s})")
        o, _ = self.env.reset(seed=s)
        c, _ = self.twin.reset(seed=s)
        if self.mj:
            np.testing.assert_allclose(ps._np(o), c, rtol=0, atol=1e-12, err_msg=f"{self.env_id}: reset(seed={s})")
            self._resync()
        else:
            assert np.array_equal(ps._np(o), c), f"{self.env_id}: reset(seed={s})"

    def capture(self, steps=G):
        if self.make_graph is None:
            return None
        self.log.append(f"capture({steps})")
        return self.make_graph(self.env, steps)

    def replay(self, g):
        """graph.replay(): consumes ``g.steps`` batches."""
        if g is None:
            return
        self.log.append(f"replay({g.steps})")
        g.replay()
        act = None
        for k in range(g.steps):  # (copy=True: every captured step has its own result tensors)
            act = self.ref.sample()
            self._twin_step(g.results[k], act, f"replay step {k} of {g.steps}")
        self._same_values(self.env.last_sampled_actions, act, "the last batch of the replay")
        self._resync()

    def copies(self):
        """deepcopy / pickle detach at the position and continue on the host; the space itself continues too (one batch each)."""
        self.log.append("deepcopy / pickle")
        dup, pk = copy.deepcopy(self.space), pickle.loads(pickle.dumps(self.space))
        want = self.ref.sample()
        self._same_values(dup.sample(), want, "sample() of a deepcopy")
        self._same_values(pk.sample(), want, "sample() of a pickled copy")
        self._same_values(self.space.sample(), want, "sample() after copying")


def run(harness, sequence):
    """Run ``sequence(harness)``; a failure names the operations that led to it."""
    try:
        sequence(harness)
    except Exception as e:
        raise AssertionError(f"{harness.env_id} after {harness.log}: {type(e).__name__}: {e}") from e
    finally:
        harness.close()


# -- the named sequences: a replay on both sides of the other operation -----------------------------------------------------------------------
def seq1_host_draw(h):
    g = h.capture()
    h.replay(g), h.np_random(5), h.replay(g), h.sample()


def seq2_ring(h):
    h.space._hip_ring_steps = 4  # a sample() draws three batches ahead
    g = h.capture()
    h.replay(g), h.sample(), h.replay(g), h.sample()
    for _ in range(3):  # exactly four sample() calls since the refill: the ring is exhausted
        h.sample()
    h.replay(g), h.sample(), h.replay(g), h.sample()
    h.check_position()


def seq3_seed(h):
    g = h.capture()
    h.replay(g), h.seed(99), h.replay(g), h.sample()


def seq4_rollout(h):
    """CartPole / Pendulum: the rollout keeps the lanes current; Ant: it invalidates them."""
    g = h.capture()
    h.replay(g), h.rollout(6), h.replay(g), h.sample()


def seq5_rollout_given(h):
    g = h.capture()
    h.replay(g), h.rollout_given(6), h.replay(g)
    h.check_position()


def seq6_eager_steps(h):
    g = h.capture()
    h.replay(g), h.step_none(), h.replay(g), h.step_sample(), h.replay(g)
    h.check_position()


def seq7_masked(h):
    """CartPole: masked and weighted draws consume 32-bit halves; the pending one travels through the replay."""
    g = h.capture()
    h.replay(g), h.sample_mask(), h.sample_mask(device=True), h.sample_probability(), h.replay(g), h.np_random(1)
    h.sample()


def seq8_two_graphs(h):
    g1, g3 = h.capture(1), h.capture(3)
    for _ in range(2):
        h.replay(g1), h.replay(g3)
    h.replay(g3), h.replay(g1), h.sample()
    h.space._hip_ring_steps = 4
    h.sample()  # the ring holds three batches drawn ahead ...
    g2 = h.capture(2)  # ... while a further graph is captured
    h.replay(g2), h.replay(g1), h.sample()
    h.check_position()


def seq11_seed_two_graphs(h):
    """Two graphs and a seed(): BOTH carry the old increment's jump; the one replayed second finds the stream already handed over."""
    g1, g3 = h.capture(1), h.capture(3)
    h.replay(g1), h.replay(g3)
    h.seed(99)
    h.replay(g1), h.replay(g3), h.sample()
    h.seed(5)
    h.replay(g3), h.replay(g1), h.replay(g3), h.np_random(2), h.replay(g1), h.sample()
    h.check_position()


def seq9_copies(h):
    g = h.capture()
    h.replay(g), h.copies(), h.replay(g), h.np_random(2), h.replay(g)
    space = h.space
    h.env.close()  # the space outlives the env with its generator at the stream's position
    h.log.append("close()")
    h._same_values(space.sample(), h.ref.sample(), "sample() of the surviving space")
    assert space.np_random.bit_generator.state == h.ref.np_random.bit_generator.state


def seq10_clip_action(h):
    """Through wrappers.ClipAction: its own capture_steps(policy="random") is refused (the wrapper's space is sampled on the host) without touching the
    stream; the wrapped env's graph goes through sequences 1 and 3."""
    import pytest

    from gymnasium_amd import wrappers
    from gymnasium_amd.gym_api import error

    w = wrappers.ClipAction(h.env)
    with pytest.raises(error.Error, match="not sampled on the device"):
        w.capture_steps(policy="random", steps=G)
    h.sample()
    g = None if h.make_graph is None else h.make_graph(w.env, G)
    h.replay(g), h.np_random(5), h.replay(g), h.sample()
    h.replay(g), h.seed(99), h.replay(g), h.sample()


NAMED = {"1-np_random": seq1_host_draw, "2-ring": seq2_ring, "3-seed": seq3_seed, "4-rollout": seq4_rollout, "5-rollout-given": seq5_rollout_given,
         "6-eager-steps": seq6_eager_steps, "8-two-graphs": seq8_two_graphs, "9-copies-close": seq9_copies, "11-seed-two-graphs": seq11_seed_two_graphs}
ENV_IDS = ["CartPole-v1", "Pendulum-v1", "Ant-v5"]


# -- seeded random sequences --------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = (0, 1, 2)
RANDOM_LENGTH = 30


def random_sequence(seed, length=RANDOM_LENGTH):
    """``length`` operations drawn from the whole list; replays make up about a third."""

    def sequence(h):
        pick = np.random.default_rng(seed)
        graphs = [h.capture(G)]
        ops = ["sample", "np_random", "rollout", "rollout_given", "step_none", "step_sample", "seed", "reset", "capture", "copies"] + ["replay"] * 5
        if h.discrete:
            ops += ["mask_host", "mask_device", "probability"]
        for _ in range(length):
            op = ops[int(pick.integers(len(ops)))]
            if op == "replay":
                h.replay(graphs[int(pick.integers(len(graphs)))])
            elif op == "capture":
                if len(graphs) < 3:
                    graphs.append(h.capture(int(pick.integers(1, 4))))
            elif op == "np_random":
                h.np_random(int(pick.integers(1, 6)))
            elif op in ("rollout", "rollout_given"):
                getattr(h, op)(int(pick.integers(1, 7)))
            elif op in ("seed", "reset"):
                getattr(h, op)(int(pick.integers(1000)))
            elif op == "mask_host":
                h.sample_mask()
            elif op == "mask_device":
                h.sample_mask(device=True)
            elif op == "probability":
                h.sample_probability()
            else:
                getattr(h, op)()
        h.sample()
        h.check_position()

    return sequence


# -- the cost of the common case ----------------------------------------------------------------------------------------------------------------
def check_back_to_back_replays_call_nothing(h):
    """Back-to-back replays are launch-bound: after the first one the hand-over makes NO engine call (hence no synchronisation); the first replay after
    another consumer does make some, and the stream still comes out right."""
    g = h.capture()
    h.replay(g)
    counting = h.env._engine = CountingEngine(h.env._engine)
    for _ in range(5):
        g.replay()
    assert counting.calls == [], f"back-to-back replays called the engine: {counting.calls}"
    h.env._engine = counting._e
    for _ in range(5 * g.steps):  # (what the five uncompared replays consumed; the twin follows them)
        h.twin.step(h.ref.sample())
    h._resync()
    h.np_random(1)
    counting = h.env._engine = CountingEngine(h.env._engine)
    g.replay()
    assert "action_sample" in counting.calls, counting.calls  # (the counter sees the hand-over when there is one)
    del counting.calls[:]
    g.replay()
    assert counting.calls == [], counting.calls
    h.env._engine = counting._e
    for _ in range(2 * g.steps):
        h.twin.step(h.ref.sample())
    h._resync()
    h.replay(g), h.sample()
    h.check_position()
