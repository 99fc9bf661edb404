"""-m gpu: the env role's episode bookkeeping of the two-role CartPole rollout (classic_kernels.h duo_env_step_word: pending autoreset, TimeLimit
counter and the reset queue's flag in one word, episode_word.h; a chunk's eight steps without a loop around them) and the one-compare range test of
the short sin / cos routine -- every output against the one-role kernel (MI355ENV_ROLLOUT_DUO=0) and against the oracle, array_equal: the
trajectory, get_state(), get_rng_state(), statistics(), the policy's actions and where its stream stands afterwards.

Sizes below, at and above a wavefront and a workgroup of 256 sub-environments; one, two and three chunks of 8 steps per launch; three consecutive
launches, so that the word is rebuilt from `meta` with pending lanes; TimeLimits of 1, 2 and 3 steps (a lane refills its reset queue twice within a
chunk) and a TimeLimit that is off (the threshold no word reaches).  CartPole is the only environment that takes these cuts."""
import os

import numpy as np
import pytest

import gymnasium_amd

pytestmark = pytest.mark.gpu
ENV_ID = "CartPole-v1"
LAUNCHES = 3
KEYS = ("obs", "rewards", "terminations", "truncations")


def same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")


def prepare(env, prep, gpu):
    """What happens between reset() and the first launch: `prep(env, step)` with a step() that takes host actions."""
    if prep is None:
        return

    def step(a):
        if gpu:
            import torch

            a = torch.from_numpy(a).cuda()
        return env.step(a)

    prep(env, step)


def device_run(duo, n, T, kw, prep=None):
    old = os.environ.get("MI355ENV_ROLLOUT_DUO")
    os.environ["MI355ENV_ROLLOUT_DUO"] = "1" if duo else "0"
    try:
        env = gymnasium_amd.make_vec(ENV_ID, num_envs=n, device=0, output="torch", **kw)
        env.reset(seed=7)
        env.action_space.seed(11)
        prepare(env, prep, True)
        outs = [{k: v.cpu().numpy() for k, v in env.rollout(T).items()} for _ in range(LAUNCHES)]
        res = dict(outs=outs, state=[np.asarray(x).copy() for x in env.get_state()], rng=env.get_rng_state().copy(), stats=env.statistics(),
                   next_action=np.asarray(env.action_space.sample()).copy())
        env.close()
        return res
    finally:
        if old is None:
            os.environ.pop("MI355ENV_ROLLOUT_DUO", None)
        else:
            os.environ["MI355ENV_ROLLOUT_DUO"] = old


def oracle_run(n, T, kw, prep=None):
    """The same calls on the oracle: step(action_space.sample()) on the host, T x LAUNCHES times."""
    from oracle import oracle

    env = gymnasium_amd.make_vec(ENV_ID, num_envs=n, _engine_factory=oracle.engine_factory, **kw)
    env.reset(seed=7)
    env.action_space.seed(11)
    prepare(env, prep, False)
    outs = []
    for _ in range(LAUNCHES):
        rows = {k: [] for k in KEYS + ("actions",)}
        for _ in range(T):
            a = env.action_space.sample()
            r = env.step(a)
            rows["actions"].append(np.asarray(a).copy())
            for j, k in enumerate(KEYS):
                rows[k].append(np.asarray(r[j]).copy())
        outs.append({k: np.stack(v) for k, v in rows.items()})
    res = dict(outs=outs, state=[np.asarray(x).copy() for x in env.get_state()], rng=env.get_rng_state().copy(), stats=env.statistics(),
               next_action=np.asarray(env.action_space.sample()).copy())
    env.close()
    return res


def check(n, T, kw, prep=None):
    duo, one, ref = device_run(True, n, T, kw, prep), device_run(False, n, T, kw, prep), oracle_run(n, T, kw, prep)
    for name, other in (("one-role kernel", one), ("oracle", ref)):
        for launch, (a, b) in enumerate(zip(duo["outs"], other["outs"])):
            assert set(a) == set(b)
            for k in a:
                assert same(a[k].reshape(b[k].shape), b[k].astype(a[k].dtype) if k == "actions" else b[k]), (name, "launch", launch, k, kw)
        for j, (x, y) in enumerate(zip(duo["state"], other["state"])):
            assert same(x, y), (name, "get_state", j, kw)
        assert same(duo["rng"], other["rng"]), (name, "get_rng_state", kw)
        for k in ("env_steps", "reset_steps", "episodes", "length_sum", "return_sum"):  # (CartPole's returns are sums of +-1 and 0: exact in any order)
            assert duo["stats"][k] == other["stats"][k], (name, "statistics", k, kw)
        # the policy stream continues where the launches left it (its actions inside the launches: the "actions" rows above, against the host's sample())
        assert same(duo["next_action"], other["next_action"].astype(duo["next_action"].dtype)), (name, "the next action_space.sample()", kw)
    assert duo["stats"]["env_steps"] + duo["stats"]["reset_steps"] >= n * T * LAUNCHES
    return duo


@pytest.mark.parametrize("T", [8, 16, 24])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_every_output_equals_the_one_role_kernel_and_the_oracle(n, T):
    for max_episode_steps in (1, 2, 3, 0):
        duo = check(n, T, {"max_episode_steps": max_episode_steps})
        if max_episode_steps:
            assert duo["stats"]["episodes"] >= n * (T * LAUNCHES // (max_episode_steps + 1) - 1)
            assert duo["outs"][0]["truncations"].any()
        else:
            assert not any(o["truncations"].any() for o in duo["outs"])


def test_a_launch_after_five_calls_of_step():
    def prep(env, step):
        for _ in range(5):
            step(env.action_space.sample())

    for kw in ({"max_episode_steps": 3}, {}):
        check(257, 16, kw, prep)


def test_terminated_and_truncated_in_the_same_step():
    """x just inside 2.4 with outward velocity under max_episode_steps=1: the first step raises both flags, the second is the reset."""
    n = 257

    def prep(env, step):
        s = np.zeros((n, 4))
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        s[:, 0] = sign * np.nextafter(2.4, 0.0)
        s[:, 1] = sign * 3.0
        s[::5, 1] = 0.0  # (some lanes stay inside: truncated alone)
        env.set_state(s, np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8))

    duo = check(n, 16, {"max_episode_steps": 1}, prep)
    first = duo["outs"][0]
    moving = np.arange(n) % 5 != 0
    assert first["terminations"][0][moving].all() and not first["terminations"][0][~moving].any() and first["truncations"][0].all()
    assert not first["terminations"][1].any() and not first["truncations"][1].any()  # the autoreset step


def test_angles_outside_the_short_routine_and_nan_angles():
    """|theta| >= 0.856 (both sides of the one-compare range test's constant 0.85546875, from the doubles next to it outwards) and NaN angles in some
    lanes: those lanes take the general routines.  With the TimeLimit off nothing ends a NaN lane's episode, so it keeps the general path busy."""
    n = 257

    def prep(env, step):
        rng = np.random.default_rng(3)
        s = rng.uniform(-0.05, 0.05, (n, 4))
        edge = 0.85546875
        wide = np.array([edge, np.nextafter(edge, 1.0), np.nextafter(edge, 0.0), 0.856, 0.9, 1.5, 3.0, 100.0, 1e5])
        k = np.arange(n)
        pick = k % 3 == 0
        s[pick, 2] = (wide[(k // 3) % wide.size] * np.where(k % 2 == 0, 1.0, -1.0))[pick]
        s[k % 16 == 5, 2] = np.nan
        env.set_state(s, np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8))

    for kw in ({"max_episode_steps": 0}, {}):
        duo = check(n, 16, kw, prep)
        assert np.isnan(duo["outs"][0]["obs"][0]).any()


def test_every_lane_pending_at_launch_start():
    n = 257

    def prep(env, step):
        state, elapsed, flags = env.get_state()
        env.set_state(state, (np.arange(n) % 7).astype(np.int32), np.ones(n, dtype=np.uint8))

    for kw in ({"max_episode_steps": 2}, {}):
        duo = check(n, 8, kw, prep)
        first = duo["outs"][0]
        assert not first["terminations"][0].any() and not first["truncations"][0].any() and (first["rewards"][0] == 0.0).all()
