"""GPU: ``action_space.sample(mask=...)`` / ``sample(probability=...)`` drawn by the engine (mi_action_sample_masked / mi_action_sample_weighted,
gymnasium_amd/csrc/action_mask.hip) against NumPy walked row by row (tests/masked_sampling_cases.py, pinned on the reference's MultiDiscrete by
tests/test_masked_sampling.py).  Everything is array_equal: actions, and the generator's state -- PCG64 words and the pending 32-bit half."""
import ctypes

import numpy as np
import pytest

import gymnasium_amd
import masked_sampling_cases as mc
import policy_suite as ps
from gymnasium_amd import _native

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097]
CHECKED = 10  # batches whose generator state is read back one by one; the batches behind them run back to back


def _kw(rows):
    return {"probability": rows} if str(rows.dtype).endswith("float64") else {"mask": rows}  # (an ndarray or a tensor)


def _run_matrix_case(env_id, n, pending):
    a = mc.IDS[env_id]
    start, acts, states = mc.expected_run(a, n, pending)
    env = gymnasium_amd.make_vec(env_id, num_envs=n, device=0)
    env.action_space.seed(4)
    if pending:
        mc.with_pending_half(env.action_space.np_random)
    assert mc.state_of(env.action_space.np_random) == start
    rows_of = mc.batches(a, n)
    if n >= 63:
        for rows in rows_of[0::2]:
            assert mc.mask_classes(rows).min() >= 0.05, "every case of the masked draw has its share of the rows"
    for b, rows in enumerate(rows_of):
        got = env.action_space.sample(**_kw(np.array(rows)))
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == (n,)
        assert np.array_equal(got, acts[b]), (env_id, n, pending, b, int(np.flatnonzero(got != acts[b])[0]))
        if b < CHECKED or b == len(rows_of) - 1:
            assert mc.state_of(env.action_space.np_random) == states[b], (env_id, n, pending, b)
    env.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("env_id", sorted(mc.IDS))
@pytest.mark.parametrize("pending", [False, True], ids=["fresh", "half-pending"])
def test_batches_equal_numpy_row_by_row(env_id, n, pending):
    _run_matrix_case(env_id, n, pending)


@pytest.mark.parametrize("n", [65, 257, 4097])
@pytest.mark.parametrize("env_id", sorted(mc.IDS))
@pytest.mark.parametrize("pending", [False, True], ids=["fresh", "half-pending"])
def test_every_batch_through_the_repair_stage(env_id, n, pending, monkeypatch):
    """MI355ENV_MASKED_FORCE_REPAIR=1, read when the env is made: the stage that otherwise only recomputes the rows behind a rejected draw redoes every
    batch from row 0.  Values and generator state are identical."""
    monkeypatch.setenv("MI355ENV_MASKED_FORCE_REPAIR", "1")
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    assert libc.getenv(b"MI355ENV_MASKED_FORCE_REPAIR") == b"1", "the engine reads the C environment"
    _run_matrix_case(env_id, n, pending)


@pytest.mark.parametrize("n,back", [(8, 3), (300, 130), (4097, 1000)])
@pytest.mark.parametrize("force", [False, True], ids=["flagged", "forced"])
def test_a_real_rejection_moves_every_later_row(n, back, force, monkeypatch):
    """PCG64(0)'s output 660 016 900 has the low half 715 827 883: for k = 6 Lemire's leftover is 2 < 4, so the row that meets it draws a second value
    and every row behind it moves by one -- in the first wavefront, in the second workgroup, mid-grid with many workgroups behind."""
    if force:
        monkeypatch.setenv("MI355ENV_MASKED_FORCE_REPAIR", "1")
    masks = np.ones((n, 6), dtype=np.int8)
    gen = mc.rejection_generator(back)
    want = mc.expected_masked(gen, masks)
    # from NumPy alone: the batch took n + 1 32-bit values, not n -- ceil((n + 1) / 2) outputs, and the half of an odd count stays pending
    raw = mc.rejection_generator(0).bit_generator.random_raw()
    assert raw & 0xFFFFFFFF == mc.REJECT_LOW_HALF and (mc.REJECT_LOW_HALF * 6) % 2**32 < (2**32 - 6) % 6
    moved = mc.rejection_generator(back)
    moved.bit_generator.advance((n + 2) // 2)
    assert mc.state_of(gen)[0] == mc.state_of(moved)[0] and mc.state_of(gen)[2] == (n + 1) % 2
    plain = mc.rejection_generator(back)  # ... where n values would have left ceil(n / 2) outputs and n % 2
    plain.bit_generator.advance((n + 1) // 2)
    assert (mc.state_of(gen)[0], mc.state_of(gen)[2]) != (mc.state_of(plain)[0], n % 2)
    env = gymnasium_amd.make_vec("Taxi-v4", num_envs=n, device=0)
    env.action_space.seed(0)
    env.action_space.np_random.bit_generator.advance(mc.REJECT_AT - back)
    got = env.action_space.sample(mask=masks)
    assert np.array_equal(got, want), int(np.flatnonzero(got != want)[0])
    assert mc.state_of(env.action_space.np_random) == mc.state_of(gen)
    env.close()


@pytest.mark.parametrize("env_id,n", [("CartPole-v1", 257), ("Taxi-v4", 4097)])
def test_device_tensors_in_and_out(env_id, n):
    """Tensors on the env's device in, an int64 tensor on it out, nothing but launches in between -- equal to a twin env fed the same rows from the host."""
    import torch

    a = mc.IDS[env_id]
    dev = gymnasium_amd.make_vec(env_id, num_envs=n, device=0, output="torch", sample_output="torch")
    host = gymnasium_amd.make_vec(env_id, num_envs=n, device=0)
    dev.action_space.seed(4), host.action_space.seed(4)
    outs = []
    for rows in mc.batches(a, n):  # back to back: the position, the half and the lane states stay on the device
        t = torch.from_numpy(np.array(rows)).to("cuda:0")
        got = dev.action_space.sample(**_kw(t))
        assert isinstance(got, torch.Tensor) and got.dtype == torch.int64 and got.device == t.device and tuple(got.shape) == (n,)
        outs.append(got)
    outs.append(dev.action_space.sample())
    for b, rows in enumerate(mc.batches(a, n)):
        assert np.array_equal(ps._np(outs[b]), host.action_space.sample(**_kw(np.array(rows)))), (env_id, b)
    assert np.array_equal(ps._np(outs[-1]), host.action_space.sample())
    assert mc.state_of(dev.action_space.np_random) == mc.state_of(host.action_space.np_random)
    dev.close(), host.close()


@pytest.mark.parametrize("env_id", ["CartPole-v1", "Taxi-v4"])
def test_one_stream_with_every_other_consumer(env_id, oracle_factory):
    """sample(), sample(mask), step(None), rollout(4), sample(probability), np_random.random(), sample(mask) on the GPU == the same calls on the
    oracle-backed twin (whose masked draws are NumPy's): actions, observations and the generator's final state."""
    n, a = 300, mc.IDS[env_id]
    kw = dict(num_envs=n, output="torch", sample_output="torch")
    gpu = gymnasium_amd.make_vec(env_id, device=0, **kw)
    cpu = gymnasium_amd.make_vec(env_id, _engine_factory=oracle_factory, **kw)
    masks, probs, masks2 = (np.array(mc.batches(a, n, 5)[b]) for b in (0, 1, 4))
    trace = {}
    for name, env in (("gpu", gpu), ("cpu", cpu)):
        out = [env.reset(seed=3)[0]]
        env.action_space.seed(4)
        out.append(env.action_space.sample())
        out.append(env.action_space.sample(mask=masks))
        out.append(env.step(None)[0]), out.append(env.last_sampled_actions.clone())
        roll = env.rollout(4)
        out += [roll["actions"], roll["obs"]]
        out.append(env.action_space.sample(probability=probs))
        out.append(np.array(env.action_space.np_random.random()))
        out.append(env.action_space.sample(mask=masks2))
        out.append(np.array(mc.state_of(env.action_space.np_random), dtype=object))
        trace[name] = out
    for k, (g, c) in enumerate(zip(trace["gpu"], trace["cpu"])):
        assert np.array_equal(ps._np(g), ps._np(c)), (env_id, k)
    gpu.close(), cpu.close()


def test_taxi_closed_loop_on_the_action_mask(oracle_factory):
    """The documented way to act in Taxi -- step(action_space.sample(info["action_mask"])) -- 30 steps of 512 sub-environments against the oracle-backed
    twin, bit for bit."""
    n = 512
    gpu = gymnasium_amd.make_vec("Taxi-v4", num_envs=n, device=0)
    cpu = gymnasium_amd.make_vec("Taxi-v4", num_envs=n, _engine_factory=oracle_factory)
    (og, ig), (oc, ic) = gpu.reset(seed=5), cpu.reset(seed=5)
    gpu.action_space.seed(6), cpu.action_space.seed(6)
    assert np.array_equal(og, oc) and np.array_equal(ig["action_mask"], ic["action_mask"])
    for t in range(30):
        ag, ac = gpu.action_space.sample(mask=ig["action_mask"]), cpu.action_space.sample(mask=ic["action_mask"])
        assert np.array_equal(ag, ac), t
        assert np.all(ig["action_mask"][np.arange(n), ag] == 1) or np.any(ig["action_mask"].sum(axis=1) == 0)
        (og, rg, teg, trg, ig), (oc, rc, tec, trc, ic) = gpu.step(ag), cpu.step(ac)
        assert np.array_equal(og, oc) and np.array_equal(rg, rc) and np.array_equal(teg, tec) and np.array_equal(trg, trc), t
        assert np.array_equal(ig["action_mask"], ic["action_mask"]), t
    assert mc.state_of(gpu.action_space.np_random) == mc.state_of(cpu.action_space.np_random)
    gpu.close(), cpu.close()


@pytest.mark.parametrize("kind", ["mask", "probability"])
def test_a_device_batch_with_an_invalid_row_is_refused_whole(kind):
    """A device mask holding a 2 / a device probability row summing to 0.5: synchronize() raises, the stream has not moved, and the next valid call
    returns what it would have returned without the refused one."""
    import torch

    n, a = 1000, 6
    env = gymnasium_amd.make_vec("Taxi-v4", num_envs=n, device=0, output="torch", sample_output="torch")
    env.action_space.seed(4)
    gen = mc.with_pending_half(mc.generator(4))
    mc.with_pending_half(env.action_space.np_random)
    masks, probs = (np.array(r) for r in mc.batches(a, n, 2))
    good = masks if kind == "mask" else probs
    bad = good.copy()
    if kind == "mask":
        bad[n - 3, 1] = 2
    else:
        bad[n - 3] *= 0.5
    first = env.action_space.sample(**{kind: torch.from_numpy(good).cuda()})
    assert np.array_equal(ps._np(first), mc.expected(gen, good))
    env.action_space.sample(**{kind: torch.from_numpy(bad).cuda()})
    with pytest.raises(_native.NativeError, match="refused"):
        env.synchronize()
    assert mc.state_of(env.action_space.np_random) == mc.state_of(gen), "position and pending half are where they were"
    again = env.action_space.sample(**{kind: torch.from_numpy(good).cuda()})
    assert np.array_equal(ps._np(again), mc.expected(gen, good))
    env.synchronize()
    assert mc.state_of(env.action_space.np_random) == mc.state_of(gen)
    env.close()


def test_a_refused_batch_writes_nothing():
    """The engine call itself: `out` keeps its contents when the batch is refused."""
    import torch

    n, a = 300, 6
    env = gymnasium_amd.make_vec("Taxi-v4", num_envs=n, device=0, output="torch", sample_output="torch")
    env.action_space.seed(4)
    eng = env.action_space.hip_use_stream()
    env._bind_stream()
    bad = np.array(mc.batches(a, n, 1)[0])
    bad[0, 0] = -1
    t, out = torch.from_numpy(bad).cuda(), torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    eng.action_sample_masked(t.data_ptr(), out.data_ptr(), _native.MI_DEVICE)
    with pytest.raises(_native.NativeError, match="refused"):
        env.synchronize()
    assert bool((out == -7).all())
    env.close()


@pytest.mark.parametrize("kind", ["mask", "probability"])
def test_full_size_batch(kind):
    n, a = 65536, 6
    rng = np.random.default_rng(11)
    rows = mc.make_masks(rng, n, a) if kind == "mask" else mc.make_probs(rng, n, a)
    env = gymnasium_amd.make_vec("Taxi-v4", num_envs=n, device=0)
    env.action_space.seed(8)
    gen = mc.generator(8)
    got = env.action_space.sample(**{kind: rows})
    assert np.array_equal(got, mc.expected(gen, rows))
    assert mc.state_of(env.action_space.np_random) == mc.state_of(gen)
    env.close()
