"""Expected values and inputs of the masked / weighted action sampling tests (tests/test_masked_sampling.py, tests/test_gpu_masked_sampling.py).

The known answer is NumPy itself: the rows are walked in index order and every row calls ``Generator.choice`` on ONE ``Generator(PCG64)`` set to the
stream's state, which is what the reference's ``MultiDiscrete.sample(mask=...)`` / ``sample(probability=...)`` does for a batched Discrete space
(spaces/multi_discrete.py:180-249).  tests/golden/masked_sampling.npz, recorded from the reference's class, pins this restatement where the
reference is not installed (the GPU box).
"""
import functools

import numpy as np

IDS = {"CartPole-v1": 2, "MountainCar-v0": 3, "FrozenLake-v1": 4, "Taxi-v4": 6}
# np.random.PCG64(0)'s raw 64-bit output number REJECT_AT (0-based) has the low half 715 827 883 = (2^32 + 2) / 6: for k = 6 Lemire's leftover is
# 715827883 * 6 mod 2^32 = 2, below the threshold (2^32 - 6) mod 6 = 4, so the bounded draw is rejected and takes a second value
REJECT_AT, REJECT_LOW_HALF = 660016900, 715827883


# -- generators -------------------------------------------------------------------------------------------------------------------------------------
def generator(seed=None, state=None):
    """A ``Generator(PCG64)``; ``state``: (state, inc, has_uint32, uinteger) as ``state_of`` returns it."""
    gen = np.random.Generator(np.random.PCG64(seed))
    if state is not None:
        st = gen.bit_generator.state
        st["state"]["state"], st["state"]["inc"], st["has_uint32"], st["uinteger"] = (int(x) for x in state)
        gen.bit_generator.state = st
    return gen


def state_of(gen):
    st = gen.bit_generator.state
    return (int(st["state"]["state"]), int(st["state"]["inc"]), int(st["has_uint32"]), int(st["uinteger"]))


def state_words(state):
    """(state, inc, has_uint32, uinteger) as six uint64 (what fits an .npz)."""
    m = (1 << 64) - 1
    return np.array([state[0] >> 64, state[0] & m, state[1] >> 64, state[1] & m, state[2], state[3]], dtype=np.uint64)


def state_from_words(w):
    w = [int(x) for x in w]
    return ((w[0] << 64) | w[1], (w[2] << 64) | w[3], w[4], w[5])


def with_pending_half(gen):
    """Leave a 32-bit half pending: one bounded 32-bit draw, the way a masked row takes it."""
    gen.choice(np.arange(3))
    assert state_of(gen)[2] == 1
    return gen


# -- the restatement: NumPy walked row by row --------------------------------------------------------------------------------------------------------
def expected_masked(gen, masks):
    out = np.zeros(len(masks), dtype=np.int64)
    for i, row in enumerate(masks):
        valid = np.flatnonzero(row == 1)
        if len(valid):
            out[i] = gen.choice(valid)
    return out


def expected_weighted(gen, probs):
    out = np.zeros(len(probs), dtype=np.int64)
    for i, row in enumerate(probs):
        valid = (row > 0) & (row <= 1)
        out[i] = gen.choice(np.flatnonzero(valid), p=(row / np.sum(row))[valid])
    return out


def expected(gen, rows):
    return expected_weighted(gen, rows) if rows.dtype == np.float64 else expected_masked(gen, rows)


# -- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def make_masks(rng, n, a, density=0.6):
    """int8 (n, a): entries 1 with probability ``density``.  Every 16th row is all zeros and the row behind it holds a single one, so that each
    of the sampler's three cases -- k == 0, k == 1, k >= 2 valid actions -- has at least 5 % of the rows of any batch of 63 rows or more whatever
    ``a`` is (the density alone leaves 0.4 % of all-zero rows at a = 6); row 2 is all ones.  A batch of one or two rows starts with the all-one
    row: it draws."""
    m = (rng.random((n, a)) < density).astype(np.int8)
    if n < 3:
        m[0] = 1
        return m
    m[0::16] = 0
    ones = np.arange(1, n, 16)
    m[ones] = 0
    m[ones, rng.integers(0, a, len(ones))] = 1
    m[2] = 1
    return m


def make_probs(rng, n, a):
    """float64 (n, a), rows alternating between: random weights with ~30 % exact zeros, normalised in float64; a float32 softmax cast to
    float64 (its sum differs from 1 in the last bits of a float32, so the division by the sum matters); row 0: a single 1.0."""
    w = rng.random((n, a)) * (rng.random((n, a)) >= 0.3)
    w[np.arange(n), rng.integers(0, a, n)] += 0.05  # (never an all-zero row)
    p = w / w.sum(axis=1, keepdims=True)
    logits = rng.normal(size=(n, a)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    soft = (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float64)
    p[1::2] = soft[1::2]
    p[0] = np.eye(a)[a // 2]
    p = np.ascontiguousarray(np.clip(p, 0.0, 1.0))
    assert np.all(np.isclose(np.add.accumulate(p, axis=1)[:, -1], 1))
    return p


def mask_classes(masks):
    """Share of rows with k == 0, k == 1, k >= 2 valid actions."""
    k = (masks == 1).sum(axis=1)
    return np.array([(k == 0).mean(), (k == 1).mean(), (k >= 2).mean()])


@functools.lru_cache(maxsize=None)
def batches(a, n, count=20, seed=0):
    """``count`` consecutive batches for a space of ``n`` x Discrete(``a``): masks and probabilities alternating, masks first."""
    rng = np.random.default_rng([seed, a, n])
    out = []
    for b in range(count):
        rows = make_masks(rng, n, a) if b % 2 == 0 else make_probs(rng, n, a)
        rows.setflags(write=False)
        out.append(rows)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected_run(a, n, pending, count=20, seed=0, space_seed=4):
    """The expected actions and generator state after every batch of ``batches(a, n)`` from ``Generator(PCG64(space_seed))`` -- with ``pending``,
    after one 32-bit draw that leaves a half buffered.  Computed once per shape and shared."""
    gen = generator(space_seed)
    if pending:
        with_pending_half(gen)
    start = state_of(gen)
    acts, states = [], []
    for rows in batches(a, n, count, seed):
        acts.append(expected(gen, rows))
        states.append(state_of(gen))
    return start, tuple(acts), tuple(states)


def rejection_generator(back):
    """PCG64(0) placed ``back`` outputs before the one whose low half is rejected for k = 6."""
    gen = generator(0)
    gen.bit_generator.advance(REJECT_AT - back)
    return gen
