"""Record masked_sampling.npz FROM THE REFERENCE: ``MultiDiscrete([A] * N).sample(mask=...)`` / ``sample(probability=...)`` of the reference's own class
(gymnasium/spaces/multi_discrete.py:143-247), a few consecutive calls on one seeded space per action count, with the generator's state -- the PCG64
words, ``has_uint32`` and ``uinteger`` -- before the first and after every call.

    GYM_REFERENCE=/path/to/reference python tests/golden/make_golden_masked_sampling.py      # rewrites tests/golden/masked_sampling.npz

Per action count A in {2, 3, 4, 6}: ``A{A}_state`` uint64 [calls + 1, 6] (tests/masked_sampling_cases.py state_words), and per call c
``A{A}_rows{c}`` (int8 masks on even, float64 probabilities on odd calls) and ``A{A}_out{c}`` (the sampled actions).  The spaces of A = 3 and
A = 6 start with a 32-bit half pending.  The inputs come from tests/masked_sampling_cases.py, so the test needs nothing but this file and NumPy.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("GYM_REFERENCE", "/root/reference"))
sys.dont_write_bytecode = True

import masked_sampling_cases as mc  # noqa: E402

SHAPES = {2: 300, 3: 300, 4: 200, 6: 200}
CALLS = 4


def main():
    from gymnasium.spaces import MultiDiscrete

    out = {}
    for a, n in SHAPES.items():
        space = MultiDiscrete([a] * n, seed=7 + a)
        if a in (3, 6):
            mc.with_pending_half(space.np_random)
        states = [mc.state_words(mc.state_of(space.np_random))]
        for c, rows in enumerate(mc.batches(a, n, CALLS, seed=1)):
            as_tuple = tuple(np.array(r) for r in rows)
            got = space.sample(probability=as_tuple) if rows.dtype == np.float64 else space.sample(mask=as_tuple)
            out[f"A{a}_rows{c}"] = np.array(rows)
            out[f"A{a}_out{c}"] = got.astype(np.int8)
            states.append(mc.state_words(mc.state_of(space.np_random)))
        out[f"A{a}_state"] = np.stack(states)
    path = os.path.join(HERE, "masked_sampling.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
