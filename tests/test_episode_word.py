"""gymnasium_amd/csrc/episode_word.h keeps the env role's pending-autoreset flag, TimeLimit counter and reset-queue flag of the two-role rollout in one
32-bit word (classic_kernels.h duo_env_step_word).  Here the header is compiled for the host and checked, exhaustively over the small cases, against
the three-register logic of duo_env_step written out below: elapsed 0 .. max_steps + 1 for max_steps in {0, 1, 2, 3, 500} x pending x have x
terminated, with and without the flag word's other bit.  `truncated` and `resetting` are functions of those (elapsed + 1 >= max_steps; pending): the
test asserts that both values of each occur for every TimeLimit that is on."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FLAG_SHIFT, ELAPSED_MASK, NEEDS_RESET, STATE_F32 = 30, (1 << 30) - 1, 1, 2
MAX_STEPS = (0, 1, 2, 3, 500)
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        d = os.path.join(HERE, "episode_word_host")
        so, src = os.path.join(d, "libepisode_word_host.so"), os.path.join(d, "harness.cpp")
        hdr = os.path.join(HERE, "..", "gymnasium_amd", "csrc", "episode_word.h")
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in (src, hdr)):
            subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so, src], check=True, cwd=d)
        _LIB = C.CDLL(so)
        for name in ("ew_encode", "ew_decode_meta", "ew_effective_flags"):
            getattr(_LIB, name).argtypes, getattr(_LIB, name).restype = [C.c_uint32, C.c_uint32], C.c_uint32
        for name in ("ew_have", "ew_with_have"):
            getattr(_LIB, name).argtypes, getattr(_LIB, name).restype = [C.c_uint32], C.c_uint32
        _LIB.ew_threshold.argtypes, _LIB.ew_threshold.restype = [C.c_int], C.c_int32
        _LIB.ew_raw_flags.argtypes, _LIB.ew_raw_flags.restype = [C.c_uint32, C.c_int, C.c_int], C.c_uint32
        _LIB.ew_step_batch.argtypes, _LIB.ew_step_batch.restype = [C.c_void_p] * 5 + [C.c_long], None
    return _LIB


def three_registers(elapsed, flags, have, te, max_steps):
    """duo_env_step's bookkeeping (classic_kernels.h) on L.elapsed, L.flags and q.have: the state after the step, the predicates and the flag word it
    hands the aux role (1 terminated, 2 truncated, 4 this was the autoreset step).  reset_flags leaves CartPole's flag word as it is."""
    resetting = (flags & NEEDS_RESET) != 0
    refill = resetting and not have
    if refill:
        have = 1  # ResetQueue::refill
    el = elapsed + 1
    tr = max_steps > 0 and el >= max_steps
    done = (not resetting) and (te or tr)
    new_flags = (flags & ~NEEDS_RESET) if resetting else ((flags | NEEDS_RESET) if done else flags)
    new_elapsed = 0 if resetting else el
    new_have = 0 if resetting else have
    bits = (4 if resetting else 0) | (1 if (not resetting and te) else 0) | (2 if (not resetting and tr) else 0)
    return dict(elapsed=new_elapsed, flags=new_flags, have=new_have, resetting=resetting, refill=refill, truncated=(not resetting) and tr, done=done, bits=bits)


def meta_of(elapsed, flags):
    return (elapsed & ELAPSED_MASK) | (flags << FLAG_SHIFT)


def cases():
    for max_steps in MAX_STEPS:
        for elapsed, pending, have, te, other in itertools.product(range(max_steps + 2), (0, 1), (0, 1), (0, 1), (0, STATE_F32)):
            yield max_steps, elapsed, pending | other, have, te


def test_word_round_trips_meta_and_have():
    L = lib()
    for max_steps, elapsed, flags, have, _ in cases():
        w = L.ew_encode(meta_of(elapsed, flags), have)
        assert L.ew_decode_meta(w, flags) == meta_of(elapsed, flags)
        assert L.ew_decode_meta(w, flags & ~NEEDS_RESET) == meta_of(elapsed, flags)  # (the kernel strips the pending bit from the flag word it keeps)
        assert L.ew_have(w) == have and L.ew_have(L.ew_with_have(w)) == 1
        assert L.ew_decode_meta(L.ew_with_have(w), flags) == meta_of(elapsed, flags)
    top = meta_of(ELAPSED_MASK, NEEDS_RESET | STATE_F32)  # every bit of `meta` set
    assert L.ew_decode_meta(L.ew_encode(top, 1), STATE_F32) == top


def test_one_step_equals_the_three_register_logic_exhaustively():
    L = lib()
    rows = list(cases())
    w = np.array([L.ew_encode(meta_of(e, f), h) for _, e, f, h, _ in rows], dtype=np.uint32)
    te = np.array([r[4] for r in rows], dtype=np.uint8)
    ms = np.array([r[0] for r in rows], dtype=np.int32)
    pred, nxt = np.empty(len(rows), np.uint32), np.empty(len(rows), np.uint32)
    L.ew_step_batch(w.ctypes.data, te.ctypes.data, ms.ctypes.data, pred.ctypes.data, nxt.ctypes.data, len(rows))
    seen = {}
    for (max_steps, elapsed, flags, have, t), p, n, w0 in zip(rows, pred, nxt, w):
        ref = three_registers(elapsed, flags, have, bool(t), max_steps)
        ctx = (max_steps, elapsed, flags, have, t)
        assert bool(p & 1) == ref["resetting"], ctx
        assert bool(p & 2) == ref["refill"], ctx
        assert bool(p & 4) == ref["truncated"], ctx
        assert bool(p & 8) == ref["done"], ctx
        assert int(n) == L.ew_encode(meta_of(ref["elapsed"], ref["flags"]), ref["have"]), ctx
        assert L.ew_decode_meta(int(n), flags) == meta_of(ref["elapsed"], ref["flags"]), ctx
        # the flag word of the aux role: masked by the env role (word alone), or raw and masked by the aux role's own pending bit
        raw = L.ew_raw_flags(int(w0), t, max_steps)
        eff = L.ew_effective_flags(flags & NEEDS_RESET, raw)
        assert eff == (ref["bits"] & 3) and bool(flags & NEEDS_RESET) == bool(ref["bits"] & 4), ctx
        assert bool(eff) == bool(ref["flags"] & NEEDS_RESET), ctx  # ... and what is left is the next step's pending bit
        seen.setdefault(max_steps, set()).add((ref["resetting"], ref["truncated"]))
    for max_steps in MAX_STEPS:
        # (max_steps = 1: every step that is no autoreset step truncates)
        want = {(True, False)} | ({(False, True)} if max_steps > 0 else set()) | ({(False, False)} if max_steps != 1 else set())
        assert seen[max_steps] == want, (max_steps, seen[max_steps])  # truncated is never raised in an autoreset step, and never with the TimeLimit off


@pytest.mark.parametrize("max_steps", MAX_STEPS)
def test_a_lane_followed_over_many_steps(max_steps):
    """The word carried from step to step (refills at every 8th step as in the kernel) against the three registers carried likewise, the aux role's
    pending bit carried from the raw flags: same flags, same `meta`, same `have` at every step, from every start."""
    L = lib()
    rng = np.random.default_rng(max_steps)
    for start_elapsed, start_flags in itertools.product((0, 1, max(max_steps - 1, 0), max_steps + 1), (0, NEEDS_RESET, STATE_F32, NEEDS_RESET | STATE_F32)):
        elapsed, flags, have = start_elapsed, start_flags, 0
        w = L.ew_encode(meta_of(elapsed, flags), 0)
        aux_pending = flags & NEEDS_RESET
        te_seq = rng.random(96) < 0.3
        for t, te in enumerate(te_seq):
            if t % 8 == 0:  # the chunk's refill of every empty queue
                have, w = 1, L.ew_with_have(w)
            ref = three_registers(elapsed, flags, have, bool(te), max_steps)
            raw = L.ew_raw_flags(w, int(te), max_steps)
            eff = L.ew_effective_flags(aux_pending, raw)
            assert (eff | (4 if aux_pending else 0)) == ref["bits"], (t, start_elapsed, start_flags)
            aux_pending = eff
            w_in, te_in, ms_in = np.array([w], np.uint32), np.array([te], np.uint8), np.array([max_steps], np.int32)
            pred, nxt = np.empty(1, np.uint32), np.empty(1, np.uint32)
            L.ew_step_batch(w_in.ctypes.data, te_in.ctypes.data, ms_in.ctypes.data, pred.ctypes.data, nxt.ctypes.data, 1)
            w = int(nxt[0])
            elapsed, flags, have = ref["elapsed"], ref["flags"], ref["have"]
            assert L.ew_decode_meta(w, start_flags & ~NEEDS_RESET) == meta_of(elapsed, flags) and L.ew_have(w) == have, (t, start_elapsed, start_flags)


def test_threshold_of_a_time_limit_that_is_off_is_never_reached():
    L = lib()
    assert L.ew_threshold(0) == L.ew_threshold(-5) == 2 ** 31 - 1
    assert L.ew_threshold(1) == 2 and L.ew_threshold(500) == 1000
