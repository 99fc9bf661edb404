"""gymnasium_amd/csrc/log1p_exact.h restates glibc's log1p on (-1, 0] -- what NumPy's Generator.standard_normal calls in the ziggurat's tail, whose
value goes into the velocities of a HalfCheetah / Ant / InvertedDoublePendulum reset bit for bit (csrc/mjx_kernels.h standard_normal).  Here the
header is compiled for the host (plainly: no sanitizer, no FMA) and compared with the RUNNING libm on more than 10^8 arguments -u spread over every
binade of u, and with the calls recorded in tests/golden/normal_sampler.npz."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_normal_sampler import MK

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
PER_CASE = 640_000  # x 53 binades x 3 kinds of argument = 1.02e8


def lib():
    global _LIB
    if _LIB is None:
        d = os.path.join(HERE, "log1p_host")
        so, src = os.path.join(d, "liblog1p_host.so"), os.path.join(d, "harness.cpp")
        hdr = os.path.join(HERE, "..", "gymnasium_amd", "csrc", "log1p_exact.h")
        if not os.path.exists(so) or any(os.path.getmtime(p) > os.path.getmtime(so) for p in (src, hdr)):
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-fPIC", "-shared", "-fvisibility=hidden", "-o", so, src], check=True, cwd=d)
        _LIB = C.CDLL(so)
        _LIB.log1p_scan.argtypes, _LIB.log1p_scan.restype = [C.c_uint64, C.c_long, C.c_int, C.c_int, C.POINTER(C.c_uint64)], None
    return _LIB


pytestmark = pytest.mark.skipif(not MK.expected_libm(), reason="host libm is not glibc 2.35's log1p: nothing to compare against")


def batch(x, name="log1p_batch"):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    getattr(lib(), name)(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_long(x.size))
    return out


def test_equals_the_running_libm_over_every_binade_of_u():
    """Per binade [2^-(b+1), 2^-b) of u, b = 0 .. 52: u = m 2^-53 (the generator's grid), u with every significand bit random, and the 2^20 doubles above
    the binade's lower end (the routine's branch points sit there)."""
    fn = lib().log1p_scan

    def part(job):
        mode, b = job
        out = (C.c_uint64 * 3)()
        fn(1000 * mode + b, PER_CASE, b, mode, out)  # (ctypes releases the GIL: the parts run side by side)
        return mode, b, out[0], out[1], out[2]

    with ThreadPoolExecutor(min(16, os.cpu_count() or 4)) as ex:
        res = list(ex.map(part, [(mode, b) for mode in range(3) for b in range(53)]))
    examined = sum(r[2] for r in res)
    differ = [(mode, b, n, hex(first)) for mode, b, _, n, first in res if n]
    assert examined >= 10 ** 8
    assert not differ, f"(kind, binade, arguments that differ from libm, bits of the first): {differ[:10]}"
    print(f"log1p_neg_unit: {examined} arguments, 0 differ from the running libm")


def test_branch_points_and_ends():
    edges = [2.0 ** -29, 2.0 ** -54, 0.2928932188134524, 0.5, 0.75, 0.875, 1 - 2.0 ** -20, 1 - 2.0 ** -40]
    pts = [(np.arange(-3000, 3001, dtype=np.int64) + np.int64(np.float64(e).view(np.uint64))).astype(np.uint64).view(np.float64) for e in edges]
    pts.append((np.float64(1.0).view(np.uint64) - np.arange(1, 3001, dtype=np.uint64)).view(np.float64))  # the largest u: 1 - 2^-53 downwards
    pts.append(np.array([0.0, 2.0 ** -53, 2.0 ** -52, 3 * 2.0 ** -53]))
    x = -np.concatenate(pts)
    got, want = batch(x), batch(x, "libm_log1p_batch")
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.signbit(got[x == 0]).all()  # log1p(-0.0) = -0.0


def test_reproduces_the_recorded_calls_of_the_tail_lanes():
    rows = MK.load()
    x = rows["log1p_x"].view(np.float64)
    assert x.size >= 3000
    assert np.array_equal(batch(x).view(np.uint64), rows["log1p_r"])
    assert np.array_equal(batch(x, "libm_log1p_batch").view(np.uint64), rows["log1p_r"])
