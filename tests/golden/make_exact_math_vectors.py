"""Record exact_math_vectors.npz: arguments and expected results, as bit patterns, of the C-library functions that sincos_exact.h and pow_exact.h
restate -- sin, cos, fmod(x, 2 pi), pow(x, 2.0), powf(x, 2.0f) -- taken from NumPy and the libm of the machine the reference runs on (glibc 2.35,
the FMA build).  tests/test_gpu_exact_math.py hands them to tests/hip/exact_math_check.hip (--vectors), so the DEVICE build is pinned to the reference's
libm even where the GPU machine's differs; tests/test_exact_math_check.py checks that this script reproduces the file byte for byte and that the running
libm and the host builds of the headers reproduce every row.

    python tests/golden/make_exact_math_vectors.py          # rewrites tests/golden/exact_math_vectors.npz

Rows: the +-2000-ulp neighbourhood of every branch point of s_sin.c, the table's 1/256 ties, tiny / subnormal / special arguments; fmod arguments whose
quotient lies in each binade from 2^20 to 2^52 (random ones and the multiples of 2 pi with both neighbours); arguments with pow(x, 2) != x * x and
powf(x, 2) != x * x (found by scanning the libm) among random and special ones.  The sin / cos columns are stored as differences of consecutive bit
patterns (neighbouring arguments have neighbouring results, which compresses 20-fold); decode() undoes that.
"""
import ctypes as C
import io
import math
import os
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "exact_math_vectors.npz")
TWO_PI = 6.283185307179586
EDGES = [2.0 ** -27, 2.0 ** -26, 0.126, 0.855469, 0.8554688, 2.426265, 105414350.0, 105414336.0,  # (the hand-over to Payne-Hanek itself: high word 0x419921fb)
         math.pi / 4, math.pi / 2, math.pi, 3 * math.pi / 2, 2 * math.pi,
         1.0 / 128, 0.5 / 128, 109.5 / 128, 110.0 / 128, 1.5707963267948966 - 0.126, 1.5707963267948966 - 0.855469]


# float32 patterns whose square is subnormal and within rounding error of a tie: powf(x, 2) != x * x there
POWF_SUBNORMAL_TIES = [0x1AC00000, 0x1B200000, 0x1B600000, 0x1B900000, 0x1BB00000, 0x1BD00000, 0x1BF00000, 0x1C080000, 0x1C180000, 0x1C427BE3]


def expected_libm():
    return (math.sin(0.5).hex(), math.cos(0.5).hex(), math.pow(1.3, 2.0).hex()) == ("0x1.eaee8744b05f0p-2", "0x1.c1528065b7d50p-1", "0x1.b0a3d70a3d70bp+0")


def _libm():
    m = C.CDLL("libm.so.6")
    m.pow.restype, m.pow.argtypes = C.c_double, [C.c_double, C.c_double]
    m.powf.restype, m.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return m


def trig_arguments():
    pts = []
    for e in EDGES:
        nb = (np.arange(-2000, 2001, dtype=np.int64) + np.int64(np.float64(e).view(np.uint64))).astype(np.uint64).view(np.float64)
        pts += [nb, -nb]
    ties = np.arange(0, 221) / 256.0
    pts += [ties, np.nextafter(ties, 1), np.nextafter(ties, -1), -ties]
    pts.append(np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, 1e-30, np.inf, -np.inf, np.nan, 1e5, -1e5, 1e8, -1e8]))
    rng = np.random.default_rng(5)
    pts.append(rng.uniform(-1, 1, 2000) * 2.0 ** rng.integers(-1070, -20, 2000).astype(np.float64))
    return np.concatenate(pts)


def fmod_arguments():
    rng = np.random.default_rng(6)
    k = np.arange(-50, 51, dtype=np.float64) * TWO_PI
    pts = [rng.uniform(-50, 50, 300), rng.uniform(-1e8, 1e8, 300), k, np.nextafter(k, np.inf), np.nextafter(k, -np.inf), np.array([0.0, -0.0, TWO_PI, -TWO_PI, math.pi, 1e15])]
    for b in range(20, 52):  # the quotient in [2^b, 2^(b+1))
        sign = np.where(rng.integers(0, 2, 48) == 0, -1.0, 1.0)
        pts.append(sign * rng.uniform(1.0, 2.0, 48) * 2.0 ** b * TWO_PI)
        q = rng.integers(2 ** b, 2 ** (b + 1), 16).astype(np.float64) * TWO_PI * np.where(rng.integers(0, 2, 16) == 0, -1.0, 1.0)
        pts += [q, np.nextafter(q, np.inf), np.nextafter(q, -np.inf)]
    x = np.concatenate(pts)
    return x[np.abs(x) < 2.0 ** 52 * TWO_PI]


def pow_arguments(m):
    """2 000 arguments with pow(x, 2) != x * x (about one in 1 200), 1 000 random ones, the special values of tests/test_pow_exact.py"""
    rng = np.random.default_rng(7)
    hard = []
    while len(hard) < 2000:
        x = rng.uniform(-10, 10, 200_000)
        hard += [v for v in x.tolist() if m.pow(v, 2.0) != v * v]
    special = [0.0, -0.0, 1.0, -1.0, 2.0, 0.5, float(np.nextafter(1.0, 2)), float(np.nextafter(1.0, 0)), 1e-200, 1e200, 5e-324, np.inf, -np.inf, 1e-160, 1e154, 3.0, -8.0, np.nan,
               2.0 ** -95, 2.0 ** 95, 1.4142135623730951, float(np.nextafter(1.4142135623730951, 0)), 2.0 ** 0.5 * 2.0 ** 20]
    return np.concatenate([np.array(hard[:2000]), rng.uniform(-10, 10, 400), rng.uniform(-1, 1, 200), rng.uniform(0.99, 1.01, 200), rng.uniform(-1e5, 1e5, 200), np.array(special)])


def powf_arguments(m):
    """2 000 float32 arguments with powf(x, 2) != x * x (0.07 %), 1 000 random ones, special values"""
    rng = np.random.default_rng(8)
    hard = []
    while len(hard) < 2000:
        x = rng.uniform(-2, 2, 200_000).astype(np.float32)
        prod = (x * x).tolist()
        hard += [v for v, p in zip(x.tolist(), prod) if m.powf(v, 2.0) != p]
    special = np.array([0.0, -0.0, 1.0, -2.0, 1e-30, 1e30, 1e-45, 1e-38, np.inf, -np.inf, np.nan, 3e38, 1e-20, 1e19], dtype=np.float32)
    # squares outside the normal range: subnormal ones (powf rounds exp2's double once, which is not x * x on a tie: the first ten are such ties), the
    # underflow and overflow thresholds, the top two binades
    ties = np.array(POWF_SUBNORMAL_TIES, dtype=np.uint32).view(np.float32)
    edge = np.concatenate([ties, (2.0 ** rng.uniform(-76.0, -62.5, 300)).astype(np.float32), (-2.0 ** rng.uniform(62.5, 64.5, 200)).astype(np.float32)])
    return np.concatenate([np.array(hard[:2000], dtype=np.float32), rng.uniform(-2, 2, 600).astype(np.float32), rng.uniform(-100, 100, 400).astype(np.float32), special, edge])


def to_delta(bits):
    """uint64 patterns -> wrapped differences of consecutive ones"""
    return np.diff(bits, prepend=np.uint64(0))


def from_delta(delta):
    return np.cumsum(delta, dtype=np.uint64)


def generate():
    """name -> array, as stored"""
    m = _libm()
    tx, fx, px, qx = trig_arguments(), fmod_arguments(), pow_arguments(m), powf_arguments(m)
    with np.errstate(invalid="ignore"):
        ts, tc = np.sin(tx), np.cos(tx)
        fr = np.fmod(fx, TWO_PI)
    pr = np.array([m.pow(v, 2.0) for v in px.tolist()])
    qr = np.array([m.powf(v, 2.0) for v in qx.tolist()], dtype=np.float32)
    u = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return {"trig_x_delta": to_delta(u(tx)), "trig_sin_delta": to_delta(u(ts)), "trig_cos_delta": to_delta(u(tc)), "fmod_x": u(fx), "fmod_r": u(fr), "pow_x": u(px), "pow_r": u(pr),
            "powf_x": qx.view(np.uint32), "powf_r": qr.view(np.uint32)}


def decode(z):
    """the stored arrays -> bit patterns per function: {"trig": (x, sin, cos), "fmod": (x, r), "pow": (x, r), "powf": (x, r)}"""
    return {"trig": (from_delta(z["trig_x_delta"]), from_delta(z["trig_sin_delta"]), from_delta(z["trig_cos_delta"])), "fmod": (z["fmod_x"], z["fmod_r"]),
            "pow": (z["pow_x"], z["pow_r"]), "powf": (z["powf_x"], z["powf_r"])}


def load(path=PATH):
    with np.load(path, allow_pickle=False) as z:
        return decode({k: z[k] for k in z.files})


def npz_bytes(arrays):
    """an .npz with nothing of the day it was written in it: the same arrays give the same bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as zf:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            zf.writestr(info, b.getvalue(), compresslevel=9)
    return buf.getvalue()


def write_flat(vec, path):
    """what exact_math_check --vectors reads: 64-bit words; "EXMATHV1", then per function {id, n, n arguments, n results (sin, then cos)}.  `vec` may hold
    a fifth function, "log1p": the (arguments, results) columns of tests/golden/normal_sampler.npz, which the caller adds"""
    with open(path, "wb") as f:
        f.write(b"EXMATHV1")
        for ident, key in ((1, "trig"), (2, "fmod"), (3, "pow"), (4, "powf"), (5, "log1p")):
            if key not in vec:
                assert key == "log1p"
                continue
            cols = [np.ascontiguousarray(c).astype(np.uint64) for c in vec[key]]
            f.write(np.array([ident, cols[0].size], dtype="<u8").tobytes())
            for c in cols:
                f.write(c.astype("<u8").tobytes())


if __name__ == "__main__":
    if not expected_libm():
        raise SystemExit("this machine's libm is not the reference's (glibc FMA build): not recording")
    data = npz_bytes(generate())
    with open(PATH, "wb") as f:
        f.write(data)
    print(PATH, len(data), "bytes")
