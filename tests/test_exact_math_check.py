"""The CPU side of the device check of the exact-math routines (tests/hip/exact_math_check.hip, run on the GPU by tests/test_gpu_exact_math.py):

  * the program cross-compiles for gfx950 with the library's flags;
  * its --describe mode (no GPU, no HIP call) shows that the inputs contain what the check claims to cover: every branch range of s_sin.c in both the
    sorted and the shuffled sin / cos set, enough arguments with pow(x, 2) != x * x, all 2^32 float32 patterns, numerators on both sides of
    SharedDivisor::ordinary(), every binade of fmod's quotient up to 2^52, every binade of log1p's u = -x down to the generator's 2^-53;
  * the recorded vectors (tests/golden/exact_math_vectors.npz) are what tests/golden/make_exact_math_vectors.py writes, byte for byte, and the running
    libm and the host builds of the headers (tests/sincos_host, tests/pow_host) reproduce every row.
"""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hip", "exact_math_check.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def vectors_module():
    spec = importlib.util.spec_from_file_location("make_exact_math_vectors", os.path.join(HERE, "golden", "make_exact_math_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def with_log1p(vectors):
    """the recorded vectors plus the log1p calls of tests/golden/normal_sampler.npz's tail lanes (arguments -u, glibc's results), as write_flat takes them"""
    with np.load(os.path.join(HERE, "golden", "normal_sampler.npz"), allow_pickle=False) as z:
        return dict(vectors, log1p=(z["log1p_x"], z["log1p_r"]))


def compile_check(exe, contract="off"):
    """hipcc with gymnasium_amd/csrc/build.py's FLAGS (imported, so that the check is compiled like the library) for gfx950"""
    from gymnasium_amd.csrc import build

    flags = [f if not f.startswith("-ffp-contract=") else "-ffp-contract=" + contract for f in build.FLAGS]
    assert "-ffp-contract=" + contract in flags
    subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", *flags, "-I", os.path.join(ROOT, "gymnasium_amd", "csrc"), SRC, "-o", exe, "-ldl"], check=True, timeout=900)
    return exe


def parse_describe(text):
    out = {}
    for line in text.splitlines():
        if line.startswith("describe "):
            _, name, *pairs = line.split()
            out[name] = {k: int(v) for k, v in (p.split("=") for p in pairs)}
    return out


@pytest.fixture(scope="module")
def described(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    exe = compile_check(str(tmp_path_factory.mktemp("exact_math") / "exact_math_check"))
    p = subprocess.run([exe, "--describe"], capture_output=True, text=True, timeout=1800, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert p.returncode == 0, p.stdout + p.stderr
    assert not re.search(r"^case ", p.stdout, re.M), "--describe must not run any case"
    return parse_describe(p.stdout)


BRANCH_RANGES = ["below_2^-27", "below_2^-26", "taylor", "table", "quarter", "reduced", "beyond", "nonfinite"]


def test_sin_cos_inputs_populate_every_branch_range_sorted_and_shuffled(described):
    s, h = described["trig.sorted"], described["trig.shuffled"]
    assert s["arguments"] == h["arguments"] >= 6 * 2 ** 24 + 19 * 2 * 4001
    for r in BRANCH_RANGES:
        assert s[r] > 0 and h[r] == s[r], r
    for r in ("taylor", "table", "quarter", "reduced"):
        assert s[r] >= 2 ** 21, r
    waves = s["uniform_wavefronts"] + s["mixed_wavefronts"]
    # sorted: all but the wavefronts at a boundary between two ranges are uniform, and a quarter of them take sincos()'s MAIN_FIRST short cut as one
    assert s["mixed_wavefronts"] <= len(BRANCH_RANGES) and s["main_first_wavefronts"] >= waves // 5
    # shuffled: every wavefront diverges
    assert h["uniform_wavefronts"] == 0 and h["main_first_wavefronts"] == 0 and h["mixed_wavefronts"] == waves


def test_square_inputs_contain_the_arguments_only_the_table_routine_gets_right(described):
    assert described["sq"]["pow_ne_product"] >= 10_000
    assert described["sq"]["arguments"] >= 5 * 2 ** 21
    g = described["sq_groups"]
    assert g["all_hard_groups_sq2"] >= 300 and g["all_hard_groups_sq3"] >= 300
    assert g["arguments"] % 6 == 0
    f = described["sqf"]
    assert f["patterns"] >= 2 ** 32 - 1
    assert f["powf_ne_product"] > 1_000_000  # 0.07 % of the finite patterns


def test_division_inputs_cover_both_sides_of_ordinary(described):
    d = described["shared_divisor"]
    assert d["pairs"] >= 2 ** 24
    assert d["numerators_outside_ordinary"] >= d["pairs"] // 100
    assert d["numerators_ordinary"] == d["pairs"] - d["numerators_outside_ordinary"] and d["numerators_ordinary"] >= d["pairs"] * 9 // 10
    assert d["divisors_2.5_to_4.5"] >= 2 ** 20 and d["divisors_outside_range"] > 0
    assert described["div_unscaled"]["pairs"] >= 2 ** 22


def test_fmod_inputs_populate_every_quotient_binade_up_to_2_52(described):
    f = described["fmod_2pi"]
    for b in range(20, 52):  # the quotient in [2^b, 2^(b+1)): up to 2^52, the routine's advertised limit
        assert f[f"quotient_2^{b}"] >= 2 ** 16, b
    assert f["quotient_below_2^20"] >= 3_000_000


def test_log1p_inputs_cover_every_binade_of_u_and_every_branch(described):
    d = described["log1p_neg_unit"]
    for b in range(1, 54):  # u in [2^-b, 2^-(b-1)): the generator's u = m 2^-53 reaches down to 2^-53
        assert d[f"u_2^-{b}"] >= 2 * 2 ** 17 + 2 ** 15, b
    assert d["arguments"] >= 53 * (2 * 2 ** 17 + 2 ** 15) and d["zero"] >= 1
    assert d["generator_grid"] >= 53 * 2 ** 17
    # the routine's three forms: x - x^2 / 2 below 2^-29 (25 binades), f = x down to 1 - sqrt(2)/2, the reduction 1 + x = 2^k (1 + f) beyond
    assert d["below_2^-29"] >= 24 * 2 ** 18 and d["direct"] >= 27 * 2 ** 18 and d["reduced"] >= 2 ** 18


# ---- the recorded vectors ------------------------------------------------------------------------------------------------------------------

def same_bits(a, b, nan_mask):
    return bool(np.all((a == b) | nan_mask))


def test_recorded_vectors_regenerate_byte_for_byte():
    mk = vectors_module()
    if not mk.expected_libm():
        pytest.skip("host libm is not glibc's FMA build: the vectors cannot be regenerated here")
    with open(mk.PATH, "rb") as f:
        committed = f.read()
    fresh = mk.generate()
    with np.load(mk.PATH, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(fresh)
        for name in z.files:  # (said first, array by array: a difference here is one of content, below one of the container)
            assert z[name].dtype == fresh[name].dtype and np.array_equal(z[name], fresh[name]), name
    assert mk.npz_bytes(fresh) == committed
    largest_other = max(os.path.getsize(os.path.join(HERE, "golden", n)) for n in os.listdir(os.path.join(HERE, "golden")) if n != os.path.basename(mk.PATH))
    assert len(committed) <= largest_other


def test_recorded_vectors_are_what_libm_and_the_host_builds_compute():
    mk = vectors_module()
    if not mk.expected_libm():
        pytest.skip("host libm is not glibc's FMA build: nothing to compare the vectors with")
    import test_pow_exact as tp
    import test_sincos_exact as ts

    v = mk.load()
    x, sn, cs = (a.view(np.float64) for a in v["trig"])
    assert x.size > 140_000
    with np.errstate(invalid="ignore"):
        assert ts.same_bits(np.sin(x), sn) and ts.same_bits(np.cos(x), cs)
    ts.check_all_forms(x)  # the host builds of every form against np.sin / np.cos, hence against the rows
    inside = np.abs(x) < 105414336.0
    s, c = ts.run_sincos(x[inside], "sincos_pair_hot_batch")
    assert ts.same_bits(s, sn[inside]) and ts.same_bits(c, cs[inside])
    fx, fr = (a.view(np.float64) for a in v["fmod"])
    assert ts.same_bits(np.fmod(fx, mk.TWO_PI), fr) and ts.same_bits(ts.run("fmod_2pi_batch", fx), fr)
    quotient = np.floor(np.abs(fx) / mk.TWO_PI)
    assert set(range(20, 52)) <= set(np.frexp(quotient[quotient >= 1])[1] - 1)
    px, pr = (a.view(np.float64) for a in v["pow"])
    assert ts.same_bits(np.array([tp.libm.pow(t, 2.0) for t in px]), pr) and ts.same_bits(tp.square(px), pr)
    with np.errstate(over="ignore"):
        assert (pr != px * px).sum() >= 2000
    n6 = px.size // 6 * 6
    assert ts.same_bits(tp._grouped(px[:n6], 3), pr[:n6]) and ts.same_bits(tp._grouped(px[:n6], 2), pr[:n6])
    qx, qr = (a.view(np.float32) for a in v["powf"])
    got, want = tp.squaref(qx), np.array([tp.libm.powf(float(t), 2.0) for t in qx], dtype=np.float32)
    nan = np.isnan(qr)
    assert same_bits(want.view(np.uint32), qr.view(np.uint32), nan & np.isnan(want)) and same_bits(got.view(np.uint32), qr.view(np.uint32), nan & np.isnan(got))
    with np.errstate(over="ignore", under="ignore"):
        assert (qr != qx * qx).sum() >= 2000
    for pattern in mk.POWF_SUBNORMAL_TIES:  # subnormal squares on a rounding tie: powf is not the product there
        (row,) = np.flatnonzero(qx.view(np.uint32) == pattern)
        assert qr.view(np.uint32)[row] != (qx[row] * qx[row]).view(np.uint32), hex(pattern)


def test_flat_vector_file_round_trips(tmp_path):
    """the file tests/test_gpu_exact_math.py hands to the program: header, four sections, every word"""
    mk = vectors_module()
    v = mk.load()
    path = str(tmp_path / "vectors.bin")
    mk.write_flat(v, path)
    w = np.fromfile(path, dtype="<u8")
    assert w[0:1].tobytes() == b"EXMATHV1"
    at = 1
    for ident, key in ((1, "trig"), (2, "fmod"), (3, "pow"), (4, "powf")):
        assert w[at] == ident and w[at + 1] == v[key][0].size
        n = int(w[at + 1])
        for k, col in enumerate(v[key]):
            assert np.array_equal(w[at + 2 + k * n: at + 2 + (k + 1) * n], col.astype(np.uint64))
        at += 2 + len(v[key]) * n
    assert at == w.size
    # ... and with the fifth section, as tests/test_gpu_exact_math.py writes it: the four above unchanged, then the log1p rows
    v5 = with_log1p(v)
    mk.write_flat(v5, path)
    w5 = np.fromfile(path, dtype="<u8")
    n = v5["log1p"][0].size
    assert n >= 3000 and np.array_equal(w5[:at], w) and w5[at] == 5 and w5[at + 1] == n and w5.size == at + 2 + 2 * n
    assert np.array_equal(w5[at + 2: at + 2 + n], v5["log1p"][0]) and np.array_equal(w5[at + 2 + n:], v5["log1p"][1])
