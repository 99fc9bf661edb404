"""-m gpu: the DEVICE build of sincos_exact.h, pow_exact.h and the division helpers of envs_classic.h, member by member, bit for bit
(tests/hip/exact_math_check.hip, compiled here with the library's flags), and of log1p_exact.h (log1p on (-1, 0], the tail of the MuJoCo resets' normal
sampler: against the log1p calls recorded in tests/golden/normal_sampler.npz and against the running libm over every binade of u):

  * every member of mi::ExactMathT<true> and mi::ExactMathT<false> against the recorded vectors of tests/golden/exact_math_vectors.npz (the reference's
    libm, whatever this machine's is), SharedDivisor behind its call sites' range tests and div_unscaled against the host's IEEE division;
  * the same members against the RUNNING libm on the host side of the program: 10^8 sin / cos arguments sorted by branch range and shuffled, fmod with
    quotients up to 2^52, the arguments with pow(x, 2) != x * x, all 2^32 float32 patterns.  Where the machine's libm is not glibc's FMA build that
    leg cannot run: it is reported as SKIPPED, never as passed;
  * every kernel launched twice on the same inputs: identical outputs.

The program runs ONCE, in one process; the tests read its output.
"""
import os
import re
import subprocess

import pytest

from test_exact_math_check import HIPCC, compile_check, vectors_module, with_log1p

pytestmark = pytest.mark.gpu

# Safety cap for the one run.  Measured on an MI355X machine with 16 host threads: 13.4 s wall for a green run of the program (its own `elapsed` line,
# docs/results_log.md; the host side -- 2^32 powf calls, 2 x 10^8 sin / cos -- is most of it), so the cap is 45 times that: room for a slower or busier host.
RUN_SECONDS_MEASURED = 13.4
RUN_TIMEOUT = 600

TRIG = ["sin", "cos", "sincos.s", "sincos.c", "sincos_spread.s", "sincos_spread.c", "sin_bounded", "cos_bounded", "sincos_bounded.s", "sincos_bounded.c", "cos_bounded_literals",
        "sincos_main_unchecked.s", "sincos_main_unchecked.c"]
TRIG_KERNELS = ["sin", "cos", "sincos", "sincos_spread", "sin_bounded", "cos_bounded", "sincos_bounded", "cos_bounded_literals", "sincos_main_unchecked"]
POLICIES = ["kasm", "builtin"]  # ExactMathT<true> / ExactMathT<false>


def with_policy(member, policy):
    head, dot, sub = member.partition(".")
    return f"{head}.{policy}{dot}{sub}"


def expected_cases(trig_sets, other_set, sqf_set):
    names = []
    for p in POLICIES:
        for s in trig_sets:
            names += [f"{with_policy(m, p)}.{s}" for m in TRIG] + [f"relaunch.{k}.{p}.{s}" for k in TRIG_KERNELS]
        for m in ("fmod_2pi", "sq", "sq_is_plain", "sq2", "sq3"):
            names += [f"{m}.{p}.{other_set}", f"relaunch.{m}.{p}.{other_set}"]
        for m in ("sqf", "sqf_is_plain"):
            names += [f"{m}.{p}.{sqf_set}", f"relaunch.{m}.{p}.{sqf_set}"]
    return names


# log1p_exact.h's log1p_neg_unit (the tail of mjx::standard_normal) has one form: no policy in its case names
VECTOR_CASES = expected_cases(["vectors"], "vectors", "vectors") + ["log1p_neg_unit.vectors", "relaunch.log1p_neg_unit.vectors"]
DIVISION_CASES = ["shared_divisor.ieee", "relaunch.shared_divisor.ieee", "div_unscaled.ieee", "relaunch.div_unscaled.ieee"]
LIBM_CASES = expected_cases(["sorted", "shuffled"], "libm", "all") + ["log1p_neg_unit.libm", "relaunch.log1p_neg_unit.libm"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """compile, write the vectors out flat, run the program once; a fault or a timeout fails here with whatever the program printed"""
    d = tmp_path_factory.mktemp("exact_math")
    assert os.path.exists(HIPCC), "hipcc is needed to build the check"
    exe = compile_check(str(d / "exact_math_check"))
    mk = vectors_module()
    flat = str(d / "vectors.bin")
    mk.write_flat(with_log1p(mk.load()), flat)
    try:
        p = subprocess.run([exe, "--vectors", flat], capture_output=True, text=True, timeout=RUN_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(f"exact_math_check did not finish within {RUN_TIMEOUT} s:\n{out[-4000:]}")
    print(p.stdout[-20000:])
    cases = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^case (\S+) checked (\d+) mismatches (\d+)$", p.stdout, re.M)}
    return p, cases


def assert_clean(run, names, floor):
    p, cases = run
    tail = p.stdout[-6000:] + p.stderr[-2000:]
    assert p.returncode in (0, 1), f"exact_math_check ended with status {p.returncode}:\n{tail}"
    missing = [n for n in names if n not in cases]
    assert not missing, f"cases that did not run: {missing[:8]} ...\n{tail}"
    wrong = {n: cases[n] for n in names if cases[n][1] != 0}
    assert not wrong, f"(checked, mismatches) {wrong}\n" + "\n".join(ln for ln in p.stdout.splitlines() if ln.startswith("  mismatch"))[:6000]
    thin = {n: cases[n][0] for n in names if cases[n][0] < floor(n)}
    assert not thin, f"cases that compared fewer values than their inputs hold: {thin}"


def test_device_build_reproduces_the_recorded_vectors_and_the_ieee_division(run):
    def floor(name):
        if "shared_divisor" in name:
            return 2 ** 24
        if "div_unscaled" in name:
            return 2 ** 22
        if "sincos_main_unchecked" in name and not name.startswith("relaunch"):
            return 40_000  # the rows inside |x| < 0.855469
        if "is_plain" in name and not name.startswith("relaunch"):
            return 400      # the rows that pass the plain-product test (the recorded arguments are mostly the ones that do not)
        return 1500 if name.startswith("relaunch.sqf") else 3000

    assert_clean(run, VECTOR_CASES + DIVISION_CASES, floor)
    # nothing the program ran goes unjudged: its cases are exactly the expected ones (the libm leg's only where that leg ran; they are judged below)
    p, cases = run
    libm_ran = re.search(r"^libm: the expected glibc FMA build$", p.stdout, re.M) is not None
    expected = set(VECTOR_CASES + DIVISION_CASES) | (set(LIBM_CASES) if libm_ran else set())
    assert set(cases) == expected, (sorted(set(cases) - expected), sorted(expected - set(cases)))
    if not libm_ran:
        assert p.returncode == 0 and all(bad == 0 for _, bad in cases.values()), p.stdout[-4000:]


def test_device_build_equals_the_running_libm(run):
    p, cases = run
    skipped = re.search(r"^libm: NOT the expected.*$", p.stdout, re.M)
    if skipped:
        assert not any(n in cases for n in LIBM_CASES)
        pytest.skip(skipped.group(0))
    assert re.search(r"^libm: the expected glibc FMA build$", p.stdout, re.M), p.stdout[:2000]

    def floor(name):
        if name.startswith("relaunch.sqf") or name.startswith("relaunch.sqf_is_plain"):
            return 2 ** 31  # (pairs of 32-bit results)
        if name.startswith("sqf_is_plain"):
            return int(0.96 * 2 * 127 * 2 ** 22)  # 31 of 32 patterns with 2^-63 <= x^2 < 2^64 pass the test
        if name.startswith("sqf"):
            return 2 ** 32
        if "sorted" in name or "shuffled" in name:
            return 20_000_000 if "sincos_main_unchecked" in name and not name.startswith("relaunch") else 90_000_000
        if name.startswith("sq_is_plain"):
            return 9_000_000
        if "log1p_neg_unit" in name:
            return 53 * (2 * 2 ** 17 + 2 ** 15)  # per binade of u: the generator's grid, full significands, the binade's lower end
        return 2_000_000

    assert_clean(run, LIBM_CASES, floor)
    assert p.returncode == 0 and all(bad == 0 for _, bad in cases.values()), p.stdout[-4000:]
