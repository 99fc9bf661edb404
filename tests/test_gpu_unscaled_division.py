"""-m gpu: envs_classic.h div_unscaled -- CartPole's thetaacc quotient without v_div_scale / v_div_fmas / v_div_fixup -- against the compiler's
float64 division, bit for bit, over the range CartPole's test on t3 admits and its edges (tests/hip/div_unscaled_check.hip, compiled here with
the library's flags)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unscaled_quotient_equals_the_division(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "div_unscaled_check")
    src = os.path.join(ROOT, "tests", "hip", "div_unscaled_check.hip")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "gymnasium_amd", "csrc"), src, "-o", exe],
                   check=True, timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches 0" in p.stdout, p.stdout
