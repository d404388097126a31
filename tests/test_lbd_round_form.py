"""k_lbd_desc (csrc/lsd.hip) rounds a sample coordinate as (int)(x + copysign(0.49999997, x)) after a float clamp, where the reference writes
(short)round(x) and two compare/select clamps.  tools/microbench/lbd_round_check.c compares the two on the CPU for every float in
[-70000, 70000] (walked by bit pattern, +-0 and the denormals included) and at 0.5 - ulp, 0.5, 2^23 +- 1 and the other edges of the
form's range; its exit status is the number of mismatches."""
import os
import shutil
import subprocess

import pytest


def test_add_and_truncate_is_round_and_clamp(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "lbd_round_check")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-pthread", "-o", exe, os.path.join(root, "tools", "microbench", "lbd_round_check.c"), "-lm"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "mismatches 0" in p.stdout, p.stdout[-2000:]
    assert "floats 24" in p.stdout          # 2 x (bits(70000.0f) + 1) patterns and the edge cases: 2.4e9
