"""The kernels of csrc/line_triang.hip keep everything in registers: no scratch, no spills.  k_nl_triangulate holds two 4 x 4 double Jacobi
solves and three key-frame records per lane; its gates are evaluated without early exits so that no saved exec mask is spilled, and this
test is what notices if that changes.  The report is filtered by name.  The figures are the compiler's own remarks
(tools/kernel_resources.py); no assembly is inspected and no GPU is needed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")
KERNELS = ("k_nl_occupancy", "k_nl_triangulate", "k_nl_resolve", "k_nl_compact")


@pytest.fixture(scope="module")
def res():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not kr.hipcc():
        pytest.skip("hipcc not found")
    return {k: v for k, v in kr.resources(os.path.join(CSRC, "line_triang.hip")).items() if k.startswith("k_nl_")}


def test_every_kernel_is_reported(res):
    assert sorted(res) == sorted(KERNELS), sorted(res)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_and_no_spills(res, name):
    r = res[name]
    print("%-18s VGPRs %3d allocated %3d SGPRs %3d spills s/v %d/%d scratch %d LDS %d" % (
        name, r["vgprs"], r["alloc"], r["sgprs"], r["sgpr_spills"], r["vgpr_spills"], r["scratch"], r["lds"]))
    assert r["scratch"] == 0 and r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0, r
