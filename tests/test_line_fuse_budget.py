"""The kernels of csrc/line_fuse.hip keep everything in registers: no scratch, no spills, and k_lf_search's chunk of records is a small part
of a compute unit's LDS, so the search's occupancy is not set by it.  The report is filtered by name.
The figures are the compiler's own remarks (tools/kernel_resources.py); no assembly is inspected and no GPU is needed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")
KERNELS = ("k_lf_lines", "k_lf_project", "k_lf_search", "k_lf_count", "k_lf_compact")
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def res():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not kr.hipcc():
        pytest.skip("hipcc not found")
    return {k: v for k, v in kr.resources(os.path.join(CSRC, "line_fuse.hip")).items() if k.startswith("k_lf_")}


def test_every_kernel_is_reported(res):
    assert sorted(res) == sorted(KERNELS), sorted(res)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_spills_and_a_quarter_of_the_lds(res, name):
    r = res[name]
    print("%-14s VGPRs %3d allocated %3d SGPRs %3d spills s/v %d/%d scratch %d LDS %d" % (
        name, r["vgprs"], r["alloc"], r["sgprs"], r["sgpr_spills"], r["vgpr_spills"], r["scratch"], r["lds"]))
    assert r["scratch"] == 0 and r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0, r
    assert r["lds"] * 4 <= CU_LDS, r
