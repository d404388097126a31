"""The four kernels of csrc/new_keyframe.hip keep everything in registers and LDS: no scratch, no spills.  The two selection kernels hold five
counters per lane across the tiles and pass one tile of keys and flags (256 x 5 bytes) through LDS; the line kernel holds its end points,
direction and normal in doubles beside them.  The figures are the compiler's own remarks (tools/kernel_resources.py); no assembly is
inspected and no GPU is needed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")
KERNELS = ("k_nkf_keys", "k_nkf_points", "k_nkf_lines", "k_nkf_struct")
LDS_CU = 160 * 1024                                             # a compute unit's LDS


@pytest.fixture(scope="module")
def res():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not kr.hipcc():
        pytest.skip("hipcc not found")
    return {k: v for k, v in kr.resources(os.path.join(CSRC, "new_keyframe.hip")).items() if k.startswith("k_nkf_")}


def test_every_kernel_is_reported(res):
    assert sorted(res) == sorted(KERNELS), sorted(res)


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_spills_and_lds_within_a_compute_unit(res, name):
    r = res[name]
    print("%-13s VGPRs %3d allocated %3d SGPRs %3d spills s/v %d/%d scratch %d LDS %d" % (
        name, r["vgprs"], r["alloc"], r["sgprs"], r["sgpr_spills"], r["vgpr_spills"], r["scratch"], r["lds"]))
    assert r["scratch"] == 0 and r["sgpr_spills"] == 0 and r["vgpr_spills"] == 0, r
    assert r["lds"] <= LDS_CU, r
    if name in ("k_nkf_points", "k_nkf_lines"): assert r["lds"] >= 256 * 5, r      # the tile of keys and flags is in LDS
