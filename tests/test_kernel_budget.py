"""The register file as a budget ("The register file as a budget").

Under the default overlap policy the first part of a batch step holds two waves of k_peac_cluster_slots on every SIMD; what runs
beside them -- a k_orb_level wave and a k_lsd_pre wave -- lives on the registers they leave: 512 - 2 x 168 = 176 = 96 + 80.  A kernel
that grows past its band does not fail any result, it just silently loses its neighbour; this test is what notices.  The figures are
the compiler's own remarks (tools/kernel_resources.py); no assembly is inspected and no GPU is needed."""
import concurrent.futures
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def res():
    kr = _tool()
    if not kr.hipcc():
        pytest.skip("hipcc not found")
    files = ["orb_level.hip", "peac.hip", "lsd.hip"]
    with concurrent.futures.ThreadPoolExecutor(len(files)) as ex:
        per_file = list(ex.map(lambda f: kr.resources(os.path.join(CSRC, f)), files))
    out = {}
    for r in per_file:
        out.update(r)
    return out


def _one(res, name):
    assert name in res, (name, sorted(res))
    r = res[name]
    print("%-28s VGPRs %3d allocated %3d SGPRs %3d spills s/v %d/%d scratch %d LDS %d" % (
        name, r["vgprs"], r["alloc"], r["sgprs"], r["sgpr_spills"], r["vgpr_spills"], r["scratch"], r["lds"]))
    return r


def test_tool_reports_every_field(res):
    r = _one(res, "k_peac_cluster_slots")
    for f in ("vgprs", "alloc", "sgprs", "sgpr_spills", "vgpr_spills", "scratch", "lds"):
        assert f in r
    assert r["alloc"] % 8 == 0 and 0 <= r["alloc"] - r["vgprs"] < 8


def test_slot_ahc_band(res):
    r = _one(res, "k_peac_cluster_slots")
    assert r["alloc"] <= 168 and r["scratch"] == 0, r


def test_orb_level_band(res):
    names = [k for k in res if k.startswith("k_orb_level<")]
    assert sorted(names) == ["k_orb_level<1>", "k_orb_level<2>", "k_orb_level<4>"], names
    for k in names:
        r = _one(res, k)
        assert r["alloc"] <= 80 and r["scratch"] == 0, (k, r)


def test_lsd_preamble_band(res):
    r = _one(res, "k_lsd_pre")
    assert r["alloc"] <= 96 and r["scratch"] == 0, r


def test_slim_flood_band(res):
    r = _one(res, "k_peac_flood<64, 1, 16>")
    assert r["alloc"] <= 80 and r["scratch"] == 0, r


def test_dense_growing_band(res):
    r = _one(res, "k_lsd_grow_dense")
    assert r["alloc"] <= 72, r


def test_first_window_fills_the_file(res):
    """two AHC waves, an LSD-preamble wave and an ORB-level wave on one SIMD: 512 registers per lane"""
    orb = max(res[k]["alloc"] for k in res if k.startswith("k_orb_level<"))
    total = 2 * res["k_peac_cluster_slots"]["alloc"] + res["k_lsd_pre"]["alloc"] + orb
    print("2 x %d + %d + %d = %d" % (res["k_peac_cluster_slots"]["alloc"], res["k_lsd_pre"]["alloc"], orb, total))
    assert total <= 512, total
