"""The oracle against the pieces of the REFERENCE that compile from their own files:

    include/peac/DisjointSet.hpp   union by size / Find / getSetSize            -> oracle/peac.c ds_union, ds_find
    include/peac/AHCParamSet.hpp   T_mse, T_ang, T_dz with the default ParamSet -> oracle/peac.c T_mse_*, T_ang_init, T_dz
    src/lineIterator.cpp           ORB_SLAM2::LineIterator                      -> oracle/frame.c line_cells

The reference's outputs on fixed inputs are committed in tests/golden/ref_pins_v1.npz (made by tests/golden/make_ref_pins.py
from oracle/_ref/libhvoref.so, `make -C oracle ref`), so the oracle is checked against them on any checkout.  Where that
library is built, the same inputs also go through it and must still give the committed vectors.

These are the only parts of the hot path that the reference itself can vouch for here (everything else needs
OpenCV 3.2 / Eigen / PCL); they shrink what is ASSUMED, they do not turn "parity unpinned" green."""
import ctypes as C
import importlib.util
import os
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libhvoref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_pins_v1.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.fixture(scope="module")
def live():
    """the generator's own calls into oracle/_ref/libhvoref.so where it is built, else None"""
    if not os.path.exists(REF):
        return None
    spec = importlib.util.spec_from_file_location("make_ref_pins", os.path.join(ROOT, "tests", "golden", "make_ref_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load_ref(REF)


@pytest.fixture(scope="module")
def ol(orc):
    L = orc.lib()
    L.orc_ds_create.restype = C.c_void_p; L.orc_ds_create.argtypes = [C.c_int]
    L.orc_ds_union.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.orc_ds_find.argtypes = [C.c_void_p, C.c_int]; L.orc_ds_set_size.argtypes = [C.c_void_p, C.c_int]
    L.orc_ds_free.argtypes = [C.c_void_p]; L.orc_ds_free.restype = None
    for f in ("orc_peac_T_mse_init", "orc_peac_T_mse_merge", "orc_peac_T_ang_init", "orc_peac_T_dz"):
        getattr(L, f).restype = C.c_double; getattr(L, f).argtypes = [C.c_double]
    L.orc_grid_line_cells.argtypes = [C.c_double] * 4 + [C.c_void_p, C.c_void_p, C.c_int]
    return L


def test_disjoint_set_matches_reference(gold, live, ol):
    """random union sequences: the returned root of every Union, every Find and every set size agree (union by
    size with the reference's tie rule: equal sizes -> x's root survives, DisjointSet.hpp:73-82)"""
    for n in (1, 2, 17, 3072):
        ops, want, final = gold["ds%d_ops" % n], gold["ds%d_out" % n], gold["ds%d_final" % n]
        assert len(ops) == 4 * n
        if live is not None:
            got_ref, final_ref = live[0].ds_outputs(live[1], n, ops)
            assert np.array_equal(got_ref, want) and np.array_equal(final_ref, final)
        b = ol.orc_ds_create(n)
        try:
            for (x, y, q), (u, f, sz) in zip(ops.tolist(), want.tolist()):
                assert ol.orc_ds_union(b, x, y) == u
                assert ol.orc_ds_find(b, q) == f
                assert ol.orc_ds_set_size(b, q) == sz
            for q in range(n):
                assert ol.orc_ds_find(b, q) == final[q]
        finally:
            ol.orc_ds_free(b)


def test_paramset_thresholds_match_reference(gold, live, ol):
    """T_mse (P_INIT / P_MERGING), T_ang(P_INIT) and T_dz over metre-scale and millimetre-scale depths, bit for bit"""
    zs, want = gold["t_z"], gold["t_out"]
    assert len(zs) == 331 + 701 + 6
    if live is not None:
        assert np.array_equal(live[0].threshold_outputs(live[1], zs), want)
        assert live[1].ref_T_ang(1, 1.0) == gold["t_ang_merging_refine"][0] and live[1].ref_T_ang(2, 1.0) == gold["t_ang_merging_refine"][1]
    for z, (mse0, mse1, mse2, ang0, dz, dzn) in zip(zs.tolist(), want.tolist()):
        assert mse0 == ol.orc_peac_T_mse_init(z)
        assert mse1 == ol.orc_peac_T_mse_merge(z)
        assert mse2 == ol.orc_peac_T_mse_merge(z)
        assert ang0 == ol.orc_peac_T_ang_init(z)
        assert dz == ol.orc_peac_T_dz(z)
        assert dzn == ol.orc_peac_T_dz(-z)
    assert gold["t_ang_merging_refine"][0] == np.cos(np.deg2rad(60.0)) and gold["t_ang_merging_refine"][1] == np.cos(np.deg2rad(30.0))


def test_grid_line_iterator_matches_reference(gold, live, ol):
    """ORB_SLAM2::LineIterator: same cells in the same order, for random segments in grid coordinates (64 x 48),
    including steep / reversed / degenerate ones and end points outside the grid"""
    segs, counts, cells = gold["line_segs"], gold["line_counts"], gold["line_cells"]
    assert len(segs) == 2006 and counts.sum() == len(cells)
    if live is not None:
        c2, cells2 = live[0].line_outputs(live[1], segs)
        assert np.array_equal(c2, counts) and np.array_equal(cells2, cells)
    cap = 512
    bx, by = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    off = 0
    for s, n1 in zip(segs.tolist(), counts.tolist()):
        n2 = ol.orc_grid_line_cells(*s, bx.ctypes.data, by.ctypes.data, cap)
        assert n1 == n2 and n1 <= cap
        assert np.array_equal(cells[off:off + n1, 0], bx[:n1]) and np.array_equal(cells[off:off + n1, 1], by[:n1])
        off += n1
