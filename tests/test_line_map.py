"""The restatement of Tracking::SearchLocalLines + Manhattan::computeStructConstInMap (tests/line_map_ref.py) on hand-made cases with the expected
values written out, on exactly representable numbers: identity Rcw, zero translation, fx = fy = 512, cx = 320, cy = 240, bounds 640 x 480.
Then the declarations, the exports and the loud failure of the LineMap constructor without a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import line_map_ref as ref
from conftest import PKG_DIR, ROOT

F32 = np.float32
CAM = (512.0, 512.0, 320.0, 240.0, 0.0)
B4 = (0.0, 640.0, 0.0, 480.0)
T_ID = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
LOG_SF = float(F32(np.log(F32(1.2))))
NEW = ["hvo_line_map_create", "hvo_line_map_destroy", "hvo_line_map_set", "hvo_line_map_set_many", "hvo_line_map_set_bad", "hvo_line_map_set_observed",
       "hvo_line_map_counts", "hvo_line_map_slot", "hvo_line_map_last_error", "hvo_search_local_lines", "hvo_stream_search_local_lines",
       "hvo_batch_search_local_lines"]


def frustum(sp=(-0.5, 0, 2), ep=(0.5, 0, 2), normal=(0, 0, 1), mx=4.0, mn=1.0, T=T_ID):
    R, t, Ow = ref.pose_parts(T)
    return ref.is_in_frustum(list(sp) + list(ep), normal, mx, mn, CAM, R, t, Ow, B4, LOG_SF)


def test_the_passing_path_known_answer():
    e, p, vc, lv = frustum()
    assert e == 0 and np.array_equal(p, np.array([192, 240, 448, 240], F32)) and vc == F32(1.0)
    assert lv == 4                                                        # ceil(log(4 / 2) / log(1.2)) = ceil(3.80)
    # a dyadic translation and an axis permutation: Xc = (Yw, Zw, Xw) + (0.25, 0, 0); mOw = -R^T t = (0, -0.25, 0)
    T = np.array([[0, 1, 0, 0.25], [0, 0, 1, 0], [1, 0, 0, 0]], np.float32)
    R, t, Ow = ref.pose_parts(T)
    assert np.array_equal(Ow, np.array([0, -0.25, 0], F32))
    e, p, vc, lv = frustum(sp=(2, -0.75, 0), ep=(2, 0.25, 0), normal=(1, 0, 0), T=T)      # camera points (-0.5, 0, 2) and (0.5, 0, 2)
    assert e == 0 and np.array_equal(p, np.array([192, 240, 448, 240], F32)) and vc == F32(1.0) and lv == 4


@pytest.mark.parametrize("exit_no,kw", [
    (1, dict(sp=(-0.5, 0, -1))), (2, dict(ep=(0.5, 0, -1))),
    (3, dict(sp=(-2, 0, 2))), (4, dict(sp=(2, 0, 2))), (5, dict(sp=(-0.5, -2, 2))), (6, dict(sp=(-0.5, 2, 2))),
    (7, dict(ep=(-2, 0, 2))), (8, dict(ep=(2, 0, 2))), (9, dict(ep=(0.5, -2, 2))), (10, dict(ep=(0.5, 2, 2))),
    (11, dict(mn=4.0)), (12, dict(mx=1.0)), (13, dict(normal=(0, 0, 0.25)))])
def test_each_of_the_13_exits(exit_no, kw):
    assert frustum(**kw)[0] == exit_no


def test_boundaries_taken_exactly():
    e, p, vc, lv = frustum(sp=(0, 0, 0), ep=(0, 0, 4))                   # z == 0 passes `< 0.0f` and divides: 0 * inf is NaN, which passes the bounds
    assert e == 0 and np.isnan(p[0]) and np.isnan(p[1]) and p[2] == 320 and p[3] == 240
    e, p, _, _ = frustum(sp=(-1.25, 0, 2), ep=(1.25, 0, 2))               # u1 == mnMinX, u2 == mnMaxX
    assert e == 0 and p[0] == 0 and p[2] == 640
    assert frustum(sp=(float(np.nextafter(F32(-1.25), F32(-2))), 0, 2), ep=(1.25, 0, 2))[0] == 3
    assert frustum(sp=(-1.25, 0, 2), ep=(float(F32(1.25) + F32(2.0 ** -22)), 0, 2))[0] == 8   # (one ulp of x is half an ulp of u at 640)
    assert frustum(mn=2.5)[0] == 0                                        # 0.8f * 2.5f rounds to 2.0f == dist
    assert frustum(mn=float(np.nextafter(F32(2.5), F32(3))))[0] == 11
    z = float(F32(1.2) * F32(2.0))                                        # dist == 1.2f * max: the mid-point at depth z has dist z exactly
    assert frustum(sp=(-0.5, 0, z), ep=(0.5, 0, z), mx=2.0, normal=(0, 0, 1))[0] == 0
    zz = float(np.nextafter(F32(z), F32(3)))
    assert frustum(sp=(-0.5, 0, zz), ep=(0.5, 0, zz), mx=2.0)[0] == 12
    assert frustum(normal=(0, 0, 0.5))[0] == 0                            # viewCos == 0.5 passes `< 0.5`
    assert frustum(normal=(0, 0, float(np.nextafter(F32(0.5), F32(0)))))[0] == 13


def test_k_inverse_and_cos_sita_known_answers():
    Ki = ref.k_inv(CAM)
    assert np.array_equal(Ki, np.array([[1 / 512, 0, -0.625], [0, 1 / 512, -0.46875], [0, 0, 1]], F32))
    kl = (320.0, 240.0, 832.0, 240.0)                                     # back-projected (0, 0, 1) and (1, 0, 1): normal (0, 1, 0)
    assert ref.cos_sita(Ki, np.eye(3, dtype=F32), kl, (1, 0.125, 0)) == 0.125
    assert ref.cos_sita(Ki, np.eye(3, dtype=F32), kl, (1, -0.0625, 3)) == 0.0625
    Rp = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], F32)                 # Rcw w = (w1, w2, w0)
    assert ref.cos_sita(Ki, Rp, kl, (7, 1, 0.25)) == 0.25


def _gate_scene():
    """slots: 0 and 1 in view; world vectors with |y| = 0.125 (gated) / 0.0625 (kept); two frame lines with the same key line"""
    n = 3
    M = dict(pos=np.tile(np.array([-0.5, 0, 2, 0.5, 0, 2.0]), (n, 1)), normal=np.tile(np.array([0, 0, 1.0]), (n, 1)), max_dist=np.full(n, 4, F32),
             min_dist=np.full(n, 1, F32), desc=np.zeros((n, 32), np.uint8), bad=np.zeros(n, np.uint8), observed=np.ones(n, np.uint8),
             wvec=np.array([[1, 0.0625, 0], [1, 0.125, 0], [1, 0.125, 0]]))
    kl = np.zeros(3, dtype=[("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"), ("octave", "<i4")])
    kl["sx"], kl["sy"], kl["ex"], kl["ey"] = 320, 240, 832, 240
    l3d = np.zeros(3, dtype=[("A", "<f8", 3), ("B", "<f8", 3), ("line_eq", "<f4", 3)])
    return M, kl, l3d


def _call(M, kl, l3d, held, search, seen_extra=()):
    return ref.search_local_lines(M, CAM, T_ID, B4, LOG_SF, 1.0, 0.95, kl, None, l3d, None, None, None, held, seen_extra, search=search)


def test_post_gate():
    M, kl, l3d = _gate_scene()
    # line 0 gets slot 0 (kept: 0.0625), line 1 gets slot 1 (removed: 0.125), line 2 held slot 2 before the call (removed too)
    canned = lambda *a: (2, np.array([0, 1], np.int32), np.array([10, 10], np.int32))
    r = _call(M, kl, l3d, [-1, -1, 2], canned)
    assert list(r["in_view_slot"]) == [0, 1] and r["n_slots_tested"] == 2 and r["n_matches"] == 2
    assert list(r["held"]) == [0, -1, -1] and r["n_gated"] == 2
    # no match: nothing is removed, the line held before included
    none = lambda *a: (0, np.array([-1, -1], np.int32), np.array([256, 256], np.int32))
    r = _call(M, kl, l3d, [-1, -1, 2], none)
    assert list(r["held"]) == [-1, -1, 2] and r["n_gated"] == 0
    # query order: two map lines assigned to frame line 0, the later one stays; a held slot that is bad is cleared first and is not `seen`
    M["bad"][2] = 1
    both = lambda *a: (2, np.array([0, 0], np.int32), np.array([10, 10], np.int32))
    r = _call(M, kl, l3d, [-1, -1, 2], both)
    assert list(r["held"]) == [-1, -1, -1] and r["n_gated"] == 1 and r["n_slots_tested"] == 2      # slot 1 (0.125) won line 0 and was gated
    # seen_extra skips a slot
    r = _call(M, kl, l3d, [-1, -1, -1], none, seen_extra=[0])
    assert list(r["in_view_slot"]) == [1] and r["n_slots_tested"] == 1


def test_struct_constraints_thresholds_and_oddities():
    I = np.eye(3, dtype=F32)
    for th, below, above in ((0.062, 2, 0), (0.9985, 0, 1)):
        a = 2 * th; b = math.sqrt(4 - a * a)
        assert math.sqrt((a * a + b * b) + 0.0) == 2.0                    # |v| is exactly 2, so the cosine is a / 2 = th exactly
        at = ref.struct_rel(I, [[1, 0, 0]], [[a, b, 0]])[0, 0]
        lo = ref.struct_rel(I, [[1, 0, 0]], [[np.nextafter(a, 0), b, 0]])[0, 0]
        hi = ref.struct_rel(I, [[1, 0, 0]], [[np.nextafter(a, 4), b, 0]])[0, 0]
        assert at == 0 and lo == below and hi == above, (th, at, lo, hi)   # both tests are strict
    assert ref.struct_rel(I, [[1, 0, 0]], [[0, 1, 0]])[0, 0] == 2          # perpendicular is tested first
    assert ref.struct_rel(I, [[-1, -1, -1]], [[1, 1, 1]])[0, 0] == 1       # a (-1,-1,-1) frame line is not skipped
    assert ref.struct_rel(I, [[1, 0, 0]], [[0, 0, 0]])[0, 0] == 0          # zero world vector: NaN compares false both ways
    assert ref.struct_rel(I, [[0, 0, 0]], [[1, 0, 0]])[0, 0] == 0
    Rp = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], F32)                 # rotCW multiplies by Rcw: (1, 0, 0) -> (0, 0, 1)
    assert ref.struct_rel(Rp, [[1, 0, 0]], [[0, 0, 5]])[0, 0] == 1 and ref.struct_rel(Rp, [[1, 0, 0]], [[5, 0, 0]])[0, 0] == 2


def test_generated_scenes_keep_their_pattern_and_the_level_cap():
    T = ref.scene_pose()
    total = rej = 0
    for n, pat in ((63, "all"), (65, "alt"), (1000, "wave"), (1000, "all"), (65, "last"), (64, "none")):
        M, r = ref.make_map(n, pat, T, seed=n)
        fp = ref.frustum_pass(M, ref.CAM, T, ref.BOUNDS, ref.LOG_SF, [])
        assert np.array_equal(fp["slots"], np.nonzero(ref.wanted_in_view(n, pat))[0])
        total += n; rej += r
    assert rej * 100 < total
    M, _ = ref.make_map(400, "none", T, seed=3)
    assert set(np.unique(ref.frustum_pass(M, ref.CAM, T, ref.BOUNDS, ref.LOG_SF, [])["exits"])) >= {1, 12, 13}


def test_new_symbols_declared_exported_and_loud_without_a_device(hvo):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvo.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in hvo.EXPORTS, n
    assert "HVO_LINE_MAP_MAX_SLOTS" in hdr
    assert ctypes.sizeof(hvo.LocalLinesResult) == 32 and ctypes.sizeof(hvo.LocalLinesParams) == 28
    lib.hvo_abi_version.restype = ctypes.c_int
    assert lib.hvo_abi_version() == 3
    with pytest.raises(hvo.HvoError, match="hvo_line_map_create"):
        hvo.LineMap(device=1023)
