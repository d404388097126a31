"""CPU checks of the restatement the GPU tests of the resident point map compare against (tests/point_map_ref.py): hand-computed known
answers of Frame::isInFrustum(MapPoint *) and MapPoint::PredictScale, the scene generator's level guard, that the committed synthetic scene
gives the search something to find and something to refuse, and agreement with the search model tests/test_guided_gpu.py uses."""
import math
import os
import re

import numpy as np

import guided_cases as gc
import point_map_ref as ref
from conftest import ROOT

F32 = np.float32
NEW = ["hvo_point_map_create", "hvo_point_map_destroy", "hvo_point_map_set", "hvo_point_map_set_many", "hvo_point_map_set_bad", "hvo_point_map_set_observed",
       "hvo_point_map_counts", "hvo_point_map_slot", "hvo_point_map_last_error", "hvo_search_local_points", "hvo_stream_search_local_points",
       "hvo_batch_search_local_points"]

# An axis permutation with a dyadic translation: Xc = (Yw + 0.5, Zw - 0.25, Xw + 2), mOw = (-2, -0.5, 0.25), every step exact.
T_PERM = ref.crafted_pose()
CAM2 = ref.CAM2                                   # (512, 512, 320, 240, 64): with z = 2, u = 256 x + 320, v = 256 y + 240, ur = u - 32
B4 = (0.0, 640.0, 0.0, 480.0)
world = ref.crafted_world                         # the world point whose camera coordinates under T_PERM are (xc, yc, zc), exactly


def frustum(P, normal=(1, 0, 0), mx=4.0, mn=1.0, log_sf=ref.LOG_SF, limit=0.5):
    R, t, Ow = ref.pose_parts(T_PERM)
    assert np.array_equal(Ow, np.array([-2, -0.5, 0.25], np.float32))
    return ref.is_in_frustum(P, np.asarray(normal, np.float32), F32(mx), F32(mn), CAM2, R, t, Ow, B4, log_sf, 8, F32(limit))


def test_the_header_and_the_binding_name_the_new_calls(hvo):
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in hvo.EXPORTS, n
    assert "#define HVO_POINT_MAP_MAX_SLOTS (1 << 20)" in hdr and "#define HVO_HELD_FOREIGN_OBSERVED (-2)" in hdr and "#define HVO_HELD_FOREIGN_UNOBSERVED (-3)" in hdr
    assert (hvo.HELD_FOREIGN_OBSERVED, hvo.HELD_FOREIGN_UNOBSERVED, hvo.POINT_MAP_MAX_SLOTS) == (ref.FOREIGN_OBSERVED, ref.FOREIGN_UNOBSERVED, ref.MAX_SLOTS)
    for cls in ("PointMap", "LocalPointsParams", "LocalPointsIO", "LocalPointsResult"):
        assert hasattr(hvo, cls)
    assert hasattr(hvo.Context, "search_local_points") and hasattr(hvo.Context, "batch_search_local_points") and hasattr(hvo.Stream, "search_local_points")


def test_bounds_edges_known_answers():
    """z = 2, so u = 256 x + 320 and v = 256 y + 240 exactly; 2^-20 in x moves u by 2^-12, which a float near 640 holds"""
    e, p, vc, lvl = frustum(world(0.25, -0.5, 2.0))
    assert e == 0 and p.tolist() == [384.0, 112.0, 352.0] and lvl == 4      # ur = u - 64 / 2; dist 2.077, ratio 1.93: ceil(3.6)
    eps = 2.0 ** -20
    for x, y, want in ((1.25, 0.0, 0), (1.25 + eps, 0.0, 3), (-1.25, 0.0, 0), (-1.25 - eps, 0.0, 2),
                       (0.0, 0.9375, 0), (0.0, 0.9375 + eps, 5), (0.0, -0.9375, 0), (0.0, -0.9375 - eps, 4)):
        e, p, _, _ = frustum(world(x, y, 2.0), normal=(1, 0, 0), mx=8.0, mn=0.5, limit=-1.0)
        assert e == want, (x, y, e, ref.EXITS[e])
        if want == 0:
            assert p[0] == F32(256 * x + 320) and p[1] == F32(256 * y + 240) and p[2] == F32(p[0] - 32)


def test_depth_sign_known_answers():
    """z is stated through the translation (Xw + tz with Xw = +-0): z = 0 and z = -0.0 pass `PcZ < 0.0f` and divide"""
    n100 = np.array([1, 0, 0], np.float32)

    def run(z, P, ty=-0.25):
        T = T_PERM.copy(); T[2, 3] = F32(z); T[1, 3] = F32(ty)
        R, t, Ow = ref.pose_parts(T)
        Pc = ref.transform(R, t, np.asarray(P, np.float32))
        return Pc, ref.is_in_frustum(np.asarray(P, np.float32), n100, F32(1e9), F32(0.0), CAM2, R, t, Ow, B4, ref.LOG_SF, 8, F32(-2.0))

    # X = 0 with z = 0: 0 * inf = NaN, and a NaN passes the four bounds tests
    Pc, (e, p, vc, lvl) = run(0.0, (0.0, -0.5, 0.25))
    assert Pc.tolist() == [0.0, 0.0, 0.0] and not np.signbit(Pc[2])
    assert e == 0 and math.isnan(p[0]) and math.isnan(p[1]) and math.isnan(p[2])
    # z = -0.0 (every product of the row and the translation are -0): not < 0, divides to -inf; X = Y = 0 make both projections NaN
    Pc, (e, p, vc, lvl) = run(-0.0, (-0.0, -0.5, -0.25), ty=0.25)
    assert Pc[2] == 0 and np.signbit(Pc[2]) and Pc[0] == 0 and Pc[1] == 0
    assert e == 0 and math.isnan(p[0]) and math.isnan(p[1])
    # the smallest step below zero fails
    assert run(-2.0 ** -20, (0.0, -0.5, 0.25))[1][0] == 1
    # X != 0 with z = 0: u = +inf fails the right bound, u = -inf the left one
    assert run(0.0, (0.0, 0.5, 0.25))[1][0] == 3 and run(0.0, (0.0, -1.5, 0.25))[1][0] == 2


def test_distance_limits_known_answers():
    """P on the optical axis: PO = (z, 0, 0), dist = z exactly.  mfMaxDistance = 2 gives maxD = 2 * float(1.2); mfMinDistance = 2 gives
    minD = 2 * float(0.8); z is put exactly there (z - 2 and back are exact: the operands are within a factor of two)"""
    zmax = F32(F32(1.2) * F32(2.0)); zmin = F32(F32(0.8) * F32(2.0))
    assert float(zmax) == 2 * float(F32(1.2)) and float(zmin) == 2 * float(F32(0.8))
    for z, mx, mn, want in ((zmax, 2.0, 0.5, 0), (zmax, np.nextafter(F32(2.0), F32(0)), 0.5, 7), (zmin, 8.0, 2.0, 0), (zmin, 8.0, np.nextafter(F32(2.0), F32(3)), 6)):
        P = world(0.0, 0.0, z)
        assert float(F32(P[0] + F32(2.0))) == float(z)
        if want == 7: assert F32(F32(1.2) * F32(mx)) < z
        if want == 6: assert F32(F32(0.8) * F32(mn)) > z
        e, p, vc, lvl = frustum(P, mx=mx, mn=mn)
        assert e == want, (z, mx, mn, ref.EXITS[e])
        if want == 0: assert p.tolist()[:2] == [320.0, 240.0] and vc == F32(1.0)


def test_view_cos_limit_known_answers():
    """PO = (2, 0, 0): viewCos = 2 nx / 2 = nx, whatever the other components"""
    P = world(0.0, 0.0, 2.0)
    e, _, vc, _ = frustum(P, normal=(0.5, 7.0, -3.0))
    assert e == 0 and vc == F32(0.5)
    assert frustum(P, normal=(np.nextafter(F32(0.5), F32(0)), 7.0, -3.0))[0] == 8
    assert frustum(P, normal=(0.25, 0, 0), limit=0.25)[0] == 0 and frustum(P, normal=(0.25, 0, 0), limit=0.2500001)[0] == 8


def test_level_and_clamp_known_answers():
    P = world(0.0, 0.0, 2.0)                                               # dist = 2
    for mx, want in ((2.0 * 1.2 ** 2.5, 3), (2.0 * 1.2 ** 0.5, 1), (2.0 * 1.2 ** 6.5, 7), (2.0 * 1.2 ** 7.5, 7), (2.0 * 1.2 ** 30, 7), (1.9, 0)):
        e, _, _, lvl = frustum(P, mx=mx, mn=0.1)
        assert e == 0 and lvl == want, (mx, lvl)
    # the lower clamp with a finer pyramid: ratio 0.85, log(0.85) / log(1.05) = -3.33, ceil -3, clamped to 0; unclamped it would be -3
    lsf = float(F32(np.log(F32(1.05))))
    assert ref.to_int(np.ceil(ref.predict_level_exact(F32(1.7), F32(2.0), lsf))) == -3
    assert frustum(P, mx=1.7, mn=0.1, log_sf=lsf)[3] == 0
    assert ref.predict_scale(F32(2.0), F32(0.0), ref.LOG_SF, 8) == 7 and ref.predict_scale(F32(np.nan), F32(1.0), ref.LOG_SF, 8) == 0     # inf saturates, NaN -> 0
    assert ref.predict_scale(F32(2.0 * 1.2 ** 2.5), F32(2.0), ref.LOG_SF, 3) == 2 and ref.predict_scale(F32(2.0 * 1.2 ** 2.5), F32(2.0), ref.LOG_SF, 1) == 0


def test_crafted_rows_of_the_gpu_test_leave_where_they_say():
    """the rows tests/test_point_map_gpu.py uploads: each leaves isInFrustum at the exit it names, under its own pose"""
    poses, rows = ref.crafted_gates()
    assert np.array_equal(poses["A"], np.array([[0, 1, 0, 0.5], [0, 0, 1, -0.25], [1, 0, 0, 2.0]], np.float32))
    M = ref.crafted_map(rows)
    want = {k: set() for k in range(9)}
    for key, T in poses.items():
        fp = ref.frustum_pass(M, CAM2, T, B4, ref.LOG_SF, 8, np.zeros(0, np.int32))
        for j, row in enumerate(rows):
            if row[1] == key:
                assert fp["exits"][j] == row[6], (row[0], ref.EXITS[fp["exits"][j]])
                want[row[6]].add(row[0])
    assert all(want[e] for e in range(9))                                 # every exit of the function occurs
    fpA = ref.frustum_pass(M, CAM2, poses["A"], B4, ref.LOG_SF, 8, np.zeros(0, np.int32))
    lv = {rows[j][0]: int(l) for j, l in zip(fpA["slots"], fpA["level"])}
    assert lv["level clamped high"] == 7 and lv["level clamped low"] == 0 and lv["viewCos on limit"] == 4


def test_generator_level_guard_and_patterns():
    T = ref.scene_pose()
    R, t, Ow = ref.pose_parts(T)
    for n, pattern in ((65, "alt"), (300, "wave"), (64, "all"), (65, "last"), (40, "none")):
        M, rejected = ref.make_map(n, pattern, T, seed=n)
        fp = ref.frustum_pass(M, ref.CAM, T, ref.BOUNDS, ref.LOG_SF, ref.N_LEVELS, np.zeros(0, np.int32))
        assert np.array_equal(fp["slots"], np.nonzero(ref.wanted_in_view(n, pattern))[0])
        for j in fp["slots"]:
            assert not ref.level_guard(M["max_dist"][j], ref._dist(M["pos"][j], Ow))
        out = fp["exits"][fp["exits"] > 0]
        if pattern in ("alt", "wave", "none"):
            assert {1, 3, 7, 8} <= set(out.tolist())                      # each of the four reasons occurs
    assert ref.level_guard(F32(2.0 * 1.2 ** 3), F32(2.0)) and not ref.level_guard(F32(2.0 * 1.2 ** 2.5), F32(2.0))


_scene = {}


def own_scene(synth, orc):
    """the committed synthetic scene's first frame with the CPU oracle's key points, and a map of that frame's own points unprojected under
    the true pose; the search runs under an estimate one centimetre off with th = 1, so that some windows miss (shared, not modified)"""
    if "s" not in _scene:
        g, d, _ = synth.make_sequence("std", 0x5EED7400, 1)
        kp, desc = orc.Orb().extract(g[0])
        ur, z = ref.stereo_from_depth(kp, kp, d[0], ref.CAM[4])
        T = ref.scene_pose(); Ts = ref.estimated_pose(T)
        good = np.nonzero(z > 0)[0]
        M = ref.empty_map(len(good), seed=3); M["observed"][:] = 1
        feats = ref.add_frame_points(M, kp, desc, z, T, range(len(good)))
        o = ref.search_local_points(M, ref.CAM, Ts, ref.BOUNDS, ref.LOG_SF, ref.N_LEVELS, ref.SF, 1.0, kp, ur, desc, np.full(len(kp), -1, np.int32))
        _scene["s"] = (kp, desc, ur, z, Ts, M, feats, o)
    return _scene["s"]


def test_not_vacuous_on_the_committed_scene(synth, orc):
    kp, desc, ur, z, T, M, feats, o = own_scene(synth, orc)
    n = len(M["pos"])
    assert n > 300 and o["n_in_view"] > 0.9 * n
    assert o["n_matches"] >= n / 2 and o["n_matches"] < n                 # at least half of the points with depth, and at least one unmatched
    # a matched point found its own feature or one with the same descriptor distance or better
    own = feats[o["in_view_slot"]]
    hit = o["match_idx"] >= 0
    assert (o["match_idx"][hit] == own[hit]).mean() > 0.9
    assert np.array_equal(np.sort(o["held"][o["held"] >= 0]), np.unique(o["held"][o["held"] >= 0]))      # observed points: one feature each


def test_search_agrees_with_the_guided_model(synth, orc, hvo):
    """the sequential restatement against the sort-based model of tests/guided_cases.py on the same query arrays, both occupancy kinds"""
    kp, desc, ur, z, T, M, feats, _ = own_scene(synth, orc)
    M = {k: v.copy() for k, v in M.items()}
    M["observed"] = (np.arange(len(M["pos"])) % 3 != 0).astype(np.uint8)
    held = np.full(len(kp), -1, np.int32); held[feats[5]] = ref.FOREIGN_OBSERVED; held[feats[6]] = ref.FOREIGN_UNOBSERVED; held[feats[7]] = 9
    for th in (1.0, 3.0, 5.0):
        fp = ref.frustum_pass(M, ref.CAM, T, ref.BOUNDS, ref.LOG_SF, ref.N_LEVELS, held)
        q = ref.queries(M, fp)
        nm, mi, md = ref.search_by_projection(*q, kp, ur, fp["t_occupied"], desc, ref.BOUNDS, th, ref.SF)
        r = F32(np.where(q[5].astype(np.float64) > 0.998, F32(2.5), F32(4.0)))
        if th != 1.0: r = (r * F32(th)).astype(F32)
        Q = gc.queries(q[1], q[2], (r * ref.SF[q[4]]).astype(F32), lo=q[4] - 1, hi=q[4], ur=q[3], blocks=q[6], desc=q[0])
        t = gc.NS(kp=kp, desc=desc, uright=ur, occ=fp["t_occupied"])
        c = gc.make("own", Q, t, {}, bounds=(ref.BOUNDS[0], ref.BOUNDS[2], ref.BOUNDS[1], ref.BOUNDS[3]))
        n2, i2, d2, _ = gc.model_search(c, "map")
        assert nm == n2 and np.array_equal(mi, i2) and np.array_equal(md[mi >= 0], d2[mi >= 0]), th
        assert nm > 100
    assert fp["t_occupied"][feats[5]] == 1 and fp["t_occupied"][feats[6]] == 0
