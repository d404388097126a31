"""ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on the GPU (csrc/kf_search.hip) against tests/kf_search_ref.py.
Integers are compared exactly, floats by their bits (a NaN by being one: IEEE 754 leaves its sign and payload open).  tests/test_kf_search.py
asserts on the CPU that every crafted case says what it is meant to say and that the planted scene is not vacuous."""
import numpy as np
import pytest

import guided_cases as gc
import kf_search_ref as ref
import point_map_ref as pm

pytestmark = pytest.mark.gpu
B4 = pm.BOUNDS
INT_KEYS = ("gate", "level", "match_idx", "match_dist", "feature_kf")
_cache = {}


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def planted(hvo):
    """the planted scene and the restatement's two answers, computed once: (10, 100), then (3, 64) on what the first search left"""
    if "planted" not in _cache:
        cand, kp, desc = ref.planted_scene(hvo.KEYPOINT_DT)
        w1 = ref.search(cand, pm.CAM, kp, desc, B4, 10.0, 100)
        c2 = ref.after(cand, w1)
        _cache["planted"] = (cand, kp, desc, w1, c2, ref.search(c2, pm.CAM, kp, desc, B4, 3.0, 64))
    return _cache["planted"]


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    n = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), n) and np.array_equal(a[~n].view(np.uint32), b[~n].view(np.uint32))


def same(got, want, what=""):
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8])
    assert same_bits(got["proj"], want["proj"]), (what, "proj")
    for k in ("n_matches", "n_searched", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])


def identical(a, b, what=""):
    for k in INT_KEYS + ("proj",):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert (a["n_matches"], a["n_searched"], a["status"]) == (b["n_matches"], b["n_searched"], b["status"]), what


def untouched(hvo, out):
    for r in out:
        for k in INT_KEYS + ("proj",):
            assert (r[k] == hvo.KF_UNTOUCHED).all(), k
        assert r["n_matches"] == r["n_searched"] == r["status"] == hvo.KF_UNTOUCHED


def run(hvo, cand, kp, desc, th, orb_dist, cam=pm.CAM, **kw):
    return ctx_of(hvo).search_by_projection_keyframe(cam, kp, desc, B4, [cand], th=th, orb_dist=orb_dist, **kw)[0]


def test_crafted_gates(hvo):
    """every gate at its boundary and a step beyond, a point behind the camera, z == 0 and NaN: gate, proj and level of every row, and the
    search on the 80-feature frame"""
    cand, kp, desc, rows = ref.crafted_candidate(hvo.KEYPOINT_DT)
    got = run(hvo, cand, kp, desc, 10.0, 100, cam=ref.CAM2)
    same(got, ref.search(cand, ref.CAM2, kp, desc, B4, 10.0, 100), "crafted")
    for i, (name, _, _, _, _, g, uv, lvl) in enumerate(rows):
        assert got["gate"][i] == g and (got["level"][i] >= 0) == (g == 0), (name, got["gate"][i], got["level"][i])
        if lvl is not None: assert got["level"][i] == lvl, name
        if uv is not None: assert got["proj"][i, 0] == np.float32(uv[0]) and (uv[1] is None or got["proj"][i, 1] == np.float32(uv[1])), (name, got["proj"][i])
    names = [r[0] for r in rows]
    i = names.index("z = -2, in bounds, in range")
    assert got["match_idx"][i] == 15 and got["match_dist"][i] == 5 and got["feature_kf"][15] == i       # no depth-sign test
    i = names.index("z = 0, NaN")
    assert np.isnan(got["proj"][i]).all() and got["gate"][i] == 0 and got["match_idx"][i] == -1
    assert got["kernel_ms"][0] > 0 and got["kernel_ms"][1] > 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_degenerate_sizes(hvo, n):
    """n entries against frames of 0, 1 and 65 features; everything skipped; everything occupied"""
    _, kp, desc, _, _, _ = planted(hvo)
    kp, desc = kp[:65], desc[:65]
    cand = ref.planted_candidate(kp, desc, pm.scene_pose(0), seed=31 + n, n=n, feats=np.random.RandomState(n).permutation(65))
    for nt in (65, 1, 0):
        c = dict(cand, occupied=cand["occupied"][:nt])
        w = ref.search(c, pm.CAM, kp[:nt], desc[:nt], B4, 10.0, 100)
        same(run(hvo, c, kp[:nt], desc[:nt], 10.0, 100), w, "n %d nt %d" % (n, nt))
        if nt == 65 and n >= 63: assert w["n_matches"] > 10
        if nt == 0 or n == 0: assert w["n_matches"] == 0 and w["status"] == 0
    c = dict(cand, skip=np.ones(n, np.uint8))
    g = run(hvo, c, kp, desc, 10.0, 100)
    same(g, ref.search(c, pm.CAM, kp, desc, B4, 10.0, 100), "all skipped")
    assert g["n_searched"] == 0 and g["n_matches"] == 0 and (g["feature_kf"] == -1).all()
    c = dict(cand, occupied=np.ones(65, np.uint8))
    g = run(hvo, c, kp, desc, 10.0, 100)
    same(g, ref.search(c, pm.CAM, kp, desc, B4, 10.0, 100), "all occupied")
    assert g["n_matches"] == 0 and (n < 63 or g["n_searched"] > 30)
    c = dict(cand, occupied=None)                                  # no occupancy array: nothing is occupied
    same(run(hvo, c, kp, desc, 10.0, 100), ref.search(c, pm.CAM, kp, desc, B4, 10.0, 100), "occupied = NULL")


def test_claims(hvo):
    """a contested best: the first entry takes it, the second its runner-up, the third finds the band empty; an occupied feature is never
    taken although it is the best"""
    f = lambda x, y, d, o: (x, y, o, gc.flip(d), 0.0)
    ent = [(200.0, 200.0, gc.BASE, 0.0)] * 3
    feats = [f(201.0, 200.0, 9, 0), f(199.0, 201.0, 20, 2), f(200.0, 199.0, 1, 3), f(202.0, 202.0, 2, 1)]
    cand, kp, desc = ref.hand_scene(hvo.KEYPOINT_DT, ent, feats, occupied=(3,))
    g = run(hvo, cand, kp, desc, 3.0, 100, cam=ref.CAM2, check_orientation=False)
    assert g["match_idx"].tolist() == [0, 1, -1] and g["match_dist"].tolist() == [9, 20, 256] and g["feature_kf"].tolist() == [0, 1, -1, -1]
    cand["occupied"][3] = 0
    g = run(hvo, cand, kp, desc, 3.0, 100, cam=ref.CAM2, check_orientation=False)
    assert g["match_idx"].tolist() == [3, 0, 1] and g["feature_kf"].tolist() == [1, 2, -1, 0] and g["n_matches"] == 3


def test_chain_past_the_ranked_keys(hvo):
    """guided_cases.chain at nt = 100: one window with 100 candidates, 40 entries; from entry 16 on every one of the HVO_SBP_K = 16 ranked keys
    has been claimed by an earlier entry, so the rescan path runs; entry i takes the feature of rank i"""
    cand, kp, desc, th, idx, dist = ref.chain_scene(hvo.KEYPOINT_DT)
    g = run(hvo, cand, kp, desc, th, 100, cam=ref.CAM2, check_orientation=False)
    assert np.array_equal(g["match_idx"], idx) and np.array_equal(g["match_dist"], dist) and g["n_matches"] == 40
    same(g, ref.search(cand, ref.CAM2, kp, desc, B4, th, 100, check_orientation=False), "chain")
    # the 16 best features occupied at entry although nobody observes them: never taken, the chain starts at rank 16
    order = np.lexsort((np.arange(100), *gc.cells(kp, gc.B0)[1::-1], gc.ham(gc.BASE[None], desc)[0]))
    cand["occupied"][order[:16]] = 1
    g = run(hvo, cand, kp, desc, th, 100, cam=ref.CAM2, check_orientation=False)
    assert np.array_equal(g["match_idx"], order[16:56]) and not (g["feature_kf"][order[:16]] >= 0).any()
    same(g, ref.search(cand, ref.CAM2, kp, desc, B4, th, 100, check_orientation=False), "chain, occupied")


def test_orb_dist_boundary(hvo):
    """dist == ORBdist is accepted and ORBdist + 1 refused; orb_dist = 256 would accept bestIdx2 = -1: HVO_ERR_INVALID_ARG, outputs untouched"""
    f = lambda x, y, d: (x, y, 1, gc.flip(d), 0.0)
    ent = [(100.0, 100.0, gc.BASE, 0.0), (300.0, 100.0, gc.BASE, 0.0), (500.0, 100.0, gc.BASE, 0.0)]
    cand, kp, desc = ref.hand_scene(hvo.KEYPOINT_DT, ent, [f(101.0, 100.0, 64), f(301.0, 100.0, 65), f(501.0, 100.0, 256)])
    g = run(hvo, cand, kp, desc, 3.0, 64, cam=ref.CAM2, check_orientation=False)
    assert g["match_idx"].tolist() == [0, -1, -1] and g["match_dist"].tolist() == [64, 256, 256]
    g = run(hvo, cand, kp, desc, 3.0, 255, cam=ref.CAM2, check_orientation=False)
    assert g["match_idx"].tolist() == [0, 1, -1]                   # the complement (distance 256) never enters bestDist
    rc, msg, out = ctx_of(hvo).search_by_projection_keyframe(ref.CAM2, kp, desc, B4, [cand], th=3.0, orb_dist=256, check=False)
    assert rc == -1 and "orb_dist" in msg
    untouched(hvo, out)


def test_rotation(hvo):
    """four bins, the fourth is culled; the same input without the check keeps all; feature_kf is the inverse of match_idx after the cull"""
    cand, kp, desc, bins = ref.rotation_scene(hvo.KEYPOINT_DT, [(5, 3), (2, 3), (9, 3), (11, 1)])
    g = run(hvo, cand, kp, desc, 1.0, 0, cam=ref.CAM2)
    same(g, ref.search(cand, ref.CAM2, kp, desc, B4, 1.0, 0), "rotation")
    assert g["match_idx"].tolist() == list(range(9)) + [-1] and g["n_matches"] == 9 and g["match_dist"][9] == 256
    inv = np.full(len(kp), -1, np.int32); inv[g["match_idx"][g["match_idx"] >= 0]] = np.flatnonzero(g["match_idx"] >= 0)
    assert np.array_equal(g["feature_kf"], inv)
    off = run(hvo, cand, kp, desc, 1.0, 0, cam=ref.CAM2, check_orientation=False)
    assert off["match_idx"].tolist() == list(range(10)) and off["n_matches"] == 10
    off = run(hvo, dict(cand, angle=None), kp, desc, 1.0, 0, cam=ref.CAM2, check_orientation=False)       # the angles may be missing then
    assert off["match_idx"].tolist() == list(range(10))


def test_limits(hvo):
    """16385 entries: HVO_ERR_UNSUPPORTED, the message names both limits, nothing is written; so for n_levels and empty bounds"""
    cand, kp, desc, _, _, _ = planted(hvo)
    n = ref.MAX_ENTRIES + 1
    big = dict(pos=np.zeros((n, 3), np.float32), skip=np.zeros(n, np.uint8), max_dist=np.ones(n, np.float32), min_dist=np.ones(n, np.float32),
               desc=np.zeros((n, 32), np.uint8), angle=np.zeros(n, np.float32), Tcw=cand["Tcw"], occupied=None)
    rc, msg, out = ctx_of(hvo).search_by_projection_keyframe(pm.CAM, kp, desc, B4, [cand, big], check=False)
    assert rc == -4 and "16384" in msg and "65535" in msg and "16385" in msg, msg
    untouched(hvo, out)
    for kw in (dict(n_levels=0), dict(n_levels=17)):
        rc, msg, out = ctx_of(hvo).search_by_projection_keyframe(pm.CAM, kp, desc, B4, [cand], check=False, **kw)
        assert rc == -1 and "n_levels" in msg
        untouched(hvo, out)
    rc, msg, out = ctx_of(hvo).search_by_projection_keyframe(pm.CAM, kp, desc, (0.0, 0.0, 0.0, 480.0), [cand], check=False)
    assert rc == -1 and "bounds" in msg
    untouched(hvo, out)


def test_planted_scene(hvo):
    """1000 key-frame entries back-projected from a 1004-feature frame, searched under the estimated pose: (10, 100), then (3, 64) on what the
    first search left, as Relocalization runs them"""
    cand, kp, desc, w1, c2, w2 = planted(hvo)
    g1 = run(hvo, cand, kp, desc, 10.0, 100)
    same(g1, w1, "(10, 100)")
    assert g1["n_matches"] >= 50
    g2 = run(hvo, ref.after(cand, g1), kp, desc, 3.0, 64)
    same(g2, w2, "(3, 64)")
    assert g2["n_matches"] >= 1
    identical(g1, run(hvo, cand, kp, desc, 10.0, 100), "twice")


def test_three_candidates_in_one_call(hvo):
    """n_kf = 3 in one call, with different poses, sizes and occupancies, equals three single calls bit for bit (and the restatement)"""
    cand, kp, desc, w1, c2, w2 = planted(hvo)
    b = dict(cand, Tcw=pm.estimated_pose(pm.scene_pose(0), 0.02)); b = {k: (v[:700] if k not in ("Tcw", "occupied") else v) for k, v in b.items()}
    b["occupied"] = np.roll(cand["occupied"], 5)
    cs = [cand, b, c2]
    ctx = ctx_of(hvo)
    three = ctx.search_by_projection_keyframe(pm.CAM, kp, desc, B4, cs, th=10.0, orb_dist=100)
    for j, c in enumerate(cs):
        identical(three[j], ctx.search_by_projection_keyframe(pm.CAM, kp, desc, B4, [c], th=10.0, orb_dist=100)[0], "candidate %d" % j)
    same(three[0], w1, "first of three")
    same(three[1], ref.search(b, pm.CAM, kp, desc, B4, 10.0, 100), "second of three")
    assert not np.array_equal(three[0]["match_idx"][:700], three[1]["match_idx"])


def test_stream_form_equals_the_host_form(hvo, synth):
    """the frame resident: key-frame points back-projected from the frame's own key points; the stream form on the resident frame equals the
    host-array form on the downloaded frame bit for bit, and the restatement"""
    g = synth.make_frame("std", 0x5EED0141)[0]
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=0.0)
    try:
        assert tuple(float(v) for v in st.bounds) == B4
        tk = st.submit(g); fr = st.collect(tk)
        kp, desc = fr["kp_un"], fr["desc"]; nf = len(kp)
        assert nf > 300
        cs = [ref.planted_candidate(kp, desc, pm.scene_pose(j), seed=50 + j, n=n, pose_dx=0.005 * (j + 1)) for j, n in enumerate((600, 257))]
        cs[1]["occupied"] = np.roll(cs[1]["occupied"], 3)
        strm = st.search_by_projection_keyframe(tk, pm.CAM, nf, cs, th=10.0, orb_dist=100)
        host = ctx_of(hvo).search_by_projection_keyframe(pm.CAM, kp, desc, B4, cs, th=10.0, orb_dist=100)
        for j in range(2):
            identical(strm[j], host[j], "stream %d" % j)
            same(strm[j], ref.search(cs[j], pm.CAM, kp, desc, B4, 10.0, 100), "stream %d" % j)
            assert strm[j]["n_matches"] > 50
        identical(strm[0], st.search_by_projection_keyframe(tk, pm.CAM, nf, cs, th=10.0, orb_dist=100)[0], "stream twice")
        rc, msg, out = st.search_by_projection_keyframe(tk, pm.CAM, nf, cs, th=10.0, orb_dist=256, check=False)
        assert rc == -1 and "orb_dist" in msg
        untouched(hvo, out)
    finally:
        st.close()


def test_stream_without_the_orb_stage_is_refused_with_a_message(hvo, synth):
    g, d = synth.make_frame("std", 0x5EED0142)
    cand, kp, desc, _, _, _ = planted(hvo)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD, bf=0.0)
    try:
        t = st.submit(g); st.collect(t)
        with pytest.raises(hvo.HvoError, match="HVO_STAGE_ORB") as e:
            st.search_by_projection_keyframe(t, pm.CAM, len(kp), [cand])
        assert e.value.status == -1
    finally:
        st.close()


def test_example_runs(hvo, synth, tmp_path):
    """examples/relocalization_refine.cpp linked against the library and run on a synthetic frame: PoseOptimization -> clear outliers ->
    SearchByProjection (10, 100) -> PoseOptimization -> SearchByProjection (3, 64) -> PoseOptimization, nothing of the frame coming down in
    between.  Its key frame holds 70 map points in four roles (24 matched, 12 matched to a wrong feature, 22 unmatched, 12 unmatched and 6 px
    off), so that with the reference's thresholds every branch runs: 24 good, + 34 by the wide search, 46 good, + 12 by the narrow search,
    58 at the end.  The frame's key points come from the ORB extraction, which has no CPU restatement here: the counts are the scene's
    construction, the pinned restatement count (>= 50 at (10, 100)) is tests/test_kf_search.py's for the planted scene."""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "relocalization_refine")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "relocalization_refine.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d = synth.make_frame("std", 0x5EED0143)
    g.tofile(tmp_path / "g.u8"); d.tofile(tmp_path / "d.u16")
    out = subprocess.check_output([exe, str(tmp_path / "g.u8"), str(tmp_path / "d.u16")]).decode()
    print(out)
    m = re.search(r"final: (\d+) inliers", out)
    assert m and int(m.group(1)) >= 50, out
    wide = re.search(r"search \(10, 100\): (\d+) additional", out); narrow = re.search(r"search \(3, 64\): (\d+) additional", out)
    assert wide and narrow and int(wide.group(1)) >= 26 and int(narrow.group(1)) >= 1, out
