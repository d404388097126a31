"""CPU checks of the restatement the GPU tests of the key-frame search compare against (tests/kf_search_ref.py): the names the feature
adds, hand-computed known answers of ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (reference
src/ORBmatcher.cc:1499-1628) under a pose whose arithmetic is exact, and that the planted scene the GPU tests run gives the search
something to find, something to refuse and something to contest.  No GPU call."""
import os
import re

import numpy as np

import guided_cases as gc
import kf_search_ref as ref
import point_map_ref as pm
from conftest import ROOT

F32 = np.float32
NEW = ["hvo_search_by_projection_keyframe", "hvo_stream_search_by_projection_keyframe"]
B4 = pm.BOUNDS


def project_one(pos, mx=4.0, mn=1.0, skip=0, cam=ref.CAM2):
    g, p, l = ref.project(np.asarray(pos, np.float32).reshape(1, 3), [skip], [F32(mx)], [F32(mn)], ref.T_CRAFTED, cam, B4, pm.LOG_SF, 8)
    return int(g[0]), p[0], int(l[0])


def test_the_header_and_the_binding_name_the_new_calls(hvo):
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in hvo.EXPORTS, n
    for t in ("hvo_kf_search_candidate", "hvo_kf_search_params", "hvo_kf_search_result"):
        assert re.search(r"}\s*%s;" % t, hdr), t
    assert "#define HVO_ABI_VERSION 3 " in hdr
    for cls in ("KfSearchCandidate", "KfSearchParams", "KfSearchResult"):
        assert hasattr(hvo, cls)
    assert hasattr(hvo.Context, "search_by_projection_keyframe") and hasattr(hvo.Stream, "search_by_projection_keyframe")
    assert (hvo.KF_SEARCH_MAX_ENTRIES, hvo.KF_SEARCH_MAX_FEATURES) == (ref.MAX_ENTRIES, ref.MAX_FEATURES) and tuple(hvo.KF_GATES) == ref.GATES
    hpp = open(os.path.join(ROOT, "include", "hvo.hpp")).read()
    assert "hvo_stream_search_by_projection_keyframe" in hpp and "hvo_search_by_projection_keyframe(" in hpp


def test_the_crafted_pose_is_exact():
    R, t, Ow = pm.pose_parts(ref.T_CRAFTED)
    assert np.array_equal(Ow, np.array([-2, -0.5, 0.25], np.float32))
    assert pm.transform(R, t, ref.world(0.5, 0.25, -2.0)).tolist() == [0.5, 0.25, -2.0]


def test_every_gate_at_its_boundary_and_one_step_beyond():
    """z = 2, so u = 256 x + 320 and v = 256 y + 240 exactly; 2^-20 in x or y moves u or v by 2^-12, which a float near 640 holds"""
    eps = 2.0 ** -20
    for x, y, want in ((1.25, 0.0, 0), (1.25 + eps, 0.0, 3), (-1.25, 0.0, 0), (-1.25 - eps, 0.0, 2),
                       (0.0, 0.9375, 0), (0.0, 0.9375 + eps, 5), (0.0, -0.9375, 0), (0.0, -0.9375 - eps, 4)):
        g, p, l = project_one(ref.world(x, y, 2.0), mx=8.0, mn=0.5)
        assert g == want, (x, y, g, ref.GATES[g])
        assert p[0] == F32(256 * x + 320) and p[1] == F32(256 * y + 240) and (l >= 0) == (want == 0)
    # the distance range, on the optical axis (PO = (z, 0, 0), dist3D = z): the factors 1.2f and 0.8f are the call's, the arguments are raw
    zmax = F32(F32(1.2) * F32(2.0)); zmin = F32(F32(0.8) * F32(2.0))
    assert project_one(ref.world(0, 0, zmax), mx=2.0, mn=0.5)[0] == 0
    assert project_one(ref.world(0, 0, zmax), mx=np.nextafter(F32(2.0), F32(0)), mn=0.5)[0] == 7
    assert project_one(ref.world(0, 0, zmin), mx=8.0, mn=2.0)[0] == 0
    assert project_one(ref.world(0, 0, zmin), mx=8.0, mn=np.nextafter(F32(2.0), F32(3)))[0] == 6
    g, p, l = project_one(ref.world(0, 0, 2.0), skip=1)
    assert (g, p.tolist(), l) == (1, [0.0, 0.0], -1)


def test_no_depth_sign_test():
    """a point at z = -2 whose projection is in bounds and whose distance is in range is searched, like its twin at z = +2: the image point is
    mirrored through the principal point; dist3D = sqrt(4 + 0.25 + 0.0625) for both, ratio 4 / 2.077 = 1.926, log / log 1.2 = 3.59: level 4"""
    g, p, l = project_one(ref.world(0.5, 0.25, 2.0))
    assert (g, p.tolist(), l) == (0, [448.0, 304.0], 4)
    g, p, l = project_one(ref.world(0.5, 0.25, -2.0))
    assert (g, p.tolist(), l) == (0, [192.0, 176.0], 4)
    # z == 0: inf is caught by a bounds test, a NaN passes all four
    g, p, l = project_one(ref.world(0, 0, 0.0), mx=1e9, mn=0.0)
    assert g == 0 and np.isnan(p).all() and l == 7
    assert project_one(ref.world(1.0, 0, 0.0), mx=1e9, mn=0.0)[0] == 3 and project_one(ref.world(-1.0, 0, 0.0), mx=1e9, mn=0.0)[0] == 2
    assert project_one(ref.world(0, 1.0, 0.0), mx=1e9, mn=0.0)[0] == 5 and project_one(ref.world(0, -1.0, 0.0), mx=1e9, mn=0.0)[0] == 4


def test_the_crafted_rows_say_what_the_restatement_computes(hvo):
    cand, kp, desc, rows = ref.crafted_candidate(hvo.KEYPOINT_DT)
    assert 35 <= len(cand["skip"]) <= 45 and len(kp) == 80
    gate, proj, level = ref.project(cand["pos"], cand["skip"], cand["max_dist"], cand["min_dist"], cand["Tcw"], ref.CAM2, B4, pm.LOG_SF, 8)
    for i, (name, _, _, _, _, g, uv, lvl) in enumerate(rows):
        assert gate[i] == g, (name, gate[i])
        assert (level[i] >= 0) == (g == 0), name
        if lvl is not None: assert level[i] == lvl, (name, level[i])
        if uv is not None:
            assert proj[i, 0] == F32(uv[0]) and (uv[1] is None or proj[i, 1] == F32(uv[1])), (name, proj[i])
    assert set(gate.tolist()) == set(range(8))
    r = ref.search(cand, ref.CAM2, kp, desc, B4, 10.0, 100)
    i = [x[0] for x in rows].index("z = -2, in bounds, in range")
    assert r["match_idx"][i] == 15 and r["match_dist"][i] == 5             # the point behind the camera finds the feature planted on its image point
    i = [x[0] for x in rows].index("z = 0, NaN")
    assert r["gate"][i] == 0 and r["match_idx"][i] == -1                    # a NaN window holds no feature
    assert r["n_matches"] == 18 and r["n_searched"] == int((gate == 0).sum())


def _feat(x, y, d, octave=1, base=gc.BASE, start=0, angle=0.0):
    return (x, y, octave, gc.flip(d, start, base), angle)


def test_acceptance_is_best_dist_le_orb_dist(hvo):
    """dist == ORBdist is accepted, ORBdist + 1 is refused; no ratio test: a runner-up at the same distance changes nothing"""
    ent = [(100.0, 100.0, gc.BASE, 0.0), (300.0, 100.0, gc.BASE, 0.0), (500.0, 100.0, gc.BASE, 0.0)]
    feats = [_feat(101.0, 100.0, 64), _feat(301.0, 100.0, 65), _feat(501.0, 100.0, 30, start=1), _feat(502.0, 100.0, 30, start=2)]
    cand, kp, desc = ref.hand_scene(hvo.KEYPOINT_DT, ent, feats)
    r = ref.search(cand, ref.CAM2, kp, desc, B4, 3.0, 64, check_orientation=False)
    assert r["level"].tolist() == [1, 1, 1] and r["match_idx"].tolist() == [0, -1, 2] and r["match_dist"].tolist() == [64, 256, 30] and r["n_matches"] == 2
    assert ref.search(cand, ref.CAM2, kp, desc, B4, 3.0, 65, check_orientation=False)["match_idx"].tolist() == [0, 1, 2]
    # a complement descriptor (distance 256) never enters bestDist, whatever ORBdist
    cand, kp, desc = ref.hand_scene(hvo.KEYPOINT_DT, ent[:1], [_feat(101.0, 100.0, 256)])
    assert ref.search(cand, ref.CAM2, kp, desc, B4, 3.0, 255, check_orientation=False)["match_idx"].tolist() == [-1]


def test_every_feature_blocks(hvo):
    """two entries contest one best feature: the first takes it, the second takes its runner-up; an occupied feature is skipped although
    it would be the best, and the level band is [level - 1, level + 1]: octaves 0 .. 2 at level 1, octave 3 is outside"""
    ent = [(200.0, 200.0, gc.BASE, 0.0), (200.0, 200.0, gc.BASE, 0.0), (200.0, 200.0, gc.BASE, 0.0)]
    feats = [_feat(201.0, 200.0, 9, octave=0), _feat(199.0, 201.0, 20, octave=2), _feat(200.0, 199.0, 1, octave=3), _feat(202.0, 202.0, 2, octave=1)]
    cand, kp, desc = ref.hand_scene(hvo.KEYPOINT_DT, ent, feats, occupied=(3,))
    r = ref.search(cand, ref.CAM2, kp, desc, B4, 3.0, 100, check_orientation=False)
    assert r["match_idx"].tolist() == [0, 1, -1] and r["match_dist"].tolist() == [9, 20, 256] and r["feature_kf"].tolist() == [0, 1, -1, -1]
    cand["occupied"][3] = 0
    r = ref.search(cand, ref.CAM2, kp, desc, B4, 3.0, 100, check_orientation=False)
    assert r["match_idx"].tolist() == [3, 0, 1] and r["feature_kf"].tolist() == [1, 2, -1, 0]
    ind = ref.search(cand, ref.CAM2, kp, desc, B4, 3.0, 100, sequential=False)
    assert ind["match_idx"].tolist() == [3, 3, 3]


def test_rotation_four_bins_the_fourth_is_culled(hvo):
    """three equal best bins and a fourth, smaller one (guided_cases' rot_3_3_3): bins 2, 5, 9 stay, bin 11 goes; feature_kf is the inverse
    of match_idx after the cull; the culled match's occupancy stayed while the loop ran"""
    cand, kp, desc, bins = ref.rotation_scene(hvo.KEYPOINT_DT, [(5, 3), (2, 3), (9, 3), (11, 1)])
    assert ref.three_maxima([0, 0, 3, 0, 0, 3, 0, 0, 0, 3, 0, 1] + [0] * 18) == (2, 5, 9)
    assert ref.three_maxima([0, 20, 2, 1] + [0] * 26) == (1, 2, -1) and ref.three_maxima([0, 20, 1, 1] + [0] * 26) == (1, -1, -1)
    r = ref.search(cand, ref.CAM2, kp, desc, B4, 1.0, 0)
    assert [r["hist"][b] for b in (2, 5, 9, 11)] == [3, 3, 3, 1] and sum(r["hist"]) == 10 and set(r["keep"]) == {2, 5, 9}
    assert r["match_idx"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, -1] and r["n_matches"] == 9 and r["feature_kf"].tolist() == list(range(9)) + [-1]
    assert r["match_dist"][9] == 256
    off = ref.search(cand, ref.CAM2, kp, desc, B4, 1.0, 0, check_orientation=False)
    assert off["match_idx"].tolist() == list(range(10)) and off["n_matches"] == 10
    assert np.array_equal(bins, [5] * 3 + [2] * 3 + [9] * 3 + [11])


def test_the_chain_runs_past_the_ranked_keys(hvo):
    """guided_cases.chain at nt = 100: 40 entries over one window of 100 candidates; from entry 16 on all 16 ranked keys are claimed"""
    cand, kp, desc, th, idx, dist = ref.chain_scene(hvo.KEYPOINT_DT)
    r = ref.search(cand, ref.CAM2, kp, desc, B4, th, 100, check_orientation=False)
    assert np.array_equal(r["match_idx"], idx) and np.array_equal(r["match_dist"], dist) and r["n_matches"] == 40 and len(set(idx.tolist())) == 40
    assert (r["level"] == 1).all() and gc.SBP_K == 16


def test_the_planted_scene_is_not_vacuous(hvo):
    cand, kp, desc = ref.planted_scene(hvo.KEYPOINT_DT)
    assert len(kp) == ref.N_FEATURES == 1004 and len(cand["skip"]) == ref.N_ENTRIES
    r = ref.search(cand, pm.CAM, kp, desc, B4, 10.0, 100)
    assert r["n_matches"] >= 50, r["n_matches"]
    cnt = np.bincount(r["gate"], minlength=8)
    assert (cnt[1:] >= 1).all() and cnt[0] >= 500, cnt
    # sequential claims matter: some entry's result is not its independent best (before the rotation cull)
    seq = ref.search(cand, pm.CAM, kp, desc, B4, 10.0, 100, check_orientation=False)
    ind = ref.search(cand, pm.CAM, kp, desc, B4, 10.0, 100, sequential=False)
    assert int((seq["match_idx"] != ind["match_idx"]).sum()) >= 1
    # the rotation cull removes something, and occupied features are never taken
    assert r["n_matches"] < seq["n_matches"] and not (cand["occupied"].astype(bool) & (r["feature_kf"] >= 0)).any()
    # points behind the camera are searched and matched
    behind = np.array([pm.transform(*pm.pose_parts(cand["Tcw"])[:2], cand["pos"][i])[2] < 0 for i in range(len(cand["skip"]))])
    assert (behind & (r["gate"] == 0)).sum() >= 10 and (behind & (r["match_idx"] >= 0)).sum() >= 10
    # no searched entry lies within 1e-4 of a level boundary (the level goes through a library log)
    for i in np.flatnonzero(r["gate"] == 0):
        assert not pm.level_guard(cand["max_dist"][i], ref.entry_dist(cand["pos"][i], cand["Tcw"])), i
    # the second search of Relocalization, (3, 64), on what the first left: it still has work and finds less
    r2 = ref.search(ref.after(cand, r), pm.CAM, kp, desc, B4, 3.0, 64)
    assert r2["n_searched"] == r["n_searched"] - r["n_matches"] and 1 <= r2["n_matches"] < r["n_matches"]
