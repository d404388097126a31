"""LocalMapping::CreateNewMapPoints on the CPU: the restatement tests/new_points_ref.py checked against itself.  Every crafted case says what it
is meant to say (the answers are stated here by hand), the random scene (seed new_points_ref.SCENE_SEED) is not vacuous, the chain and the
independent-pairs formulation agree, and the Jacobi reading of cv::SVD::compute is as accurate as stated.  No GPU is needed."""
import math

import numpy as np

import new_points_ref as ref

_cache = {}


def scene():
    if "scene" not in _cache:
        cur, kfs = ref.random_scene()
        _cache["scene"] = (cur, kfs) + ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    return _cache["scene"]


def mono_pair(c, n, T=ref.T_RIGHT, **kw):
    res, summ = ref.full(ref.side(c, mono=True), [ref.side(n, Tcw=T, mono=True, **kw)], ref.CAM2, ref.CAM2[4])
    return res[0], summ


def test_the_crafted_pose_is_exact():
    """0.25 m to the right under CAM2: F12 has two entries, +-1/2048, and the epipolar distance is (y2 - y1)^2"""
    kc = ref.neighbour_constants(ref.CAM2, ref.pose(ref.IDENTITY), dict(Tcw=ref.T_RIGHT, mb=ref.MB2))
    assert kc["F"] == [[0.0, 0.0, 0.0], [0.0, 0.0, -1.0 / 2048], [0.0, 1.0 / 2048, 0.0]] and kc["gate"] == 0 and kc["baseline"] == 0.25
    assert ref.epipolar_dsqr(kc["F"], 100.0, 50.0, 300.0, 53.0)[1] == 9.0
    assert kc["ex"] == -math.inf and math.isnan(kc["ey"])       # the epipole of a sideways neighbour lies at infinity: 1.0f / 0


def test_crafted_searches_say_what_they_mean():
    for name, c, n, want_idx, want_dist in ref.search_cases():
        r, _ = mono_pair(c, n)
        assert r["match_idx2"].tolist() == want_idx and r["match_dist"].tolist() == want_dist, (name, r["match_idx2"], r["match_dist"])
    c, n, T, want = ref.epipole_case()
    res, _ = ref.full(ref.side(c), [ref.side(n, Tcw=T, mb=0.0)], ref.CAM2, ref.CAM2[4])
    kc = ref.neighbour_constants(ref.CAM2, ref.pose(ref.IDENTITY), dict(Tcw=T, mb=0.0))
    assert (kc["ex"], kc["ey"]) == (320.0, 240.0) and res[0]["match_idx2"].tolist() == want == [-1, 1, 2]
    c, n, want = ref.node_size_case()
    r, _ = mono_pair(c, n)
    assert r["match_idx2"].tolist() == want and (r["match_dist"] == 3).all() and len(n) == 1 + 15 + 16 + 17 + 65 + 200


def test_the_epipolar_bound_from_both_sides():
    """the two candidates' dsqr are the closest floats to 3.84 that a float y2 reaches (the step of y2 moves dsqr by four of its own steps)"""
    c, n, want = ref.bound_case()
    kc = ref.neighbour_constants(ref.CAM2, ref.pose(ref.IDENTITY), dict(Tcw=ref.T_RIGHT, mb=ref.MB2))
    d = [ref.epipolar_dsqr(kc["F"], 300.0, 2.0, 300.0, float(np.float32(r[1])))[1] for r in n]
    print("dsqr either side of 3.84:", d)
    assert d[0] < 3.84 < d[1] and d[1] - d[0] < 1e-6 and np.nextafter(np.float32(n[0][1]), np.float32(9)) == np.float32(n[1][1])
    assert mono_pair(c, n)[0]["match_idx2"].tolist() == want == [0, -1]


def test_f12_of_the_current_pose_is_zero_and_nothing_matches():
    c = [ref.pt(0.1 * k, 0.05 * k, 2.0, stereo=False, node=k) for k in range(5)]
    r, summ = mono_pair(c, c, T=ref.IDENTITY, mb=0.0)
    assert r["gate"] == 0 and (r["match_idx2"] == -1).all() and (r["outcome"] == ref.NO_MATCH).all() and summ["n_new"] == 0


def test_crafted_triangulations_say_what_they_mean():
    seen_o, seen_b = set(), set()
    for cam, cases in ((ref.CAM2, ref.triangulation_cases()), (ref.CAM4, ref.reproj_bound_cases())):
        for name, a, b, T, mb1, mb2, want_o, want_b in cases:
            _, _, r, s = ref.run_pair(a, b, T, cam=cam, mb1=mb1, mb2=mb2)
            assert (r["outcome"][0], r["branch"][0]) == (want_o, want_b), (name, ref.OUTCOMES[r["outcome"][0]], r["branch"][0])
            assert s["n_new"] == (1 if want_o == ref.CREATED else 0) and (r["x3d"][0] == 0).all() == (want_o in (ref.LOW_PARALLAX, ref.NO_DEPTH)), name
            seen_o.add(want_o); seen_b.add(want_b)
    for name, a, T1, b, T2, mb1, mb2, want_o, want_b in ref.degenerate_cases():
        _, _, r, _ = ref.run_pair(a, b, T2, T1=T1, mb1=mb1, mb2=mb2)
        assert (r["outcome"][0], r["branch"][0]) == (want_o, want_b), (name, ref.OUTCOMES[r["outcome"][0]])
        seen_o.add(want_o)
    assert seen_o | {ref.OCCUPIED, ref.NO_MATCH} == set(range(12)) and seen_b == {0, 1, 2, 3}      # (OCCUPIED and NO_MATCH: search_cases)


def test_the_chi_square_bounds_are_one_float_step_apart():
    """the eight bound cases come in pairs whose errors are adjacent floats: e * e <= limit < next(e) * next(e), in float products"""
    cases = ref.reproj_bound_cases()
    s2 = float(ref.SIGMA2[1])
    for k in range(0, len(cases), 2):
        on, off = cases[k], cases[k + 1]
        side_ = 1 if on[0].startswith("current") else 2
        col = 3 if "stereo" in on[0] else 0
        e0, e1 = np.float32(on[side_][col]), np.float32(off[side_][col])
        lim = (7.8 if "stereo" in on[0] else 5.991) * s2
        assert np.nextafter(e0, np.float32(9)) == e1 and float(e0 * e0) <= lim < float(e1 * e1), on[0]
        assert on[6] == ref.CREATED and off[6] in (ref.REPROJ_1, ref.REPROJ_2)


def test_random_scene_is_not_vacuous():
    cur, kfs, res, summ = scene()
    ref.vacuity(res, summ, 1000)
    assert [r["gate"] for r in res] == [0, 0, ref.GATE_BASELINE, 0]
    for j, r in enumerate(res):
        print("neighbour %d: gate %d, outcomes %s, branches of the created %s, ties %d, creates %d" % (
            j, r["gate"], np.bincount(r["outcome"], minlength=12), np.bincount(r["branch"][r["outcome"] == ref.CREATED], minlength=4), len(r["ties"]), r["n_created"]))


def test_the_chain_equals_independent_pairs_plus_resolve():
    """the device's formulation, in numpy, on the restatement's pair results: the owner is the first neighbour reporting CREATED under the initial
    occupancy, and its list is the owner's features in ascending order -- exactly what the sequential chain produced"""
    cur, kfs, res, summ = scene()
    created = np.stack([r["outcome"] == ref.CREATED for r in res])
    owner = np.where(created.any(axis=0), created.argmax(axis=0), -1)
    assert np.array_equal(owner, summ["owner"]) and summ["n_new"] == int((owner >= 0).sum()) > 600
    for j, r in enumerate(res):
        idx1 = np.flatnonzero(owner == j)
        assert np.array_equal(r["created_idx1"], idx1) and np.array_equal(r["created_idx2"], r["match_idx2"][idx1]) and r["n_created"] == len(idx1)
    # a prefix of the neighbours gives the prefix of the results
    for k in (1, 2, 3):
        pres, psum = ref.create_new_map_points(cur, kfs[:k], ref.CAM, ref.CAM[4])[:2]
        for j in range(k):
            assert np.array_equal(pres[j]["created_idx1"], res[j]["created_idx1"])


def test_the_ragged_scene_says_something():
    """the restatement's own answer on new_points_ref.ragged_scene: neighbours of 65, 0, 300, 1 and 17 features in one call, the empty one inside
    the list, neighbour 2 monocular, neighbour 0 alone with raw key points.  At least two neighbours create, one is empty, and the created
    points come from the triangulation and from a stereo branch, on the stereo neighbour and on the monocular one"""
    cur, kfs = ref.ragged_scene()
    assert tuple(len(k["kp_un"]) for k in kfs) == ref.RAGGED and ref.RAGGED[1] == 0 and max(ref.RAGGED) == len(cur["kp_un"]) == 300
    assert kfs[2]["uright"] is None and kfs[2]["depth"] is None and all(k["uright"] is not None for j, k in enumerate(kfs) if j != 2)
    assert [k["kp"] is not None for k in kfs] == [True, False, False, False, False] and not np.array_equal(kfs[0]["kp"]["x"], kfs[0]["kp_un"]["x"])
    res, summ = ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    assert tuple(r["n_created"] for r in res) == ref.RAGGED_CREATED and [r["gate"] for r in res] == [0] * 5 and summ["n_new"] == 195
    assert sum(r["n_created"] > 0 for r in res) >= 2
    for j in (0, 2):
        br = np.bincount(res[j]["branch"][res[j]["outcome"] == ref.CREATED], minlength=4)
        assert br[1] > 0 and br[2] + br[3] > 0, (j, br)
    br0 = np.bincount(res[0]["branch"][res[0]["outcome"] == ref.CREATED], minlength=4)
    assert br0[3] > 0                                                  # the neighbour's own stereo branch: the one that unprojects its RAW key point
    assert (res[1]["match_idx2"] == -1).all() and (res[1]["outcome"][cur["has_map_point"] == 0] == ref.NO_MATCH).all()


def test_the_full_size_scene_says_something():
    """4096 features on both sides (one more is refused), 64 nodes of 64 features each: the restatement creates 2563 points"""
    cur, kfs = ref.full_size_scene()
    assert len(cur["kp_un"]) == len(kfs[0]["kp_un"]) == ref.MAX_FEATURES == 4096 and len(kfs) == 1
    assert np.bincount(cur["node_id"]).max() == 64 and len(set(cur["node_id"].tolist())) == 64
    res, summ = ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    assert summ["n_new"] == res[0]["n_created"] == ref.FULL_SIZE_CREATED and res[0]["gate"] == 0
    full = dict(cur, has_map_point=np.ones(4096, np.uint8))
    ores, osum = ref.full(full, kfs, ref.CAM, ref.CAM[4])
    assert (ores[0]["outcome"] == ref.OCCUPIED).all() and osum["n_new"] == 0 and (osum["owner"] == -1).all()


def test_jacobi_reading_accuracy():
    """noise-free planted points, 200 pairs, baselines 0.1 .. 0.5 m, depths 0.5 .. 8 m: the restatement's linear triangulation against the same
    float32 A solved by numpy.linalg.svd in float64; at most 4 times the error of numpy.linalg.svd on the float32 A against the same solution
    (numpy hands a float32 matrix to the double LAPACK routine and rounds the result, so that error is one rounding of the vector)"""
    rng = np.random.RandomState(5)
    fx, fy, cx, cy = (ref.f32(v) for v in ref.CAM[:4])
    e_jac, e_f32 = [], []
    P1 = ref.pose(ref.IDENTITY)
    for _ in range(200):
        b = rng.uniform(0.1, 0.5); ang = rng.uniform(0, 2 * math.pi)
        T2 = ref.Tcw_of(ref.yaw(rng.uniform(-0.05, 0.05)), (b * math.cos(ang), b * math.sin(ang), 0.0))
        P2 = ref.pose(T2)
        X = np.array([rng.uniform(-1, 1), rng.uniform(-0.7, 0.7), 1.0]) * rng.uniform(0.5, 8)
        xn = []
        for R, t, _ in (P1, P2):
            Pc = np.array(R) @ X + np.array(t)
            xn += [ref.f32(Pc[0] / Pc[2]), ref.f32(Pc[1] / Pc[2])]
        A = ref.triangulation_rows(xn[0], xn[1], (P1[0], P1[1]), xn[2], xn[3], (P2[0], P2[1]))
        x = ref.svd4_last(A)
        got = np.array(x[:3]) / x[3]
        v64 = np.linalg.svd(np.array(A, np.float64))[2][3]; want = v64[:3] / v64[3]
        v32 = np.linalg.svd(np.array(A, np.float32))[2][3].astype(np.float64); lap = v32[:3] / v32[3]
        e_jac.append(np.linalg.norm(got - want) / np.linalg.norm(want)); e_f32.append(np.linalg.norm(lap - want) / np.linalg.norm(want))
    print("relative error against the float64 SVD of the same A: Jacobi reading max %.3g mean %.3g, numpy.linalg.svd on the float32 A max %.3g mean %.3g" % (
        max(e_jac), np.mean(e_jac), max(e_f32), np.mean(e_f32)))
    assert max(e_jac) <= 4 * max(e_f32), (max(e_jac), max(e_f32))


def test_stereo_parallax_reading_against_libm():
    """(d d - h h) / (d d + h h) against glibc's float cos(2 atan2(h, d)) over depths 0.1 .. 40 m: printed for DESIGN.md, not a threshold beyond
    a few float steps"""
    d = np.linspace(0.1, 40.0, 40001).astype(np.float32)
    h = np.float32(ref.MB) / np.float32(2)
    libm = np.cos(np.float32(2) * np.arctan2(h, d)).astype(np.float32)
    mine = np.array([ref.stereo_cos(ref.MB, float(v)) for v in d[::40]], np.float32)
    diff = np.abs(libm[::40].astype(np.float64) - mine.astype(np.float64)).max()
    print("largest difference from the float libm evaluation: %.3g (%.2f float steps at 1)" % (diff, diff / 2.0 ** -24))
    assert diff <= 4 * 2.0 ** -24


def test_host_tool_gives_the_same_answers(tmp_path):
    """tools/new_points_host.cpp, the single-thread loop that tools/new_points_timing.py times beside the device: the same created lists, the same
    points bit for bit and the same owners as the restatement, on the random scene and on every feature monocular"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import new_points_host_io as io
    import point_map_ref as pm
    exe = io.build(str(tmp_path), root)
    cur, kfs, res, summ = scene()
    assert io.same_answer(io.run(exe, str(tmp_path), cur, kfs, ref.CAM, pm.SF, ref.SIGMA2), res, summ)
    mono = dict(cur, uright=None, depth=None); kmono = [dict(k, uright=None, depth=None) for k in kfs[:2]]
    mres, msum = ref.full(mono, kmono, ref.CAM, ref.CAM[4])
    assert msum["n_new"] > 300 and io.same_answer(io.run(exe, str(tmp_path), mono, kmono, ref.CAM, pm.SF, ref.SIGMA2), mres, msum)
