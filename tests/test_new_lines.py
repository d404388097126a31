"""LocalMapping::CreateNewMapLinesConstraint on the CPU: the restatement tests/new_lines_ref.py checked against itself.  Every crafted case says
what it is meant to say (the answers are stated by hand in new_lines_ref), the random scene (seed new_lines_ref.SCENE_SEED) is not vacuous,
the sequential loops and the independent-triples formulation agree, and the end points are as accurate as the Jacobi reading of
cv::SVD::compute is stated to be.  No GPU is needed."""
import numpy as np

import new_lines_ref as ref

_cache = {}
Z = lambda n: np.zeros(n, np.uint8)


def scene():
    if "scene" not in _cache:
        cur, kfs = ref.random_scene()
        _cache["scene"] = (cur, kfs) + ref.full(cur, kfs)
    return _cache["scene"]


def test_the_crafted_views_are_exact():
    """the base segment projects to x = 384 / 320 / 448, y = 176 .. 304; F21 of the neighbour 0.25 m to the right has two entries"""
    rows = [ref.see(ref.PS, ref.PE, T) for T in (ref.IDENTITY, ref.T_R, ref.T_L)]
    assert [r[:4] for r in rows] == [(384.0, 176.0, 384.0, 304.0), (320.0, 176.0, 320.0, 304.0), (448.0, 176.0, 448.0, 304.0)]
    cur, kfs = ref.base_triple()
    k1 = ref.keyframe_constants(cur); k2 = ref.keyframe_constants(kfs[0], k1)
    assert k2["F21"] == [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0 / 2048], [0.0, -1.0 / 2048, 0.0]] and k2["gate"] == 0 and k2["baseline"] == 0.25
    assert k2["M"] == [[512.0, 0.0, 320.0, -128.0], [0.0, 512.0, 240.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    assert ref.sigma2_table()[:3] == [1.0, ref.f32(ref.f32(1.2) * ref.f32(1.2)), ref.f32(ref.f32(ref.f32(1.2) * ref.f32(1.2)) ** 2)]


def test_every_outcome_code_has_a_crafted_triple():
    seen = set()
    for name, cur, kfs, want in ref.full_call_cases():
        for pairing in (ref.AS_WRITTEN, ref.ALIGNED):                  # nothing is gated: the two pairings are one
            m, p, s = ref.full(cur, kfs, pairing=pairing)
            assert len(p) == 1 and int(p[0]["outcome"][0]) == want, (name, ref.N_CODES, int(p[0]["outcome"][0]))
            assert s["n_new"] == (1 if want == ref.CREATED else 0), name
            x = p[0]["line3d"][0]
            assert (x[:3] == 0).all() == (want < ref.W_ZERO_E and want != ref.CREATED) and (x[3:] == 0).all() == (want <= ref.W_ZERO_E and want != ref.CREATED), (name, x)
            assert (p[0]["outcome"][1:] == ref.NO_MATCH).all(), name   # the two lines beside it match nothing
        seen.add(want)
    cur, kfs = ref.idx_range_scene()
    assert int(ref.full(cur, kfs)[1][0]["outcome"][0]) == ref.IDX_RANGE
    seen.add(ref.IDX_RANGE)
    seen |= {w for _, _, w in ref.occupied_shift_scenes()}
    assert seen == set(range(ref.N_CODES)) - {ref.OCCUPIED_1, ref.W_ZERO_E}, sorted(seen)      # what whole calls reach
    for name, kw, want in ref.direct_cases():                           # the two that no call reaches, with their neighbours in the order
        assert ref.direct(**kw) == want, (name, ref.direct(**kw))
        seen.add(want)
    for cur, kfs, want in ref.occupied_shift_scenes():                 # the two occupancy codes a call reaches, through a shifted pair
        assert int(ref.full(cur, kfs)[1][0]["outcome"][0]) == want and ref.full(cur, kfs, pairing=ref.ALIGNED)[2]["n_new"] == 1
    assert seen == set(range(ref.N_CODES)), sorted(set(range(ref.N_CODES)) - seen)


def test_the_parallel_line_is_caught_by_the_epipolar_gate():
    """under the sideways baseline every epipolar line is horizontal: the horizontal segment's Result is 1, the vertical one's 0"""
    for name, cur, kfs, want in ref.full_call_cases():
        if want not in (ref.EPI_PARALLEL, ref.CREATED): continue
        k1 = ref.keyframe_constants(cur); kc = [ref.keyframe_constants(k, k1) for k in kfs]
        tr = {}
        ref.front(k1, kc[0], kc[1], cur["kl"][0], kfs[0]["kl"][0], kfs[1]["kl"][0], kfs[0]["linefn"][0], trace=tr)
        assert (tr["result1"], tr["result2"]) == ((1.0, 1.0) if want == ref.EPI_PARALLEL else (0.0, 0.0)), (name, tr)


def test_the_bounds_from_both_sides():
    """CosSita 0.0087, chi-square 3.84 and the 0.85 overlap: two ADJACENT floats of one input coordinate, the first passes the gate and the second
    is refused by it"""
    cases = ref.bound_cases()
    assert len(cases) == 6
    for k in range(0, 6, 2):
        (n0, c0, k0, w0), (n1, c1, k1, w1) = cases[k], cases[k + 1]
        assert ref.outcome00(c0, k0) == w0 != w1 == ref.outcome00(c1, k1), n0
        ends = lambda c, kf: np.array([[s["kl"][0][f] for f in ("sx", "sy", "ex", "ey")] for s in (c, kf[0], kf[1])], np.float32).reshape(-1)
        fa, fb = ends(c0, k0), ends(c1, k1)
        d = np.flatnonzero(fa != fb)
        assert len(d) >= 1 and all(np.nextafter(fa[i], np.float32(np.inf)) == fb[i] for i in d), (n0, fa[d], fb[d])
        print(n0, "->", w0, "|", w1, "at", fa[d], fb[d])
    assert [c[3] for c in cases[1::2]] == [ref.NOT_COPLANAR, ref.REPROJ, ref.OVERLAP_2]
    assert cases[0][3] != ref.NOT_COPLANAR and cases[2][3] == ref.CREATED and cases[4][3] == ref.CREATED


def test_a_nan_overlap_ratio_passes():
    o, ratios = ref.nan_overlap_case()
    assert o == ref.CREATED and len(ratios) == 3 and all(np.isnan(r1) and np.isnan(r2) for r1, r2 in ratios), (o, ratios)
    m, p, s = ref.full(*ref.nan_overlap_scene())                       # the whole call triangulates exactly the end points used above
    assert int(p[0]["outcome"][0]) == ref.CREATED and p[0]["line3d"][0].tolist() == [0.125, 0.25, 2.0, 0.375, 0.25, 2.0] and s["n_new"] == 1


def test_crafted_searches_say_what_they_mean():
    for name, d1, d2, h1, h2, th, nr, want in ref.search_cases():
        m, n = ref.search_for_triangulation(np.array(d1), np.array(d2), h1, h2, th, nr)
        assert m.tolist() == want and n == sum(w >= 0 for w in want), (name, m)
    d1, d2, th, want = ref.ratio_case()
    assert ref.search_for_triangulation(np.array(d1), np.array(d2), Z(3), Z(6), th, 0.85)[0].tolist() == want == [0, -1, 4]
    for d1, d2, want in ref.mad_cases():
        assert ref.search_for_triangulation(np.array(d1), np.array(d2), Z(5), Z(10))[0].tolist() == want
    assert [w.count(-1) for _, _, w in ref.mad_cases()] == [0, 1, 0]
    # fewer than two lines on either side: knnMatch(k = 2) cannot rank
    A = np.array(ref.search_cases()[0][1])
    assert (ref.search_for_triangulation(A, A[:1], Z(3), Z(1))[0] == -1).all() and (ref.search_for_triangulation(A[:1], A, Z(1), Z(3))[0] == -1).all()


def test_the_pairing_quirk():
    """three neighbours, the middle one gated: AS_WRITTEN applies match vector 2 to key frame 1"""
    cur, kfs = ref.gated_middle_scene()
    w = ref.full(cur, kfs, pairing=ref.AS_WRITTEN); a = ref.full(cur, kfs, pairing=ref.ALIGNED)
    assert [m["gate"] for m in w[0]] == [0, ref.GATE_BASELINE, 0] and w[2]["n_pairs"] == a[2]["n_pairs"] == 1
    assert [(p["kf2"], p["kf3"], p["mv2"], p["mv3"]) for p in w[1]] == [(0, 1, 0, 2)] and [(p["kf2"], p["kf3"], p["mv2"], p["mv3"]) for p in a[1]] == [(0, 2, 0, 2)]
    assert a[2]["n_new"] == 1 and a[1][0]["created_idx0"].tolist() == [0] and w[2]["n_new"] == 0 and int(w[1][0]["outcome"][0]) == ref.PARALLAX_S
    cur, kfs = ref.idx_range_scene()
    w = ref.full(cur, kfs, pairing=ref.AS_WRITTEN); a = ref.full(cur, kfs, pairing=ref.ALIGNED)
    assert int(w[1][0]["outcome"][0]) == ref.IDX_RANGE and int(a[1][0]["outcome"][0]) == ref.CREATED and int(w[0][2]["match_idx"][0]) == 2 and len(kfs[1]["kl"]) == 1


def test_random_scene_is_not_vacuous():
    cur, kfs, m, p, s = scene()
    assert len(cur["kl"]) == 200 and len(kfs) == 4 and s["n_pairs"] == 6 and all(x["gate"] == 0 for x in m)
    assert sum(x["n_created"] > 0 for x in p) >= 2
    created = np.stack([x["outcome"] == ref.CREATED for x in p])
    assert (created.sum(axis=0) >= 2).sum() >= 1                       # resolve decides
    codes = set(np.concatenate([x["outcome"] for x in p]).tolist())
    assert len(codes) >= 6, sorted(codes)
    print("matched", [x["n_matched"] for x in m], "created", [x["n_created"] for x in p], "codes", sorted(codes), "contested", int((created.sum(axis=0) >= 2).sum()))


def test_the_sequential_loops_equal_independent_triples_plus_resolve():
    for pairing, sc in ((ref.AS_WRITTEN, scene()), (ref.ALIGNED, scene()), (ref.AS_WRITTEN, None), (ref.ALIGNED, None)):
        if sc is None:
            cur, kfs = ref.random_scene(n=120, seed=7, skip=(1,))     # a gated neighbour inside the list: shifted pairs
            m, p, s = ref.full(cur, kfs, pairing=pairing)
        elif pairing == ref.AS_WRITTEN: cur, kfs, m, p, s = sc
        else:
            cur, kfs = sc[:2]; m, p, s = ref.full(cur, kfs, pairing=pairing)
        created = np.stack([x["outcome"] == ref.CREATED for x in p])
        owner = np.where(created.any(axis=0), created.argmax(axis=0), -1)
        assert np.array_equal(owner, s["owner_pair"]) and s["n_new"] == int((owner >= 0).sum())
        for q, x in enumerate(p):
            i0 = np.flatnonzero(owner == q)
            assert np.array_equal(x["created_idx0"], i0) and np.array_equal(x["created_idx1"], m[x["mv2"]]["match_idx"][i0]) and np.array_equal(x["created_idx2"], m[x["mv3"]]["match_idx"][i0])
    assert scene()[4]["n_new"] > 50


def test_end_points_against_a_float64_svd():
    """the restatement's end points against numpy.linalg.svd in float64 on the same float32 systems: at most 4 times the error of
    numpy.linalg.svd on the float32 matrix (the bound tests/test_new_points.py asserts for this solve)"""
    cur, kfs, m, p, s = scene()
    k1 = ref.keyframe_constants(cur); kc = [ref.keyframe_constants(k, k1) for k in kfs]
    e_jac, e_f32 = [], []
    for x in p:
        for ikl in np.flatnonzero(x["outcome"] == ref.CREATED):
            i1, i2 = int(m[x["mv2"]]["match_idx"][ikl]), int(m[x["mv3"]]["match_idx"][ikl])
            for A in ref.systems(k1, kc[x["kf2"]], kc[x["kf3"]], cur["kl"][ikl], kfs[x["kf2"]]["linefn"][i1], kfs[x["kf3"]]["linefn"][i2]):
                v = ref.svd4_last(A); got = np.array(v[:3]) / v[3]
                v64 = np.linalg.svd(np.array(A, np.float64))[2][3]; want = v64[:3] / v64[3]
                v32 = np.linalg.svd(np.array(A, np.float32))[2][3].astype(np.float64); lap = v32[:3] / v32[3]
                e_jac.append(np.linalg.norm(got - want) / np.linalg.norm(want)); e_f32.append(np.linalg.norm(lap - want) / np.linalg.norm(want))
    print("%d systems: Jacobi reading max %.3g mean %.3g, numpy.linalg.svd on the float32 A max %.3g mean %.3g" % (len(e_jac), max(e_jac), np.mean(e_jac), max(e_f32), np.mean(e_f32)))
    assert len(e_jac) > 100 and max(e_jac) <= 4 * max(e_f32), (max(e_jac), max(e_f32))


def test_host_tool_gives_the_same_answers(tmp_path):
    """tools/new_lines_host.cpp, the single-thread loop that tools/new_lines_timing.py times beside the device: the same created lists, the same
    end points bit for bit and the same owners as the restatement, on the random scene under both pairings, with a gated neighbour and on the
    toy map"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("new_lines_timing", os.path.join(root, "tools", "new_lines_timing.py"))
    io = importlib.util.module_from_spec(spec); spec.loader.exec_module(io)
    exe = io.build_host(str(tmp_path), root)
    cur, kfs, m, p, s = scene()
    assert io.same_answer(io.run_host(exe, str(tmp_path), cur, kfs), p, s)
    for pairing in (ref.AS_WRITTEN, ref.ALIGNED):
        c2, k2 = ref.random_scene(n=120, seed=7, skip=(1,))
        m2, p2, s2 = ref.full(c2, k2, pairing=pairing)
        assert s2["n_pairs"] == 3 and io.same_answer(io.run_host(exe, str(tmp_path), c2, k2, pairing=pairing), p2, s2)
    c3, k3 = ref.toy_map()
    m3, p3, s3 = ref.full(c3, k3)
    assert s3["n_new"] == 5 and io.same_answer(io.run_host(exe, str(tmp_path), c3, k3), p3, s3)
