"""LocalMapping::CreateNewMapPoints on the GPU (csrc/new_points.hip) against tests/new_points_ref.py.  Integers are compared exactly, floats by
their bits (a NaN by being one).  tests/test_new_points.py asserts on the CPU that every crafted case says what it is meant to say and that
the random scene (seed new_points_ref.SCENE_SEED) is not vacuous; the conditions are asserted here again on the restatement's own output
before the device is compared with it.  The restatement runs the sequential chain; the device evaluates independent pairs and resolves."""
import numpy as np
import pytest

import new_points_ref as ref

pytestmark = pytest.mark.gpu
INT_KEYS = ("match_idx2", "match_dist", "outcome", "branch", "created_idx1", "created_idx2")
PAIR_KEYS = ("match_idx2", "match_dist", "outcome", "branch", "x3d")
_cache = {}


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def scene():
    """the random scene, 1000 features x 4 neighbours, and the restatement's answer, computed once"""
    if "scene" not in _cache:
        cur, kfs = ref.random_scene()
        _cache["scene"] = (cur, kfs) + ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    return _cache["scene"]


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    n = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), n) and np.array_equal(a[~n].view(np.uint32), b[~n].view(np.uint32))


def same(got, want, what=""):
    (gr, gs), (wr, ws) = got, want
    assert len(gr) == len(wr), what
    for j, (g, w) in enumerate(zip(gr, wr)):
        for k in INT_KEYS:
            assert np.array_equal(g[k], w[k]), (what, j, k, np.flatnonzero(np.asarray(g[k]) != np.asarray(w[k]))[:8] if len(g[k]) == len(w[k]) else (len(g[k]), len(w[k])))
        assert same_bits(g["x3d"], w["x3d"]), (what, j, "x3d", np.flatnonzero((g["x3d"] != w["x3d"]).any(axis=1))[:8])
        for k in ("n_created", "gate", "status"):
            assert g[k] == w[k], (what, j, k, g[k], w[k])
    assert np.array_equal(gs["owner"], ws["owner"]) and gs["n_new"] == ws["n_new"], (what, "summary")


def identical(a, b, what=""):
    (ar, asum), (br, bsum) = a, b
    assert len(ar) == len(br)
    for j, (x, y) in enumerate(zip(ar, br)):
        for k in INT_KEYS + ("x3d",):
            assert x[k].tobytes() == y[k].tobytes(), (what, j, k)
        assert (x["n_created"], x["gate"], x["status"]) == (y["n_created"], y["gate"], y["status"]), (what, j)
    assert asum["owner"].tobytes() == bsum["owner"].tobytes() and asum["n_new"] == bsum["n_new"], what


def untouched(hvo, res, summ):
    for r in res:
        for k in INT_KEYS + ("x3d",):
            assert len(r[k]) > 0 and (r[k] == hvo.NP_UNTOUCHED).all(), k
        assert r["n_created"] == r["gate"] == r["status"] == hvo.NP_UNTOUCHED
    assert (summ["owner"] == hvo.NP_UNTOUCHED).all() and summ["n_new"] == hvo.NP_UNTOUCHED


def run(hvo, cur, kfs, cam=ref.CAM, **kw):
    return ctx_of(hvo).create_new_map_points(cam, cur, kfs, **kw)


def both(hvo, cur, kfs, cam, what):
    got = run(hvo, cur, kfs, cam=cam)
    same(got, ref.full(cur, kfs, cam, cam[4]), what)
    return got[0], got[1]


def test_crafted_searches(hvo):
    """ties, the order of acceptance, dist 50 / 51, the epipolar bound from both sides, two idx1 on one idx2, nodes on one side, occupied
    features, octaves outside the pyramid; the epipole gate just inside and just outside; node sizes 1, 15, 16, 17, 65, 200; F12 = 0"""
    for name, c, n, want_idx, want_dist in ref.search_cases():
        res, _ = both(hvo, ref.side(c, mono=True), [ref.side(n, Tcw=ref.T_RIGHT, mono=True)], ref.CAM2, name)
        assert res[0]["match_idx2"].tolist() == want_idx and res[0]["match_dist"].tolist() == want_dist, name
    c, n, want = ref.bound_case()
    res, _ = both(hvo, ref.side(c, mono=True), [ref.side(n, Tcw=ref.T_RIGHT, mono=True)], ref.CAM2, "epipolar bound")
    assert res[0]["match_idx2"].tolist() == want == [0, -1]
    c, n, T, want = ref.epipole_case()
    res, _ = both(hvo, ref.side(c), [ref.side(n, Tcw=T, mb=0.0)], ref.CAM2, "epipole")
    assert res[0]["match_idx2"].tolist() == want == [-1, 1, 2]
    c, n, want = ref.node_size_case()
    res, summ = both(hvo, ref.side(c, mono=True), [ref.side(n, Tcw=ref.T_RIGHT, mono=True)], ref.CAM2, "node sizes")
    assert res[0]["match_idx2"].tolist() == want and (res[0]["match_dist"] == 3).all()
    assert all(ms > 0 for ms in summ["kernel_ms"])
    # a neighbour with the current pose and mb = 0: F12 = 0, den == 0 for every candidate, nothing matches
    c = [ref.pt(0.1 * k, 0.05 * k, 2.0, stereo=False, node=k) for k in range(5)]
    res, summ = both(hvo, ref.side(c, mono=True), [ref.side(c, Tcw=ref.IDENTITY, mb=0.0, mono=True)], ref.CAM2, "F12 = 0")
    assert res[0]["gate"] == 0 and (res[0]["match_idx2"] == -1).all() and (res[0]["outcome"] == ref.NO_MATCH).all() and summ["n_new"] == 0


def test_crafted_triangulations(hvo):
    """every outcome code and every branch, the chi-square gates (mono and stereo, both sides) on the bound and one float step beyond, W_ZERO,
    ZERO_DIST and NO_DEPTH, each with the answer tests/test_new_points.py states by hand"""
    seen = set()
    for cam, cases in ((ref.CAM2, ref.triangulation_cases()), (ref.CAM4, ref.reproj_bound_cases())):
        for name, a, b, T, mb1, mb2, want_o, want_b in cases:
            res, summ = both(hvo, ref.side([a], mb=mb1), [ref.side([b], Tcw=T, mb=mb2)], cam, name)
            assert (res[0]["outcome"][0], res[0]["branch"][0]) == (want_o, want_b), (name, res[0]["outcome"], res[0]["branch"])
            assert summ["n_new"] == (1 if want_o == ref.CREATED else 0) and res[0]["created_idx1"].tolist() == ([0] if want_o == ref.CREATED else []), name
            seen.add(int(res[0]["outcome"][0]))
    for name, a, T1, b, T2, mb1, mb2, want_o, want_b in ref.degenerate_cases():
        res, _ = both(hvo, ref.side([a], Tcw=T1, mb=mb1), [ref.side([b], Tcw=T2, mb=mb2)], ref.CAM2, name)
        assert (res[0]["outcome"][0], res[0]["branch"][0]) == (want_o, want_b), (name, res[0]["outcome"], res[0]["branch"])
        seen.add(int(res[0]["outcome"][0]))
    assert seen | {ref.OCCUPIED, ref.NO_MATCH} == set(range(12)), seen


@pytest.mark.parametrize("n1,n2", [(0, 5), (5, 0), (1, 1), (0, 0)])
def test_small_feature_counts(hvo, n1, n2):
    cur, kfs = ref.random_scene(n=max(n1, n2, 1), seed=3, poses=ref.SCENE_POSES[:1], twins=0, occupied=0.0)
    cut = lambda s, n: dict(s, **{k: (None if s[k] is None else s[k][:n]) for k in ("kp_un", "uright", "depth", "desc", "node_id", "has_map_point")})
    cur = cut(cur, n1); kfs = [cut(kfs[0], n2)]
    res, summ = both(hvo, cur, kfs, ref.CAM, "%d x %d" % (n1, n2))
    assert res[0]["status"] == 0 and len(res[0]["match_idx2"]) == n1 and (n1 and n2 or summ["n_new"] == 0)
    res0, summ0 = run(hvo, cur, [])                                  # n_kf == 0: HVO_OK with nothing created
    assert res0 == [] and summ0["n_new"] == 0 and (summ0["owner"] == -1).all() and len(summ0["owner"]) == n1


def test_random_scene(hvo):
    """1000 features, four neighbours (forward, lateral with yaw, below mb, lateral).  The conditions first, on the restatement"""
    cur, kfs, wres, wsum = scene()
    ref.vacuity(wres, wsum, 1000)
    for j, r in enumerate(wres):
        print("neighbour %d: gate %d, outcomes %s, branches of the created %s, ties %d, creates %d" % (
            j, r["gate"], np.bincount(r["outcome"], minlength=12), np.bincount(r["branch"][r["outcome"] == ref.CREATED], minlength=4), len(r["ties"]), r["n_created"]))
    got = run(hvo, cur, kfs)
    same(got, (wres, wsum), "scene")
    identical(got, run(hvo, cur, kfs), "twice")
    for r in got[0]:
        assert (np.diff(r["created_idx1"]) > 0).all()
    mono = dict(cur, uright=None, depth=None); kmono = [dict(k, uright=None, depth=None) for k in kfs]
    same(run(hvo, mono, kmono), ref.full(mono, kmono, ref.CAM, ref.CAM[4]), "every feature monocular")


def chain_scene():
    if "chain" not in _cache:
        poses = (ref.SCENE_POSES[0], ref.SCENE_POSES[1], ref.SCENE_POSES[3], ref.SCENE_POSES[2], (np.eye(3), (-0.2, 0.1, 0)))
        cur, kfs = ref.random_scene(n=300, seed=7, poses=poses, other_node=0.4, skip=(2,))
        _cache["chain"] = (cur, kfs) + ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    return _cache["chain"]


def test_chain(hvo):
    """five neighbours; number 2 carries the skip byte, number 3 lies below mb.  A point created by neighbour 0 keeps owner 0 although later
    neighbours report CREATED for it; a feature refused at 0 and 1 is created at 4, past the two neighbours that create nothing and block
    nothing; the results of the first k neighbours equal a call with only those k, byte for byte"""
    cur, kfs, wres, wsum = chain_scene()
    assert [r["gate"] for r in wres] == [0, 0, ref.GATE_SKIP, ref.GATE_BASELINE, 0]
    cr = np.stack([r["outcome"] == ref.CREATED for r in wres]); own = wsum["owner"]
    assert ((own == 0) & (cr[1] | cr[4])).sum() > 20 and ((own == 4) & ~cr[0] & ~cr[1]).sum() > 5 and ((own == 1) & ~cr[0]).sum() > 5
    assert not cr[2].any() and not cr[3].any() and wres[2]["n_created"] == wres[3]["n_created"] == 0
    got = run(hvo, cur, kfs)
    same(got, (wres, wsum), "chain")
    for r in got[0]:
        assert (np.diff(r["created_idx1"]) > 0).all()
    for k in range(1, 6):
        pre = run(hvo, cur, kfs[:k])
        for j in range(k):
            for key in INT_KEYS + ("x3d",):
                assert pre[0][j][key].tobytes() == got[0][j][key].tobytes(), (k, j, key)
            assert pre[0][j]["n_created"] == got[0][j]["n_created"]
        assert np.array_equal(pre[1]["owner"], np.where(got[1]["owner"] < k, got[1]["owner"], -1))


@pytest.mark.parametrize("width", [1, 10, 20, 64])
def test_widths(hvo, width):
    """`width` neighbours on a 200-feature key frame: each neighbour's pair results equal its own single-neighbour call; the owner is the first
    neighbour reporting CREATED and the lists are its features; ten neighbours are compared with the restatement's chain as well"""
    poses = [(ref.yaw(0.002 * j), (0.1 + 0.01 * j, 0.02 * (j % 3), 0.05 * (j % 4))) for j in range(width)]
    cur, kfs = ref.random_scene(n=200, seed=40 + width, poses=poses, twins=5)
    res, summ = run(hvo, cur, kfs)
    created = np.stack([r["outcome"] == ref.CREATED for r in res])
    owner = np.where(created.any(axis=0), created.argmax(axis=0), -1)
    assert np.array_equal(summ["owner"], owner) and summ["n_new"] == int((owner >= 0).sum()) > 100
    for j in range(width):
        one = run(hvo, cur, [kfs[j]])[0][0]
        for k in PAIR_KEYS:
            assert one[k].tobytes() == res[j][k].tobytes(), (j, k)
        idx1 = np.flatnonzero(owner == j)
        assert np.array_equal(res[j]["created_idx1"], idx1) and np.array_equal(res[j]["created_idx2"], res[j]["match_idx2"][idx1])
    if width == 10:
        same((res, summ), ref.full(cur, kfs, ref.CAM, ref.CAM[4]), "ten neighbours")


def test_ragged_neighbours(hvo):
    """neighbours of 65, 0, 300, 1 and 17 features in ONE call (every neighbour is padded to the stride of the largest), the empty one
    inside the list, neighbour 2 monocular, neighbour 0 alone with raw key points: the call equals the restatement, each neighbour's pair
    results equal its own single-neighbour call byte for byte, and so does the list with the empty neighbour moved to the front and to the end"""
    cur, kfs = ref.ragged_scene()
    want = ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    assert tuple(r["n_created"] for r in want[0]) == ref.RAGGED_CREATED and want[1]["n_new"] == 195
    got = run(hvo, cur, kfs)
    same(got, want, "ragged")
    for j, k in enumerate(kfs):
        one = run(hvo, cur, [k])[0][0]
        for key in PAIR_KEYS:
            assert one[key].tobytes() == got[0][j][key].tobytes(), (j, key)
    for order in ((1, 0, 2, 3, 4), (0, 2, 3, 4, 1)):
        perm = [kfs[j] for j in order]
        pgot = run(hvo, cur, perm)
        same(pgot, ref.full(cur, perm, ref.CAM, ref.CAM[4]), "empty neighbour at %d" % order.index(1))
        for pos, j in enumerate(order):
            for key in PAIR_KEYS:
                assert pgot[0][pos][key].tobytes() == got[0][j][key].tobytes(), (order, j, key)


def test_full_size(hvo):
    """4096 features on both sides, the limit itself (4097 is refused above): k_bow_csr sorts a full 32 KB of keys and the search key's 16-bit
    CSR position reaches its largest value.  Then every current feature occupied: every outcome is OCCUPIED and nothing is created"""
    cur, kfs = ref.full_size_scene()
    want = ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    assert want[1]["n_new"] == ref.FULL_SIZE_CREATED
    got = run(hvo, cur, kfs)
    same(got, want, "4096 x 4096")
    res, summ = run(hvo, dict(cur, has_map_point=np.ones(ref.MAX_FEATURES, np.uint8)), kfs)
    assert (res[0]["outcome"] == ref.OCCUPIED).all() and (res[0]["branch"] == 0).all() and res[0]["n_created"] == 0 and len(res[0]["created_idx1"]) == 0
    assert summ["n_new"] == 0 and (summ["owner"] == -1).all() and res[0]["status"] == 0


def test_stream_form_equals_the_host_form(hvo, synth):
    """the current key frame resident with its bag of words: the stream form equals the host-array form on the downloaded frame bit for bit,
    and the restatement; a frame without its bag of words is refused with the stream's error text"""
    import bow_ref
    g, d = synth.make_frame("std", 0x5EED0161)
    voc = bow_ref.make_vocabulary(4, 4, 161)
    v = hvo.Vocabulary(voc["k"], voc["L"], voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"], device=0)
    cam = ref.CAM + (ref.MB,)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=ref.CAM[4])
    try:
        tk = st.submit(g, d); fr = st.collect(tk)
        n = len(fr["kp_un"])
        assert n > 300 and (fr["uright"] >= 0).sum() > 100 and (fr["uright"] < 0).sum() > 0
        has = (np.arange(n) % 4 == 0).astype(np.uint8)
        kfs = None
        rc, msg, res, summ = st.create_new_map_points(tk, v, cam, ref.IDENTITY, has, [], check=False)
        assert rc == -1 and "bag of words" in msg and summ["n_new"] == hvo.NP_UNTOUCHED, (rc, msg)
        b = st.compute_bow(tk, v, levelsup=2)
        assert len(set(b["node_id"].tolist())) > 8
        kfs = ref.neighbours_of_frame(fr["kp_un"], fr["uright"], fr["zdepth"], fr["desc"], b["node_id"], (ref.SCENE_POSES[1], ref.SCENE_POSES[0]), ref.CAM, 161, ref.MB)
        cur = dict(kp_un=fr["kp_un"], kp=fr["kp"], uright=fr["uright"], depth=fr["zdepth"], desc=fr["desc"], node_id=b["node_id"], has_map_point=has, Tcw=ref.IDENTITY, mb=ref.MB)
        want = ref.full(cur, kfs, ref.CAM, ref.CAM[4])
        assert want[1]["n_new"] > 100 and len({int(x) for r in want[0] for x in r["branch"]}) == 4
        strm = st.create_new_map_points(tk, v, cam, ref.IDENTITY, has, kfs)
        host = run(hvo, cur, kfs)
        identical(strm, host, "stream")
        same(strm, want, "stream")
        identical(strm, st.create_new_map_points(tk, v, cam, ref.IDENTITY, has, kfs), "stream twice")
        rc, msg, res, summ = st.create_new_map_points(tk, v, cam, ref.IDENTITY, has, kfs, th_low=256, check=False)
        assert rc == -1 and "th_low" in msg
        untouched(hvo, res, summ)
    finally:
        st.close(); v.close()


def test_refusals_leave_the_outputs_untouched(hvo):
    cur, kfs = ref.random_scene(n=64, seed=9, poses=ref.SCENE_POSES[:2], twins=0)
    ctx = ctx_of(hvo)
    for kw, code, word in ((dict(th_low=256), -1, "th_low"), (dict(n_levels=0), -1, "n_levels"), (dict(n_levels=17), -1, "n_levels")):
        rc, msg, res, summ = ctx.create_new_map_points(ref.CAM, cur, kfs, check=False, **kw)
        assert rc == code and word in msg, msg
        untouched(hvo, res, summ)
    for missing in ("desc", "node_id", "has_map_point", "depth"):
        rc, msg, res, summ = ctx.create_new_map_points(ref.CAM, cur, [kfs[0], dict(kfs[1], n=len(kfs[1]["kp_un"]), **{missing: None})], check=False)
        assert rc == -1 and "neighbour 1" in msg, (missing, msg)
        untouched(hvo, res, summ)
    rc, msg, res, summ = ctx.create_new_map_points(ref.CAM, cur, [kfs[0]] * 65, check=False)
    assert rc == -4 and "65 neighbours" in msg, msg
    untouched(hvo, res, summ)
    nt = ref.MAX_FEATURES + 1
    fat = dict(kp_un=np.zeros(nt, ref.KP_DT), kp=None, uright=None, depth=None, desc=np.zeros((nt, 32), np.uint8), node_id=np.zeros(nt, np.int32),
               has_map_point=np.zeros(nt, np.uint8), Tcw=kfs[0]["Tcw"], mb=ref.MB)
    for c, k in ((cur, [kfs[0], fat]), (fat, kfs)):
        rc, msg, res, summ = ctx.create_new_map_points(ref.CAM, c, k, check=False)
        assert rc == -4 and "4097" in msg and "4096" in msg, msg
        untouched(hvo, res, summ)
    assert run(hvo, cur, kfs)[0][0]["status"] == 0                    # and the context goes on working


def test_example_runs(hvo, synth, tmp_path):
    """examples/create_map_points.cpp linked against the library and run on a synthetic frame: the resident current key frame against three
    neighbours, the caller's walk over the created lists, and the walk of a caller that leaves after neighbour 0"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "create_map_points")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "create_map_points.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d = synth.make_frame("std", 0x5EED0163)
    g.tofile(tmp_path / "g.u8"); d.tofile(tmp_path / "d.u16")
    out = subprocess.check_output([exe, str(tmp_path / "g.u8"), str(tmp_path / "d.u16")]).decode()
    print(out)
    nb = re.findall(r"neighbour (\d): gate (\d), (\d+) matches, (\d+) created", out)
    cur = re.search(r"current key frame: (\d+) features, (\d+) map points", out)
    end = re.search(r"created (\d+) new map points \(the call says (\d+)\); the current key frame now holds (\d+); leaving after neighbour 0: (\d+)", out)
    assert len(nb) == 3 and cur and end, out
    created = [int(x[3]) for x in nb]
    assert [int(x[1]) for x in nb] == [0, 2, 0] and created[1] == 0 and int(nb[1][2]) == 0
    assert created[0] > 50 and created[2] > 0 and int(nb[2][2]) > created[2]         # neighbour 2 matches features that neighbour 0 already served
    assert int(end.group(1)) == int(end.group(2)) == sum(created) and int(end.group(3)) == int(cur.group(2)) + sum(created) and int(end.group(4)) == created[0]
