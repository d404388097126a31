"""ORBmatcher::Fuse(pKF, vpMapPoints, th) on the GPU (csrc/fuse.hip) against tests/fuse_ref.py.  Integers are compared exactly, floats by
their bits (a NaN by being one: IEEE 754 leaves its sign and payload open).  tests/test_fuse.py asserts on the CPU that every crafted case
says what it is meant to say and that the random scene (seed fuse_ref.SCENE_SEED) is not vacuous; the caps are asserted here again on the
restatement's own output before the device is compared with it."""
import numpy as np
import pytest

import fuse_ref as ref
import point_map_ref as pm

pytestmark = pytest.mark.gpu
B4 = pm.BOUNDS
INT_KEYS = ("best_idx", "best_dist", "gate", "level", "fused_entry", "fused_idx")
_cache = {}


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def big(hvo):
    """the random scene, 1000 features x 1500 entries, and the restatement's answer, computed once"""
    if "big" not in _cache:
        kf, mp = ref.random_scene(hvo.KEYPOINT_DT, 1000, 1500)
        _cache["big"] = (kf, mp, ref.fuse(kf, mp, pm.CAM))
    return _cache["big"]


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    n = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), n) and np.array_equal(a[~n].view(np.uint32), b[~n].view(np.uint32))


def same(got, want, what=""):
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8] if len(got[k]) == len(want[k]) else (len(got[k]), len(want[k])))
    assert same_bits(got["proj"], want["proj"]), (what, "proj")
    for k in ("n_fused", "n_searched", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])


def identical(a, b, what=""):
    for k in INT_KEYS + ("proj",):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)
    assert (a["n_fused"], a["n_searched"], a["status"]) == (b["n_fused"], b["n_searched"], b["status"]), what


def untouched(hvo, out):
    for r in out:
        for k in INT_KEYS + ("proj",):
            assert len(r[k]) > 0 and (r[k] == hvo.FUSE_UNTOUCHED).all(), k
        assert r["n_fused"] == r["n_searched"] == r["status"] == hvo.FUSE_UNTOUCHED


def run(hvo, kf, mp, cam=pm.CAM, **kw):
    return ctx_of(hvo).fuse_points(cam, [kf], mp, B4, **kw)[0]


def test_crafted_gates(hvo):
    """every gate alone, z = 0 and NaN projections, the distance and viewing-angle limits on the limit and one step beyond, the level clamp"""
    rows = ref.crafted_gates()
    mp, skip = ref.rows_map(rows)
    kp, desc = ref.random_keyframe(hvo.KEYPOINT_DT, 80, 3)
    kf = dict(kp_un=kp, uright=None, desc=desc, Tcw=ref.T_CRAFTED, skip=skip)
    got = run(hvo, kf, mp, cam=ref.CAM2)
    same(got, ref.fuse(kf, mp, ref.CAM2), "crafted")
    for i, (name, _, _, _, _, _, g, p3, lvl) in enumerate(rows):
        assert got["gate"][i] == g and (got["level"][i] >= 0) == (g == 0), (name, got["gate"][i], got["level"][i])
        if lvl is not None: assert got["level"][i] == lvl, name
        if p3 is not None:
            for k in range(3):
                if p3[k] is not None: assert got["proj"][i, k] == np.float32(p3[k]), (name, k, got["proj"][i])
    i = [r[0] for r in rows].index("z = 0: NaN projection fails IsInImage")
    assert np.isnan(got["proj"][i, :2]).all() and got["gate"][i] == ref.OUT_OF_IMAGE
    assert all(ms > 0 for ms in got["kernel_ms"])


def test_crafted_searches(hvo):
    """the chi-square gates one float step either side of 7.8 and 5.99, uright = NULL, the two ties, the feature outside the grid, the level
    band and th_low, each with the answer tests/test_fuse.py states by hand"""
    dt = hvo.KEYPOINT_DT
    kf, mp, want = ref.chi2_cases(dt)
    g = run(hvo, kf, mp, cam=ref.CAM2)
    same(g, ref.fuse(kf, mp, ref.CAM2), "chi2")
    assert g["best_idx"].tolist() == [0, -1, 2, -1, 4]
    g = run(hvo, dict(kf, uright=None), mp, cam=ref.CAM2)
    assert g["best_idx"].tolist() == [0, -1, 2, 3, -1]
    kf, mp = ref.tie_cases(dt)
    g = run(hvo, kf, mp, cam=ref.CAM2)
    same(g, ref.fuse(kf, mp, ref.CAM2), "ties")
    assert g["best_idx"].tolist() == [1, 2, -1] and g["best_dist"].tolist() == [9, 9, 256] and g["fused_entry"].tolist() == [0, 1] and g["fused_idx"].tolist() == [1, 2]
    # the level band: feature k has distance 4 + k; feature 0, the nearest descriptor, lies below the band (or above it), feature 1 inside
    for level, octaves in ((3, (1, 2, 3, 4)), (0, (1, 0, -1)), (7, (5, 6, 7))):
        kf, mp = ref.hand_scene(dt, [(300.0, 200.0, ref.BASE)], [(300.5, 200.0, q, ref.flip(4 + k)) for k, q in enumerate(octaves)], uright=False, level=level)
        if level == 7: mp["max_dist"][0] = np.float32(mp["max_dist"][0] * 1.2 ** 20)       # far past the top: PredictScale clamps
        g = run(hvo, kf, mp, cam=ref.CAM2)
        same(g, ref.fuse(kf, mp, ref.CAM2), "band %d" % level)
        assert g["level"][0] == level and g["best_idx"][0] == 1 and g["best_dist"][0] == 5, (level, g["best_idx"], g["best_dist"])
    ent = [(100.0, 100.0, ref.BASE), (300.0, 100.0, ref.BASE), (500.0, 100.0, ref.BASE)]
    kf, mp = ref.hand_scene(dt, ent, [(101.0, 100.0, 1, ref.flip(50)), (301.0, 100.0, 1, ref.flip(51)), (501.0, 100.0, 1, ref.flip(256))], uright=False)
    g = run(hvo, kf, mp, cam=ref.CAM2)
    assert g["best_dist"].tolist() == [50, 51, 256] and g["fused_entry"].tolist() == [0] and g["n_fused"] == 1
    assert run(hvo, kf, mp, cam=ref.CAM2, th_low=51)["fused_entry"].tolist() == [0, 1]


@pytest.mark.parametrize("nt", [0, 1, 63, 64, 65])
def test_sizes(hvo, nt):
    """nt features against 0, 1, 15, 16, 17, 255, 256 and 257 entries: the group of 16 lanes, the block of 256 entries and the compaction's
    block offsets at and around their sizes"""
    for n in (0, 1, 15, 16, 17, 255, 256, 257):
        kf, mp = ref.random_scene(hvo.KEYPOINT_DT, nt, n, seed=100 + nt)
        w = ref.fuse(kf, mp, pm.CAM)
        g = run(hvo, kf, mp)
        same(g, w, "nt %d n %d" % (nt, n))
        if nt == 0 or n == 0: assert w["n_fused"] == 0 and g["status"] == 0 and (g["best_idx"] == -1).all()
        if nt >= 63 and n >= 255: assert w["n_fused"] > 40, w["n_fused"]


def test_random_scene(hvo):
    """1000 features x 1500 entries.  The caps first, on the restatement: a quarter fused, every gate code, a tie at the best distance"""
    kf, mp, w = big(hvo)
    ref.vacuity(w, 1500)
    print("fused %d of 1500, searched %d, entries with a tie %d, gates %s" % (w["n_fused"], w["n_searched"], int((w["n_ties"] > 1).sum()), np.bincount(w["gate"], minlength=7)))
    g = run(hvo, kf, mp)
    same(g, w, "big")
    identical(g, run(hvo, kf, mp), "twice")
    same(run(hvo, dict(kf, uright=None), mp), ref.fuse(dict(kf, uright=None), mp, pm.CAM), "mono")


def test_crowded_cell(hvo):
    """200 features in one cell: one group of 16 lanes loops 13 times over a single CSR run"""
    kf, mp = ref.random_scene(hvo.KEYPOINT_DT, 200, 257, seed=ref.SCENE_SEED + 3, crowd=200)
    w = ref.fuse(kf, mp, pm.CAM)
    grid, _, _ = pm.build_grid(kf["kp_un"], B4)
    assert max(len(v) for v in grid.values()) == 200 and w["n_cand"].max() >= 8 and w["n_fused"] * 4 >= 257
    same(run(hvo, kf, mp), w, "crowded")


def test_key_frames_in_one_call(hvo):
    """n_kf = 3 with a map side of its own each (different sizes), and n_kf = 31 against one shared map side: each equals its single call
    and the restatement; the shared form equals the per-key-frame form given the same map 31 times"""
    ctx = ctx_of(hvo)
    sc = [ref.random_scene(hvo.KEYPOINT_DT, nt, n, seed=200 + j, pose=j, pose_dx=0.001 * (j + 1)) for j, (nt, n) in enumerate(((65, 257), (300, 100), (64, 17)))]
    three = ctx.fuse_points(pm.CAM, [s[0] for s in sc], [s[1] for s in sc], B4)
    for j, (kf, mp) in enumerate(sc):
        same(three[j], ref.fuse(kf, mp, pm.CAM), "per key frame %d" % j)
        identical(three[j], run(hvo, kf, mp), "per key frame %d alone" % j)
    kf0, mp = ref.random_scene(hvo.KEYPOINT_DT, 65, 40, seed=300)
    kfs = []
    for j in range(31):
        kf, _ = ref.random_scene(hvo.KEYPOINT_DT, 65, 40, seed=300, pose_dx=0.0005 * j)       # the same features, another pose, another skip set
        kf["skip"] = ((np.arange(40) + j) % 7 == 0).astype(np.uint8)
        kfs.append(kf)
    shared = ctx.fuse_points(pm.CAM, kfs, mp, B4)
    each = ctx.fuse_points(pm.CAM, kfs, [mp] * 31, B4)
    nf = 0
    for j in range(31):
        identical(shared[j], each[j], "shared %d" % j)
        same(shared[j], ref.fuse(kfs[j], mp, pm.CAM), "shared %d" % j)
        nf += shared[j]["n_fused"]
    assert nf > 31 * 5 and len({r["n_fused"] for r in shared}) > 1


def test_ragged_key_frames(hvo):
    """four key frames in ONE call with a map side each: 65, 0, 300 and 64 features against 257, 40, 0 and 17 entries -- an empty key frame
    and an empty map side inside the list --, uright = NULL on key frame 2, skip = NULL on key frame 1.  include/hvo.h allows n = 0 on either
    side with NULL arrays and a NULL skip: each key frame equals the restatement and its own single call.  Then the same four key frames
    against ONE shared map side"""
    ctx = ctx_of(hvo)
    kfs, maps, shared_kfs, shared = ref.ragged_keyframes(hvo.KEYPOINT_DT)
    assert [(len(k["kp_un"]), len(m["pos"])) for k, m in zip(kfs, maps)] == list(ref.RAGGED)
    got = ctx.fuse_points(pm.CAM, kfs, maps, B4)
    for j, (kf, mp) in enumerate(zip(kfs, maps)):
        same(got[j], ref.fuse(kf, mp, pm.CAM), "ragged %d" % j)
        identical(got[j], run(hvo, kf, mp), "ragged %d alone" % j)
    assert got[0]["n_fused"] > 40 and got[3]["n_fused"] > 3 and got[1]["n_fused"] == got[2]["n_fused"] == 0
    assert got[1]["n_searched"] == 40 and (got[1]["best_idx"] == -1).all() and len(got[2]["best_idx"]) == 0 and got[2]["status"] == 0
    sh = ctx.fuse_points(pm.CAM, shared_kfs, shared, B4)
    for j, kf in enumerate(shared_kfs):
        same(sh[j], ref.fuse(kf, shared, pm.CAM), "shared %d" % j)
        identical(sh[j], run(hvo, kf, shared), "shared %d alone" % j)
    assert sh[2]["n_fused"] > 40 and sh[1]["n_fused"] == 0 and sh[1]["n_searched"] > 100


def test_slot_form(hvo):
    """the map side as slots of a resident point map equals the array form on the same points: a permuted subset of the slots, a bad slot
    (counted as skipped), and a slot past the map's end, which is refused whole"""
    kf, mp, _ = big(hvo)
    n = 300
    m = hvo.PointMap(0, 16)
    try:
        m.set_many(0, mp["pos"][:n], mp["normal"][:n], mp["max_dist"][:n], mp["min_dist"][:n], mp["desc"][:n])
        m.set_bad(7)
        slots = np.random.RandomState(4).permutation(n)[:257].astype(np.int32)
        assert 7 in slots
        sub = {k: np.asarray(v)[slots] for k, v in mp.items()}
        skip = kf["skip"][slots].copy()
        kfa = dict(kf, skip=np.where(slots == 7, 1, skip).astype(np.uint8))
        want = run(hvo, kfa, sub)
        got = ctx_of(hvo).fuse_points_slots(m, slots, pm.CAM, [dict(kf, skip=skip)], B4)[0]
        identical(got, want, "slots")
        same(got, ref.fuse(kfa, sub, pm.CAM), "slots")
        assert got["gate"][list(slots).index(7)] == ref.SKIP and got["n_fused"] > 40
        two = ctx_of(hvo).fuse_points_slots(m, slots, pm.CAM, [dict(kf, skip=skip), dict(kf, skip=skip, uright=None)], B4)
        identical(two[0], want, "slots, two key frames")
        bad = slots.copy(); bad[100] = n
        rc, msg, out = ctx_of(hvo).fuse_points_slots(m, bad, pm.CAM, [dict(kf, skip=skip)], B4, check=False)
        assert rc == -1 and "slot 300" in msg and "slot 300" in hvo.lib().hvo_point_map_last_error(m.h).decode(), msg
        untouched(hvo, out)
        empty = ctx_of(hvo).fuse_points_slots(m, np.zeros(0, np.int32), pm.CAM, [dict(kf, skip=None)], B4)[0]
        assert empty["n_fused"] == 0 and empty["status"] == 0 and len(empty["best_idx"]) == 0
    finally:
        m.close()


def test_refusals_leave_the_outputs_untouched(hvo):
    kf, mp, _ = big(hvo)
    ctx = ctx_of(hvo)
    for kw, code, word in ((dict(th_low=256), -1, "th_low"), (dict(n_levels=0), -1, "n_levels"), (dict(n_levels=17), -1, "n_levels")):
        rc, msg, out = ctx.fuse_points(pm.CAM, [kf], mp, B4, check=False, **kw)
        assert rc == code and word in msg, msg
        untouched(hvo, out)
    rc, msg, out = ctx.fuse_points(pm.CAM, [kf], mp, (0.0, 0.0, 0.0, 480.0), check=False)
    assert rc == -1 and "bounds" in msg
    untouched(hvo, out)
    nt = ref.MAX_FEATURES + 1
    fat = dict(kp_un=np.zeros(nt, hvo.KEYPOINT_DT), uright=None, desc=np.zeros((nt, 32), np.uint8), Tcw=kf["Tcw"], skip=None)
    rc, msg, out = ctx.fuse_points(pm.CAM, [kf, fat], mp, B4, check=False)
    assert rc == -4 and "65535" in msg and "65536" in msg, msg
    untouched(hvo, out)
    assert run(hvo, kf, mp)["status"] == 0                          # and the context goes on working


def test_65535_features_and_65536_entries(hvo):
    """the limits themselves are served: a key frame of 65535 features (the last CSR position a 16-bit rank holds) whose last feature is an
    entry's only candidate, and 65536 entries of which only a few are not skipped"""
    nt = ref.MAX_FEATURES
    rng = np.random.RandomState(9)
    kp = np.zeros(nt, hvo.KEYPOINT_DT); kp["size"] = 31; kp["class_id"] = -1
    kp["x"] = rng.uniform(8, 600, nt).astype(np.float32); kp["y"] = rng.uniform(8, 440, nt).astype(np.float32); kp["octave"] = 5
    kp["x"][-1] = 634.0; kp["y"][-1] = 474.0; kp["octave"][-1] = 1            # alone in the last cell (63, 47): CSR position 65534
    desc = rng.randint(0, 256, (nt, 32)).astype(np.uint8); desc[-1] = ref.flip(7)
    grid, _, _ = pm.build_grid(kp, B4)
    assert grid[(63, 47)] == [nt - 1] and sum(len(v) for v in grid.values()) == nt
    n = 65536
    kf1, mp1 = ref.hand_scene(hvo.KEYPOINT_DT, [(633.0, 473.0, ref.BASE), (300.0, 200.0, ref.BASE)], [(634.0, 474.0, 1, ref.flip(7))], uright=False)
    mp = {k: np.zeros((n,) + np.asarray(v).shape[1:], np.asarray(v).dtype) for k, v in mp1.items()}
    for k in mp: mp[k][[5, n - 1]] = mp1[k]
    skip = np.ones(n, np.uint8); skip[[5, n - 1]] = 0
    kf = dict(kp_un=kp, uright=None, desc=desc, Tcw=ref.T_CRAFTED, skip=skip)
    g = run(hvo, kf, mp, cam=ref.CAM2)
    assert g["best_idx"][5] == nt - 1 and g["best_dist"][5] == 7 and g["gate"][n - 1] == 0 and g["n_searched"] == 2
    assert g["fused_entry"].tolist() == [5] and g["fused_idx"].tolist() == [nt - 1] and (g["gate"][skip == 1] == ref.SKIP).all()


def test_stream_form_equals_the_host_form(hvo, synth):
    """the frame resident with its mvuRight: the entries are its own key points unprojected at their depth, searched under a perturbed pose;
    arrays and slots; the stream form equals the host-array form on the downloaded frame bit for bit, and the restatement"""
    g, d = synth.make_frame("std", 0x5EED0151)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=pm.CAM[4])
    m = hvo.PointMap(0, 16)
    try:
        assert tuple(float(v) for v in st.bounds) == B4
        tk = st.submit(g, d); fr = st.collect(tk)
        kp, desc, ur, zd = fr["kp_un"], fr["desc"], fr["uright"], fr["zdepth"]
        assert len(kp) > 300 and (ur >= 0).sum() > 100
        kf, mp = ref.random_scene(hvo.KEYPOINT_DT, 0, 700, seed=61, frame=(kp, desc, ur, zd))
        w = ref.fuse(kf, mp, pm.CAM)
        assert w["n_fused"] * 4 >= 700 and w["n_fused"] < 700
        strm = st.fuse_points(tk, pm.CAM, kf["Tcw"], maps=mp, skip=kf["skip"])
        host = run(hvo, kf, mp)
        identical(strm, host, "stream")
        same(strm, w, "stream")
        identical(strm, st.fuse_points(tk, pm.CAM, kf["Tcw"], maps=mp, skip=kf["skip"]), "stream twice")
        m.set_many(0, mp["pos"], mp["normal"], mp["max_dist"], mp["min_dist"], mp["desc"])
        identical(st.fuse_points(tk, pm.CAM, kf["Tcw"], point_map=m, slots=np.arange(700), skip=kf["skip"]), host, "stream, slots")
        rc, msg, out = st.fuse_points(tk, pm.CAM, kf["Tcw"], maps=mp, skip=kf["skip"], th_low=256, check=False)
        assert rc == -1 and "th_low" in msg
        untouched(hvo, [out])
        rc, msg, out = st.fuse_points(tk, pm.CAM, kf["Tcw"], point_map=m, slots=[0, 700], check=False)
        assert rc == -1 and "slot 700" in msg
        untouched(hvo, [out])
    finally:
        m.close(); st.close()


def test_stream_without_the_orb_stage_is_refused_with_a_message(hvo, synth):
    g, d = synth.make_frame("std", 0x5EED0152)
    kf, mp, _ = big(hvo)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD, bf=0.0)
    try:
        t = st.submit(g); st.collect(t)
        with pytest.raises(hvo.HvoError, match="HVO_STAGE_ORB") as e:
            st.fuse_points(t, pm.CAM, kf["Tcw"], maps=mp)
        assert e.value.status == -1
    finally:
        st.close()


def test_example_runs(hvo, synth, tmp_path):
    """examples/fuse_neighbors.cpp linked against the library and run on a synthetic frame: both halves of SearchInNeighbors with the caller's
    walk.  The neighbours see the current key frame's points 3 and 6 cm aside with six descriptor bits flipped, so most of its map points fuse
    into each neighbour (replacing where the neighbour holds a point, adding where it does not), and the second call finds the current key
    frame's own features for the neighbours' surviving points"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "fuse_neighbors")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fuse_neighbors.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d = synth.make_frame("std", 0x5EED0153)
    g.tofile(tmp_path / "g.u8"); d.tofile(tmp_path / "d.u16")
    out = subprocess.check_output([exe, str(tmp_path / "g.u8"), str(tmp_path / "d.u16")]).decode()
    print(out)
    first = re.findall(r"first loop, neighbour (\d): (\d+) searched, (\d+) fused: (\d+) replaced, (\d+) added, (\d+) skipped", out)
    second = re.search(r"second call: (\d+) candidates, (\d+) searched, (\d+) fused: (\d+) replaced, (\d+) added, (\d+) skipped", out)
    cur = re.search(r"current key frame: (\d+) features, (\d+) map points", out)
    assert len(first) == 2 and second and cur, out
    npts = int(cur.group(2))
    assert npts > 50
    for _, searched, fused, replaced, added, skipped in first:
        assert int(fused) * 2 >= npts and int(replaced) > 0 and int(added) > 0 and int(fused) == int(replaced) + int(added) + int(skipped), out
    assert int(second.group(3)) > 0 and int(second.group(3)) == int(second.group(4)) + int(second.group(5)) + int(second.group(6)), out
