"""Tracking::SearchLocalPoints on the GPU against a resident point map (csrc/local_points.hip), host-array, stream and batch forms, compared
with tests/point_map_ref.py.  Everything is reproducible float / double arithmetic, so every comparison is exact: integers with array_equal,
floats bit-equal through .view(np.uint32), a NaN by its bits like any other value (the NaN projections of the z == 0 rows are 0xFFC00000
on the device and in the restatement).  The one number that goes through a library log, the predicted level, is compared exactly too: the scene generators draw no point within 1e-4 of a level boundary (tests/test_point_map.py checks them)."""
import ctypes as C

import numpy as np
import pytest

import point_map_ref as ref

pytestmark = pytest.mark.gpu
CAM, B4, LOG_SF, NL, SF = ref.CAM, ref.BOUNDS, ref.LOG_SF, ref.N_LEVELS, ref.SF
KW = dict(log_scale_factor=LOG_SF, n_levels=NL)
_cache = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame(hvo, synth):
    """one synthetic frame's points (shared, never modified): key points, descriptors, mvuRight, mvDepth, the depth image"""
    if "f" not in _cache:
        g, d, _ = synth.make_sequence("std", 0x5EED7400, 1)
        ctx = hvo.Context()
        kp, desc = ctx.extract_orb(g[0]); ctx.close()
        ur, z = ref.stereo_from_depth(kp, kp, d[0], CAM[4])
        assert len(kp) >= 1000 and (z > 0).sum() > 900
        _cache["f"] = (kp, desc, ur, z)
    return _cache["f"]


def subset(fr, n):
    kp, desc, ur, z = fr
    s = slice(None, None, len(kp) // n) if n else slice(0, 0)
    return kp[s][:n].copy(), desc[s][:n].copy(), ur[s][:n].copy(), z[s][:n].copy()


def upload(hvo, M, slots=0):
    pm = hvo.PointMap(slots=slots)
    if len(M["pos"]):
        pm.set_many(0, M["pos"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
    return pm


def same(r, o, what=""):
    assert (r.n_slots_tested, r.n_in_view, r.n_matches, r.status) == (o["n_slots_tested"], o["n_in_view"], o["n_matches"], 0), (what, r.to_dict(), o)
    assert np.array_equal(r.in_view_slot, o["in_view_slot"]) and np.all(np.diff(r.in_view_slot) > 0), what
    assert np.array_equal(bits(r.proj), bits(o["proj"])), (what, r.proj[:4], o["proj"][:4])
    assert np.array_equal(bits(r.view_cos), bits(o["view_cos"])), what
    assert np.array_equal(r.level, o["level"]), (what, np.nonzero(r.level != o["level"])[0][:5])
    assert np.array_equal(r.match_idx, o["match_idx"]), (what, np.nonzero(r.match_idx != o["match_idx"])[0][:5])
    assert np.array_equal(r.match_dist, o["match_dist"]), what
    assert np.array_equal(r.held, o["held"]), what


def run_both(ctx, pm, M, sub, T, held=None, seen_extra=(), th=1.0, cam=CAM, limit=0.5):
    kp, desc, ur, _ = sub
    held = np.full(len(kp), -1, np.int32) if held is None else held
    r = ctx.search_local_points(pm, cam, T, kp, ur, desc, B4, held=held, seen_extra=seen_extra, th=th, view_cos_limit=limit, **KW)
    o = ref.search_local_points(M, cam, T, B4, LOG_SF, NL, SF, th, kp, ur, desc, held, seen_extra, limit=np.float32(limit))
    return r, o


@pytest.mark.parametrize("n,pattern", [(0, "none"), (1, "all"), (1, "none"), (63, "alt"), (64, "all"), (64, "last"), (65, "last"), (65, "wave"),
                                       (1000, "alt"), (1000, "wave"), (1000, "none"), (1000, "all"), (4097, "wave"), (4097, "last"), (4097, "alt")])
def test_compaction_order_and_frustum(hvo, synth, gpu_ctx, n, pattern):
    fr = frame(hvo, synth); T = ref.scene_pose()
    M, _ = ref.make_map(n, pattern, T, seed=n + len(pattern))
    pm = upload(hvo, M)
    try:
        sub = subset(fr, 64 if n <= 1000 else 1)
        assert len(sub[0]) == (64 if n <= 1000 else 1)
        r, o = run_both(gpu_ctx, pm, M, sub, T)
        same(r, o, what=(n, pattern))
        assert np.array_equal(r.in_view_slot, np.nonzero(ref.wanted_in_view(n, pattern))[0])
        assert r.n_slots_tested == n and pm.counts()[0] == n
    finally:
        pm.close()


def test_every_gate_alone_on_crafted_slots(hvo, synth, gpu_ctx):
    poses, rows = ref.crafted_gates()
    M = ref.crafted_map(rows)
    nr = len(rows)
    # three more copies of "u on max": a bad one, one seen through held, one seen through seen_extra
    for k in M: M[k] = np.concatenate([M[k], np.repeat(M[k][:1], 3, axis=0)])
    M["bad"][nr] = 1
    pm = upload(hvo, M)
    try:
        sub = subset(frame(hvo, synth), 8)
        held = np.full(8, -1, np.int32); held[3] = nr + 1
        for key, T in poses.items():
            r, o = run_both(gpu_ctx, pm, M, sub, T, held=held, seen_extra=[nr + 2], cam=ref.CAM2)
            same(r, o, what=key)
            assert r.n_slots_tested == nr                                # all but the bad one and the two seen ones
            for j, row in enumerate(rows):
                if row[1] == key:
                    assert (j in r.in_view_slot) == (row[6] == 0), (key, row[0])
            assert not set(range(nr, nr + 3)) & set(r.in_view_slot.tolist())
            if key in ("B", "C"):                                         # the NaN projection is in view and is reported as NaN
                j = [i for i, row in enumerate(rows) if row[1] == key and row[6] == 0][0]
                q = list(r.in_view_slot).index(j)
                assert np.isnan(r.proj[q]).all() and r.match_idx[q] == -1
        # without the seen marks the three copies behave like the original, except the bad one
        r, o = run_both(gpu_ctx, pm, M, sub, poses["A"], cam=ref.CAM2)
        same(r, o, what="unseen")
        assert nr not in r.in_view_slot and nr + 1 in r.in_view_slot and nr + 2 in r.in_view_slot
    finally:
        pm.close()


def own_map(fr_sub, T, n_extra=0, seed=3):
    """a map of the frame's own points with depth (all observed), followed by n_extra generated slots -> (M, feature of every own slot)"""
    kp, desc, ur, z = fr_sub
    good = np.nonzero(z > 0)[0]
    M = ref.empty_map(len(good), seed); M["observed"][:] = 1
    feats = ref.add_frame_points(M, kp, desc, z, T, range(len(good)))
    if n_extra:
        X, _ = ref.make_map(n_extra, "alt", T, seed=seed + 1)
        for k in M: M[k] = np.concatenate([M[k], X[k]])
    return M, feats


@pytest.mark.parametrize("nf", [200, 1000])
def test_search_of_the_frames_own_points(hvo, synth, gpu_ctx, nf):
    """the map holds the frame's own points seen from the true pose; the search runs under an estimate a centimetre off, so th = 1 misses
    some.  Equal to the restatement, and to hvo_search_by_projection_tracked fed the restatement's in-view arrays"""
    sub = subset(frame(hvo, synth), nf)
    assert len(sub[0]) == nf
    T = ref.scene_pose(); Ts = ref.estimated_pose(T)
    M, feats = own_map(sub, T, n_extra=50)
    pm = upload(hvo, M)
    try:
        kp, desc, ur, _ = sub
        seen = {}
        for th in (1.0, 3.0, 5.0):
            r, o = run_both(gpu_ctx, pm, M, sub, Ts, th=th)
            same(r, o, what=(nf, th))
            seen[th] = o["n_matches"]
            fp = ref.frustum_pass(M, CAM, Ts, B4, LOG_SF, NL, np.full(nf, -1, np.int32)); q = ref.queries(M, fp)
            nm, mi, md = gpu_ctx.search_by_projection_tracked(q[0], q[1], q[2], q[3], q[4], q[5], q[6], th, kp, ur, fp["t_occupied"], desc,
                                                              (B4[0], B4[2], B4[1], B4[3]))
            assert nm == r.n_matches and np.array_equal(mi, r.match_idx) and np.array_equal(md, r.match_dist), th
        n_own = len(feats)
        assert n_own / 2 <= seen[1.0] < n_own and seen[3.0] > seen[1.0]
    finally:
        pm.close()


def test_ownership(hvo, synth, gpu_ctx):
    sub = subset(frame(hvo, synth), 200)
    kp, desc, ur, z = sub
    T = ref.scene_pose()
    good = np.nonzero(z > 0)[0]
    f = [int(v) for v in good[10:90:8]]                                   # ten features, apart from each other
    # slots: 0 bad (held by f0) | 1 observed, held by f1; 2 = f1's own point | 3 unobserved, held by f2; 4 = f2's own point | 5 = f3's own point
    # (f3 holds -2) | 6 = f4's own point (f4 holds -3) | 7, 8 observed, both f5's point | 9, 10 unobserved, both f6's point | 11 = f7's own point
    M = ref.empty_map(12, seed=7)
    ref.add_frame_points(M, kp, desc, z, T, range(12), feats=[f[7], f[8], f[1], f[9], f[2], f[3], f[4], f[5], f[5], f[6], f[6], f[7]])
    M["observed"][:] = [1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 1]; M["bad"][0] = 1
    held = np.full(len(kp), -1, np.int32)
    held[f[0]], held[f[1]], held[f[2]], held[f[3]], held[f[4]] = 0, 1, 3, ref.FOREIGN_OBSERVED, ref.FOREIGN_UNOBSERVED
    pm = upload(hvo, M)
    try:
        r, o = run_both(gpu_ctx, pm, M, sub, T, held=held, th=3.0)
        same(r, o, what="ownership")
        h = r.held; q = {int(s): i for i, s in enumerate(r.in_view_slot)}
        assert h[f[0]] == -1                                              # the held bad slot is cleared
        assert 0 not in q and 1 not in q and 3 not in q                   # bad; seen; seen
        assert h[f[1]] == 1 and r.match_idx[q[2]] != f[1]                 # a held observed slot blocks its feature
        assert h[f[2]] == 4 and r.match_idx[q[4]] == f[2]                 # a held unobserved slot is overwritten
        assert h[f[3]] == ref.FOREIGN_OBSERVED and r.match_idx[q[5]] != f[3]      # -2 blocks and passes through
        assert h[f[4]] == 6 and r.match_idx[q[6]] == f[4]                 # -3 is overwritten
        assert r.match_idx[q[7]] == f[5] and r.match_idx[q[8]] != f[5] and h[f[5]] == 7       # two observed points, one descriptor: the first takes it
        assert r.match_idx[q[9]] == f[6] and r.match_idx[q[10]] == f[6] and h[f[6]] == 10     # two unobserved points: the later one keeps it
        # set_bad / set_observed are visible in the next call
        pm.set_bad(7, True); M["bad"][7] = 1
        pm.set_observed(4, False); M["observed"][4] = 0
        r2, o2 = run_both(gpu_ctx, pm, M, sub, T, held=held, th=3.0)
        same(r2, o2, what="after flags")
        assert 7 not in r2.in_view_slot and r2.held[f[5]] == 8
    finally:
        pm.close()


def test_pool_of_eight_descriptors_on_256_points(hvo, synth, gpu_ctx):
    """descriptors from a pool of eight (two of them one bit apart) on both sides: many equal distances, several map points want one feature,
    observed and unobserved claimants"""
    kp, desc, ur, z = subset(frame(hvo, synth), 200)
    T = ref.scene_pose()
    pool = np.random.RandomState(9).randint(0, 256, (8, 32)).astype(np.uint8); pool[1] = pool[0]; pool[1, 0] ^= 1
    desc = pool[(np.arange(len(kp)) * 3) % 8].copy()
    M = ref.empty_map(256, seed=8)
    ref.add_frame_points(M, kp, desc, z, T, range(0, 256, 2), pool=pool)
    ref.add_frame_points(M, kp, desc, z, T, range(1, 256, 2), pool=pool[::-1])         # every feature is wanted by two map points
    M["observed"] = (np.arange(256) % 3 != 0).astype(np.uint8)
    pm = upload(hvo, M)
    try:
        for th in (1.0, 5.0):
            r, o = run_both(gpu_ctx, pm, M, (kp, desc, ur, z), T, th=th)
            same(r, o, what=("pool", th))
        mi = o["match_idx"][o["match_idx"] >= 0]
        assert o["n_matches"] > 40 and len(np.unique(mi)) < len(mi)       # a feature was claimed twice (the later claim stands)
        assert len(np.unique(o["match_dist"][o["match_idx"] >= 0])) <= 4 and (np.bincount(o["match_dist"][o["match_idx"] >= 0]).max() > 10)
    finally:
        pm.close()


def _raw_call(hvo, ctx, pm, sub, T, held, n_slots):
    kp, desc, ur, _ = sub
    io, a = hvo._lp_io(len(kp), n_slots, held, None)
    res = hvo.LocalPointsResult()
    keep = [np.ascontiguousarray(kp), np.ascontiguousarray(ur, np.float32), np.ascontiguousarray(desc, np.uint8)]
    F = hvo.LocalPointsFrame(); F.kp_un, F.uright, F.desc = (v.ctypes.data for v in keep); F.n = len(kp)
    Tc = np.ascontiguousarray(T, np.float32).reshape(12); c = hvo._pose_cam(CAM); p = hvo._lp_params(B4, LOG_SF, NL, CAM[4], 1.0, 100, 0.8, 0.5)
    rc = hvo.lib().hvo_search_local_points(ctx.h, pm.h, C.byref(c), hvo._p(Tc), C.byref(p), C.byref(F), C.byref(io), C.byref(res))
    return rc, res, a


def test_limits(hvo, synth, gpu_ctx):
    fr = frame(hvo, synth); T = ref.scene_pose()
    sub = subset(fr, 8)
    M1, feats = own_map(sub, T)
    one = {k: v[:1] for k, v in M1.items()}                               # feature feats[0]'s own point, observed
    others = [i for i in range(8) if i != feats[0]]
    held = np.full(8, -1, np.int32); held[others[0]] = 3; held[others[1]] = 5          # two features hold slots 3 and 5
    n = 16387                                                             # two of them are held, hence seen: 16385 in view
    M = {k: np.repeat(v, n, axis=0) for k, v in one.items()}
    pm = upload(hvo, M)
    try:
        with pytest.raises(hvo.HvoError, match="16384"):
            gpu_ctx.search_local_points(pm, CAM, T, sub[0], sub[2], sub[1], B4, held=held, **KW)
        rc, res, a = _raw_call(hvo, gpu_ctx, pm, sub, T, held, n)
        assert rc == -4 and res.status == -4 and res.n_in_view == n - 2 and np.array_equal(a["held"], held)
        assert np.all(a["in_view_slot"] == 0) and np.all(a["match_idx"] == -1)        # no output was written
        # exactly 16384 in view runs: the first query takes the feature (it is observed), the others find it occupied
        pm.set_bad(n - 1, True)
        r = gpu_ctx.search_local_points(pm, CAM, T, sub[0], sub[2], sub[1], B4, held=held, th=3.0, **KW)
        assert (r.n_in_view, r.n_slots_tested, r.status) == (16384, 16384, 0)
        assert np.array_equal(r.in_view_slot, np.setdiff1d(np.arange(n - 1), [3, 5]))
        assert r.match_idx[0] == feats[0] and r.held[feats[0]] == 0 and r.n_matches == 1 + int((r.match_idx[1:] >= 0).sum())
        assert not np.any(r.match_idx[1:] == feats[0])
        assert len(np.unique(bits(r.proj), axis=0)) == 1 and len(np.unique(r.level)) == 1
        # a slot index of HVO_POINT_MAP_MAX_SLOTS is refused
        with pytest.raises(hvo.HvoError) as e:
            pm.set(hvo.POINT_MAP_MAX_SLOTS, one["pos"][0], one["normal"][0], 1.0, 1.0, one["desc"][0])
        assert e.value.status == -4 and pm.counts()[0] == n
    finally:
        pm.close()


def test_map_life_cycle(hvo, synth, gpu_ctx):
    fr = frame(hvo, synth); T = ref.scene_pose(); sub = subset(fr, 64)
    pm = hvo.PointMap(slots=0)                                            # created with 0 slots
    try:
        assert pm.counts() == (0, 0, 0)
        r = gpu_ctx.search_local_points(pm, CAM, T, sub[0], sub[2], sub[1], B4, **KW)
        assert (r.n_in_view, r.n_slots_tested, r.n_matches) == (0, 0, 0) and np.all(r.held == -1)
        M, _ = ref.make_map(100, "alt", T, seed=31)
        pm.set_many(0, M["pos"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
        pm.set(103, M["pos"][2], M["normal"][2], M["max_dist"][2], M["min_dist"][2], M["desc"][2], observed=False)      # past the end
        assert pm.counts()[0] == 104 and pm.slot(100)["bad"] and pm.slot(102)["bad"] and not pm.slot(103)["bad"] and not pm.slot(103)["observed"]
        s = pm.slot(103)
        assert s["pos"].tobytes() == M["pos"][2].tobytes() and s["normal"].tobytes() == M["normal"][2].tobytes() and s["desc"].tobytes() == M["desc"][2].tobytes()
        assert np.float32(s["max_dist"]).tobytes() == M["max_dist"][2].tobytes() and np.float32(s["min_dist"]).tobytes() == M["min_dist"][2].tobytes()
        M104 = {k: np.concatenate([v, np.repeat(v[2:3], 4, axis=0)]) for k, v in M.items()}
        M104["bad"][100:103] = 1; M104["observed"][103] = 0
        r, o = run_both(gpu_ctx, pm, M104, sub, T)
        same(r, o, what="extended")
        assert 103 in r.in_view_slot and 2 in r.in_view_slot
        # set_many of 5000 over a map of 104: the storage regrows, every slot is replaced
        B, _ = ref.make_map(5000, "wave", T, seed=32)
        pm.set_many(0, B["pos"], B["normal"], B["max_dist"], B["min_dist"], B["desc"], B["observed"], B["bad"])
        assert pm.counts() == (5000, 5000, int(B["observed"].sum()))
        r, o = run_both(gpu_ctx, pm, B, sub, T)
        same(r, o, what="regrown")
        # a shorter local map: 300 slots rewritten, the tail marked bad in the same call
        S, _ = ref.make_map(300, "alt", T, seed=33)
        N = {k: np.concatenate([S[k], B[k][300:]]) for k in B}; N["bad"][300:] = 1
        pm.set_many(0, N["pos"], N["normal"], N["max_dist"], N["min_dist"], N["desc"], N["observed"], N["bad"])
        assert pm.counts()[:2] == (5000, 300)
        r, o = run_both(gpu_ctx, pm, N, sub, T)
        same(r, o, what="shorter")
        assert r.n_slots_tested == 300 and r.in_view_slot.max() < 300
        pm.set_bad(0, True); N["bad"][0] = 1; pm.set_bad(4000, False); N["bad"][4000] = 0; pm.set_observed(2, not N["observed"][2]); N["observed"][2] ^= 1
        r, o = run_both(gpu_ctx, pm, N, sub, T)
        same(r, o, what="flags")
        assert 0 not in r.in_view_slot and r.n_slots_tested == 300 and pm.counts()[1] == 300
    finally:
        pm.close()


def test_regrowth_carries_live_slots_through_the_regrid(hvo, synth, gpu_ctx):
    """60 slots in a map of capacity 64, then slot 70: the storage regrows to 128 with live slots in it, whose components move to the new
    stride of the mirror and go up again whole; 60 .. 69 are skipped and stay bad.  Then 130 slots: 256, every slot replaced"""
    T = ref.scene_pose(); sub = subset(frame(hvo, synth), 8)
    assert len(sub[0]) == 8
    M, _ = ref.make_map(60, "alt", T, seed=41)
    M["bad"][::7] = 1
    assert 0 < M["observed"].sum() < 60 and not M["bad"][2]
    pm = hvo.PointMap(slots=0)                                            # capacity 64
    try:
        pm.set_many(0, M["pos"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
        pm.set(70, M["pos"][2], M["normal"][2], M["max_dist"][2], M["min_dist"][2], M["desc"][2])
        assert pm.counts() == (71, int((M["bad"] == 0).sum()) + 1, int(M["observed"].sum()) + 1)
        M71 = {k: np.concatenate([v, np.zeros((10,) + v.shape[1:], v.dtype), v[2:3]]) for k, v in M.items()}
        M71["bad"][60:70] = 1; M71["observed"][70] = 1
        for j in (0, 59, 70):
            s = pm.slot(j)
            assert s["pos"].tobytes() == M71["pos"][j].tobytes() and s["normal"].tobytes() == M71["normal"][j].tobytes(), j
            assert np.float32(s["max_dist"]).tobytes() == M71["max_dist"][j].tobytes() and np.float32(s["min_dist"]).tobytes() == M71["min_dist"][j].tobytes(), j
            assert s["desc"].tobytes() == M71["desc"][j].tobytes() and (s["bad"], s["observed"]) == (bool(M71["bad"][j]), bool(M71["observed"][j])), j
        assert pm.slot(60)["bad"] and pm.slot(69)["bad"]
        r, o = run_both(gpu_ctx, pm, M71, sub, T)
        same(r, o, what="regrown to 128")
        assert 2 in r.in_view_slot and 70 in r.in_view_slot and r.in_view_slot.max() == 70
        B, _ = ref.make_map(130, "alt", T, seed=42)
        pm.set_many(0, B["pos"], B["normal"], B["max_dist"], B["min_dist"], B["desc"], B["observed"], B["bad"])
        assert pm.counts() == (130, 130, int(B["observed"].sum()))
        r, o = run_both(gpu_ctx, pm, B, sub, T)
        same(r, o, what="regrown to 256")
        assert r.n_in_view == 65
    finally:
        pm.close()


def test_resident_forms_and_determinism(hvo, synth):
    """a 640 x 480 frame through a Stream equals the host-array form on its collected outputs; frame k of a batch of 3 under 3 poses equals the
    stream form bit for bit; the same call twice gives the same bytes"""
    g, d, _ = synth.make_sequence("std", 0x5EED7500, 3)
    T = [ref.estimated_pose(ref.scene_pose(k), 0.005 * k) for k in range(3)]
    st = hvo.Stream(depth=4, stages=hvo.STAGE_ORB, bf=CAM[4]); ctx = hvo.Context(max_batch=4)
    pm = None
    keys = ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist")
    try:
        assert tuple(float(v) for v in st.bounds) == B4
        t = [st.submit(g[k], d[k]) for k in range(3)]
        rs = [st.collect(x) for x in t]
        M, feats = own_map((rs[0]["kp_un"], rs[0]["desc"], rs[0]["uright"], rs[0]["zdepth"]), ref.scene_pose(0), n_extra=200)
        M["observed"][::4] = 0
        pm = upload(hvo, M)
        out = []
        for k in range(3):
            kp, desc, ur = rs[k]["kp_un"], rs[k]["desc"], rs[k]["uright"]
            held = np.full(len(kp), -1, np.int32); held[2] = 8; held[5] = ref.FOREIGN_OBSERVED
            a = st.search_local_points(pm, t[k], CAM, T[k], len(kp), held=held, seen_extra=[0, 10], th=3.0, **KW)
            h = ctx.search_local_points(pm, CAM, T[k], kp, ur, desc, B4, held=held, seen_extra=[0, 10], th=3.0, **KW)
            a2 = st.search_local_points(pm, t[k], CAM, T[k], len(kp), held=held, seen_extra=[0, 10], th=3.0, **KW)
            for key in keys:
                assert getattr(a, key).tobytes() == getattr(h, key).tobytes(), (k, key)
                assert getattr(a, key).tobytes() == getattr(a2, key).tobytes(), (k, key)
            assert (a.n_in_view, a.n_matches, a.n_slots_tested) == (h.n_in_view, h.n_matches, h.n_slots_tested) == (a2.n_in_view, a2.n_matches, a2.n_slots_tested)
            if k == 0:
                same(a, ref.search_local_points(M, CAM, T[0], B4, LOG_SF, NL, SF, 3.0, kp, ur, desc, held, [0, 10]), what="stream")
                assert a.n_matches > len(feats) / 2
            out.append((a, held))
        ctx.batch_upload(g, d); ctx.batch_run(hvo.STAGE_ORB)
        bs = ctx.batch_search_local_points(pm, CAM, T, [len(r["kp"]) for r in rs], held=[o[1] for o in out], seen_extra=[[0, 10]] * 3, th=3.0, **KW)
        for k in range(3):
            for key in keys:
                assert getattr(bs[k], key).tobytes() == getattr(out[k][0], key).tobytes(), (k, key)
            assert (bs[k].n_in_view, bs[k].n_matches, bs[k].n_slots_tested) == (out[k][0].n_in_view, out[k][0].n_matches, out[k][0].n_slots_tested)
        assert len({b.n_matches for b in bs}) > 1 or len({b.in_view_slot.tobytes() for b in bs}) > 1       # the three poses differ in effect
    finally:
        if pm: pm.close()
        ctx.close(); st.close()


def test_stream_without_the_orb_stage_is_refused_with_a_message(hvo, synth):
    g, d, _ = synth.make_sequence("std", 0x5EED7600, 1)
    pm = hvo.PointMap()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD, bf=CAM[4])
    try:
        t = st.submit(g[0], d[0]); st.collect(t)
        with pytest.raises(hvo.HvoError, match="HVO_STAGE_ORB") as e:
            st.search_local_points(pm, t, CAM, ref.scene_pose(), 0, **KW)
        assert e.value.status == -1
    finally:
        st.close(); pm.close()
