"""Tracking::SearchLocalLines + Manhattan::computeStructConstInMap on the GPU against a resident line map (csrc/local_lines.hip), host-array,
stream and batch forms, compared with tests/line_map_ref.py.  Everything is reproducible float / double arithmetic, so every comparison is
exact: integers with array_equal, floats bit-equal through .view(np.uint32) -- a tolerance would hide a contracted multiply-add
(tests/test_plane_assoc_gpu.py argues the same).  The one number that goes through a library log, the predicted level, is compared exactly
too: the scene generator draws no line within 1e-4 of a level boundary (tests/test_line_map.py checks the generator)."""
import numpy as np
import pytest

import line_map_ref as ref
import local_map_lines_ref as core

pytestmark = pytest.mark.gpu
CAM, B4, LOG_SF = ref.CAM, ref.BOUNDS, ref.LOG_SF
_cache = {}


def frame(hvo, synth):
    """one synthetic frame's lines (shared, never modified): key lines, descriptors, line functions, 3-D lines, line grid"""
    if "f" not in _cache:
        g, d, _ = synth.make_sequence("std", 0x5EED7100, 1)
        ctx = hvo.Context(lsd_nfeatures=200)
        kl, ld, fn = ctx.extract_lsd(g[0]); l3 = ctx.lines_3d(kl, d[0], seed=3)
        assert len(kl) >= 200 and (l3["good"] == 1).sum() >= 60       # the 200-line shapes below are 200 lines
        _cache["f"] = (g, d, kl, ld, fn, l3); ctx.close()
    return _cache["f"]


def subset(ctx, fr, n):
    _, _, kl, ld, fn, l3 = fr
    kl, ld, fn, l3 = kl[:n], ld[:n], fn[:n], l3[:n]
    cs, ci = ctx.assign_lines_to_grid(kl, np.array([B4[0], B4[1], B4[2], B4[3]], np.float32)) if n else (np.zeros(64 * 48 + 1, np.int32), np.zeros(0, np.int32))
    return kl, ld, fn, l3, cs, ci


def add_frame_lines(M, kl, ld, l3d, Tcw, slots, pool=None, tilt_every=0):
    """overwrite `slots` of the map with the frame's own good 3-D lines seen from Tcw, so that the search has something to find.  tilt_every:
    every such line's world vector is turned 10 degrees towards the normal of the plane through the camera centre and the line -- inside the
    search's 15 degree gate, and |CosSita| = sin 10 = 0.17 > 0.09, so the post-gate takes the match away again"""
    T = np.asarray(Tcw, np.float64).reshape(3, 4); R, t = T[:, :3], T[:, 3]
    good = np.nonzero(l3d["good"] == 1)[0]
    for k, j in enumerate(slots):
        i = good[k % len(good)]
        A, B = R.T @ (l3d["A"][i] - t), R.T @ (l3d["B"][i] - t)
        mid = 0.5 * (A + B); ow = -R.T @ t; d = np.linalg.norm(mid - ow)
        M["pos"][j] = np.concatenate([A, B]); M["wvec"][j] = A - B; M["normal"][j] = (mid - ow) / d
        if tilt_every and k % tilt_every == 0:
            u = (A - B) / np.linalg.norm(A - B); pl = np.cross(A - ow, B - ow); pl /= np.linalg.norm(pl)
            M["wvec"][j] = np.cos(np.radians(10)) * u + np.sin(np.radians(10)) * pl
        M["max_dist"][j] = np.float32(d * 2.03); M["min_dist"][j] = np.float32(d * 0.5)
        M["desc"][j] = ld[i] if pool is None else pool[k % len(pool)]


def upload(hvo, M):
    lm = hvo.LineMap(slots=0)
    if len(M["pos"]):
        lm.set_many(0, M["pos"], M["wvec"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
    return lm


def same(r, o, rel=True, what=""):
    assert (r.n_slots_tested, r.n_in_view, r.n_matches, r.n_gated, r.status) == (o["n_slots_tested"], o["n_in_view"], o["n_matches"], o["n_gated"], 0), (what, r.to_dict(), o)
    assert np.array_equal(r.in_view_slot, o["in_view_slot"]) and np.all(np.diff(r.in_view_slot) > 0), what
    assert np.array_equal(r.proj.view(np.uint32), o["proj"].view(np.uint32)) and np.array_equal(r.view_cos.view(np.uint32), o["view_cos"].view(np.uint32)), what
    assert np.array_equal(r.level, o["level"]), (what, np.nonzero(r.level != o["level"])[0][:5])
    assert np.array_equal(r.match_idx, o["match_idx"]) and np.array_equal(r.match_dist, o["match_dist"]), what
    assert np.array_equal(r.held, o["held"]), what
    assert np.array_equal(r.n_par, o["n_par"]) and np.array_equal(r.n_perp, o["n_perp"]), what
    if rel: assert np.array_equal(r.rel_map, o["rel_map"]), what


def run_both(hvo, ctx, lm, M, fr_sub, T, held, seen_extra=(), th=1.0, rel=True):
    kl, ld, fn, l3, cs, ci = fr_sub
    r = ctx.search_local_lines(lm, CAM, T, kl, fn, l3, ld, cs, ci, B4, held=held, seen_extra=seen_extra, log_scale_factor=LOG_SF, th=th, rel_map=rel)
    o = ref.search_local_lines(M, CAM, T, B4, LOG_SF, th, 0.95, kl, fn, l3, ld, cs, ci, held, seen_extra)
    return r, o


@pytest.mark.parametrize("n,pattern", [(0, "none"), (1, "all"), (1, "none"), (63, "alt"), (64, "all"), (64, "last"), (65, "last"), (65, "wave"),
                                       (1000, "alt"), (1000, "wave"), (1000, "none"), (4097, "all"), (4097, "wave"), (4097, "last")])
def test_compaction_order_and_frustum(hvo, synth, gpu_ctx, n, pattern):
    fr = frame(hvo, synth); T = ref.scene_pose()
    M, _ = ref.make_map(n, pattern, T, seed=n + len(pattern))
    lm = upload(hvo, M)
    try:
        sub = subset(gpu_ctx, fr, 64 if n <= 1000 else 1)
        r, o = run_both(hvo, gpu_ctx, lm, M, sub, T, np.full(len(sub[0]), -1, np.int32))
        same(r, o, what=(n, pattern))
        assert np.array_equal(r.in_view_slot, np.nonzero(ref.wanted_in_view(n, pattern))[0])
        assert lm.counts()[0] == n
    finally:
        lm.close()


@pytest.mark.parametrize("nl", [0, 1, 64, 65, 200])
def test_frame_line_counts_skips_and_matches(hvo, synth, gpu_ctx, nl):
    """map lines made from the frame's own 3-D lines among generated ones; bad and seen_extra slots interleaved; held slots (one of them bad)"""
    fr = frame(hvo, synth); T = ref.scene_pose()
    n = 300
    M, _ = ref.make_map(n, "alt", T, seed=5)
    sub = subset(gpu_ctx, fr, nl)
    assert len(sub[0]) == nl
    add_frame_lines(M, sub[0] if nl else fr[2], sub[1] if nl else fr[3], sub[3] if nl else fr[5], T, range(1, n, 2), tilt_every=3)
    M["bad"][::7] = 1
    if nl > 3:                                                            # slot 2's world vector = the normal of frame line 3's interpretation plane:
        k3 = sub[0][3]; Ki = ref.k_inv(CAM).astype(np.float64)            # CosSita = 1, so the line that holds it before the call loses it
        N = np.cross(Ki @ [k3["sx"], k3["sy"], 1.0], Ki @ [k3["ex"], k3["ey"], 1.0])
        M["wvec"][2] = np.asarray(T, np.float64)[:, :3].T @ N; M["observed"][2] = 1     # (observed: no match may claim line 3 over it)
    lm = upload(hvo, M)
    try:
        held = np.full(nl, -1, np.int32)
        if nl > 3: held[0], held[1], held[3] = 14, 9, 2                 # slot 14 is bad; 9 and 2 are not
        extra = np.arange(3, n, 11)
        for th in (1.0, 5.0):
            r, o = run_both(hvo, gpu_ctx, lm, M, sub, T, held, extra, th=th)
            same(r, o, what=(nl, th))
        if nl >= 64:
            assert o["n_matches"] > 5 and o["n_in_view"] > 100
            assert o["n_gated"] > 1 and (o["held"] >= 0).sum() > 3        # the post-gate fired and left some
            assert held[3] == 2 and o["held"][3] == -1                    # a line held before the call was removed too
        if nl > 3: assert o["held"][0] != 14
        r2, _ = run_both(hvo, gpu_ctx, lm, M, sub, T, held, extra, th=5.0, rel=False)      # without the optional matrix; and repeatability
        assert r2.rel_map is None
        same(r2, o, rel=False)
        assert r2.to_dict()["held"].tobytes() == r.held.tobytes() and r2.proj.tobytes() == r.proj.tobytes()
        # the merged search core, fed with the restatement's queries, gives the same matches
        if nl:
            fp = ref.frustum_pass(M, CAM, T, B4, LOG_SF, held, extra); q = ref.queries(M, fp)
            kl, ld, fn, l3, cs, ci = sub
            nm, mi, md = gpu_ctx.search_lines_by_projection_map(q[0], q[1], q[2], q[3], q[4], kl, fn, l3, ld, fp["t_occupied"], cs, ci, np.array(B4, np.float32), th=5.0)
            assert nm == r.n_matches and np.array_equal(mi, r.match_idx) and np.array_equal(md, r.match_dist)
    finally:
        lm.close()


def test_ties_updates_and_two_contexts(hvo, synth, gpu_ctx):
    """descriptors from a pool of four (two at distance 1) on both sides: several map lines want the same frame line, observed and unobserved
    claimants; then set_bad / set_observed / a replaced slot are seen by the next call, from a second context too"""
    fr = frame(hvo, synth); T = ref.scene_pose()
    n = 260
    M, _ = ref.make_map(n, "none", T, seed=8)
    pool = np.random.RandomState(9).randint(0, 256, (4, 32)).astype(np.uint8); pool[1] = pool[0]; pool[1, 0] ^= 1
    kl, ld, fn, l3, cs, ci = subset(gpu_ctx, fr, 200)
    ld = pool[(np.arange(len(kl)) * 3) % 4].copy()
    add_frame_lines(M, kl, ld, l3, T, range(0, n, 2), pool=pool)
    add_frame_lines(M, kl, ld, l3, T, range(1, n, 2), pool=pool[::-1])    # every frame line is wanted by two map lines
    M["observed"] = (np.arange(n) % 3 != 0).astype(np.uint8)
    sub = (kl, ld, fn, l3, cs, ci)
    lm = upload(hvo, M); ctx2 = hvo.Context()
    try:
        held = np.full(len(kl), -1, np.int32)
        r, o = run_both(hvo, gpu_ctx, lm, M, sub, T, held, th=5.0)
        same(r, o, what="ties")
        mi = o["match_idx"][o["match_idx"] >= 0]
        assert o["n_matches"] > 10 and len(np.unique(mi)) < len(mi)       # a frame line was claimed twice (the later claim stands)
        lm.set_bad(0, True); M["bad"][0] = 1
        lm.set_observed(2, not M["observed"][2]); M["observed"][2] ^= 1
        M["pos"][4] = M["pos"][6]; M["wvec"][4] = M["wvec"][6]; M["normal"][4] = M["normal"][6]; M["max_dist"][4] = M["max_dist"][6]; M["min_dist"][4] = M["min_dist"][6]
        lm.set(4, M["pos"][4], M["wvec"][4], M["normal"][4], M["max_dist"][4], M["min_dist"][4], M["desc"][4], observed=bool(M["observed"][4]))
        s = lm.slot(4)
        assert np.array_equal(s["pos"], M["pos"][4]) and s["max_dist"] == M["max_dist"][4] and not s["bad"]
        r, o2 = run_both(hvo, gpu_ctx, lm, M, sub, T, held, th=5.0)
        same(r, o2, what="after updates")
        assert 0 not in o2["in_view_slot"]
        r3, _ = run_both(hvo, ctx2, lm, M, sub, T, held, th=5.0)
        same(r3, o2, what="second context")
        lm.set(n + 2, M["pos"][1], M["wvec"][1], M["normal"][1], 1.0, 1.0, M["desc"][1])     # a slot past the end: the skipped ones start bad
        assert lm.counts()[:2] == (n + 3, int((M["bad"] == 0).sum()) + 1) and lm.slot(n)["bad"]
    finally:
        ctx2.close(); lm.close()


def test_query_limit_leaves_held_untouched(hvo, synth, gpu_ctx):
    fr = frame(hvo, synth); T = ref.scene_pose()
    one, _ = ref.make_map(1, "all", T, seed=2)
    n = 16387                                                             # two of them are held, hence seen: 16385 in view
    M = {k: np.repeat(v, n, axis=0) for k, v in one.items()}
    lm = upload(hvo, M)
    try:
        kl, ld, fn, l3, cs, ci = subset(gpu_ctx, fr, 8)
        held = np.array([-1, 3, -1, -1, 5, -1, -1, -1], np.int32)
        with pytest.raises(hvo.HvoError, match="16384"):
            gpu_ctx.search_local_lines(lm, CAM, T, kl, fn, l3, ld, cs, ci, B4, held=held)
        io, a = hvo._ll_io(8, n, held, None, False)
        res = hvo.LocalLinesResult()
        F = hvo.LocalLinesFrame(); keep = [np.ascontiguousarray(v) for v in (kl, fn, l3, ld, cs, ci)]
        for k, v in zip(("kl", "linefn", "l3d", "desc", "cell_start", "cell_items"), keep): setattr(F, k, v.ctypes.data)
        F.n_kl = 8
        import ctypes as C
        Tc = np.ascontiguousarray(T, np.float32).reshape(12); c = hvo._pose_cam(CAM); p = hvo._ll_params(B4, LOG_SF, 1.0, 0.95)
        rc = hvo.lib().hvo_search_local_lines(gpu_ctx.h, lm.h, C.byref(c), hvo._p(Tc), C.byref(p), C.byref(F), C.byref(io), C.byref(res))
        assert rc == -4 and res.n_in_view == n - 2 and np.array_equal(a["held"], held)
    finally:
        lm.close()


def test_regrowth_carries_live_slots_through_the_regrid(hvo, synth, gpu_ctx):
    """60 slots in a map of capacity 64, then slot 70: the storage regrows to 128 with live slots in it, whose components move to the new
    stride of the mirror and go up again whole; 60 .. 69 are skipped and stay bad.  Then 130 slots: 256, every slot replaced"""
    T = ref.scene_pose(); sub = subset(gpu_ctx, frame(hvo, synth), 8)
    assert len(sub[0]) == 8
    held = np.full(8, -1, np.int32)
    M, _ = ref.make_map(60, "alt", T, seed=41)
    M["bad"][::7] = 1
    assert 0 < M["observed"].sum() < 60 and not M["bad"][2]
    lm = hvo.LineMap(slots=0)                                             # capacity 64
    try:
        lm.set_many(0, M["pos"], M["wvec"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
        lm.set(70, M["pos"][2], M["wvec"][2], M["normal"][2], M["max_dist"][2], M["min_dist"][2], M["desc"][2])
        assert lm.counts() == (71, int((M["bad"] == 0).sum()) + 1, int(M["observed"].sum()) + 1)
        M71 = {k: np.concatenate([v, np.zeros((10,) + v.shape[1:], v.dtype), v[2:3]]) for k, v in M.items()}
        M71["bad"][60:70] = 1; M71["observed"][70] = 1
        for j in (0, 59, 70):
            s = lm.slot(j)
            assert all(s[k].tobytes() == M71[k][j].tobytes() for k in ("pos", "wvec", "normal", "desc")), j
            assert np.float32(s["max_dist"]).tobytes() == M71["max_dist"][j].tobytes() and np.float32(s["min_dist"]).tobytes() == M71["min_dist"][j].tobytes(), j
            assert (s["bad"], s["observed"]) == (bool(M71["bad"][j]), bool(M71["observed"][j])), j
        assert lm.slot(60)["bad"] and lm.slot(69)["bad"]
        r, o = run_both(hvo, gpu_ctx, lm, M71, sub, T, held)
        same(r, o, what="regrown to 128")
        assert 2 in r.in_view_slot and 70 in r.in_view_slot and r.in_view_slot.max() == 70
        B, _ = ref.make_map(130, "alt", T, seed=42)
        lm.set_many(0, B["pos"], B["wvec"], B["normal"], B["max_dist"], B["min_dist"], B["desc"], B["observed"], B["bad"])
        assert lm.counts() == (130, 130, int(B["observed"].sum()))
        r, o = run_both(hvo, gpu_ctx, lm, B, sub, T, held)
        same(r, o, what="regrown to 256")
        assert r.n_in_view == 65
    finally:
        lm.close()


def test_rel_map_200_by_1000(hvo, synth, gpu_ctx):
    fr = frame(hvo, synth); T = ref.scene_pose()
    R = np.asarray(T, np.float64)[:, :3]
    # world vectors around Rcw times the three axes, three face diagonals and six generic directions: against a frame line along an axis
    # 1 of 12 is parallel and 3 of 12 are perpendicular, about a third nonzero
    V = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, -1], [2, 1, 1], [1, 2, -1]], np.float64)
    M, _ = ref.make_map(1000, "all", T, seed=11, axes=(R @ (V / np.linalg.norm(V, axis=1)[:, None]).T).T)   # rotCW multiplies by Rcw
    kl, ld, fn, l3, cs, ci = subset(gpu_ctx, fr, 200)
    assert len(kl) == 200
    l3 = l3.copy()
    l3["line_eq"] = (np.eye(3)[np.arange(len(l3)) % 3] + np.random.RandomState(4).normal(0, 0.01, (len(l3), 3))).astype(np.float32)
    l3["line_eq"][7] = -1.0; l3["line_eq"][9] = 0.0
    lm = upload(hvo, M)
    try:
        sub = (kl, ld, fn, l3, cs, ci)
        r, o = run_both(hvo, gpu_ctx, lm, M, sub, T, np.full(len(kl), -1, np.int32))
        same(r, o, what="rel")
        assert r.rel_map.shape == (len(kl), 1000) and 0.2 < (o["rel_map"] != 0).mean() < 0.5 and (o["rel_map"] == 1).any() and (o["rel_map"] == 2).any()
    finally:
        lm.close()


STAGES = lambda hvo: hvo.STAGE_LSD | hvo.STAGE_ORB | hvo.STAGE_GRIDS | hvo.STAGE_LINES3D


def test_resident_forms(hvo, synth):
    """a 640 x 480 frame through a Stream equals the host-array form on its collected outputs; frame k of a batch of 3 equals the stream form"""
    g, d, _ = synth.make_sequence("std", 0x5EED7200, 3)
    T = [ref.scene_pose(k) for k in range(3)]
    st = hvo.Stream(depth=4, stages=STAGES(hvo), bf=0.0); ctx = hvo.Context(max_batch=4)
    lm = None
    try:
        b4 = tuple(float(v) for v in st.bounds)
        assert b4 == B4
        t = [st.submit(g[k], d[k]) for k in range(3)]
        rs = [st.collect(x) for x in t]
        M, _ = ref.make_map(400, "alt", T[0], seed=21)
        add_frame_lines(M, rs[0]["kl"], rs[0]["ldesc"], rs[0]["lines3d"], T[0], range(1, 400, 2))
        lm = upload(hvo, M)
        out = []
        for k in range(3):
            kl, ld, fn, l3 = rs[k]["kl"], rs[k]["ldesc"], rs[k]["linefn"], rs[k]["lines3d"]; cs, ci = rs[k]["ln_grid"]
            held = np.full(len(kl), -1, np.int32); held[2] = 8
            a = st.search_local_lines(lm, t[k], CAM, T[k], len(kl), held=held, seen_extra=[0, 10], log_scale_factor=LOG_SF, th=5.0, rel_map=True)
            h = ctx.search_local_lines(lm, CAM, T[k], kl, fn, l3, ld, cs, ci, b4, held=held, seen_extra=[0, 10], log_scale_factor=LOG_SF, th=5.0, rel_map=True)
            for key in ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist", "n_par", "n_perp", "rel_map"):
                assert getattr(a, key).tobytes() == getattr(h, key).tobytes(), (k, key)
            assert (a.n_in_view, a.n_matches, a.n_gated, a.n_slots_tested) == (h.n_in_view, h.n_matches, h.n_gated, h.n_slots_tested)
            if k == 0:
                same(a, ref.search_local_lines(M, CAM, T[0], b4, LOG_SF, 5.0, 0.95, kl, fn, l3, ld, cs, ci, held, [0, 10]), what="stream")
                assert a.n_matches > 5
            out.append((a, held))
        ctx.set_tail_params(seed=t[0] + 1)                            # the batch's 3-D line seeds run seed + f, the stream's ticket + 1
        ctx.batch_upload(g, d); ctx.batch_run(STAGES(hvo))                # (the grids stage needs ORB and LSD)
        bs = ctx.batch_search_local_lines(lm, CAM, T, [len(r["kl"]) for r in rs], held=[o[1] for o in out], seen_extra=[[0, 10]] * 3, log_scale_factor=LOG_SF,
                                          th=5.0, rel_map=True)
        for k in range(3):
            for key in ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist", "n_par", "n_perp", "rel_map"):
                assert getattr(bs[k], key).tobytes() == getattr(out[k][0], key).tobytes(), (k, key)
    finally:
        if lm: lm.close()
        ctx.close(); st.close()


def test_resident_refusals_carry_a_message(hvo, synth):
    g, d, _ = synth.make_sequence("std", 0x5EED7300, 1)
    lm = hvo.LineMap()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_ORB | hvo.STAGE_GRIDS, bf=0.0)
    st2 = hvo.Stream(depth=2, stages=STAGES(hvo), bf=0.0)
    try:
        t = st.submit(g[0], d[0]); st.collect(t)
        with pytest.raises(hvo.HvoError, match="LINES3D"):
            st.search_local_lines(lm, t, CAM, ref.scene_pose(), 0)
        t = st2.submit(g[0]); st2.collect(t)
        with pytest.raises(hvo.HvoError, match="without depth"):
            st2.search_local_lines(lm, t, CAM, ref.scene_pose(), 0)
    finally:
        st.close(); st2.close(); lm.close()
