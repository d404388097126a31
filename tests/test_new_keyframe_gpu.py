"""Context.create_keyframe_features / Stream.create_keyframe_features (csrc/new_keyframe.hip) on the device against tests/new_keyframe_ref.py.
Everything is reproducible float / double arithmetic in a stated order, so every comparison is exact: integers with array_equal, floats by
their bits, a NaN by being one (new_keyframe_ref.same_bits)."""
import numpy as np
import pytest

import line_map_ref as lmr
import new_keyframe_ref as kr
import point_map_ref as pmr

pytestmark = pytest.mark.gpu
F32 = np.float32
CAM = pmr.CAM
T0 = kr.scene_pose(0)
N_SLOTS = 40                                                     # the maps the held patterns point into: even slots observed, odd ones not
COUNTS = (0, 1, 63, 64, 65, 99, 100, 101, 102, 255, 256, 257)


@pytest.fixture(scope="module")
def kfi(hvo):
    k = hvo.KeyFrameInsert()
    yield k
    k.close()


def _maps(hvo, n=N_SLOTS, seed=3):
    """a point map and a line map of n slots with random contents, observed on the even slots -> (pmap, lmap, observed)"""
    rng = np.random.RandomState(seed)
    obs = (np.arange(n) % 2 == 0).astype(np.uint8)
    pmap = hvo.PointMap(slots=0); lmap = hvo.LineMap(slots=0)
    if n:
        pmap.set_many(0, rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)), rng.uniform(1, 2, n), rng.uniform(0, 1, n), rng.randint(0, 256, (n, 32)), obs)
        lmap.set_many(0, rng.uniform(-1, 1, (n, 6)), rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3)), rng.uniform(1, 2, n), rng.uniform(0, 1, n),
                      rng.randint(0, 256, (n, 32)), obs)
    return pmap, lmap, obs.astype(bool)


def _snapshot(m):
    n = m.counts()[0]
    return n, [m.slot(j) for j in range(n)]


def _same_slots(a, b):
    if a[0] != b[0]: return False
    for x, y in zip(a[1], b[1]):
        for k in x:
            if not (kr.same_bits(x[k], y[k]) if isinstance(x[k], np.ndarray) else x[k] == y[k]): return False
    return True


def _points(M, n_extra=7, seed=0):
    """M candidates among M + n_extra features (the rest without depth), shuffled"""
    kp, z, desc = kr.make_points(M + n_extra, 100 + M + seed, zero_rate=0.0)
    z = np.abs(z); z[z == 0] = 1.0
    rng = np.random.RandomState(M + seed)
    off = rng.permutation(M + n_extra)[:n_extra]
    z[off] = np.where(np.arange(n_extra) % 2 == 0, 0.0, -1.0)
    return kp, z.astype(F32), desc


def _lines(hvo, n, seed):
    kl, ldesc, A, B = kr.make_lines(n, seed, keyline_dt=hvo.KEYLINE_DT)
    l3 = np.zeros(n, hvo.LINE3D_DT); l3["A"] = A; l3["B"] = B
    return kl, ldesc, l3


def _th(z, where):
    zz = np.sort(z[z > 0])
    if where == "below" or len(zz) == 0: return 0.25
    return float(zz[len(zz) // 2]) if where == "inside" else 100.0


def _both(hvo, ctx, kfi, pmap, lmap, obs, mode, kp=None, z=None, desc=None, kl=None, ldesc=None, l3=None, **kw):
    want = kr.create(mode, CAM, T0, kp_un=kp, depth=z, desc=desc, keylines=kl, ldesc=ldesc, l3d_A=None if l3 is None else l3["A"],
                     l3d_B=None if l3 is None else l3["B"], pt_observed=obs, ln_observed=obs, **kw)
    got = ctx.create_keyframe_features(kfi, pmap, lmap, CAM, T0, kp, z, desc, kl, ldesc, l3, mode=mode, **kw)
    bad = kr.compare(got, want)
    assert not bad, (bad, mode, kw.get("th_depth"))
    assert (got.n_points_created, got.n_lines_created) == (want["n_points_created"], want["n_lines_created"])
    return got, want


@pytest.mark.parametrize("M", COUNTS)
def test_point_counts_thresholds_and_modes(hvo, gpu_ctx, kfi, M):
    """M candidates, thDepth below, inside and above their range, the three modes, returned values only"""
    pmap, lmap, obs = _maps(hvo)
    try:
        kp, z, desc = _points(M)
        held = kr.held_pattern(len(z), "mixed", N_SLOTS, np.random.RandomState(M))
        before = _snapshot(pmap)
        for where in ("below", "inside", "above"):
            for mode in (kr.KEYFRAME, kr.TEMPORAL, kr.INIT):
                got, _ = _both(hvo, gpu_ctx, kfi, pmap, None, obs, mode, kp, z, desc, th_depth=_th(z, where), held_points=held)
                assert got.n_point_candidates == M
        assert _same_slots(before, _snapshot(pmap))               # first = -1: the map is read, never written
    finally:
        pmap.close(); lmap.close()


@pytest.mark.parametrize("M", COUNTS + (2041,))
def test_line_counts_thresholds_and_geometry(hvo, gpu_ctx, kfi, M):
    """line candidates (2041 + 7 = 2048 key lines at the last), both line_geometry readings, the init gate"""
    pmap, lmap, obs = _maps(hvo)
    try:
        kl, ldesc, l3 = _lines(hvo, M + 7, 200 + M)
        l3["A"][:, 2] = np.where(l3["A"][:, 2] == 0, 1.5, l3["A"][:, 2]); l3["B"][:, 2] = np.where(l3["B"][:, 2] == 0, 1.25, l3["B"][:, 2])
        l3["A"][:7, 2] = 0; l3["A"][1:7:2, 0] = 0                   # seven non-candidates; three of them fail init's x gate too
        kl["octave"][M // 2] = 3                                   # outside line_n_levels = 1: refused per entry where the level is read
        held = kr.held_pattern(M + 7, "mixed", N_SLOTS, np.random.RandomState(M))
        z = np.array([kr.line_key(l3["A"][i], l3["B"][i]) for i in range(M + 7)], F32); z[:7] = 0
        for where in ("below", "inside", "above"):
            for geo in (1, 0):
                got, want = _both(hvo, gpu_ctx, kfi, None, lmap, obs, kr.KEYFRAME, kl=kl, ldesc=ldesc, l3=l3, th_depth=_th(z, where), held_lines=held, line_geometry=geo)
                assert got.n_line_candidates == M and got.ln_rel.shape == (len(want["ln_index"]), M + 7)
        _both(hvo, gpu_ctx, kfi, None, lmap, obs, kr.INIT, kl=kl, ldesc=ldesc, l3=l3)
    finally:
        pmap.close(); lmap.close()


def test_all_depths_equal_and_depth_on_the_threshold(hvo, gpu_ctx, kfi):
    pmap, lmap, obs = _maps(hvo)
    try:
        kp, z, desc = _points(300)
        z[z > 0] = F32(2.5)
        for th in (1.0, 2.5, 3.0):
            got, _ = _both(hvo, gpu_ctx, kfi, pmap, None, obs, kr.KEYFRAME, kp, z, desc, th_depth=th)
            assert len(got.pt_index) == (101 if th < 2.5 else 300) and (np.diff(got.pt_index) > 0).all()
        kl, ldesc, l3 = _lines(hvo, 300, 9)
        l3["A"][:, 2] = 2.0; l3["B"][:, 2] = 1.0
        got, _ = _both(hvo, gpu_ctx, kfi, None, lmap, obs, kr.KEYFRAME, kl=kl, ldesc=ldesc, l3=l3, th_depth=1.0)
        assert got.ln_index.tolist() == list(range(101))
    finally:
        pmap.close(); lmap.close()


@pytest.mark.parametrize("pattern", kr.HELD_PATTERNS)
def test_held_patterns(hvo, gpu_ctx, kfi, pattern):
    pmap, lmap, obs = _maps(hvo)
    try:
        kp, z, desc = _points(400); kl, ldesc, l3 = _lines(hvo, 300, 17)
        hp = kr.held_pattern(len(z), pattern, N_SLOTS, np.random.RandomState(1)); hl = kr.held_pattern(300, pattern, N_SLOTS, np.random.RandomState(2))
        for mode in (kr.KEYFRAME, kr.TEMPORAL, kr.INIT):
            _both(hvo, gpu_ctx, kfi, pmap, lmap, obs, mode, kp, z, desc, kl, ldesc, l3, th_depth=1.0, held_points=hp, held_lines=hl)
    finally:
        pmap.close(); lmap.close()


def test_many_blocks_and_bad_levels(hvo, gpu_ctx, kfi):
    """4100 features (17 work groups), levels outside the table planted among the created ones"""
    pmap, lmap, obs = _maps(hvo)
    try:
        kp, z, desc = _points(4093)
        kp["octave"][::97] = 8; kp["octave"][5::211] = -1
        got, want = _both(hvo, gpu_ctx, kfi, pmap, None, obs, kr.KEYFRAME, kp, z, desc, th_depth=100.0)
        assert (got.pt_status == kr.BAD_LEVEL).sum() >= 40 and (got.pt_slot == -1).all()
        got, _ = _both(hvo, gpu_ctx, kfi, pmap, None, obs, kr.KEYFRAME, kp, z, desc, th_depth=100.0, first_point_slot=N_SLOTS)
        made = got.pt_status == kr.CREATED
        assert got.pt_slot[made].tolist() == list(range(N_SLOTS, N_SLOTS + int(made.sum()))) and (got.pt_slot[~made] == -1).all()
    finally:
        pmap.close(); lmap.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(hvo, gpu_ctx, kfi):
    pmap, lmap, obs = _maps(hvo)
    try:
        sp, sl = _snapshot(pmap), _snapshot(lmap)
        kp, z, desc = _points(16385 - 7); kl, ldesc, l3 = _lines(hvo, 64, 5)
        hp = np.full(len(z), -1, np.int32); hl = np.full(64, -1, np.int32)

        def refused(status, match, **kw):
            a = dict(kp_un=kp[:50], depth=z[:50], desc=desc[:50], keylines=kl, ldesc=ldesc, lines3d=l3, held_points=hp[:50].copy(), held_lines=hl.copy(),
                     first_point_slot=N_SLOTS, first_line_slot=N_SLOTS)
            a.update(kw)
            with pytest.raises(hvo.HvoError, match=match) as e:
                gpu_ctx.create_keyframe_features(kfi, pmap, lmap, CAM, T0, **a)
            assert e.value.status == status
            assert _same_slots(sp, _snapshot(pmap)) and _same_slots(sl, _snapshot(lmap))

        refused(-4, "16385 features", kp_un=kp, depth=z, desc=desc, held_points=hp)
        kl2, ld2, l32 = _lines(hvo, 2049, 6)
        refused(-4, "2049 key lines", keylines=kl2, ldesc=ld2, lines3d=l32, held_lines=np.full(2049, -1, np.int32))
        nan = l3.copy(); nan["A"][9, 2] = np.nan; nan["B"][9, 2] = np.nan
        refused(-1, "NaN", lines3d=nan)
        bad = hp[:50].copy(); bad[3] = N_SLOTS
        refused(-1, "held_points", held_points=bad)
        refused(-1, "beyond the map", first_point_slot=N_SLOTS + 1)
        # held is the caller's array: the binding copies it, so the C call's own array is checked through the io block
        p, io, a = hvo._kfi_args(50, 64, kr.KEYFRAME, 3.0, 8, 1, 1.2, 1, None, None, N_SLOTS, N_SLOTS, hp[:50], hl)
        F = hvo.KfiFrame(); F.n_kp = 50; F.n_kl = 64
        keep = [np.ascontiguousarray(v) for v in (kp[:50], z[:50], desc[:50], kl, ldesc, nan)]
        for name, v in zip(("kp_un", "depth", "desc", "keylines", "ldesc", "lines3d"), keep): setattr(F, name, v.ctypes.data)
        import ctypes as C
        T = np.ascontiguousarray(T0, F32).reshape(12); c = hvo._pose_cam(CAM); r = hvo.KfiResult()
        rc = hvo.lib().hvo_create_keyframe_features(kfi.h, gpu_ctx.h, pmap.h, lmap.h, C.byref(c), hvo._p(T), C.byref(p), C.byref(F), C.byref(io), C.byref(r))
        assert rc == -1 and (a["held_points"][:50] == -1).all() and (a["held_lines"][:64] == -1).all() and (a["pt_index"] == hvo.KFI_UNTOUCHED).all()
    finally:
        pmap.close(); lmap.close()


# ---------------------------------------------------------------------------------------------------------------- the maps
def _frame(hvo, synth, cache={}):
    """one synthetic 640 x 480 frame on host arrays (shared, never modified)"""
    if "f" not in cache:
        g, d, _ = synth.make_sequence("std", 0x5EED7900, 1)
        ctx = hvo.Context(lsd_nfeatures=200)
        kp, desc = ctx.extract_orb(g[0]); kl, ld, fn = ctx.extract_lsd(g[0]); l3 = ctx.lines_3d(kl, d[0], seed=3)
        ur, z = pmr.stereo_from_depth(kp, kp, d[0], CAM[4])
        cs, ci = ctx.assign_lines_to_grid(kl, np.array(lmr.BOUNDS, F32))
        ctx.close()
        cache["f"] = dict(g=g[0], d=d[0], kp=kp, desc=desc, ur=ur, z=z, kl=kl, ld=ld, fn=fn, l3=l3, cs=cs, ci=ci)
    return cache["f"]


@pytest.mark.parametrize("existing,slots0", [(0, 0), (N_SLOTS, 0), (N_SLOTS, 4096)])
def test_map_side(hvo, synth, gpu_ctx, kfi, existing, slots0):
    """first at 0 on an empty map, appended behind existing slots (a regrowth: the maps start at 64 slots of capacity), and with room made
    beforehand.  The slots read back equal the returned values, the device arrays serve a following search, a refresh with the key frame as
    sole observer changes nothing, and the other slots keep their bytes"""
    f = _frame(hvo, synth)
    pmap, lmap, obs = _maps(hvo, existing)
    if slots0:                                                      # capacity made beforehand: no regrowth inside the call
        pmap.close(); lmap.close(); pmap = hvo.PointMap(slots=slots0); lmap = hvo.LineMap(slots=slots0)
        rng = np.random.RandomState(3); o8 = obs.astype(np.uint8)
        pmap.set_many(0, rng.uniform(-1, 1, (existing, 3)), rng.uniform(-1, 1, (existing, 3)), rng.uniform(1, 2, existing), rng.uniform(0, 1, existing),
                      rng.randint(0, 256, (existing, 32)), o8)
        lmap.set_many(0, rng.uniform(-1, 1, (existing, 6)), rng.uniform(-1, 1, (existing, 3)), rng.uniform(-1, 1, (existing, 3)), rng.uniform(1, 2, existing),
                      rng.uniform(0, 1, existing), rng.randint(0, 256, (existing, 32)), o8)
    try:
        sp, sl = _snapshot(pmap), _snapshot(lmap)
        got, want = _both(hvo, gpu_ctx, kfi, pmap, lmap, obs, kr.KEYFRAME, f["kp"], f["z"], f["desc"], f["kl"], f["ld"], f["l3"], th_depth=100.0,
                          first_point_slot=existing, first_line_slot=existing, line_n_levels=8)
        npt, nln = got.n_points_created, got.n_lines_created
        assert npt > 900 and nln > 40 and (got.pt_status == 0).all() and (got.ln_status == 0).all()
        assert pmap.counts() == (existing + npt, existing + npt, existing // 2 + npt) and lmap.counts() == (existing + nln, existing + nln, existing // 2 + nln)
        ap, al = _snapshot(pmap), _snapshot(lmap)
        assert _same_slots((existing, ap[1][:existing]), sp) and _same_slots((existing, al[1][:existing]), sl)
        for e in range(npt):
            s = ap[1][existing + e]
            assert kr.same_bits(s["pos"], got.pt_pos[e]) and kr.same_bits(s["normal"], got.pt_normal[e]) and np.array_equal(s["desc"], f["desc"][got.pt_index[e]])
            assert (F32(s["max_dist"]), F32(s["min_dist"]), s["bad"], s["observed"]) == (got.pt_max_dist[e], got.pt_min_dist[e], False, True)
            assert got.held_points[got.pt_index[e]] == existing + e
        for e in range(nln):
            s = al[1][existing + e]
            assert kr.same_bits(s["pos"], got.ln_pos[e]) and kr.same_bits(s["normal"], got.ln_normal[e]) and kr.same_bits(s["wvec"], got.ln_wvec[e])
            assert np.array_equal(s["desc"], f["ld"][got.ln_index[e]]) and (F32(s["max_dist"]), F32(s["min_dist"]), s["bad"], s["observed"]) == (got.ln_max_dist[e], got.ln_min_dist[e], False, True)
        if existing == 0:
            # the device arrays: a search of the same frame under the same pose equals the restatement's search of a map made of the returned values
            Mp = dict(pos=got.pt_pos, normal=got.pt_normal, max_dist=got.pt_max_dist, min_dist=got.pt_min_dist, desc=f["desc"][got.pt_index],
                      bad=np.zeros(npt, np.uint8), observed=np.ones(npt, np.uint8))
            held = np.full(len(f["kp"]), -1, np.int32)
            r = gpu_ctx.search_local_points(pmap, CAM, T0, f["kp"], f["ur"], f["desc"], pmr.BOUNDS, held=held, log_scale_factor=pmr.LOG_SF, n_levels=8)
            o = pmr.search_local_points(Mp, CAM, T0, pmr.BOUNDS, pmr.LOG_SF, 8, pmr.SF, 1.0, f["kp"], f["ur"], f["desc"], held, ())
            assert r.n_in_view == npt == o["n_in_view"] and np.array_equal(r.in_view_slot, o["in_view_slot"])
            # (the predicted level is not compared: maxd / dist is sf[level] exactly here, on the boundary of a library log)
            assert kr.same_bits(r.proj, o["proj"]) and kr.same_bits(r.view_cos, o["view_cos"])
            own = r.match_idx == got.pt_index                        # a new point that found its own feature: its descriptor on the device is the feature's
            assert own.sum() > 0.5 * npt and (r.match_dist[own] == 0).all()
            Ml = dict(pos=got.ln_pos, wvec=got.ln_wvec, normal=got.ln_normal, max_dist=got.ln_max_dist, min_dist=got.ln_min_dist, desc=f["ld"][got.ln_index],
                      bad=np.zeros(nln, np.uint8), observed=np.ones(nln, np.uint8))
            hl = np.full(len(f["kl"]), -1, np.int32)
            r = gpu_ctx.search_local_lines(lmap, lmr.CAM, T0, f["kl"], f["fn"], f["l3"], f["ld"], f["cs"], f["ci"], lmr.BOUNDS, held=hl, log_scale_factor=lmr.LOG_SF, th=1.0)
            o = lmr.search_local_lines(Ml, lmr.CAM, T0, lmr.BOUNDS, lmr.LOG_SF, 1.0, 0.95, f["kl"], f["fn"], f["l3"], f["ld"], f["cs"], f["ci"], hl, ())
            assert r.n_in_view == o["n_in_view"] > 0 and np.array_equal(r.in_view_slot, o["in_view_slot"]) and r.n_slots_tested == nln
            assert kr.same_bits(r.proj, o["proj"]) and kr.same_bits(r.view_cos, o["view_cos"])
        # UpdateNormalAndDepth / UpdateAverageDir with the key frame as sole observer: nothing moves
        Ow = kr.camera_parts(T0)[1]
        for m, n, idx, lev, desc, kw in ((pmap, npt, got.pt_index, f["kp"]["octave"], f["desc"], {}), (lmap, nln, got.ln_index, f["kl"]["octave"], f["ld"], dict(scale_factor=1.2))):
            obs1 = dict(obs_start=np.arange(n + 1), obs_desc=desc[idx], obs_Ow=np.tile(Ow, (n, 1)), ref_Ow=np.tile(Ow, (n, 1)), ref_level=lev[idx])
            out = m.refresh(gpu_ctx, np.arange(existing, existing + n), obs1, n_levels=8, **kw)
            assert (out["status"] == 0).all()
        assert _same_slots(ap, _snapshot(pmap)) and _same_slots(al, _snapshot(lmap))
    finally:
        pmap.close(); lmap.close()


# ---------------------------------------------------------------------------------------------------------------- the stream form
def test_stream_form_equals_the_host_form(hvo, synth, gpu_ctx, kfi):
    """a 640 x 480 synthetic frame through a Stream: the resident form equals the host-array form on the collected arrays bit for bit, a second
    call returns the same bytes, and the refusals of a frame without depth and of a stream without a stage name what is missing"""
    g, d, _ = synth.make_sequence("std", 0x5EED7A00, 1)
    stages = hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_LINES3D
    st = hvo.Stream(depth=2, stages=stages, bf=CAM[4]); st2 = hvo.Stream(depth=2, stages=hvo.STAGE_ORB | hvo.STAGE_LSD, bf=CAM[4])
    pmap, lmap, obs = _maps(hvo); pm2, lm2, _ = _maps(hvo)
    try:
        t = st.submit(g[0], d[0]); r = st.collect(t)
        n_kp, n_kl = len(r["kp_un"]), len(r["kl"])
        hp = kr.held_pattern(n_kp, "mixed", N_SLOTS, np.random.RandomState(1)); hl = kr.held_pattern(n_kl, "mixed", N_SLOTS, np.random.RandomState(2))
        kw = dict(th_depth=100.0, held_points=hp, held_lines=hl, first_point_slot=N_SLOTS, first_line_slot=N_SLOTS, line_n_levels=8)
        a = st.create_keyframe_features(kfi, pmap, lmap, t, CAM, T0, n_kp, n_kl, **kw)
        b = gpu_ctx.create_keyframe_features(kfi, pm2, lm2, CAM, T0, r["kp_un"], r["zdepth"], r["desc"], r["kl"], r["ldesc"], r["lines3d"], **kw)
        keys = kr.POINT_KEYS + kr.LINE_KEYS
        assert not kr.compare(a, {k: getattr(b, k) for k in keys + ("pt_status", "ln_status")}) and a.n_points_created == b.n_points_created > 100 and a.n_lines_created > 10
        assert _same_slots(_snapshot(pmap), _snapshot(pm2)) and _same_slots(_snapshot(lmap), _snapshot(lm2))
        want = kr.create(kr.KEYFRAME, CAM, T0, kp_un=r["kp_un"], depth=r["zdepth"], desc=r["desc"], keylines=r["kl"], ldesc=r["ldesc"], l3d_A=r["lines3d"]["A"],
                         l3d_B=r["lines3d"]["B"], pt_observed=obs, ln_observed=obs, **kw)
        assert not kr.compare(a, want)
        # the same inputs again (returned values only: the maps have changed): the same bytes twice
        kw.update(first_point_slot=-1, first_line_slot=-1)
        c1 = st.create_keyframe_features(kfi, pmap, lmap, t, CAM, T0, n_kp, n_kl, **kw); c2 = st.create_keyframe_features(kfi, pmap, lmap, t, CAM, T0, n_kp, n_kl, **kw)
        assert not kr.compare(c1, {k: getattr(c2, k) for k in keys + ("pt_status", "ln_status")})
        sp = _snapshot(pmap)
        t2 = st.submit(g[0]); st.collect(t2)
        with pytest.raises(hvo.HvoError, match="without depth"): st.create_keyframe_features(kfi, pmap, lmap, t2, CAM, T0, n_kp, n_kl, **kw)
        t3 = st2.submit(g[0], d[0]); st2.collect(t3)
        with pytest.raises(hvo.HvoError, match="HVO_STAGE_LINES3D"): st2.create_keyframe_features(kfi, pmap, lmap, t3, CAM, T0, n_kp, n_kl, **kw)
        assert _same_slots(sp, _snapshot(pmap))
    finally:
        for m in (pmap, lmap, pm2, lm2): m.close()
        st.close(); st2.close()


def test_example_runs(hvo, tmp_path):
    """examples/create_keyframe.cpp linked against the library: hvo::Tracking::CreateNewKeyFrame on its toy frame prints what the restatement
    gives, the points read back from their slots"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "create_keyframe")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "create_keyframe.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.check_output([exe]).decode()
    print(out)
    kp = np.zeros(6, kr.KEYPOINT_DT)
    kp["x"] = [100, 500, 320, 250, 420, 60]; kp["y"] = [120, 90, 240, 400, 300, 200]; kp["octave"] = [0, 2, 1, 0, 3, 1]
    z = np.array([2, 1, 0, 3, 1, 2.5], F32)
    kl = np.zeros(3, hvo.KEYLINE_DT); kl["sx"] = [100, 150, 200]
    A = np.array([[-0.5, 0.25, 2.0], [0.5, -0.5, 3.0], [0, 0, 0]]); B = np.array([[0.5, 0.25, 2.0], [0.5, 0.5, 3.0], [0, 0, 0]])
    T = np.array([[1, 0, 0, 0.25], [0, 1, 0, -0.125], [0, 0, 1, 0.5]], F32)
    w = kr.create(kr.KEYFRAME, (535.4, 539.2, 320.1, 247.6), T, kp_un=kp, depth=z, desc=np.zeros((6, 32), np.uint8), keylines=kl, ldesc=np.zeros((3, 32), np.uint8),
                  l3d_A=A, l3d_B=B, th_depth=2.25, held_points=[-1, -1, -1, 0, 1, kr.FOREIGN_UNOBSERVED], held_lines=[-1, -1, -1], pt_observed=[True, False],
                  ln_observed=[True, False], first_point_slot=2, first_line_slot=2)
    assert w["pt_index"].tolist() == [1, 4, 0, 5] and w["pt_slot"].tolist() == [2, 3, 4, 5] and w["ln_index"].tolist() == [0, 1] and w["ln_rel"].tolist() == [[1, 2, 0], [2, 1, 0]]
    assert re.search(r"created 4 of 5 point candidates and 2 of 2 line candidates, .* the maps hold 6 and 4 slots", out)
    rows = re.findall(r"point (\d+): feature (\d+) slot (\d+) status (\d+) desc (\d+) pos (\S+) (\S+) (\S+) normal (\S+) (\S+) (\S+) range (\S+) (\S+)", out)
    assert len(rows) == 4
    for e, r in enumerate(rows):
        assert [int(v) for v in r[:5]] == [e, w["pt_index"][e], w["pt_slot"][e], 0, 16 * w["pt_index"][e] + 1], r
        assert np.array([float(v) for v in r[5:]], F32).tobytes() == np.concatenate([w["pt_pos"][e], w["pt_normal"][e], [w["pt_max_dist"][e], w["pt_min_dist"][e]]]).astype(F32).tobytes(), r
    rows = re.findall(r"line (\d+): feature (\d+) slot (\d+) status (\d+) start (\S+) (\S+) (\S+) end (\S+) (\S+) (\S+) range (\S+) (\S+) rel (\d) (\d) (\d)", out)
    assert len(rows) == 2
    for e, r in enumerate(rows):
        assert [int(v) for v in r[:4]] == [e, w["ln_index"][e], w["ln_slot"][e], 0] and [int(v) for v in r[12:]] == w["ln_rel"][e].tolist(), r
        assert np.array([float(v) for v in r[4:10]]).tobytes() == w["ln_pos"][e].tobytes(), r
        assert np.array([float(v) for v in r[10:12]], F32).tobytes() == np.array([w["ln_max_dist"][e], w["ln_min_dist"][e]], F32).tobytes(), r
    assert ("held points %d %d %d %d %d %d lines %d %d %d" % (tuple(w["held_points"]) + tuple(w["held_lines"]))) in out


def test_dirty_workspace_large_then_small(hvo, gpu_ctx):
    """the workspace pre-filled with 0x00 and 0xFF, a large call then a small one: the same results as a fresh workspace gives"""
    pmap, lmap, obs = _maps(hvo)
    try:
        big = _points(3000) + _lines(hvo, 700, 41); small = _points(70) + _lines(hvo, 30, 42)
        outs = []
        for fill in (None, 0x00, 0xFF):
            k = hvo.KeyFrameInsert()
            try:
                res = []
                for kp, z, desc, kl, ld, l3 in (big, small):
                    if fill is not None: k.debug_fill(fill)
                    res.append(_both(hvo, gpu_ctx, k, pmap, lmap, obs, kr.KEYFRAME, kp, z, desc, kl, ld, l3, th_depth=2.0)[0])
                    if fill is not None: k.debug_fill(fill)
                outs.append(res)
            finally:
                k.close()
        for res in outs[1:]:
            for x, y in zip(res, outs[0]):
                assert not kr.compare(x, {k: getattr(y, k) for k in kr.POINT_KEYS + kr.LINE_KEYS + ("pt_status", "ln_status")})
    finally:
        pmap.close(); lmap.close()
