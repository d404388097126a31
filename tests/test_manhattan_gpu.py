"""Manhattan-frame tracking on the GPU, Tracking::TrackManhattanFrame (reference src/Tracking.cc:1172-1348; csrc/manhattan.hip): the host-array,
stream and batch forms against the CPU restatement tests/manhattan_ref.py (integer fields and membership bits equal; R and axis_vec within
1e-5; density within 1e-5 relative) and against each other (bit-equal)."""
import ctypes

import numpy as np
import pytest

import manhattan_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
PERM = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], F32)


def check(res, na, la, o):
    r = res.to_dict()
    for k in ("found", "n_found", "n_in_cone", "n_selected", "min_num_sn", "tracked"):
        assert r[k] == o[k], (k, r[k], o[k])
    assert r["status"] == 0
    assert np.array_equal(na, o["normal_axes"]) and np.array_equal(la, o["line_axes"])
    assert np.abs(r["R"] - o["R"]).max() <= 1e-5, (r["R"], o["R"])
    assert np.abs(r["axis_vec"] - o["axis_vec"]).max() <= 1e-5
    assert np.all(np.abs(r["density"] - o["density"]) <= 1e-5 * np.abs(o["density"]))
    return r["n_found"]


def host(ctx, normals, l3d, R):
    normals = np.asarray(normals, F32).reshape(-1, 3)
    res, na, la = ctx.track_manhattan(normals, l3d, R, axes=True)
    return check(res, na, la, ref.track_manhattan(normals, l3d, R))


def crafted():
    """(normals, l3d, R_true) of the CPU known-answer sets"""
    rng = np.random.RandomState(11)
    out = []
    n, Rt = ref.three_families(seed=1); out.append((n, None, Rt))
    Rt = ref.rot((0.3, 0.1, -0.6), 17.0)
    for pair in ((0, 1), (1, 2), (0, 2)):
        for handed in (1.0, -1.0):
            R = Rt.copy(); R[:, 2] *= handed
            n = np.concatenate([ref.family(rng, R[:, c], 400, 0.5) for c in pair] + [ref.scatter(rng, 100, R)]).astype(F32)
            out.append((n, None, R))
    Rt = ref.rot((0.1, 0.9, 0.3), 31.0)
    n = np.concatenate([ref.family(rng, Rt[:, 0], 1000, 0.5), ref.family(rng, Rt[:, 1], 30, 0.5), ref.family(rng, Rt[:, 2], 10, 0.5),
                        ref.scatter(rng, 500, Rt)]).astype(F32)
    out.append((n, None, Rt))                                                         # (b + a) / 2 threshold
    n, Rt = ref.three_families(seed=6, n=100)
    out.append((np.concatenate([n, np.full((6000, 3), np.nan, F32)]), None, Rt))     # NaN normals
    Rt = ref.rot((0.7, -0.2, 0.4), 14.0)
    n = np.concatenate([ref.family(rng, Rt[:, 0], 200, 0.5), ref.family(rng, Rt[:, 1], 200, 0.5)]).astype(F32)
    l3d = np.concatenate([ref.lines_along(rng, ref.family(rng, Rt[:, 2], 30, 1.0)),
                          ref.lines_along(rng, ref.family(rng, Rt[:, 2], 40, 1.0), good=np.zeros(40))])
    out.append((n, l3d, Rt))                                                          # an axis from lines alone
    n, Rt = ref.three_families(seed=8, n=300)
    out.append((n, ref.lines_along(rng, np.concatenate([ref.family(rng, Rt[:, c], 20, 2.0) for c in range(3)])), Rt))
    return out


def r_lasts(Rt):
    return [np.eye(3, dtype=F32), (ref.rot((1.0, 1.0, 0.0), 5.0) @ Rt).astype(F32), (Rt @ PERM).astype(F32), Rt.astype(F32)]


def test_host_form_crafted(gpu_ctx):
    seen = set()
    for normals, l3d, Rt in crafted():
        for R in r_lasts(Rt):
            seen.add(host(gpu_ctx, normals, l3d, R))
    nb, s_in, s_out = ref.boundary_normals()
    res, na, la = gpu_ctx.track_manhattan(nb, None, np.eye(3, dtype=F32), axes=True)
    assert list(res.n_in_cone) == [1, 0, 0] and list(na) == [1, 0]
    host(gpu_ctx, nb, None, np.eye(3, dtype=F32))
    assert {0, 2, 3} <= seen, seen


def test_host_form_synthetic_frames(hvo, gpu_ctx, synth):
    g, d = synth.make_batch("std", 0x5EED4100, 3)
    seen = set()
    Rw = ref.rot((0.0, 1.0, 0.0), 9.5).astype(F32)               # between the side wall and the back wall: three axes
    for k in range(3):
        sn = gpu_ctx.surface_normals(d[k])
        kl, _, _ = gpu_ctx.extract_lsd(g[k])
        l3d = gpu_ctx.lines_3d(kl, d[k], seed=5 + k)
        assert len(sn) == 80 * 107 and l3d["good"].sum() > 3
        for R in [np.eye(3, dtype=F32), (ref.rot((1.0, 1.0, 0.0), 5.0)).astype(F32), PERM, Rw]:
            seen.add(host(gpu_ctx, sn["normal"], l3d, R))
    assert {2, 3} <= seen, seen


def _seq_stream(hvo, synth, n=16, w=640, h=480):
    g, d, _ = synth.make_sequence("std", 0x5EED4200, n, w=w, h=h)
    return g, d


def test_stream_form_chained(hvo, gpu_ctx, synth):
    g, d = _seq_stream(hvo, synth)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL, seed=3)
    R = np.eye(3, dtype=F32); tracked = 0
    try:
        for k in range(len(g)):
            t = st.submit(g[k], d[k])
            res, na, la = st.track_manhattan(t, R, axes=True)
            r = st.collect(t)
            l3d = r["lines3d"]; sn = r["normals"]
            hres, hna, hla = gpu_ctx.track_manhattan(sn, l3d, R, axes=True)
            assert bytes(res) == bytes(hres), k                     # bit-equal to the host form on the ticket's tail
            assert np.array_equal(na, hna) and np.array_equal(la[:len(l3d)], hla) and not la[len(l3d):].any()
            check(res, na, la[:len(l3d)], ref.track_manhattan(sn["normal"], l3d, R))
            R = np.array(res.R[:], F32).reshape(3, 3)                 # mLastRcm
            tracked += res.tracked
        assert tracked >= len(g) // 2, tracked
    finally:
        st.close()


def test_batch_form_chained(hvo, synth):
    g, d = _seq_stream(hvo, synth)
    n = len(g)
    ctx = hvo.Context(max_batch=n)
    try:
        ctx.batch_upload(g, d)
        stages = hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL
        ctx.batch_run(stages)
        res = ctx.batch_download(hvo.STAGE_LSD | hvo.STAGE_PLANES)
        ctx.batch_download_tail(stages, res)
        R0 = (ref.rot((0.2, 1.0, 0.1), 4.0)).astype(F32)
        out = ctx.batch_track_manhattan(R0)
        assert len(out) == n
        R = R0
        for k in range(n):
            h = ctx.track_manhattan(res[k]["normals"], res[k]["lines3d"], R)
            assert bytes(out[k]) == bytes(h), k
            R = np.array(h.R[:], F32).reshape(3, 3)
        three = ctx.batch_track_manhattan(R0, n=3)
        assert [bytes(x) for x in three] == [bytes(x) for x in out[:3]]
    finally:
        ctx.close()


def test_edges(hvo, gpu_ctx, synth):
    L = hvo.lib()
    R = np.eye(3, dtype=F32)
    res = gpu_ctx.track_manhattan(np.zeros((0, 3), F32), None, R)           # no normals, no lines: R passes through
    assert res.tracked == 0 and res.n_found == 0 and res.min_num_sn == 0 and np.array_equal(np.array(res.R[:], F32), R.reshape(9))
    assert L.hvo_track_manhattan(None, None, 0, None, 0, R.ctypes.data, ctypes.byref(hvo.MfResult()), None, None) == -1
    assert L.hvo_track_manhattan(gpu_ctx.h, None, 5, None, 0, R.ctypes.data, None, None, None) == -1
    assert L.hvo_track_manhattan(gpu_ctx.h, None, 0, None, 0, None, None, None, None) == -1
    assert L.hvo_batch_track_manhattan(None, 1, R.ctypes.data, None) == -1
    g, d = synth.make_batch("std", 0x5EED4300, 1)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_PLANES, seed=3)     # without the two stages
    try:
        t = st.submit(g[0], d[0])
        with pytest.raises(hvo.HvoError):
            st.track_manhattan(t, R)
        assert b"HVO_STAGE_PLANE_TAIL" in L.hvo_stream_last_error(st.h)
        st.collect(t)
    finally:
        st.close()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL, seed=3)
    try:
        t = st.submit(g[0], d[0])
        assert L.hvo_stream_track_manhattan(st.h, t, None, None, None, None) == -1
        assert L.hvo_stream_track_manhattan(st.h, t + 5, R.ctypes.data, ctypes.byref(hvo.MfResult()), None, None) == -1   # not in the ring
        assert b"no such frame" in L.hvo_stream_last_error(st.h)
        res = st.track_manhattan(t, R)                                          # without the membership arrays
        st.collect(t)
        assert res.status == 0
    finally:
        st.close()
    ctx = hvo.Context(max_batch=1)                                             # a batch run without the two stages
    try:
        ctx.batch_upload(g, d); ctx.batch_run(hvo.STAGE_LSD)
        with pytest.raises(hvo.HvoError):
            ctx.batch_track_manhattan(R)
        assert b"HVO_STAGE_PLANE_TAIL" in L.hvo_last_error(ctx.h)
    finally:
        ctx.close()


def test_stream_beside_local_map_line_search(hvo, gpu_ctx, synth):
    """a tracker's frame: Manhattan tracking, the local-map line search (whose scratch grows on its first call and again for more map lines),
    Manhattan tracking again -- on one stream.  Each Manhattan result is bit-equal to the host form on the frame's tail."""
    g, d = _seq_stream(hvo, synth, n=2)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL | hvo.STAGE_GRIDS,
                    seed=3)
    R = ref.rot((0.0, 1.0, 0.0), 9.5).astype(F32)
    try:
        r0 = st.collect(st.submit(g[0], d[0]))
        good = np.nonzero(r0["lines3d"]["good"])[0]
        kl = r0["kl"][good]; l3 = r0["lines3d"][good]
        q = np.stack([kl["sx"], kl["sy"], kl["ex"], kl["ey"]], axis=1).astype(np.float32)
        vc = np.ones(len(q), np.float32); wv = (l3["A"] - l3["B"]).astype(np.float64); qd = r0["ldesc"][good]
        assert len(q) > 5
        t = st.submit(g[1], d[1])
        out = [st.track_manhattan(t, R, axes=True)]
        for rep in (1, 8):                                                     # first call allocates, the second grows the scratch
            idx = np.tile(np.arange(len(q)), rep)
            st.search_lines_by_projection_map(t, q[idx], vc[idx], wv[idx], qd[idx])
            out.append(st.track_manhattan(t, R, axes=True))
        r1 = st.collect(t)
        h, hna, hla = gpu_ctx.track_manhattan(r1["normals"], r1["lines3d"], R, axes=True)
        for res, na, la in out:
            assert bytes(res) == bytes(h) and np.array_equal(na, hna) and np.array_equal(la[:len(hla)], hla)
        assert h.n_found >= 2
    finally:
        st.close()


def test_large_frame(hvo, synth):
    """one 1280 x 960 frame (34 080 normals) through the host and the stream forms"""
    w, h = 1280, 960
    g, d, _ = synth.make_sequence("std", 0x5EED4400, 1, w=w, h=h)
    kw = dict(fx=535.4 * 2, fy=539.2 * 2, cx=320.1 * 2, cy=247.6 * 2)
    st = hvo.Stream(width=w, height=h, depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL, seed=3, **kw)
    ctx = hvo.Context(**kw)
    try:
        t = st.submit(g[0], d[0])
        R = ref.rot((1.0, 0.0, 0.0), 3.0).astype(F32)
        res, na, la = st.track_manhattan(t, R, axes=True)
        r = st.collect(t)
        assert len(r["normals"]) == 34080
        hres, hna, hla = ctx.track_manhattan(r["normals"], r["lines3d"], R, axes=True)
        assert bytes(res) == bytes(hres) and np.array_equal(na, hna)
        check(res, na, la[:len(r["lines3d"])], ref.track_manhattan(r["normals"]["normal"], r["lines3d"], R))
        assert res.n_found >= 2
    finally:
        st.close(); ctx.close()
