"""Map-plane association on the GPU, PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:10-81; csrc/plane_assoc.hip) through
the C ABI: the host, stream and batch forms against the CPU restatement tests/plane_assoc_ref.py.  Everything is reproducible float arithmetic
plus an exact minimum, so every comparison is array_equal / bit-equal: a tolerance would hide a contracted multiply-add."""
import ctypes

import numpy as np
import pytest

import plane_assoc_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
THS = (ref.DEFAULT_TH, ref.TUM3_TH)
TAIL = lambda hvo: hvo.STAGE_PLANES | hvo.STAGE_PLANE_TAIL


def build_map(hvo, slot_list, **kw):
    m = hvo.PlaneMap(**kw)
    for j, (w, xyz, bad) in enumerate(slot_list):
        m.set(j, w, xyz)
        if bad:
            m.set_bad(j)
    return m


def check(res, o, dm=None, am=None):
    """a PlaneMatch against the restatement's dict: integers equal, floats bit-equal"""
    r = res.to_dict()
    assert r["n_planes"] == o["n_planes"] and r["n_matches"] == o["n_matches"], (r["n_planes"], r["n_matches"], o["n_matches"])
    for k in ("match", "vertical", "parallel"):
        assert np.array_equal(r[k], o[k]), (k, r[k], o[k])
    assert np.array_equal(r["pM"].view(np.uint32), o["pM"].view(np.uint32))
    assert np.array_equal(r["dist"], o["dist"]), (r["dist"], o["dist"])
    n = r["n_planes"]
    assert all(v == -1 for v in res.match[n:]) and all(v == -1 for v in res.plane_idx[n:])
    if dm is not None:
        assert np.array_equal(dm, o["dist_mat"])
        assert np.array_equal(am, o["angle_mat"], equal_nan=True)


def same_but_plane_idx(a, b):
    """two PlaneMatch bit-equal except plane_idx (the host form numbers its planes 0..n-1, the resident forms give the record's index)"""
    a, b = bytes(a), bytes(b)
    return a[:8 + 768] == b[:8 + 768] and a[8 + 1024:] == b[8 + 1024:]


def host(ctx, m, coef, Tcw, slots, th):
    res, dm, am = ctx.match_planes(m, coef, Tcw, th, matrices=True)
    o = ref.search_map(coef, Tcw, slots, th)
    check(res, o, dm, am)
    assert list(res.plane_idx[:len(coef)]) == list(range(len(coef)))
    return o


def test_host_form_crafted(hvo, gpu_ctx):
    for name, coef, Tcw, slots, th, exp in ref.crafted_cases():
        m = build_map(hvo, slots)
        try:
            o = host(gpu_ctx, m, coef, Tcw, slots, th)
            assert (o["match"][0], o["vertical"][0], o["parallel"][0]) == tuple(exp[:3]), name
        finally:
            m.close()


def test_host_form_generated_scenes(hvo, gpu_ctx):
    """0 slots to a few thousand, more than 1 M points, sizes that are no multiples of 64, one slot with most of the points"""
    tot = dict(match=0, vertical=0, parallel=0, fell=0, unmatched=0, fell_parallel=0)
    for sc in ref.SCENES + [ref.BIG_SCENE]:
        coef, Tcw, slots = ref.make_scene(*sc)
        m = build_map(hvo, slots)
        try:
            assert m.counts() == (len(slots), sum(1 for s in slots if not s[2]), sum(len(s[1]) for s in slots))
            for th in THS:
                o = host(gpu_ctx, m, coef, Tcw, slots, th)
                for k, v in ref.scene_stats(o).items():
                    tot[k] += v
            again = gpu_ctx.match_planes(m, coef, Tcw, THS[0])                 # the same call twice: the scratch is re-initialised
            assert bytes(again) == bytes(gpu_ctx.match_planes(m, coef, Tcw, THS[0]))
        finally:
            m.close()
    assert all(v > 0 for v in tot.values()), tot


def test_map_mutation(hvo, gpu_ctx):
    """replace a slot by a larger cloud past the initial capacities, mark bad, mark good: equal to the restatement on the mutated map, and
    the other slots' columns do not move"""
    coef, Tcw, slots = ref.make_scene(*ref.SCENES[3])
    rng = np.random.RandomState(9)
    m = build_map(hvo, slots, slots=4, points=100)                              # both capacities grow while the map is built
    try:
        res0, dm0, am0 = gpu_ctx.match_planes(m, coef, Tcw, None, matrices=True)
        check(res0, ref.search_map(coef, Tcw, slots), dm0, am0)
        j = int(res0.match[0]) if res0.match[0] >= 0 else 5
        w = slots[j][0]
        slots[j] = (w, ref.plane_cloud(rng, w.astype(np.float64), 200001), slots[j][2])       # far past every capacity so far
        m.set(j, *slots[j][:2])
        res1, dm1, am1 = gpu_ctx.match_planes(m, coef, Tcw, None, matrices=True)
        check(res1, ref.search_map(coef, Tcw, slots), dm1, am1)
        keep = np.arange(len(slots)) != j
        assert np.array_equal(dm0[:, keep], dm1[:, keep]) and np.array_equal(am0, am1, equal_nan=True)
        slots[j] = (w, slots[j][1][:11], slots[j][2]); m.set(j, w, slots[j][1])                # and smaller again, in the same room
        host(gpu_ctx, m, coef, Tcw, slots, ref.TUM3_TH)
        for k in sorted(set(int(v) for v in res0.match[:res0.n_planes] if v >= 0))[:3]:        # matched slots go bad
            slots[k] = (slots[k][0], slots[k][1], True); m.set_bad(k, True)
        o = host(gpu_ctx, m, coef, Tcw, slots, ref.DEFAULT_TH)
        assert not np.array_equal(o["match"], np.array(res0.match[:res0.n_planes]))
        for k in range(len(slots)):                                                            # and every slot good
            slots[k] = (slots[k][0], slots[k][1], False); m.set_bad(k, False)
        host(gpu_ctx, m, coef, Tcw, slots, ref.DEFAULT_TH)
        m.set(len(slots) + 2, slots[0][0], slots[0][1])                                        # a slot past the end: the skipped ones are bad and empty
        slots += [(np.zeros(4, F32), np.zeros((0, 3), F32), True)] * 2 + [(slots[0][0], slots[0][1], False)]
        host(gpu_ctx, m, coef, Tcw, slots, ref.DEFAULT_TH)
        c, n, bad = m.slot(len(slots) - 2)
        assert n == 0 and bad and m.counts()[0] == len(slots)
    finally:
        m.close()


def _frame_map(rng, pcs, cloud, T_wc):
    """map slots from a frame's downloaded plane tail, moved into the world by T_wc (4 x 4, camera -> world): per valid plane its cloud and
    its coefficients (T_wc^-T coef); returns (slots, index of each valid plane among the records)"""
    slots, idx = [], []
    Tcw = np.linalg.inv(T_wc)
    for i, pc in enumerate(pcs):
        if not pc["valid"]:
            continue
        xyz = cloud[pc["first"]: pc["first"] + pc["n_points"]].astype(np.float64)
        xyz_w = (xyz @ T_wc[:3, :3].T + T_wc[:3, 3]).astype(F32)
        slots.append(((Tcw.T @ pc["coef"].astype(np.float64)).astype(F32), xyz_w, False)); idx.append(i)
    return slots, idx


def _stream_case(hvo, gpu_ctx, synth, w, h, seed, **kw):
    g, d, _ = synth.make_sequence("std", seed, 3, w=w, h=h)
    st = hvo.Stream(width=w, height=h, depth=2, stages=TAIL(hvo), seed=3, **kw)
    rng = np.random.RandomState(3)
    T_wc = np.eye(4); T_wc[:3, :3] = ref.rot((0.3, 1.0, -0.2), 25.0); T_wc[:3, 3] = (0.4, -1.1, 2.3)
    Tcw = np.linalg.inv(T_wc)[:3].astype(F32)
    m = None
    try:
        r0 = st.collect(st.submit(g[0], d[0]))
        slots, idx0 = _frame_map(rng, r0["plane_clouds"], r0["cloud_xyz"].reshape(-1, 3), T_wc)
        assert len(slots) >= 2
        filler = ref.make_scene(77, 70, 20000)[2]                                # other map planes around them
        slots = filler[:35] + slots + filler[35:]
        m = build_map(hvo, slots)
        for k in (0, 1, 2):                                                     # the frame itself, then later frames of the same scene
            t = st.submit(g[k], d[k])
            out = [st.match_planes(m, t, Tcw, th) for th in THS]
            r = st.collect(t)
            pcs = r["plane_clouds"]; valid = np.nonzero(pcs["valid"])[0]
            coef = pcs["coef"][valid]
            for res, th in zip(out, THS):
                assert list(res.plane_idx[:res.n_planes]) == list(valid)
                check(res, ref.search_map(coef, Tcw, slots, th))
                assert same_but_plane_idx(res, gpu_ctx.match_planes(m, coef, Tcw, th))       # bit-equal to the host form
            if k == 0:                                                          # each valid plane finds its own map plane
                assert list(out[0].match[:len(valid)]) == [35 + i for i in range(len(valid))]
                assert out[0].n_matches == len(valid)
    finally:
        st.close()
        if m:
            m.close()


def test_stream_form_640(hvo, gpu_ctx, synth):
    _stream_case(hvo, gpu_ctx, synth, 640, 480, 0x5EED5100)


def test_stream_form_1280(hvo, gpu_ctx, synth):
    _stream_case(hvo, gpu_ctx, synth, 1280, 960, 0x5EED5200, fx=535.4 * 2, fy=539.2 * 2, cx=320.1 * 2, cy=247.6 * 2)


def test_batch_form(hvo, synth):
    """a resident batch of distinct frames under distinct poses: per frame bit-equal to the host form; again after another hvo_batch_run"""
    n = 6
    g, d, _ = synth.make_sequence("std", 0x5EED5300, n)
    g2, d2, _ = synth.make_sequence("std", 0x5EED5400, n)
    ctx = hvo.Context(max_batch=n)
    rng = np.random.RandomState(4)
    m = None
    try:
        Tcw = np.stack([ref.pose(ref.rot(rng.normal(size=3), rng.uniform(0, 40)), rng.uniform(-1, 1, 3)) for _ in range(n)])
        for it, (gg, dd) in enumerate(((g, d), (g2, d2))):
            ctx.batch_upload(gg, dd); ctx.batch_run(TAIL(hvo))
            res = ctx.batch_download(hvo.STAGE_PLANES); ctx.batch_download_tail(TAIL(hvo), res)
            if m is None:
                T_wc = np.vstack([Tcw[0].astype(np.float64), [0, 0, 0, 1]]); T_wc = np.linalg.inv(T_wc)
                slots, _ = _frame_map(rng, res[0]["plane_clouds"], res[0]["cloud_xyz"].reshape(-1, 3), T_wc)
                slots = slots + ref.make_scene(78, 200, 90000)[2]
                m = build_map(hvo, slots)
            for th in THS:
                out = ctx.batch_match_planes(m, Tcw, th)
                assert len(out) == n
                for k in range(n):
                    valid = np.nonzero(res[k]["plane_clouds"]["valid"])[0]
                    h = ctx.match_planes(m, res[k]["plane_clouds"]["coef"][valid], Tcw[k], th)
                    assert list(out[k].plane_idx[:out[k].n_planes]) == list(valid)
                    assert same_but_plane_idx(out[k], h), (it, k)
                if it == 0:
                    assert out[0].n_matches == out[0].n_planes >= 2
            three = ctx.batch_match_planes(m, Tcw[:3], THS[0])
            assert [bytes(x) for x in three] == [bytes(x) for x in ctx.batch_match_planes(m, Tcw, THS[0])[:3]]
    finally:
        ctx.close()
        if m:
            m.close()


def test_edges(hvo, gpu_ctx, synth):
    L = hvo.lib()
    T = ref.T_EXACT; c = ref.exact_frame_plane().reshape(1, 4)
    res = hvo.PlaneMatch()
    m = hvo.PlaneMap()
    try:
        r = gpu_ctx.match_planes(m, c, T)                                      # empty map: all -1, no error
        assert (r.n_planes, r.n_matches, r.match[0], r.vertical[0], r.parallel[0]) == (1, 0, -1, -1, -1)
        m.set(0, *ref.slot(1.0, [0.0625])[:2])
        r = gpu_ctx.match_planes(m, np.zeros((0, 4), F32), T)                  # no frame planes
        assert (r.n_planes, r.n_matches) == (0, 0) and all(v == -1 for v in r.match)
        r = gpu_ctx.match_planes(m, np.tile(c, (64, 1)), T)                    # 64 planes are allowed
        assert r.n_planes == 64 and r.n_matches == 64
        big = np.tile(c, (65, 1))
        assert L.hvo_match_planes(gpu_ctx.h, m.h, big.ctypes.data, 65, T.ctypes.data, None, ctypes.byref(res), None, None) == -1
        assert L.hvo_match_planes(gpu_ctx.h, m.h, c.ctypes.data, -1, T.ctypes.data, None, ctypes.byref(res), None, None) == -1
        assert L.hvo_match_planes(None, m.h, c.ctypes.data, 1, T.ctypes.data, None, ctypes.byref(res), None, None) == -1
        assert L.hvo_match_planes(gpu_ctx.h, None, c.ctypes.data, 1, T.ctypes.data, None, ctypes.byref(res), None, None) == -1
        assert L.hvo_match_planes(gpu_ctx.h, m.h, None, 1, T.ctypes.data, None, ctypes.byref(res), None, None) == -1
        assert L.hvo_match_planes(gpu_ctx.h, m.h, c.ctypes.data, 1, None, None, ctypes.byref(res), None, None) == -1
        assert L.hvo_match_planes(gpu_ctx.h, m.h, c.ctypes.data, 1, T.ctypes.data, None, None, None, None) == -1
        nan_th = np.array([0.1, np.nan, 0.08, 0.99], F32)
        assert L.hvo_match_planes(gpu_ctx.h, m.h, c.ctypes.data, 1, T.ctypes.data, nan_th.ctypes.data, ctypes.byref(res), None, None) == -1
        assert L.hvo_plane_map_set_bad(m.h, 1, 1) == -1 and L.hvo_plane_map_set_bad(m.h, -1, 1) == -1          # a slot out of range
        assert L.hvo_plane_map_set(m.h, -1, c.ctypes.data, None, 0) == -1 and L.hvo_plane_map_set(m.h, 1 << 20, c.ctypes.data, None, 0) == -1
        assert L.hvo_plane_map_set(m.h, 0, c.ctypes.data, None, 5) == -1 and L.hvo_plane_map_set(m.h, 0, None, None, 0) == -1
        assert L.hvo_plane_map_slot(m.h, 1, None, None, None) == -1 and L.hvo_plane_map_counts(None, None, None, None) == -1
        assert L.hvo_batch_match_planes(None, m.h, 1, T.ctypes.data, None, ctypes.byref(res)) == -1
        g, d = synth.make_batch("std", 0x5EED5500, 1)
        st = hvo.Stream(depth=2, stages=hvo.STAGE_PLANES, seed=3)               # without the stage
        try:
            t = st.submit(g[0], d[0])
            with pytest.raises(hvo.HvoError):
                st.match_planes(m, t, T)
            assert b"HVO_STAGE_PLANE_TAIL" in L.hvo_stream_last_error(st.h)
            st.collect(t)
        finally:
            st.close()
        st = hvo.Stream(depth=2, stages=TAIL(hvo), seed=3)
        try:
            t = st.submit(g[0], d[0])
            assert L.hvo_stream_match_planes(st.h, m.h, t + 5, T.ctypes.data, None, ctypes.byref(res)) == -1
            assert b"no such frame" in L.hvo_stream_last_error(st.h)
            assert L.hvo_stream_match_planes(st.h, None, t, T.ctypes.data, None, ctypes.byref(res)) == -1
            assert L.hvo_stream_match_planes(st.h, m.h, t, None, None, ctypes.byref(res)) == -1
            st.collect(t)
        finally:
            st.close()
        ctx = hvo.Context(max_batch=1)                                          # a batch run without the stage
        try:
            ctx.batch_upload(g, d); ctx.batch_run(hvo.STAGE_PLANES)
            with pytest.raises(hvo.HvoError):
                ctx.batch_match_planes(m, T.reshape(1, 12))
            assert b"HVO_STAGE_PLANE_TAIL" in L.hvo_last_error(ctx.h)
        finally:
            ctx.close()
    finally:
        m.close()


def test_stream_beside_manhattan_and_line_search(hvo, gpu_ctx, synth):
    """a tracker's frame on one stream: plane association, Manhattan tracking, the local-map line search (its scratch grows on the first call and
    again for more map lines), the association against a map that grew meanwhile, the same map from a context in between.  Every association
    is equal to the restatement on the frame's downloaded tail, and Manhattan tracking is unchanged by it."""
    g, d, _ = synth.make_sequence("std", 0x5EED5600, 2)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL | hvo.STAGE_GRIDS, seed=3)
    rng = np.random.RandomState(6)
    T_wc = np.eye(4); T_wc[:3, :3] = ref.rot((1.0, 0.2, 0.1), 12.0); T_wc[:3, 3] = (0.1, 0.2, -0.3)
    Tcw = np.linalg.inv(T_wc)[:3].astype(F32)
    R = ref.rot((0.0, 1.0, 0.0), 9.5).astype(F32)
    m = None
    try:
        r0 = st.collect(st.submit(g[0], d[0]))
        slots, _ = _frame_map(rng, r0["plane_clouds"], r0["cloud_xyz"].reshape(-1, 3), T_wc)
        m = build_map(hvo, slots)
        good = np.nonzero(r0["lines3d"]["good"])[0]
        kl = r0["kl"][good]; l3 = r0["lines3d"][good]
        q = np.stack([kl["sx"], kl["sy"], kl["ex"], kl["ey"]], axis=1).astype(np.float32)
        vc = np.ones(len(q), np.float32); wv = (l3["A"] - l3["B"]).astype(np.float64); qd = r0["ldesc"][good]
        t = st.submit(g[1], d[1])
        pa = [(st.match_planes(m, t, Tcw), list(slots))]
        mf = [st.track_manhattan(t, R)]
        more = ref.make_scene(79, 300, 120000)[2]
        for rep, extra in ((1, more[:100]), (8, more[100:])):
            idx = np.tile(np.arange(len(q)), rep)
            st.search_lines_by_projection_map(t, q[idx], vc[idx], wv[idx], qd[idx])
            for s in extra:                                                     # the map grows between the calls
                m.set(len(slots), s[0], s[1]); slots.append((s[0], s[1], False))
            pa.append((st.match_planes(m, t, Tcw), list(slots)))
            mf.append(st.track_manhattan(t, R))
            gpu_ctx.match_planes(m, np.zeros((3, 4), F32) + 0.5, Tcw)           # the map's scratch used from a context in between
        r1 = st.collect(t)
        valid = np.nonzero(r1["plane_clouds"]["valid"])[0]; coef = r1["plane_clouds"]["coef"][valid]
        assert len(valid) >= 2
        for res, sl in pa:
            check(res, ref.search_map(coef, Tcw, sl))
        assert pa[0][0].n_matches >= 1
        h = gpu_ctx.track_manhattan(r1["normals"], r1["lines3d"], R)
        assert all(bytes(x) == bytes(h) for x in mf)
    finally:
        st.close()
        if m:
            m.close()
