"""MapPlane::UpdateCoefficientsAndPoints on the GPU (reference src/MapPlane.cc:300-368; csrc/plane_update.hip) through the C ABI: the host
and stream forms against the CPU restatement tests/plane_update_ref.py.  Exact integer sums and reproducible double arithmetic: every
comparison is bit-equal, on the uint32 views.

The kernel sorts (voxel, point) keys with a bitonic network: 64 lanes a wave, PU_TILE = 4096 keys per LDS tile, the key array padded to a
power of two.  The sizes below cross a wave (63 / 64 / 65 points), one tile (4096 / 4097) and two tiles plus one (8193)."""
import ctypes

import numpy as np
import pytest

import plane_assoc_ref as aref
import plane_update_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32
I34 = np.eye(4, dtype=F32)[:3]
MERGE, INSERT = ref.MERGE, ref.INSERT
TILE = 4096


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def build_map(hvo, slot_list, **kw):
    m = hvo.PlaneMap(**kw)
    for j, (w, xyz, bad) in enumerate(slot_list):
        m.set(j, w, xyz)
        if bad:
            m.set_bad(j)
    return m


def read_map(m):
    return [[m.slot(j)[0], m.points(j), m.slot(j)[2]] for j in range(m.counts()[0])]


def check_map(m, slots, what=""):
    """the device map against the restatement's list: coefficients, flags and clouds bit-equal"""
    assert m.counts()[0] == len(slots), (what, m.counts(), len(slots))
    for j, (w, xyz, bad) in enumerate(slots):
        c, n, b = m.slot(j)
        assert n == len(xyz) and b == bool(bad), (what, j, n, len(xyz), b, bad)
        assert np.array_equal(bits(c), bits(w)), (what, j, c, w)
        assert np.array_equal(bits(m.points(j)), bits(xyz)), (what, j)
    assert m.counts()[2] == sum(len(s[1]) for s in slots)


def check_result(r, o, what=""):
    for k in ("status", "n_frame", "n_before", "n_after"):
        assert np.array_equal(r[k], o[k]), (what, k, r[k], o[k])
    assert r["n_done"] == o["n_done"], what


def run(ctx, m, slots, rec, cloud, Tcw, ops, Twc=None, what=""):
    """one call on the device and on the restatement (slots is updated in place), compared"""
    r = ctx.update_map_planes(m, rec, cloud, Tcw, ops, Twc)
    o = ref.apply(slots, rec, cloud, Tcw, Twc, ops)
    check_result(r, o, what)
    check_map(m, slots, what)
    return r


def plain_slot(xyz, bad=False, coef=(0, 0, 1, -1)):
    return [np.array(coef, F32), np.asarray(xyz, F32).reshape(-1, 3), bad]


def grid_points(n, z=1.0):
    """n points in n distinct voxels, coordinates in 64ths + a voxel's multiple: distinct, finite, none on a voxel face"""
    k = np.arange(n)
    return np.stack([(k % 37) * 0.1 + 3 / 64, (k // 37) * 0.1 + 3 / 64, np.full(n, z)], axis=1).astype(F32)


def test_host_form_crafted_voxel_cases(hvo, gpu_ctx):
    """the restatement's known answers through the kernel: one voxel's mean, the voxel faces, a lower bound that moves down, the refusal"""
    inv = F32(1.0) / F32(0.1)
    edge = []
    for k in (-7, -3, -1, 1, 2, 3, 7, 10, 33):
        c = F32(k) * F32(0.1)
        edge += [np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))]
    edge = np.array(edge, F32)
    a = np.array([[3, 3, 3], [15, 3, 3], [3, 9, 3], [3, 3, 23]], F32) / 64
    cases = [("one voxel", [[1 / 64, 2 / 64, 3 / 64], [3 / 64, 4 / 64, 5 / 64], [3 / 64, 4 / 64, 6 / 64]], np.zeros((0, 3))),
             ("faces x", np.stack([edge, np.zeros_like(edge), np.ones_like(edge)], axis=1), [[0.05, 0.05, 1.05]]),
             ("faces z", np.stack([np.zeros_like(edge), np.ones_like(edge), edge], axis=1), [[0.05, 1.05, 0.05]]),
             ("bound moves down", a[::-1], np.array([[-35, -15, -9]], F32) / 64),
             ("slot not sorted", a[:2], a[[3, 2, 0]]),
             ("overflow", [[0, 0, 0], [1e9, 0, 0]], [[0.05, 0.05, 0.05]]),
             ("overflow cells", [[0, 0, 0], [2000, 2000, 2000]], [[0.05, 0.05, 0.05]]),
             ("overflow in the slot", [[0, 0, 0]], [[0.05, 0.05, 0.05], [0, -3e9, 0]])]
    for name, frame, slot in cases:
        rec, cloud = ref.records_for([frame])
        slots = [plain_slot(slot)]
        m = build_map(hvo, slots)
        try:
            r = run(gpu_ctx, m, slots, rec, cloud, I34, [(0, 0, MERGE)], what=name)
            assert (r["status"][0] == ref.UNSUPPORTED) == name.startswith("overflow"), name
            if name == "one voxel":
                assert r["n_after"][0] == 1
            if name == "bound moves down":
                assert np.array_equal(bits(slots[0][1]), bits(np.concatenate([np.array([[-35, -15, -9]], F32) / 64, a])))
        finally:
            m.close()


def test_host_form_crafted_poses(hvo, gpu_ctx):
    """the transform's cases through the kernel: the identity, each branch of Quaterniond(Matrix3d), w < 0, a rotation orthonormal to 1e-7
    only, a translation of 1e3; a MERGE under Tcw and an INSERT under the float inverse"""
    rng = np.random.RandomState(20)
    for name, Tcw in ref.transform_cases():
        T4 = np.vstack([Tcw.astype(np.float64), [0, 0, 0, 1]])
        Twc = np.linalg.inv(T4)[:3].astype(F32)
        world = ref.wall(rng, 300, 2.0)
        frame = (np.hstack([ref.wall(rng, 90, 2.0).astype(np.float64), np.ones((90, 1))]) @ T4.T)[:, :3].astype(F32)
        rec, cloud = ref.records_for([frame], [aref.camera_coef(Tcw, (0, 0, 1, -2))])
        slots = [plain_slot(world)]
        m = build_map(hvo, slots)
        try:
            r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(0, 0, MERGE), (0, 1, INSERT)], Twc, what=name)
            assert r["n_done"] == 2 and r["n_after"][0] > 0 and r["n_after"][1] > 0, name
        finally:
            m.close()


@pytest.mark.parametrize("n_frame", [1, 5])
def test_host_form_slot_sizes_padding_and_rooms(hvo, gpu_ctx, n_frame):
    """slots of 0, 1, 3, 4, 5, 63, 64, 65 points: the NaN padding to four, a room that doubles (64 -> 128), the other slots' bytes"""
    sizes = [0, 1, 3, 4, 5, 63, 64, 65]
    slots = [plain_slot(grid_points(n)) for n in sizes]
    m = build_map(hvo, slots)
    try:
        frame = grid_points(400)[-n_frame:] + F32(0.5 / 64)                     # new voxels, none of the slots'
        rec, cloud = ref.records_for([frame, grid_points(3)])                   # plane 1 falls into the slots' first voxels
        for j in range(len(sizes)):
            before = read_map(m)
            run(gpu_ctx, m, slots, rec, cloud, I34, [(0, j, MERGE)], what=("grow", j))
            run(gpu_ctx, m, slots, rec, cloud, I34, [(1, j, MERGE)], what=("fuse", j))
            for i, s in enumerate(read_map(m)):
                if i != j:
                    assert np.array_equal(bits(s[1]), bits(before[i][1])), (j, i)
        res, dm, am = gpu_ctx.match_planes(m, np.array([[0, 0, 1, -1]], F32), I34, None, matrices=True)   # the padding is NaN: it never wins
        o = aref.search_map(np.array([[0, 0, 1, -1]], F32), I34, [tuple(s) for s in slots])
        assert np.array_equal(dm, o["dist_mat"]) and res.match[0] == o["match"][0]
    finally:
        m.close()


def test_host_form_lists(hvo, gpu_ctx):
    """the same slot twice, INSERT past the end, INSERT then MERGE into it, a bad slot, a NaN point in a slot, a refusal between two good ones"""
    rng = np.random.RandomState(21)
    clouds = [ref.voxel_grid(ref.wall(rng, n, 2.0)) for n in (40, 90, 150, 7)] + [np.array([[0, 0, 1], [1e9, 0, 1]], F32)]
    coefs = [aref.camera_coef(I34, (0, 0, 1, -2 - 0.25 * i)) for i in range(5)]
    rec, cloud = ref.records_for(clouds, coefs, valid=[1, 1, 0, 1, 1])          # frame planes 0, 1, 2, 3 = records 0, 1, 3, 4
    Tcw = ref.random_pose(rng, 0.5)
    Twc = np.linalg.inv(np.vstack([Tcw.astype(np.float64), [0, 0, 0, 1]]))[:3].astype(F32)
    nan_cloud = ref.wall(rng, 30, 2.0); nan_cloud[4, 0] = np.nan; nan_cloud[9, 2] = -np.inf
    slots = [plain_slot(ref.wall(rng, 200, 2.0)), plain_slot(ref.wall(rng, 77, 2.0), bad=True), plain_slot(nan_cloud)]
    m = build_map(hvo, slots)
    try:
        run(gpu_ctx, m, slots, rec, cloud, Tcw, [(0, 0, MERGE), (1, 0, MERGE), (0, 0, MERGE)], what="same slot three times")
        run(gpu_ctx, m, slots, rec, cloud, Tcw, [(1, 1, MERGE), (2, 2, MERGE)], what="bad slot, NaN slot")
        assert m.slot(1)[2] and np.isfinite(m.points(2)).all()
        r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(0, 0, MERGE), (3, 1, MERGE), (1, 2, MERGE)], what="refusal between two good ones")
        assert list(r["status"]) == [0, ref.UNSUPPORTED, 0] and r["n_done"] == 2
        r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(0, 6, INSERT)], Twc, what="INSERT past the end")
        assert m.counts()[:2] == (7, 3) and [m.slot(j)[1:] for j in (3, 4, 5)] == [(0, True)] * 3
        run(gpu_ctx, m, slots, rec, cloud, Tcw, [(1, 7, INSERT), (0, 7, MERGE), (2, 4, INSERT), (1, 1, INSERT)], Twc, what="INSERT then MERGE; replaced slots keep their flag")
        assert m.slot(4)[2] and m.slot(1)[2] and not m.slot(7)[2]
        r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(3, 9, INSERT), (0, 9, MERGE), (0, 3, MERGE)], Twc, what="a refused INSERT does not extend the map")
        assert list(r["status"]) == [ref.UNSUPPORTED, ref.UNSUPPORTED, 0] and m.counts()[0] == 8
        # the map's extension follows list order also when an INSERT is refused: slot 10 exists (skipped over: bad, empty) by the time its
        # own operation runs, because the second INSERT into 12 came first in the list
        r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(3, 12, INSERT), (0, 12, INSERT), (1, 10, INSERT)], Twc, what="refused INSERT, INSERT, INSERT below it")
        assert list(r["status"]) == [ref.UNSUPPORTED, 0, 0] and m.counts()[0] == 13 and m.slot(10)[2] and not m.slot(12)[2]
        r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(3, 15, INSERT), (0, 15, INSERT), (1, 14, MERGE), (3, 17, INSERT), (2, 16, INSERT)], Twc, what="refused INSERT, INSERT, MERGE below it")
        assert list(r["status"]) == [ref.UNSUPPORTED, 0, 0, ref.UNSUPPORTED, 0] and m.counts()[0] == 17 and m.slot(14)[1:] == (len(slots[14][1]), True)
        for _ in range(3):                                                      # the same refusal again and again: the map stays as it is
            r = run(gpu_ctx, m, slots, rec, cloud, Tcw, [(3, 0, MERGE), (3, 20, INSERT)], Twc, what="repeated refusal")
            assert r["n_done"] == 0 and m.counts()[0] == 17
        run(gpu_ctx, m, slots, rec, cloud, Tcw, [], what="an empty list")
    finally:
        m.close()


def test_host_form_malformed_lists(hvo, gpu_ctx):
    rng = np.random.RandomState(22)
    rec, cloud = ref.records_for([ref.wall(rng, 20), ref.wall(rng, 30)], valid=[1, 0])
    slots = [plain_slot(ref.wall(rng, 50)), plain_slot(ref.wall(rng, 60))]
    m = build_map(hvo, slots)
    L = hvo.lib()
    try:
        before = read_map(m); counts = m.counts()
        good = (0, 0, MERGE)
        bad_lists = [("plane index", [good, (1, 1, MERGE)], None), ("negative plane", [(-1, 0, MERGE)], None), ("MERGE into no slot", [good, (0, 2, MERGE)], None),
                     ("INSERT without Twc", [good, (0, 2, INSERT)], None), ("unknown op", [good, (0, 1, 2)], I34), ("negative slot", [(0, -1, INSERT)], I34),
                     ("slot beyond the range", [(0, 1 << 20, INSERT)], I34)]
        for name, ops, Twc in bad_lists:
            with pytest.raises(hvo.HvoError) as e:
                gpu_ctx.update_map_planes(m, rec, cloud, I34, ops, Twc)
            assert e.value.status == -1 and "plane map update" in str(e.value), name
        u = hvo.PlaneUpdate(); res = hvo.PlaneUpdateResult()
        args = lambda: (gpu_ctx.h, m.h, hvo._p(rec), len(rec), hvo._p(cloud), len(cloud), hvo._p(I34), None, ctypes.byref(u), ctypes.byref(res))
        for n in (-1, 65):
            u.n = n
            assert L.hvo_update_map_planes(*args()) == -1
        u.n = 1
        rec2 = rec.copy(); rec2["first"][0] = len(cloud) - 5                    # a record whose cloud leaves the frame's cloud
        assert L.hvo_update_map_planes(gpu_ctx.h, m.h, hvo._p(rec2), len(rec2), hvo._p(cloud), len(cloud), hvo._p(I34), None, ctypes.byref(u), ctypes.byref(res)) == -1
        assert L.hvo_update_map_planes(None, m.h, hvo._p(rec), len(rec), hvo._p(cloud), len(cloud), hvo._p(I34), None, ctypes.byref(u), ctypes.byref(res)) == -1
        assert L.hvo_update_map_planes(gpu_ctx.h, None, hvo._p(rec), len(rec), hvo._p(cloud), len(cloud), hvo._p(I34), None, ctypes.byref(u), ctypes.byref(res)) == -1
        assert L.hvo_update_map_planes(gpu_ctx.h, m.h, hvo._p(rec), len(rec), hvo._p(cloud), len(cloud), None, None, ctypes.byref(u), ctypes.byref(res)) == -1
        assert L.hvo_update_map_planes(gpu_ctx.h, m.h, hvo._p(rec), 65, hvo._p(cloud), len(cloud), hvo._p(I34), None, ctypes.byref(u), ctypes.byref(res)) == -1
        n = ctypes.c_int(0)
        assert L.hvo_plane_map_get_points(m.h, 2, None, 0, ctypes.byref(n)) == -1 and L.hvo_plane_map_get_points(m.h, 0, None, 0, ctypes.byref(n)) == -5 and n.value == 50
        assert m.counts() == counts
        for a, b in zip(read_map(m), before):
            assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[0]), bits(b[0])) and a[2] == b[2]
    finally:
        m.close()


def test_host_form_generated(hvo, gpu_ctx):
    """slots of 1000, 4097 and 20000 points and the sizes around the sort's tile, frame clouds of 1, 257 and 2000 points, random poses; one,
    several and 64 operations a call; the untouched slots' bytes stay, also when the pool grows (the map starts with room for 4096 points)"""
    rng = np.random.RandomState(23)
    sizes = [1000, 4097, 20000, TILE - 1, TILE, 2 * TILE, 3000]
    slots = [plain_slot(ref.wall(rng, n)) for n in sizes]
    m = build_map(hvo, slots, slots=2, points=4096)
    try:
        for step, ops in enumerate([[(0, 0, MERGE)], [(1, 2, MERGE)], [(2, 3, MERGE), (2, 4, MERGE), (2, 5, MERGE)], [(1, 1, MERGE), (0, 2, MERGE), (0, 1, MERGE), (1, 6, MERGE)]]):
            Tcw = ref.random_pose(rng, 1.0)
            T4 = np.vstack([Tcw.astype(np.float64), [0, 0, 0, 1]])
            frames = [(np.hstack([ref.wall(rng, n).astype(np.float64), np.ones((n, 1))]) @ T4.T)[:, :3].astype(F32) for n in (257, 2000, 1)]
            rec, cloud = ref.records_for(frames)
            before = read_map(m)
            r = run(gpu_ctx, m, slots, rec, cloud, Tcw, ops, what=("generated", step))
            assert r["n_done"] == len(ops)
            touched = {s for _, s, _ in ops}
            for j, s in enumerate(read_map(m)):
                if j not in touched:
                    assert np.array_equal(bits(s[1]), bits(before[j][1])), (step, j)
    finally:
        m.close()


def test_host_form_64_operations(hvo, gpu_ctx):
    """64 frame planes into 64 slots in one call, then 64 operations on 8 slots (eight rounds)"""
    rng = np.random.RandomState(24)
    slots = [plain_slot(ref.wall(rng, 150 + 13 * j, 3.0)) for j in range(64)]
    frames = [ref.wall(rng, 20 + j, 3.0) for j in range(64)]
    rec, cloud = ref.records_for(frames)
    Tcw = ref.random_pose(rng, 0.3)
    m = build_map(hvo, slots)
    try:
        run(gpu_ctx, m, slots, rec, cloud, Tcw, [(j, 63 - j, MERGE) for j in range(64)], what="64 slots")
        run(gpu_ctx, m, slots, rec, cloud, Tcw, [(j, j % 8, MERGE) for j in range(64)], what="8 slots, 8 rounds")
    finally:
        m.close()


def _observe(rng, world, cloud_w, Tcw, n):
    """a frame's voxel cloud of a world plane: n of its world points seen from the pose, voxel-filtered in the camera frame as the tail does"""
    T4 = np.vstack([Tcw.astype(np.float64), [0, 0, 0, 1]])
    pick = cloud_w[rng.randint(0, len(cloud_w), n)].astype(np.float64) + rng.normal(scale=0.01, size=(n, 3))
    return ref.voxel_grid((np.hstack([pick, np.ones((n, 1))]) @ T4.T)[:, :3].astype(F32)), aref.camera_coef(Tcw, world)


def test_sequence_of_updates_keeps_the_map_matchable(hvo, gpu_ctx):
    """eight updates in a row against the restatement chained; after each, the association on the updated map equals the restatement's on
    its map and, bit for bit, the association on a fresh map filled through set: the pool layout and the chunk list are right"""
    rng = np.random.RandomState(25)
    worlds = [np.array(w, F32) for w in ((0, 0, 1, -2), (1, 0, 0, 1.5), (0, 1, 0, -1))]
    walls = [aref.plane_cloud(rng, w, 3000, extent=6.0) for w in worlds]
    slots = [[w, ref.voxel_grid(c[:900]), False] for w, c in zip(worlds, walls)]
    m = build_map(hvo, slots, points=1024)
    try:
        for step in range(8):
            Tcw = np.asarray(aref.pose(aref.rot(rng.normal(size=3), rng.uniform(0, 15)), rng.uniform(-0.5, 0.5, 3)), F32)
            obs = [_observe(rng, w, c, Tcw, 400 + 150 * step) for w, c in zip(worlds, walls)]
            rec, cloud = ref.records_for([o[0] for o in obs], [o[1] for o in obs])
            coef = rec["coef"]
            pm = gpu_ctx.match_planes(m, coef, Tcw)
            assert list(pm.match[:3]) == [0, 1, 2], (step, list(pm.match[:3]))
            run(gpu_ctx, m, slots, rec, cloud, Tcw, [(i, pm.match[i], MERGE) for i in range(3)], what=("sequence", step))
            res, dm, am = gpu_ctx.match_planes(m, coef, Tcw, None, matrices=True)
            o = aref.search_map(coef, Tcw, [tuple(s) for s in slots])
            assert np.array_equal(res.to_dict()["match"], o["match"]) and np.array_equal(dm, o["dist_mat"]) and np.array_equal(res.to_dict()["dist"], o["dist"])
            fresh = build_map(hvo, slots)
            try:
                assert bytes(gpu_ctx.match_planes(fresh, coef, Tcw)) == bytes(res)
            finally:
                fresh.close()
        assert all(len(s[1]) > 900 for s in slots)
    finally:
        m.close()


def test_stream_form(hvo, gpu_ctx, synth):
    """a synthetic frame with the plane tail resident: the stream form equals the host form on the arrays collect returned, bit for bit; the
    frame's own results are the same as for a frame that was not used for an update; the refusals without the stage, without depth and
    for a frame that is not in the ring"""
    g, d, _ = synth.make_sequence("std", 0x5EED5100, 2)
    rng = np.random.RandomState(26)
    Tcw = ref.random_pose(rng, 1.0)
    Twc = np.linalg.inv(np.vstack([Tcw.astype(np.float64), [0, 0, 0, 1]]))[:3].astype(F32)
    st = hvo.Stream(width=640, height=480, depth=2, stages=hvo.STAGE_PLANES | hvo.STAGE_PLANE_TAIL, seed=3)
    ma = mb = None
    try:
        plain = st.collect(st.submit(g[0], d[0]))
        rec, cloud = plain["plane_clouds"], plain["cloud_xyz"].reshape(-1, 3)
        nv = int(rec["valid"].sum())
        assert nv >= 2
        ops0 = [(i, i, INSERT) for i in range(nv)]
        ops1 = [(i, nv - 1 - i, MERGE) for i in range(nv)] + [(0, nv + 1, INSERT), (1, 0, MERGE)]
        ma, mb = hvo.PlaneMap(), hvo.PlaneMap()
        t = st.submit(g[0], d[0])
        ra = st.update_map_planes(ma, t, Tcw, ops0, Twc)
        rb = gpu_ctx.update_map_planes(mb, rec, cloud, Tcw, ops0, Twc)
        ra1 = st.update_map_planes(ma, t, Tcw, ops1, Twc)
        rb1 = gpu_ctx.update_map_planes(mb, rec, cloud, Tcw, ops1, Twc)
        for x, y in ((ra, rb), (ra1, rb1)):
            check_result(x, y, "stream against host")
        assert ra["n_done"] == nv and ra1["n_done"] == nv + 2 and ma.counts()[0] == nv + 2
        check_map(ma, read_map(mb), "stream against host")
        slots = []
        ref.apply(slots, rec, cloud, Tcw, Twc, ops0); ref.apply(slots, rec, cloud, Tcw, Twc, ops1)
        check_map(ma, slots, "stream against the restatement")
        with pytest.raises(hvo.HvoError) as e:
            st.update_map_planes(ma, t, Tcw, [(nv, 0, MERGE)])
        assert e.value.status == -1
        used = st.collect(t)                                                    # the frame's results did not change
        for k in plain:
            if isinstance(plain[k], np.ndarray):
                assert plain[k].tobytes() == used[k].tobytes(), k
        with pytest.raises(hvo.HvoError) as e:                                  # a stream that runs the plane stages refuses a frame without depth at
            st.submit(g[1], None)                                               # submit: the update's own refusal (its FrameNeed row) has nothing to see
        assert e.value.status == -1
        with pytest.raises(hvo.HvoError) as e:
            st.update_map_planes(ma, t + 1, Tcw, ops1, Twc)
        assert e.value.status == -1 and "no such frame" in str(e.value)
    finally:
        st.close()
        for m in (ma, mb):
            if m:
                m.close()
    st = hvo.Stream(width=640, height=480, depth=2, stages=hvo.STAGE_PLANES, seed=3)
    m = hvo.PlaneMap()
    try:
        t = st.submit(g[0], d[0])
        with pytest.raises(hvo.HvoError) as e:
            st.update_map_planes(m, t, Tcw, [])
        assert e.value.status == -1 and "HVO_STAGE_PLANE_TAIL" in str(e.value)
        st.collect(t)
    finally:
        st.close(); m.close()


def test_example_runs(hvo, synth, tmp_path):
    """examples/plane_map_update.cpp linked against the library and run on two frames of a synthetic sequence: the first frame's planes are
    inserted, the second frame's are matched, merged and matched again"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "plane_map_update")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "plane_map_update.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d, _ = synth.make_sequence("std", 0x5EED5100, 2)
    args = []
    for k in range(2):
        g[k].tofile(tmp_path / ("g%d.u8" % k)); d[k].tofile(tmp_path / ("d%d.u16" % k))
        args += [str(tmp_path / ("g%d.u8" % k)), str(tmp_path / ("d%d.u16" % k))]
    out = subprocess.check_output([exe] + args).decode()
    print(out)
    seeded = re.search(r"map: (\d+) planes, (\d+) points", out)
    assert seeded and int(seeded.group(1)) >= 2 and int(seeded.group(2)) > 0, out
    upd = re.search(r"frame 1 planes (\d+) matched (\d+) inliers (-?\d+) updated (\d+) points (\d+) -> (\d+) newPlane \d rematched (\d+)", out)
    assert upd, out
    matched, updated, before, after, rematched = (int(upd.group(i)) for i in (2, 4, 5, 6, 7))
    assert matched >= 1 and updated == matched and after >= before and rematched >= matched, out
    assert re.search(r"slot 0: (\d+) points", out)
