"""Every operation that runs on a frame resident on the device has a batch form (hvo_batch_*: frame f of the resident batch) and a stream form
(hvo_stream_*: a slot of the ring).  Both describe the frame through one FrameView (csrc/frame_view.hpp); this file pins what that may not
move: which frames are refused, with which status and message, and that the two forms compute the same bytes on the same frame.

Part 1, the refusal matrix: one table drives every resident operation in both forms at 640 x 480.  Two cases of the matrix cannot be reached
through the API and are checked where they can be: a stream that runs the plane stages refuses a frame without depth at submit, so "submitted
without depth" exists for the line operations only; and hvo_batch_upload forgets the stages that ran, so a batch without depth is refused
by its missing stages (the status is checked, and that the stage refusal is the one that speaks).

Part 2, the same frame in two forms: three distinct frames at 501 x 397 (the odd geometry of tests/test_tail_edges_gpu.py: pitches and
per-frame strides are not round) as a batch of 3 under max_batch = 4 and through a stream of depth 4.  n = 3 under max_batch = 4 is the smallest
case in which every per-frame offset matters (f * kp_cap, f * nfeat * 3, f * tail block, f * depth frame, the max(n, max_batch) plan size):
frame 2 reads other memory if one is off.  Everything compared is integer or reproducible float arithmetic in a fixed order, so every
comparison is of bytes.  The PnP solver and SearchByBoW have no batch form: their stream form is compared with the host-array form on the
frame's collected arrays (as tests/test_pnp_gpu.py and tests/test_bow_gpu.py do)."""
import numpy as np
import pytest

import line_map_ref as lref
import point_map_ref as pref

pytestmark = pytest.mark.gpu
CAM = (535.4, 539.2, 320.1, 247.6, 40.0)                  # fx, fy, cx, cy, bf
I34 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
RW, RH, SEED = 501, 397, 9


def _rot(axis, deg):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a); t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def _pose(k):
    return np.concatenate([_rot((0.3, 1.0, -0.2), 0.4 * (k + 1)), [[0.01 * k], [-0.005], [0.02 - 0.01 * k]]], axis=1).astype(np.float32)


# ====================================================================================================== 1. the refusal matrix
@pytest.fixture(scope="module")
def maps(hvo):
    from test_bow_gpu import upload as voc_upload, vocab
    m = dict(planes=hvo.PlaneMap(), lines=hvo.LineMap(), points=hvo.PointMap(), voc=voc_upload(hvo, vocab("w", 3, 3, 17)))
    yield m
    for v in m.values():
        v.close()


def _ops(m):
    """name -> (what the refusals start with, stream call (st, ticket), batch call (ctx, n) or None, the forms in which the parent commit sets a
    message for a frame that does not exist: s = no such frame in the ring, b = n beyond the resident batch)"""
    side = dict(match_kf=np.full(4, -1, np.int32), pos=np.zeros((4, 3), np.float32), bad=np.zeros(4, bool))
    pr = dict(Tcw=I34, counts=(0, 0, 0))
    return {
        "manhattan": ("Manhattan tracking", lambda st, t: st.track_manhattan(t, np.eye(3)), lambda c, n: c.batch_track_manhattan(np.eye(3), n=n), "s"),
        "planes": ("plane association", lambda st, t: st.match_planes(m["planes"], t, I34), lambda c, n: c.batch_match_planes(m["planes"], [I34] * n), "s"),
        "pose": ("pose optimisation", lambda st, t: st.pose_optimize(t, CAM, I34, (0, 0, 0)), lambda c, n: c.batch_pose_optimize(CAM, [pr] * n), "sb"),
        "line_struct": ("line structure", lambda st, t: st.line_struct_optimize(t, 0), lambda c, n: c.batch_line_struct_optimize([0] * n), "sb"),
        "local_lines": ("local lines", lambda st, t: st.search_local_lines(m["lines"], t, CAM, I34, 0),
                        lambda c, n: c.batch_search_local_lines(m["lines"], CAM, [I34] * n, [0] * n), "sb"),
        "local_points": ("local points", lambda st, t: st.search_local_points(m["points"], t, CAM, I34, 0),
                         lambda c, n: c.batch_search_local_points(m["points"], CAM, [I34] * n, [0] * n), "sb"),
        "bow": ("bag of words", lambda st, t: st.compute_bow(t, m["voc"]), lambda c, n: c.batch_compute_bow(m["voc"], n), "b"),
        "pnp": ("pnp", lambda st, t: st.pnp_ransac(t, CAM, [side]), None, "s"),
    }


def _refused(hvo, call, *needles):
    with pytest.raises(hvo.HvoError) as e:
        call()
    assert e.value.status == -1, str(e.value)                 # HVO_ERR_INVALID_ARG
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def test_refusal_matrix(hvo, synth, maps):
    ops = _ops(maps)
    g, d = synth.make_frame("std", 0x5EED0002)
    FULL = hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL | hvo.STAGE_GRIDS
    needs_depth = ("line_struct", "local_lines")              # (the plane operations: see the module docstring)
    # ---- the stream forms
    st = hvo.Stream(depth=2, stages=hvo.STAGE_PLANES)                           # a needed stage missing: every operation lacks one
    try:
        t = st.submit(g, d)
        for name, (what, s_call, _, _) in ops.items():
            _refused(hvo, lambda: s_call(st, t), what + ": the stream must run ")
        st.collect(t)
    finally:
        st.close()
    st = hvo.Stream(depth=2, stages=FULL, bf=0.0)                               # an unknown ticket; bf <= 0
    try:
        t = st.submit(g, d)
        for name, (what, s_call, _, msg) in ops.items():
            if name == "pose":                                                   # (bf is refused before the ticket is looked at)
                _refused(hvo, lambda: s_call(st, t), "pose optimisation: the stream was created with bf <= 0 (no mvuRight)")
            else:
                _refused(hvo, lambda: s_call(st, t + 5), *([what + ": no such frame in the ring"] if "s" in msg else []))
        _refused(hvo, lambda: st.search_lines_by_projection_map(t + 5, np.zeros((1, 4)), np.ones(1), np.ones((1, 3)), np.zeros((1, 32), np.uint8)))
        st.collect(t)
    finally:
        st.close()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_LINES3D | hvo.STAGE_GRIDS, bf=40.0)      # a frame submitted without depth
    try:
        t = st.submit(g)
        for name in needs_depth:
            _refused(hvo, lambda: ops[name][1](st, t), ops[name][0] + ": the frame was submitted without depth (no 3-D lines)")
        _refused(hvo, lambda: st.search_lines_by_projection_map(t, np.zeros((1, 4)), np.ones(1), np.ones((1, 3)), np.zeros((1, 32), np.uint8)),
                 "local-map line search: the frame was submitted without depth (no 3-D lines)")
        ops["bow"][1](st, t)                                                     # (needs no depth: it runs)
        st.collect(t)
    finally:
        st.close()
    # ---- the batch forms
    ctx = hvo.Context(max_batch=2)
    try:
        ctx.batch_upload(g[None], d[None]); ctx.batch_run(hvo.STAGE_PLANES)      # a needed stage missing
        for name, (what, _, b_call, _) in ops.items():
            if b_call: _refused(hvo, lambda: b_call(ctx, 1), what + ": the last hvo_batch_run must include ")
        ctx.batch_run(FULL)                                                      # n beyond the resident batch; bf <= 0
        for name, (what, _, b_call, msg) in ops.items():
            if b_call: _refused(hvo, lambda: b_call(ctx, 2), *([what + ": n beyond the resident batch"] if "b" in msg else []))
        _refused(hvo, lambda: ctx.batch_pose_optimize(CAM[:4] + (0.0,), [dict(Tcw=I34, counts=(0, 0, 0))]), "pose optimisation: bf <= 0 (no mvuRight)")
        assert len(ctx.batch_pose_optimize(CAM, [dict(Tcw=I34, counts=(0, 0, 0))])) == 1          # (the same call with bf > 0 runs)
        ctx.batch_upload(g[None]); ctx.batch_run(hvo.STAGE_ORB | hvo.STAGE_LSD)  # uploaded without depth: refused by the stages that could not run
        for name in needs_depth + ("pose",):
            _refused(hvo, lambda: ops[name][2](ctx, 1), ops[name][0] + ": the last hvo_batch_run must include ")
    finally:
        ctx.close()


# ====================================================================================================== 2. the same frame, two forms
@pytest.fixture(scope="module")
def world(hvo, synth):
    """three frames at 501 x 397, resident twice: frames 0..2 of a batch under max_batch = 4, tickets 0..2 of a stream of depth 4; with the
    stream's collected outputs (the inputs of the map sides built below)"""
    FULL = hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_VP | hvo.STAGE_PLANE_TAIL | hvo.STAGE_GRIDS
    g, d = synth.make_batch("std", 0x5EED3310, 3, w=RW, h=RH)
    st = hvo.Stream(width=RW, height=RH, depth=4, stages=FULL, bf=CAM[4], seed=SEED)
    ctx = hvo.Context(max_batch=4)
    try:
        t = [st.submit(g[k], d[k]) for k in range(3)]
        assert t == [0, 1, 2]                                 # the 3-D lines draw with seed + ticket in the stream, seed + f in the batch
        fr = [st.collect(x) for x in t]
        ctx.set_tail_params(seed=SEED)
        ctx.batch_upload(g, d); ctx.batch_run(FULL)
        for f in fr:
            assert f["status"] == 0 and len(f["kp"]) > 200 and len(f["kl"]) > 5 and f["plane_clouds"]["valid"].sum() >= 1
        assert len({len(f["kp"]) for f in fr}) == 3           # three different frames
        yield dict(st=st, ctx=ctx, t=t, fr=fr)
    finally:
        st.close(); ctx.close()


def _same_bytes(a, b, what):
    assert bytes(a) == bytes(b), what


def test_manhattan_and_planes(hvo, world, maps):
    st, ctx, t, fr = world["st"], world["ctx"], world["t"], world["fr"]
    R0 = _rot((0.2, 1.0, 0.1), 4.0).astype(np.float32)
    out = ctx.batch_track_manhattan(R0, n=3)
    R = R0
    for k in range(3):                                        # the batch chains its frames: frame k starts from frame k - 1's R
        s = st.track_manhattan(t[k], R)
        _same_bytes(out[k], s, ("manhattan", k))
        R = np.array(s.R[:], np.float32).reshape(3, 3)
    assert any(o.n_found > 0 for o in out)
    assert [bytes(x) for x in ctx.batch_track_manhattan(R0, n=2)] == [bytes(x) for x in out[:2]]
    # plane association: frame 0's own planes (camera 0 = world) and two others are the map
    pm = hvo.PlaneMap()
    try:
        pc = fr[0]["plane_clouds"]; coef0 = pc["coef"][pc["valid"] != 0]
        for j, c in enumerate(list(coef0) + [np.array([0.6, 0.0, 0.8, 1.5], np.float32), np.array([0.0, 1.0, 0.0, -1.0], np.float32)]):
            pm.set(j, c, np.zeros((1, 3), np.float32))
        T = np.stack([I34, _pose(1), _pose(2)])
        out = ctx.batch_match_planes(pm, T)
        for k in range(3):
            _same_bytes(out[k], st.match_planes(pm, t[k], T[k]), ("planes", k))
        assert out[0].n_planes == len(coef0) and len({bytes(x) for x in out}) == 3
        assert [bytes(x) for x in ctx.batch_match_planes(pm, T[:2])] == [bytes(x) for x in out[:2]]
    finally:
        pm.close()


def _map_side(f, Tcw, rng):
    """a frame's own points, lines and planes seen from Tcw, with noise: the map side of a pose problem (as tests/test_pose_opt_gpu.py builds it)"""
    fx, fy, cx, cy, _ = CAM
    kp, l3d = f["kp_un"], f["lines3d"]
    pc = f["plane_clouds"]; coef = pc["coef"][pc["valid"] != 0]
    n, nl, m = len(kp), len(f["linefn"]), len(coef)
    R, tt = Tcw[:, :3].astype(np.float64), Tcw[:, 3].astype(np.float64)
    z = np.where(f["zdepth"] > 0, f["zdepth"], 2.0).astype(np.float64)
    Xc = np.stack([(kp["x"] - cx) / fx * z, (kp["y"] - cy) / fy * z, z], axis=1)
    ms = dict(pt_has=(rng.uniform(size=n) < 0.7).astype(np.uint8), pt_xyz=((Xc - tt) @ R + rng.normal(0, 0.004, Xc.shape)).astype(np.float32),
              ln_has=((l3d["good"] != 0) & (rng.uniform(size=nl) < 0.8)).astype(np.uint8),
              ln_xyz=np.concatenate([(l3d["A"] - tt) @ R, (l3d["B"] - tt) @ R], axis=1) + rng.normal(0, 0.004, (nl, 6)))
    pl_w = np.zeros((m, 3, 4), np.float32)
    for i in range(m):
        nc, dc = coef[i, :3].astype(np.float64), float(coef[i, 3])
        nw = R.T @ nc; pl_w[i, 0] = np.concatenate([nw, [dc + nc @ tt]]); pl_w[i, 1] = pl_w[i, 0]; pl_w[i, 1, 3] += 1.0
        t1 = np.cross(nw, [0.3, 0.5, 0.8]); pl_w[i, 2] = np.concatenate([t1 / np.linalg.norm(t1), [1.0]])
    ms.update(pl_has=np.ones((m, 3), np.uint8), pl_coef_w=pl_w)
    return (n, nl, m), ms


def test_pose_optimisation(hvo, world):
    st, ctx, t, fr = world["st"], world["ctx"], world["t"], world["fr"]
    rng = np.random.RandomState(5)
    pr, sides = [], []
    for k in range(3):
        counts, ms = _map_side(fr[k], _pose(k), rng)
        sides.append((counts, ms)); pr.append(dict(Tcw=_pose(k), counts=counts, **ms))
    out = ctx.batch_pose_optimize(CAM, pr)
    for k in range(3):
        s = st.pose_optimize(t[k], CAM, _pose(k), sides[k][0], **sides[k][1])
        _same_bytes(out[k], s, ("pose", k))
        for key in ("pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier"):
            assert np.array_equal(getattr(out[k], key), getattr(s, key)), (k, key)
        assert s.n_initial >= 3 and s.ret > 0
    two = ctx.batch_pose_optimize(CAM, pr[:2])
    assert [bytes(x) for x in two] == [bytes(x) for x in out[:2]]
    _refused(hvo, lambda: st.pose_optimize(t[2] + 9, CAM, I34, (0, 0, 0)), "pose optimisation: no such frame in the ring")


def test_local_map_searches(hvo, world):
    from test_line_map_gpu import add_frame_lines, upload as lines_upload
    from test_point_map_gpu import own_map, upload as points_upload
    st, ctx, t, fr = world["st"], world["ctx"], world["t"], world["fr"]
    T = [lref.scene_pose(k) for k in range(3)]
    M, _ = lref.make_map(400, "alt", T[0], seed=21)
    add_frame_lines(M, fr[0]["kl"], fr[0]["ldesc"], fr[0]["lines3d"], T[0], range(1, 400, 2))
    lm = lines_upload(hvo, M)
    keys = ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist", "n_par", "n_perp", "rel_map")
    try:
        nkl = [len(f["kl"]) for f in fr]
        held = [np.full(n, -1, np.int32) for n in nkl]
        for h in held: h[2] = 8
        kw = dict(seen_extra=[[0, 10]] * 3, log_scale_factor=lref.LOG_SF, th=5.0, rel_map=True)
        out = ctx.batch_search_local_lines(lm, lref.CAM, T, nkl, held=[h.copy() for h in held], **kw)
        for k in range(3):
            s = st.search_local_lines(lm, t[k], lref.CAM, T[k], nkl[k], held=held[k].copy(), seen_extra=[0, 10], log_scale_factor=lref.LOG_SF, th=5.0, rel_map=True)
            for key in keys:
                assert getattr(out[k], key).tobytes() == getattr(s, key).tobytes(), ("local lines", k, key)
            assert (out[k].n_in_view, out[k].n_matches, out[k].n_gated, out[k].n_slots_tested) == (s.n_in_view, s.n_matches, s.n_gated, s.n_slots_tested)
        assert out[0].n_in_view > 0 and out[0].n_matches > 0
        two = ctx.batch_search_local_lines(lm, lref.CAM, T[:2], nkl[:2], held=[h.copy() for h in held[:2]], seen_extra=[[0, 10]] * 2, log_scale_factor=lref.LOG_SF,
                                           th=5.0, rel_map=True)
        for k in range(2):
            for key in keys:
                assert getattr(two[k], key).tobytes() == getattr(out[k], key).tobytes(), ("local lines, n = 2", k, key)
    finally:
        lm.close()
    # the points
    T = [pref.estimated_pose(pref.scene_pose(k), 0.005 * k) for k in range(3)]
    M, feats = own_map((fr[0]["kp_un"], fr[0]["desc"], fr[0]["uright"], fr[0]["zdepth"]), pref.scene_pose(0), n_extra=200)
    M["observed"][::4] = 0
    pm = points_upload(hvo, M)
    keys = ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist")
    try:
        nkp = [len(f["kp"]) for f in fr]
        held = [np.full(n, -1, np.int32) for n in nkp]
        for h in held: h[2] = 8; h[5] = hvo.HELD_FOREIGN_OBSERVED
        kw = dict(th=3.0, log_scale_factor=pref.LOG_SF, n_levels=pref.N_LEVELS)
        out = ctx.batch_search_local_points(pm, CAM, T, nkp, held=[h.copy() for h in held], seen_extra=[[0, 10]] * 3, **kw)
        for k in range(3):
            s = st.search_local_points(pm, t[k], CAM, T[k], nkp[k], held=held[k].copy(), seen_extra=[0, 10], **kw)
            for key in keys:
                assert getattr(out[k], key).tobytes() == getattr(s, key).tobytes(), ("local points", k, key)
            assert (out[k].n_in_view, out[k].n_matches, out[k].n_slots_tested) == (s.n_in_view, s.n_matches, s.n_slots_tested)
        assert out[0].n_matches > len(feats) / 4
        two = ctx.batch_search_local_points(pm, CAM, T[:2], nkp[:2], held=[h.copy() for h in held[:2]], seen_extra=[[0, 10]] * 2, **kw)
        for k in range(2):
            for key in keys:
                assert getattr(two[k], key).tobytes() == getattr(out[k], key).tobytes(), ("local points, n = 2", k, key)
    finally:
        pm.close()


def test_bag_of_words_and_pnp(hvo, world):
    import pnp_ref
    from test_bow_gpu import same_bow, upload as voc_upload, vocab
    from test_pnp_gpu import params_of
    st, ctx, t, fr = world["st"], world["ctx"], world["t"], world["fr"]
    v = voc_upload(hvo, vocab((4, 6, 4), 4, 6, 104))
    try:
        out = ctx.batch_compute_bow(v, 3, levelsup=4)
        sb = [st.compute_bow(t[k], v, levelsup=4) for k in range(3)]
        for k in range(3):
            assert out[k]["computed"] and sb[k]["computed"]
            same_bow(out[k], sb[k], "frame %d" % k)
            assert len(out[k]["word_id"]) == len(fr[k]["kp"]) and len(out[k]["bow_word"]) > 10
        two = ctx.batch_compute_bow(v, 2, levelsup=4)
        for k in range(2):
            same_bow(two[k], out[k], "n = 2, frame %d" % k)
        # SearchByBoW has no batch form: the stream form on frame 2 against the host-array form on its collected arrays
        kfs = [dict(desc=fr[j]["desc"][::o], node_id=sb[j]["node_id"][::o], has_map_point=(np.arange(len(fr[j]["desc"])) % 5 != 0), angle=fr[j]["kp"]["angle"][::o])
               for j, o in ((2, -1), (0, 1))]
        frame = dict(desc=fr[2]["desc"], node_id=sb[2]["node_id"], angle=fr[2]["kp"]["angle"])
        n2 = len(fr[2]["desc"])
        hs = ctx.search_by_bow(frame, kfs, nnratio=0.9, check_orientation=True, th_low=80)
        ss = st.search_by_bow(t[2], v, kfs, nnratio=0.9, check_orientation=True, th_low=80)
        for j in range(2):
            assert np.array_equal(ss[j][0][:n2], hs[j][0]) and ss[j][1] == hs[j][1] and (ss[j][0][n2:] == -1).all(), j
        assert hs[0][1] > 100
    finally:
        v.close()
    # the PnP solver has no batch form either: the stream form on frame 2 against the host-array form (the constructor's compaction on the host)
    kp = fr[2]["kp_un"]; nf = len(kp)
    rng = np.random.RandomState(5)
    scale = np.ones(8, np.float32)
    for i in range(1, 8): scale[i] = scale[i - 1] * np.float32(1.2)
    cam = pnp_ref.CAM
    sides, probs = [], []
    for j, (nk, keep) in enumerate(((200, 0.5), (90, 0.9))):
        sc = pnp_ref.planted_scene(40 + j, nk)
        R = sc["Tcw"].reshape(3, 4)[:, :3]; tt = sc["Tcw"].reshape(3, 4)[:, 3]
        match = np.full(nf, -1, np.int32)
        who = np.sort(rng.permutation(nf)[:nk]); match[who] = rng.permutation(nk)
        match[who[rng.rand(nk) > keep]] = -1
        z = rng.uniform(1.0, 4.0, nk); pos = np.zeros((nk, 3), np.float32)
        for i in np.nonzero(match >= 0)[0]:
            m = match[i]
            pos[m] = (R.T @ (np.array([(kp["x"][i] - cam[2]) / cam[0] * z[m], (kp["y"][i] - cam[3]) / cam[1] * z[m], z[m]]) - tt)).astype(np.float32)
        bad = rng.rand(nk) < 0.1
        sides.append(dict(match_kf=match, pos=pos, bad=bad))
        idx = np.array([i for i in range(nf) if match[i] >= 0 and not bad[match[i]]], np.int32)
        probs.append(dict(p3d=pos[match[idx]], p2d=np.stack([kp["x"][idx], kp["y"][idx]], 1), sigma2=scale[kp["octave"][idx]] * scale[kp["octave"][idx]],
                          feature_index=idx, n_features=nf))
    P = params_of(hvo, pnp_ref.default_params(seed=21))
    host = ctx.pnp_ransac(cam, probs, P, want_sample=True)
    strm = st.pnp_ransac(t[2], cam, sides, P, want_sample=True)
    for j in range(2):
        h, s = host[j], strm[j]
        assert h["N"] == s["N"] == len(probs[j]["p3d"]) and h["T"] == s["T"] > 0 and s["n_features"] == nf
        for key in ("hyp_sample", "hyp_inliers", "hyp_event", "best_Tcw"):
            assert h[key].tobytes() == s[key].tobytes(), (j, key)
        assert np.array_equal(h["best_inliers"], s["best_inliers"]) and len(h["events"]) == len(s["events"])
        for a, b in zip(h["events"], s["events"]):
            assert a["Tcw"].tobytes() == b["Tcw"].tobytes() and a["n_inliers"] == b["n_inliers"] and np.array_equal(a["inliers"], b["inliers"])


def test_line_structure(hvo, world):
    """last: the optimisation rewrites A, B of the resident 3-D lines in both forms"""
    st, ctx, t, fr = world["st"], world["ctx"], world["t"], world["fr"]
    nkl = [len(f["kl"]) for f in fr]
    def same(a, b, what):
        _same_bytes(a, b, what)
        assert a.rel.tobytes() == b.rel.tobytes() and a.lines.tobytes() == b.lines.tobytes(), what
    c3 = ctx.batch_line_struct_optimize(nkl, mode=hvo.LINE_STRUCT_CONSTRAINTS)               # part 1 alone rewrites nothing: n = 2 against n = 3
    c2 = ctx.batch_line_struct_optimize(nkl[:2], mode=hvo.LINE_STRUCT_CONSTRAINTS)
    for k in range(2):
        same(c2[k], c3[k], ("constraints, n = 2", k))
    out = ctx.batch_line_struct_optimize(nkl)
    for k in range(3):
        same(c3[k], st.line_struct_optimize(t[k], nkl[k], mode=hvo.LINE_STRUCT_CONSTRAINTS), ("constraints", k))
        same(out[k], st.line_struct_optimize(t[k], nkl[k]), ("line structure", k))
    assert any(o.n_edges > 0 for o in out)
    _refused(hvo, lambda: ctx.batch_line_struct_optimize(nkl), "optimised already")
    _refused(hvo, lambda: st.line_struct_optimize(t[1], nkl[1]), "optimised already")
