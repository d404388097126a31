"""Every entry point that stages through the context's call arena (hvo_call_arena, csrc/arena.hip) or a slot map's call scratch, run on an
arena whose contents the test controls.  The modules' own GPU tests compare each call with its restatement but find the arena holding what
hipMalloc returned or what the same call left there at a similar size; an application runs fuse after create_new_map_points after pnp on
one context at changing sizes.  A kernel that reads a counter, a pass byte, a padded tail entry or a margin nobody initialised, or a
download that copies a range only partly written, shows here as a result that depends on the fill byte or on the call before.

DESIGN.md section 8 holds the reading this run confirms (what each site uploads, clears, trusts a kernel to write, and copies back); the
first fill any case sees is 0x00.  tests/arena_cases.py is the case table, tests/test_call_arena.py its census on the CPU.

  1. dirty arena       fills 0x00, 0xFF, 0x7F of the whole capacity (and of the map's scratch), proven by peeking; S three times: byte-identical, = want(S)
  2. stale self        L, S, L with no fill between: S = the dirty-arena S, both L equal and = want(L)
  3. other leftovers   all cases round-robin on ONE context: S of each, L of each in reverse order, S of each again = the results of 1 and 2
  4. regrowth          the capacity never shrinks and grows only when the request exceeds it; results either side of a regrowth = 1 and 2
  5. stream forms      the forms that stage through the ring slot's context, under the three fills of ITS arena = the host-array form"""
import numpy as np
import pytest

import arena_cases as ac

pytestmark = pytest.mark.gpu
FILLS = (0x00, 0xFF, 0x7F)
ROOM = 64 << 20                     # no case asks for more (the largest, normals_lpvo at 640 x 480, asks for 29 MB): no fill is lost to a regrowth
NAMES = [c.name for c in ac.CASES]
_base = {}


@pytest.fixture(scope="module")
def env():
    return ac.env()


def peek_is(ctx, cap, fill, *where):
    """a sample of the arena holds the fill: its first and last 4 KiB and 4 KiB from the middle"""
    for off in (0, (cap // 2) & ~4095, cap - 4096):
        b = ctx.debug_call_arena_peek(*where, off, 4096)
        assert len(b) == 4096 and (b == fill).all(), (hex(fill), off, np.unique(b)[:4])


def opened(env, c, i):
    return c.open(env, i) if c.open else {}


def closed(*objs):
    for o in objs:
        for v in o.values(): v.close()


def baseline(env, name):
    """steps 1 and 2 of a case on a context of its own -> (S result, L result), kept for steps 3 and 4"""
    if name in _base:
        return _base[name]
    c = ac.BY_NAME[name]
    (iS, wS), (iL, wL) = ac.inputs(env, name, "S"), ac.inputs(env, name, "L")
    ctx = env.hvo.Context(max_batch=4)
    oS, oL = opened(env, c, iS), opened(env, c, iL)
    try:
        assert ctx.debug_call_arena() == 0
        cap = ctx.debug_call_arena(None, ROOM)
        assert cap >= ROOM
        if c.uses_map: c.run(env, ctx, iS, oS)                            # the map's scratch exists from its first call on (that call finds what hipMalloc returned)
        outs = []
        for fill in FILLS:
            assert ctx.debug_call_arena(fill, ROOM) == cap
            peek_is(ctx, cap, fill)
            if c.uses_map: oS["map"].debug_fill_scratch(fill)
            outs.append(c.run(env, ctx, iS, oS))
            assert ctx.debug_call_arena() == cap                          # the call did not regrow: it ran on the fill
        if c.arena:                                                       # the call did write there: the fill is gone from the start of the arena
            assert (ctx.debug_call_arena_peek(0, 64) != FILLS[-1]).any()
        ac.identical(outs[0], outs[1], name + ": fill 0x00 against 0xFF")
        ac.identical(outs[0], outs[2], name + ": fill 0x00 against 0x7F")
        if c.want: c.check(env, outs[0], wS)
        L1 = c.run(env, ctx, iL, oL); S2 = c.run(env, ctx, iS, oS); L2 = c.run(env, ctx, iL, oL)
        ac.identical(S2, outs[0], name + ": S after L")
        ac.identical(L1, L2, name + ": L after S")
        if c.want: c.check(env, L1, wL)
        assert ctx.debug_call_arena() == cap
        _base[name] = (outs[0], L1)
    finally:
        closed(oS, oL); ctx.close()
    return _base[name]


@pytest.mark.parametrize("name", NAMES)
def test_dirty_arena_and_stale_self(env, name):
    baseline(env, name)


def test_other_calls_leftovers(env):
    """S of each case, L of each in reverse order, S of each again, on ONE context that starts without an arena: every regrowth on the way
    hands the next call what hipMalloc returns, every other call finds another call's layout"""
    base = {n: baseline(env, n) for n in NAMES}
    ctx = env.hvo.Context(max_batch=4)
    objs = {(n, s): opened(env, ac.BY_NAME[n], ac.inputs(env, n, s)[0]) for n in NAMES for s in "SL"}
    caps = [0]
    try:
        for size, order in (("S", NAMES), ("L", NAMES[::-1]), ("S", NAMES)):
            for n in order:
                got = ac.BY_NAME[n].run(env, ctx, ac.inputs(env, n, size)[0], objs[(n, size)])
                ac.identical(got, base[n][0 if size == "S" else 1], "%s %s in the round" % (n, size))
                caps.append(ctx.debug_call_arena())
        assert all(b >= a for a, b in zip(caps, caps[1:])) and caps[-1] > 0
    finally:
        closed(*objs.values()); ctx.close()


def test_regrowth(env):
    """smallest request, largest, smallest, and one in between: the capacity is what hvo_call_arena's rule gives for the request that made it
    grow, it grows only when a request exceeds it, it never shrinks, and the results do not depend on which side of a regrowth they ran"""
    seq = [("undistort_keypoints", "S"), ("normals_lpvo", "L"), ("undistort_keypoints", "S"), ("lines_3d", "L"), ("track_manhattan", "S")]
    need = [ac.BY_NAME[n].arena(env, ac.inputs(env, n, s)[0]) for n, s in seq]
    assert need[0] == min(need) and need[1] == max(need) and need[0] < need[4] < need[3] < need[1]
    ctx = env.hvo.Context(max_batch=1)
    try:
        cap = ctx.debug_call_arena()
        assert cap == 0
        for (n, s), want in zip(seq, need):
            got = ac.BY_NAME[n].run(env, ctx, ac.inputs(env, n, s)[0], {})
            now = ctx.debug_call_arena()
            assert now == (ac.arena_capacity(want) if want > cap else cap), (n, s, want, cap, now)
            ac.identical(got, baseline(env, n)[0 if s == "S" else 1], "%s %s at capacity %d" % (n, s, now))
            cap = now
        assert cap == ac.arena_capacity(need[1])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- the layouts' totals
# debug_call_arena() after ONE call on a fresh context = arena_capacity(the layout's total): the capacities commit 4d54914 gave on the device,
# whose layouts were hand arithmetic on bytes.  They pin every total of the typed layouts (csrc/call_stage.hpp) to 4 KiB.
CAPACITY = {("search_by_projection_keyframe", "S"): 32768, ("search_by_projection_keyframe", "L"): 380928,
            ("fuse_points", "S"): 69632, ("fuse_points", "L"): 126976,
            ("fuse_points_slots", "S"): 49152, ("fuse_points_slots", "L"): 69632,
            ("create_new_map_points", "S"): 61440, ("create_new_map_points", "L"): 159744,
            ("pnp_ransac", "S"): 16384, ("pnp_ransac", "L"): 81920,
            ("search_by_bow", "S"): 20480, ("search_by_bow", "L"): 139264,
            ("pose_optimize", "S"): 12288, ("pose_optimize", "L"): 102400,
            ("line_struct_optimize", "S"): 32768, ("line_struct_optimize", "L"): 225280,
            # the three sites that staged through match.hip's own arena until they became staged calls: measured on the commit before (dd67507)
            # as that arena's capacity after one call, (total + 4096) * 3 / 2, inverted to the layout's total (a multiple of 256 every time:
            # 75776, 276992; 85504, 248064; 57856, 192768; 8704, 117248; 12544, 135424) and pinned as arena_capacity(total)
            ("create_new_map_lines", "S"): 98304, ("create_new_map_lines", "L"): 348160,
            ("fuse_lines", "S"): 110592, ("fuse_lines", "L"): 311296,
            ("fuse_lines_slots", "S"): 73728, ("fuse_lines_slots", "L"): 241664,
            ("refresh_map_points", "S"): 12288, ("refresh_map_points", "L"): 147456,
            ("refresh_map_lines", "S"): 16384, ("refresh_map_lines", "L"): 172032}


@pytest.mark.parametrize("name,size", sorted(CAPACITY))
def test_layout_total_of_one_call(env, name, size):
    c = ac.BY_NAME[name]
    i, _ = ac.inputs(env, name, size)
    ctx = env.hvo.Context(max_batch=4)
    o = opened(env, c, i)
    try:
        c.run(env, ctx, i, o)
        assert ctx.debug_call_arena() == CAPACITY[(name, size)]
    finally:
        closed(o); ctx.close()


def _times_ok(ms, n):
    ms = tuple(ms)
    assert len(ms) == n and all(np.isfinite(v) and v >= 0 for v in ms), ms


def test_kernel_times(env):
    """the last call's device times: 0.0 on a context whose calls launched nothing (no candidate, no frame feature), finite and not negative
    after a call that ran, and of the documented length in the three results that carry them.  No magnitude is asserted"""
    hvo = env.hvo
    ctx = hvo.Context(max_batch=4)
    try:
        with pytest.raises(hvo.HvoError):
            ctx.pnp_ransac(ac.pnp_ref.CAM, [], hvo.pnp_params(**ac.PNP_P))
        assert ctx.pnp_last_kernel_ms() == (0.0, 0.0)
        with pytest.raises(hvo.HvoError):
            ctx.line_struct_optimize([])
        assert ctx.line_opt_last_kernel_ms() == (0.0, 0.0)
        i, _ = ac.inputs(env, "search_by_bow", "S")
        none = dict(desc=np.zeros((0, 32), np.uint8), node_id=np.zeros(0, np.int32), angle=np.zeros(0, np.float32))
        got = ctx.search_by_bow(none, [i["kf"]])
        assert got[0][1] == 0 and len(got[0][0]) == 0 and ctx.bow_last_kernel_ms() == (0.0, 0.0)
        for name, last, n in (("pnp_ransac", ctx.pnp_last_kernel_ms, 2), ("search_by_bow", ctx.bow_last_kernel_ms, 2), ("line_struct_optimize", ctx.line_opt_last_kernel_ms, 2)):
            ac.BY_NAME[name].run(env, ctx, ac.inputs(env, name, "S")[0], {})
            _times_ok(last(), n)
        assert ctx.bow_last_kernel_ms()[0] == 0.0                                      # no ComputeBoW ran on this context
        kfs = ac.BY_NAME["search_by_projection_keyframe"].run(env, ctx, ac.inputs(env, "search_by_projection_keyframe", "S")[0], {})
        _times_ok(kfs[0]["kernel_ms"], 2)
        fused = ac.BY_NAME["fuse_points"].run(env, ctx, ac.inputs(env, "fuse_points", "S")[0], {})
        _times_ok(fused[0]["kernel_ms"], 3)
        _, summary = ac.BY_NAME["create_new_map_points"].run(env, ctx, ac.inputs(env, "create_new_map_points", "S")[0], {})
        _times_ok(summary["kernel_ms"], 3)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the stream forms
@pytest.fixture(scope="module")
def world(env):
    """one synthetic frame with depth, submitted and collected: every stage, so that every form finds what it needs on the ring slot"""
    import new_points_ref as npr
    hvo = env.hvo
    g, d = env.synth.make_frame("std", 0x5EED5300)
    st = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_FRAME, bf=npr.CAM[4])
    ctx = hvo.Context(max_batch=1)
    v = ac._voc_open(env, dict(voc=ac._voc()))["voc"]
    try:
        tk = st.submit(g, d); fr = st.collect(tk)
        assert fr["status"] == 0 and len(fr["kp_un"]) > 300 and (fr["uright"] >= 0).sum() > 100
        yield dict(st=st, ctx=ctx, tk=tk, fr=fr, voc=v, voc_host=ac._voc())
    finally:
        v.close(); st.close(); ctx.close()


def under_fills(st, tk, call):
    cap = st.debug_call_arena(tk, None, ROOM)
    outs = []
    for fill in FILLS:
        assert st.debug_call_arena(tk, fill, ROOM) == cap
        peek_is(st, cap, fill, tk)
        outs.append(call())
        assert st.debug_call_arena(tk) == cap
    ac.identical(outs[0], outs[1], "stream: fill 0x00 against 0xFF")
    ac.identical(outs[0], outs[2], "stream: fill 0x00 against 0x7F")
    return outs[0]


def test_stream_fuse_points(env, world):
    import fuse_ref
    import point_map_ref as pm
    import test_fuse_gpu as t
    st, tk, fr = world["st"], world["tk"], world["fr"]
    kf, mp = fuse_ref.random_scene(env.hvo.KEYPOINT_DT, 0, 700, seed=61, frame=(fr["kp_un"], fr["desc"], fr["uright"], fr["zdepth"]))
    w = fuse_ref.fuse(kf, mp, pm.CAM)
    assert w["n_fused"] * 4 >= 700 and w["n_fused"] < 700
    strm = under_fills(st, tk, lambda: st.fuse_points(tk, pm.CAM, kf["Tcw"], maps=mp, skip=kf["skip"]))
    t.identical(strm, world["ctx"].fuse_points(pm.CAM, [kf], mp, pm.BOUNDS)[0], "stream against host")
    t.same(strm, w, "stream")


def test_stream_search_by_projection_keyframe(env, world):
    import kf_search_ref as ref
    import point_map_ref as pm
    import test_kf_search_gpu as t
    st, tk, fr = world["st"], world["tk"], world["fr"]
    kp, desc = fr["kp_un"], fr["desc"]; nf = len(kp)
    cs = [ref.planted_candidate(kp, desc, pm.scene_pose(j), seed=50 + j, n=n, pose_dx=0.005 * (j + 1)) for j, n in enumerate((600, 257))]
    strm = under_fills(st, tk, lambda: st.search_by_projection_keyframe(tk, pm.CAM, nf, cs, th=10.0, orb_dist=100))
    host = world["ctx"].search_by_projection_keyframe(pm.CAM, kp, desc, pm.BOUNDS, cs, th=10.0, orb_dist=100)
    for j in range(2):
        t.identical(strm[j], host[j], "stream %d" % j)
        t.same(strm[j], ref.search(cs[j], pm.CAM, kp, desc, pm.BOUNDS, 10.0, 100), "stream %d" % j)
        assert strm[j]["n_matches"] > 50


def test_stream_pnp_ransac(env, world):
    import pnp_ref as ref
    st, tk, fr = world["st"], world["tk"], world["fr"]
    kp = fr["kp_un"]; nf = len(kp)
    rng = np.random.RandomState(5)
    scale = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(7, np.float32(1.2), np.float32)])).astype(np.float32)
    sides, probs = [], []
    for j, (nk, keep) in enumerate(((300, 0.6), (120, 0.9))):
        sc = ref.planted_scene(40 + j, nk)
        R = sc["Tcw"].reshape(3, 4)[:, :3]; tv = sc["Tcw"].reshape(3, 4)[:, 3]
        match = np.full(nf, -1, np.int32)
        who = np.sort(rng.permutation(nf)[:nk]); match[who] = rng.permutation(nk)
        match[who[rng.rand(nk) > keep]] = -1
        z = rng.uniform(1.0, 4.0, nk); pos = np.zeros((nk, 3), np.float32)
        for i in np.nonzero(match >= 0)[0]:
            m = match[i]
            pc = np.array([(kp["x"][i] - ref.CAM[2]) / ref.CAM[0] * z[m], (kp["y"][i] - ref.CAM[3]) / ref.CAM[1] * z[m], z[m]])
            pos[m] = (R.T @ (pc - tv)).astype(np.float32)
        bad = rng.rand(nk) < 0.1
        outl = rng.rand(nk) < 0.2; pos[outl] += rng.randn(int(outl.sum()), 3).astype(np.float32)
        sides.append(dict(match_kf=match, pos=pos, bad=bad))
        idx = np.array([i for i in range(nf) if match[i] >= 0 and not bad[match[i]]], np.int32)
        oc = np.clip(kp["octave"][idx], 0, 7)
        probs.append(dict(p3d=pos[match[idx]], p2d=np.stack([kp["x"][idx], kp["y"][idx]], 1), sigma2=scale[oc] * scale[oc], feature_index=idx, n_features=nf))
    P = env.hvo.pnp_params(**ref.default_params(seed=21))
    strm = under_fills(st, tk, lambda: st.pnp_ransac(tk, ref.CAM, sides, P, want_sample=True))
    host = world["ctx"].pnp_ransac(ref.CAM, probs, P, want_sample=True)
    for j in range(2):
        h, s = host[j], strm[j]
        assert h["N"] == s["N"] == len(probs[j]["p3d"]) and h["T"] == s["T"] > 0 and h["events"] and len(h["events"]) == len(s["events"])
        for k in ("hyp_sample", "hyp_inliers", "hyp_event", "best_Tcw"):
            assert h[k].tobytes() == s[k].tobytes(), (j, k)
        assert np.array_equal(h["best_inliers"], s["best_inliers"]) and s["n_features"] == nf
        for a, b in zip(h["events"], s["events"]):
            assert a["Tcw"].tobytes() == b["Tcw"].tobytes() and a["n_inliers"] == b["n_inliers"] and np.array_equal(a["inliers"], b["inliers"])
            assert a["hyp_Tcw"].tobytes() == b["hyp_Tcw"].tobytes() and np.array_equal(a["hyp_inliers"], b["hyp_inliers"])


def test_stream_pose_optimize(env, world):
    import pose_opt_ref as ref
    st, tk, out = world["st"], world["tk"], world["fr"]
    kp_un, uright, l3d, linefn = out["kp_un"], out["uright"], out["lines3d"], out["linefn"]
    pc = out["plane_clouds"]; coef = pc["coef"][pc["valid"] != 0]
    n, nl, m = len(kp_un), len(linefn), len(coef)
    r0 = np.random.RandomState(5)
    Tcw = np.concatenate([ref.rot_vec([0.01, -0.02, 0.015]), [[0.02], [-0.01], [0.03]]], axis=1).astype(np.float32)
    fx, fy, cx, cy, bf = ref.CAM
    z = np.where(out["zdepth"] > 0, out["zdepth"], 2.0).astype(np.float64)
    Xc = np.stack([(kp_un["x"] - cx) / fx * z, (kp_un["y"] - cy) / fy * z, z], axis=1)
    R_, t_ = Tcw[:, :3].astype(np.float64), Tcw[:, 3].astype(np.float64)
    Xw = ((Xc - t_) @ R_ + r0.normal(0, 0.004, Xc.shape)).astype(np.float32)
    pt_has = (r0.uniform(size=n) < 0.7).astype(np.uint8)
    ln_has = ((l3d["good"] != 0) & (r0.uniform(size=nl) < 0.8)).astype(np.uint8)
    ln_xyz = np.concatenate([(l3d["A"] - t_) @ R_, (l3d["B"] - t_) @ R_], axis=1) + r0.normal(0, 0.004, (nl, 6))
    pl_w = np.zeros((m, 3, 4), np.float32)
    for i in range(m):
        nc, dc = coef[i, :3].astype(np.float64), float(coef[i, 3])
        nw = R_.T @ nc; pl_w[i, 0] = np.concatenate([nw, [dc + nc @ t_]]); pl_w[i, 1] = pl_w[i, 0]; pl_w[i, 1, 3] += 1.0
        t1 = np.cross(nw, [0.3, 0.5, 0.8]); pl_w[i, 2] = np.concatenate([t1 / np.linalg.norm(t1), [1.0]])
    ms = dict(pt_has=pt_has, pt_xyz=Xw, ln_has=ln_has, ln_xyz=ln_xyz, pl_has=np.ones((m, 3), np.uint8), pl_coef_w=pl_w)
    rs = under_fills(st, tk, lambda: st.pose_optimize(tk, ref.CAM, Tcw, (n, nl, m), **ms))
    rh = world["ctx"].pose_optimize(ref.CAM, dict(Tcw=Tcw, kp_un=kp_un, uright=uright, linefn=linefn, lines3d=l3d, plane_coef=coef, **ms))
    assert rs.n_initial >= 3 and rs.ret > 0 and bytes(rs) == bytes(rh)
    for k in ("pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier"):
        assert np.array_equal(getattr(rs, k), getattr(rh, k)), k


def test_stream_bow_search_and_create_new_map_points(env, world):
    """the frame's bag of words first (it lives in a block of its own, not in the arena), then the two forms that read it: SearchByBoW, which
    the reading found staging through the slot's arena like the five the module tests name, and CreateNewMapPoints"""
    import bow_ref
    import new_points_ref as ref
    import test_new_points_gpu as t
    st, tk, fr, v = world["st"], world["tk"], world["fr"], world["voc"]
    n = len(fr["kp_un"])
    b = st.compute_bow(tk, v, levelsup=2)
    assert len(set(b["node_id"].tolist())) > 8
    # SearchByBoW: the frame itself in reversed feature order (every feature has its twin) is the key frame
    kf = dict(desc=fr["desc"][::-1], node_id=b["node_id"][::-1], has_map_point=(np.arange(n) % 5 != 0), angle=fr["kp"]["angle"][::-1])
    frame = dict(desc=fr["desc"], node_id=b["node_id"], angle=fr["kp"]["angle"])
    ss = under_fills(st, tk, lambda: st.search_by_bow(tk, v, [kf], nnratio=0.9, check_orientation=True, th_low=80))
    want = bow_ref.search_by_bow(kf, frame, 0.9, True, 80)
    hs = world["ctx"].search_by_bow(frame, [kf], nnratio=0.9, check_orientation=True, th_low=80)
    assert np.array_equal(ss[0][0][:n], want[0]) and ss[0][1] == want[1] > 100 and (ss[0][0][n:] == -1).all()
    assert np.array_equal(hs[0][0], want[0]) and hs[0][1] == want[1]
    # CreateNewMapPoints
    cam = ref.CAM + (ref.MB,)
    has = (np.arange(n) % 4 == 0).astype(np.uint8)
    kfs = ref.neighbours_of_frame(fr["kp_un"], fr["uright"], fr["zdepth"], fr["desc"], b["node_id"], (ref.SCENE_POSES[1], ref.SCENE_POSES[0]), ref.CAM, 161, ref.MB)
    cur = dict(kp_un=fr["kp_un"], kp=fr["kp"], uright=fr["uright"], depth=fr["zdepth"], desc=fr["desc"], node_id=b["node_id"], has_map_point=has, Tcw=ref.IDENTITY, mb=ref.MB)
    w = ref.full(cur, kfs, ref.CAM, ref.CAM[4])
    assert w[1]["n_new"] > 50
    strm = under_fills(st, tk, lambda: st.create_new_map_points(tk, v, cam, ref.IDENTITY, has, kfs))
    t.identical(strm, world["ctx"].create_new_map_points(ref.CAM, cur, kfs), "stream against host")
    t.same(strm, w, "stream")


def test_stream_line_struct_optimize(env):
    """the seventh stream form the reading found on the slot's arena.  Part 2 rewrites the frame's resident 3-D lines and is refused a second
    time, so the three fills run part 1 alone (the pair pass and the copy of the end points); then both parts once, on the last fill.  A
    stream of its own: the other forms' frame keeps its lines"""
    hvo = env.hvo
    g, d = env.synth.make_frame("std", 0x5EED5301)
    st = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_FRAME, bf=40.0)
    ctx = hvo.Context(max_batch=1)
    try:
        tk = st.submit(g, d); out = st.collect(tk)
        l3d, linefn = out["lines3d"], out["linefn"]; nl = len(linefn)
        assert nl > 20 and (l3d["good"] != 0).sum() > 5
        part1 = under_fills(st, tk, lambda: st.line_struct_optimize(tk, nl, mode=hvo.LINE_STRUCT_CONSTRAINTS))
        host1 = ctx.line_struct_optimize(dict(linefn=linefn, lines3d=l3d), mode=hvo.LINE_STRUCT_CONSTRAINTS)
        ac.identical(part1, host1, "part 1: stream against host")
        assert (part1.rel != 0).sum() > 10 and np.array_equal(part1.lines, np.concatenate([l3d["A"], l3d["B"]], axis=1))
        both = st.line_struct_optimize(tk, nl)
        ac.identical(both, ctx.line_struct_optimize(dict(linefn=linefn, lines3d=l3d)), "both parts: stream against host")
        assert np.array_equal(np.abs(both.rel), part1.rel) and both.n_lines == nl           # part 2 only turns the sign of an edge it rejects
    finally:
        st.close(); ctx.close()
