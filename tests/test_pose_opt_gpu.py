"""Optimizer::PoseOptimization on the GPU (csrc/pose_opt.hip) through the Python binding, against the CPU restatement tests/pose_opt_ref.py.
Flags, counts and the return value must be EQUAL on scenes the generator accepted (no edge's chi2 within ref.BAND of its threshold at the
end of any round: a condition on the inputs).  The pose must agree within 8 D, D measured on the CPU (ref.measured_D: edge-order sums and
numpy's libm against the kernel's tree order with every sin / cos / atan2 result moved by one ulp); it is measured here again and printed.
Iterations, trials and lambda are printed, not compared.  Figures: profiles/r09_pose_opt.txt."""
import numpy as np
import pytest

import pose_opt_ref as ref

pytestmark = pytest.mark.gpu
N_SCENES = 8


@pytest.fixture(scope="module")
def scenes():
    sc, gen = ref.accepted_scenes(N_SCENES, need_cover=True)
    print("scenes generated %d accepted %d (rejected share %.2f)" % (gen, len(sc), 1 - len(sc) / gen))
    assert len(sc) * 2 > gen
    D = ref.measured_D(sc)
    print("D = %.3e, tolerance 8 D = %.3e" % (D, 8 * D))
    return sc, D


def kw(hvo, P):
    return ref.to_binding(P, hvo.KEYPOINT_DT, hvo.LINE3D_DT)


def same_decisions(r, R):
    assert (r.ret, r.n_initial, r.n_bad, r.n_line_bad, r.n_edges, r.rounds) == (R.ret, R.n_initial, R.n_bad, R.n_line_bad, R.n_edges, R.rounds)
    assert np.array_equal(r.pt_outlier, R.pt_outlier) and np.array_equal(r.ln_outlier, R.ln_outlier)
    assert np.array_equal(r.vp_outlier, R.vp_outlier) and np.array_equal(r.pl_outlier, R.pl_outlier)


def test_scenes_against_restatement(hvo, gpu_ctx, scenes):
    sc, D = scenes
    worst = 0.0
    cover = np.zeros((6, 2), int)
    for P, R, _ in sc:
        r = gpu_ctx.pose_optimize(ref.CAM, kw(hvo, P))
        d = float(np.abs(np.array(r.Tcw_d).reshape(3, 4) - R.Tcw).max()); worst = max(worst, d)
        print("ret %d nBad %d nLineBad %d | GPU its %s trials %s lambda %s | ref its %s trials %s | pose diff %.3e"
              % (r.ret, r.n_bad, r.n_line_bad, list(r.iterations), list(r.trials), ["%.3g" % v for v in r.lam], R.iterations, R.trials, d))
        same_decisions(r, R)
        for k, (f, has) in enumerate(((R.pt_outlier, P.pt_has), (R.ln_outlier, P.ln_has), (R.vp_outlier, R.present[len(P.kp_xy) + 2 * len(P.linefn):len(P.kp_xy) + 3 * len(P.linefn)]),
                                      (R.pl_outlier[:, 0], P.pl_has[:, 0]), (R.pl_outlier[:, 1], P.pl_has[:, 1]), (R.pl_outlier[:, 2], P.pl_has[:, 2]))):
            cover[k, 0] += int(((f == 0) & (np.asarray(has) != 0)).sum()); cover[k, 1] += int((f != 0).sum())
        assert np.allclose(np.array(r.Tcw), np.array(r.Tcw_d), rtol=0, atol=1e-6)
    print("largest GPU - restatement pose difference %.3e (D %.3e, bound %.3e)" % (worst, D, 8 * D))
    assert cover.min() > 0, cover                         # every one of the six edge types with inliers and with outliers
    assert worst <= 8 * D


def test_same_bytes_twice_and_batch_equals_singles(hvo, gpu_ctx, scenes):
    sc, _ = scenes
    probs = [kw(hvo, P) for P, _, _ in sc]
    singles = [gpu_ctx.pose_optimize(ref.CAM, p) for p in probs]
    again = [gpu_ctx.pose_optimize(ref.CAM, p) for p in probs]
    batch = gpu_ctx.pose_optimize(ref.CAM, probs)
    for a, b, c in zip(singles, again, batch):
        assert bytes(a) == bytes(b) == bytes(c)
        for k in ("pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier"):
            assert np.array_equal(getattr(a, k), getattr(b, k)) and np.array_equal(getattr(a, k), getattr(c, k))


def sub(P, pts=True, lines=True, planes=True, n_pts=None):
    h = P.pt_has.copy()
    if not pts: h[:] = 0
    if n_pts is not None: h[n_pts:] = 0
    return ref.Problem(P.cam, P.Tcw, P.kp_xy, P.uright, P.inv_sigma2, h, P.pt_xyz, P.linefn, P.l3d_A, P.l3d_B,
                       P.ln_has * (1 if lines else 0), P.ln_xyz, P.pl_coef, P.pl_has * (1 if planes else 0), P.pl_map)


CASES = ["no_lines", "no_planes", "only_planes", "only_points", "pts0", "pts1", "pts2", "pts3"]


def partial(P, case):
    return {"no_lines": lambda: sub(P, lines=False), "no_planes": lambda: sub(P, planes=False), "only_planes": lambda: sub(P, pts=False, lines=False),
            "only_points": lambda: sub(P, lines=False, planes=False), "pts0": lambda: sub(P, lines=False, planes=False, n_pts=0),
            "pts1": lambda: sub(P, lines=False, planes=False, n_pts=1), "pts2": lambda: sub(P, lines=False, planes=False, n_pts=2),
            "pts3": lambda: sub(P, lines=False, planes=False, n_pts=3)}[case]()


@pytest.fixture(scope="module")
def partial_base():
    """the first generated scene all of whose partial problems the generator's rule accepts"""
    for seed in range(2000, 2040):
        P, _ = ref.make_scene(seed)
        rs = {c: ref.pose_optimization(partial(P, c)) for c in CASES}
        if all(ref.accepted(r) for r in rs.values()):
            return P, rs
    pytest.fail("no scene with every partial problem accepted")


@pytest.mark.parametrize("case", CASES)
def test_partial_problems(hvo, gpu_ctx, partial_base, scenes, case):
    P, rs = partial_base
    Q, R = partial(P, case), rs[case]
    assert ref.accepted(R)
    r = gpu_ctx.pose_optimize(ref.CAM, kw(hvo, Q))
    print(case, "ret", r.ret, R.ret, "rounds", r.rounds, R.rounds, "its", list(r.iterations), R.iterations)
    same_decisions(r, R)
    if R.n_initial < 3:
        assert r.ret == 0 and r.rounds == 0 and np.array_equal(np.array(r.Tcw, np.float32).reshape(3, 4), Q.Tcw)
    else:
        D = scenes[1]                                                     # D of the accepted set: the margin of 8 covers scenes not in the set
        d = float(np.abs(np.array(r.Tcw_d).reshape(3, 4) - R.Tcw).max())
        print(case, "pose diff %.3e, bound %.3e" % (d, 8 * D))
        assert d <= 8 * D


def test_three_edge_case_counts_and_lambda(hvo, gpu_ctx):
    """iterations, trials and the final lambda ARE compared where every trial's decision is far from rounding: three noisy stereo points
    (the fewest correspondences the function runs on; two return 0) started 0.05 rad / 0.1 m off.  Every trial of the restatement changes
    chi2 by more than 1e-4 of itself, nine orders above the rounding of the sums, so the sign of rho cannot differ."""
    P, _ = ref.make_scene(14, n_pts=3, n_lines=0, n_planes=0, noise=2.0, outliers=0.0, mono=0.0, off=(0.05, 0.1))
    R = ref.pose_optimization(P)
    assert R.rounds == 1 and min(abs(x) for st in R.steps for x in st) > 1e-5
    r = gpu_ctx.pose_optimize(ref.CAM, kw(hvo, P))
    print("three edges: its %s trials %s lambda %.6g chi2 %.6g | ref %s %s %.6g %.6g" % (list(r.iterations), list(r.trials), r.lam[0], r.chi2[0], R.iterations, R.trials, R.lam[0], R.chi2[0]))
    assert list(r.iterations) == R.iterations and list(r.trials) == R.trials and r.rounds == 1
    assert np.isclose(r.lam[0], R.lam[0], rtol=1e-6) and np.isclose(r.chi2[0], R.chi2[0], rtol=1e-6)
    same_decisions(r, R)


def test_2000_points_and_64_planes(hvo, gpu_ctx, scenes):
    """the 1280 x 960 configuration's feature count and 64 frame planes with all three roles.  With 2800 edges some chi2 always lies inside
    the band at the end of some round, so no such scene is `accepted`: the call must equal itself (twice, and inside a batch) bit for bit,
    agree with the restatement on every edge that stays outside the band in all rounds, and its pose lies within 8 D."""
    P, _ = ref.make_scene(3000, n_pts=2000, n_lines=300, n_planes=64)
    R = ref.pose_optimization(P)
    a = gpu_ctx.pose_optimize(ref.CAM, kw(hvo, P)); b = gpu_ctx.pose_optimize(ref.CAM, kw(hvo, P))
    c = gpu_ctx.pose_optimize(ref.CAM, [kw(hvo, P), kw(hvo, P)])
    assert bytes(a) == bytes(b) == bytes(c[0]) == bytes(c[1])
    assert a.n_initial == R.n_initial == 2000 + 192 and a.n_edges == R.n_edges
    clear = np.ones(len(R.present), bool)
    for chi in R.round_chi2:
        with np.errstate(invalid="ignore"):
            clear &= ~(np.abs(chi.astype(np.float64) - R.thresholds) <= ref.BAND * R.thresholds)
    n, nl, m = 2000, 300, 64
    assert np.array_equal(a.pt_outlier[clear[:n]], R.pt_outlier[clear[:n]])
    ln_clear = clear[n:n + 2 * nl:2] & clear[n + 1:n + 2 * nl:2]
    assert np.array_equal(a.ln_outlier[ln_clear], R.ln_outlier[ln_clear])
    pl_clear = clear[n + 3 * nl:].reshape(3, m).T
    assert np.array_equal(a.pl_outlier[pl_clear], R.pl_outlier[pl_clear])
    d = float(np.abs(np.array(a.Tcw_d).reshape(3, 4) - R.Tcw).max())
    D = max(scenes[1], ref.measured_D([(P, R, None)]))                    # the accepted set's D, or this scene's own if larger
    print("2000 points, 300 lines, 64 planes x 3 roles: %d edges outside the band of %d, pose diff %.3e, D %.3e, its %s trials %s"
          % (int(clear.sum()), len(clear), d, D, list(a.iterations), list(a.trials)))
    assert d <= 8 * D


def test_early_return_is_defined(hvo, gpu_ctx):
    P, R = ref.crafted_early_return()
    r = gpu_ctx.pose_optimize(ref.CAM, kw(hvo, P))
    assert r.vp_outlier[0] == 1 and R.vp_outlier[0] == 1
    same_decisions(r, R)


def test_error_paths(hvo, gpu_ctx, synth, scenes):
    P = scenes[0][0][0]
    k = kw(hvo, P)
    k["Tcw"] = P.Tcw.copy(); k["Tcw"][0, 0] = np.nan
    with pytest.raises(hvo.HvoError):                                     # a NaN pose: refused before the launch, for a list too
        gpu_ctx.pose_optimize(ref.CAM, k)
    with pytest.raises(hvo.HvoError):
        gpu_ctx.pose_optimize(ref.CAM, [kw(hvo, P), k])
    g, d = synth.make_frame("std", 0x5EED0002)
    T = P.Tcw
    s = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_ORB)              # missing stages
    try:
        with pytest.raises(hvo.HvoError):
            s.pose_optimize(s.submit(g), ref.CAM, T, (0, 0, 0))
    finally:
        s.close()
    s = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_FRAME, bf=40.0)   # a frame without depth; no such frame
    try:
        t0 = s.submit(g, d)
        with pytest.raises(hvo.HvoError):                                 # a stream with the tail stages refuses a frame without depth at submit:
            s.submit(g)                                                   # the call's own had_depth test is a guard behind that
        with pytest.raises(hvo.HvoError):
            s.pose_optimize(t0 + 5, ref.CAM, T, (0, 0, 0))
        s.pose_optimize(t0, ref.CAM, T, (0, 0, 0))                        # the frame with depth runs (no correspondences: ret 0)
    finally:
        s.close()
    s = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_FRAME, bf=0.0)    # bf <= 0: no mvuRight
    try:
        with pytest.raises(hvo.HvoError):
            s.pose_optimize(s.submit(g, d), ref.CAM, T, (0, 0, 0))
    finally:
        s.close()
    c = hvo.Context(max_batch=2)
    try:
        gg, dd = synth.make_batch("std", 0x5EED0002, 2)
        pr = dict(Tcw=T, counts=(0, 0, 0))
        c.batch_upload(gg, dd); c.batch_run(hvo.STAGE_ALL)                # no tail stages
        with pytest.raises(hvo.HvoError):
            c.batch_pose_optimize(ref.CAM, [pr])
        c.batch_run(hvo.STAGE_FRAME)
        with pytest.raises(hvo.HvoError):                                 # n beyond the batch
            c.batch_pose_optimize(ref.CAM, [pr, pr, pr])
        assert len(c.batch_pose_optimize(ref.CAM, [pr, pr])) == 2
        c.batch_upload(gg); c.batch_run(hvo.STAGE_ORB | hvo.STAGE_LSD)    # without depth
        with pytest.raises(hvo.HvoError):
            c.batch_pose_optimize(ref.CAM, [pr])
    finally:
        c.close()


def test_stream_form_equals_host_form(hvo, synth):
    """the resident frame's own arrays, downloaded, through the host form: the same bytes, so the same result bit for bit"""
    stages = hvo.STAGE_FRAME
    s = hvo.Stream(640, 480, depth=2, stages=stages, bf=40.0)
    ctx = hvo.Context()
    try:
        g, d = synth.make_frame("std", 0x5EED0002)
        t = s.submit(g, d)
        out = s.collect(t)
        tail = out
        kp_un, uright = out["kp_un"], out["uright"]
        l3d, linefn = tail["lines3d"], out["linefn"]
        pc = tail["plane_clouds"]
        coef = pc["coef"][pc["valid"] != 0]
        n, nl, m = len(kp_un), len(linefn), len(coef)
        r0 = np.random.RandomState(5)
        Tcw = np.concatenate([ref.rot_vec([0.01, -0.02, 0.015]), [[0.02], [-0.01], [0.03]]], axis=1).astype(np.float32)
        fx, fy, cx, cy, bf = ref.CAM
        z = np.where(out["zdepth"] > 0, out["zdepth"], 2.0).astype(np.float64)
        Xc = np.stack([(kp_un["x"] - cx) / fx * z, (kp_un["y"] - cy) / fy * z, z], axis=1)
        R_, t_ = Tcw[:, :3].astype(np.float64), Tcw[:, 3].astype(np.float64)
        Xw = ((Xc - t_) @ R_ + r0.normal(0, 0.004, Xc.shape)).astype(np.float32)
        pt_has = (r0.uniform(size=n) < 0.7).astype(np.uint8)
        A, B = l3d["A"], l3d["B"]
        ln_has = ((l3d["good"] != 0) & (r0.uniform(size=nl) < 0.8)).astype(np.uint8)
        notgood = np.flatnonzero(l3d["good"] == 0)
        ln_has[notgood[:2]] = 1                                           # a matched line without a good 3-D line: A = B = 0 drops its vanishing-direction edge
        ln_xyz = np.concatenate([(A - t_) @ R_, (B - t_) @ R_], axis=1) + r0.normal(0, 0.004, (nl, 6))
        pl_w = np.zeros((m, 3, 4), np.float32)
        for i in range(m):
            nc, dc = coef[i, :3].astype(np.float64), float(coef[i, 3])
            nw = R_.T @ nc; pl_w[i, 0] = np.concatenate([nw, [dc + nc @ t_]]); pl_w[i, 1] = pl_w[i, 0]; pl_w[i, 1, 3] += 1.0
            t1 = np.cross(nw, [0.3, 0.5, 0.8]); pl_w[i, 2] = np.concatenate([t1 / np.linalg.norm(t1), [1.0]])
        pl_has = np.ones((m, 3), np.uint8)
        ms = dict(pt_has=pt_has, pt_xyz=Xw, ln_has=ln_has, ln_xyz=ln_xyz, pl_has=pl_has, pl_coef_w=pl_w)
        rs = s.pose_optimize(t, ref.CAM, Tcw, (n, nl, m), **ms)
        # the context's level table: mvInvLevelSigma2 = 1 / (scale * scale) in float
        scale = np.ones(8, np.float32)
        for i in range(1, 8): scale[i] = scale[i - 1] * np.float32(1.2)
        inv_s2 = (np.float32(1.0) / (scale * scale))[np.clip(kp_un["octave"], 0, 7)]
        rh = ctx.pose_optimize(ref.CAM, dict(Tcw=Tcw, kp_un=kp_un, uright=uright, inv_sigma2=inv_s2, linefn=linefn, lines3d=l3d, plane_coef=coef, **ms))
        print("stream form: n %d nl %d m %d ret %d nBad %d nLineBad %d its %s" % (n, nl, m, rs.ret, rs.n_bad, rs.n_line_bad, list(rs.iterations)))
        assert rs.n_initial >= 3 and rs.ret > 0
        assert bytes(rs) == bytes(rh)
        for k in ("pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier"):
            assert np.array_equal(getattr(rs, k), getattr(rh, k)), k
        rn = ctx.pose_optimize(ref.CAM, dict(Tcw=Tcw, kp_un=kp_un, uright=uright, linefn=linefn, lines3d=l3d, plane_coef=coef, **ms))   # the level table
        assert bytes(rn) == bytes(rh)
        if len(notgood):
            assert not l3d["A"][notgood[0]].any() and not l3d["B"][notgood[0]].any() and rs.vp_outlier[notgood[0]] == 0
        print("stream form kernel time %.3f ms" % s.pose_last_kernel_ms(t))
        # the plane side as slots of a PlaneMap: an hvo_plane_match passed on as it is
        pmap = hvo.PlaneMap()
        try:
            for i in range(m):
                for r_ in range(3): pmap.set(3 * i + r_, pl_w[i, r_], np.zeros((1, 3), np.float32))
            slots = dict(match=3 * np.arange(m), parallel=3 * np.arange(m) + 1, vertical=3 * np.arange(m) + 2)
            slots["parallel"][0] = -1
            ms2 = dict(ms); ms2.pop("pl_has"); ms2.pop("pl_coef_w")
            rsl = s.pose_optimize(t, ref.CAM, Tcw, (n, nl, m), plane_map=pmap, plane_match=slots, **ms2)
            ph = pl_has.copy(); ph[0, 1] = 0
            rco = s.pose_optimize(t, ref.CAM, Tcw, (n, nl, m), **dict(ms, pl_has=ph))
            assert bytes(rsl) == bytes(rco) and np.array_equal(rsl.pl_outlier, rco.pl_outlier)
        finally:
            pmap.close()
        # the resident batch: frame k of a batch = the stream form on the same image, pose and map side (k1 = 0, mvuRight formed in the kernel)
        bc = hvo.Context(max_batch=3)
        try:
            g2, d2 = synth.make_frame("std", 0x5EED0003)
            bc.set_tail_params(seed=0)                                    # frame f draws with seed + f, the stream's ticket 0 with its seed 1
            bc.batch_upload(np.stack([g2, g, g2]), np.stack([d2, d, d2])); bc.batch_run(hvo.STAGE_FRAME)
            Tb = Tcw.copy(); Tb[0, 3] += 0.01
            pr = [dict(Tcw=Tb, counts=(0, 0, 0)), dict(Tcw=Tcw, counts=(n, nl, m), **ms), dict(Tcw=Tb, counts=(n, nl, m), **ms)]
            rb = bc.batch_pose_optimize(ref.CAM, pr)
            singles = [bc.batch_pose_optimize(ref.CAM, pr[:1])[0]]
            assert bytes(rb[0]) == bytes(singles[0])                      # a batch of n = n single calls
            rb2 = bc.batch_pose_optimize(ref.CAM, pr[:2])
            assert bytes(rb2[1]) == bytes(rb[1]) and rb[2].n_initial > 0
            print("batch form: frame 1 ret %d its %s; lines3d seeds: stream ticket %d, batch frame 1" % (rb[1].ret, list(rb[1].iterations), t))
            assert t == 0 and bytes(rb[1]) == bytes(rs)
            assert np.array_equal(rb[1].pt_outlier, rs.pt_outlier) and np.array_equal(rb[1].pl_outlier, rs.pl_outlier)
            print("batch kernel time for 3 frames %.3f ms" % bc.pose_last_kernel_ms())
        finally:
            bc.close()
    finally:
        s.close(); ctx.close()


def test_chain_search_associate_optimise_search(hvo, synth, orc, scenes):
    """the chain the call exists for, on a streamed synthetic sequence: per frame SearchByProjection(Cur, Last) whole on the device under the
    predicted pose (the last optimised one), plane association against a resident map, PoseOptimization on the resident frame with the
    association passed on as slots, and the optimised pose feeds the next frame's search: only map-side arrays cross PCIe.  The same chain
    with the restatement in place of the optimisation (searches still on the device, under its own poses) must give a trajectory within
    8 D per frame, accumulated (D of the accepted set, or of the frame's own problem where that is larger)."""
    K = 5
    g, d, off = synth.make_sequence("std", 0x5EED2100, K)
    cam = (535.4, 539.2, 320.1, 247.6, 40.0, 40.0 / 535.4)
    st = hvo.Stream(depth=3, stages=hvo.STAGE_FRAME, bf=cam[4])
    pmap = hvo.PlaneMap()
    scale = np.ones(8, np.float32)
    for i in range(1, 8): scale[i] = scale[i - 1] * np.float32(1.2)
    inv_s2_tab = np.float32(1.0) / (scale * scale)
    I34 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    try:
        def backproject(fr, T):
            z = fr["zdepth"]; sel = np.flatnonzero(z > 0).astype(np.int32); kp = fr["kp_un"][sel]
            Xc = np.stack([(kp["x"] - cam[2]) * z[sel] / cam[0], (kp["y"] - cam[3]) * z[sel] / cam[1], z[sel]], axis=1).astype(np.float64)
            R, t = T[:, :3].astype(np.float64), T[:, 3].astype(np.float64)
            return sel, ((Xc - t) @ R).astype(np.float32)
        t_prev = st.submit(g[0], d[0]); f_prev = st.collect(t_prev)
        pc = f_prev["plane_clouds"]; coef0 = pc["coef"][pc["valid"] != 0]
        for j, c in enumerate(coef0): pmap.set(j, c, np.zeros((1, 3), np.float32))        # frame 0's planes are the map (camera 0 = world)
        poseA = I34.copy(); poseB = I34.copy(); worst = 0.0; Dsum = 0.0
        for k in range(1, K):
            tk = st.submit(g[k], d[k]); fk = st.collect(tk)
            n, nl = len(fk["kp_un"]), len(fk["linefn"])
            pck = fk["plane_clouds"]; coefk = pck["coef"][pck["valid"] != 0]; m = len(coefk)
            out = []
            for pose, use_gpu in ((poseA, True), (poseB, False)):
                sel, X = backproject(f_prev, pose_prev[0 if use_gpu else 1] if k > 1 else I34)
                Tl = (pose_prev[0 if use_gpu else 1] if k > 1 else I34)
                ng, mi, md = st.project_last(tk, t_prev, cam, pose, Tl, sel, X, np.ones(len(sel), np.uint8), 15.0)
                pt_has = np.zeros(n, np.uint8); pt_xyz = np.zeros((n, 3), np.float32)
                ok = mi >= 0; pt_has[mi[ok]] = 1; pt_xyz[mi[ok]] = X[ok]
                pm = st.match_planes(pmap, tk, pose)
                if use_gpu:
                    r = st.pose_optimize(tk, cam[:5], pose, (n, nl, m), pt_has=pt_has, pt_xyz=pt_xyz, ln_has=np.zeros(nl, np.uint8), plane_map=pmap, plane_match=pm)
                    new = np.array(r.Tcw, np.float32).reshape(3, 4); out.append((new, r.ret, int(ok.sum())))
                else:
                    sl = np.stack([np.array(pm.match[:m]), np.array(pm.parallel[:m]), np.array(pm.vertical[:m])], axis=1)
                    pl_map = np.zeros((m, 3, 4), np.float32)
                    for i in range(m):
                        for r_ in range(3):
                            if sl[i, r_] >= 0: pl_map[i, r_] = coef0[sl[i, r_]]
                    P = ref.Problem(cam[:5], pose, np.stack([fk["kp_un"]["x"], fk["kp_un"]["y"]], axis=1), fk["uright"], inv_s2_tab[np.clip(fk["kp_un"]["octave"], 0, 7)],
                                    pt_has, pt_xyz, fk["linefn"], fk["lines3d"]["A"], fk["lines3d"]["B"], np.zeros(nl, np.uint8), None, coefk, (sl >= 0).astype(np.uint8), pl_map)
                    R = ref.pose_optimization(P)
                    Dsum += max(scenes[1], ref.measured_D([(P, R, None)]))
                    out.append((R.Tcw.astype(np.float32), R.ret, int(ok.sum())))
            pose_prev = (poseA, poseB)
            poseA, poseB = out[0][0], out[1][0]
            diff = float(np.abs(poseA.astype(np.float64) - poseB.astype(np.float64)).max()); worst = max(worst, diff)
            print("frame %d: matches %d / %d, ret GPU %d restatement %d, |pose difference| %.3e, accumulated 8 D %.3e, t = %s"
                  % (k, out[0][2], out[1][2], out[0][1], out[1][1], diff, 8 * Dsum, poseA[:, 3]))
            assert out[0][2] > 50 and out[0][1] > 30
            assert diff <= 8 * Dsum + 2 * 6e-8 * k                                        # + the float32 rounding of the pose handed on (SetPose holds floats)
            t_prev, f_prev = tk, fk
    finally:
        pmap.close(); st.close()
