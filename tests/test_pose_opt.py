"""CPU tests of the pose-optimisation restatement (tests/pose_opt_ref.py) by known answers, its behaviour on generated scenes, and the
presence of the new entry points in the header, the library and the binding."""
import ctypes
import os
import re

import numpy as np

import pose_opt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ref.Ops()


def test_exp_against_rodrigues_and_inverse():
    w = np.array([0.3, -0.2, 0.5]); u = np.concatenate([w, [0.1, 0.2, -0.3]])
    q, t = ref.se3_exp(u, OPS)
    assert np.allclose(ref.quat_to_R(q), ref.rot_vec(w), atol=1e-15)
    a = ref.se3_exp(u, OPS); b = ref.se3_exp(-u, OPS)
    I = ref.se3_to_Tcw(ref.se3_mul(a, b))
    assert np.allclose(I, np.eye(4)[:3], atol=1e-15)
    # theta < 1e-5: I + Omega + Omega^2, V = R (se3quat.h:243-249)
    q, t = ref.se3_exp([1e-9, 0, 0, 0, 1.0, 0], OPS)
    assert abs(t[2] - 1e-9) < 1e-24 and t[1] == 1.0 - 1e-18


def test_stereo_jacobian_against_numeric_rule():
    """the analytic Jacobians against g2o's own numeric rule (delta 1e-9, central).  The stereo edge's projection rounds 1 / z to float, so
    its own difference quotient at 1e-9 is 0 or a jump (which is why the edge is analytic): rows 0 and 1 are compared through the
    monocular projection of the same points, row 2 = row 0 - bf d(1 / z) with 1 / z of the perturbed poses in double."""
    P, _ = ref.make_scene(3, n_pts=20, n_lines=0, n_planes=0, noise=0.0, outliers=0.0, mono=0.3)
    G = ref._Edges(P, OPS)
    pose = ref.se3_from_Tcw(P.Tcw)
    J = G.point_jacobian(pose)
    assert G.stereo.sum() > 5 and (~G.stereo).sum() > 2 and np.all(J[~G.stereo, 2] == 0)
    M = ref.Problem(P.cam, P.Tcw, P.kp_xy, -np.ones(20), P.inv_sigma2, None, P.pt_xyz)
    Gm = ref._Edges(M, OPS)
    pp = ref.perturbed(pose, OPS)
    X = lambda p: P.pt_xyz.astype(np.float64) @ ref.quat_to_R(p[0]).T + p[1]
    for d in range(6):
        num = (Gm.errors(pp[2 * d])[0] - Gm.errors(pp[2 * d + 1])[0]) / (2 * ref.DELTA)
        # rounding of the quotient: ~1e-13 of a ~500 px projection over 2e-9
        assert np.allclose(num[:, :2], J[:, :2, d], rtol=0, atol=1e-3), d
        diz = (1.0 / X(pp[2 * d])[:, 2] - 1.0 / X(pp[2 * d + 1])[:, 2]) / (2 * ref.DELTA)
        row2 = num[:, 0] + P.cam[4] * diz                            # error = obs - projection
        assert np.allclose(row2[G.stereo], J[G.stereo, 2, d], rtol=0, atol=1e-3), d


def test_huber_three_values():
    d = ref.f32sqrt(5.991)
    assert ref.huber(1.0, d, d * d) == (1.0, 1.0, 0.0)
    assert ref.huber(d * d, d, d * d) == (d * d, 1.0, 0.0)
    r = ref.huber(16.0, d, d * d)
    assert r == (2 * 4.0 * d - d * d, d / 4.0, -0.5 * (d / 4.0) / 16.0)


def test_plane3d_known_answers():
    assert np.array_equal(ref.plane_normalize([[0, 0, 2, -4]]), [[0, 0, -1, 2]])          # the sign rule: d >= 0
    assert np.array_equal(ref.plane_normalize([[0, 3, 0, 6]]), [[0, 1, 0, 2]])
    p = ref.plane_normalize([[0.3, -0.5, 0.8, 1.5]])
    assert np.allclose(ref.plane_ominus(p, p, OPS), 0, atol=1e-15)
    q = p.copy(); q[:, :3] = -q[:, :3]
    assert np.allclose(ref.plane_ominus_par(q, p, OPS), 0, atol=1e-15)                     # a flipped normal is parallel all the same
    a = ref.plane_normalize([[1.0, 0, 0, 1]]); b = ref.plane_normalize([[0, 1.0, 0, 2]])
    assert np.allclose(ref.plane_ominus_ver(a, b, OPS), 0, atol=1e-15)
    T = ref.plane_transform(np.eye(3), np.array([0.0, 0.0, 1.0]), ref.plane_normalize([[0, 0, 1.0, 2.0]]))
    assert np.array_equal(T, [[0, 0, 1, 1]])                                               # d' = d - t . n


def test_lambda_after_accepted_and_rejected_step():
    """a two-residual quadratic worked by hand: H = diag(2, 8, 1, 1, 1, 1), b = (2, 8, 0, ...): the step is (1, 1) up to lambda, so
    scale = x . (lambda x + b) + 1e-3 = 10.001.  lambda0 = tau * max diagonal = 8e-5.
      chi 2 -> 0: rho = 0.19998, alpha = 1 - (2 rho - 1)^3 = 1.216 -> clamped to 2/3: lambda = lambda0 * 2/3
      chi 10 -> 0: rho = 0.9999, alpha = 6e-4 -> raised to 1/3: lambda = lambda0 / 3
      chi 2 -> 5, 5, 1: two rejections multiply lambda by ni = 2, then 4 (ni ends at 8), the third trial is accepted and resets ni to 2."""
    H = np.diag([2.0, 8.0, 1, 1, 1, 1]); b = np.array([2.0, 8.0, 0, 0, 0, 0])
    pose = ref.se3_from_Tcw(np.eye(4)[:3])
    lm = ref.Levenberg(lambda p: (H, b, 2.0), lambda p: 0.0, OPS)
    lm.solve(0, pose)
    assert lm.lam == 8e-5 * (2.0 / 3.0) and lm.ni == 2.0 and lm.trials == 1
    lm = ref.Levenberg(lambda p: (H, b, 10.0), lambda p: 0.0, OPS)
    lm.solve(0, pose)
    assert lm.lam == 8e-5 * (1.0 / 3.0)
    chis = iter([5.0, 5.0, 1.0])
    lm2 = ref.Levenberg(lambda p: (H, b, 2.0), lambda p: next(chis), OPS)
    lm2.solve(0, pose)
    assert lm2.trials == 3 and lm2.ni == 2.0 and lm2.chi == 1.0
    lam3 = 8e-5 * 2 * 4
    x = np.array([2 / (2 + lam3), 8 / (8 + lam3)])
    rho = (2.0 - 1.0) / (x[0] * (lam3 * x[0] + 2) + x[1] * (lam3 * x[1] + 8) + 1e-3)
    assert np.isclose(lm2.lam, lam3 * max(1 / 3.0, min(2 / 3.0, 1 - (2 * rho - 1) ** 3)), rtol=1e-12)


def test_noise_free_scene_returns_true_pose():
    """measured: 2.4e-7 at most over these seeds (float32 map points and key points, the 1e-9 difference quotient); asserted with a margin of 4"""
    worst = 0.0
    for seed in (5, 6, 7):
        P, T = ref.make_scene(seed, noise=0.0, outliers=0.0)
        r = ref.pose_optimization(P)
        worst = max(worst, float(np.abs(r.Tcw - T).max()))
        assert r.n_bad == 0 and r.n_line_bad == 0 and r.ret == r.n_initial
    print("noise-free: largest pose error %.3e" % worst)
    assert worst < 1e-6


def test_gross_outliers_flagged_and_pose_recovered():
    P, T = ref.make_scene(1002)
    r = ref.pose_optimization(P)
    assert r.pt_outlier.sum() > 10 and r.ln_outlier.sum() > 0 and r.pl_outlier.sum() > 0
    assert np.abs(r.Tcw - T).max() < 2e-3 < np.abs(P.Tcw - T).max()
    assert r.ret == r.n_initial - r.n_bad - r.n_line_bad


def test_round0_outlier_can_return():
    """30 % of the points carry one consistent 10 px shift (a second motion).  Round 0 ends between the two populations and flags points of
    both; once the minority is out of the graph the pose moves to the majority, whose flagged points are recomputed and are inliers again."""
    P, T = ref.make_scene(1002, outliers=0.0, n_pts=200, n_lines=0, n_planes=0, noise=0.3)
    n = len(P.kp_xy); k = int(0.3 * n)
    P.kp_xy[:k, 0] += 10; P.uright[:k] = np.where(P.uright[:k] < 0, -1, P.uright[:k] + 10)
    r = ref.pose_optimization(P)
    first = r.round_chi2[0][:n] > np.where(P.uright < 0, 5.991, 7.815)
    back = first & (r.pt_outlier == 0)
    print("flagged after round 0: %d, of them inliers at the end: %d" % (first.sum(), back.sum()))
    assert back.sum() >= 1 and not back[:k].any() and r.pt_outlier[:k].all()


def test_line_with_one_bad_end_is_no_outlier():
    P, _ = ref.make_scene(1003, outliers=0.0)
    P.ln_xyz[0, 3:] += 0.5                                        # the end point leaves the line, the start point stays on it
    r = ref.pose_optimization(P)
    n = len(P.kp_xy)
    assert r.round_chi2[-1][n + 1] > 3.84 and r.round_chi2[-1][n] <= 3.84 and r.ln_outlier[0] == 0


def test_fewer_than_three_correspondences():
    P, _ = ref.make_scene(1004, n_planes=0)
    P.pt_has[2:] = 0
    r = ref.pose_optimization(P)
    assert r.ret == 0 and r.n_initial == 2 and np.array_equal(r.Tcw, P.Tcw.astype(np.float64)) and r.rounds == 0


def test_vanishing_direction_skip_rules():
    P, _ = ref.make_scene(1005, n_lines=4)
    P.l3d_B[0, 1] = P.l3d_A[0, 1]                                 # one zero component of the frame's direction (Optimizer.cc:827)
    P.ln_xyz[1, 5] = P.ln_xyz[1, 2]                               # one zero component of the map line's direction (:853)
    G = ref._Edges(P, OPS)
    assert list(G.present[G.o_vp:G.o_pl]) == [False, False, True, True]
    assert G.present[G.o_ln:G.o_vp].all()                         # the end-point edges stay


def test_early_return_contributes_nothing_and_is_flagged():
    P, r = ref.crafted_early_return()
    assert r.vp_outlier[0] == 1 and r.n_bad == 0 and r.n_line_bad == 0 and r.ret == 8
    assert all(c[-1] == 0 for c in r.round_chi2)


def test_tree_order_and_ulp_model_keep_decisions():
    sc, gen = ref.accepted_scenes(3)
    D = ref.measured_D(sc)
    print("generated %d, D = %.3e" % (gen, D))
    assert 0 < D < 1e-5
    for P, R, _ in sc:
        b = ref.pose_optimization(P, ref.Ops("tree", 7))
        assert np.array_equal(b.pt_outlier, R.pt_outlier) and b.ret == R.ret


def test_entry_points_declared_exported_and_bound(hvo):
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    L = hvo.lib()
    for sym in ("hvo_pose_optimize", "hvo_stream_pose_optimize", "hvo_batch_pose_optimize", "hvo_pose_last_kernel_ms", "hvo_stream_pose_last_kernel_ms"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert hasattr(L, sym), sym
    # sizes of the C structs as include/hvo.h lays them out on LP64
    assert ctypes.sizeof(hvo.PoseResult) == 12 * 8 + 12 * 4 + 6 * 4 + 8 * 4 + 2 * 4 + 8 * 8 == 272
    assert ctypes.sizeof(hvo.PoseProblem) == 12 * 4 + 4 * 4 + 16 * 8 == 192
    assert ctypes.sizeof(hvo.PoseFlags) == 32 and ctypes.sizeof(hvo.PosePlaneParams) == 48
    assert "to_dict" in dir(hvo.PoseResult)
