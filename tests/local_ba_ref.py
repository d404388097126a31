"""CPU restatement (numpy float64) of Optimizer::LocalMapOptimization (reference src/Optimizer.cc:3014-3940) and a deterministic window
generator.  g2o cannot be built here (no Eigen), so tests/test_local_ba.py pins this file by known answers and csrc/local_ba.hip is tested
against it.

What is restated, with the files it was written from:
  graph          Optimizer.cc:3169-3639: one SE3 vertex per key frame (fixed iff mnId == 0, outside observers fixed), one XYZ vertex per
                 point, two per line; a line is skipped whole on a NaN or |x_end - x_start| < 1e-5 (:3358-3366); par / perp entries are
                 skipped on idx < 0, linefn[0] == 0.0 or -1.0, or a NaN (:3484-3501)
  edges          EdgeSE3ProjectXYZ (Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:80-109, analytic Jacobian .cpp:103-139),
                 DistPt2Line2DMultiFrame (include/g2oMSC.h:561-610), ParEptsNVector3DSingleFrame (:123-169), ParEptsNVector2DMultiFrame
                 (:443-500), PerpEptsNVector2DMultiFrame (:502-559), ComputeAngle2D / ComputeAngle3D (:11-34)
  Jacobians      g2o's numeric rule for every line edge: central differences, delta 1e-9, per non-fixed vertex, times 1 / (2 delta)
                 (core/base_binary_edge.hpp:147, core/base_multi_edge.hpp:72)
  quadratic form core/base_binary_edge.hpp constructQuadraticForm with RobustKernelHuber::robustify (pose_opt_ref.huber_v)
  Levenberg      core/optimization_algorithm_levenberg.cpp:61-189 (lambda's start, computeScale, rho, the 1/3 rule, ni, ten trials, the
                 nBad stop), SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-421); terminate() is polled before an iteration
                 (:376) and after a trial (levenberg.cpp:149), the reference polls at Optimizer.cc:3641 and :3650
  rounds         optimize(5), the classification of :3656-3743 (kernels removed, outliers to level 1; the Manhattan edges are not
                 touched and keep their kernel), initializeOptimization(0), optimize(10), the erase tests of :3753-3847
  write-back     :3903-3939 through Converter::toCvMat (float)

The formulation: no edge joins two different lines, so a line's (start, end) pair is ONE 6-dimensional landmark beside the 3-dimensional
points.  Every landmark block (plus lambda) is eliminated; the dense reduced system over the free key frames is factored by LDL^T without
pivoting ("not positive" = a pivot <= 0).  tests/test_local_ba.py compares that step with numpy.linalg.solve on the full system.

The readings (include/hvo.h), each a switch of `local_map_optimization` so that a test can show what it changes:
  1 end_cam_current    the END-point edge and the par / perp edges take fx fy cx cy of key frame 0, the start edge its observer's
  2 stored_error       chi2() is read from the error an edge HOLDS: a level-1 edge is never evaluated again, its erase test reads round
                       1's last evaluation (the last trial, accepted or not); isDepthPositive() is evaluated at the final estimate
  3 final_start_twice  the erase test of a line observation reads its START edge twice; the classification reads start or end
  4 walk_erased(pairing="as_written") pairs the erased line observation i with the key frame of observation i // 2 in global push order
  5 manh_erase is a flag per line; the walk never erases a Manhattan observation (vpLineManhKF is never filled)
  6 zero points or zero lines are ordinary inputs;  7 a key-frame index outside the list is refused;  8 isBad() reads as false.
SE3Quat::map is the quaternion's rotation matrix applied to the point, as in pose_opt_ref.py, which is imported, not edited."""
import numpy as np

import pose_opt_ref as po
from pose_opt_ref import Ops, se3_exp, se3_mul, se3_from_Tcw, se3_to_Tcw, quat_to_R, huber_v, f32sqrt, rot_vec, F32, DELTA

PT, START, END, MANH, PAR, PERP = range(6)
LIMITS = dict(free_kf=64, kf=1024, points=65536, lines=16384, pt_obs=1 << 20, ln_obs=1 << 18, struct=1 << 18)
OPTIMISED, NOTHING, STOPPED = 0, 1, 2
CAM = (535.4, 539.2, 320.1, 247.6)


def default_params():
    return dict(iterations=(5, 10), max_trials=10, stop_at_poll=-1, huber_delta=(f32sqrt(5.991), f32sqrt(3.84), f32sqrt(0.08)),
                chi2_gate=(5.991, 3.84, 0.13), inv_sigma=(0.3, 0.3, 0.5))


class Window:
    """one call's input in the C ABI's arrays and types (include/hvo.h hvo_local_ba_graph)"""
    FIELDS = (("Tcw", F32, (-1, 3, 4)), ("fixed", np.uint8, (-1,)), ("cam", F32, (-1, 4)), ("pt_pos", F32, (-1, 3)),
              ("pt_obs_start", np.int32, (-1,)), ("pt_obs_kf", np.int32, (-1,)), ("pt_obs_uv", F32, (-1, 2)), ("pt_obs_inv_sigma2", F32, (-1,)),
              ("ln_pos", np.float64, (-1, 6)), ("ln_manh_idx", np.int32, (-1,)), ("ln_obs_start", np.int32, (-1,)), ("ln_obs_kf", np.int32, (-1,)),
              ("ln_obs_fn", np.float64, (-1, 3)), ("par_start", np.int32, (-1,)), ("par_kf", np.int32, (-1,)), ("par_idx", np.int32, (-1,)),
              ("par_fn", np.float64, (-1, 3)), ("par_map_size", np.int32, (-1,)), ("perp_start", np.int32, (-1,)), ("perp_kf", np.int32, (-1,)),
              ("perp_idx", np.int32, (-1,)), ("perp_fn", np.float64, (-1, 3)), ("perp_map_size", np.int32, (-1,)))

    def __init__(self, **kw):
        n_kf = len(kw["Tcw"]); n_pts = len(kw.get("pt_pos", ())); n_ln = len(kw.get("ln_pos", ()))
        zeros = dict(pt_obs_start=n_pts + 1, ln_obs_start=n_ln + 1, par_start=n_ln + 1, perp_start=n_ln + 1, ln_manh_idx=n_ln, par_map_size=n_ln,
                     perp_map_size=n_ln, fixed=n_kf)
        for name, dt, shape in self.FIELDS:
            v = kw.get(name)
            if v is None:
                v = np.zeros(zeros.get(name, 0), dt)
            setattr(self, name, np.ascontiguousarray(np.asarray(v, dt).reshape(shape)))
        self.manh_axis = np.ascontiguousarray(np.asarray(kw.get("manh_axis", np.eye(3)), np.float64).reshape(3, 3))
        self.manh_available = int(kw.get("manh_available", 0))
        self.n_kf, self.n_points, self.n_lines = n_kf, n_pts, n_ln

    def as_dict(self):
        d = {name: getattr(self, name) for name, _, _ in self.FIELDS}
        d.update(manh_axis=self.manh_axis, manh_available=self.manh_available)
        return d

    def copy(self, **changes):
        d = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in self.as_dict().items()}
        d.update(changes)
        return Window(**d)


class Refused(ValueError):
    pass


def check_limits(G):
    """the refusals of the C ABI, in its order; raises Refused with the reason"""
    def no(why): raise Refused(why)
    if G.n_kf > LIMITS["kf"]: no("more than 1024 key frames")
    if G.n_points > LIMITS["points"]: no("more than 65536 points")
    if G.n_lines > LIMITS["lines"]: no("more than 16384 lines")
    if len(G.pt_obs_kf) > LIMITS["pt_obs"]: no("more than 2^20 point observations")
    if len(G.ln_obs_kf) > LIMITS["ln_obs"]: no("more than 2^18 line observations")
    if len(G.par_kf) + len(G.perp_kf) > LIMITS["struct"]: no("more than 2^18 par plus perp entries")
    if int((G.fixed == 0).sum()) > LIMITS["free_kf"]: no("more than 64 free key frames")
    for kf in (G.pt_obs_kf, G.ln_obs_kf, G.par_kf, G.perp_kf):
        if len(kf) and (kf.min() < 0 or kf.max() >= G.n_kf): no("a key-frame index outside the call's list")
    for start, kf, what in ((G.pt_obs_start, G.pt_obs_kf, "point"), (G.ln_obs_start, G.ln_obs_kf, "line")):
        if len(kf):
            owner = np.repeat(np.arange(len(start) - 1), np.diff(start))
            key = owner.astype(np.int64) * G.n_kf + kf
            if len(np.unique(key)) != len(key): no("a key frame observes one %s twice" % what)


class _Graph:
    """the edges in g2o's insertion order: per point its observations; per made line the Manhattan edge, (start, end) per observation,
    the par entries, the perp entries"""
    def __init__(self, G, prm, end_cam_current=True):
        self.G = G
        nkf, npts = G.n_kf, G.n_points
        self.free_kf = np.flatnonzero(G.fixed == 0); self.nf = len(self.free_kf)
        self.kf_free = -np.ones(nkf, int); self.kf_free[self.free_kf] = np.arange(self.nf)
        cam = G.cam.astype(np.float64); cam0 = cam[0] if nkf else np.zeros(4)
        kind, lm, kf, m, info, delta, ecam, src = [], [], [], [], [], [], [], []

        def add(k, l, f, mm, i, d, c, s):
            kind.append(k); lm.append(l); kf.append(f); m.append(mm); info.append(i); delta.append(d); ecam.append(c); src.append(s)
            return len(kind) - 1
        hd = prm["huber_delta"]; isg = prm["inv_sigma"]
        self.pt_edge = -np.ones(len(G.pt_obs_kf), int)
        for i in range(npts):
            for o in range(G.pt_obs_start[i], G.pt_obs_start[i + 1]):
                k = int(G.pt_obs_kf[o])
                self.pt_edge[o] = add(PT, i, k, [float(G.pt_obs_uv[o, 0]), float(G.pt_obs_uv[o, 1]), 0.0], float(G.pt_obs_inv_sigma2[o]), hd[0], cam[k], o)
        self.line_made = np.zeros(G.n_lines, np.uint8); self.lm_line = [-1] * npts
        self.ln_start_edge = -np.ones(len(G.ln_obs_kf), int); self.ln_end_edge = -np.ones(len(G.ln_obs_kf), int)
        self.par_edge = -np.ones(len(G.par_kf), int); self.perp_edge = -np.ones(len(G.perp_kf), int); self.manh_edge = -np.ones(G.n_lines, int)
        self.push_kf = []                                                     # vpLineEdgeKF: two entries per observation, in push order
        self.push_obs = []                                                    # vpMapLineEdge / vpLineEdgesSP: one entry per observation
        for i in range(G.n_lines):
            X = G.ln_pos[i]
            if np.isnan(X).any() or abs(X[3] - X[0]) < 0.00001:
                continue
            self.line_made[i] = 1; l = len(self.lm_line); self.lm_line.append(i)
            a = int(G.ln_manh_idx[i])
            if G.manh_available and 0 < a <= 3:
                self.manh_edge[i] = add(MANH, l, -1, list(G.manh_axis[:, a - 1]), isg[1], hd[2], cam0, i)
            for o in range(G.ln_obs_start[i], G.ln_obs_start[i + 1]):
                k = int(G.ln_obs_kf[o])
                self.ln_start_edge[o] = add(START, l, k, list(G.ln_obs_fn[o]), isg[0], hd[1], cam[k], o)
                self.ln_end_edge[o] = add(END, l, k, list(G.ln_obs_fn[o]), isg[0], hd[1], cam0 if end_cam_current else cam[k], o)
                self.push_kf += [k, k]; self.push_obs.append(o)
            for which, st, kfv, idx, fn, size, out in ((PAR, G.par_start, G.par_kf, G.par_idx, G.par_fn, G.par_map_size, self.par_edge),
                                                       (PERP, G.perp_start, G.perp_kf, G.perp_idx, G.perp_fn, G.perp_map_size, self.perp_edge)):
                for o in range(st[i], st[i + 1]):
                    ln = fn[o]
                    if idx[o] < 0 or ln[0] == 0.0 or ln[0] == -1.0 or np.isnan(ln).any():
                        continue
                    k = int(kfv[o])
                    out[o] = add(which, l, k, list(ln), isg[2] + int(size[i]) / 10.0, hd[2], cam0 if end_cam_current else cam[k], o)
        self.nlm = len(self.lm_line); self.E = len(kind)
        self.kind = np.array(kind, int); self.lm = np.array(lm, int); self.kf = np.array(kf, int)
        self.m = np.array(m, np.float64).reshape(-1, 3); self.info = np.array(info, np.float64); self.delta = np.array(delta, np.float64)
        self.cam = np.array(ecam, np.float64).reshape(-1, 4); self.src = np.array(src, int)
        self.kfi = np.maximum(self.kf, 0)
        self.ef = np.where(self.kf >= 0, self.kf_free[self.kfi], -1)                 # the edge's free key frame or -1
        self.dim = np.array([3] * npts + [6] * (self.nlm - npts), int)
        self.is_pt = self.kind == PT
        lm0 = np.zeros((self.nlm, 6)); lm0[:npts, :3] = G.pt_pos.astype(np.float64)
        for l in range(npts, self.nlm): lm0[l] = G.ln_pos[self.lm_line[l]]
        self.lm0 = lm0
        self.pose0 = [se3_from_Tcw(G.Tcw[k]) for k in range(nkf)]
        self.counts = [int((self.kind == k).sum()) for k in range(6)]

    # ---- computeError, vectorised over the edges; R (E x 3 x 3), t (E x 3) the observer's pose per edge, X (E x 6) its landmark
    @staticmethod
    def _map(R, t, X):
        return np.stack([((R[:, i, 0] * X[:, 0] + R[:, i, 1] * X[:, 1]) + R[:, i, 2] * X[:, 2]) + t[:, i] for i in range(3)], axis=1)

    def _project(self, R, t, X):
        Y = self._map(R, t, X)
        return np.stack([Y[:, 0] / Y[:, 2] * self.cam[:, 0] + self.cam[:, 2], Y[:, 1] / Y[:, 2] * self.cam[:, 1] + self.cam[:, 3]], axis=1)

    def errors(self, R, t, X):
        m, k = self.m, self.kind
        err = np.zeros((self.E, 2))
        with np.errstate(invalid="ignore", divide="ignore"):
            ps = self._project(R, t, X[:, :3]); pe = self._project(R, t, X[:, 3:])
            e_pt = m[:, :2] - ps
            e_s = (m[:, 0] * ps[:, 0] + m[:, 1] * ps[:, 1]) + m[:, 2]
            e_e = (m[:, 0] * pe[:, 0] + m[:, 1] * pe[:, 1]) + m[:, 2]
            d = X[:, 3:] - X[:, :3]
            dot = (m[:, 0] * d[:, 0] + m[:, 1] * d[:, 1]) + m[:, 2] * d[:, 2]
            ma = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]); mb = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            e_m = 1 - np.abs(dot / (ma * mb))
            lb = pe - ps; la0 = m[:, 0] / m[:, 2]; la1 = m[:, 1] / m[:, 2]
            dot2 = lb[:, 0] * la0 + lb[:, 1] * la1
            ang = np.abs(dot2 / (np.sqrt(lb[:, 0] * lb[:, 0] + lb[:, 1] * lb[:, 1]) * np.sqrt(la0 * la0 + la1 * la1)))
        err[:, 0] = np.select([k == PT, k == START, k == END, k == MANH, k == PAR], [e_pt[:, 0], e_s, e_e, e_m, 1 - ang], ang)
        err[:, 1] = np.where(k == PT, e_pt[:, 1], 0.0)
        return err

    def chi2(self, err):
        return self.info * err[:, 0] * err[:, 0] + self.info * err[:, 1] * err[:, 1]

    def gather(self, poses, lm):
        Rk = np.array([quat_to_R(p[0]) for p in poses]).reshape(-1, 3, 3); tk = np.array([p[1] for p in poses]).reshape(-1, 3)
        return Rk[self.kfi], tk[self.kfi], lm[self.lm]

    def point_jacobians(self, R, t, X):
        """EdgeSE3ProjectXYZ::linearizeOplus for every edge (used where kind == PT): (E x 2 x 6 landmark, E x 2 x 6 pose)"""
        Y = self._map(R, t, X[:, :3])
        fx, fy = self.cam[:, 0], self.cam[:, 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            x, y, z = Y[:, 0], Y[:, 1], Y[:, 2]; z_2 = z * z; c = -1. / z
            t0 = np.stack([c * fx, c * 0.0, c * (-x / z * fx)], axis=1); t1 = np.stack([c * 0.0, c * fy, c * (-y / z * fy)], axis=1)
            Jl = np.zeros((self.E, 2, 6)); Jp = np.zeros((self.E, 2, 6))
            for j in range(3):
                Jl[:, 0, j] = (t0[:, 0] * R[:, 0, j] + t0[:, 1] * R[:, 1, j]) + t0[:, 2] * R[:, 2, j]
                Jl[:, 1, j] = (t1[:, 0] * R[:, 0, j] + t1[:, 1] * R[:, 1, j]) + t1[:, 2] * R[:, 2, j]
            Jp[:, 0, 0] = x * y / z_2 * fx; Jp[:, 0, 1] = -(1 + (x * x / z_2)) * fx; Jp[:, 0, 2] = y / z * fx; Jp[:, 0, 3] = -1. / z * fx; Jp[:, 0, 5] = x / z_2 * fx
            Jp[:, 1, 0] = (1 + y * y / z_2) * fy; Jp[:, 1, 1] = -x * y / z_2 * fy; Jp[:, 1, 2] = -x / z * fy; Jp[:, 1, 4] = -1. / z * fy; Jp[:, 1, 5] = y / z_2 * fy
        return Jl, Jp

    def numeric_jacobians(self, poses, lm, ops):
        """g2o's numeric rule for every edge: landmark columns, and pose columns where the observer is free"""
        R, t, X = self.gather(poses, lm)
        scalar = 1.0 / (2 * DELTA)
        Jl = np.zeros((self.E, 2, 6)); Jp = np.zeros((self.E, 2, 6))
        for d in range(6):
            Xa = X.copy(); Xa[:, d] = X[:, d] + DELTA; Xb = X.copy(); Xb[:, d] = X[:, d] + (-DELTA)
            Jl[:, :, d] = scalar * (self.errors(R, t, Xa) - self.errors(R, t, Xb))
        Jl[self.is_pt, :, 3:] = 0.0
        for d in range(6):
            pa, pb = list(poses), list(poses)
            for k in self.free_kf:
                u = np.zeros(6); u[d] = DELTA; pa[k] = se3_mul(se3_exp(u, ops), poses[k])
                u = np.zeros(6); u[d] = -DELTA; pb[k] = se3_mul(se3_exp(u, ops), poses[k])
            Ra, ta, _ = self.gather(pa, lm); Rb, tb, _ = self.gather(pb, lm)
            Jp[:, :, d] = scalar * (self.errors(Ra, ta, X) - self.errors(Rb, tb, X))
        Jp[self.ef < 0] = 0.0
        return Jl, Jp

    def jacobians(self, poses, lm, ops):
        R, t, X = self.gather(poses, lm)
        Jl, Jp = self.numeric_jacobians(poses, lm, ops)
        Al, Ap = self.point_jacobians(R, t, X)
        Jl[self.is_pt] = Al[self.is_pt]; Jp[self.is_pt] = Ap[self.is_pt]
        Jp[self.ef < 0] = 0.0
        return Jl, Jp


def ldlt_dense(S, b):
    """x of S x = b by LDL^T without pivoting, right-looking and column by column as the one-workgroup kernel does it; ok = every pivot > 0"""
    S = np.array(S, np.float64); n = len(b); ok = True
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(n):
            d = S[j, j]
            if not (d > 0): ok = False
            raw = S[j + 1:, j].copy(); l = raw / d
            S[j + 1:, j + 1:] = S[j + 1:, j + 1:] - l[:, None] * raw[None, :]
            S[j + 1:, j] = l
        y = np.array(b, np.float64)
        for j in range(n):
            y[j + 1:] = y[j + 1:] - S[j + 1:, j] * y[j]
        y = y / np.diag(S)
        for j in range(n - 1, -1, -1):
            y[:j] = y[:j] - S[j, :j] * y[j]
    return y, ok


def _inv_ldlt(H, dim):
    """(L x 6 x 6) inverses of the leading dim x dim blocks by LDL^T without pivoting, column by column"""
    n = len(H); out = np.zeros((n, 6, 6))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for dd in (3, 6):
            sel = np.flatnonzero(dim == dd)
            if not len(sel): continue
            A = H[sel]; L = np.zeros((len(sel), 6, 6)); D = np.zeros((len(sel), 6))
            for j in range(dd):
                s = A[:, j, j].copy()
                for k in range(j): s = s - L[:, j, k] * L[:, j, k] * D[:, k]
                D[:, j] = s
                for i in range(j + 1, dd):
                    s2 = A[:, i, j].copy()
                    for k in range(j): s2 = s2 - L[:, i, k] * L[:, j, k] * D[:, k]
                    L[:, i, j] = s2 / D[:, j]
            inv = np.zeros((len(sel), 6, 6))
            for c in range(dd):
                y = np.zeros((len(sel), 6)); x = np.zeros((len(sel), 6))
                for i in range(dd):
                    s = np.full(len(sel), 1.0 if i == c else 0.0)
                    for k in range(i): s = s - L[:, i, k] * y[:, k]
                    y[:, i] = s
                for i in range(dd - 1, -1, -1):
                    s = y[:, i] / D[:, i]
                    for k in range(i + 1, dd): s = s - L[:, k, i] * x[:, k]
                    x[:, i] = s
                inv[:, :dd, c] = x[:, :dd]
            out[sel] = inv
    return out


class Linearisation:
    """the blocks of one linearisation: Hpp (nf x 6 x 6), bp, Hll (L x 6 x 6), bl, Hpl (nf x L x 6 x 6), chi2 and the vertices' activity"""
    def __init__(self, g, poses, lm, active, robust, ops):
        self.g = g
        R, t, X = g.gather(poses, lm)
        err = g.errors(R, t, X); chi = g.chi2(err)
        use = robust | (g.kind == MANH)
        r0, r1 = huber_v(chi, g.delta, g.delta * g.delta)
        r0 = np.where(use, r0, chi); r1 = np.where(use, r1, 1.0)
        self.chi_edges = chi
        self.rho = np.where(active, r0, 0.0)
        Jl, Jp = g.jacobians(poses, lm, ops)
        Jl[~active] = 0.0; Jp[~active] = 0.0
        self.Jl, self.Jp = Jl, Jp
        w = np.where(active, r1 * g.info, 0.0); we = g.info[:, None] * err; r1a = np.where(active, r1, 0.0)

        def quad(Ja, Jb):
            return (Ja[:, 0, :, None] * w[:, None, None]) * Jb[:, 0, None, :] + (Ja[:, 1, :, None] * w[:, None, None]) * Jb[:, 1, None, :]

        def grad(Ja):
            return -(r1a[:, None] * (Ja[:, 0] * we[:, 0:1] + Ja[:, 1] * we[:, 1:2]))
        order = np.arange(g.E) if ops.order == "seq" else np.arange(g.E)[::-1]       # tree: another fixed order of the same terms
        nf, L = g.nf, g.nlm
        self.Hll = np.zeros((L, 6, 6)); self.bl = np.zeros((L, 6)); self.Hpp = np.zeros((nf, 6, 6)); self.bp = np.zeros((nf, 6)); self.Hpl = np.zeros((nf, L, 6, 6))
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(self.Hll, g.lm[order], quad(Jl, Jl)[order]); np.add.at(self.bl, g.lm[order], grad(Jl)[order])
            pe = order[(g.ef[order] >= 0) & active[order]]
            np.add.at(self.Hpp, g.ef[pe], quad(Jp, Jp)[pe]); np.add.at(self.bp, g.ef[pe], grad(Jp)[pe])
            np.add.at(self.Hpl, (g.ef[pe], g.lm[pe]), quad(Jp, Jl)[pe])
        self.lm_act = np.zeros(L, bool); self.lm_act[g.lm[active]] = True
        self.kf_act = np.zeros(nf, bool); self.kf_act[g.ef[active & (g.ef >= 0)]] = True
        self.chi = float(ops.sum0(self.rho))
        dl = np.abs(np.einsum("lii->li", self.Hll)); dp = np.abs(np.einsum("lii->li", self.Hpp))
        self.max_diag = float(max(dl[self.lm_act].max() if self.lm_act.any() else 0.0, dp[self.kf_act].max() if self.kf_act.any() else 0.0, 0.0))

    def step(self, lam, ops):
        """(dx nf x 6, dl L x 6, ok, scale) of (H + lambda I) x = b with every landmark eliminated"""
        g = self.g; nf, L = g.nf, g.nlm; n6 = 6 * nf
        H = self.Hll.copy()
        for d in range(6):
            H[:, d, d] = np.where(d < g.dim, H[:, d, d] + lam, 1.0)
        H[~self.lm_act] = np.eye(6)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if ops.order == "seq":
                Hinv = np.zeros((L, 6, 6))
                for dd in (3, 6):
                    sel = np.flatnonzero(g.dim == dd)
                    if len(sel):
                        try:
                            Hinv[sel[:, None, None], np.arange(dd)[None, :, None], np.arange(dd)[None, None, :]] = np.linalg.inv(H[sel][:, :dd, :dd])
                        except np.linalg.LinAlgError:
                            Hinv[sel] = _inv_ldlt(H[sel], g.dim[sel])
            else:
                Hinv = _inv_ldlt(H, g.dim)
            Hinv[~self.lm_act] = 0.0
            Y = np.einsum("flab,lbc->flac", self.Hpl, Hinv)
            Yr = Y.transpose(0, 2, 1, 3).reshape(n6, L * 6); Wr = self.Hpl.transpose(0, 2, 1, 3).reshape(n6, L * 6)
            S = -(Yr @ Wr.T)
            rhs = self.bp.reshape(-1) - Yr @ self.bl.reshape(-1)
            for f in range(nf):
                s = slice(6 * f, 6 * f + 6)
                if self.kf_act[f]:
                    S[s, s] = self.Hpp[f] + S[s, s] + lam * np.eye(6)
                else:
                    S[s, s] = np.eye(6); rhs[s] = 0.0
            dx, ok = ldlt_dense(S, rhs)
            v = self.bl.reshape(-1) - Wr.T @ dx
            dl = np.einsum("lab,lb->la", Hinv, v.reshape(L, 6))
            dl[~self.lm_act] = 0.0
            for d in range(6): dl[g.dim <= d, d] = 0.0
            dx = dx.reshape(nf, 6); dx[~self.kf_act] = 0.0
            terms = np.concatenate([(dl * (lam * dl + self.bl)).sum(axis=1), (dx * (lam * dx + self.bp)).sum(axis=1)])
            scale = float(ops.sum0(terms))
        return dx, dl, ok, scale

    def full_system(self):
        """the dense Hessian and gradient over (free key frames, landmarks) for numpy.linalg.solve; the landmarks' unused and inactive
        dimensions are left out.  Returns (H, b, index of every kept landmark coordinate)"""
        g = self.g; nf, L = g.nf, g.nlm; n6 = 6 * nf
        keep = np.array([[self.lm_act[l] and d < g.dim[l] for d in range(6)] for l in range(L)]).reshape(-1)
        idx = np.flatnonzero(keep); n = n6 + len(idx)
        H = np.zeros((n, n)); b = np.zeros(n)
        for f in range(nf): H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = self.Hpp[f]
        b[:n6] = self.bp.reshape(-1)
        Hll = np.zeros((L * 6, L * 6))
        for l in range(L): Hll[6 * l:6 * l + 6, 6 * l:6 * l + 6] = self.Hll[l]
        H[n6:, n6:] = Hll[np.ix_(idx, idx)]
        Wr = self.Hpl.transpose(0, 2, 1, 3).reshape(n6, L * 6)[:, idx]
        H[:n6, n6:] = Wr; H[n6:, :n6] = Wr.T
        b[n6:] = self.bl.reshape(-1)[idx]
        return H, b, idx


class Result:
    pass


def local_map_optimization(G, params=None, ops=None, end_cam_current=True, stored_error=True, final_start_twice=True):
    """the whole call.  params: default_params() with changes; params["stop_at_poll"] = k makes the k-th poll (0-based) and every
    later one read "stop".  Raises Refused where the C ABI returns HVO_ERR_UNSUPPORTED."""
    prm = default_params(); prm.update(params or {})
    ops = ops or Ops()
    check_limits(G)
    g = _Graph(G, prm, end_cam_current)
    res = Result(); res.graph = g
    res.line_made = g.line_made.copy(); res.par_made = (g.par_edge >= 0).astype(np.uint8); res.perp_made = (g.perp_edge >= 0).astype(np.uint8)
    res.pt_erase = np.zeros(len(G.pt_obs_kf), np.uint8); res.ln_erase = np.zeros(len(G.ln_obs_kf), np.uint8); res.manh_erase = np.zeros(G.n_lines, np.uint8)
    res.par_erase = np.zeros(len(G.par_kf), np.uint8); res.perp_erase = np.zeros(len(G.perp_kf), np.uint8)
    res.iterations = [0, 0]; res.trials = [0, 0]; res.lam = [0.0, 0.0]; res.chi2 = [0.0, 0.0]; res.rounds = 0; res.stopped_at = -1
    res.n_free_kf = g.nf; res.n_pt_edges, res.n_line_obs, _, res.n_manh_edges, res.n_par_edges, res.n_perp_edges = g.counts
    res.n_lines_made = g.nlm - G.n_points
    res.round_chi2 = []; res.steps = []; res.margins = []

    def inputs():
        res.Tcw_d = G.Tcw.astype(np.float64); res.Tcw_f = G.Tcw.copy(); res.pt_d = G.pt_pos.astype(np.float64); res.pt_f = G.pt_pos.copy()
        res.ln_d = G.ln_pos.copy(); res.ln_f = G.ln_pos.astype(F32)
    if g.nf == 0 or g.E == 0:
        inputs(); res.status = NOTHING; return res
    polls = [0, -1]

    def poll():
        k = polls[0]; polls[0] += 1
        s = prm["stop_at_poll"] >= 0 and k >= prm["stop_at_poll"]
        if s and polls[1] < 0: polls[1] = k
        return s
    if poll():
        inputs(); res.stopped_at = polls[1]; res.status = STOPPED; return res
    poses, lm = list(g.pose0), g.lm0.copy()
    level = np.zeros(g.E, bool); held = np.zeros(g.E)                               # the chi2 of the error each edge holds
    gate = np.array(prm["chi2_gate"])[[0, 1, 1, 2, 2, 2]][g.kind]

    def evaluate(ps, l, active, robust):
        R, t, X = g.gather(ps, l)
        chi = g.chi2(g.errors(R, t, X))
        held[active] = chi[active]
        use = robust | (g.kind == MANH)
        r0 = np.where(use, huber_v(chi, g.delta, g.delta * g.delta)[0], chi)
        return float(ops.sum0(np.where(active, r0, 0.0)))

    def depth_positive(ps, l):
        R, t, X = g.gather(ps, l)
        return g._map(R, t, X[:, :3])[:, 2] > 0.0
    for rnd in range(2):
        active = ~level; robust = rnd == 0
        lam, ni, cur, nbad, its, trials, ok = 0.0, 2.0, 0.0, 0, 0, 0, True
        it = 0
        while active.any() and it < prm["iterations"][rnd]:
            if poll(): break
            if not ok: break
            lin = Linearisation(g, poses, lm, active, robust, ops)
            held[active] = lin.chi_edges[active]
            cur = lin.chi; ini = cur
            if it == 0: lam = 1e-5 * lin.max_diag; ni = 2.0; nbad = 0
            rho = 0.0; q = 0
            while True:
                dx, dl, ok2, scale = lin.step(lam, ops)
                tp = list(poses)
                for f, k in enumerate(g.free_kf):
                    if lin.kf_act[f]: tp[k] = se3_mul(se3_exp(dx[f], ops), poses[k])
                tl = lm + dl
                tmp = evaluate(tp, tl, active, robust); trials += 1
                if not ok2: tmp = np.finfo(np.float64).max
                rho = (cur - tmp) / (scale + 1e-3)
                res.steps.append((cur - tmp) / cur if cur > 0 else 0.0)
                if rho > 0 and np.isfinite(tmp):
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha); ni = 2.0; cur = tmp; poses, lm = tp, tl
                else:
                    lam *= ni; ni *= 2
                q += 1
                if not (rho < 0 and q < prm["max_trials"] and not poll()): break
            its += 1; it += 1
            if q == prm["max_trials"] or rho == 0: ok = False; continue
            res.margins.append(abs((ini - cur) * 1e3 - ini) / ini if ini > 0 else 1.0)
            if (ini - cur) * 1e3 < ini: nbad += 1
            else: nbad = 0
            if nbad >= 3: ok = False
        res.iterations[rnd] = its; res.trials[rnd] = trials; res.lam[rnd] = lam; res.chi2[rnd] = cur; res.rounds = rnd + 1
        if not stored_error:                                                        # the other reading: every test evaluates the estimate
            R, t, X = g.gather(poses, lm); held = g.chi2(g.errors(R, t, X))
        res.round_chi2.append(held.copy())
        if rnd == 1: break
        if poll(): break
        dp = depth_positive(poses, lm)
        with np.errstate(invalid="ignore"):
            over = held > gate
        level |= g.is_pt & (over | ~dp)
        s, e = g.ln_start_edge[g.ln_start_edge >= 0], g.ln_end_edge[g.ln_start_edge >= 0]
        bad = over[s] | over[e]
        level[s[bad]] = True; level[e[bad]] = True
        level |= ((g.kind == PAR) | (g.kind == PERP)) & over
    if len(res.round_chi2) < 2 and stored_error: res.round_chi2.append(held.copy())
    if not stored_error and res.rounds == 2:
        R, t, X = g.gather(poses, lm); held = g.chi2(g.errors(R, t, X))
    dp = depth_positive(poses, lm)
    with np.errstate(invalid="ignore"):
        over = held > gate
    m = g.pt_edge >= 0; res.pt_erase[m] = over[g.pt_edge[m]] | ~dp[g.pt_edge[m]]
    m = g.ln_start_edge >= 0
    res.ln_erase[m] = over[g.ln_start_edge[m]] if final_start_twice else (over[g.ln_start_edge[m]] | over[g.ln_end_edge[m]])
    m = g.manh_edge >= 0; res.manh_erase[m] = over[g.manh_edge[m]]
    m = g.par_edge >= 0; res.par_erase[m] = over[g.par_edge[m]]
    m = g.perp_edge >= 0; res.perp_erase[m] = over[g.perp_edge[m]]
    res.held = held; res.gate = gate; res.level = level
    res.Tcw_d = np.array([se3_to_Tcw(p) for p in poses]).reshape(-1, 3, 4); res.Tcw_f = res.Tcw_d.astype(F32)
    res.pt_d = lm[:G.n_points, :3].copy(); res.pt_f = res.pt_d.astype(F32)
    res.ln_d = G.ln_pos.copy()
    for l in range(G.n_points, g.nlm): res.ln_d[g.lm_line[l]] = lm[l]
    res.ln_f = res.ln_d.astype(F32)
    res.stopped_at = polls[1]; res.status = OPTIMISED
    return res


def walk_erased(G, res, pairing="as_written"):
    """the host walk of :3849-3901 as lists of what it erases: (points [(kf, point)], lines [(kf, line)], par [(line, kf, k)], perp
    [(line, kf, k)]).  as_written: the erased line observation i (in push order) is paired with vpLineEdgeKF[i], which holds TWO entries
    per observation, i.e. the key frame of observation i // 2 (reading 4); aligned: with its own key frame.  No Manhattan observation
    is erased (reading 5): res.manh_erase is the caller's."""
    pt_owner = np.repeat(np.arange(G.n_points), np.diff(G.pt_obs_start)); ln_owner = np.repeat(np.arange(G.n_lines), np.diff(G.ln_obs_start))
    points = [(int(G.pt_obs_kf[o]), int(pt_owner[o])) for o in np.flatnonzero(res.pt_erase)]
    push = [o for o in range(len(G.ln_obs_kf)) if res.line_made[ln_owner[o]]]       # vpLineEdgesSP's order: observations of made lines
    lines = []
    for i, o in enumerate(push):
        if res.ln_erase[o]:
            kf = int(G.ln_obs_kf[push[i // 2]]) if pairing == "as_written" else int(G.ln_obs_kf[o])
            lines.append((kf, int(ln_owner[o])))
    out = []
    for start, kfv, flags in ((G.par_start, G.par_kf, res.par_erase), (G.perp_start, G.perp_kf, res.perp_erase)):
        owner = np.repeat(np.arange(G.n_lines), np.diff(start)); lst = []
        for o in np.flatnonzero(flags):
            first = o
            while first > start[owner[o]] and kfv[first - 1] == kfv[o]: first -= 1
            lst.append((int(owner[o]), int(kfv[o]), int(o - first)))                  # k: the entry's position in its key frame's vector
        out.append(lst)
    return points, lines, out[0], out[1]


# ---------------------------------------------------------------- windows
def make_window(seed, n_free=4, n_fixed_local=1, n_outside=2, n_points=60, n_lines=10, noise=0.03, outliers=0.03, off=(0.001, 0.002),
                lm_off=0.003, max_obs=8, min_obs=2, structural=True, skip_cases=True, cam=CAM, neighbours=None):
    """key frames on a path looking down +z at points and lines in a box; each landmark is seen by a subset of the key frames; pixel noise
    and a share of gross outliers; Manhattan-aligned lines; par / perp entries with the skip cases.  Key frame 0 is the current one; the
    fixed local key frame (mnId == 0) and the outside observers come last.  neighbours = k: a point is seen by k consecutive key frames
    (the W shape).  Returns (Window, truth dict)."""
    r = np.random.RandomState(seed)
    fx, fy, cx, cy = cam
    nkf = n_free + n_fixed_local + n_outside
    Rs, ts = [], []
    step = 0.25 if nkf <= 16 else 0.15
    for k in range(nkf):
        Rk = rot_vec(r.uniform(-0.05, 0.05, 3)); c = np.array([step * k, r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05)])
        Rs.append(Rk); ts.append(-Rk @ c)
    span = step * (nkf - 1)

    def proj(k, X):
        Y = X @ Rs[k].T + ts[k]
        return np.stack([Y[..., 0] / Y[..., 2] * fx + cx, Y[..., 1] / Y[..., 2] * fy + cy], axis=-1), Y[..., 2]

    def visible(k, X):
        uv, z = proj(k, X)
        return (z > 0.5) & (uv[..., 0] > 10) & (uv[..., 0] < 630) & (uv[..., 1] > 10) & (uv[..., 1] < 470)

    def pick(vis, first=None):
        ks = np.flatnonzero(vis)
        if first is not None:
            ks = ks[(ks >= first) & (ks < first + neighbours) | (ks >= n_free)][:neighbours + 2]
        elif len(ks) > max_obs:
            ks = np.sort(r.choice(ks, max_obs, replace=False))
        return ks
    fixed = np.zeros(nkf, np.uint8); fixed[n_free:] = 1
    Xp = np.stack([r.uniform(-1.5, span + 1.5, n_points), r.uniform(-1.2, 1.2, n_points), r.uniform(2.5, 6.0, n_points)], axis=1)
    first = None
    if neighbours is not None:
        first = np.minimum(np.arange(n_points) % max(n_free, 1), max(n_free - neighbours, 0))
        Xp[:, 0] = step * (first + (neighbours - 1) / 2.0) + r.uniform(-0.5, 0.5, n_points)
    pt_start, pt_kf, pt_uv, pt_s2 = [0], [], [], []
    for i in range(n_points):
        for _ in range(50):
            ks = pick(np.array([visible(k, Xp[i]) for k in range(nkf)]), None if first is None else first[i])
            if len(ks) >= min_obs or first is not None: break
            Xp[i] = [r.uniform(-1.5, span + 1.5), r.uniform(-1.2, 1.2), r.uniform(2.5, 6.0)]
        for k in ks:
            uv = proj(k, Xp[i])[0] + r.normal(0, noise, 2)
            if r.uniform() < outliers: uv = uv + r.choice([-1, 1], 2) * r.uniform(20, 50, 2)
            pt_kf.append(k); pt_uv.append(uv); pt_s2.append(1.0 / (1.2 ** r.randint(0, 8)) ** 2)
        pt_start.append(len(pt_kf))
    # lines: a share along the world axes (the Manhattan frame is the identity)
    A = np.stack([r.uniform(-1.0, span + 1.0, n_lines), r.uniform(-1.0, 1.0, n_lines), r.uniform(2.5, 5.5, n_lines)], axis=1)
    manh = np.zeros(n_lines, np.int32); B = np.zeros_like(A)
    for i in range(n_lines):
        if i % 3 != 2:
            ax = i % 3 if i % 3 < 2 else 0
            d = np.zeros(3); d[ax] = 1.0; d = rot_vec(r.normal(0, 0.04 * noise, 3)) @ d
            manh[i] = ax + 1
            if r.uniform() < outliers * 2: manh[i] = (ax + 1) % 3 + 1              # a wrong axis
        else:
            d = r.normal(size=3); d /= np.linalg.norm(d)
            if abs(d[0]) < 0.2: d[0] = 0.3
        B[i] = A[i] + d * r.uniform(0.4, 0.9)
    ln_start, ln_kf, ln_fn = [0], [], []
    par = dict(start=[0], kf=[], idx=[], fn=[], size=[]); perp = dict(start=[0], kf=[], idx=[], fn=[], size=[])
    for i in range(n_lines):
        ks = pick(np.array([visible(k, A[i]) and visible(k, B[i]) for k in range(nkf)]))
        for k in ks:
            pa = np.append(proj(k, A[i])[0] + r.normal(0, noise, 2), 1.0); pb = np.append(proj(k, B[i])[0] + r.normal(0, noise, 2), 1.0)
            if r.uniform() < outliers: pa[1] += r.uniform(15, 40); pb[1] += r.uniform(15, 40)
            l = np.cross(pa, pb); l = l / np.sqrt(l[0] ** 2 + l[1] ** 2)
            ln_kf.append(k); ln_fn.append(l)
        ln_start.append(len(ln_kf))
        for which, lst in ((0, par), (1, perp)):
            keys = 0
            if structural and len(ks):
                for k in ks[:3]:
                    keys += 1
                    for j in range(1 + (i + k) % 2):
                        # the 2-D direction of the projected line in key frame 0's camera, as the edge computes it (reading 1)
                        d2 = proj(k, B[i])[0] - proj(k, A[i])[0]; d2 = d2 / np.linalg.norm(d2)
                        ang = r.normal(0, 0.2 * noise) + (1.3 if r.uniform() < outliers else 0.0)
                        c, s = np.cos(ang), np.sin(ang); d2 = np.array([c * d2[0] - s * d2[1], s * d2[0] + c * d2[1]])
                        fn = np.array([d2[0], d2[1], 1.0]) if which == 0 else np.array([-d2[1], d2[0], 1.0])
                        fn = fn * r.uniform(0.5, 2.0); idx = int(r.randint(0, 200))
                        if skip_cases:
                            u = r.uniform()
                            if u < 0.04: idx = -1
                            elif u < 0.08: fn[0] = 0.0
                            elif u < 0.12: fn[0] = -1.0
                            elif u < 0.16: fn[1] = np.nan
                        lst["kf"].append(k); lst["idx"].append(idx); lst["fn"].append(fn)
            lst["start"].append(len(lst["kf"])); lst["size"].append(keys)
    # the start: poses and landmarks off the truth
    Tcw = np.zeros((nkf, 3, 4))
    for k in range(nkf):
        if fixed[k]: R0, t0 = Rs[k], ts[k]
        else: R0 = rot_vec(r.normal(0, off[0] / np.sqrt(3), 3)) @ Rs[k]; t0 = ts[k] + r.normal(0, off[1] / np.sqrt(3), 3)
        Tcw[k, :, :3] = R0; Tcw[k, :, 3] = t0
    Ltrue = np.concatenate([A, B], axis=1)
    W = Window(Tcw=Tcw, fixed=fixed, cam=np.tile(np.array(cam, F32), (nkf, 1)), pt_pos=Xp + r.normal(0, lm_off, Xp.shape),
               pt_obs_start=pt_start, pt_obs_kf=pt_kf, pt_obs_uv=np.array(pt_uv).reshape(-1, 2), pt_obs_inv_sigma2=pt_s2,
               ln_pos=Ltrue + r.normal(0, lm_off, Ltrue.shape), ln_manh_idx=manh, ln_obs_start=ln_start, ln_obs_kf=ln_kf,
               ln_obs_fn=np.array(ln_fn).reshape(-1, 3), par_start=par["start"], par_kf=par["kf"], par_idx=par["idx"],
               par_fn=np.array(par["fn"]).reshape(-1, 3), par_map_size=par["size"], perp_start=perp["start"], perp_kf=perp["kf"], perp_idx=perp["idx"],
               perp_fn=np.array(perp["fn"]).reshape(-1, 3), perp_map_size=perp["size"], manh_axis=np.eye(3), manh_available=1)
    truth = dict(Tcw=np.array([np.concatenate([Rs[k], ts[k][:, None]], axis=1) for k in range(nkf)]), points=Xp, lines=Ltrue)
    return W, truth


SHAPES = dict(
    S=dict(n_free=4, n_fixed_local=1, n_outside=2, n_points=60, n_lines=10),
    M=dict(n_free=24, n_fixed_local=1, n_outside=7, n_points=1500, n_lines=120, min_obs=5, outliers=0.02),
    W=dict(n_free=64, n_fixed_local=0, n_outside=2, n_points=64 * 30, n_lines=16, neighbours=5, outliers=0.005),
    T=dict(n_free=32, n_fixed_local=1, n_outside=7, n_points=6000, n_lines=600, min_obs=5, outliers=0.02))      # the timing window: 40 key frames


def shape_window(shape, seed, **kw):
    a = dict(SHAPES[shape]); a.update(kw)
    return make_window(seed, **a)


BAND = po.BAND       # a window is accepted when no edge's chi2 lies within +-2 % of its gate at the end of either round


def accepted(res, band=BAND):
    """no edge's held chi2 within the band of its gate at the end of either round, every chi2 finite, and no Levenberg decision on a
    knife's edge (a trial that changed chi2 by less than 1e-6 of itself, or the nBad test within 1e-6 of its threshold): two correct
    implementations take the same decisions on an accepted window"""
    g = res.graph
    if res.status != OPTIMISED: return True
    for held in res.round_chi2:
        with np.errstate(invalid="ignore"):
            if np.any(np.abs(held - res.gate) <= band * res.gate) or np.any(~np.isfinite(held)):
                return False
    if any(abs(s) < 1e-6 for s in res.steps) or any(m < 1e-6 for m in res.margins):
        return False
    return True


DECISIONS = ("iterations", "trials", "rounds", "pt_erase", "ln_erase", "manh_erase", "par_erase", "perp_erase")


def same_decisions(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in DECISIONS)


TREE_SEEDS = (7, 8, 9)


def accepted_scenes(shape, count, seed0=1000, tree_seeds=TREE_SEEDS, **kw):
    """(scenes, generated): (Window, Result, truth, Results of the other arithmetic) in seed order.  A window is in the set when it passes
    `accepted` AND the restatement takes the same decisions (iterations, trials, every flag) under Ops("tree", s) for every s of
    tree_seeds, three different roundings: lambda shrinks
    by up to a third per good step, and once it is small the rounding noise of the numeric Jacobians (about 2e-5 per entry at delta 1e-9)
    moves a line's end points along the line, which no edge observes, far enough to change which trial is rejected -- on such a window
    two correct implementations need not take the same number of trials.  More than half rejected is an error."""
    out, gen, s = [], 0, seed0
    while len(out) < count:
        W, T = shape_window(shape, s, **kw); s += 1; gen += 1
        R = local_map_optimization(W)
        if accepted(R):
            bs = []
            for sd in tree_seeds:
                bs.append(local_map_optimization(W, ops=Ops("tree", sd)))
                if not same_decisions(R, bs[-1]): break
            else:
                out.append((W, R, T, bs))
        assert gen <= 2 * max(len(out), 2) + 2 and gen < 100, "more than half of the generated windows rejected"
    return out, gen


def measured_D(scenes, seeds=TREE_SEEDS):
    """D of tests/test_local_ba_gpu.py, one figure each for (poses, points, lines) -- a line's end points slide along the line, which no
    edge observes, so their D is orders above the others' and one common figure would test nothing: the largest difference of any entry between the restatement with g2o's
    edge-order sums, LAPACK's landmark inverses and numpy's libm, and the restatement with the other fixed order of the sums, the
    kernel's tree for chi2 and scale, its LDL^T landmark inverses and every sin / cos result moved by one ulp in a pseudo-random direction
    (one run per seed; the largest difference counts)"""
    D = np.zeros(3)
    for sc in scenes:
        W, R = sc[0], sc[1]
        for b in (sc[3] if len(sc) > 3 and seeds == TREE_SEEDS else [local_map_optimization(W, ops=Ops("tree", sd)) for sd in seeds]):
            D = np.maximum(D, [float(np.abs(R.Tcw_d - b.Tcw_d).max()), float(np.abs(R.pt_d - b.pt_d).max()) if len(R.pt_d) else 0.0,
                               float(np.abs(R.ln_d - b.ln_d).max()) if len(R.ln_d) else 0.0])
    return D


def to_binding(W):
    """the graph argument of the Python binding's LocalBA.optimize"""
    return W.as_dict()
