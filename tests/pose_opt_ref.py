"""CPU restatement (numpy float64) of Optimizer::PoseOptimization for the RGB-D tracker (reference src/Optimizer.cc:590-1478) and a
deterministic scene generator.  g2o cannot be built here (no Eigen), so tests/test_pose_opt.py pins this file by known answers.

What is restated, with the files it was written from:
  edges          EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose (Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp}: the
                 stereo projection's `const float invz`, :299-306; analytic Jacobians :266-288, :335-364), DistPt2Line2DMultiFrameOnlyPose
                 (include/g2oMSC.h:612-662), DistVp2VpOnlyPose (g2oMSC.h:766-846), EdgePlaneOnlyPose / EdgeParallelPlaneOnlyPose /
                 EdgeVerticalPlaneOnlyPose (g2oAddition/EdgePlane.h:128, EdgeParallelPlane.h:112, EdgeVerticalPlane.h:114) over
                 g2oAddition/Plane3D.h
  Jacobians      g2o's numeric rule: central differences, delta 1e-9, through SE3Quat::exp(update) * estimate, times 1 / (2 delta)
                 (core/base_unary_edge.hpp:82-130)
  quadratic form core/base_unary_edge.hpp:43-72 with RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91)
  Levenberg      core/optimization_algorithm_levenberg.cpp:61-189; SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-421) stops a
                 round at the first iteration that is not OK
  rounds         Optimizer.cc:1183-1466
Readings (the same in csrc/pose_opt.hip): a pose is kept as unit quaternion + translation like SE3Quat, and points and
planes are mapped with the quaternion's rotation matrix (Eigen's toRotationMatrix) instead of Eigen's vector form of q v q^-1; the dense
6 x 6 solve is LDL^T without pivoting, "not positive" = a pivot <= 0; Plane3D::rotation is Rz(azimuth) Ry(-elevation) as a matrix product;
an evaluation of DistVp2VpOnlyPose that takes the early return (a vanishing z of either direction) yields error 0 for that evaluation
(the reference keeps a stale or uninitialised _error) and flags the edge when it is the evaluation a round's classification reads.
A stored _error is never kept per edge: classification re-evaluates at the pose of the round's last computeActiveErrors (the last trial,
accepted or not), which is the same arithmetic on the same inputs."""
import numpy as np

DELTA = 1e-9
F32 = np.float32


class Ops:
    """arithmetic that may differ between two correct implementations: the libm calls and the order of the sums over the edges"""
    def __init__(self, order="seq", ulp_seed=None):
        self.order = order
        self.rng = np.random.RandomState(ulp_seed) if ulp_seed is not None else None

    def _nudge(self, v):
        if self.rng is None:
            return v
        v = np.asarray(v, np.float64)
        d = self.rng.randint(0, 2, size=v.shape) * 2 - 1
        return np.nextafter(v, np.where(d > 0, np.inf, -np.inf))

    def sin(self, x): return self._nudge(np.sin(x))
    def cos(self, x): return self._nudge(np.cos(x))
    def atan2(self, y, x): return self._nudge(np.arctan2(y, x))

    def sum0(self, a):
        """sum over axis 0 (the edges, in insertion order).  seq: one running sum, as g2o adds edge after edge.  tree: the kernel's fixed
        tree -- thread t of 256 adds edges t, t + 256, ... in order, a wave halves 64 lanes (lane i += lane i + 32, 16, ... 1), waves 0..3
        are added in order."""
        a = np.asarray(a, np.float64)
        if a.shape[0] == 0:
            return np.zeros(a.shape[1:])
        if self.order == "seq":
            return np.cumsum(a, axis=0)[-1]
        n = a.shape[0]; k = (n + 255) // 256
        p = np.zeros((k * 256,) + a.shape[1:]); p[:n] = a
        p = np.cumsum(p.reshape((k, 256) + a.shape[1:]), axis=0)[-1].reshape((4, 64) + a.shape[1:])
        off = 32
        while off:
            p[:, :off] = p[:, :off] + p[:, off:2 * off]; off //= 2
        return ((p[0, 0] + p[1, 0]) + p[2, 0]) + p[3, 0]


# ---------------------------------------------------------------- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h)
def quat_from_R(m):
    """Eigen::Quaterniond(Matrix3d), (w, x, y, z)"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0); q[0] = 0.5 * t; t = 0.5 / t
        q[1] = (m[2, 1] - m[1, 2]) * t; q[2] = (m[0, 2] - m[2, 0]) * t; q[3] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]: i = 1
        if m[2, 2] > m[i, i]: i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0); q[1 + i] = 0.5 * t; t = 0.5 / t
        q[0] = (m[k, j] - m[j, k]) * t; q[1 + j] = (m[j, i] + m[i, j]) * t; q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def quat_normalize(q):
    """SE3Quat::normalizeRotation: w >= 0, unit norm"""
    if q[0] < 0: q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def quat_to_R(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def se3_exp(u, ops):
    """SE3Quat::exp (se3quat.h:229-263): update = (omega, upsilon); theta < 1e-5 takes I + Omega + Omega^2 for R and V"""
    u = np.asarray(u, np.float64)
    om, up = u[:3], u[3:]
    th = np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    Om = skew(om); Om2 = Om @ Om
    if th < 0.00001:
        R = np.eye(3) + Om + Om2; V = R
    else:
        s, c = float(ops.sin(th)), float(ops.cos(th))
        R = np.eye(3) + s / th * Om + (1 - c) / (th * th) * Om2
        V = np.eye(3) + (1 - c) / (th * th) * Om + (th - s) / (th * th * th) * Om2
    return quat_normalize(quat_from_R(R)), V @ up


def se3_mul(a, b):
    """SE3Quat::operator*: (qa qb, ta + Ra tb), normalised"""
    return quat_normalize(quat_mul(a[0], b[0])), a[1] + quat_to_R(a[0]) @ b[1]


def se3_from_Tcw(T):
    T = np.asarray(T, np.float64).reshape(3, 4)
    return quat_normalize(quat_from_R(T[:, :3])), T[:, 3].copy()


def se3_to_Tcw(p):
    return np.concatenate([quat_to_R(p[0]), p[1].reshape(3, 1)], axis=1)


# ---------------------------------------------------------------- Plane3D (g2oAddition/Plane3D.h), vectorised over rows
def plane_normalize(c):
    """Plane3D::normalize (:175-180): divide by |n|, then the sign rule d >= 0"""
    c = np.asarray(c, np.float64).reshape(-1, 4)
    n = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
    c = c * (1.0 / n)[:, None]
    return np.where((c[:, 3] < 0.0)[:, None], -c, c)


def plane_transform(R, t, c):
    """operator*(Isometry3D, Plane3D) (:186-199)"""
    n = c[:, :3] @ R.T
    d = c[:, 3] - (t[0] * n[:, 0] + t[1] * n[:, 1] + t[2] * n[:, 2])
    v = np.concatenate([n, d[:, None]], axis=1)
    v = np.where((d < 0.0)[:, None], -v, v)
    return plane_normalize(v)


def _rot_T_apply(v, m, ops):
    """rotation(v)^T m and then (azimuth, elevation) of the result (:46-82): rotation = Rz(az) Ry(-el)"""
    az = ops.atan2(v[:, 1], v[:, 0]); el = ops.atan2(v[:, 2], np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]))
    ca, sa, ce, se = ops.cos(az), ops.sin(az), ops.cos(-el), ops.sin(-el)
    # R = [[ca ce, -sa, ca se], [sa ce, ca, sa se], [-se, 0, ce]]
    n0 = ca * ce * m[:, 0] + sa * ce * m[:, 1] - se * m[:, 2]
    n1 = -sa * m[:, 0] + ca * m[:, 1]
    n2 = ca * se * m[:, 0] + sa * se * m[:, 1] + ce * m[:, 2]
    return ops.atan2(n1, n0), ops.atan2(n2, np.sqrt(n0 * n0 + n1 * n1))


def plane_ominus(local, meas, ops):
    a, e = _rot_T_apply(local[:, :3], meas[:, :3], ops)
    return np.stack([a, e, (-local[:, 3]) - (-meas[:, 3])], axis=1)


def plane_ominus_par(local, meas, ops):
    nor = local[:, :3]
    dot = meas[:, 0] * nor[:, 0] + meas[:, 1] * nor[:, 1] + meas[:, 2] * nor[:, 2]
    nor = np.where((dot < 0)[:, None], -nor, nor)
    a, e = _rot_T_apply(nor, meas[:, :3], ops)
    return np.stack([a, e, np.zeros_like(a)], axis=1)


def plane_ominus_ver(local, meas, ops):
    n, m = local[:, :3], meas[:, :3]
    v = np.stack([n[:, 1] * m[:, 2] - n[:, 2] * m[:, 1], n[:, 2] * m[:, 0] - n[:, 0] * m[:, 2], n[:, 0] * m[:, 1] - n[:, 1] * m[:, 0]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        ax = v / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])[:, None]
    s, c = np.sin(np.pi / 2), np.cos(np.pi / 2)            # constants of Eigen::AngleAxisd(M_PI / 2, axis).toRotationMatrix()
    sa = s * ax; ca = (1 - c) * ax
    t01 = ca[:, 0] * ax[:, 1]; t02 = ca[:, 0] * ax[:, 2]; t12 = ca[:, 1] * ax[:, 2]
    R00 = ca[:, 0] * ax[:, 0] + c; R11 = ca[:, 1] * ax[:, 1] + c; R22 = ca[:, 2] * ax[:, 2] + c
    b = np.stack([R00 * n[:, 0] + (t01 - sa[:, 2]) * n[:, 1] + (t02 + sa[:, 1]) * n[:, 2],
                  (t01 + sa[:, 2]) * n[:, 0] + R11 * n[:, 1] + (t12 - sa[:, 0]) * n[:, 2],
                  (t02 - sa[:, 1]) * n[:, 0] + (t12 + sa[:, 0]) * n[:, 1] + R22 * n[:, 2]], axis=1)
    a, e = _rot_T_apply(b, m, ops)
    return np.stack([a, e, np.zeros_like(a)], axis=1)


# ---------------------------------------------------------------- robust kernel
def huber(e, delta, dsqr):
    """RobustKernelHuber::robustify: (rho, rho', rho'')"""
    if e <= dsqr:
        return e, 1.0, 0.0
    s = np.sqrt(e)
    r1 = delta / s
    return 2 * s * delta - dsqr, r1, -0.5 * r1 / e


def huber_v(e, delta, dsqr):
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(e)
        out = ~(e <= dsqr)
        return np.where(out, 2 * s * delta - dsqr, e), np.where(out, delta / s, 1.0)


PLANE_PARAMS = dict(angle_info=0.5, distance_info=50.0, parallel_info=0.1, vertical_info=0.1, chi=100.0, vp_chi=50.0)   # TUM3.yaml


class Problem:
    """one frame's PoseOptimization input.  Arrays keep the reference's types: float32 where it holds floats (key points, mvuRight,
    mvInvLevelSigma2, map-point and plane positions, the camera), float64 for line functions, 3-D lines and map-line end points."""
    def __init__(self, cam, Tcw, kp_xy=None, uright=None, inv_sigma2=None, pt_has=None, pt_xyz=None,
                 linefn=None, l3d_A=None, l3d_B=None, ln_has=None, ln_xyz=None, pl_coef=None, pl_has=None, pl_map=None, plane_params=None):
        z = lambda s, t: np.zeros(s, t)
        self.cam = tuple(float(F32(v)) for v in cam)                      # fx fy cx cy bf
        self.Tcw = np.asarray(Tcw, F32).reshape(3, 4)
        self.kp_xy = z((0, 2), F32) if kp_xy is None else np.asarray(kp_xy, F32).reshape(-1, 2)
        n = len(self.kp_xy)
        self.uright = -np.ones(n, F32) if uright is None else np.asarray(uright, F32)
        self.inv_sigma2 = np.ones(n, F32) if inv_sigma2 is None else np.asarray(inv_sigma2, F32)
        self.pt_has = np.ones(n, np.uint8) if pt_has is None else np.asarray(pt_has, np.uint8)
        self.pt_xyz = z((n, 3), F32) if pt_xyz is None else np.asarray(pt_xyz, F32).reshape(n, 3)
        self.linefn = z((0, 3), np.float64) if linefn is None else np.asarray(linefn, np.float64).reshape(-1, 3)
        nl = len(self.linefn)
        self.l3d_A = z((nl, 3), np.float64) if l3d_A is None else np.asarray(l3d_A, np.float64).reshape(nl, 3)
        self.l3d_B = z((nl, 3), np.float64) if l3d_B is None else np.asarray(l3d_B, np.float64).reshape(nl, 3)
        self.ln_has = np.ones(nl, np.uint8) if ln_has is None else np.asarray(ln_has, np.uint8)
        self.ln_xyz = z((nl, 6), np.float64) if ln_xyz is None else np.asarray(ln_xyz, np.float64).reshape(nl, 6)
        self.pl_coef = z((0, 4), F32) if pl_coef is None else np.asarray(pl_coef, F32).reshape(-1, 4)
        m = len(self.pl_coef)
        self.pl_has = z((m, 3), np.uint8) if pl_has is None else np.asarray(pl_has, np.uint8).reshape(m, 3)
        self.pl_map = z((m, 3, 4), F32) if pl_map is None else np.asarray(pl_map, F32).reshape(m, 3, 4)
        self.plane_params = dict(PLANE_PARAMS) if plane_params is None else dict(plane_params)


class Result:
    def to_dict(self):
        return dict(self.__dict__)


def f32sqrt(x):
    return float(F32(np.sqrt(x)))


class _Edges:
    """the graph in insertion order: points (mono or stereo by mvuRight), line start / end pairs, vanishing directions, planes, parallel
    planes, vertical planes.  Every slot of the index space exists; `present` marks the edges the reference inserts."""
    def __init__(self, P, ops):
        self.P, self.ops = P, ops
        n, nl, m = len(P.kp_xy), len(P.linefn), len(P.pl_coef)
        self.n, self.nl, self.m = n, nl, m
        self.o_ln, self.o_vp, self.o_pl = n, n + 2 * nl, n + 3 * nl
        E = self.E = n + 3 * nl + 3 * m
        fx, fy, cx, cy, bf = P.cam
        self.present = np.zeros(E, bool)
        self.info = np.zeros((E, 3)); self.delta = np.zeros(E); self.chi_th = np.zeros(E)
        self.stereo = ~(P.uright < 0)
        self.present[:n] = P.pt_has != 0
        s2 = P.inv_sigma2.astype(np.float64)
        self.info[:n, 0] = s2; self.info[:n, 1] = s2; self.info[:n, 2] = np.where(self.stereo, s2, 0.0)
        self.delta[:n] = np.where(self.stereo, f32sqrt(7.815), f32sqrt(5.991))
        lh = P.ln_has != 0
        self.present[self.o_ln:self.o_vp:2] = lh; self.present[self.o_ln + 1:self.o_vp:2] = lh
        self.info[self.o_ln:self.o_pl] = 1.0; self.delta[self.o_ln:self.o_pl] = f32sqrt(3.84)
        self.vp_obs = P.l3d_B - P.l3d_A                                   # mvLines3D[i].second - .first (Optimizer.cc:823)
        self.vp_dw = P.ln_xyz[:, 3:] - P.ln_xyz[:, :3]
        self.present[self.o_vp:self.o_pl] = lh & np.all(self.vp_obs != 0.0, axis=1) & np.all(self.vp_dw != 0.0, axis=1)   # :827, :853
        pp = P.plane_params
        ai = 3282.8 / (pp["angle_info"] * pp["angle_info"]); di = pp["distance_info"] * pp["distance_info"]
        pi_ = 3282.8 / (pp["parallel_info"] * pp["parallel_info"]); vi = 3282.8 / (pp["vertical_info"] * pp["vertical_info"])
        o = self.o_pl
        for r, inf, d in ((0, (ai, ai, di), f32sqrt(pp["chi"])), (1, (pi_, pi_, 0.0), f32sqrt(pp["vp_chi"])), (2, (vi, vi, 0.0), f32sqrt(pp["vp_chi"]))):
            self.present[o + r * m:o + (r + 1) * m] = P.pl_has[:, r] != 0
            self.info[o + r * m:o + (r + 1) * m] = inf; self.delta[o + r * m:o + (r + 1) * m] = d
        self.dsqr = self.delta * self.delta
        self.meas = plane_normalize(P.pl_coef) if m else np.zeros((0, 4))
        with np.errstate(invalid="ignore", divide="ignore"):
            self.mapc = [plane_normalize(P.pl_map[:, r]) if m else np.zeros((0, 4)) for r in range(3)]

    def errors(self, pose):
        """computeError of every edge at a pose: (E x 3 errors, the vanishing-direction edges' early-return mask)"""
        P, ops = self.P, self.ops
        fx, fy, cx, cy, bf = P.cam
        R, t = quat_to_R(pose[0]), pose[1]
        err = np.zeros((self.E, 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.n:
                X = P.pt_xyz.astype(np.float64) @ R.T + t
                u = X[:, 0] / X[:, 2] * fx + cx; v = X[:, 1] / X[:, 2] * fy + cy                       # mono: project2d, then * f + c
                iz = (1.0 / X[:, 2]).astype(F32).astype(np.float64)                                    # stereo: const float invz
                us = X[:, 0] * iz * fx + cx; vs = X[:, 1] * iz * fy + cy; ur = us - bf * iz
                ox, oy, orr = P.kp_xy[:, 0].astype(np.float64), P.kp_xy[:, 1].astype(np.float64), P.uright.astype(np.float64)
                err[:self.n, 0] = np.where(self.stereo, ox - us, ox - u)
                err[:self.n, 1] = np.where(self.stereo, oy - vs, oy - v)
                err[:self.n, 2] = np.where(self.stereo, orr - ur, 0.0)
            early = np.zeros(self.nl, bool)
            if self.nl:
                S = P.ln_xyz[:, :3] @ R.T + t; Epd = P.ln_xyz[:, 3:] @ R.T + t
                l = P.linefn
                for k, X in ((0, S), (1, Epd)):
                    pu = X[:, 0] / X[:, 2] * fx + cx; pv = X[:, 1] / X[:, 2] * fy + cy
                    err[self.o_ln + k:self.o_vp:2, 0] = l[:, 0] * pu + l[:, 1] * pv + l[:, 2]
                m = self.vp_obs
                dc = Epd - S
                dot = m[:, 0] * dc[:, 0] + m[:, 1] * dc[:, 1] + m[:, 2] * dc[:, 2]
                den = np.sqrt(dc[:, 0] * dc[:, 0] + dc[:, 1] * dc[:, 1] + dc[:, 2] * dc[:, 2]) * np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
                dc = np.where((dot / den < 0.0)[:, None], S - Epd, dc)
                a = np.stack([fx * m[:, 0] + cx * m[:, 2], fy * m[:, 1] + cy * m[:, 2], m[:, 2]], axis=1)
                b = np.stack([fx * dc[:, 0] + cx * dc[:, 2], fy * dc[:, 1] + cy * dc[:, 2], dc[:, 2]], axis=1)
                early = (a[:, 2] == 0.0) | (b[:, 2] == 0.0)
                a0, a1 = a[:, 0] / a[:, 2], a[:, 1] / a[:, 2]; b0, b1 = b[:, 0] / b[:, 2], b[:, 1] / b[:, 2]
                na = np.sqrt(a0 * a0 + a1 * a1); nb = np.sqrt(b0 * b0 + b1 * b1)
                a0, a1, b0, b1 = a0 / na, a1 / na, b0 / nb, b1 / nb
                d0, d1 = a0 - b0, a1 - b1
                err[self.o_vp:self.o_pl, 0] = np.where(early, 0.0, np.sqrt(d0 * d0 + d1 * d1))
            if self.m:
                o, m_ = self.o_pl, self.m
                err[o:o + m_] = plane_ominus(plane_transform(R, t, self.mapc[0]), self.meas, ops)
                err[o + m_:o + 2 * m_] = plane_ominus_par(plane_transform(R, t, self.mapc[1]), self.meas, ops)
                err[o + 2 * m_:o + 3 * m_] = plane_ominus_ver(plane_transform(R, t, self.mapc[2]), self.meas, ops)
        err[~self.present] = 0.0
        return err, early

    def chi2(self, err):
        return self.info[:, 0] * err[:, 0] * err[:, 0] + self.info[:, 1] * err[:, 1] * err[:, 1] + self.info[:, 2] * err[:, 2] * err[:, 2]

    def point_jacobian(self, pose):
        """linearizeOplus of the two point edges (types_six_dof_expmap.cpp:266-288, :335-364): n x 3 x 6"""
        P = self.P
        fx, fy, cx, cy, bf = P.cam
        X = P.pt_xyz.astype(np.float64) @ quat_to_R(pose[0]).T + pose[1]
        with np.errstate(invalid="ignore", divide="ignore"):
            x, y = X[:, 0], X[:, 1]; invz = 1.0 / X[:, 2]; iz2 = invz * invz
            J = np.zeros((self.n, 3, 6))
            J[:, 0, 0] = x * y * iz2 * fx; J[:, 0, 1] = -(1 + (x * x * iz2)) * fx; J[:, 0, 2] = y * invz * fx
            J[:, 0, 3] = -invz * fx; J[:, 0, 5] = x * iz2 * fx
            J[:, 1, 0] = (1 + y * y * iz2) * fy; J[:, 1, 1] = -x * y * iz2 * fy; J[:, 1, 2] = -x * invz * fy
            J[:, 1, 4] = -invz * fy; J[:, 1, 5] = y * iz2 * fy
            s = self.stereo
            J[s, 2, 0] = J[s, 0, 0] - bf * y[s] * iz2[s]; J[s, 2, 1] = J[s, 0, 1] + bf * x[s] * iz2[s]; J[s, 2, 2] = J[s, 0, 2]
            J[s, 2, 3] = J[s, 0, 3]; J[s, 2, 5] = J[s, 0, 5] - bf * iz2[s]
        return J


def perturbed(pose, ops):
    """the 12 poses of the numeric Jacobian: exp(+-delta e_d) * estimate"""
    out = []
    for d in range(6):
        for sgn in (1.0, -1.0):
            u = np.zeros(6); u[d] = sgn * DELTA
            out.append(se3_mul(se3_exp(u, ops), pose))
    return out


def ldlt_solve(H, b):
    """x of H x = b by LDL^T without pivoting; ok = every pivot > 0"""
    n = len(b); L = np.eye(n); D = np.zeros(n); ok = True
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            s = H[j, j]
            for k in range(j): s = s - L[j, k] * L[j, k] * D[k]
            D[j] = s
            if not (s > 0): ok = False
            for i in range(j + 1, n):
                s2 = H[i, j]
                for k in range(j): s2 = s2 - L[i, k] * L[j, k] * D[k]
                L[i, j] = s2 / D[j]
        y = np.zeros(n)
        for i in range(n):
            s = b[i]
            for k in range(i): s = s - L[i, k] * y[k]
            y[i] = s
        x = np.zeros(n)
        for i in range(n - 1, -1, -1):
            s = y[i] / D[i]
            for k in range(i + 1, n): s = s - L[k, i] * x[k]
            x[i] = s
    return x, ok


class Levenberg:
    """OptimizationAlgorithmLevenberg over one pose vertex.  sys_fn(pose) -> (H, b, robust chi2); chi_fn(pose) -> robust chi2"""
    def __init__(self, sys_fn, chi_fn, ops):
        self.sys_fn, self.chi_fn, self.ops = sys_fn, chi_fn, ops
        self.lam = 0.0; self.ni = 2.0; self.nbad = 0; self.trials = 0; self.last_eval = None; self.chi = 0.0
        self.steps = []                       # per trial: (chi before - chi after) / chi before, the quantity whose sign decides the trial

    def solve(self, it, pose):
        """one call of solve(iteration): returns (pose, ok)"""
        H, b, cur = self.sys_fn(pose)
        ini = cur
        if it == 0:
            self.lam = 1e-5 * max(0.0, max(abs(H[j, j]) for j in range(6))); self.ni = 2.0; self.nbad = 0      # tau * maxDiagonal
        rho = 0.0; q = 0
        while True:
            x, ok2 = ldlt_solve(H + self.lam * np.eye(6), b)
            trial = se3_mul(se3_exp(x, self.ops), pose)
            tmp = self.chi_fn(trial); self.last_eval = trial; self.trials += 1
            if not ok2: tmp = np.finfo(np.float64).max
            scale = 0.0
            for j in range(6): scale += x[j] * (self.lam * x[j] + b[j])
            scale += 1e-3
            rho = (cur - tmp) / scale
            self.steps.append((cur - tmp) / cur if cur > 0 else 0.0)
            if rho > 0 and np.isfinite(tmp):
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                self.lam *= max(1.0 / 3.0, alpha); self.ni = 2.0; cur = tmp; pose = trial
            else:
                self.lam *= self.ni; self.ni *= 2
            q += 1
            if not (rho < 0 and q < 10): break
        self.chi = cur
        if q == 10 or rho == 0: return pose, False
        if (ini - cur) * 1e3 < ini: self.nbad += 1
        else: self.nbad = 0
        return pose, self.nbad < 3


def pose_optimization(P, ops=None):
    ops = ops or Ops()
    G = _Edges(P, ops)
    n, nl, m, E = G.n, G.nl, G.m, G.E
    res = Result()
    res.n_initial = int(G.present[:n].sum() + G.present[G.o_pl:].sum())
    res.n_edges = int(G.present.sum())
    res.pt_outlier = np.zeros(n, np.uint8); res.ln_outlier = np.zeros(nl, np.uint8); res.vp_outlier = np.zeros(nl, np.uint8)
    res.pl_outlier = np.zeros((m, 3), np.uint8)
    res.iterations = [0] * 4; res.trials = [0] * 4; res.lam = [0.0] * 4; res.chi2 = [0.0] * 4; res.rounds = 0
    res.n_bad = res.n_line_bad = 0
    pose0 = se3_from_Tcw(P.Tcw)
    res.Tcw = P.Tcw.astype(np.float64); res.ret = 0; res.round_chi2 = []; res.steps = []
    if res.n_initial < 3:
        return res
    level1 = np.zeros(E, bool)                       # e->level() == 1
    robust = True
    th = np.zeros(E, F32); th[:n] = np.where(G.stereo, F32(7.815), F32(5.991)); th[G.o_ln:G.o_vp] = F32(3.84)
    pose = pose0
    for rnd in range(4):
        pose = pose0
        active = G.present & ~level1

        def weights(err):
            c = G.chi2(err)
            if robust:
                r0, r1 = huber_v(c, G.delta, G.dsqr)
            else:
                r0, r1 = c, np.ones(E)
            return np.where(active, r0, 0.0), r1

        def chi_fn(p):
            return float(ops.sum0(weights(G.errors(p)[0])[0]))

        def sys_fn(p):
            err, _ = G.errors(p)
            r0, r1 = weights(err)
            J = np.zeros((E, 3, 6))
            if n: J[:n] = G.point_jacobian(p)
            pp = perturbed(p, ops)
            for d in range(6):
                e1 = G.errors(pp[2 * d])[0]; e2 = G.errors(pp[2 * d + 1])[0]
                J[n:, :, d] = (1.0 / (2 * DELTA)) * (e1[n:] - e2[n:])
            J[~active] = 0.0
            we = G.info * err                                               # omega * _error
            bvec = -(r1[:, None] * np.einsum("eki,ek->ei", J, we))
            Hm = np.einsum("eki,ek,ekj->eij", J, r1[:, None] * G.info, J)
            bvec[~active] = 0.0; Hm[~active] = 0.0
            tot = ops.sum0(np.concatenate([Hm.reshape(E, 36), bvec, r0[:, None]], axis=1))
            return tot[:36].reshape(6, 6), tot[36:42], float(tot[42])

        lm = Levenberg(sys_fn, chi_fn, ops)
        its = 0
        for it in range(10):
            pose, ok = lm.solve(it, pose); its += 1
            if not ok: break
        res.steps.append(list(lm.steps)); res.iterations[rnd] = its; res.trials[rnd] = lm.trials; res.lam[rnd] = lm.lam; res.chi2[rnd] = lm.chi; res.rounds = rnd + 1
        # classification (Optimizer.cc:1188-1458): a flagged edge is recomputed at the estimate, the others hold the last trial's error
        e_est, early_est = G.errors(pose); e_last, early_last = G.errors(lm.last_eval)
        err = np.where(level1[:, None], e_est, e_last)
        chi = G.chi2(err).astype(F32)
        res.round_chi2.append(chi.copy())
        with np.errstate(invalid="ignore"):
            bad_pt = chi[:n] > th[:n]
            cs, ce = chi[G.o_ln:G.o_vp:2], chi[G.o_ln + 1:G.o_vp:2]
            bad_ln = (cs > F32(3.84)) & (ce > F32(3.84))
            early = np.where(level1[G.o_vp:G.o_pl], early_est, early_last)
            bad_vp = early | (chi[G.o_vp:G.o_pl].astype(np.float64) > 3.84)
            o = G.o_pl
            bad_pl = np.stack([chi[o:o + m].astype(np.float64) > P.plane_params["chi"],
                               chi[o + m:o + 2 * m].astype(np.float64) > P.plane_params["vp_chi"],
                               chi[o + 2 * m:o + 3 * m].astype(np.float64) > P.plane_params["vp_chi"]], axis=1) if m else np.zeros((0, 3), bool)
        level1[:n] = bad_pt
        level1[G.o_ln:G.o_vp:2] = bad_ln; level1[G.o_ln + 1:G.o_vp:2] = bad_ln
        level1[G.o_vp:G.o_pl] = bad_vp
        for r in range(3): level1[o + r * m:o + (r + 1) * m] = bad_pl[:, r]
        level1 &= G.present
        res.n_bad = int(level1[:n].sum() + level1[o:].sum()); res.n_line_bad = int(level1[G.o_ln:G.o_vp:2].sum())
        if rnd == 2: robust = False
        if res.n_edges < 10: break
    res.pt_outlier = level1[:n].astype(np.uint8); res.ln_outlier = level1[G.o_ln:G.o_vp:2].astype(np.uint8)
    res.vp_outlier = level1[G.o_vp:G.o_pl].astype(np.uint8)
    res.pl_outlier = np.stack([level1[o + r * m:o + (r + 1) * m] for r in range(3)], axis=1).astype(np.uint8) if m else np.zeros((0, 3), np.uint8)
    res.Tcw = se3_to_Tcw(pose)
    res.ret = res.n_initial - res.n_bad - res.n_line_bad
    res.thresholds = np.concatenate([th[:G.o_vp].astype(np.float64), np.full(nl, 3.84), np.full(m, P.plane_params["chi"]), np.full(2 * m, P.plane_params["vp_chi"])])
    res.present = G.present
    return res


# ---------------------------------------------------------------- scenes
def rot_vec(w):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    if th == 0: return np.eye(3)
    K = skew(w / th)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


CAM = (535.4, 539.2, 320.1, 247.6, 40.0)     # TUM3.yaml fx fy cx cy bf


def make_scene(seed, n_pts=300, n_lines=60, n_planes=6, noise=0.5, outliers=0.1, mono=0.2, off=(0.02, 0.03), cam=CAM):
    """a camera pose, map points / lines / planes seen from it, pixel noise, a share of gross outliers, and an initial pose off the truth by
    a motion-model-sized error (off = radians, metres).  Returns (Problem, true Tcw)."""
    r = np.random.RandomState(seed)
    fx, fy, cx, cy, bf = cam
    g = noise / 0.5                                                          # scales the 3-D line and plane noise with the pixel noise
    Rt = rot_vec(r.uniform(-0.3, 0.3, 3)); tt = r.uniform(-0.5, 0.5, 3)
    to_world = lambda Xc: (Xc - tt) @ Rt                                     # Xw = R^T (Xc - t)

    def cam_points(k):
        z = r.uniform(1.0, 5.0, k); u = r.uniform(20, 620, k); v = r.uniform(20, 460, k)
        return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)

    Xc = cam_points(n_pts)
    Xw = to_world(Xc).astype(F32)
    Xc = Xw.astype(np.float64) @ Rt.T + tt
    u = Xc[:, 0] / Xc[:, 2] * fx + cx + r.normal(0, noise, n_pts); v = Xc[:, 1] / Xc[:, 2] * fy + cy + r.normal(0, noise, n_pts)
    ur = u - bf / Xc[:, 2] + r.normal(0, noise, n_pts)
    octave = r.randint(0, 8, n_pts)
    inv_s2 = (1.0 / (1.2 ** octave) ** 2).astype(F32)
    is_mono = r.uniform(size=n_pts) < mono
    ur = np.where(is_mono, -1.0, ur)
    bad = r.uniform(size=n_pts) < outliers
    u = u + bad * r.choice([-1, 1], n_pts) * r.uniform(15, 60, n_pts)
    # lines
    A = cam_points(n_lines); B = A + r.uniform(0.2, 0.8, (n_lines, 3)) * r.choice([-1, 1], (n_lines, 3))
    B[:, 2] = np.maximum(B[:, 2], 0.6)
    Lw = np.concatenate([to_world(A), to_world(B)], axis=1)
    pa = np.stack([A[:, 0] / A[:, 2] * fx + cx, A[:, 1] / A[:, 2] * fy + cy, np.ones(n_lines)], axis=1)
    pb = np.stack([B[:, 0] / B[:, 2] * fx + cx, B[:, 1] / B[:, 2] * fy + cy, np.ones(n_lines)], axis=1)
    pa[:, :2] += r.normal(0, noise, (n_lines, 2)); pb[:, :2] += r.normal(0, noise, (n_lines, 2))
    lbad = r.uniform(size=n_lines) < outliers
    pa[:, 1] += lbad * r.uniform(15, 40, n_lines); pb[:, 1] += lbad * r.uniform(15, 40, n_lines)
    l = np.cross(pa, pb); l = l / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2)[:, None]
    A3 = A + r.normal(0, 0.005 * g, A.shape); B3 = B + r.normal(0, 0.005 * g, B.shape)   # the frame's own 3-D lines (depth noise)
    vbad = r.uniform(size=n_lines) < outliers
    B3 = np.where(vbad[:, None], A3 + r.uniform(0.2, 0.6, (n_lines, 3)), B3)
    # planes: world planes seen in the camera; each frame plane gets a match, and a parallel and a vertical one built from it
    pl_coef = np.zeros((n_planes, 4), F32); pl_map = np.zeros((n_planes, 3, 4), F32); pl_has = np.ones((n_planes, 3), np.uint8)
    for i in range(n_planes):
        nc = r.normal(size=3); nc /= np.linalg.norm(nc); dc = r.uniform(0.5, 3.0)
        nw = Rt.T @ nc; dw = dc + nc @ tt                                      # n.Xc + d = 0 with Xc = R Xw + t
        jit = lambda s: rot_vec(r.normal(0, s, 3))
        pl_coef[i] = np.concatenate([jit(0.003 * g) @ nc, [dc + r.normal(0, 0.003 * g)]])
        pl_map[i, 0] = np.concatenate([nw, [dw]])
        pl_map[i, 1] = np.concatenate([jit(0.004 * g) @ nw, [dw + r.uniform(0.5, 1.5)]])
        t1 = np.cross(nw, r.normal(size=3)); t1 /= np.linalg.norm(t1)
        pl_map[i, 2] = np.concatenate([jit(0.004 * g) @ t1, [r.uniform(0.5, 3.0)]])
        k = r.uniform()
        if k < outliers: pl_map[i, 0, 3] += 0.6                                # a wrong match: half a metre off
        elif k < 2 * outliers: pl_map[i, 1, :3] = rot_vec(r.choice([-1, 1]) * 0.2 * t1) @ pl_map[i, 1, :3]
        elif k < 3 * outliers: pl_map[i, 2, :3] = rot_vec(0.2 * np.cross(nw, t1)) @ pl_map[i, 2, :3]
    R0 = rot_vec(r.normal(0, off[0] / np.sqrt(3), 3)) @ Rt; t0 = tt + r.normal(0, off[1] / np.sqrt(3), 3)
    Ttrue = np.concatenate([Rt, tt[:, None]], axis=1)
    P = Problem(cam, np.concatenate([R0, t0[:, None]], axis=1), np.stack([u, v], axis=1), ur, inv_s2, None, Xw,
                l, A3, B3, None, Lw, pl_coef, pl_has, pl_map)
    return P, Ttrue


BAND = 0.02     # a scene is accepted when no present edge's chi2 lies within +-2 % of its threshold at the end of any round


def accepted(res, band=BAND):
    for chi in res.round_chi2:
        c = chi.astype(np.float64)[res.present]; t = res.thresholds[res.present]
        with np.errstate(invalid="ignore"):
            if np.any(np.abs(c - t) <= band * t) or np.any(~np.isfinite(c)):
                return False
    return True


def coverage(P, R):
    """per edge type (points, lines, vanishing directions, planes, parallel, vertical): (inliers, outliers) among the inserted edges"""
    n, nl = len(P.kp_xy), len(P.linefn)
    rows = ((R.pt_outlier, P.pt_has), (R.ln_outlier, P.ln_has), (R.vp_outlier, R.present[n + 2 * nl:n + 3 * nl]),
            (R.pl_outlier[:, 0], P.pl_has[:, 0]), (R.pl_outlier[:, 1], P.pl_has[:, 1]), (R.pl_outlier[:, 2], P.pl_has[:, 2]))
    return np.array([[int(((f == 0) & (np.asarray(h) != 0)).sum()), int((f != 0).sum())] for f, h in rows])


def accepted_scenes(count, seed0=1000, need_cover=False, **kw):
    """(scenes, generated): scenes (Problem, Result, true pose) in seed order that pass `accepted`.  need_cover: keep generating past
    `count` until the accepted set holds every one of the six edge types with inliers and with outliers.  More than half of the generated
    scenes rejected is an error: the accepted ones would be a corner."""
    out, gen, s = [], 0, seed0
    cover = np.zeros((6, 2), int)
    while len(out) < count or (need_cover and cover.min() == 0):
        P, T = make_scene(s, **kw); s += 1; gen += 1
        R = pose_optimization(P)
        if accepted(R):
            out.append((P, R, T)); cover += coverage(P, R)
        assert gen <= 2 * max(len(out), 4) + 4 and gen < 200, "more than half of the generated scenes rejected"
    return out, gen


def measured_D(scenes, seed=7):
    """D of tests/test_pose_opt_gpu.py: the largest difference of any Tcw entry between the restatement with g2o's edge-order sums and
    numpy's libm, and with the kernel's tree order and every sin / cos / atan2 result moved by one ulp in a pseudo-random direction"""
    D = 0.0
    for P, R, _ in scenes:
        b = pose_optimization(P, Ops("tree", seed))
        D = max(D, float(np.abs(R.Tcw - b.Tcw).max()))
    return D


def to_binding(P, keypoint_dt, line3d_dt):
    """the keyword arguments of the Python binding's pose_optimize for a Problem"""
    kp = np.zeros(len(P.kp_xy), keypoint_dt); kp["x"] = P.kp_xy[:, 0]; kp["y"] = P.kp_xy[:, 1]
    l3 = np.zeros(len(P.linefn), line3d_dt); l3["A"] = P.l3d_A; l3["B"] = P.l3d_B
    return dict(Tcw=P.Tcw, kp_un=kp, uright=P.uright, inv_sigma2=P.inv_sigma2, linefn=P.linefn, lines3d=l3, plane_coef=P.pl_coef,
                pt_has=P.pt_has, pt_xyz=P.pt_xyz, ln_has=P.ln_has, ln_xyz=P.ln_xyz, pl_has=P.pl_has, pl_coef_w=P.pl_map)


def crafted_early_return():
    """pins the defined behaviour of DistVp2VpOnlyPose's early return: a map line with end points (1e-300, 1e-300, 1e-300) and
    (2e-300, 2e-300, 2e-300) passes the insertion rules (no zero component, Optimizer.cc:853), and under any pose with a translation of
    ordinary size both end points map to the translation exactly, so dc[2] == 0 at every evaluation.  The edge contributes nothing and is
    flagged in every round; eight exact stereo points hold the pose, and the key line passes through the one pixel both end points project to.  Returns (Problem, restatement result)."""
    fx, fy, cx, cy, bf = CAM
    t = np.array([0.125, -0.25, 0.5])
    Xc = np.array([[0.5, 0.4, 2], [-0.6, 0.3, 3], [0.2, -0.5, 2.5], [-0.3, -0.4, 4], [0.7, -0.1, 3.5], [0.1, 0.6, 2.25], [0.4, 0.2, 5], [-0.5, 0.1, 2.75]])
    X = (Xc - t).astype(F32)
    uv = np.stack([Xc[:, 0] / Xc[:, 2] * fx + cx, Xc[:, 1] / Xc[:, 2] * fy + cy], axis=1)
    ur = uv[:, 0] - bf / Xc[:, 2]
    T = np.concatenate([np.eye(3), t[:, None]], axis=1)
    ln = np.array([[1e-300, 1e-300, 1e-300, 2e-300, 2e-300, 2e-300]])
    P = Problem(CAM, T, uv, ur, np.ones(len(X), F32), None, X, [[0.0, 1.0, -(t[1] / t[2] * fy + cy)]], [[0.0, 0.0, 2.0]], [[1.0, 1.0, 2.5]], None, ln)
    return P, pose_optimization(P)
