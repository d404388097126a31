"""CPU restatement of Tracking::TrackManhattanFrame(mLastRcm, vSurfaceNormal, mVF3DLines) (reference src/Tracking.cc:1172-1348) with
ProjectSN2Conic (953-1026), ProjectSN2MF (1028-1150) and MeanShift (1152-1170).  Test infrastructure only: numpy float32 / float64, one step
per step of the reference, written from its semantics.  The outer loop runs once (i < 1), so its closing acos test has no effect.

cv::Mat R_cm = R_cm_update (1181) is a shallow copy: the mean shift of axis 2 and 3 reads the columns the earlier axes wrote, and fewer than
two found axes return R_last with the one found column replaced (R_cm_update = R_cm is then a self-assignment).

Readings of arithmetic that the reference leaves to OpenCV ("Manhattan tracking readings"):
  - sqrt / abs / tan of a float under `using namespace std` are the float overloads (sqrtf, fabsf, tanf);
  - no contraction into FMAs; float sums left to right;
  - R_mc * (ma_x, ma_y, 1): products and sums in double, left to right, rounded to float; cv::norm of that float vector: double;
    Mat / double: each element divided in double and rounded to float;
  - Mat::cross of two CV_32F columns: in float; cv::determinant of a 3 x 3 CV_32F: cofactor expansion along row 0 in double;
  - SVD: U V^T is the orthogonal polar factor (unique for a nonsingular matrix): here numpy's SVD in double, compared at a tolerance;
  - MeanShift's sums are sequential here (the reference's order); the kernel sums over a fixed tree, so the double sums differ in the
    last bits and the float results are compared at a tolerance.  Integer decisions do not depend on any of these readings."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
SIN_N = math.sin(0.2018)     # ProjectSN2Conic, normals
SIN_L = math.sin(0.1018)     # ProjectSN2Conic, lines
SIN_MS = math.sin(0.2518)    # ProjectSN2MF


def directions(l3d):
    """mVF3DLines' direction of every key line (RandomLine3d::director = (A - B) / sqrt((A - B).(A - B)), LineExtractor.cpp:321) and the good mask"""
    A = np.asarray(l3d["A"], F64).reshape(-1, 3); B = np.asarray(l3d["B"], F64).reshape(-1, 3)
    d = A - B
    s = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d / s[:, None]
    return d, np.asarray(l3d["good"]).reshape(-1) != 0


def cols(a):
    """columns (x, y, z) of R_cm that n_ini takes for axis a (Tracking.cc:1189-1201)"""
    return a % 3, (a + 1) % 3, a - 1


def proj_f(R, a, n):
    """n_ini of normals: float products, summed left to right in float"""
    R = np.asarray(R, F32); n = np.asarray(n, F32)
    out = []
    for c in cols(a):
        out.append(((R[0, c] * n[:, 0]).astype(F32) + (R[1, c] * n[:, 1]).astype(F32)).astype(F32) + (R[2, c] * n[:, 2]).astype(F32))
    return [o.astype(F32) for o in out]


def proj_d(R, a, d):
    """n_ini of lines: float entries times the double direction, summed in double, stored into a Point3f"""
    R = np.asarray(R, F32); d = np.asarray(d, F64)
    out = []
    for c in cols(a):
        out.append(((F64(R[0, c]) * d[:, 0] + F64(R[1, c]) * d[:, 1]) + F64(R[2, c]) * d[:, 2]).astype(F32))
    return out


def lam(x, y):
    """sqrt(x x + y y) in float (std::sqrt(float)), as a double"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(((x * x).astype(F32) + (y * y).astype(F32)).astype(F32)).astype(F32).astype(F64)


def cone_masks(R, a, n, d, good):
    """ProjectSN2Conic for axis a: the normals within sin 0.2018, the good lines within sin 0.1018"""
    with np.errstate(invalid="ignore"):
        x, y, _ = proj_f(R, a, n)
        mn = lam(x, y) < SIN_N
        x, y, _ = proj_d(R, a, d)
        ml = (lam(x, y) < SIN_L) & good
    return mn, ml


def mean_shift_axis(Rc, a, n_sel, d_sel, num_of_sn):
    """ProjectSN2MF(a, R_mc_new, cone normals, cone lines, numOfSN) -> (R_cm_Rec or zeros, density, kept, entered masks)"""
    xn, yn, zn = proj_f(Rc, a, n_sel)
    xl, yl, zl = proj_d(Rc, a, d_sel)
    x = np.concatenate([xn, xl]); y = np.concatenate([yn, yl]); z = np.concatenate([zn, zl])
    with np.errstate(invalid="ignore", divide="ignore"):
        l = lam(x, y)
        entered = l < SIN_MS
        tan_alfa = l / np.abs(z).astype(F64)
        alfa = np.arcsin(l)
        q = alfa / tan_alfa
        mx = (q * x.astype(F64)) / z.astype(F64)
        my = (q * y.astype(F64)) / z.astype(F64)
    keep = entered & ~np.isnan(mx) & ~np.isnan(my)
    mx, my = mx[keep], my[keep]
    kept = int(keep.sum())
    rec, density = np.zeros(3, F32), F32(0)
    if kept > num_of_sn:
        with np.errstate(invalid="ignore", over="ignore"):
            nrm = np.sqrt(mx * mx + my * my)
            k = np.exp((-20.0 * nrm) * nrm)
            den = np.cumsum(k)[-1]; nx = np.cumsum(k * mx)[-1]; ny = np.cumsum(k * my)[-1]
            cx, cy = nx / den, ny / den
            density = F32(den / kept)
            alfa = F32(math.sqrt(cx * cx + cy * cy))
            t = F32(np.tan(alfa) / alfa)
            ma_x, ma_y = F32(F64(t) * cx), F32(F64(t) * cy)
            cx_, cy_, cz_ = cols(a)
            Rc = np.asarray(Rc, F32)
            v = np.array([F32((F64(Rc[r, cx_]) * F64(ma_x) + F64(Rc[r, cy_]) * F64(ma_y)) + F64(Rc[r, cz_])) for r in range(3)], F32)
            nv = math.sqrt((F64(v[0]) * F64(v[0]) + F64(v[1]) * F64(v[1])) + F64(v[2]) * F64(v[2]))
            rec = np.array([F32(F64(v[r]) / nv) for r in range(3)], F32)
    nn = len(n_sel)
    return rec, density, kept, entered[:nn], entered[nn:]


def cross_f(u, v):
    u = np.asarray(u, F32); v = np.asarray(v, F32)
    return np.array([F32(u[1] * v[2]) - F32(u[2] * v[1]), F32(u[2] * v[0]) - F32(u[0] * v[2]), F32(u[0] * v[1]) - F32(u[1] * v[0])], F32)


def det_d(M):
    m = np.asarray(M, F32).astype(F64)
    c0 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c1 = m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]
    c2 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    return (m[0, 0] * c0 - m[0, 1] * c1) + m[0, 2] * c2


def polar(M):
    """R = U V^T of the SVD of M (3 x 3 float), computed in double"""
    U, _, Vt = np.linalg.svd(np.asarray(M, F64))
    return (U @ Vt).astype(F32)


def track_manhattan(normals, l3d, R_last):
    """-> dict(R, axis_vec, density, found, n_found, n_in_cone, n_selected, min_num_sn, tracked, normal_axes, line_axes).
    normals: (N, 3) float32 (vSurfaceNormal[i].normal, NaN ones included); l3d: LINE3D_DT-like with fields A, B, good (every key line);
    R_last: 3 x 3 float32."""
    n = np.asarray(normals, F32).reshape(-1, 3)
    if l3d is None or len(l3d) == 0:
        d, good = np.zeros((0, 3), F64), np.zeros(0, bool)
    else:
        d, good = directions(l3d)
    R0 = np.asarray(R_last, F32).reshape(3, 3).copy()
    R = R0.copy()                                   # R_cm_update; R_cm aliases it
    gidx = np.nonzero(good)[0]                      # mVF3DLines = the good lines, in key-line order
    dg = d[gidx]
    cones = [cone_masks(R0, a, n, dg, np.ones(len(dg), bool)) for a in (1, 2, 3)]
    n_in_cone = [int(c[0].sum()) for c in cones]
    thr = len(n) // 20
    a_, b_, c_ = n_in_cone
    if a_ > b_: a_, b_ = b_, a_
    if b_ > c_: b_, c_ = c_, b_
    if a_ > b_: a_, b_ = b_, a_
    if b_ < thr:
        thr = (b_ + a_) // 2
    found = [0, 0, 0]; axis_vec = np.zeros((3, 3), F32); density = np.zeros(3, F32); n_sel = [0, 0, 0]
    nax = np.zeros(len(n), np.uint8); lax = np.zeros(len(good), np.uint8)
    for a in (1, 2, 3):
        mn, ml = cones[a - 1]
        rec, den, kept, en_n, en_l = mean_shift_axis(R, a, n[mn], dg[ml], thr)
        n_sel[a - 1] = kept
        nax[np.nonzero(mn)[0][en_n]] |= np.uint8(1 << (a - 1))
        lax[gidx[np.nonzero(ml)[0][en_l]]] |= np.uint8(1 << (a - 1))
        if (F64(rec[0]) + F64(rec[1])) + F64(rec[2]) != 0.0:       # sum(R_cm_Rec)[0] != 0
            found[a - 1] = 1
            R[:, a - 1] = rec
            axis_vec[a - 1] = rec
            density[a - 1] = den
    nf = sum(found)
    if nf >= 2:
        if nf == 2:
            if found[0] and found[1]: w, col = cross_f(R[:, 0], R[:, 1]), 2
            elif found[1] and found[2]: w, col = cross_f(R[:, 2], R[:, 1]), 0
            else: w, col = cross_f(R[:, 0], R[:, 2]), 1
            R[:, col] = w
            if abs(det_d(R) + 1.0) < 0.5:
                R[:, col] = -w
        R = polar(R)
    return dict(R=R, axis_vec=axis_vec, density=density, found=found, n_found=nf, n_in_cone=n_in_cone, n_selected=n_sel, min_num_sn=thr,
                tracked=int(nf >= 2), normal_axes=nax, line_axes=lax)


# ---- crafted inputs (shared by the CPU and GPU tests) ----------------------------------------------------------------------------------
L3D_FIELDS = [("A", "<f8", 3), ("B", "<f8", 3), ("line_nor", "<f8", 3), ("line_eq", "<f4", 3), ("good", "<i4"),
              ("n_samples", "<i4"), ("n_inliers", "<i4"), ("inlier_mask", "<u4"), ("pad", "<i4")]
L3D_DT = np.dtype(L3D_FIELDS)


def rot(axis, deg):
    """rotation matrix about a unit axis (Rodrigues), float64"""
    k = np.asarray(axis, F64); k = k / np.linalg.norm(k); a = math.radians(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def family(rng, axis, count, noise_deg, symmetric=True):
    """unit vectors around `axis`, tilted by a Gaussian of noise_deg degrees; symmetric: each tilt comes with its opposite"""
    axis = np.asarray(axis, F64); axis = axis / np.linalg.norm(axis)
    t = np.cross(axis, [0.3, 0.5, 0.8]); t /= np.linalg.norm(t); b = np.cross(axis, t)
    m = count // 2 if symmetric else count
    e = rng.normal(0.0, math.radians(noise_deg), (m, 2))
    if symmetric:
        e = np.concatenate([e, -e])
    v = axis[None, :] + e[:, :1] * t[None, :] + e[:, 1:] * b[None, :]
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def scatter(rng, count, R, min_deg=25.0):
    """unit vectors farther than min_deg from every column of R and its opposite (outside every cone)"""
    out = []
    while len(out) < count:
        v = rng.normal(size=3); v /= np.linalg.norm(v)
        if np.all(np.abs(np.asarray(R, F64).T @ v) < math.cos(math.radians(min_deg))):
            out.append(v)
    return np.array(out, F64).reshape(-1, 3)


def lines_along(rng, dirs, good=None):
    """LINE3D_DT records whose A - B run along `dirs` (a random midpoint, a random length 0.1-1 m)"""
    dirs = np.asarray(dirs, F64).reshape(-1, 3)
    out = np.zeros(len(dirs), L3D_DT)
    mid = rng.uniform(-1, 1, (len(dirs), 3)) + np.array([0, 0, 3.0])
    ln = rng.uniform(0.1, 1.0, len(dirs))[:, None]
    out["A"] = mid + 0.5 * ln * dirs; out["B"] = mid - 0.5 * ln * dirs
    out["good"] = 1 if good is None else np.asarray(good, np.int32)
    return out


def three_families(seed=0, n=600, noise=0.5, R_true=None):
    """normals around the three columns of R_true (and their opposites), plus a scatter outside every cone"""
    rng = np.random.RandomState(seed)
    R_true = rot((0.2, -0.7, 0.4), 23.0) if R_true is None else R_true
    parts = [family(rng, s * R_true[:, c], n // 2, noise) for c in range(3) for s in (1, -1)]
    parts.append(scatter(rng, n // 3, R_true))
    return np.concatenate(parts).astype(F32), R_true


def boundary_normals():
    """with R = I, axis 1 takes lambda = |n.y|: n.y one float ulp inside and one outside sin(0.2018)"""
    s_in = F32(SIN_N)
    while float(s_in) >= SIN_N:
        s_in = np.nextafter(s_in, F32(0))
    while float(np.nextafter(s_in, F32(1))) < SIN_N:
        s_in = np.nextafter(s_in, F32(1))
    s_out = np.nextafter(s_in, F32(1))
    def unit(s):
        return np.array([math.sqrt(1.0 - float(s) * float(s)), float(s), 0.0], F32)
    n = np.array([unit(s_in), unit(s_out)], F32); n[:, 1] = [s_in, s_out]
    return n, s_in, s_out
