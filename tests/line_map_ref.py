"""CPU restatement of the line side of Tracking::TrackLocalMapWithLines: Tracking::SearchLocalLines (reference src/Tracking.cc:3279-3392) with
Frame::isInFrustum(MapLine *, 0.5) (src/Frame.cc:1429-1499) and MapLine::PredictScale (src/MapLine.cpp:549-558), the search core
(tests/local_map_lines_ref.py), the CosSita > 0.09 post-gate, and Manhattan::computeStructConstInMap (src/Manhattan.cpp:163-224).  Test
infrastructure only: numpy float32 / float64, one step per step of the reference, written from its semantics.

Readings (OpenCV and Eigen are not in the reference tree; DESIGN.md section 7 states the same ones):
  Mat_<float> << double      each entry rounded to float
  mRcw * X + mtcw            the row's products summed in float, left to right, then (float)((double)sum + (double)t)
  mOw                        -Rcw^T tcw: double sums, times -1.0, rounded to float
  0.5 * (SP + EP) - mOw      float, element-wise
  cv::norm                   sqrt of the double sum of squares, stored to float
  Mat::dot (CV_32F)          accumulates in double; divided by the float dist in double; rounded to the float viewCos
  PredictScale               float ratio, float log, float division, float ceil
  K.inv()                    closed form in double, each entry rounded to float
  K.inv() x, Rcw v           double products and sums, left to right, rounded to float once
  Mat::cross                 float; Mat /= double: each element divided in double, rounded to float
  rotCW                      Rcw as double times the double line equation"""
import math

import numpy as np

import local_map_lines_ref as core

F32 = np.float32
MAX_QUERIES = 16384


def f32(x):
    return F32(x)


def pose_parts(Tcw):
    T = np.asarray(Tcw, np.float32).reshape(3, 4)
    R = T[:, :3].copy(); t = T[:, 3].copy()
    Ow = np.zeros(3, np.float32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s = s + float(R[k, r]) * float(t[k])
        Ow[r] = F32(s * -1.0)
    return R, t, Ow


def transform(R, t, X):
    """Rcw X + tcw of a float 3-vector"""
    out = np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            s = F32(R[r, 0] * X[0]); s = F32(s + F32(R[r, 1] * X[1])); s = F32(s + F32(R[r, 2] * X[2]))
            out[r] = F32(float(s) * 1.0 + float(t[r]) * 1.0)
    return out


def predict_level_exact(max_dist, dist, log_scale_factor):
    """log(ratio) / logScaleFactor before the ceil, in float (numpy's float32 log)"""
    with np.errstate(all="ignore"):
        ratio = F32(F32(max_dist) / F32(dist))
        return F32(F32(np.log(ratio)) / F32(log_scale_factor))


def to_int(v):
    v = float(v)
    if v != v: return 0
    return int(max(-2147483648.0, min(2147483647.0, v)))


def is_in_frustum(pos, normal, max_dist, min_dist, cam, R, t, Ow, bounds4, log_scale_factor, limit=F32(0.5)):
    """-> (exit, proj, view_cos, level): exit 0 = in view, else which of the 13 conditions returned false -- 1 SPcZ < 0, 2 EPcZ < 0, 3 / 4 u1 below /
    above, 5 / 6 v1, 7 / 8 u2, 9 / 10 v2, 11 dist below 0.8 min, 12 dist above 1.2 max, 13 viewCos below the limit"""
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    P = np.asarray(pos, np.float64).astype(np.float32)
    SP, EP = P[:3], P[3:]
    with np.errstate(all="ignore"):
        SPc = transform(R, t, SP); EPc = transform(R, t, EP)
        if SPc[2] < F32(0.0): return 1, None, None, None
        if EPc[2] < F32(0.0): return 2, None, None, None
        invz1 = F32(F32(1.0) / SPc[2])
        u1 = F32(F32(F32(fx * SPc[0]) * invz1) + cx); v1 = F32(F32(F32(fy * SPc[1]) * invz1) + cy)
        if u1 < minX: return 3, None, None, None
        if u1 > maxX: return 4, None, None, None
        if v1 < minY: return 5, None, None, None
        if v1 > maxY: return 6, None, None, None
        invz2 = F32(F32(1.0) / EPc[2])
        u2 = F32(F32(F32(fx * EPc[0]) * invz2) + cx); v2 = F32(F32(F32(fy * EPc[1]) * invz2) + cy)
        if u2 < minX: return 7, None, None, None
        if u2 > maxX: return 8, None, None, None
        if v2 < minY: return 9, None, None, None
        if v2 > maxY: return 10, None, None, None
        maxD = F32(F32(1.2) * F32(max_dist)); minD = F32(F32(0.8) * F32(min_dist))
        OM = np.array([F32(F32(F32(0.5) * F32(SP[k] + EP[k])) - Ow[k]) for k in range(3)], np.float32)
        d = [float(v) for v in OM]
        dist = F32(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if dist < minD: return 11, None, None, None
        if dist > maxD: return 12, None, None, None
        pn = np.asarray(normal, np.float64).astype(np.float32)
        dot = (d[0] * float(pn[0]) + d[1] * float(pn[1])) + d[2] * float(pn[2])
        vc = F32(np.float64(dot) / np.float64(dist))
        if vc < limit: return 13, None, None, None
        lvl = to_int(np.ceil(predict_level_exact(max_dist, dist, log_scale_factor)))
    return 0, np.array([u1, v1, u2, v2], np.float32), vc, lvl


def k_inv(cam):
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = float(F32(cam[0])), 0.0, float(F32(cam[2])), 0.0, float(F32(cam[1])), float(F32(cam[3])), 0.0, 0.0, 1.0
    det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20)
    d = 1.0 / det
    t = [(a11 * a22 - a12 * a21) * d, (a02 * a21 - a01 * a22) * d, (a01 * a12 - a02 * a11) * d,
         (a12 * a20 - a10 * a22) * d, (a00 * a22 - a02 * a20) * d, (a02 * a10 - a00 * a12) * d,
         (a10 * a21 - a11 * a20) * d, (a01 * a20 - a00 * a21) * d, (a00 * a11 - a01 * a10) * d]
    return np.array(t, np.float64).astype(np.float32).reshape(3, 3)


def gemm_d(M, v):
    """3 x 3 float matrix times a float 3-vector: double products and sums, left to right, rounded to float"""
    return np.array([F32((float(M[r, 0]) * float(v[0]) + float(M[r, 1]) * float(v[1])) + float(M[r, 2]) * float(v[2])) for r in range(3)], np.float32)


def cos_sita(Ki, R, kl, wvec):
    """CosSita of Tracking.cc:3365-3379 for the key line kl (sx, sy, ex, ey) and the map line's world vector"""
    w = np.asarray(wvec, np.float64).astype(np.float32)
    with np.errstate(all="ignore"):
        S = gemm_d(Ki, np.array([kl[0], kl[1], 1.0], np.float32)); E = gemm_d(Ki, np.array([kl[2], kl[3], 1.0], np.float32))
        N = np.array([F32(F32(S[1] * E[2]) - F32(S[2] * E[1])), F32(F32(S[2] * E[0]) - F32(S[0] * E[2])), F32(F32(S[0] * E[1]) - F32(S[1] * E[0]))], np.float32)
        n = [float(v) for v in N]
        nrm = np.float64(math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
        N = np.array([F32(np.float64(v) / nrm) for v in n], np.float32)
        C = gemm_d(R, w)
        return abs((float(N[0]) * float(C[0]) + float(N[1]) * float(C[1])) + float(N[2]) * float(C[2]))


def struct_rel(R, line_eq, wvecs):
    """computeStructConstInMap's relation of every frame line (line_eq, (n, 3) float) against the world vectors ((m, 3) double): (n, m) int8"""
    le = np.asarray(line_eq, np.float32).astype(np.float64).reshape(-1, 3); W = np.asarray(wvecs, np.float64).reshape(-1, 3)
    Rd = np.asarray(R, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        lw = np.stack([(Rd[r, 0] * le[:, 0] + Rd[r, 1] * le[:, 1]) + Rd[r, 2] * le[:, 2] for r in range(3)], axis=1)
        dot = (lw[:, None, 0] * W[None, :, 0] + lw[:, None, 1] * W[None, :, 1]) + lw[:, None, 2] * W[None, :, 2]
        ma = np.sqrt((lw[:, 0] * lw[:, 0] + lw[:, 1] * lw[:, 1]) + lw[:, 2] * lw[:, 2]); mb = np.sqrt((W[:, 0] * W[:, 0] + W[:, 1] * W[:, 1]) + W[:, 2] * W[:, 2])
        ang = np.abs(dot / (ma[:, None] * mb[None, :]))
        rel = np.where(ang < 0.062, 2, np.where(ang > 0.9985, 1, 0)).astype(np.int8)
    return rel


def frustum_pass(M, cam, Tcw, bounds4, log_scale_factor, held, seen_extra=()):
    """the loops of Tracking.cc:3290-3340 -> dict(held (bad ones cleared), t_occupied, n_tested, slots, proj, view_cos, level, exits)"""
    ns = len(M["pos"]); bad = np.asarray(M["bad"]).astype(bool); obs = np.asarray(M["observed"]).astype(bool)
    held = np.asarray(held, np.int32).copy()
    seen = np.zeros(ns, bool)
    for i, h in enumerate(held):
        if h >= 0 and bad[h]: held[i] = -1
        elif h >= 0: seen[h] = True
    for e in seen_extra: seen[int(e)] = True
    t_occ = np.array([h >= 0 and obs[h] for h in held], np.uint8)
    R, t, Ow = pose_parts(Tcw)
    slots, proj, vcs, lvls, exits, nt = [], [], [], [], np.full(ns, -1, np.int32), 0
    for j in range(ns):
        if seen[j] or bad[j]: continue
        nt += 1
        e, p, vc, lv = is_in_frustum(M["pos"][j], M["normal"][j], M["max_dist"][j], M["min_dist"][j], cam, R, t, Ow, bounds4, log_scale_factor)
        exits[j] = e
        if e == 0:
            slots.append(j); proj.append(p); vcs.append(vc); lvls.append(lv)
    return dict(held=held, t_occupied=t_occ, n_tested=nt, slots=np.array(slots, np.int32), proj=np.array(proj, np.float32).reshape(-1, 4),
                view_cos=np.array(vcs, np.float32), level=np.array(lvls, np.int32), exits=exits)


def queries(M, fp):
    """the arrays hvo_search_lines_by_projection_map takes, for the frustum pass's survivors"""
    s = fp["slots"]
    return (fp["proj"], fp["view_cos"], np.asarray(M["wvec"], np.float64).reshape(-1, 3)[s], np.asarray(M["desc"], np.uint8).reshape(-1, 32)[s],
            np.asarray(M["observed"]).astype(np.uint8)[s])


def search_local_lines(M, cam, Tcw, bounds4, log_scale_factor, th, nn_ratio, t_kl, t_fn, t_l3d, t_desc, cell_start, cell_items, held, seen_extra=(),
                       search=None):
    """the whole call.  M: dict(pos (n, 6), wvec, normal (n, 3), max_dist, min_dist (n), desc (n, 32), bad, observed (n)).  search: a stand-in for the
    core (the tests of the post-gate pass canned matches) -> dict as the library's result"""
    fp = frustum_pass(M, cam, Tcw, bounds4, log_scale_factor, held, seen_extra)
    nq = len(fp["slots"]); nt = len(t_kl)
    out = dict(n_slots_tested=fp["n_tested"], n_in_view=nq, in_view_slot=fp["slots"], proj=fp["proj"], view_cos=fp["view_cos"], level=fp["level"],
               status=0, n_matches=0, n_gated=0, match_idx=np.full(nq, -1, np.int32), match_dist=np.full(nq, 256, np.int32))
    if nq > MAX_QUERIES:
        out.update(status=-4, held=np.asarray(held, np.int32).copy()); return out
    held = fp["held"].copy()
    R = pose_parts(Tcw)[0]
    if nq > 0 and nt > 0:
        q = queries(M, fp)
        fn = search or core.search_lines_by_projection_map
        nm, mi, md = fn(q[0], q[1], q[2], q[3], q[4], t_kl, t_fn, t_l3d, t_desc, fp["t_occupied"], cell_start, cell_items, bounds4, th, nn_ratio)
        out.update(n_matches=nm, match_idx=np.asarray(mi, np.int32), match_dist=np.asarray(md, np.int32))
        for k in range(nq):
            if mi[k] >= 0: held[mi[k]] = fp["slots"][k]
        if nm:
            Ki = k_inv(cam); W = np.asarray(M["wvec"], np.float64).reshape(-1, 3)
            for i in range(nt):
                if held[i] >= 0 and cos_sita(Ki, R, (t_kl["sx"][i], t_kl["sy"][i], t_kl["ex"][i], t_kl["ey"][i]), W[held[i]]) > 0.09:
                    held[i] = -1; out["n_gated"] += 1
    rel = struct_rel(R, np.asarray(t_l3d["line_eq"], np.float32).reshape(-1, 3), np.asarray(M["wvec"], np.float64).reshape(-1, 3)[fp["slots"]]) if nt else np.zeros((0, nq), np.int8)
    out.update(held=held, rel_map=rel, n_par=(rel == 1).sum(axis=1).astype(np.int32), n_perp=(rel == 2).sum(axis=1).astype(np.int32))
    return out


# ---- scenes for the GPU tests (and the CPU check of the generator itself) ----
CAM = (512.0, 512.0, 320.0, 240.0, 0.0)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
LOG_SF = float(F32(np.log(F32(1.2))))
PATTERNS = ("none", "all", "alt", "wave", "last")


def scene_pose(seed=0):
    """a camera rotated 20 degrees about y and 10 about x, off the origin (nothing special about it)"""
    a, b = np.radians(20.0 + seed), np.radians(10.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]); Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return np.hstack([Rx @ Ry, np.array([[0.3], [-0.2], [0.5]])]).astype(np.float32)


def wanted_in_view(n, pattern):
    j = np.arange(n)
    return {"none": j < 0, "all": j >= 0, "alt": j % 2 == 0, "wave": j % 64 == 5, "last": j == n - 1}[pattern]


def make_map(n, pattern, Tcw, seed=1, axes=None):
    """n map lines of which exactly the slots of `pattern` are in view under Tcw; the others fail isInFrustum for one of four reasons in turn
    (behind the camera, outside the image, out of the distance range, seen from behind).  A line in view whose log(ratio) / logScaleFactor
    lies within 1e-4 of an integer is drawn again (the predicted level is the one number here that goes through a library log); fewer than
    1 % may be rejected.  axes: world vectors drawn around these directions (else along the line) -> (map dict, rejected count)"""
    rng = np.random.RandomState(seed)
    T = np.asarray(Tcw, np.float64).reshape(3, 4); R, t = T[:, :3], T[:, 3]
    want = wanted_in_view(n, pattern)
    M = dict(pos=np.zeros((n, 6)), wvec=np.zeros((n, 3)), normal=np.zeros((n, 3)), max_dist=np.zeros(n, np.float32), min_dist=np.zeros(n, np.float32),
             desc=rng.randint(0, 256, (n, 32)).astype(np.uint8), bad=np.zeros(n, np.uint8), observed=(rng.rand(n) < 0.7).astype(np.uint8))
    Rf, tf, Ow = pose_parts(Tcw)
    rejected = 0
    for j in range(n):
        while True:
            uv = np.array([rng.uniform(60, 580), rng.uniform(60, 420)]); duv = rng.uniform(-50, 50, 2); z = rng.uniform(1.0, 4.0, 2)
            ends = []
            for k, (p, zz) in enumerate(((uv, z[0]), (uv + duv, z[0] + 0.2 * (z[1] - 2.5)))):
                Xc = np.array([(p[0] - CAM[2]) / CAM[0] * zz, (p[1] - CAM[3]) / CAM[1] * zz, zz])
                ends.append(R.T @ (Xc - t))
            fail = 0 if want[j] else 1 + j % 4
            if fail == 1: ends = [R.T @ (-(R @ e + t) - t) for e in ends]                      # behind the camera
            if fail == 2: ends[1] = R.T @ (np.array([5.0, 0.0, 1.0]) * (R @ ends[1] + t)[2] - t)     # u2 far to the right
            mid = 0.5 * (ends[0] + ends[1]); ow = -R.T @ t
            d = np.linalg.norm(mid - ow); nrm = (mid - ow) / d
            if fail == 4: nrm = -nrm
            mx, mn = F32(d * rng.uniform(1.3, 3.0)), F32(d * rng.uniform(0.3, 0.9))
            if fail == 3: mx, mn = F32(d * 0.5), F32(d * 0.2)
            pos = np.concatenate(ends)
            e, _, _, _ = is_in_frustum(pos, nrm, mx, mn, CAM, Rf, tf, Ow, BOUNDS, LOG_SF)
            assert (e == 0) == bool(want[j]), (j, e, fail)
            if e == 0:
                dist = F32(math.sqrt(sum(float(F32(F32(0.5) * F32(F32(pos[k]) + F32(pos[k + 3])) - Ow[k])) ** 2 for k in range(3))))
                x = float(predict_level_exact(mx, dist, LOG_SF))
                if abs(x - round(x)) < 1e-4:
                    rejected += 1; continue
            break
        M["pos"][j] = pos; M["normal"][j] = nrm; M["max_dist"][j] = mx; M["min_dist"][j] = mn
        w = ends[1] - ends[0]
        if axes is not None:
            w = np.asarray(axes, np.float64)[j % len(axes)] + rng.normal(0, 0.02, 3)
        M["wvec"][j] = w
    assert rejected * 100 < max(n, 100), rejected
    return M, rejected
