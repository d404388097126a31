"""CPU restatement of the point side of Tracking::TrackLocalMapWithLines: Tracking::SearchLocalPoints (reference src/Tracking.cc:3227-3277) with
Frame::isInFrustum(MapPoint *, 0.5) (src/Frame.cc:1371-1427), MapPoint::PredictScale (src/MapPoint.cc:400-415) and
ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-132) over Frame::GetFeaturesInArea (src/Frame.cc:1502-1555).  Test
infrastructure only: numpy float32 / float64 chosen operation by operation, one step per step of the reference, the search sequential.

Readings (OpenCV is not in the reference tree; DESIGN.md section 7 states the same ones):
  mRcw * P + mtcw            the row's products summed in float, left to right, then (float)((double)sum + (double)t)
  PcZ < 0.0f                 as written: z == 0 and -0.0 pass and divide; a NaN projection passes the four bounds tests
  invz, u, v, ur             one float division; fx * PcX * invz + cx in float, left to right; u - mbf * invz
  mOw                        -Rcw^T tcw: double sums, times -1.0, rounded to float
  P - mOw                    float, element-wise
  cv::norm                   sqrt of the double sum of squares, stored to float
  PO.dot(Pn) / dist          the dot product in double, the quotient in double, rounded to the float viewCos
  PredictScale               float ratio, float log, float division, float ceil (MapPoint.cc sits under `using namespace std`), then the
                             clamp to [0, n_levels - 1]; the conversion to int saturates and a NaN gives 0"""
import math

import numpy as np

F32 = np.float32
MAX_QUERIES, MAX_FEATURES, MAX_SLOTS = 16384, 65535, 1 << 20
FOREIGN_OBSERVED, FOREIGN_UNOBSERVED = -2, -3
COLS, ROWS = 64, 48
TH_HIGH = 100


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


def predict_scale(max_dist, dist, log_scale_factor, n_levels):
    with np.errstate(all="ignore"):
        n = to_int(np.ceil(predict_level_exact(max_dist, dist, log_scale_factor)))
    return 0 if n < 0 else (n_levels - 1 if n >= n_levels else n)


EXITS = ("in view", "PcZ < 0", "u < minX", "u > maxX", "v < minY", "v > maxY", "dist < 0.8 min", "dist > 1.2 max", "viewCos < limit")


def is_in_frustum(pos, normal, max_dist, min_dist, cam, R, t, Ow, bounds4, log_scale_factor, n_levels=8, limit=F32(0.5)):
    """-> (exit, (u, v, ur), view_cos, level): exit 0 = in view, else the index into EXITS of the condition that returned false"""
    fx, fy, cx, cy, bf = (F32(v) for v in cam[:5])
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    P = np.asarray(pos, np.float32)
    with np.errstate(all="ignore"):
        Pc = transform(R, t, P)
        if Pc[2] < F32(0.0): return 1, None, None, None
        invz = F32(F32(1.0) / Pc[2])
        u = F32(F32(F32(fx * Pc[0]) * invz) + cx); v = F32(F32(F32(fy * Pc[1]) * invz) + cy)
        if u < minX: return 2, None, None, None
        if u > maxX: return 3, None, None, None
        if v < minY: return 4, None, None, None
        if v > maxY: return 5, None, None, None
        maxD = F32(F32(1.2) * F32(max_dist)); minD = F32(F32(0.8) * F32(min_dist))
        d = [float(F32(P[k] - Ow[k])) for k in range(3)]
        dist = F32(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if dist < minD: return 6, None, None, None
        if dist > maxD: return 7, None, None, None
        pn = np.asarray(normal, np.float32)
        dot = (d[0] * float(pn[0]) + d[1] * float(pn[1])) + d[2] * float(pn[2])
        vc = F32(np.float64(dot) / np.float64(dist))
        if vc < F32(limit): return 8, None, None, None
        lvl = predict_scale(max_dist, dist, log_scale_factor, n_levels)
        ur = F32(u - F32(bf * invz))
    return 0, np.array([u, v, ur], np.float32), vc, lvl


def frustum_pass(M, cam, Tcw, bounds4, log_scale_factor, n_levels, held, seen_extra=(), limit=F32(0.5)):
    """the loops of Tracking.cc:3230-3264 -> dict(held (bad ones cleared), t_occupied, n_tested, slots, proj, view_cos, level, exits)"""
    ns = len(M["pos"]); bad = np.asarray(M["bad"]).astype(bool); obs = np.asarray(M["observed"]).astype(bool)
    held = np.asarray(held, np.int32).copy()
    seen = np.zeros(ns, bool)
    for i, h in enumerate(held):
        if h >= 0 and bad[h]: held[i] = -1
        elif h >= 0: seen[h] = True
    for e in seen_extra: seen[int(e)] = True
    t_occ = np.array([(h >= 0 and obs[h]) or h == FOREIGN_OBSERVED for h in held], np.uint8)
    R, t, Ow = pose_parts(Tcw)
    slots, proj, vcs, lvls, exits, nt = [], [], [], [], np.full(ns, -1, np.int32), 0
    for j in range(ns):
        if seen[j] or bad[j]: continue
        nt += 1
        e, p, vc, lv = is_in_frustum(M["pos"][j], M["normal"][j], M["max_dist"][j], M["min_dist"][j], cam, R, t, Ow, bounds4, log_scale_factor, n_levels, limit)
        exits[j] = e
        if e == 0:
            slots.append(j); proj.append(p); vcs.append(vc); lvls.append(lv)
    return dict(held=held, t_occupied=t_occ, n_tested=nt, slots=np.array(slots, np.int32), proj=np.array(proj, np.float32).reshape(-1, 3),
                view_cos=np.array(vcs, np.float32), level=np.array(lvls, np.int32), exits=exits)


def queries(M, fp):
    """the arrays hvo_search_by_projection_tracked takes, for the frustum pass's survivors: desc, u, v, ur, level, view_cos, blocks"""
    s = fp["slots"]
    return (np.asarray(M["desc"], np.uint8).reshape(-1, 32)[s], fp["proj"][:, 0].copy(), fp["proj"][:, 1].copy(), fp["proj"][:, 2].copy(), fp["level"], fp["view_cos"],
            np.asarray(M["observed"]).astype(np.uint8)[s])


# ---- ORBmatcher::SearchByProjection(F, vpMapPoints, th), sequential ----
def _round_away(v):
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


def build_grid(kp, bounds4):
    """Frame::AssignFeaturesToGrid with PosInGrid (src/Frame.cc:1680-1690): cell (ix, iy) -> feature indices in ascending order"""
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    invW = F32(F32(COLS) / F32(maxX - minX)); invH = F32(F32(ROWS) / F32(maxY - minY))
    grid = {}
    for i in range(len(kp)):
        px = _round_away(F32(F32(kp["x"][i] - minX) * invW)); py = _round_away(F32(F32(kp["y"][i] - minY) * invH))
        if px < 0 or px >= COLS or py < 0 or py >= ROWS: continue
        grid.setdefault((px, py), []).append(i)
    return grid, invW, invH


def features_in_area(kp, grid, invW, invH, bounds4, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea: the indices in its visiting order (cells by column, then row, then insertion order)"""
    minX, minY = F32(bounds4[0]), F32(bounds4[2])
    x, y, r = F32(x), F32(y), F32(r)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(r)): return []          # (the C conversion of a NaN to int is undefined; no |d| < r holds)
    cx0 = max(0, int(math.floor(F32(F32(F32(x - minX) - r) * invW))))
    if cx0 >= COLS: return []
    cx1 = min(COLS - 1, int(math.ceil(F32(F32(F32(x - minX) + r) * invW))))
    if cx1 < 0: return []
    cy0 = max(0, int(math.floor(F32(F32(F32(y - minY) - r) * invH))))
    if cy0 >= ROWS: return []
    cy1 = min(ROWS - 1, int(math.ceil(F32(F32(F32(y - minY) + r) * invH))))
    if cy1 < 0: return []
    check = min_level > 0 or max_level >= 0
    out = []
    for ix in range(cx0, cx1 + 1):
        for iy in range(cy0, cy1 + 1):
            for j in grid.get((ix, iy), ()):
                o = int(kp["octave"][j])
                if check:
                    if o < min_level: continue
                    if max_level >= 0 and o > max_level: continue
                if abs(F32(kp["x"][j] - x)) < r and abs(F32(kp["y"][j] - y)) < r:
                    out.append(j)
    return out


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def search_by_projection(q_desc, q_u, q_v, q_ur, q_level, q_vc, q_blocks, t_kp, t_uright, t_occupied, t_desc, bounds4, th, scale_factors, th_high=TH_HIGH,
                         nn_ratio=0.8):
    """ORBmatcher.cc:45-132 over the in-view list, in order.  t_occupied[j]: feature j holds a point with observations; a match by a query with
    q_blocks set makes its feature occupied for the queries after it -> (nmatches, match_idx, match_dist)"""
    nq = len(q_u)
    grid, invW, invH = build_grid(t_kp, bounds4)
    occ = np.asarray(t_occupied).astype(bool).copy()
    mi = np.full(nq, -1, np.int32); md = np.full(nq, 256, np.int32); nm = 0
    t_desc = np.asarray(t_desc, np.uint8).reshape(-1, 32)
    for i in range(nq):
        lvl = int(q_level[i])
        r = F32(2.5) if float(q_vc[i]) > 0.998 else F32(4.0)
        if F32(th) != F32(1.0): r = F32(r * F32(th))
        rad = F32(r * F32(scale_factors[lvl]))
        idxs = features_in_area(t_kp, grid, invW, invH, bounds4, q_u[i], q_v[i], rad, lvl - 1, lvl)
        if not idxs: continue
        best, best2, lev, lev2, bidx = 256, 256, -1, -1, -1
        for j in idxs:
            if occ[j]: continue
            if t_uright is not None and t_uright[j] > 0:
                if abs(F32(q_ur[i] - t_uright[j])) > rad: continue
            d = int(_POP[q_desc[i] ^ t_desc[j]].sum())
            if d < best:
                best2, best, lev2, lev, bidx = best, d, lev, int(t_kp["octave"][j]), j
            elif d < best2:
                lev2, best2 = int(t_kp["octave"][j]), d
        if best <= th_high:
            if lev == lev2 and F32(best) > F32(F32(nn_ratio) * F32(best2)): continue
            mi[i] = bidx; md[i] = best; nm += 1
            if q_blocks[i]: occ[bidx] = True
    return nm, mi, md


def search_local_points(M, cam, Tcw, bounds4, log_scale_factor, n_levels, scale_factors, th, t_kp, t_uright, t_desc, held, seen_extra=(), th_high=TH_HIGH,
                        nn_ratio=0.8, limit=F32(0.5), search=None):
    """the whole call.  M: dict(pos, normal (n, 3) float32, max_dist, min_dist (n), desc (n, 32), bad, observed (n)) -> dict as the library's result"""
    fp = frustum_pass(M, cam, Tcw, bounds4, log_scale_factor, n_levels, held, seen_extra, limit)
    nq = len(fp["slots"]); nt = len(t_kp)
    out = dict(n_slots_tested=fp["n_tested"], n_in_view=nq, in_view_slot=fp["slots"], proj=fp["proj"], view_cos=fp["view_cos"], level=fp["level"],
               status=0, n_matches=0, match_idx=np.full(nq, -1, np.int32), match_dist=np.full(nq, 256, np.int32))
    if nq > MAX_QUERIES:
        out.update(status=-4, held=np.asarray(held, np.int32).copy()); return out
    held = fp["held"].copy()
    if nq > 0 and nt > 0:
        q = queries(M, fp)
        fn = search or search_by_projection
        nm, mi, md = fn(q[0], q[1], q[2], q[3], q[4], q[5], q[6], t_kp, t_uright, fp["t_occupied"], t_desc, bounds4, th, scale_factors, th_high, nn_ratio)
        out.update(n_matches=nm, match_idx=np.asarray(mi, np.int32), match_dist=np.asarray(md, np.int32))
        for k in range(nq):
            if mi[k] >= 0: held[mi[k]] = fp["slots"][k]                 # F.mvpMapPoints[bestIdx] = pMP: the later one in order keeps it
    out["held"] = held
    return out


# ---- scenes for the GPU tests (and the CPU checks of the generator itself) ----
CAM = (535.4, 539.2, 320.1, 247.6, 40.0)          # fx, fy, cx, cy, bf
BOUNDS = (0.0, 640.0, 0.0, 480.0)                 # mnMinX, mnMaxX, mnMinY, mnMaxY
LOG_SF = float(F32(np.log(F32(1.2))))
N_LEVELS = 8
SF = np.cumprod(np.concatenate([[F32(1.0)], np.full(7, F32(1.2), F32)])).astype(F32)      # mvScaleFactors of the default 8-level pyramid
DEPTH_FACTOR = F32(1.0 / 5000.0)
PATTERNS = ("none", "all", "alt", "wave", "last")


def scene_pose(seed=0):
    """a camera rotated a few degrees about y and x, off the origin (nothing special about it)"""
    a, b = np.radians(6.0 + 2.0 * seed), np.radians(4.0)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]); Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return np.hstack([Rx @ Ry, np.array([[0.3], [-0.2], [0.5]])]).astype(np.float32)


def estimated_pose(Tcw, dx=0.01):
    """the pose a tracker would search under: the true one with the camera a centimetre off along x"""
    T = np.asarray(Tcw, np.float32).copy(); T[0, 3] = F32(T[0, 3] + F32(dx))
    return T


def wanted_in_view(n, pattern):
    j = np.arange(n)
    return {"none": j < 0, "all": j >= 0, "alt": j % 2 == 0, "wave": j % 64 == 5, "last": j == n - 1}[pattern]


def empty_map(n, seed=1):
    rng = np.random.RandomState(seed)
    return dict(pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), max_dist=np.zeros(n, np.float32), min_dist=np.zeros(n, np.float32),
                desc=rng.randint(0, 256, (n, 32)).astype(np.uint8), bad=np.zeros(n, np.uint8), observed=(rng.rand(n) < 0.7).astype(np.uint8))


def level_guard(max_dist, dist, log_scale_factor=LOG_SF):
    """True when log(ratio) / logScaleFactor lies within 1e-4 of an integer (the predicted level goes through a library log)"""
    x = float(predict_level_exact(max_dist, dist, log_scale_factor))
    return not math.isfinite(x) or abs(x - round(x)) < 1e-4


def _dist(pos, Ow):
    d = [float(F32(F32(pos[k]) - Ow[k])) for k in range(3)]
    return F32(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def make_map(n, pattern, Tcw, seed=1, cam=CAM, bounds4=BOUNDS):
    """n map points of which exactly the slots of `pattern` are in view under Tcw; the others fail isInFrustum for one of four reasons in turn
    (behind the camera, outside the image, out of the distance range, seen from behind).  A point in view whose log(ratio) / logScaleFactor
    lies within 1e-4 of an integer is drawn again; fewer than 1 % may be rejected -> (map dict, rejected count)"""
    rng = np.random.RandomState(seed)
    T = np.asarray(Tcw, np.float64).reshape(3, 4); R, t = T[:, :3], T[:, 3]
    want = wanted_in_view(n, pattern)
    M = empty_map(n, seed)
    Rf, tf, Ow = pose_parts(Tcw)
    ow = -R.T @ t
    rejected = 0
    for j in range(n):
        while True:
            uv = np.array([rng.uniform(40, 600), rng.uniform(40, 440)]); z = rng.uniform(1.0, 4.0)
            Xc = np.array([(uv[0] - cam[2]) / cam[0] * z, (uv[1] - cam[3]) / cam[1] * z, z])
            fail = 0 if want[j] else 1 + (j // 2) % 4
            if fail == 1: Xc = -Xc                                          # behind the camera
            if fail == 2: Xc = np.array([5.0 * z, Xc[1], z])               # u far to the right
            X = (R.T @ (Xc - t)).astype(np.float32)
            d = np.linalg.norm(X.astype(np.float64) - ow); nrm = (X.astype(np.float64) - ow) / d
            if fail == 4: nrm = -nrm
            mx, mn = F32(d * rng.uniform(1.3, 3.0)), F32(d * rng.uniform(0.3, 0.9))
            if fail == 3: mx, mn = F32(d * 0.5), F32(d * 0.2)
            nrm = nrm.astype(np.float32)
            e = is_in_frustum(X, nrm, mx, mn, cam, Rf, tf, Ow, bounds4, LOG_SF, N_LEVELS)[0]
            assert (e == 0) == bool(want[j]), (j, e, fail)
            if e == 0 and level_guard(mx, _dist(X, Ow)):
                rejected += 1; continue
            break
        M["pos"][j] = X; M["normal"][j] = nrm; M["max_dist"][j] = mx; M["min_dist"][j] = mn
    assert rejected * 100 < max(n, 100), rejected
    return M, rejected


def stereo_from_depth(kp, kp_un, depth, bf, dfac=DEPTH_FACTOR):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:1940-1961) as k_stereo_from_rgbd states it -> (mvuRight, mvDepth)"""
    n = len(kp); ur = np.full(n, -1, np.float32); z = np.full(n, -1, np.float32)
    h, w = depth.shape
    for i in range(n):
        v, u = int(kp["y"][i]), int(kp["x"][i])
        if 0 <= u < w and 0 <= v < h:
            d = F32(F32(depth[v, u]) * F32(dfac))
            if d > 0 and float(d) < 7.0:
                z[i] = d; ur[i] = F32(kp_un["x"][i] - F32(F32(bf) / d))
    return ur, z


def add_frame_points(M, kp_un, desc, zdepth, Tcw, slots, cam=CAM, pool=None, feats=None):
    """overwrite `slots` of the map with the frame's own key points that have depth, unprojected and seen from Tcw, so that the search has
    something to find: slot slots[k] is feature feats[k] (default: the features with depth in order, cycled).  mfMaxDistance is the distance
    times the octave's scale factor, divided by sqrt(1.2): log(ratio) / logScaleFactor = octave - 0.5, half a level from the integers, so the
    predicted level is the feature's octave -> the feature of every slot written"""
    T = np.asarray(Tcw, np.float64).reshape(3, 4); R, t = T[:, :3], T[:, 3]
    ow = -R.T @ t
    good = np.nonzero(zdepth > 0)[0]
    used = []
    for k, j in enumerate(slots):
        i = int(good[k % len(good)] if feats is None else feats[k])
        z = float(zdepth[i])
        Xc = np.array([(float(kp_un["x"][i]) - cam[2]) / cam[0] * z, (float(kp_un["y"][i]) - cam[3]) / cam[1] * z, z])
        X = (R.T @ (Xc - t)).astype(np.float32)
        d = np.linalg.norm(X.astype(np.float64) - ow)
        M["pos"][j] = X; M["normal"][j] = ((X.astype(np.float64) - ow) / d).astype(np.float32)
        M["max_dist"][j] = F32(d * float(SF[int(kp_un["octave"][i])]) / math.sqrt(1.2)); M["min_dist"][j] = F32(M["max_dist"][j] / SF[N_LEVELS - 1])
        M["desc"][j] = desc[i] if pool is None else pool[k % len(pool)]
        used.append(i)
    return np.array(used, np.int32)


# ---- crafted slots: every gate of isInFrustum alone, under poses whose arithmetic is exact ----
# The pose is an axis permutation with a dyadic translation (crafted_pose), the camera dyadic too.
CAM2 = (512.0, 512.0, 320.0, 240.0, 64.0)         # with z = 2: u = 256 x + 320, v = 256 y + 240, ur = u - 32


def crafted_pose(tz=2.0, ty=-0.25):
    """Xc = (Yw + 0.5, Zw + ty, Xw + tz); mOw = (-tz, -0.5, -ty)"""
    return np.array([[0, 1, 0, 0.5], [0, 0, 1, ty], [1, 0, 0, tz]], np.float32)


def crafted_world(xc, yc, zc):
    """the world point whose camera coordinates under crafted_pose() are (xc, yc, zc), exactly for the values used here"""
    return np.array([F32(zc) - F32(2.0), F32(xc) - F32(0.5), F32(yc) + F32(0.25)], np.float32)


def crafted_gates():
    """-> (poses, rows): rows of (name, pose key, pos, normal, mfMaxDistance, mfMinDistance, the exit expected under that pose).  Under pose "A"
    z = 2 for the bounds rows (u = 256 x + 320, v = 256 y + 240: 2^-20 in x moves u by 2^-12) and P lies on the optical axis for the distance and
    angle rows (PO = (z, 0, 0), dist = z, viewCos = the normal's x).  "B": tz = 0; "C": tz = -0.0 with every product of the row -0; "D": tz = -2^-20"""
    poses = dict(A=crafted_pose(), B=crafted_pose(0.0), C=crafted_pose(-0.0, 0.25), D=crafted_pose(-2.0 ** -20))
    eps = 2.0 ** -20
    n1 = (1.0, 0.0, 0.0)
    rows = []
    for name, x, y, e in (("u on max", 1.25, 0, 0), ("u beyond max", 1.25 + eps, 0, 3), ("u on min", -1.25, 0, 0), ("u beyond min", -1.25 - eps, 0, 2),
                          ("v on max", 0, 0.9375, 0), ("v beyond max", 0, 0.9375 + eps, 5), ("v on min", 0, -0.9375, 0), ("v beyond min", 0, -0.9375 - eps, 4)):
        rows.append((name, "A", crafted_world(x, y, 2.0), (1.0, 0.25, 0.25), 8.0, 0.5, e))
    zmax = F32(F32(1.2) * F32(2.0)); zmin = F32(F32(0.8) * F32(2.0))
    rows += [("dist on max", "A", crafted_world(0, 0, zmax), n1, 2.0, 0.5, 0), ("dist beyond max", "A", crafted_world(0, 0, zmax), n1, np.nextafter(F32(2.0), F32(0)), 0.5, 7),
             ("dist on min", "A", crafted_world(0, 0, zmin), n1, 8.0, 2.0, 0), ("dist below min", "A", crafted_world(0, 0, zmin), n1, 8.0, np.nextafter(F32(2.0), F32(3)), 6),
             ("viewCos on limit", "A", crafted_world(0, 0, 2.0), (0.5, 7.0, -3.0), 4.0, 1.0, 0),
             ("viewCos below limit", "A", crafted_world(0, 0, 2.0), (np.nextafter(F32(0.5), F32(0)), 7.0, -3.0), 4.0, 1.0, 8),
             ("level clamped high", "A", crafted_world(0, 0, 2.0), n1, 2.0 * 1.2 ** 30, 0.1, 0), ("level clamped low", "A", crafted_world(0, 0, zmax), n1, 2.0, 0.1, 0),
             ("behind", "A", crafted_world(0, 0, -1.0), (-1.0, 0, 0), 8.0, 0.1, 1),
             # z == 0: X = Y = 0 gives NaN projections, which pass the bounds tests; X != 0 gives an infinite u
             ("z = 0, NaN", "B", (0.0, -0.5, 0.25), (0.0, 0.0, 0.0), 1e9, 0.0, 0), ("z = 0, u = +inf", "B", (0.0, 0.5, 0.25), (0.0, 0.0, 0.0), 1e9, 0.0, 3),
             ("z = -0.0, NaN", "C", (-0.0, -0.5, -0.25), (0.0, 0.0, 0.0), 1e9, 0.0, 0),
             ("z just below 0", "D", (0.0, -0.5, 0.25), (0.0, 0.0, 0.0), 1e9, 0.0, 1)]
    return poses, rows


def crafted_map(rows, seed=5):
    M = empty_map(len(rows), seed)
    for j, (_, _, pos, nrm, mx, mn, _) in enumerate(rows):
        M["pos"][j] = np.asarray(pos, np.float32); M["normal"][j] = np.asarray(nrm, np.float32); M["max_dist"][j] = F32(mx); M["min_dist"][j] = F32(mn)
    return M
