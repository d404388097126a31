"""CPU restatement of ORBmatcher::Fuse(KeyFrame *, const vector<MapPoint *> &, float th) (reference src/ORBmatcher.cc:838-994) with
KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:627-666), KeyFrame::IsInImage (:780-783) and MapPoint::PredictScale(dist, KeyFrame *)
(src/MapPoint.cc:383-398).  Test infrastructure only: numpy float32 / float64 chosen operation by operation, one step per step of the
reference, the loops sequential.  GetFeaturesInArea walks REAL per-cell lists (point_map_ref.build_grid) in the reference's order; the
device walks a column-major CSR, so the two formulations check each other.

Readings (OpenCV is not in the reference tree; csrc/fuse.hip and DESIGN.md section 7 state the same ones):
  Rcw * p3Dw + tcw       point_map_ref.transform
  z < 0.0f               as written: z == 0 and -0.0 pass and divide
  invz = 1 / z           one FLOAT division (the text has the int literal 1)
  u = fx * x + cx        x = X * invz: two float products
  IsInImage              u >= minX && u < maxX && v >= minY && v < maxY: a NaN fails
  ur = u - bf * invz     float
  Ow, p3Dw - Ow, norm    point_map_ref.pose_parts; float difference; sqrt of the double sum of squares, stored to float
  PO.dot(Pn)             double accumulation in order, compared with the double 0.5 * dist3D
  PredictScale           point_map_ref.predict_scale on the RAW mfMaxDistance
  radius                 th * mvScaleFactors[level], a float product
  cell range             as written, in addition to the two fabs tests
  e2                     float, left to right; e2 * mvInvLevelSigma2[octave] a float product compared with the double 7.8 / 5.99;
                         mvuRight[idx] >= 0 chooses (a NaN takes the mono gate); a negative octave is in no band"""
import math

import numpy as np

import point_map_ref as pm

F32 = np.float32
MAX_FEATURES, MAX_ENTRIES = 65535, 1 << 20
GATES = ("searched", "skip", "behind", "out of image", "dist < 0.8 min", "dist > 1.2 max", "view angle")
SEARCHED, SKIP, BEHIND, OUT_OF_IMAGE, DIST_MIN, DIST_MAX, VIEW_ANGLE = range(7)
TH, TH_LOW = 3.0, 50
INV_SIGMA2 = (F32(1.0) / (pm.SF * pm.SF)).astype(F32)             # mvInvLevelSigma2 of the default 8-level pyramid (ORBextractor.cc:428-436)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def project_entry(P, normal, max_dist, min_dist, R, t, Ow, cam, bounds4, log_scale_factor, n_levels):
    """lines 865-900 for one entry -> (gate, (u, v, ur) as far as computed, level or -1)"""
    fx, fy, cx, cy, bf = (F32(v) for v in cam[:5])
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    z3 = (F32(0), F32(0), F32(0))
    with np.errstate(all="ignore"):
        Pc = pm.transform(R, t, P)
        if Pc[2] < F32(0.0): return BEHIND, z3, -1
        invz = F32(F32(1.0) / Pc[2])
        x = F32(Pc[0] * invz); y = F32(Pc[1] * invz)
        u = F32(F32(fx * x) + cx); v = F32(F32(fy * y) + cy)
        if not (u >= minX and u < maxX and v >= minY and v < maxY): return OUT_OF_IMAGE, (u, v, F32(0)), -1
        ur = F32(u - F32(bf * invz))
        maxD = F32(F32(1.2) * F32(max_dist)); minD = F32(F32(0.8) * F32(min_dist))
        d = [float(F32(P[k] - Ow[k])) for k in range(3)]
        dist = F32(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if dist < minD: return DIST_MIN, (u, v, ur), -1
        if dist > maxD: return DIST_MAX, (u, v, ur), -1
        dot = (d[0] * float(normal[0]) + d[1] * float(normal[1])) + d[2] * float(normal[2])
        if dot < 0.5 * float(dist): return VIEW_ANGLE, (u, v, ur), -1
        return SEARCHED, (u, v, ur), pm.predict_scale(max_dist, dist, log_scale_factor, n_levels)


def features_in_area(kp, grid, invW, invH, bounds4, x, y, r):
    """KeyFrame::GetFeaturesInArea: the indices in its visiting order (ix outer, iy inner, then the cell's vector)"""
    minX, minY = F32(bounds4[0]), F32(bounds4[2])
    x, y, r = F32(x), F32(y), F32(r)
    with np.errstate(all="ignore"):
        cx0 = max(0, pm.to_int(np.floor(F32(F32(F32(x - minX) - r) * invW))))
        if cx0 >= pm.COLS: return []
        cx1 = min(pm.COLS - 1, pm.to_int(np.ceil(F32(F32(F32(x - minX) + r) * invW))))
        if cx1 < 0: return []
        cy0 = max(0, pm.to_int(np.floor(F32(F32(F32(y - minY) - r) * invH))))
        if cy0 >= pm.ROWS: return []
        cy1 = min(pm.ROWS - 1, pm.to_int(np.ceil(F32(F32(F32(y - minY) + r) * invH))))
        if cy1 < 0: return []
        out = []
        for ix in range(cx0, cx1 + 1):
            for iy in range(cy0, cy1 + 1):
                for j in grid.get((ix, iy), ()):
                    if abs(F32(kp["x"][j] - x)) < r and abs(F32(kp["y"][j] - y)) < r: out.append(j)
    return out


def chi2_pass(u, v, ur, kpx, kpy, kpr, inv_sigma2):
    """lines 927-951 for one candidate: True when it survives the gate"""
    with np.errstate(all="ignore"):
        ex = F32(u - kpx); ey = F32(v - kpy)
        if kpr >= 0:
            er = F32(ur - kpr)
            e2 = F32(F32(F32(ex * ex) + F32(ey * ey)) + F32(er * er))
            return not (float(F32(e2 * inv_sigma2)) > 7.8)
        e2 = F32(F32(ex * ex) + F32(ey * ey))
        return not (float(F32(e2 * inv_sigma2)) > 5.99)


def fuse(kf, mp, cam, bounds4=pm.BOUNDS, th=TH, th_low=TH_LOW, log_scale_factor=pm.LOG_SF, n_levels=pm.N_LEVELS, scale_factors=pm.SF, inv_sigma2=INV_SIGMA2):
    """one Fuse call.  kf = dict(kp_un, uright (or None), desc, Tcw, skip (or None)); mp = dict(pos, normal, max_dist, min_dist, desc) ->
    dict as the library's result plus n_cand (candidates that reached the descriptor) and n_ties (candidates at the final best distance)"""
    kp = kf["kp_un"]; nt = len(kp); n = len(mp["pos"])
    ur_t = None if kf.get("uright") is None else np.asarray(kf["uright"], np.float32)
    t_desc = np.asarray(kf["desc"], np.uint8).reshape(-1, 32); q_desc = np.asarray(mp["desc"], np.uint8).reshape(-1, 32)
    skip = np.zeros(n, bool) if kf.get("skip") is None else np.asarray(kf["skip"]).astype(bool)
    R, t, Ow = pm.pose_parts(kf["Tcw"])
    grid, invW, invH = pm.build_grid(kp, bounds4)
    bi = np.full(n, -1, np.int32); bd = np.full(n, 256, np.int32); gate = np.full(n, SKIP, np.int8); level = np.full(n, -1, np.int32)
    proj = np.zeros((n, 3), np.float32); n_cand = np.zeros(n, np.int32); n_ties = np.zeros(n, np.int32)
    pos = np.asarray(mp["pos"], np.float32).reshape(-1, 3); nrm = np.asarray(mp["normal"], np.float32).reshape(-1, 3)
    for i in range(n):
        if skip[i]: continue
        g, p3, lvl = project_entry(pos[i], nrm[i], mp["max_dist"][i], mp["min_dist"][i], R, t, Ow, cam, bounds4, log_scale_factor, n_levels)
        gate[i] = g; proj[i] = p3; level[i] = lvl
        if g != SEARCHED: continue
        u, v, ur = p3
        radius = F32(F32(th) * F32(scale_factors[lvl]))
        best, bidx, dists = 256, -1, []
        for j in features_in_area(kp, grid, invW, invH, bounds4, u, v, radius):
            o = int(kp["octave"][j])
            if o < lvl - 1 or o > lvl or o < 0: continue
            kpr = F32(-1.0) if ur_t is None else ur_t[j]
            if not chi2_pass(u, v, ur, kp["x"][j], kp["y"][j], kpr, F32(inv_sigma2[o])): continue
            d = int(_POP[q_desc[i] ^ t_desc[j]].sum())
            dists.append(d)
            if d < best: best, bidx = d, j
        bi[i] = bidx; bd[i] = best; n_cand[i] = len(dists); n_ties[i] = sum(1 for d in dists if d == best and best < 256)
    fe = np.flatnonzero(bd <= th_low).astype(np.int32)
    return dict(best_idx=bi, best_dist=bd, gate=gate, level=level, proj=proj, fused_entry=fe, fused_idx=bi[fe], n_fused=len(fe),
                n_searched=int((gate == SEARCHED).sum()), status=0, n_cand=n_cand, n_ties=n_ties)


# ---- crafted entries under point_map_ref.crafted_pose() with CAM2, where the arithmetic is exact ----
CAM2 = pm.CAM2                                    # (512, 512, 320, 240, 64): with z = 2, u = 256 x + 320, v = 256 y + 240, ur = u - 32
T_CRAFTED = pm.crafted_pose()                     # Xc = (Yw + 0.5, Zw - 0.25, Xw + 2); Ow = (-2, -0.5, 0.25)
world = pm.crafted_world
N_TOWARDS = np.array([1.0, 0.0, 0.0], np.float32)  # a normal along PO for a point on the optical axis (PO = (z, 0, 0) in world axes)


def _dist(pos):
    _, _, Ow = pm.pose_parts(T_CRAFTED)
    return pm._dist(np.asarray(pos, np.float32), Ow)


def max_dist_for_level(dist, l):
    """mfMaxDistance for which log(ratio) / logScaleFactor = l - 0.5: half a level from the integers, the predicted level is l"""
    return F32(float(dist) * float(pm.SF[l]) / math.sqrt(1.2))


def normal_of(pos):
    """a unit normal along PO: PO.dot(Pn) = dist3D, far from the gate"""
    _, _, Ow = pm.pose_parts(T_CRAFTED)
    d = np.asarray(pos, np.float64) - Ow.astype(np.float64)
    return (d / max(np.linalg.norm(d), 1e-30)).astype(np.float32)


def crafted_gates():
    """-> rows of (name, pos, normal, mfMaxDistance, mfMinDistance, skip, expected gate, expected (u, v, ur) or None, expected level or None)"""
    eps = 2.0 ** -20
    rows = []
    on = lambda x, y, z=2.0: world(x, y, z)
    for name, x, y, g in (("u on min", -1.25, 0, 0), ("u below min", -1.25 - eps, 0, 3), ("u just below max", 1.25 - eps, 0, 0), ("u on max", 1.25, 0, 3),
                          ("v on min", 0, -0.9375, 0), ("v below min", 0, -0.9375 - eps, 3), ("v just below max", 0, 0.9375 - eps, 0), ("v on max", 0, 0.9375, 3)):
        p = on(x, y)
        uv = (F32(256 * x + 320), F32(256 * y + 240))
        rows.append((name, p, normal_of(p), 8.0, 0.5, 0, g, (uv[0], uv[1], F32(uv[0] - 32) if g == 0 else F32(0)), None))
    zmax = F32(F32(1.2) * F32(2.0)); zmin = F32(F32(0.8) * F32(2.0))
    ax = lambda z: world(0, 0, z)
    half = np.array([0.5, math.sqrt(0.75), 0.0], np.float32)       # PO = (z, 0, 0): dot = 0.5 z exactly
    rows += [("skipped", ax(2.0), N_TOWARDS, 4.0, 1.0, 1, SKIP, (0.0, 0.0, 0.0), None),
             ("skipped, NaN position", np.array([np.nan] * 3, np.float32), N_TOWARDS, np.nan, np.nan, 1, SKIP, (0.0, 0.0, 0.0), None),
             ("behind", ax(-2.0), N_TOWARDS, 4.0, 1.0, 0, BEHIND, (0.0, 0.0, 0.0), None),
             ("z = 0: NaN projection fails IsInImage", ax(0.0), N_TOWARDS, 1e9, 0.0, 0, OUT_OF_IMAGE, None, None),
             ("z = 0, u = +inf", world(1.0, 0, 0.0), N_TOWARDS, 1e9, 0.0, 0, OUT_OF_IMAGE, (np.inf, None, 0.0), None),
             ("NaN position", np.array([np.nan, 0, 0], np.float32), N_TOWARDS, 4.0, 1.0, 0, OUT_OF_IMAGE, None, None),
             ("dist on max", ax(zmax), N_TOWARDS, 2.0, 0.5, 0, 0, (320.0, 240.0, None), 0),
             ("dist beyond max", ax(zmax), N_TOWARDS, np.nextafter(F32(2.0), F32(0)), 0.5, 0, DIST_MAX, (320.0, 240.0, None), None),
             ("dist on min", ax(zmin), N_TOWARDS, 8.0, 2.0, 0, 0, (320.0, 240.0, None), None),
             ("dist below min", ax(zmin), N_TOWARDS, 8.0, np.nextafter(F32(2.0), F32(3)), 0, DIST_MIN, (320.0, 240.0, None), None),
             ("view angle on the limit", ax(2.0), half, 4.0, 1.0, 0, 0, (320.0, 240.0, 288.0), None),
             ("view angle below the limit", ax(2.0), np.array([np.nextafter(F32(0.5), F32(0)), math.sqrt(0.75), 0.0], np.float32), 4.0, 1.0, 0, VIEW_ANGLE, (320.0, 240.0, 288.0), None),
             ("level clamped high", ax(2.0), N_TOWARDS, 2.0 * 1.2 ** 30, 0.1, 0, 0, (320.0, 240.0, 288.0), 7),
             ("level clamped low", ax(zmax), N_TOWARDS, 2.0, 0.1, 0, 0, (320.0, 240.0, None), 0),
             ("level 4", world(0.5, 0.25, 2.0), normal_of(world(0.5, 0.25, 2.0)), 4.0, 1.0, 0, 0, (448.0, 304.0, 416.0), 4)]
    return rows


def rows_map(rows, seed=5):
    rng = np.random.RandomState(seed)
    n = len(rows)
    mp = dict(pos=np.stack([np.asarray(r[1], np.float32) for r in rows]), normal=np.stack([np.asarray(r[2], np.float32) for r in rows]),
              max_dist=np.array([r[3] for r in rows], np.float32), min_dist=np.array([r[4] for r in rows], np.float32),
              desc=rng.randint(0, 256, (n, 32)).astype(np.uint8))
    return mp, np.array([r[5] for r in rows], np.uint8)


BASE = np.arange(32, dtype=np.uint8) * 7 + 3


def flip(k, base=BASE):
    """base with its first k bits flipped: Hamming distance k"""
    bits = np.unpackbits(base); bits[:k] ^= 1
    return np.packbits(bits)


def hand_scene(kp_dt, entries, feats, uright=True, level=1):
    """entries: (u, v, descriptor) at z = 2 on the crafted pose with predicted level `level` (ur = u - 32); feats: (x, y, octave, descriptor,
    uright or None = -1) -> (kf, mp)"""
    n, nt = len(entries), len(feats)
    pos = np.zeros((n, 3), np.float32); mx = np.zeros(n, np.float32); nrm = np.zeros((n, 3), np.float32)
    for i, e in enumerate(entries):
        pos[i] = world((e[0] - 320.0) / 256.0, (e[1] - 240.0) / 256.0, 2.0); mx[i] = max_dist_for_level(_dist(pos[i]), level); nrm[i] = normal_of(pos[i])
    kp = np.zeros(nt, kp_dt); kp["size"] = 31; kp["class_id"] = -1
    ur = np.full(nt, -1.0, np.float32)
    for j, f in enumerate(feats):
        kp["x"][j], kp["y"][j], kp["octave"][j] = f[0], f[1], f[2]
        if len(f) > 4 and f[4] is not None: ur[j] = f[4]
    kf = dict(kp_un=kp, uright=ur if uright else None, desc=np.stack([f[3] for f in feats]) if nt else np.zeros((0, 32), np.uint8), Tcw=T_CRAFTED, skip=None)
    mp = dict(pos=pos, normal=nrm, max_dist=mx, min_dist=(mx / pm.SF[7]).astype(F32), desc=np.stack([e[2] for e in entries]))
    return kf, mp


def step(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


def chi2_cases(kp_dt):
    """the two gates at one float step of the feature's coordinate on either side of the literals.  Level 0 (mvInvLevelSigma2 = 1): entry k
    at (u, v) = (64 + 96 k, 240), ur = u - 32, with one feature of its own: a mono feature at (x, 240) has e2 = (u - x)^2, a stereo feature
    at (u, 240) with mvuRight r has e2 = (ur - r)^2.  x and r are two ADJACENT floats: the last for which the float e2 is <= the double
    literal and the first for which it is above -> (kf, mp, expected survival per feature)"""
    def around(c, lit):
        """adjacent floats (a, b) below c: with e = float(c - a), float(e * e) <= lit, and with e = float(c - b), float(e * e) > lit"""
        sq = lambda a: float(F32(F32(F32(c) - a) * F32(F32(c) - a)))
        a = F32(c - math.sqrt(lit))
        while sq(a) > lit: a = step(a, True)
        while sq(step(a, False)) <= lit: a = step(a, False)
        assert sq(a) <= lit < sq(step(a, False))
        return a, step(a, False)
    ent, feats, want = [], [], []
    for k in range(5):
        u0, v0 = 64.0 + 96.0 * k, 240.0
        ent.append((u0, v0, BASE))
        m_in, m_out = around(u0, 5.99); s_in, s_out = around(u0 - 32.0, 7.8)
        x, r, ok = ((m_in, None, True), (m_out, None, False), (F32(u0), s_in, True), (F32(u0), s_out, False),
                    (m_out, F32(u0 - 32.0), True))[k]               # the last: e2 > 5.99 with mvuRight >= 0 and er = 0 passes the stereo gate
        feats.append((x, v0, 0, flip(3 + k), r))
        want.append(ok)
    kf, mp = hand_scene(kp_dt, ent, feats, level=0)
    return kf, mp, want


def tie_cases(kp_dt):
    """equal descriptors at equal distance.  Cells are 10 x 10 px on the 640 x 480 bounds, cell = round(x / 10); level 1, radius 3.6.
    Entry 0 at (204, 200) looks at the columns 20 and 21: feature 0 at (206, 200) lies in column 21, feature 1 at (203, 200) in column 20:
    the HIGHER index is visited first and wins.  Entry 1 at (400, 200): features 2 and 3 at (401, 200) and (402, 201), both in cell
    (40, 20): the lower index wins.  Feature 4 at (636, 100) rounds to column 64 > 63: it is in no cell, and entry 2 at (634, 100), 2 px
    away, inside the radius, the band and the chi-square gate, never finds it -> (kf, mp); best_idx = [1, 2, -1]"""
    d = flip(9)
    ent = [(204.0, 200.0, BASE), (400.0, 200.0, BASE), (634.0, 100.0, BASE)]
    feats = [(206.0, 200.0, 1, d), (203.0, 200.0, 1, d), (401.0, 200.0, 1, d), (402.0, 201.0, 1, d), (636.0, 100.0, 1, d)]
    return hand_scene(kp_dt, ent, feats, uright=False)


# ---- random scenes ----
SCENE_SEED = 11


def random_keyframe(kp_dt, nt, seed, crowd=0):
    """nt key points on 640 x 480 with octaves, mvuRight (a third -1) and random descriptors; the first `crowd` of them packed into the one cell
    around (300, 200)"""
    rng = np.random.RandomState(seed)
    kp = np.zeros(nt, kp_dt); kp["size"] = 31; kp["class_id"] = -1
    kp["x"] = rng.uniform(8, 632, nt).astype(F32); kp["y"] = rng.uniform(8, 472, nt).astype(F32)
    kp["octave"] = rng.choice(8, nt, p=[0.26, 0.2, 0.16, 0.12, 0.1, 0.07, 0.05, 0.04])
    c = min(crowd, nt)
    # cell (30, 20) holds x in [295, 305), y in [195, 205); the margins leave room for random_scene's twins (+0.75, -0.5)
    kp["x"][:c] = rng.uniform(296.0, 303.5, c).astype(F32); kp["y"][:c] = rng.uniform(196.5, 204.0, c).astype(F32); kp["octave"][:c] = rng.randint(0, 2, c)
    desc = rng.randint(0, 256, (nt, 32)).astype(np.uint8)
    return kp, desc


def _flip_bits(rng, d, k):
    bits = np.unpackbits(d); bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def random_scene(kp_dt, nt, n, seed=SCENE_SEED, cam=pm.CAM, pose=0, pose_dx=0.002, crowd=0, with_uright=True, frame=None):
    """a key frame of nt features and a map side of n entries.  Entry i, i % 8 < 5: feature f's point at its depth (1 .. 4 m) back-projected
    under the true pose, its descriptor f's with 0 .. 60 bits flipped (so best_dist <= 50 for most), its level f's octave (i % 8 == 4: the
    descriptor of entry i - 1's feature copied bit for bit on a twin feature's point: ties).  i % 8 == 5: one of the gates 1 .. 6 in turn.
    i % 8 == 6: a random point in view with a random descriptor.  i % 8 == 7: a point with f's descriptor 2 px off at octave + 1.
    The search runs under point_map_ref.estimated_pose(true pose, pose_dx).  frame = (kp_un, desc, uright or None, depth): an extracted
    frame instead of the random key frame (a feature without depth is planted at 2 m) -> (kf, mp)"""
    rng = np.random.RandomState(seed + 1)
    Ttrue = pm.scene_pose(pose); Test = pm.estimated_pose(Ttrue, pose_dx)
    T = np.asarray(Ttrue, np.float64).reshape(3, 4); R, t = T[:, :3], T[:, 3]
    _, _, Ow = pm.pose_parts(Test)
    if frame is None:
        kp, desc = random_keyframe(kp_dt, nt, seed, crowd)
        if nt >= 4:                                                 # twins: feature 6 k + 1 repeats 6 k's descriptor a pixel away at the same octave
            for k in range(0, nt - 1, 6):
                desc[k + 1] = desc[k]; kp["x"][k + 1] = F32(kp["x"][k] + 0.75); kp["y"][k + 1] = F32(kp["y"][k] - 0.5); kp["octave"][k + 1] = kp["octave"][k]
        depth = rng.uniform(1.0, 4.0, max(nt, 1))
        ur = (kp["x"] - F32(cam[4]) / depth[:nt].astype(F32)).astype(F32)
        ur[rng.rand(nt) < 0.33] = -1.0
    else:
        kp, desc, ur, depth = frame; nt = len(kp); with_uright = ur is not None
        depth = np.where(np.asarray(depth) > 0, depth, 2.0).astype(np.float64)
        if nt == 0: depth = np.ones(1)
    pos = np.zeros((n, 3), np.float32); nrm = np.zeros((n, 3), np.float32); mx = np.ones(n, np.float32); mn = np.zeros(n, np.float32)
    qd = rng.randint(0, 256, (n, 32)).astype(np.uint8); skip = np.zeros(n, np.uint8)

    def back(u, v, z):
        Xc = np.array([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z])
        return (R.T @ (Xc - t)).astype(np.float32)

    def plant(i, u, v, z, octave):
        while True:
            X = back(u, v, z)
            d = pm._dist(X, Ow)
            m = max_dist_for_level(d, octave)
            if not pm.level_guard(m, d): break
            z = z * 1.01
        pos[i] = X; mx[i] = m; mn[i] = F32(m / pm.SF[7])
        dd = X.astype(np.float64) - Ow.astype(np.float64); nrm[i] = (dd / np.linalg.norm(dd)).astype(np.float32)

    for i in range(n):
        k = i % 8
        f = int(rng.randint(0, nt)) if nt else -1
        if nt == 0 or k == 6:
            plant(i, rng.uniform(20, 620), rng.uniform(20, 460), rng.uniform(1.0, 4.0), int(rng.randint(0, 8)))
        elif k < 4:
            if k == 3 and nt >= 4: f = 6 * int(rng.randint(0, (nt + 4) // 6))
            f = min(f, nt - 1)
            plant(i, float(kp["x"][f]), float(kp["y"][f]), float(depth[f]), int(kp["octave"][f])); qd[i] = _flip_bits(rng, desc[f], int(rng.randint(0, 61)))
            if k == 3: qd[i] = desc[f]
        elif k == 4:
            plant(i, float(kp["x"][f]) + 0.5, float(kp["y"][f]), float(depth[f]), int(kp["octave"][f])); qd[i] = _flip_bits(rng, desc[f], 40)
        elif k == 5:
            g = 1 + (i // 8) % 6
            plant(i, float(kp["x"][f]), float(kp["y"][f]), 2.0, int(kp["octave"][f])); qd[i] = desc[f]
            if g == SKIP: skip[i] = 1
            elif g == BEHIND: pos[i] = back(float(kp["x"][f]), float(kp["y"][f]), -2.0)
            elif g == OUT_OF_IMAGE: pos[i] = back(-40.0 if i % 16 < 8 else 300.0, 200.0 if i % 16 < 8 else 520.0, 2.0)
            elif g == DIST_MIN: mn[i] = F32(mx[i] * 4.0)
            elif g == DIST_MAX: mx[i] = F32(mx[i] * 0.1); mn[i] = F32(mx[i] * 0.1)
            else: nrm[i] = -nrm[i]
        else:
            plant(i, float(kp["x"][f]) + 2.0, float(kp["y"][f]) - 2.0, float(depth[f]), min(7, int(kp["octave"][f]) + 1)); qd[i] = desc[f]
    kf = dict(kp_un=kp, uright=ur if with_uright else None, desc=desc, Tcw=Test, skip=skip)
    mp = dict(pos=pos, normal=nrm, max_dist=mx, min_dist=mn, desc=qd)
    return kf, mp


def vacuity(w, n):
    """the caps the random scenes must meet on the restatement's own output"""
    assert w["n_fused"] * 4 >= n, ("fused", w["n_fused"], n)
    assert set(np.unique(w["gate"]).tolist()) == set(range(7)), np.unique(w["gate"])
    assert (w["n_ties"] > 1).any(), "no entry with more than one candidate at the best distance"


RAGGED = ((65, 257), (0, 40), (300, 0), (64, 17))     # (features, map entries) of the four key frames of one call


def ragged_keyframes(kp_dt):
    """four key frames for ONE call with a map side each: an empty key frame and an empty map side inside the list, uright = None on key frame
    2, skip = None on key frame 1; then the same key frames against one shared map side made from key frame 2's own features (skip bytes
    of the shared length) -> (kfs, maps, shared_kfs, shared_map)"""
    sc = [random_scene(kp_dt, nt, n, seed=400 + j, pose=j, pose_dx=0.001 * (j + 1)) for j, (nt, n) in enumerate(RAGGED)]
    kfs = [s[0] for s in sc]; maps = [s[1] for s in sc]
    kfs[2] = dict(kfs[2], uright=None); kfs[1] = dict(kfs[1], skip=None)
    _, shared = random_scene(kp_dt, 300, 257, seed=402, pose=2, pose_dx=0.003)
    shared_kfs = [dict(kf, skip=None if j == 1 else ((np.arange(257) + j) % 7 == 0).astype(np.uint8)) for j, kf in enumerate(kfs)]
    return kfs, maps, shared_kfs, shared
