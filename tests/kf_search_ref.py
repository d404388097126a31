"""CPU restatement of ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (reference src/ORBmatcher.cc:1499-1628),
the refinement Tracking::Relocalization runs between its pose optimisations (src/Tracking.cc:3871 and :3885).  Test infrastructure only:
numpy float32 / float64 chosen operation by operation, one step per step of the reference, the loop sequential.  Built from point_map_ref
(pose_parts, transform, predict_scale, build_grid, features_in_area, level_guard); ComputeThreeMaxima as guided_cases.rotation states it by
hand (strict > keeps the first of equal bins ahead; a bin survives when its count is >= 0.1f * the best).

Readings (OpenCV is not in the reference tree; csrc/kf_search.hip and DESIGN.md section 7 state the same ones):
  Rcw * x3Dw + tcw       point_map_ref.transform
  invzc = 1.0 / z        the text divides the double 1.0: double quotient, rounded to float.  NO sign test follows
  u, v                   fx * xc * invzc + cx in float, left to right
  Ow, x3Dw - Ow, norm    point_map_ref.pose_parts; float difference; sqrt of the double sum of squares, stored to float
  distance range         dist3D < 0.8f * mfMinDistance, dist3D > 1.2f * mfMaxDistance (float products)
  PredictScale           point_map_ref.predict_scale on the RAW mfMaxDistance
  window                 radius = th * mvScaleFactors[level] (float), GetFeaturesInArea(u, v, radius, level - 1, level + 1)
  the loop               every non-NULL feature is skipped; bestDist starts at 256, strictly smaller distances enter; bestDist <= ORBdist accepts
  rotation               rot = kf angle - frame angle (+ 360 when negative), bin = round(rot * (1.0f / 30)), 30 -> 0; three maxima; the rest is culled"""
import math

import numpy as np

import guided_cases as gc
import point_map_ref as pm

F32 = np.float32
MAX_ENTRIES, MAX_FEATURES = 16384, 65535
GATES = ("searched", "skip", "u < minX", "u > maxX", "v < minY", "v > maxY", "dist < 0.8 min", "dist > 1.2 max")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1630-1673) over the bins' counts -> (ind1, ind2, ind3)"""
    max1 = max2 = max3 = 0; ind1 = ind2 = ind3 = -1
    for b, s in enumerate(hist):
        if s > max1: max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, b
        elif s > max2: max3, max2, ind3, ind2 = max2, s, ind2, b
        elif s > max3: max3, ind3 = s, b
    if F32(max2) < F32(F32(0.1) * F32(max1)): ind2 = ind3 = -1
    elif F32(max3) < F32(F32(0.1) * F32(max1)): ind3 = -1
    return ind1, ind2, ind3


def rot_bin(angle_kf, angle_frame):
    rot = F32(F32(angle_kf) - F32(angle_frame))
    if rot < 0.0: rot = F32(rot + F32(360.0))
    b = pm._round_away(F32(rot * F32(F32(1.0) / F32(30))))
    return 0 if b == 30 else b


def project(pos, skip, max_dist, min_dist, Tcw, cam, bounds4, log_scale_factor, n_levels):
    """lines 1517-1550 per entry -> (gate (n) int8, proj (n, 2) float32, level (n) int32).  proj is (0, 0) for a skipped entry and the
    projection for every other one; level is -1 for every entry that is not searched"""
    n = len(skip)
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    R, t, Ow = pm.pose_parts(Tcw)
    gate = np.ones(n, np.int8); proj = np.zeros((n, 2), np.float32); level = np.full(n, -1, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            if skip[i]: continue
            P = np.asarray(pos[i], np.float32)
            Pc = pm.transform(R, t, P)
            invz = F32(np.float64(1.0) / np.float64(Pc[2]))
            u = F32(F32(F32(fx * Pc[0]) * invz) + cx); v = F32(F32(F32(fy * Pc[1]) * invz) + cy)
            proj[i] = (u, v)
            if u < minX: gate[i] = 2; continue
            if u > maxX: gate[i] = 3; continue
            if v < minY: gate[i] = 4; continue
            if v > maxY: gate[i] = 5; continue
            d = [float(F32(P[k] - Ow[k])) for k in range(3)]
            dist = F32(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
            if dist < F32(F32(0.8) * F32(min_dist[i])): gate[i] = 6; continue
            if dist > F32(F32(1.2) * F32(max_dist[i])): gate[i] = 7; continue
            gate[i] = 0; level[i] = pm.predict_scale(max_dist[i], dist, log_scale_factor, n_levels)
    return gate, proj, level


def entry_dist(pos, Tcw):
    """dist3D of one entry, as project() forms it"""
    _, _, Ow = pm.pose_parts(Tcw)
    return pm._dist(np.asarray(pos, np.float32), Ow)


def search(cand, cam, t_kp, t_desc, bounds4, th, orb_dist, check_orientation=True, log_scale_factor=pm.LOG_SF, n_levels=pm.N_LEVELS, scale_factors=pm.SF,
           sequential=True):
    """the whole call for one candidate: cand = dict(pos, skip, max_dist, min_dist, desc, angle, Tcw, occupied (or None)) -> dict as the
    library's result.  sequential=False: no entry's match blocks another (every entry's independent best under the occupancy at entry),
    without the rotation cull"""
    n, nt = len(cand["skip"]), len(t_kp)
    gate, proj, level = project(cand["pos"], cand["skip"], cand["max_dist"], cand["min_dist"], cand["Tcw"], cam, bounds4, log_scale_factor, n_levels)
    mi = np.full(n, -1, np.int32); md = np.full(n, 256, np.int32); fk = np.full(nt, -1, np.int32)
    out = dict(gate=gate, proj=proj, level=level, match_idx=mi, match_dist=md, feature_kf=fk, n_matches=0, n_searched=int((gate == 0).sum()), status=0)
    if n == 0 or nt == 0: return out
    grid, invW, invH = pm.build_grid(t_kp, bounds4)
    occ = np.zeros(nt, bool) if cand.get("occupied") is None else np.asarray(cand["occupied"]).astype(bool).copy()
    t_desc = np.asarray(t_desc, np.uint8).reshape(-1, 32); q_desc = np.asarray(cand["desc"], np.uint8).reshape(-1, 32)
    bins = np.full(n, -1, np.int32); nm = 0
    for i in range(n):
        if gate[i] != 0: continue
        l = int(level[i])
        radius = F32(F32(th) * F32(scale_factors[l]))
        idxs = pm.features_in_area(t_kp, grid, invW, invH, bounds4, proj[i, 0], proj[i, 1], radius, l - 1, l + 1)
        best, bidx = 256, -1
        for j in idxs:
            if occ[j]: continue
            d = int(_POP[q_desc[i] ^ t_desc[j]].sum())
            if d < best: best, bidx = d, j
        if best <= orb_dist:
            mi[i] = bidx; md[i] = best; nm += 1
            if sequential: occ[bidx] = True
            if check_orientation and sequential: bins[i] = rot_bin(cand["angle"][i], t_kp["angle"][bidx])
    if check_orientation and sequential:
        hist = [int((bins == b).sum()) for b in range(30)]
        keep = three_maxima(hist)
        for i in range(n):
            if bins[i] >= 0 and bins[i] not in keep:
                mi[i] = -1; md[i] = 256; nm -= 1
        out["hist"] = hist; out["keep"] = keep
    if sequential:
        for i in range(n):
            if mi[i] >= 0: fk[mi[i]] = i
    out["n_matches"] = nm
    return out


def after(cand, r):
    """the candidate for the next search of Relocalization: what was found joins sAlreadyFound, the frame holds the matches"""
    c = dict(cand)
    c["skip"] = (np.asarray(cand["skip"]).astype(bool) | (r["match_idx"] >= 0)).astype(np.uint8)
    occ = np.zeros(len(r["feature_kf"]), bool) if cand.get("occupied") is None else np.asarray(cand["occupied"]).astype(bool)
    c["occupied"] = (occ | (r["feature_kf"] >= 0)).astype(np.uint8)
    return c


# ---- crafted entries: every gate alone, under point_map_ref.crafted_pose() with CAM2, where the arithmetic is exact ----
CAM2 = pm.CAM2                                    # (512, 512, 320, 240, 64): with z = 2, u = 256 x + 320, v = 256 y + 240
T_CRAFTED = pm.crafted_pose()                     # Xc = (Yw + 0.5, Zw - 0.25, Xw + 2); Ow = (-2, -0.5, 0.25)
world = pm.crafted_world


def crafted_entries():
    """-> rows of (name, pos, mfMaxDistance, mfMinDistance, skip, expected gate, expected (u, v) or None, expected level or None).
    Bounds rows: z = 2 (2^-20 in x moves u by 2^-12, which a float near 640 holds).  Distance rows: P on the optical axis, PO = (z, 0, 0),
    dist3D = z.  No row depends on the sign of z but through u and v: at z = -2 the image point is mirrored through the principal point."""
    eps = 2.0 ** -20
    rows = []
    for name, x, y, g in (("u on max", 1.25, 0, 0), ("u beyond max", 1.25 + eps, 0, 3), ("u on min", -1.25, 0, 0), ("u beyond min", -1.25 - eps, 0, 2),
                          ("v on max", 0, 0.9375, 0), ("v beyond max", 0, 0.9375 + eps, 5), ("v on min", 0, -0.9375, 0), ("v beyond min", 0, -0.9375 - eps, 4)):
        rows.append((name, world(x, y, 2.0), 8.0, 0.5, 0, g, (F32(256 * x + 320), F32(256 * y + 240)), None))
    zmax = F32(F32(1.2) * F32(2.0)); zmin = F32(F32(0.8) * F32(2.0))
    rows += [("dist on max", world(0, 0, zmax), 2.0, 0.5, 0, 0, (320.0, 240.0), 0),
             ("dist beyond max", world(0, 0, zmax), np.nextafter(F32(2.0), F32(0)), 0.5, 0, 7, (320.0, 240.0), None),
             ("dist on min", world(0, 0, zmin), 8.0, 2.0, 0, 0, (320.0, 240.0), None),
             ("dist below min", world(0, 0, zmin), 8.0, np.nextafter(F32(2.0), F32(3)), 0, 6, (320.0, 240.0), None),
             # the depth sign is not tested: both are searched, at mirrored image points.  dist3D = sqrt(4 + 0.25 + 0.0625) = 2.077 for both,
             # ratio 4 / 2.077 = 1.926, log / log(1.2) = 3.59: level 4 (as test_point_map.py's first known answer)
             ("z = +2", world(0.5, 0.25, 2.0), 4.0, 1.0, 0, 0, (448.0, 304.0), 4),
             ("z = -2, in bounds, in range", world(0.5, 0.25, -2.0), 4.0, 1.0, 0, 0, (192.0, 176.0), 4),
             ("z = -2, beyond max u", world(-1.25 - eps, 0, -2.0), 8.0, 0.5, 0, 3, None, None),      # mirrored: x < 0 lands right of the image
             # z == 0: X = Y = 0 gives NaN projections, which pass the four bounds tests and find nothing; X != 0 gives an infinite u.
             # dist3D = 0 for the first: max / 0 = inf, its log and ceil are inf, the conversion saturates, the clamp gives the top level
             ("z = 0, NaN", world(0, 0, 0.0), 1e9, 0.0, 0, 0, None, 7),
             ("z = 0, u = +inf", world(1.0, 0, 0.0), 1e9, 0.0, 0, 3, (np.inf, None), None),
             ("z = 0, u = -inf", world(-1.0, 0, 0.0), 1e9, 0.0, 0, 2, (-np.inf, None), None),
             ("z = 0, v = +inf", world(0, 1.0, 0.0), 1e9, 0.0, 0, 5, None, None),
             ("z = 0, v = -inf", world(0, -1.0, 0.0), 1e9, 0.0, 0, 4, None, None),
             ("NaN position", np.array([np.nan, 0, 0], np.float32), 4.0, 1.0, 0, 0, None, 0),       # every comparison is false; PredictScale's NaN -> 0
             ("skipped", world(0, 0, 2.0), 4.0, 1.0, 1, 1, (0.0, 0.0), None),
             ("skipped, NaN position", np.array([np.nan] * 3, np.float32), np.nan, np.nan, 1, 1, (0.0, 0.0), None),
             ("level clamped high", world(0, 0, 2.0), 2.0 * 1.2 ** 30, 0.1, 0, 0, (320.0, 240.0), 7),
             ("level clamped low", world(0, 0, zmax), 2.0, 0.1, 0, 0, (320.0, 240.0), 0)]
    return rows


def max_dist_for_level(dist, l):
    """mfMaxDistance for which log(ratio) / logScaleFactor = l - 0.5: half a level from the integers, the predicted level is l"""
    return F32(float(dist) * float(pm.SF[l]) / math.sqrt(1.2))


def crafted_candidate(kp_dt, seed=3):
    """the crafted rows as one candidate (about 40 entries: each row, then ordinary entries on a lattice) against an 80-feature frame: a
    feature of octave 1 on every lattice entry's image point and on some rows', the rest scattered -> (cand, t_kp, t_desc, rows)"""
    rng = np.random.RandomState(seed)
    rows = crafted_entries()
    lat = [(64.0 + 96.0 * (k % 6), 80.0 + 160.0 * (k // 6)) for k in range(14)]           # image points of ordinary entries at z = 2
    n = len(rows) + len(lat)
    pos = np.zeros((n, 3), np.float32); mx = np.zeros(n, np.float32); mn = np.zeros(n, np.float32); skip = np.zeros(n, np.uint8)
    for i, r in enumerate(rows):
        pos[i] = r[1]; mx[i] = F32(r[2]); mn[i] = F32(r[3]); skip[i] = r[4]
    for k, (u, v) in enumerate(lat):
        i = len(rows) + k
        pos[i] = world((u - 320.0) / 256.0, (v - 240.0) / 256.0, 2.0)
        mx[i] = max_dist_for_level(entry_dist(pos[i], T_CRAFTED), 1); mn[i] = F32(mx[i] / pm.SF[7])
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    nt = 80
    kp = np.zeros(nt, kp_dt); kp["size"] = 31; kp["class_id"] = -1
    kp["x"] = rng.uniform(20, 620, nt).astype(F32); kp["y"] = rng.uniform(20, 460, nt).astype(F32); kp["octave"] = rng.randint(0, 8, nt)
    kp["angle"] = rng.uniform(0, 360, nt).astype(F32)
    t_desc = rng.randint(0, 256, (nt, 32)).astype(np.uint8)
    angle = rng.uniform(0, 360, n).astype(F32)
    for k, (u, v) in enumerate(lat):                                                         # feature k sits a pixel off lattice entry k's image point
        i = len(rows) + k
        kp["x"][k] = F32(u + 1.0); kp["y"][k] = F32(v - 1.0); kp["octave"][k] = 1 + (k % 2); t_desc[k] = gc.flip(3 + k, k, desc[i]); angle[i] = F32(kp["angle"][k] + 33.0) % F32(360)
    for k, name in enumerate(("z = +2", "z = -2, in bounds, in range", "dist on max", "level clamped high")):     # and on four rows' image points
        i = [r[0] for r in rows].index(name); j = len(lat) + k
        kp["x"][j], kp["y"][j] = rows[i][6]; kp["octave"][j] = rows[i][7]; t_desc[j] = gc.flip(5, j, desc[i]); angle[i] = F32(kp["angle"][j] + 33.0) % F32(360)
    cand = dict(pos=pos, skip=skip, max_dist=mx, min_dist=mn, desc=desc, angle=angle, Tcw=T_CRAFTED, occupied=np.zeros(nt, np.uint8))
    return cand, kp, t_desc, rows


# ---- small hand-stated searches (entries at z = 2 under the crafted pose, level 1: radius = 1.2 th, band [0, 2]) ----
def hand_scene(kp_dt, entries, feats, occupied=()):
    """entries: (u, v, descriptor, angle); feats: (x, y, octave, descriptor, angle) -> (cand, t_kp, t_desc)"""
    n, nt = len(entries), len(feats)
    pos = np.zeros((n, 3), np.float32); mx = np.zeros(n, np.float32)
    for i, e in enumerate(entries):
        pos[i] = world((e[0] - 320.0) / 256.0, (e[1] - 240.0) / 256.0, 2.0); mx[i] = max_dist_for_level(entry_dist(pos[i], T_CRAFTED), 1)
    kp = np.zeros(nt, kp_dt); kp["size"] = 31; kp["class_id"] = -1
    for j, f in enumerate(feats):
        kp["x"][j], kp["y"][j], kp["octave"][j], kp["angle"][j] = f[0], f[1], f[2], f[4]
    occ = np.zeros(nt, np.uint8); occ[list(occupied)] = 1
    cand = dict(pos=pos, skip=np.zeros(n, np.uint8), max_dist=mx, min_dist=(mx / pm.SF[7]).astype(F32), desc=np.stack([e[2] for e in entries]),
                angle=np.array([e[3] for e in entries], F32), Tcw=T_CRAFTED, occupied=occ)
    return cand, kp, np.stack([f[3] for f in feats])


def rotation_scene(kp_dt, counts):
    """isolated one-to-one pairs as guided_cases.rotation lays them out: counts = [(bin, n), ...]; pair k of a bin has
    kf angle - frame angle = 30 bin - 7 + k % 15 degrees -> (cand, t_kp, t_desc, bins)"""
    _, q, t, r = gc.rotation(kp_dt, "rot", counts, tail=False)
    entries = [(float(q.u[i]), float(q.v[i]), q.desc[i], float(q.angle[i])) for i in range(len(q.u))]
    feats = [(float(t.kp["x"][j]), float(t.kp["y"][j]), 1, t.desc[j], float(t.kp["angle"][j])) for j in range(len(t.kp))]
    cand, kp, t_desc = hand_scene(kp_dt, entries, feats)
    return cand, kp, t_desc, r.bins


def chain_scene(kp_dt, nt=100, Q=40):
    """guided_cases.chain at nt features: Q identical entries over one window that holds all nt features, every one a candidate of every
    entry, so entry i takes the i-th feature in (distance, cellX, cellY, index) order and from entry 16 on every ranked key is claimed: the
    rescan path.  The window is th = 400 / 1.2 at level 1 (radius 400), centred on (320, 240); the features' octaves are 0 .. 2, inside the
    band [0, 2] -> (cand, t_kp, t_desc, th, expected match_idx, expected match_dist)"""
    c = gc.chain(kp_dt, "chain%d" % nt, nt, Q=Q)
    assert set(np.unique(c.t.kp["octave"]).tolist()) <= {0, 1, 2}
    entries = [(320.0, 240.0, c.q.desc[i], 0.0) for i in range(Q)]
    feats = [(float(c.t.kp["x"][j]), float(c.t.kp["y"][j]), int(c.t.kp["octave"][j]), c.t.desc[j], 0.0) for j in range(nt)]
    cand, kp, t_desc = hand_scene(kp_dt, entries, feats)
    th = F32(F32(400.0) / F32(1.2))
    assert F32(th * pm.SF[1]) >= F32(399.9)
    n, idx, dist = c.expect["last"]
    return cand, kp, t_desc, float(th), idx, dist


# ---- the planted scene of the GPU tests (and of the CPU checks of the generator itself) ----
N_FEATURES, N_ENTRIES, SCENE_SEED = 1004, 1000, 20


def planted_frame(kp_dt, seed=SCENE_SEED, nt=N_FEATURES):
    """a synthetic 640 x 480 frame: nt key points with octaves, angles and random descriptors"""
    rng = np.random.RandomState(seed)
    kp = np.zeros(nt, kp_dt); kp["size"] = 31; kp["class_id"] = -1
    kp["x"] = rng.uniform(16, 624, nt).astype(F32); kp["y"] = rng.uniform(16, 464, nt).astype(F32)
    kp["octave"] = rng.choice(8, nt, p=[0.26, 0.2, 0.16, 0.12, 0.1, 0.07, 0.05, 0.04]); kp["angle"] = rng.uniform(0, 360, nt).astype(F32)
    return kp, rng.randint(0, 256, (nt, 32)).astype(np.uint8)


def _flip_bits(rng, d, k):
    bits = np.unpackbits(d); bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def planted_candidate(kp, desc, Tcw_true, seed=SCENE_SEED, n=N_ENTRIES, cam=pm.CAM, bounds4=pm.BOUNDS, feats=None, pose_dx=0.01):
    """a key frame whose map points are the frame's key points back-projected under the true pose; the search runs under
    point_map_ref.estimated_pose(Tcw_true).  Entry i (i % 10 < 7) is feature feats[i] at a depth of 1 .. 4 m, its level the feature's octave,
    its descriptor the feature's with 0 .. 70 bits flipped, its angle the feature's + 40 degrees (every 23rd: anything).  i % 10 == 7: a
    second, worse copy of an earlier entry (the same feature is its independent best: sequential claims matter).  i % 10 == 8: one of the
    seven gates in turn.  i % 10 == 9: a point behind the camera whose projection is a feature's.  Every 17th feature is occupied at entry.
    An entry in view whose log(ratio) / logScaleFactor lies within 1e-4 of an integer under the search pose is drawn again -> cand"""
    rng = np.random.RandomState(seed + 1)
    nt = len(kp)
    T = np.asarray(Tcw_true, np.float64).reshape(3, 4); R, t = T[:, :3], T[:, 3]
    Test = pm.estimated_pose(Tcw_true, pose_dx)
    feats = rng.permutation(nt) if feats is None else np.asarray(feats)
    pos = np.zeros((n, 3), np.float32); mx = np.zeros(n, np.float32); mn = np.zeros(n, np.float32); skip = np.zeros(n, np.uint8)
    qd = rng.randint(0, 256, (n, 32)).astype(np.uint8); ang = rng.uniform(0, 360, n).astype(F32)

    def back(u, v, z):
        Xc = np.array([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z])
        return (R.T @ (Xc - t)).astype(np.float32)

    def plant(i, f, z, flips):
        while True:
            X = back(float(kp["x"][f]), float(kp["y"][f]), z)
            d = entry_dist(X, Test)
            m = max_dist_for_level(d, int(kp["octave"][f]))
            if not pm.level_guard(m, d): break
            z = z * 1.01
        pos[i] = X; mx[i] = m; mn[i] = F32(m / pm.SF[7])
        qd[i] = _flip_bits(rng, desc[f], flips); ang[i] = F32((float(kp["angle"][f]) + 40.0) % 360.0)

    planted = []
    for i in range(n):
        k = i % 10
        f = int(feats[i % len(feats)])
        if k < 7:
            plant(i, f, rng.uniform(1.0, 4.0), int(rng.randint(0, 71))); planted.append(i)
            if i % 23 == 0: ang[i] = F32(rng.uniform(0, 360))
        elif k == 7:
            src = planted[int(rng.randint(0, len(planted)))]
            pos[i] = pos[src]; mx[i] = mx[src]; mn[i] = mn[src]; ang[i] = ang[src]; qd[i] = _flip_bits(rng, qd[src], 6)
        elif k == 8:
            g = 1 + (i // 10) % 7
            plant(i, f, 2.0, 10)
            if g == 1: skip[i] = 1
            elif g in (2, 3, 4, 5):
                u, v = {2: (-40.0, 200.0), 3: (700.0, 200.0), 4: (300.0, -30.0), 5: (300.0, 520.0)}[g]
                pos[i] = back(u, v, 2.0)
            elif g == 6: mn[i] = F32(mx[i] * 4.0)
            else: mx[i] = F32(mx[i] * 0.1); mn[i] = F32(mx[i] * 0.1)
        else:
            plant(i, f, 2.0, 10)
            X = back(float(kp["x"][f]), float(kp["y"][f]), -2.0)      # behind the camera, on the ray through f: it projects onto f
            d = entry_dist(X, Test); m = max_dist_for_level(d, int(kp["octave"][f]))
            if not pm.level_guard(m, d): pos[i] = X; mx[i] = m; mn[i] = F32(m / pm.SF[7])
    occ = np.zeros(nt, np.uint8); occ[::17] = 1
    return dict(pos=pos, skip=skip, max_dist=mx, min_dist=mn, desc=qd, angle=ang, Tcw=Test, occupied=occ)


def planted_scene(kp_dt, seed=SCENE_SEED):
    kp, desc = planted_frame(kp_dt, seed)
    return planted_candidate(kp, desc, pm.scene_pose(0), seed), kp, desc
