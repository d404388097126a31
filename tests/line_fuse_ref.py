"""CPU restatement of LSDmatcher::Fuse(KeyFrame *, const vector<MapLine *> &, float th) (reference src/LSDmatcher.cpp:1297-1434) with
KeyFrame::GetLinesInArea (src/KeyFrame.cc:668-702), KeyFrame::IsInImage and MapLine::PredictScale (src/MapLine.cpp:549-558).  Test
infrastructure only, and the DEFINITION the device is compared with: numpy float32 / float64 chosen operation by operation, one step per step
of the reference, the loops sequential: per entry, per key line, with a real vIndices list from a real GetLinesInArea (it normalises every key
line's direction again for every entry; the device forms it once per key frame).

The readings (csrc/line_fuse.hip, include/hvo.h and DESIGN.md section 7 state the same):
  1. Which descriptors.  The text compares the map line's LBD descriptor with pKF->mDescriptors.row(idx): ORB rows under a line index.  Here
     kf["desc_rows"] are "the rows the candidates are compared with": mLineDescriptors (intended) or mDescriptors (as written).  A candidate
     idx >= len(desc_rows) is not compared.  No flag.
  2. The predicted level.  MapLine::PredictScale is unclamped.  level_rule CLAMPED (default) clamps to [0, n_levels - 1] before the radius and
     the band; AS_WRITTEN keeps it, and an entry whose level is outside [0, n_levels) gets the gate LEVEL and is not searched.
     log_scale_factor is a parameter of its own; the table is sf[0] = 1, sf[l] = sf[l - 1] * scale_factor in float.
  3. `return false` on a negative depth: no stop is applied here.  Every entry is evaluated, such an entry has the gate BEHIND, and
     behind_entry lists them.  walk() below applies the stop (stop_on_behind, the default and as written) or continues.
Kept as written: the entry order (skip, then both depths); IsInImage(u1, v1) before u2, v2 are computed (a NaN fails); the two distance gates;
the double 0.5 * dist of the angle gate; the band [level - 1, level] on kl.octave; an empty vIndices gives no match; strict `dist < bestDist`
in ascending line index; acceptance at bestDist <= th_low.
Arithmetic taken from the sibling restatements:
  Rcw * SP + tcw        tests/fuse_ref.py (point_map_ref.transform); Ow from point_map_ref.pose_parts
  invz, u               the text has 1.0f / z and fx * X * invz + cx: one float division, the products left to right (not fuse_ref's grouping)
  0.5 * (SP + EP)       tests/map_refresh_ref.py: f32(SP * 0.5 + EP * 0.5), products and sum in double, ONE rounding; minus Ow in float
  cv::norm              tests/fuse_ref.py: the square root of the double sum of squares left to right, stored to float
  Mat::dot              tests/fuse_ref.py: double accumulation in order, compared with the double 0.5 * dist
  PredictScale          point_map_ref.predict_level_exact (float ratio, float log, float division), ceil, saturating conversion
Inside GetLinesInArea: x1 + x2 is a float sum, 0.5 * it and the differences and squares are double, the sum is rounded to the float
`distance` and compared with the float r * r by `>`; both directions are normalised in float with the float sqrt; CosSita is the float abs of
the float sum of two float products; `CosSita < 0.998f` continues, so a NaN passes."""
import math

import numpy as np

import point_map_ref as pm

F32 = np.float32
MAX_LINES, MAX_ENTRIES = 2048, 65536
GATES = ("searched", "skip", "behind", "out of image", "dist < 0.8 min", "dist > 1.2 max", "view angle", "level")
SEARCHED, SKIP, BEHIND, OUT_OF_IMAGE, DIST_MIN, DIST_MAX, VIEW_ANGLE, LEVEL = range(8)
CLAMPED, AS_WRITTEN = "clamped", "as written"
TH, TH_LOW, COS_TH = 3.0, 50, F32(0.998)
LOG_SF = pm.LOG_SF
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def scale_table(n_levels, scale_factor):
    sf = [F32(1.0)]
    for _ in range(1, n_levels): sf.append(F32(sf[-1] * F32(scale_factor)))
    return np.array(sf, np.float32)


def lines_in_area(kl, x1, y1, x2, y2, r):
    """KeyFrame::GetLinesInArea -> vIndices"""
    x1, y1, x2, y2, r = F32(x1), F32(y1), F32(x2), F32(y2), F32(r)
    out = []
    with np.errstate(all="ignore"):
        d1x = F32(x1 - x2); d1y = F32(y1 - y2)
        n1 = F32(np.sqrt(F32(F32(d1x * d1x) + F32(d1y * d1y))))
        d1x = F32(d1x / n1); d1y = F32(d1y / n1)
        for i in range(len(kl)):
            ex = 0.5 * float(F32(x1 + x2)) - float(kl["pt_x"][i]); ey = 0.5 * float(F32(y1 + y2)) - float(kl["pt_y"][i])
            distance = F32(ex * ex + ey * ey)
            if distance > F32(r * r): continue
            d2x = F32(kl["sx"][i] - kl["ex"][i]); d2y = F32(kl["sy"][i] - kl["ey"][i])
            n2 = F32(np.sqrt(F32(F32(d2x * d2x) + F32(d2y * d2y))))
            d2x = F32(d2x / n2); d2y = F32(d2y / n2)
            cos = F32(abs(F32(F32(d1x * d2x) + F32(d1y * d2y))))
            if cos < COS_TH: continue
            out.append(i)
    return out


def project_entry(P6, normal, max_distance, min_distance, R, t, Ow, cam, bounds4, log_scale_factor, n_levels, level_rule):
    """lines 1325-1374 for one entry -> (gate, (u1, v1, u2, v2) as far as computed, level or -1, log(ratio) / logScaleFactor or None)"""
    fx, fy, cx, cy = (F32(v) for v in cam[:4])
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    Z = F32(0)
    inside = lambda u, v: bool(u >= minX and u < maxX and v >= minY and v < maxY)
    with np.errstate(all="ignore"):
        SP = np.array([F32(P6[0]), F32(P6[1]), F32(P6[2])], np.float32); EP = np.array([F32(P6[3]), F32(P6[4]), F32(P6[5])], np.float32)
        SPc = pm.transform(R, t, SP); EPc = pm.transform(R, t, EP)
        if SPc[2] < F32(0.0) or EPc[2] < F32(0.0): return BEHIND, (Z, Z, Z, Z), -1, None
        invz1 = F32(F32(1.0) / SPc[2])
        u1 = F32(F32(F32(fx * SPc[0]) * invz1) + cx); v1 = F32(F32(F32(fy * SPc[1]) * invz1) + cy)
        if not inside(u1, v1): return OUT_OF_IMAGE, (u1, v1, Z, Z), -1, None
        invz2 = F32(F32(1.0) / EPc[2])
        u2 = F32(F32(F32(fx * EPc[0]) * invz2) + cx); v2 = F32(F32(F32(fy * EPc[1]) * invz2) + cy)
        uv = (u1, v1, u2, v2)
        if not inside(u2, v2): return OUT_OF_IMAGE, uv, -1, None
        maxD = F32(F32(1.2) * F32(max_distance)); minD = F32(F32(0.8) * F32(min_distance))
        d = [float(F32(F32(float(SP[k]) * 0.5 + float(EP[k]) * 0.5) - Ow[k])) for k in range(3)]
        dist = F32(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        if dist < minD: return DIST_MIN, uv, -1, None
        if dist > maxD: return DIST_MAX, uv, -1, None
        pn = [float(F32(normal[k])) for k in range(3)]
        dot = (d[0] * pn[0] + d[1] * pn[1]) + d[2] * pn[2]
        if dot < 0.5 * float(dist): return VIEW_ANGLE, uv, -1, None
        exact = pm.predict_level_exact(max_distance, dist, log_scale_factor)
        lvl = pm.to_int(np.ceil(exact))
        if level_rule == AS_WRITTEN:
            if lvl < 0 or lvl >= n_levels: return LEVEL, uv, lvl, exact
        else:
            lvl = 0 if lvl < 0 else (n_levels - 1 if lvl >= n_levels else lvl)
        return SEARCHED, uv, lvl, exact


def fuse(kf, mp, th=TH, th_low=TH_LOW, log_scale_factor=LOG_SF, n_levels=3, scale_factor=1.2, level_rule=CLAMPED):
    """one Fuse call.  kf = dict(kl, desc_rows, Tcw, cam, bounds, skip (or None)); mp = dict(pos (n x 6), normal (n x 3), max_distance,
    min_distance, desc) -> dict as the library's result, plus n_cand (candidates that reached the descriptor), n_ties (candidates at the
    final best distance) and level_exact (log(ratio) / logScaleFactor where PredictScale ran, else NaN)"""
    kl = kf["kl"]; n = len(mp["pos"])
    rows = np.asarray(kf["desc_rows"], np.uint8).reshape(-1, 32); q_desc = np.asarray(mp["desc"], np.uint8).reshape(-1, 32)
    skip = np.zeros(n, bool) if kf.get("skip") is None else np.asarray(kf["skip"]).astype(bool)
    R, t, Ow = pm.pose_parts(kf["Tcw"])
    sf = scale_table(n_levels, scale_factor)
    bi = np.full(n, -1, np.int32); bd = np.full(n, 256, np.int32); gate = np.full(n, SKIP, np.int8); level = np.full(n, -1, np.int32)
    proj = np.zeros((n, 4), np.float32); n_cand = np.zeros(n, np.int32); n_ties = np.zeros(n, np.int32); level_exact = np.full(n, np.nan, np.float32)
    pos = np.asarray(mp["pos"], np.float64).reshape(-1, 6); nrm = np.asarray(mp["normal"], np.float64).reshape(-1, 3)
    for i in range(n):
        if skip[i]: continue
        g, uv, lvl, exact = project_entry(pos[i], nrm[i], mp["max_distance"][i], mp["min_distance"][i], R, t, Ow, kf["cam"], kf["bounds"], log_scale_factor, n_levels, level_rule)
        gate[i] = g; proj[i] = uv; level[i] = lvl
        if exact is not None: level_exact[i] = exact
        if g != SEARCHED: continue
        radius = F32(F32(th) * sf[lvl])
        best, bidx, dists = 256, -1, []
        for j in lines_in_area(kl, uv[0], uv[1], uv[2], uv[3], radius):
            o = int(kl["octave"][j])
            if o < lvl - 1 or o > lvl: continue
            if j >= len(rows): continue
            d = int(_POP[q_desc[i] ^ rows[j]].sum())
            dists.append(d)
            if d < best: best, bidx = d, j
        bi[i] = bidx; bd[i] = best; n_cand[i] = len(dists); n_ties[i] = sum(1 for d in dists if d == best and best < 256)
    fe = np.flatnonzero(bd <= th_low).astype(np.int32); be = np.flatnonzero(gate == BEHIND).astype(np.int32)
    return dict(best_idx=bi, best_dist=bd, gate=gate, level=level, proj=proj, fused_entry=fe, fused_idx=bi[fe], behind_entry=be, n_fused=len(fe),
                n_behind=len(be), n_searched=int((gate == SEARCHED).sum()), status=0, n_cand=n_cand, n_ties=n_ties, level_exact=level_exact)


RESULT_KEYS = ("best_idx", "best_dist", "gate", "level", "proj", "fused_entry", "fused_idx", "behind_entry", "n_fused", "n_behind", "n_searched", "status")


def walk(res, still_skipped, on_fused, stop_on_behind=True):
    """hvo::LSDmatcher::walkFused: the fused and the behind entries merged in entry order.  still_skipped(entry): the caller's
    `isBad() || IsInKeyFrame(pKF)` now; on_fused(entry, idx) -> True when it called Replace.  With stop_on_behind the walk of this key frame
    ends at the first behind entry that is still not skipped when the walk reaches it -> dict(n_fused, stopped_at (or -1), replaced)"""
    ev = sorted([(int(e), 1, int(i)) for e, i in zip(res["fused_entry"], res["fused_idx"])] + [(int(e), 0, -1) for e in res["behind_entry"]])
    out = dict(n_fused=0, stopped_at=-1, replaced=False)
    for e, fused, idx in ev:
        if still_skipped(e): continue
        if not fused:
            if stop_on_behind: out["stopped_at"] = e; break
            continue
        if on_fused(e, idx): out["replaced"] = True
        out["n_fused"] += 1
    return out


# ---- crafted entries under point_map_ref.crafted_pose() with CAM2, where the arithmetic is exact ----
CAM2 = pm.CAM2                                    # (512, 512, 320, 240, 64): with z = 2, u = 256 x + 320, v = 256 y + 240
T_CRAFTED = pm.crafted_pose()                     # Xc = (Yw + 0.5, Zw - 0.25, Xw + 2); Ow = (-2, -0.5, 0.25)
world = pm.crafted_world
N_TOWARDS = (1.0, 0.0, 0.0)                       # a normal along OM for a mid-point on the optical axis (OM = (z, 0, 0) in world axes)
BASE = np.arange(32, dtype=np.uint8) * 7 + 3


def flip(k, base=BASE):
    """base with its first k bits flipped: Hamming distance k"""
    bits = np.unpackbits(base); bits[:k] ^= 1
    return np.packbits(bits)


def step(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf))


def seg(xc1, yc1, z1, xc2, yc2, z2):
    """the 6 doubles of the world line whose ends have these camera coordinates under T_CRAFTED"""
    return np.concatenate([world(xc1, yc1, z1), world(xc2, yc2, z2)]).astype(np.float64)


def seg_px(u1, v1, u2, v2, z=2.0):
    """... whose ends project to these pixels at depth z (exact for the values used here: z = 2 or a power of two times it)"""
    s = z / 512.0
    return seg((u1 - 320.0) * s, (v1 - 240.0) * s, z, (u2 - 320.0) * s, (v2 - 240.0) * s, z)


def _ow():
    return pm.pose_parts(T_CRAFTED)[2]


def mid_dist(P6):
    S = np.asarray(P6[:3], np.float32); E = np.asarray(P6[3:], np.float32)
    mid = np.array([F32(float(S[k]) * 0.5 + float(E[k]) * 0.5) for k in range(3)], np.float32)
    return pm._dist(mid, _ow())


def normal_of(P6):
    """a unit normal along OM: OM.dot(pn) = dist, far from the gate"""
    S = np.asarray(P6[:3], np.float64); E = np.asarray(P6[3:], np.float64)
    d = 0.5 * (S + E) - _ow().astype(np.float64)
    return d / max(np.linalg.norm(d), 1e-30)


def max_for_level(dist, l, log_scale_factor=LOG_SF):
    """mfMaxDistance for which log(ratio) / logScaleFactor = l - 0.5: half a level from the integers, the predicted level is l"""
    return F32(float(dist) * math.exp((l - 0.5) * float(log_scale_factor)))


def keylines(kl_dt, rows):
    """rows of (sx, sy, ex, ey, octave): pt = the float mid-point"""
    kl = np.zeros(len(rows), kl_dt); kl["class_id"] = np.arange(len(rows))
    for i, (sx, sy, ex, ey, o) in enumerate(rows):
        kl["sx"][i], kl["sy"][i], kl["ex"][i], kl["ey"][i], kl["octave"][i] = sx, sy, ex, ey, o
        kl["pt_x"][i] = F32(F32(F32(sx) + F32(ex)) * F32(0.5)); kl["pt_y"][i] = F32(F32(F32(sy) + F32(ey)) * F32(0.5))
    kl["sox"], kl["soy"], kl["eox"], kl["eoy"] = kl["sx"], kl["sy"], kl["ex"], kl["ey"]
    kl["length"] = np.hypot(kl["sx"] - kl["ex"], kl["sy"] - kl["ey"]); kl["num_pixels"] = kl["length"].astype(np.int32) + 1
    return kl


def make_kf(kl, desc_rows, Tcw=T_CRAFTED, cam=CAM2, bounds=pm.BOUNDS, skip=None):
    return dict(kl=kl, desc_rows=np.asarray(desc_rows, np.uint8).reshape(-1, 32), Tcw=np.asarray(Tcw, np.float32), cam=tuple(cam[:4]), bounds=tuple(bounds), skip=skip)


def make_map(rows, seed=5):
    """rows of (pos6, normal3, mfMaxDistance, mfMinDistance[, desc])"""
    rng = np.random.RandomState(seed)
    n = len(rows)
    return dict(pos=np.array([r[0] for r in rows], np.float64).reshape(n, 6), normal=np.array([r[1] for r in rows], np.float64).reshape(n, 3),
                max_distance=np.array([r[2] for r in rows], np.float32), min_distance=np.array([r[3] for r in rows], np.float32),
                desc=np.stack([np.asarray(r[4], np.uint8) if len(r) > 4 else rng.randint(0, 256, 32).astype(np.uint8) for r in rows]) if n else np.zeros((0, 32), np.uint8))


def crafted_gates(kl_dt):
    """one entry per gate code and per side of every comparison -> (kf, mp, expected gates, names).  The key frame holds one line nobody
    matches.  The mid-point of the distance and angle rows lies on the optical axis: OM = (z, 0, 0), dist = z."""
    zmax = F32(F32(1.2) * F32(2.0)); zmin = F32(F32(0.8) * F32(2.0))
    ax = lambda z, a=0.125: seg(-a, 0.0, z, a, 0.0, z)             # ends either side of the axis at depth z
    half = (0.5, math.sqrt(0.75), 0.0)                             # dot = 0.5 z exactly
    inn = seg_px(300.0, 200.0, 340.0, 220.0)
    rows, want, names, skip = [], [], [], []

    def add(name, P, nrm, mx, mn, g, sk=0):
        rows.append((P, nrm, mx, mn)); want.append(g); names.append(name); skip.append(sk)
    add("searched", inn, normal_of(inn), 8.0, 0.5, SEARCHED)
    add("skipped", inn, normal_of(inn), 8.0, 0.5, SKIP, 1)
    add("skipped, NaN position", np.full(6, np.nan), N_TOWARDS, np.nan, np.nan, SKIP, 1)
    add("start behind only", seg(0.0, 0.0, -2.0, 0.125, 0.0, 2.0), N_TOWARDS, 8.0, 0.5, BEHIND)
    add("end behind only", seg(0.0, 0.0, 2.0, 0.125, 0.0, -2.0), N_TOWARDS, 8.0, 0.5, BEHIND)
    add("both behind", seg(0.0, 0.0, -2.0, 0.125, 0.0, -2.0), N_TOWARDS, 8.0, 0.5, BEHIND)
    add("u1 on max, u2 in", seg_px(640.0, 200.0, 600.0, 200.0), N_TOWARDS, 8.0, 0.5, OUT_OF_IMAGE)
    add("u1 in, u2 on max", seg_px(600.0, 200.0, 640.0, 200.0), N_TOWARDS, 8.0, 0.5, OUT_OF_IMAGE)
    add("u1 just below max, u2 in", seg_px(float(step(640.0, False)), 200.0, 600.0, 200.0), normal_of(seg_px(620.0, 200.0, 600.0, 200.0)), 8.0, 0.5, SEARCHED)
    add("v1 below min", seg_px(300.0, -2.0 ** -10, 300.0, 40.0), N_TOWARDS, 8.0, 0.5, OUT_OF_IMAGE)
    add("v2 on min", seg_px(300.0, 40.0, 300.0, 0.0), normal_of(seg_px(300.0, 40.0, 300.0, 0.0)), 8.0, 0.5, SEARCHED)
    add("start at z = 0: NaN or inf fails IsInImage", seg(0.0, 0.0, 0.0, 0.125, 0.0, 2.0), N_TOWARDS, 1e9, 0.0, OUT_OF_IMAGE)
    add("dist on max", ax(zmax), N_TOWARDS, 2.0, 0.5, SEARCHED)
    add("dist a step inside max", ax(zmax), N_TOWARDS, float(step(2.0, True)), 0.5, SEARCHED)
    add("dist beyond max", ax(zmax), N_TOWARDS, float(step(2.0, False)), 0.5, DIST_MAX)
    add("dist on min", ax(zmin), N_TOWARDS, 8.0, 2.0, SEARCHED)
    add("dist a step inside min", ax(zmin), N_TOWARDS, 8.0, float(step(2.0, False)), SEARCHED)
    add("dist below min", ax(zmin), N_TOWARDS, 8.0, float(step(2.0, True)), DIST_MIN)
    add("view angle on the limit", ax(2.0), half, 4.0, 1.0, SEARCHED)
    add("view angle below the limit", ax(2.0), (float(step(0.5, False)), math.sqrt(0.75), 0.0), 4.0, 1.0, VIEW_ANGLE)
    kl = keylines(kl_dt, [(10.0, 470.0, 30.0, 470.0, 0)])
    mp = make_map(rows)
    return make_kf(kl, [flip(0)], skip=np.array(skip, np.uint8)), mp, want, names


LOG_11 = float(F32(np.log(F32(1.1))))


def crafted_levels(kl_dt, n_levels=3):
    """run with log_scale_factor = LOG_11: entries on the optical axis at dist 2 whose level is -1 (ratio 1 / 1.15: log / log 1.1 = -1.47; the
    distance gate dist > 1.2 max does not fire), 0, n_levels - 1, n_levels and far above -> (kf, mp, unclamped levels).  Under AS_WRITTEN the
    first and the last two get the gate LEVEL; CLAMPED searches them at 0 and n_levels - 1."""
    P = seg(-0.125, 0.0, 2.0, 0.125, 0.0, 2.0)
    lv = [-1, 0, n_levels - 1, n_levels, 40]
    rows = [(P, N_TOWARDS, F32(2.0 / 1.15) if l == -1 else max_for_level(2.0, l, LOG_11), 0.01, flip(l + 1)) for l in lv]
    kl = keylines(kl_dt, [(256.0, 240.0, 384.0, 240.0, 0), (256.0, 240.5, 384.0, 240.5, n_levels - 1)])
    return make_kf(kl, [flip(0), flip(0)]), make_map(rows), lv


def cos_pair(length=64.0):
    """two ADJACENT floats (dy_in, dy_out): a key line with start - end = (length, dy) has CosSita >= 0.998f against a horizontal
    projection with dy_in and < 0.998f with dy_out, in GetLinesInArea's own float arithmetic"""
    def cos(dy):
        dx = F32(length); dy = F32(dy)
        n = F32(np.sqrt(F32(F32(dx * dx) + F32(dy * dy))))
        return F32(abs(F32(F32(F32(-1.0) * F32(dx / n)) + F32(F32(0.0) * F32(dy / n)))))
    lo, hi = F32(3.5), F32(4.5)
    assert cos(lo) >= COS_TH > cos(hi)
    while step(lo, True) != hi:
        mid = F32((float(lo) + float(hi)) / 2)
        if mid == lo or mid == hi: mid = step(lo, True)
        if cos(mid) >= COS_TH: lo = mid
        else: hi = mid
    return lo, hi


def crafted_search(kl_dt, n_levels=3, chunk_tie=True):
    """entry k is the horizontal segment (u0 - 32, v0) .. (u0 + 32, v0) at z = 2 with u0 = 64 + 48 k (two rows: v0 = 100, 300): unit direction
    (-1, 0), mid-point (u0, v0), level `lvl`, radius 3 * 1.2^lvl.  Each has key lines of its own -> (kf, mp, expected best_idx, best_dist,
    names).  With chunk_tie the key frame has 300 lines and the tie of the last entry straddles the 256-record chunk boundary."""
    sf = scale_table(n_levels, 1.2)
    top = n_levels - 1
    lines, rows, ent, want, names = [], [], [], [], []

    def line(cx, cy, dx, dy, o, desc):
        """a key line with pt = (cx, cy) and start - end = (dx, dy), both exact"""
        lines.append((cx, cy, dx, dy, o)); rows.append(desc)
        return len(lines) - 1

    def entry(name, lvl, desc, zero=False):
        k = len(ent); u0 = 64.0 + 48.0 * (k % 12); v0 = 100.0 + 200.0 * (k // 12)
        P = seg_px(u0, v0, u0, v0) if zero else seg_px(u0 - 32.0, v0, u0 + 32.0, v0)
        ent.append((P, normal_of(P), max_for_level(mid_dist(P), lvl), 0.01, desc)); names.append(name)
        return u0, v0, float(F32(F32(3.0) * sf[lvl]))

    far = lambda: line(600.0, 450.0, 20.0, 0.0, 0, flip(200))
    # the mid-point gate: distance == r * r is inside (`>`), one float step further is outside
    u, v, r = entry("mid-point on r", 0, flip(0)); a = line(u + r, v, 64.0, 0.0, 0, flip(3)); want.append((a, 3))
    u, v, r = entry("mid-point a step inside r", 0, flip(0)); a = line(float(step(u + r, False)), v, 64.0, 0.0, 0, flip(4)); want.append((a, 4))
    u, v, r = entry("mid-point a step beyond r", 0, flip(0)); line(float(step(u + r, True)), v, 64.0, 0.0, 0, flip(5)); want.append((-1, 256))
    # the cosine gate
    dy_in, dy_out = cos_pair()
    u, v, r = entry("cosine on the limit's inside", 0, flip(0)); a = line(u, v, 64.0, float(dy_in), 0, flip(6)); want.append((a, 6))
    u, v, r = entry("cosine a step outside", 0, flip(0)); line(u, v, 64.0, float(dy_out), 0, flip(7)); want.append((-1, 256))
    u, v, r = entry("a zero-length key line passes (NaN)", 0, flip(0)); a = line(u + 1.0, v, 0.0, 0.0, 0, flip(8)); want.append((a, 8))
    u, v, r = entry("a zero-length key line beyond r does not", 0, flip(0)); line(u + r + 1.0, v, 0.0, 0.0, 0, flip(8)); want.append((-1, 256))
    u, v, r = entry("a zero-length projection passes every direction (NaN)", 0, flip(0), zero=True); a = line(u, v + 1.0, 0.0, 64.0, 0, flip(9)); want.append((a, 9))
    # the band [level - 1, level]
    u, v, r = entry("octave above the band at level 0", 0, flip(0)); line(u, v, 64.0, 0.0, 1, flip(1)); a = line(u, v + 1.0, 64.0, 0.0, -1, flip(10)); want.append((a, 10))
    u, v, r = entry("band at the top level", top, flip(0))
    line(u, v, 64.0, 0.0, top - 2, flip(1)); line(u, v, 64.0, 0.0, top + 1, flip(2)); a = line(u, v + 1.0, 64.0, 0.0, top - 1, flip(12)); line(u, v - 1.0, 64.0, 0.0, top, flip(13))
    want.append((a, 12))
    # ties, acceptance, missing rows
    u, v, r = entry("equal distances: the lower index", 0, flip(0)); a = line(u + 1.0, v, 64.0, 0.0, 0, flip(20)); line(u - 1.0, v, 64.0, 0.0, 0, flip(20)); want.append((a, 20))
    u, v, r = entry("best distance 50 is accepted", 0, flip(0)); a = line(u, v, 64.0, 0.0, 0, flip(50)); want.append((a, 50))
    u, v, r = entry("best distance 51 is not", 0, flip(0)); a = line(u, v, 64.0, 0.0, 0, flip(51)); want.append((a, 51))
    u, v, r = entry("a strictly better later line wins", 0, flip(0)); line(u, v, 64.0, 0.0, 0, flip(30)); a = line(u, v + 0.5, -64.0, 0.0, 0, flip(29)); want.append((a, 29))
    if chunk_tie:
        u, v, r = entry("equal distances across the chunk boundary", 0, flip(0))
        while len(lines) < 255: far()
        a = line(u + 1.0, v, 64.0, 0.0, 0, flip(22))               # index 255: the last record of the first chunk
        line(u - 1.0, v, 64.0, 0.0, 0, flip(22))                   # index 256: the first of the second
        line(u, v + 1.0, 64.0, 0.0, 0, flip(23))
        want.append((a, 22))
        while len(lines) < 300: far()
    # start = (dx, dy), end = the origin: start - end is exact.  GetLinesInArea reads the position from pt alone, which is set apart
    kl = keylines(kl_dt, [(dx, dy, 0.0, 0.0, o) for cx, cy, dx, dy, o in lines])
    for i, (cx, cy, dx, dy, o) in enumerate(lines): kl["pt_x"][i] = cx; kl["pt_y"][i] = cy
    return make_kf(kl, np.stack(rows)), make_map(ent), np.array([w[0] for w in want], np.int32), np.array([w[1] for w in want], np.int32), names


def short_rows(kl_dt):
    """the as-written call with ORB rows: 6 lines, 4 rows.  Entry 0's best line (index 5) and its runner-up (index 4) have no row; index 2
    wins.  Entry 1 sees only lines without a row -> (kf, mp, best_idx, best_dist)"""
    P0 = seg_px(100.0 - 32.0, 100.0, 100.0 + 32.0, 100.0); P1 = seg_px(300.0 - 32.0, 100.0, 300.0 + 32.0, 100.0)
    rows = [(100.0, 101.0, 36.0, 101.0, 0), (500.0, 400.0, 520.0, 400.0, 0), (132.0, 100.5, 68.0, 100.5, 0), (500.0, 420.0, 520.0, 420.0, 0),
            (132.0, 99.5, 68.0, 99.5, 0), (132.0, 100.0, 68.0, 100.0, 0), (332.0, 100.0, 268.0, 100.0, 0)]
    kl = keylines(kl_dt, rows)
    mp = make_map([(P0, normal_of(P0), max_for_level(mid_dist(P0), 0), 0.01, flip(0)), (P1, normal_of(P1), max_for_level(mid_dist(P1), 0), 0.01, flip(0))])
    return make_kf(kl, np.stack([flip(40), flip(2), flip(33), flip(2)])), mp, np.array([2, -1], np.int32), np.array([33, 256], np.int32)


# ---- the random scene ----
SCENE_SEED, SCENE_KF, SCENE_LINES, SCENE_ENTRIES, SCENE_LEVELS = 7, 3, 120, 150, 3


def _flip_bits(rng, d, k):
    bits = np.unpackbits(d); bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def random_scene(kl_dt, n_kf=SCENE_KF, n_lines=SCENE_LINES, n=SCENE_ENTRIES, seed=SCENE_SEED, n_levels=SCENE_LEVELS, cam=pm.CAM, bounds=pm.BOUNDS, pose_ids=None):
    """n_kf key frames of n_lines key lines each and ONE map side of n entries.  W = 3/4 n_lines of the world segments are seen by every key frame
    (their projections under its true pose; the search runs under point_map_ref.estimated_pose); a sixth of n_lines are twins (a line of the
    first kind half a pixel away with the same descriptor and octave: ties), the rest random lines; each key frame's lines are shuffled.
    Entry i < min(W, 3/5 n) is world segment i with 0 .. 45 bits of its descriptor flipped and the level of its octave; the others cycle
    through the gates 1 .. 7 (7: a level far above the table).  pose_ids: point_map_ref.scene_pose's argument per key frame (default: its
    index, two degrees apart) -> (kfs, mp)"""
    rng = np.random.RandomState(seed)
    W = max(n_lines * 3 // 4, min(n_lines, 1)); n_twin = n_lines // 6
    Ww = max(W, 8); n_good = min(Ww, n * 3 // 5)                   # world segments: a key frame with few lines still has entries in view
    fx, fy, cx, cy = cam[:4]
    pose_ids = list(range(n_kf)) if pose_ids is None else pose_ids
    Ttrue = [np.asarray(pm.scene_pose(pose_ids[j]), np.float64).reshape(3, 4) for j in range(n_kf)]
    Test = [pm.estimated_pose(pm.scene_pose(pose_ids[j]), 0.001 * (pose_ids[j] + 1)) for j in range(n_kf)]

    def back(T, u, v, z):
        Xc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        return T[:, :3].T @ (Xc - T[:, 3])

    def proj(T, X):
        Xc = T[:, :3] @ X + T[:, 3]
        return fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
    seg_w = np.zeros((Ww, 6)); octv = rng.randint(0, n_levels, Ww); wdesc = rng.randint(0, 256, (Ww, 32)).astype(np.uint8)
    for w in range(Ww):
        u = rng.uniform(120, 520); v = rng.uniform(100, 380); ang = rng.uniform(0, np.pi); L = rng.uniform(20, 60); z = rng.uniform(1.5, 4.0)
        seg_w[w, :3] = back(Ttrue[0], u - L * np.cos(ang), v - L * np.sin(ang), z); seg_w[w, 3:] = back(Ttrue[0], u + L * np.cos(ang), v + L * np.sin(ang), z * rng.uniform(0.9, 1.1))
    kfs = []
    for j in range(n_kf):
        rows, desc = [], []
        for w in range(W):
            a = proj(Ttrue[j], seg_w[w, :3]); b = proj(Ttrue[j], seg_w[w, 3:])
            rows.append((a[0], a[1], b[0], b[1], int(octv[w]))); desc.append(_flip_bits(rng, wdesc[w], int(rng.randint(0, 6))))
        for k in range(min(n_twin, W)):
            r = rows[3 * k % W]; rows.append((r[0] + 0.5, r[1] - 0.25, r[2] + 0.5, r[3] - 0.25, r[4])); desc.append(desc[3 * k % W])
        while len(rows) < n_lines:
            u = rng.uniform(20, 620); v = rng.uniform(20, 460); ang = rng.uniform(0, np.pi); L = rng.uniform(10, 60)
            rows.append((u - L * np.cos(ang), v - L * np.sin(ang), u + L * np.cos(ang), v + L * np.sin(ang), int(rng.randint(0, n_levels)))); desc.append(rng.randint(0, 256, 32).astype(np.uint8))
        rows, desc = rows[:n_lines], desc[:n_lines]
        order = rng.permutation(n_lines)
        kl = keylines(kl_dt, [rows[q] for q in order])
        kfs.append(make_kf(kl, np.stack([desc[q] for q in order]) if n_lines else np.zeros((0, 32), np.uint8), Tcw=Test[j], cam=cam, bounds=bounds,
                           skip=np.zeros(n, np.uint8)))
    _, _, Ow = pm.pose_parts(Test[0])
    ent = []
    for i in range(n):
        w = i if i < n_good else int(rng.randint(0, Ww))
        P = seg_w[w].copy()
        mid = (0.5 * (P[:3] + P[3:])).astype(np.float32)
        d = pm._dist(mid, Ow)
        mx = max_for_level(d, int(octv[w])); mn = F32(mx / 4.0)
        dd = 0.5 * (P[:3] + P[3:]) - Ow.astype(np.float64); nrm = dd / np.linalg.norm(dd)
        qd = _flip_bits(rng, wdesc[w], int(rng.randint(0, 46)))
        if i >= n_good:
            g = 1 + (i - n_good) % 7
            if g == SKIP:
                for kf in kfs: kf["skip"][i] = 1
            elif g == BEHIND: P[3 * (i % 2):3 * (i % 2) + 3] = back(Ttrue[0], 300.0, 200.0, -2.0)
            elif g == OUT_OF_IMAGE: P[3 * (i % 2):3 * (i % 2) + 3] = back(Ttrue[0], -60.0 if i % 4 < 2 else 700.0, 200.0, 2.0)
            elif g == DIST_MIN: mn = F32(mx * 4.0)
            elif g == DIST_MAX: mx = F32(mx * 0.1); mn = F32(mx * 0.1)
            elif g == VIEW_ANGLE: nrm = -nrm
            else: mx = F32(mx * 100.0)
        ent.append((P, nrm, mx, mn, qd))
    for j, kf in enumerate(kfs):                                   # IsInKeyFrame differs per key frame
        if n: kf["skip"][(np.arange(n) + j) % 23 == 0] = 1
    return kfs, make_map(ent)


def scene_vacuity(ws, n, level_rule):
    """what the random scene must show on the restatement's own output, over its key frames"""
    gates = set()
    for w in ws: gates |= set(np.unique(w["gate"]).tolist())
    assert gates == set(range(8 if level_rule == AS_WRITTEN else 7)), (level_rule, sorted(gates))
    assert sum(w["n_fused"] for w in ws) * 4 >= n * len(ws), [w["n_fused"] for w in ws]
    assert sum(int((w["n_ties"] > 1).sum()) for w in ws) >= 10, [int((w["n_ties"] > 1).sum()) for w in ws]
    for w in ws:
        x = w["level_exact"][np.isfinite(w["level_exact"])]
        assert (np.abs(x - np.round(x)) > 1e-3).all(), "a predicted level within 1e-3 of an integer: the library log may round it either way"


IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def map_from_frame(kl, ldesc, cam, seed, n_levels=2, copies=1):
    """a map side made from an extracted frame's own key lines under the identity pose: entry i is key line i's (i modulo the line count with
    `copies` > 1) segment at 2 .. 3 m with up to 45 bits of its descriptor flipped and the level of its octave; every fifth entry is moved a
    few pixels, every seventh lies behind"""
    rng = np.random.RandomState(seed)
    fx, fy, cx, cy = cam[:4]
    ent = []
    for e in range(len(kl) * copies):
        i = e % len(kl)
        z = rng.uniform(2.0, 3.0); off = 6.0 if e % 5 == 4 else 0.0
        P = np.array([(kl["sx"][i] + off - cx) / fx * z, (kl["sy"][i] - cy) / fy * z, z, (kl["ex"][i] + off - cx) / fx * z, (kl["ey"][i] - cy) / fy * z, z], np.float64)
        if e % 7 == 6: P[2] = -z
        mid = (0.5 * (P[:3] + P[3:])).astype(np.float32)
        d = pm._dist(mid, np.zeros(3, np.float32))
        nrm = 0.5 * (P[:3] + P[3:]); nrm = nrm / max(np.linalg.norm(nrm), 1e-30)
        mx = max_for_level(d, min(max(int(kl["octave"][i]), 0), n_levels - 1))
        ent.append((P, nrm, mx, F32(mx / 4.0), _flip_bits(rng, np.asarray(ldesc[i], np.uint8), int(rng.randint(0, 46)))))
    return make_map(ent)


def cut(kf, m):
    """the key frame with its first m lines (and rows)"""
    return dict(kf, kl=kf["kl"][:m], desc_rows=kf["desc_rows"][:m])


# ---- the toy map of examples/fuse_line_neighbors.cpp and what its two calls and walks print ----
TOY_W, TOY_BEHIND = 12, 12


def _toy_world(k):
    ua, va = 80 + 40 * k, 100 + 20 * k; ub, vb = ua + 48, va + 8 * (k % 3)
    return [0.0, (ua - 320) / 256 - 0.5, (va - 240) / 256 + 0.25, 0.0, (ub - 320) / 256 - 0.5, (vb - 240) / 256 + 0.25]


def _toy_desc(k, flipped):
    return flip(flipped, ((7 * np.arange(32) + 3 + 13 * k) & 255).astype(np.uint8))


def toy_run(kl_dt, stop_on_behind, fuse_call=None):
    """-> the lines the example prints for one run.  fuse_call(kfs, mp) -> one result per key frame (default: this restatement)"""
    fuse_call = fuse_call or (lambda kfs, mp: [fuse(kf, mp, n_levels=1) for kf in kfs])
    lines, kfs = [], []

    def add_line(k, flipped, kf, idx, outside):
        m = dict(pos=[-4, -0.5, 0.25, -4, -0.25, 0.25] if k == TOY_BEHIND else _toy_world(k), desc=np.zeros(32, np.uint8) if k == TOY_BEHIND else _toy_desc(k, flipped),
                 bad=False, obs=[(kf, idx)] + [(-1, q) for q in range(outside)])
        lines.append(m); kfs[kf]["ml"][idx] = len(lines) - 1
    seg_of = lambda j, i: ((i if i < 5 else TOY_BEHIND if i == 5 else i - 1) if j == 0 else (i + TOY_W - 3 * j) % TOY_W)
    for j in range(3):
        n = TOY_W + 1 if j == 0 else TOY_W
        rows, desc = [], []
        for i in range(n):
            k = seg_of(j, i)
            if k == TOY_BEHIND: rows.append((10.0, 10.0, 30.0, 10.0, 0)); desc.append(np.zeros(32, np.uint8))
            else:
                sx, sy = 80.0 + 40 * k + 2 * j, 100.0 + 20 * k
                rows.append((sx, sy, sx + 48, sy + 8 * (k % 3), 0)); desc.append(_toy_desc(k, (k + j) % 4))
        T = np.array([[0, 1, 0, 0.5 + j / 128.0], [0, 0, 1, -0.25], [1, 0, 0, 2]], np.float32)
        kfs.append(dict(kf=make_kf(keylines(kl_dt, rows), np.stack(desc), Tcw=T), ml=[-1] * n))
    for i in range(TOY_W + 1):
        k = seg_of(0, i); add_line(k, 0, 0, i, 1 if (k != TOY_BEHIND and k % 4 == 0) else 0)
    for k in range(0, TOY_W, 3): add_line(k, 1, 1, (k + 3) % TOY_W, 2 if k % 6 == 0 else 0)
    for k in range(1, TOY_W, 4): add_line(k, 2, 2, (k + 6) % TOY_W, 1 if k == 5 else 0)
    in_kf = lambda m, kf: any(o[0] == kf for o in m["obs"])

    def replace(a, b):
        if a == b: return
        obs, lines[a]["obs"] = lines[a]["obs"], []
        lines[a]["bad"] = True
        for o in obs:
            if o[0] < 0: lines[b]["obs"].append(o)
            elif not in_kf(lines[b], o[0]): kfs[o[0]]["ml"][o[1]] = b; lines[b]["obs"].append(o)
            else: kfs[o[0]]["ml"][o[1]] = -1

    def do_walk(what, kf, entries, res):
        seen = []

        def on_fused(e, idx):
            pML, inKF = entries[e], kfs[kf]["ml"][idx]
            seen.append((e, idx))
            if inKF >= 0:
                if lines[inKF]["bad"]: return False
                if len(lines[inKF]["obs"]) > len(lines[pML]["obs"]): replace(pML, inKF)
                else: replace(inKF, pML)
                return True
            lines[pML]["obs"].append((kf, idx)); kfs[kf]["ml"][idx] = pML
            return False
        w = walk(res, lambda e: entries[e] < 0 or lines[entries[e]]["bad"] or in_kf(lines[entries[e]], kf), on_fused, stop_on_behind)
        return "%s kf %d: fused %d stopped_at %d replaced %d |%s" % (what, kf, w["n_fused"], w["stopped_at"], 1 if w["replaced"] else 0, "".join(" %d>%d" % s for s in seen))
    side = lambda idx: make_map([(lines[i]["pos"], (1.0, 0.0, 0.0), 3.0, 1.0, lines[i]["desc"]) for i in idx])
    out = ["stop_on_behind %d" % (1 if stop_on_behind else 0)]
    cur = list(kfs[0]["ml"])
    targets = [dict(kfs[j]["kf"], skip=np.array([c < 0 or lines[c]["bad"] or in_kf(lines[c], j) for c in cur], np.uint8)) for j in (1, 2)]
    res = fuse_call(targets, side(cur))
    for j in (1, 2): out.append(do_walk("call 1", j, cur, res[j - 1]))
    cand = []
    for j in (1, 2):
        for pML in kfs[j]["ml"]:
            if pML < 0 or lines[pML]["bad"] or pML in cand: continue
            cand.append(pML)
    current = dict(kfs[0]["kf"], skip=np.array([in_kf(lines[c], 0) for c in cand], np.uint8))
    res = fuse_call([current], side(cand))
    out.append(do_walk("call 2", 0, cand, res[0]))
    out.append("bad:%s | observations:%s" % ("".join(" %d" % i for i, m in enumerate(lines) if m["bad"]), "".join(" %d" % len(m["obs"]) for m in lines)))
    return out
