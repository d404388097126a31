"""CPU restatement of the new map points and map lines of Tracking::CreateNewKeyFrame (reference src/Tracking.cc:3032-3187), of
Tracking::StereoInitialization (1364-1400) and of the temporal points of Tracking::UpdateLastFrame (2194-2246), with Frame::UnprojectStereo
(src/Frame.cc:2088-2102), Frame::PtToWorldCoord (include/Frame.h:147-150), the two MapPoint constructors (src/MapPoint.cc:32-69),
MapPoint::UpdateNormalAndDepth / MapLine::UpdateAverageDir for a single observer and Manhattan::computeStructConstrains(Frame &, MapLine *, ..)
(src/Manhattan.cpp:66-105).  Test infrastructure only, and THE DEFINITION of what csrc/new_keyframe.hip computes: the selection is written as
the reference writes it (sort, counters, break); the closed forms the kernels use stand beside it and tests/test_new_keyframe.py holds them
equal on every case.

Readings (the shared ones are imported: map_refresh_ref, point_map_ref, line_map_ref):
  held                 mvpMapPoints[i] / mvpMapLines[i] as a slot, -1, FOREIGN_OBSERVED or FOREIGN_UNOBSERVED; `Observations() < 1` is a slot
                       without the observed flag or FOREIGN_UNOBSERVED
  sort                 pair<float, int>: (z, i), equal depths by index.  The line key is (float)(sz > ez ? sz : ez); a NaN key leaves the
                       sort undefined: the frame is refused (Refused)
  UnprojectStereo      x = (u - cx) * z * invfx in float, left to right, invfx = 1.0f / fx; mRwc * x3Dc + mOw by point_map_ref.transform with
                       mRwc = Rcw^T and mOw of pose_parts
  point normal         key frame / init: map_refresh_ref.point_geometry with the one observer (0 + u, then times 1 / 1: -0.0 becomes +0.0);
                       temporal: the Frame constructor's (P - Ow) / norm: Mat / scalar, no sum, -0.0 stays.  point_dist and the range as there
  PtToWorldCoord       Rwc and Ow widened to double, ((r0 p0 + r1 p1) + r2 p2) + Ow
  line                 world_vector, line_geometry, line_dist of map_refresh_ref with the one observer, the key line's octave and
                       line_scale_factors (line_geometry = 1); normal 0 and distances 0 (line_geometry = 0)
  a level outside the table   the reference reads out of bounds.  Here the entry is counted by the loop as the reference counts it, gets
                       status BAD_LEVEL, takes no slot and is not created; a held value the loop cleared stays cleared
  computeAngle         dot / (|a| |b|) in double, sums left to right: the reading of line_map_ref.struct_rel"""
import math

import numpy as np

import line_map_ref as lm
import map_refresh_ref as mr
import point_map_ref as pm

F32 = np.float32
KEYFRAME, INIT, TEMPORAL = 0, 1, 2
CREATED, BAD_LEVEL = 0, 1
FOREIGN_OBSERVED, FOREIGN_UNOBSERVED = pm.FOREIGN_OBSERVED, pm.FOREIGN_UNOBSERVED
MAX_FEATURES, MAX_LINES = 16384, 2048
COS_PAR, COS_PERP = math.cos(3.0 * 0.0174533), math.cos((90.0 - 3.0) * 0.0174533)
KEYPOINT_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


class Refused(Exception):
    pass


def creatable(h, observed):
    """bCreateNew: !pMP, or pMP->Observations() < 1"""
    if h == -1 or h == FOREIGN_UNOBSERVED: return True
    if h == FOREIGN_OBSERVED: return False
    return not observed[h]


# ------------------------------------------------------------------------------------------------ the loops as the reference writes them
def point_loop(depth, held, observed, th):
    """Tracking.cc:3049-3097 (and 2196-2246): -> (entries, processed) as feature indices in loop order; entries are the bCreateNew ones"""
    v = [(float(z), i) for i, z in enumerate(depth) if z > 0]
    entries, processed = [], []
    if not v: return entries, processed
    v.sort()
    n_points = 0
    for z, i in v:
        processed.append(i)
        if creatable(int(held[i]), observed): entries.append(i)
        n_points += 1
        if z > th and n_points > 100: break
    return entries, processed


def line_key(A, B):
    sz, ez = float(A[2]), float(B[2])
    with np.errstate(all="ignore"):
        return float(F32(sz if sz > ez else ez))


def line_loop(l3d_A, l3d_B, held, observed, th):
    """Tracking.cc:3102-3187: the counter and the break sit inside `if (bCreateNew)`"""
    v = []
    for i in range(len(l3d_A)):
        if l3d_A[i][2] == 0 or l3d_B[i][2] == 0: continue
        z = line_key(l3d_A[i], l3d_B[i])
        if z != z: raise Refused("a NaN line depth")
        v.append((z, i))
    entries = []
    if not v: return entries
    v.sort()
    n_lines = 0
    for z, i in v:
        if creatable(int(held[i]), observed):
            entries.append(i)                                    # (mvLines3D[i].first.z() != 0.0 holds for every candidate: both arms count)
            n_lines += 1
            if z > th and n_lines > 100: break
    return entries


def init_points(depth):
    return [i for i, z in enumerate(depth) if z > 0]


def init_lines(kl_sx, l3d_A):
    return [i for i in range(len(kl_sx)) if kl_sx[i] > 0.0 and l3d_A[i][0] != 0]


# ------------------------------------------------------------------------------------------------ the closed forms the kernels use
def _ranks(keys, cand, creat):
    order = sorted((keys[i], i) for i in range(len(keys)) if cand[i])
    rank = {i: r for r, (_, i) in enumerate(order)}
    crank, k = {}, 0
    for _, i in order:
        crank[i] = k
        if creat[i]: k += 1
    return order, rank, crank


def point_closed(depth, held, observed, th):
    n = len(depth)
    cand = [depth[i] > 0 for i in range(n)]; creat = [cand[i] and creatable(int(held[i]), observed) for i in range(n)]
    order, rank, _ = _ranks([float(z) for z in depth], cand, creat)
    M = len(order); c = sum(1 for z, _ in order if z <= th)
    limit = max(c, 100)
    processed = [i for _, i in order if rank[i] <= limit]
    assert len(processed) == min(M, limit + 1)
    return [i for i in processed if creat[i]], processed


def line_closed(l3d_A, l3d_B, held, observed, th):
    n = len(l3d_A)
    cand = [not (l3d_A[i][2] == 0 or l3d_B[i][2] == 0) for i in range(n)]
    keys = [line_key(l3d_A[i], l3d_B[i]) for i in range(n)]
    if any(cand[i] and keys[i] != keys[i] for i in range(n)): raise Refused("a NaN line depth")
    creat = [cand[i] and creatable(int(held[i]), observed) for i in range(n)]
    order, _, crank = _ranks(keys, cand, creat)
    c = sum(1 for z, i in order if creat[i] and z <= th)
    return [i for _, i in order if creat[i] and crank[i] <= max(c, 100)]


# ------------------------------------------------------------------------------------------------ one entry
def camera_parts(Tcw):
    """mRwc (rows), mOw"""
    R, _, Ow = pm.pose_parts(Tcw)
    return R.T.copy(), Ow


def unproject(u, v, z, cam, Rwc, Ow):
    fx, fy, cx, cy = (F32(t) for t in cam[:4])
    with np.errstate(all="ignore"):
        invfx, invfy = F32(F32(1.0) / fx), F32(F32(1.0) / fy)
        x = F32(F32(F32(F32(u) - cx) * F32(z)) * invfx); y = F32(F32(F32(F32(v) - cy) * F32(z)) * invfy)
        return pm.transform(Rwc, Ow, np.array([x, y, F32(z)], F32))


def point_entry(P, Ow, level, n_levels, sf, temporal):
    """(normal, max_dist, min_dist) of a new point seen from Ow alone"""
    Pf = [float(t) for t in P]; O = [float(t) for t in Ow]
    with np.errstate(all="ignore"):
        if temporal:
            d = [mr.f32(Pf[c] - O[c]) for c in range(3)]
            inv = mr.ddiv(1.0, mr.dsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
            nrm = [mr.f32(d[c] * inv) for c in range(3)]
        else:
            nrm = mr.point_geometry(Pf, [O])
        dist = mr.point_dist(Pf, O)
        mx = mr.f32(dist * float(sf[level])); mi = mr.f32(mr.ddiv(mx, float(sf[n_levels - 1])))
    return np.array(nrm, F32), F32(mx), F32(mi)


def pt_to_world(Rwc, Ow, P):
    R = np.asarray(Rwc, F32).astype(np.float64); O = np.asarray(Ow, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        return [float(((R[r, 0] * P[0] + R[r, 1] * P[1]) + R[r, 2] * P[2]) + O[r]) for r in range(3)]


def line_entry(A, B, Rwc, Ow, level, n_levels, lsf, line_geometry):
    """(pos 6, wvec, normal, max_dist, min_dist)"""
    P = pt_to_world(Rwc, Ow, [float(t) for t in A]) + pt_to_world(Rwc, Ow, [float(t) for t in B])
    O = [float(t) for t in Ow]
    with np.errstate(all="ignore"):
        w = mr.world_vector(P)
        if not line_geometry:
            return np.array(P), np.array(w), np.zeros(3), F32(0), F32(0)
        nrm = mr.line_geometry(P, [O])
        mx = mr.f32(mr.line_dist(P, O) * lsf[level]); mi = mr.f32(mr.ddiv(mx, lsf[n_levels - 1]))
    return np.array(P), np.array(w), np.array(nrm), F32(mx), F32(mi)


def compute_angle_abs(a, b):
    with np.errstate(all="ignore"):
        a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
        dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
        ma = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); mb = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        return np.abs(dot / (ma * mb))


def frame_dirs(l3d_A, l3d_B, Rwc, Ow):
    """line_ep_world - line_stp_world of every frame line (n, 3), the same operations as pt_to_world element by element"""
    R = np.asarray(Rwc, F32).astype(np.float64); O = np.asarray(Ow, F32).astype(np.float64)
    A = np.asarray(l3d_A, np.float64).reshape(-1, 3); B = np.asarray(l3d_B, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        w = lambda P: np.stack([((R[r, 0] * P[:, 0] + R[r, 1] * P[:, 1]) + R[r, 2] * P[:, 2]) + O[r] for r in range(3)], axis=1)
        return w(B) - w(A)


def struct_row(pos6, l3d_A, l3d_B, Rwc, Ow, cos_par=COS_PAR, cos_perp=COS_PERP, dirs=None):
    """computeStructConstrains of one new line against every frame line: 0 / 1 parallel / 2 perpendicular"""
    le = frame_dirs(l3d_A, l3d_B, Rwc, Ow) if dirs is None else dirs
    ml = [pos6[3 + c] - pos6[c] for c in range(3)]
    ang = compute_angle_abs(le.T, ml)
    row = np.where(ang < cos_perp, 2, np.where(ang > cos_par, 1, 0)).astype(np.uint8)
    row[np.asarray(l3d_A, np.float64).reshape(-1, 3)[:, 0] == 0.0] = 0
    return row


# ------------------------------------------------------------------------------------------------ the call
def create(mode, cam, Tcw, kp_un=None, depth=None, desc=None, keylines=None, ldesc=None, l3d_A=None, l3d_B=None, th_depth=3.0, held_points=None,
           held_lines=None, pt_observed=(), ln_observed=(), first_point_slot=-1, first_line_slot=-1, n_levels=pm.N_LEVELS, sf=pm.SF, line_n_levels=1,
           line_scale_factor=1.2, line_geometry=1, cos_par=COS_PAR, cos_perp=COS_PERP, closed=False):
    """-> dict of the arrays hvo_create_keyframe_features returns.  pt_observed / ln_observed: the observed flag of every slot of the two
    maps.  closed: select by the closed forms instead of the loops.  Raises Refused where the call refuses whole."""
    n_kp = 0 if kp_un is None else len(kp_un); n_kl = 0 if keylines is None or mode == TEMPORAL else len(keylines)
    if n_kp > MAX_FEATURES or n_kl > MAX_LINES: raise Refused("too many features")
    hp = np.full(n_kp, -1, np.int32) if held_points is None or mode == INIT else np.array(held_points, np.int32)[:n_kp].copy()
    hl = np.full(n_kl, -1, np.int32) if held_lines is None or mode == INIT else np.array(held_lines, np.int32)[:n_kl].copy()
    Rwc, Ow = camera_parts(Tcw)
    th = float(F32(th_depth))
    temporal = mode == TEMPORAL
    fp = -1 if temporal else first_point_slot; fl = -1 if temporal else first_line_slot
    out = {}
    # points
    if mode == INIT: ents = init_points(depth) if n_kp else []
    else: ents = (point_closed if closed else point_loop)(depth, hp, pt_observed, th)[0] if n_kp else []
    idx, slot, status, pos, nrm, mx, mi = [], [], [], [], [], [], []
    k = 0
    for i in ents:
        lvl = int(kp_un["octave"][i]); idx.append(i)
        if not 0 <= lvl < n_levels:
            status.append(BAD_LEVEL); slot.append(-1); pos.append(np.zeros(3, F32)); nrm.append(np.zeros(3, F32)); mx.append(F32(0)); mi.append(F32(0))
            if not temporal: hp[i] = -1
            continue
        P = unproject(kp_un["x"][i], kp_un["y"][i], depth[i], cam, Rwc, Ow)
        n_, a_, b_ = point_entry(P, Ow, lvl, n_levels, sf, temporal)
        s = fp + k if fp >= 0 else -1
        k += 1
        status.append(CREATED); slot.append(s); pos.append(P); nrm.append(n_); mx.append(a_); mi.append(b_)
        hp[i] = s if s >= 0 else (FOREIGN_UNOBSERVED if temporal else FOREIGN_OBSERVED)
    out.update(held_points=hp, pt_index=np.array(idx, np.int32), pt_slot=np.array(slot, np.int32), pt_status=np.array(status, np.uint8),
               pt_pos=np.array(pos, F32).reshape(-1, 3), pt_normal=np.array(nrm, F32).reshape(-1, 3), pt_max_dist=np.array(mx, F32), pt_min_dist=np.array(mi, F32),
               pt_desc=np.asarray(desc, np.uint8).reshape(-1, 32)[idx] if idx else np.zeros((0, 32), np.uint8), n_points_created=k)
    # lines
    if n_kl:
        if mode == INIT: ents = init_lines(keylines["sx"], l3d_A)
        else: ents = (line_closed if closed else line_loop)(l3d_A, l3d_B, hl, ln_observed, th)
    else: ents = []
    lsf = mr.line_scale_factors(line_n_levels, line_scale_factor)
    dirs = frame_dirs(l3d_A, l3d_B, Rwc, Ow) if ents and mode == KEYFRAME else None
    idx, slot, status, pos, wv, nrm, mx, mi, rel = [], [], [], [], [], [], [], [], []
    k = 0
    for i in ents:
        lvl = int(keylines["octave"][i]); idx.append(i)
        if line_geometry and not 0 <= lvl < line_n_levels:
            status.append(BAD_LEVEL); slot.append(-1); pos.append(np.zeros(6)); wv.append(np.zeros(3)); nrm.append(np.zeros(3)); mx.append(F32(0)); mi.append(F32(0))
            rel.append(np.zeros(n_kl, np.uint8)); hl[i] = -1
            continue
        P, w, n_, a_, b_ = line_entry(l3d_A[i], l3d_B[i], Rwc, Ow, lvl, line_n_levels, lsf, line_geometry)
        s = fl + k if fl >= 0 else -1
        k += 1
        status.append(CREATED); slot.append(s); pos.append(P); wv.append(w); nrm.append(n_); mx.append(a_); mi.append(b_)
        if mode == KEYFRAME: rel.append(struct_row(P, l3d_A, l3d_B, Rwc, Ow, cos_par, cos_perp, dirs))
        hl[i] = s if s >= 0 else FOREIGN_OBSERVED
    out.update(held_lines=hl, ln_index=np.array(idx, np.int32), ln_slot=np.array(slot, np.int32), ln_status=np.array(status, np.uint8),
               ln_pos=np.array(pos, np.float64).reshape(-1, 6), ln_wvec=np.array(wv, np.float64).reshape(-1, 3), ln_normal=np.array(nrm, np.float64).reshape(-1, 3),
               ln_max_dist=np.array(mx, F32), ln_min_dist=np.array(mi, F32), n_lines_created=k,
               ln_desc=np.asarray(ldesc, np.uint8).reshape(-1, 32)[idx] if idx else np.zeros((0, 32), np.uint8),
               ln_rel=np.array(rel, np.uint8).reshape(-1, n_kl) if mode == KEYFRAME and n_kl else np.zeros((0, n_kl), np.uint8))
    return out


POINT_KEYS = ("held_points", "pt_index", "pt_slot", "pt_status", "pt_pos", "pt_normal", "pt_max_dist", "pt_min_dist")
LINE_KEYS = ("held_lines", "ln_index", "ln_slot", "ln_status", "ln_pos", "ln_wvec", "ln_normal", "ln_max_dist", "ln_min_dist", "ln_rel")
GEOMETRY_KEYS = ("pt_pos", "pt_normal", "pt_max_dist", "pt_min_dist", "ln_pos", "ln_wvec", "ln_normal", "ln_max_dist", "ln_min_dist")


def same_bits(a, b):
    """integers exact, floats by their bits, a NaN by being one"""
    a = np.asarray(a); b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype: return False
    if a.dtype.kind != "f": return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def compare(got, want, keys=POINT_KEYS + LINE_KEYS):
    """the keys that differ.  Geometry of an entry that was not created is not compared (the call leaves it unwritten)"""
    bad = []
    for k in keys:
        g, w = np.asarray(getattr(got, k) if not isinstance(got, dict) else got[k]), np.asarray(want[k])
        if k in GEOMETRY_KEYS and g.shape == w.shape:
            made = np.asarray(want["pt_status" if k.startswith("pt_") else "ln_status"]) == CREATED
            g, w = g[made], w[made]
        if not same_bits(g, w): bad.append(k)
    return bad


# ------------------------------------------------------------------------------------------------ scenes
def scene_pose(seed=0):
    return pm.scene_pose(seed)


HELD_PATTERNS = ("none", "slots", "foreign", "mixed")


def held_pattern(n, pattern, n_slots, rng):
    """what n features hold: nothing; a slot each (observed and unobserved ones, drawn from n_slots); the two foreign values in turn; a fifth each
    of -1, observed slots, unobserved slots (the caller's flags alternate: even slots are observed) and the two foreign values"""
    if pattern == "none": return np.full(n, -1, np.int32)
    if pattern == "slots": return rng.randint(0, n_slots, n).astype(np.int32)
    if pattern == "foreign": return np.where(np.arange(n) % 2 == 0, FOREIGN_OBSERVED, FOREIGN_UNOBSERVED).astype(np.int32)
    kind = rng.randint(0, 5, n); even = 2 * rng.randint(0, n_slots // 2, n)
    return np.select([kind == 0, kind == 1, kind == 2, kind == 3], [-1, even, even + 1, FOREIGN_OBSERVED], FOREIGN_UNOBSERVED).astype(np.int32)


def make_points(n, seed, z_lo=0.5, z_hi=6.0, zero_rate=0.1, levels=8):
    """n key points with depths in [z_lo, z_hi), a tenth without depth (0) and one negative"""
    rng = np.random.RandomState(seed)
    kp = np.zeros(n, KEYPOINT_DT)
    kp["x"] = rng.uniform(10, 630, n).astype(F32); kp["y"] = rng.uniform(10, 470, n).astype(F32); kp["octave"] = rng.randint(0, levels, n)
    z = rng.uniform(z_lo, z_hi, n).astype(F32)
    z[rng.uniform(size=n) < zero_rate] = 0
    if n > 3: z[3] = -1.0
    return kp, z, rng.randint(0, 256, (n, 32)).astype(np.uint8)


def make_lines(n, seed, z_lo=0.5, z_hi=6.0, zero_rate=0.1, keyline_dt=None):
    """-> (keylines, ldesc, A, B): camera-frame end points; a tenth have a zero end point"""
    rng = np.random.RandomState(seed)
    dt = keyline_dt or np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                                 ("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"), ("sox", "<f4"), ("soy", "<f4"), ("eox", "<f4"), ("eoy", "<f4"),
                                 ("length", "<f4"), ("num_pixels", "<i4")])
    kl = np.zeros(n, dt)
    kl["sx"] = rng.uniform(1, 630, n); kl["sy"] = rng.uniform(1, 470, n); kl["ex"] = rng.uniform(1, 630, n); kl["ey"] = rng.uniform(1, 470, n)
    A = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(z_lo, z_hi, n)])
    # directions near a few axes, so that parallel and perpendicular pairs exist
    axes = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0.6, 0.8, 0]])
    B = A + axes[rng.randint(0, 4, n)] * rng.uniform(0.2, 1.0, (n, 1)) + rng.normal(0, 0.004, (n, 3))
    B[:, 2] = np.where(B[:, 2] == 0, 0.5, B[:, 2])
    zero = rng.uniform(size=n) < zero_rate
    A[zero] = 0; B[zero] = 0
    return kl, rng.randint(0, 256, (n, 32)).astype(np.uint8), A, B
