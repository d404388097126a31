"""CPU restatement of PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:10-68) with PointDistanceFromPlane (:69-81) and
Frame::ComputePlaneWorldCoeff (src/Frame.cc:2275-2280), in scalar float32 arithmetic in the written order, the loop over the map planes as
the reference has it.  It is the yardstick of csrc/plane_assoc.hip (tests/test_plane_assoc.py checks it on known answers without a GPU,
tests/test_plane_assoc_gpu.py compares the device forms with it bit for bit), and it holds the seeded scene generator both use.

Readings taken: the 4 x 4 CV_32F product of ComputePlaneWorldCoeff has its products and sums in double, left to right
over r = 0..3, rounded to float once; `angle` and the point distances are float expressions evaluated left to right without contraction;
`abs` is the float overload; `double dis` holds a float value, so `dis < ldTh` and `ldTh = dis` are float comparisons and copies."""
import numpy as np

F32 = np.float32
DEFAULT_TH = (0.1, 0.86, 0.08716, 0.9962)        # include/PlaneMatcher.h:17
TUM3_TH = (0.05, 0.985, 0.08716, 0.9962)         # Plane.AssociationDisRef, AssociationAngRef, VerticalThreshold, ParallelThreshold (TUM3 settings)


def world_coeff(Tcw, coef):
    """Frame::ComputePlaneWorldCoeff (Frame.cc:2275-2280): transpose(mTcw) * mvPlaneCoefficients[idx]; Tcw = rows 0..2 (3 x 4), row 3 = (0, 0, 0, 1)"""
    T = np.vstack([np.asarray(Tcw, F32).reshape(3, 4), np.array([[0, 0, 0, 1]], F32)]).astype(np.float64)
    c = np.asarray(coef, F32).astype(np.float64)
    out = np.zeros(4, F32)
    with np.errstate(all="ignore"):
        for k in range(4):
            s = T[0, k] * c[0]
            for r in range(1, 4):
                s = s + T[r, k] * c[r]
            out[k] = F32(s)
    return out


def point_distances(pM, xyz):
    """|pM0 x + pM1 y + pM2 z + pM3| of every point, float32, left to right (PlaneMatcher.cpp:72-75)"""
    p = np.asarray(pM, F32); c = np.asarray(xyz, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.abs(((p[0] * c[:, 0] + p[1] * c[:, 1]) + p[2] * c[:, 2]) + p[3])


def point_distance_from_plane(pM, xyz):
    """PointDistanceFromPlane (PlaneMatcher.cpp:69-81): res = 100; `if (dis < res) res = dis` over the cloud -- a NaN distance never wins"""
    d = point_distances(pM, xyz)
    d = d[d < F32(100.0)]
    return F32(d.min()) if len(d) else F32(100.0)


def search_map(coef, Tcw, slots, th=DEFAULT_TH):
    """SearchMapByCoefficients.  coef: (n, 4) camera-frame plane coefficients; slots: list of (coef4, xyz (m, 3), bad) in the caller's order.
    Returns dict(n_planes, n_matches, match, vertical, parallel, dist, pM, dist_mat, angle_mat, fell_through): the slot arrays hold -1 where
    the reference leaves NULL; dist is the matched distance (100 without a match); dist_mat holds 100 where the gate did not pass or the slot
    is bad; angle_mat is computed for bad slots too; fell_through[i] lists the slots that passed the angle gate, were not consumed by the
    association and went on to the vertical / parallel tests."""
    coef = np.asarray(coef, F32).reshape(-1, 4)
    n, ns = len(coef), len(slots)
    dTh, aTh, verTh, parTh = (F32(v) for v in th)
    out = dict(n_planes=n, n_matches=0, match=np.full(n, -1, np.int32), vertical=np.full(n, -1, np.int32), parallel=np.full(n, -1, np.int32),
               dist=np.full(n, 100.0, F32), pM=np.zeros((n, 4), F32), dist_mat=np.full((n, ns), 100.0, F32), angle_mat=np.zeros((n, ns), F32),
               fell_through=[[] for _ in range(n)])
    W = [np.asarray(s[0], F32) for s in slots]
    with np.errstate(all="ignore"):
        for i in range(n):                                                   # PlaneMatcher.cpp:16
            pM = world_coeff(Tcw, coef[i]); out["pM"][i] = pM
            ldTh, lverTh, lparTh = dTh, verTh, parTh                         # :20-22
            found = False
            for j in range(ns):                                              # :25
                pW = W[j]
                angle = F32(F32(F32(pM[0] * pW[0]) + F32(pM[1] * pW[1])) + F32(pM[2] * pW[2]))     # :31-33
                out["angle_mat"][i, j] = angle
                if slots[j][2]:                                              # :26 isBad
                    continue
                if angle > aTh or angle < -aTh:                              # :36
                    dis = point_distance_from_plane(pM, slots[j][1])         # :38
                    out["dist_mat"][i, j] = dis
                    if dis < ldTh:                                           # :39
                        ldTh = dis; out["match"][i] = j; out["dist"][i] = dis; found = True
                        continue
                    out["fell_through"][i].append(j)
                if angle < lverTh and angle > -lverTh:                       # :49
                    lverTh = F32(abs(angle)); out["vertical"][i] = j
                    continue
                if angle > lparTh or angle < -lparTh:                        # :57
                    lparTh = F32(abs(angle)); out["parallel"][i] = j
            if found:
                out["n_matches"] += 1
    return out


# ---- poses and the seeded scene generator ---------------------------------------------------------------------------------------------

def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg); K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pose(R, t):
    """rows 0..2 of Tcw as (3, 4) float32"""
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)]).astype(F32)


def camera_coef(Tcw, world):
    """a world plane's coefficients in the camera frame, in float64 (the inverse of ComputePlaneWorldCoeff): Tcw^-T world"""
    T = np.vstack([np.asarray(Tcw, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    return np.linalg.solve(T.T, np.asarray(world, np.float64)).astype(F32)


def plane_cloud(rng, world, n, extent=2.0, noise=0.003):
    """n points near the world plane (unit normal, d): a patch of the given extent around the plane's point nearest a random centre"""
    nrm = np.asarray(world[:3], np.float64); d = float(world[3])
    u = np.cross(nrm, [0.3, -0.5, 0.8]); u /= np.linalg.norm(u); v = np.cross(nrm, u)
    c = rng.uniform(-2.0, 2.0, 3); c = c - (nrm @ c + d) * nrm
    ab = rng.uniform(-extent, extent, (n, 2))
    return (c + ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0.0, noise, (n, 1)) * nrm).astype(F32)


def make_scene(seed, n_slots, total_points, n_frame=12, big_share=0.0):
    """A Manhattan room: three families of map planes (walls, floors, at several offsets) plus oblique ones, in the caller's order shuffled;
    cloud sizes log-uniform in 1 .. ~50 000 scaled to total_points, none a multiple of 64 on purpose, a few empty, a few bad, a few with NaN
    points; big_share > 0 gives one slot that share of all points.  The frame sees some of the map's planes under a jittered pose, plus
    planes that are in no map slot.  Returns (coef (n_frame, 4), Tcw (3, 4), slots)."""
    rng = np.random.RandomState(seed)
    Rw = rot(rng.normal(size=3), rng.uniform(0, 180))                       # the room's axes in the world
    slots = []
    sizes = np.exp(rng.uniform(0.0, np.log(50000.0), n_slots)) if n_slots else np.zeros(0)
    if n_slots:
        sizes = sizes * (total_points * (1.0 - big_share) / sizes.sum())
        sizes = np.clip(sizes.astype(np.int64), 1, 50000)
        sizes[sizes % 64 == 0] += 1
        if big_share > 0:
            sizes[rng.randint(n_slots)] = int(total_points * big_share) | 1
    worlds = []
    for j in range(n_slots):
        kind = rng.randint(8)
        if kind < 6:                                                         # a family plane, slightly off its axis
            nrm = Rw[:, kind % 3] * (1.0 if kind < 3 else -1.0) + rng.normal(0, 0.004, 3)
        else:                                                                # oblique
            nrm = rng.normal(size=3)
        nrm = nrm / np.linalg.norm(nrm)
        w = np.array([nrm[0], nrm[1], nrm[2], rng.choice([-3.0, -2.0, -1.0, -0.5, 0.5, 1.0, 2.0, 3.0]) + rng.normal(0, 0.01)])
        worlds.append(w)
        r = rng.rand()
        npts = 0 if r < 0.02 else int(sizes[j])
        xyz = plane_cloud(rng, w, npts) if npts else np.zeros((0, 3), F32)
        if npts and r > 0.97:
            xyz[rng.randint(npts, size=max(1, npts // 7))] = np.nan          # NaN points never win the minimum
        slots.append((w.astype(F32), xyz, bool(0.02 <= r < 0.06)))
    Rcw = rot(rng.normal(size=3), rng.uniform(0, 180)); Tcw = pose(Rcw, rng.uniform(-1.5, 1.5, 3))
    coef = np.zeros((n_frame, 4), F32)
    for i in range(n_frame):
        r = rng.rand()
        if n_slots and r < 0.6:                                              # a map plane seen again, jittered in angle and offset
            w = worlds[rng.randint(n_slots)].copy()
            w[:3] += rng.normal(0, 0.01, 3); w[:3] /= np.linalg.norm(w[:3]); w[3] += rng.normal(0, 0.02)
        elif r < 0.85:                                                       # a family plane at an offset no slot has
            nrm = Rw[:, rng.randint(3)] * rng.choice([-1.0, 1.0]); w = np.array([nrm[0], nrm[1], nrm[2], rng.uniform(5.0, 9.0)])
        else:
            nrm = rng.normal(size=3); nrm /= np.linalg.norm(nrm); w = np.array([nrm[0], nrm[1], nrm[2], rng.uniform(-3, 3)])
        coef[i] = camera_coef(Tcw, w)
    return coef, Tcw, slots


# the generated cases of the CPU and GPU tests: (seed, slots, total points, frame planes, share of the points in one slot)
SCENES = [(101, 0, 0, 5, 0.0), (102, 1, 37, 3, 0.0), (103, 63, 9000, 12, 0.0), (104, 130, 60000, 20, 0.0), (105, 517, 150000, 33, 0.0),
          (106, 300, 400000, 64, 0.7)]
BIG_SCENE = (107, 3001, 1100000, 40, 0.3)          # a few thousand slots, more than 1 M points (GPU test only: the restatement takes a while)


def scene_stats(o):
    """what a result exercises: counts of match / vertical / parallel / fall-through / unmatched frame planes"""
    return dict(match=int((o["match"] >= 0).sum()), vertical=int((o["vertical"] >= 0).sum()), parallel=int((o["parallel"] >= 0).sum()),
                fell=int(sum(len(f) for f in o["fell_through"])), unmatched=int((o["match"] < 0).sum()),
                fell_parallel=int(sum(int(o["parallel"][i] in f) for i, f in enumerate(o["fell_through"]))))


# ---- crafted known-answer cases -----------------------------------------------------------------------------------------------------------
# Poses under which the 4 x 4 product is exact in float and in double alike: an axis-permutation rotation and a dyadic translation.  The frame
# plane is built so that pM = (1, 0, 0, 0) exactly (the world plane x = 0): a slot with coefficients (a, ., ., .) has angle a exactly, and a
# cloud point with x = d has distance |d| exactly.

PERM = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float64)
T_EXACT = pose(PERM, (0.5, -0.25, 2.0))


def exact_frame_plane(d=0.0):
    """camera-frame coefficients whose world coefficients under T_EXACT are (1, 0, 0, d) exactly (d dyadic)"""
    n = PERM @ np.array([1.0, 0.0, 0.0])
    return np.array([n[0], n[1], n[2], d - np.array([0.5, -0.25, 2.0]) @ n], F32)


def slot(angle, dists, bad=False):
    """a map slot whose angle with the exact frame plane is `angle` and whose cloud has the distances `dists` (NaN allowed)"""
    d = np.asarray(dists, F32).reshape(-1)
    xyz = np.stack([d, np.linspace(-1, 1, len(d)).astype(F32), np.full(len(d), 0.75, F32)], axis=1) if len(d) else np.zeros((0, 3), F32)
    return (np.array([angle, 0.25, -0.5, 3.0], F32), xyz, bad)


def crafted_cases():
    """(name, coef, Tcw, slots, th, expected (match, vertical, parallel, dist)) for one frame plane each; expected written by hand"""
    D, T3 = DEFAULT_TH, TUM3_TH
    dTh, aTh, verTh, parTh = (F32(v) for v in D)
    below = lambda v: np.nextafter(F32(v), F32(0))
    above = lambda v: np.nextafter(F32(v), F32(2))
    c = exact_frame_plane().reshape(1, 4)
    far = [1.0, 2.0]
    cases = [
        ("tie match: first wins, the second falls through to parallel", [slot(1.0, [0.0625, 0.5]), slot(1.0, [0.5, 0.0625])], D, (0, -1, 1, 0.0625)),
        ("tie match below parTh: first wins", [slot(0.9, [0.0625, 0.5]), slot(0.9, [0.5, 0.0625])], D, (0, -1, -1, 0.0625)),
        ("closer later slot takes over", [slot(1.0, [0.0625]), slot(1.0, [0.5, 0.03125])], D, (1, -1, -1, 0.03125)),
        ("tie vertical: first wins", [slot(0.05, far), slot(0.05, far), slot(-0.05, far)], D, (-1, 0, -1, 100.0)),
        ("smaller |angle| later takes over vertical", [slot(0.05, far), slot(-0.03125, far)], D, (-1, 1, -1, 100.0)),
        ("tie parallel: first wins", [slot(0.999, far), slot(0.999, far), slot(-0.999, far)], D, (-1, -1, 0, 100.0)),
        ("larger |angle| later takes over parallel", [slot(0.998, far), slot(-0.9995, far)], D, (-1, -1, 1, 100.0)),
        ("fall-through: gated, not closer, becomes parallel", [slot(1.0, [0.03125]), slot(0.9990234375, [0.0625])], D, (0, -1, 1, 0.03125)),
        ("the same slot consumed once the closer one is bad", [slot(1.0, [0.03125], bad=True), slot(0.9990234375, [0.0625])], D, (1, -1, -1, 0.0625)),
        ("fall-through under aTh 0.985 < parTh", [slot(1.0, [0.03125]), slot(0.9970703125, [0.046875])], T3, (0, -1, 1, 0.03125)),
        ("gated under 0.86 but not 0.985: parallel needs parTh", [slot(0.9, [0.0]), slot(0.99, [0.0])], T3, (1, -1, -1, 0.0)),
        ("angle == aTh is not gated (strict)", [slot(aTh, [0.0])], D, (-1, -1, -1, 100.0)),
        ("angle just above aTh is gated", [slot(above(aTh), [0.0])], D, (0, -1, -1, 0.0)),
        ("angle == -aTh is not gated", [slot(-aTh, [0.0])], D, (-1, -1, -1, 100.0)),
        ("angle == verTh is not vertical (strict)", [slot(verTh, far)], D, (-1, -1, -1, 100.0)),
        ("angle just below verTh is vertical", [slot(below(verTh), far)], D, (-1, 0, -1, 100.0)),
        ("angle == parTh is not parallel (strict)", [slot(parTh, far)], D, (-1, -1, -1, 100.0)),
        ("angle just above parTh is parallel", [slot(above(parTh), far)], D, (-1, -1, 0, 100.0)),
        ("dis == dTh is no match (strict), falls to parallel", [slot(1.0, [dTh])], D, (-1, -1, 0, 100.0)),
        ("dis just below dTh matches", [slot(1.0, [below(dTh)])], D, (0, -1, -1, float(below(dTh)))),
        ("negative angles: match", [slot(-1.0, [-0.0625])], D, (0, -1, -1, 0.0625)),
        ("negative angles: vertical and parallel", [slot(-0.05, far), slot(-0.999, far)], D, (-1, 0, 1, 100.0)),
        ("a bad slot is skipped in every role", [slot(1.0, [0.0], bad=True), slot(0.01, far, bad=True), slot(1.0, [0.0625]), slot(0.05, far)], D, (2, 3, -1, 0.0625)),
        ("empty cloud: dis = 100, falls to parallel", [slot(1.0, [])], D, (-1, -1, 0, 100.0)),
        ("NaN points never win", [slot(1.0, [np.nan, 0.0625, np.nan])], D, (0, -1, -1, 0.0625)),
        ("all-NaN cloud: dis = 100", [slot(1.0, [np.nan, np.nan])], D, (-1, -1, 0, 100.0)),
        ("NaN angle takes no role", [slot(np.nan, [0.0]), slot(0.05, far)], D, (-1, 1, -1, 100.0)),
        ("vertical consumes the slot before parallel sees it", [slot(0.05, far), slot(0.04, far)], (0.1, 0.86, 0.08716, 0.03), (-1, 1, -1, 100.0)),
    ]
    return [(name, c, T_EXACT, slots, th, exp) for name, slots, th, exp in cases]
