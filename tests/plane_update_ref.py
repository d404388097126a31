"""The numpy restatement of MapPlane::UpdateCoefficientsAndPoints (reference src/MapPlane.cc:337-368 with a frame, :300-335 without) as
csrc/plane_update.hip computes it.  Five steps:
  1. transform_matrix   Converter::toSE3Quat(mTcw) -> Isometry3d -> inverse(), in double (the readings of pose_opt_ref)
  2. transform          pcl::transformPointCloud: (float)(M00 x + M01 y + M02 z + M03) per row, in double, left to right
  3.                    the slot's cloud appended
  4. voxel_grid         pcl::VoxelGrid(0.1) as oracle/planes_tail.c states it, the centroid the exact mean (2^-24 m fixed point)
  5.                    the SACSegmentation block writes only locals: not run
apply() runs a list of operations on a map kept as a list of [coef, cloud, bad]."""
import numpy as np

import plane_assoc_ref
import pose_opt_ref

F32 = np.float32
MERGE, INSERT = 0, 1
MAX_POINTS = 1 << 20
OK, UNSUPPORTED = 0, -4
INT32_MAX = 2 ** 31 - 1


def transform_matrix(Tcw):
    """(3, 4) float64: rows 0..2 of inverse(toSE3Quat(Tcw))"""
    T = np.asarray(Tcw, F32).reshape(3, 4).astype(np.float64)
    q = pose_opt_ref.quat_normalize(pose_opt_ref.quat_from_R(T[:, :3]))
    R = pose_opt_ref.quat_to_R(q)
    M = np.zeros((3, 4))
    for r in range(3):
        l0, l1, l2 = R[0, r], R[1, r], R[2, r]
        M[r, 0], M[r, 1], M[r, 2] = l0, l1, l2
        M[r, 3] = ((-l0) * T[0, 3] + (-l1) * T[1, 3]) + (-l2) * T[2, 3]
    return M


def insert_matrix(Twc):
    """Converter::toMatrix4d(GetPoseInverse()): the float entries widened"""
    return np.asarray(Twc, F32).reshape(3, 4).astype(np.float64)


def transform(M, xyz):
    p = np.asarray(xyz, F32).reshape(-1, 3).astype(np.float64)
    out = np.empty((len(p), 3), F32)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = (((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]).astype(F32)
    return out


def voxel_grid(xyz):
    """-> the filtered cloud (n, 3) float32 in ascending voxel index, or None when the operation is refused (index overflow)"""
    p = np.asarray(xyz, F32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        return np.zeros((0, 3), F32)
    inv = F32(1.0) / F32(0.1)
    with np.errstate(all="ignore"):
        lo = np.floor(p.min(axis=0) * inv); hi = np.floor(p.max(axis=0) * inv)       # float32
    if not (np.all(lo >= -2.0 ** 31) and np.all(lo < 2.0 ** 31) and np.all(hi >= -2.0 ** 31) and np.all(hi < 2.0 ** 31)):
        return None
    minb = [int(v) for v in lo]; div = [int(h) - m + 1 for h, m in zip(hi, minb)]
    if div[0] * div[1] * div[2] > INT32_MAX:
        return None
    ijk = (np.floor(p * inv) - np.array(minb).astype(F32)).astype(np.int64)          # float32 subtraction, then (int)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    fix = np.rint(p.astype(np.float64) * 16777216.0).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    idx, fix = idx[order], fix[order]
    head = np.flatnonzero(np.concatenate([[True], idx[1:] != idx[:-1]]))
    n = np.diff(np.concatenate([head, [len(idx)]]))
    sums = np.add.reduceat(fix, head, axis=0)                                          # exact: 64-bit integers
    return (sums.astype(np.float64) / (n.astype(np.float64) * 16777216.0)[:, None]).astype(F32)


def valid_planes(records):
    return [i for i in range(len(records)) if records["valid"][i]]


def plane_points(records, cloud, i):
    """frame plane i (the i-th valid record) -> its voxel cloud"""
    r = records[valid_planes(records)[i]]
    return np.asarray(cloud, F32).reshape(-1, 3)[r["first"]:r["first"] + r["n_points"]]


def apply(map_slots, records, cloud, Tcw, Twc, ops):
    """map_slots: list of [coef (4,) float32, cloud (n, 3) float32, bad]; changed in place.  ops: (plane, slot, op) in list order.
    -> dict(status, n_frame, n_before, n_after, n_done) as hvo_plane_update_result"""
    M = transform_matrix(Tcw)
    res = dict(status=[], n_frame=[], n_before=[], n_after=[], n_done=0)
    val = valid_planes(records)
    for plane, slot, op in ops:
        pts = plane_points(records, cloud, plane)
        there = slot < len(map_slots)
        before = map_slots[slot][1] if (op == MERGE and there) else np.zeros((0, 3), F32)
        res["n_frame"].append(len(pts)); res["n_before"].append(len(before))
        out = None
        if len(pts) + len(before) <= MAX_POINTS and (op == INSERT or there):
            out = voxel_grid(np.concatenate([transform(M if op == MERGE else insert_matrix(Twc), pts), before]))
        if out is None:
            res["status"].append(UNSUPPORTED); res["n_after"].append(len(before))
            continue
        res["status"].append(OK); res["n_after"].append(len(out)); res["n_done"] += 1
        if op == MERGE:
            map_slots[slot][1] = out
        else:
            coef = plane_assoc_ref.world_coeff(np.asarray(Tcw, F32).reshape(3, 4), records["coef"][val[plane]])
            while len(map_slots) < slot:
                map_slots.append([np.zeros(4, F32), np.zeros((0, 3), F32), True])  # skipped over: bad and empty
            if slot == len(map_slots):
                map_slots.append([coef, out, False])
            else:
                map_slots[slot][0] = coef; map_slots[slot][1] = out
    for k in ("status", "n_frame", "n_before", "n_after"):
        res[k] = np.array(res[k], np.int32)
    return res


# ---------------------------------------------------------------- inputs
def records_for(clouds, coefs=None, valid=None):
    """PLANE_CLOUD_DT-shaped records (coef, valid, first, n_points) and the packed cloud for a list of per-plane clouds"""
    dt = np.dtype([("coef", "<f4", 4), ("valid", "<i4"), ("gate_ok", "<i4"), ("first", "<i4"), ("n_points", "<i4"), ("n_pixels", "<i4"), ("n_inliers", "<i4")])
    rec = np.zeros(len(clouds), dt); first = 0
    for i, c in enumerate(clouds):
        c = np.asarray(c, F32).reshape(-1, 3)
        rec["first"][i] = first; rec["n_points"][i] = len(c); first += len(c)
        rec["valid"][i] = 1 if valid is None else valid[i]; rec["gate_ok"][i] = rec["valid"][i]
        rec["coef"][i] = (0, 0, 1, -1) if coefs is None else coefs[i]
    cloud = np.concatenate([np.asarray(c, F32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), F32)
    return rec, cloud


def transform_cases():
    """(name, Tcw (3, 4) float32): identity, each branch of Quaterniond(Matrix3d), w < 0, a float rotation orthonormal to 1e-7 only, t = 1e3"""
    rot, pose = plane_assoc_ref.rot, plane_assoc_ref.pose
    out = [("identity", pose(np.eye(3), (0, 0, 0))),
           ("trace > 0", pose(rot((0.3, -0.5, 0.8), 40), (0.5, -0.25, 1.5))),
           ("m00 largest", pose(rot((1, 0.05, -0.03), 175), (0.1, 0.2, 0.3))),
           ("m11 largest", pose(rot((0.04, 1, 0.06), 172), (-0.4, 0.9, 0.1))),
           ("m22 largest", pose(rot((-0.05, 0.03, 1), 178), (2.0, -1.0, 0.5))),
           ("translation 1e3", pose(rot((0.2, 0.9, -0.1), 65), (1000.0, -1000.0, 1000.0)))]
    # w < 0 before the flip: in the m00 branch w = (m21 - m12) * t, negative for a rotation about -x by almost 180 degrees
    out.append(("w < 0", pose(rot((-1, 0.02, 0.01), 176), (0.3, 0.1, -0.2))))
    R = rot((0.5, 0.4, -0.7), 33).astype(np.float64)
    R = (R * (1 + 1e-7) + 1e-7 * np.array([[0, 1, -1], [-1, 0, 1], [1, -1, 0]])).astype(F32)
    out.append(("orthonormal to 1e-7", np.concatenate([R, np.array([[0.7], [-0.2], [0.4]], F32)], axis=1)))
    return [(n, np.asarray(T, F32).reshape(3, 4)) for n, T in out]


def random_pose(rng, t=3.0):
    return np.asarray(plane_assoc_ref.pose(plane_assoc_ref.rot(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-t, t, 3)), F32).reshape(3, 4)


def wall(rng, n, extent=8.0):
    """n points of a wall in the world frame: about one per 0.1 m voxel and a little more, so that merges both add and fuse"""
    p = np.stack([rng.uniform(-extent, extent, n), rng.uniform(-extent / 2, extent / 2, n), 2.0 + 0.02 * rng.normal(size=n)], axis=1)
    return p.astype(F32)
