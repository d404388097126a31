"""CPU restatement of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:335-580) with LocalMapping::ComputeF12 (:1779-1796),
ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:668-836), ORBmatcher::CheckDistEpipolarLine (:143-160) and KeyFrame::UnprojectStereo
(src/KeyFrame.cc:785-801).  Test infrastructure only, and THE DEFINITION of the readings csrc/new_points.hip states at its head: Python
floats are IEEE doubles, f32() rounds to float (a double result of + - * / sqrt of two floats rounds to the same float as the float
operation: 53 >= 2 * 24 + 2), one step per step of the reference.

Two formulations that check each other:
  * create_new_map_points() runs the REAL SEQUENTIAL CHAIN: neighbour by neighbour, SearchForTriangulation over real per-node lists (the
    merge of two sorted FeatureVectors) under the occupancy as it stands, every match triangulated in ascending idx1, the occupancy byte set
    when a point is created.
  * pairs_under_initial_occupancy() evaluates every (neighbour, idx1) pair alone, as the device does; the device's owner / created lists
    (independent pairs + resolve) are compared with the chain's.

Readings: see csrc/new_points.hip.  In short: dot3f = ((a0 b0 + a1 b1) + a2 b2) in float; R p + t = sm_row; cv::norm / Mat::dot are double
sums; K.inv() is OpenCV's closed 3 x 3 form in double; the stereo parallax is (d d - h h) / (d d + h h) in double; cv::SVD::compute is a
one-sided Jacobi of exactly 12 sweeps in double on the float entries of A, the highest index among equal smallest norms, the vector rounded
to float once; Mat / scalar scales by the double reciprocal; an octave outside [0, n_levels) refuses the pair."""
import math

import numpy as np

import point_map_ref as pm

F32 = np.float32
KP_DT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
MAX_FEATURES, MAX_NEIGHBOURS = 4096, 64
TH_LOW = 50
SWEEPS = 12
CREATED, OCCUPIED, NO_MATCH, LOW_PARALLAX, W_ZERO, NO_DEPTH, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(12)
OUTCOMES = ("created", "occupied", "no match", "low parallax", "w == 0", "no depth", "behind 1", "behind 2", "reproj 1", "reproj 2", "zero dist", "scale")
GATE_SEARCHED, GATE_SKIP, GATE_BASELINE = 0, 1, 2
SIGMA2 = (pm.SF * pm.SF).astype(F32)                  # mvLevelSigma2 of the default 8-level pyramid (ORBextractor.cc:428-436)
SCALE_FACTOR = 1.2
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_ERR = dict(all="ignore")


def f32(x):
    return float(F32(x))


def ddiv(a, b):
    return float(np.float64(a) / np.float64(b))


def dot3f(a, b):
    s = f32(a[0] * b[0]); s = f32(s + f32(a[1] * b[1])); s = f32(s + f32(a[2] * b[2]))
    return s


def row(a, b, c):
    """sm_row"""
    return f32(dot3f(a, b) * 1.0 + c * 1.0)


def dotd(a, b):
    s = a[0] * b[0]; s = s + a[1] * b[1]; s = s + a[2] * b[2]
    return s


def normd(a):
    return math.sqrt(dotd(a, a))


def pose(Tcw):
    """(R as 3 rows, t, Ow) as Python floats holding float values"""
    R, t, Ow = pm.pose_parts(Tcw)
    return [[float(v) for v in r] for r in R], [float(v) for v in t], [float(v) for v in Ow]


def col(R, c):
    return [R[0][c], R[1][c], R[2][c]]


def inv3(m):
    """OpenCV's closed form on float entries: cofactors and determinant in double, each entry (float)(cofactor * (1 / det))"""
    (a00, a01, a02), (a10, a11, a12), (a20, a21, a22) = m
    d = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20)
    d = ddiv(1.0, d)
    return [[f32((a11 * a22 - a12 * a21) * d), f32((a02 * a21 - a01 * a22) * d), f32((a01 * a12 - a02 * a11) * d)],
            [f32((a12 * a20 - a10 * a22) * d), f32((a00 * a22 - a02 * a20) * d), f32((a02 * a10 - a00 * a12) * d)],
            [f32((a10 * a21 - a11 * a20) * d), f32((a01 * a20 - a00 * a21) * d), f32((a00 * a11 - a01 * a10) * d)]]


def mul3(A, B):
    return [[dot3f(A[r], col(B, c)) for c in range(3)] for r in range(3)]


def neighbour_constants(cam, cur_pose, kf):
    """Ow2, the gate (skip, then baseline < mb), ComputeF12 and the epipole"""
    with np.errstate(**_ERR):
        fx, fy, cx, cy = (f32(v) for v in cam[:4])
        R1, t1, Ow1 = cur_pose
        R2, t2, Ow2 = pose(kf["Tcw"])
        baseline = f32(normd([f32(Ow2[k] - Ow1[k]) for k in range(3)]))
        gate = GATE_SKIP if kf.get("skip") else (GATE_BASELINE if baseline < f32(kf["mb"]) else GATE_SEARCHED)
        R12 = [[dot3f(R1[r], R2[q]) for q in range(3)] for r in range(3)]
        t12 = [row([-v for v in R12[r]], t2, t1[r]) for r in range(3)]
        tx = [[0.0, -t12[2], t12[1]], [t12[2], 0.0, -t12[0]], [-t12[1], t12[0], 0.0]]
        Kt = [[fx, 0.0, 0.0], [0.0, fy, 0.0], [cx, cy, 1.0]]; K = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
        F = mul3(mul3(mul3(inv3(Kt), tx), R12), inv3(K))
        C = [row(R2[r], Ow1, t2[r]) for r in range(3)]
        invz = f32(ddiv(1.0, C[2]))
        ex = f32(f32(f32(fx * C[0]) * invz) + cx); ey = f32(f32(f32(fy * C[1]) * invz) + cy)
    return dict(R=R2, t=t2, Ow=Ow2, F=F, ex=ex, ey=ey, gate=gate, baseline=baseline, mb=f32(kf["mb"]))


def node_lists(node_id):
    """the FeatureVector: node -> feature indices in ascending order (negative: in no node)"""
    fv = {}
    for i, n in enumerate(np.asarray(node_id).tolist()):
        if n >= 0: fv.setdefault(n, []).append(i)
    return fv


def _side(kf):
    n = len(kf["kp_un"])
    st = kf.get("uright") is not None
    return dict(n=n, x=kf["kp_un"]["x"].astype(np.float64), y=kf["kp_un"]["y"].astype(np.float64), oct=kf["kp_un"]["octave"].astype(np.int64),
                kp=(kf["kp_un"] if kf.get("kp") is None else kf["kp"]),
                ur=(np.asarray(kf["uright"], np.float32).astype(np.float64) if st else np.full(n, -1.0)),
                depth=(np.asarray(kf["depth"], np.float32).astype(np.float64) if st else np.full(n, -1.0)),
                desc=np.asarray(kf["desc"], np.uint8).reshape(-1, 32), fv=node_lists(kf["node_id"]))


def epipolar_dsqr(F, x1, y1, x2, y2):
    """(den, dsqr) of CheckDistEpipolarLine, floats"""
    with np.errstate(**_ERR):
        a = f32(f32(f32(x1 * F[0][0]) + f32(y1 * F[1][0])) + F[2][0])
        b = f32(f32(f32(x1 * F[0][1]) + f32(y1 * F[1][1])) + F[2][1])
        c = f32(f32(f32(x1 * F[0][2]) + f32(y1 * F[1][2])) + F[2][2])
        num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
        den = f32(f32(a * a) + f32(b * b))
        if den == 0.0: return den, float("nan")
        return den, f32(ddiv(f32(num * num), den))


def search_for_triangulation(S1, S2, kc, has1, has2, th_low=TH_LOW, n_levels=pm.N_LEVELS, sf=pm.SF, sigma2=SIGMA2, ties=None):
    """ORBmatcher.cc:668-836 with mbCheckOrientation and bOnlyStereo false -> (vMatches12, its distances; 256 where none)"""
    n1 = S1["n"]
    m12 = np.full(n1, -1, np.int32); md = np.full(n1, 256, np.int32)
    F = kc["F"]
    fv1, fv2 = S1["fv"], S2["fv"]
    for node in sorted(set(fv1) & set(fv2)):                       # the merge of the two sorted maps meets exactly the common nodes, ascending
        l2 = fv2[node]; d2 = S2["desc"][l2]
        for i1 in fv1[node]:
            if has1[i1]: continue
            o1 = int(S1["oct"][i1])
            if o1 < 0 or o1 >= n_levels: continue
            st1 = S1["ur"][i1] >= 0
            x1, y1 = S1["x"][i1], S1["y"][i1]
            dists = _POP[d2 ^ S1["desc"][i1]].sum(axis=1)
            best, bidx, nt = th_low, -1, 0
            for p, i2 in enumerate(l2):
                if has2[i2]: continue                               # vbMatched2 is never set
                dist = int(dists[p])
                if dist > th_low or dist > best: continue
                o2 = int(S2["oct"][i2])
                if o2 < 0 or o2 >= n_levels: continue
                x2, y2 = S2["x"][i2], S2["y"][i2]
                if not st1 and not S2["ur"][i2] >= 0:
                    dx = f32(kc["ex"] - x2); dy = f32(kc["ey"] - y2)
                    if f32(f32(dx * dx) + f32(dy * dy)) < f32(100.0 * float(sf[o2])): continue
                den, dsqr = epipolar_dsqr(F, x1, y1, x2, y2)
                if den == 0.0: continue
                if dsqr < 3.84 * float(sigma2[o2]):
                    nt = nt + 1 if dist == best and bidx >= 0 else 1
                    bidx, best = i2, dist
            if bidx >= 0:
                m12[i1] = bidx; md[i1] = best
                if ties is not None and nt > 1: ties.append(i1)
    return m12, md


def _rot(num, den2):
    if den2 * 0.5 == 0.0: return 1.0, 0.0
    th = ddiv(num, den2)
    at = -th if th < 0.0 else th
    tt = ddiv(1.0, at + math.sqrt(th * th + 1.0))
    if th < 0.0: tt = -tt
    cc = ddiv(1.0, math.sqrt(tt * tt + 1.0))
    return cc, tt * cc


def svd4_last(A):
    """the right singular vector of the smallest singular value of the 4 x 4 float A (rows of Python floats holding floats)"""
    W = [list(r) for r in A]; V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    with np.errstate(**_ERR):
        for _ in range(SWEEPS):
            for p in range(3):
                for q in range(p + 1, 4):
                    al = be = ga = 0.0
                    for r in range(4):
                        wp, wq = W[r][p], W[r][q]
                        al = al + wp * wp; be = be + wq * wq; ga = ga + wp * wq
                    c, s = _rot(be - al, 2.0 * ga)
                    for M in (W, V):                                 # the working columns and V stay in double
                        for r in range(4):
                            mp, mq = M[r][p], M[r][q]
                            M[r][p] = c * mp - s * mq; M[r][q] = s * mp + c * mq
        best, x = 0.0, None
        for c in range(4):
            s2 = 0.0
            for r in range(4): s2 = s2 + W[r][c] * W[r][c]
            if c == 0 or s2 <= best: best, x = s2, [f32(V[r][c]) for r in range(4)]      # vt is CV_32F: rounded once
    return x


def stereo_cos(mb, depth):
    h = f32(mb / 2.0); d = float(depth)
    dd = d * d; hh = h * h
    return f32(ddiv(dd - hh, dd + hh))


def triangulation_rows(xn1, yn1, P1, xn2, yn2, P2):
    """A (4 x 4): each element one float product then one float subtraction"""
    T1 = [P1[0][r] + [P1[1][r]] for r in range(3)]; T2 = [P2[0][r] + [P2[1][r]] for r in range(3)]
    return [[f32(f32(xn1 * T1[2][c]) - T1[0][c]) for c in range(4)], [f32(f32(yn1 * T1[2][c]) - T1[1][c]) for c in range(4)],
            [f32(f32(xn2 * T2[2][c]) - T2[0][c]) for c in range(4)], [f32(f32(yn2 * T2[2][c]) - T2[1][c]) for c in range(4)]]


def _reproj_fails(R, t, X, z, cam, bf, kx, ky, kur, stereo, sig):
    fx, fy, cx, cy = cam
    x = f32(dotd(R[0], X) + t[0]); y = f32(dotd(R[1], X) + t[1])
    invz = f32(ddiv(1.0, z))
    u = f32(f32(f32(fx * x) * invz) + cx); v = f32(f32(f32(fy * y) * invz) + cy)
    ex = f32(u - kx); ey = f32(v - ky)
    if not stereo:
        e2 = f32(f32(ex * ex) + f32(ey * ey))
        return e2 > 5.991 * sig, e2
    ur = f32(u - f32(bf * invz)); er = f32(ur - kur)
    e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
    return e2 > 7.8 * sig, e2


def triangulate(S1, S2, P1, mb1, kc, i1, i2, cam, bf, scale_factor=SCALE_FACTOR, sf=pm.SF, sigma2=SIGMA2, trace=None):
    """LocalMapping.cc:416-559 for one match -> (outcome, branch, x3D as three floats)"""
    with np.errstate(**_ERR):
        fx, fy, cx, cy = cam4 = tuple(f32(v) for v in cam[:4])
        bf = f32(bf)
        invfx = f32(ddiv(1.0, fx)); invfy = f32(ddiv(1.0, fy))
        R1, t1, Ow1 = P1
        R2, t2, Ow2 = kc["R"], kc["t"], kc["Ow"]
        x1, y1, x2, y2 = S1["x"][i1], S1["y"][i1], S2["x"][i2], S2["y"][i2]
        ur1, ur2 = S1["ur"][i1], S2["ur"][i2]
        st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
        xn1 = f32(f32(x1 - cx) * invfx); yn1 = f32(f32(y1 - cy) * invfy); xn2 = f32(f32(x2 - cx) * invfx); yn2 = f32(f32(y2 - cy) * invfy)
        ray1 = [dot3f(col(R1, k), [xn1, yn1, 1.0]) for k in range(3)]; ray2 = [dot3f(col(R2, k), [xn2, yn2, 1.0]) for k in range(3)]
        cosr = f32(ddiv(dotd(ray1, ray2), normd(ray1) * normd(ray2)))
        cs = f32(cosr + 1.0)
        s1 = s2 = cs
        if st1: s1 = stereo_cos(mb1, S1["depth"][i1])
        elif st2: s2 = stereo_cos(kc["mb"], S2["depth"][i2])
        cst = s2 if s2 < s1 else s1
        zero = (0.0, 0.0, 0.0)
        if trace is not None: trace.update(cosr=cosr, s1=s1, s2=s2)
        if cosr < cst and cosr > 0.0 and (st1 or st2 or cosr < 0.9998):
            br = 1
            x = svd4_last(triangulation_rows(xn1, yn1, (R1, t1), xn2, yn2, (R2, t2)))
            if x[3] == 0.0: return W_ZERO, br, zero
            iw = ddiv(1.0, x[3])
            X = [f32(x[k] * iw) for k in range(3)]
        elif (st1 and s1 < s2) or (st2 and s2 < s1):
            first = st1 and s1 < s2
            br = 2 if first else 3
            S, i, R, Ow = (S1, i1, R1, Ow1) if first else (S2, i2, R2, Ow2)
            z = float(S["depth"][i])
            if not z > 0.0: return NO_DEPTH, br, zero
            u, v = float(S["kp"]["x"][i]), float(S["kp"]["y"][i])
            xc = f32(f32(f32(u - cx) * z) * invfx); yc = f32(f32(f32(v - cy) * z) * invfy)
            X = [row(col(R, k), [xc, yc, z], Ow[k]) for k in range(3)]
        else:
            return LOW_PARALLAX, 0, zero
        X3 = tuple(X)
        z1 = f32(dotd(R1[2], X) + t1[2])
        if z1 <= 0.0: return BEHIND_1, br, X3
        z2 = f32(dotd(R2[2], X) + t2[2])
        if z2 <= 0.0: return BEHIND_2, br, X3
        o1, o2 = int(S1["oct"][i1]), int(S2["oct"][i2])
        bad, e1 = _reproj_fails(R1, t1, X, z1, cam4, bf, x1, y1, ur1, st1, float(sigma2[o1]))
        if trace is not None: trace.update(e1=e1)
        if bad: return REPROJ_1, br, X3
        bad, e2 = _reproj_fails(R2, t2, X, z2, cam4, bf, x2, y2, ur2, st2, float(sigma2[o2]))
        if trace is not None: trace.update(e2=e2)
        if bad: return REPROJ_2, br, X3
        d1 = f32(normd([f32(X[k] - Ow1[k]) for k in range(3)])); d2 = f32(normd([f32(X[k] - Ow2[k]) for k in range(3)]))
        if d1 == 0.0 or d2 == 0.0: return ZERO_DIST, br, X3
        rd = f32(ddiv(d2, d1)); ro = f32(ddiv(float(sf[o1]), float(sf[o2]))); rf = f32(1.5 * f32(scale_factor))
        if f32(rd * rf) < ro or rd > f32(ro * rf): return SCALE, br, X3
        return CREATED, br, X3


def pairs_under_initial_occupancy(cur, kfs, cam, bf, th_low=TH_LOW, n_levels=pm.N_LEVELS, scale_factor=SCALE_FACTOR):
    """every neighbour alone under the initial occupancy: list of dict(match_idx2, match_dist, outcome, branch, x3d, gate, ties)"""
    S1 = _side(cur); P1 = pose(cur["Tcw"]); n1 = S1["n"]
    has1 = np.asarray(cur["has_map_point"]).astype(bool)
    out = []
    for kf in kfs:
        kc = neighbour_constants(cam, P1, kf)
        m12 = np.full(n1, -1, np.int32); md = np.full(n1, 256, np.int32)
        outcome = np.where(has1, OCCUPIED, NO_MATCH).astype(np.int8); branch = np.zeros(n1, np.int8); x3d = np.zeros((n1, 3), np.float32); ties = []
        if kc["gate"] == GATE_SEARCHED and n1 and len(kf["kp_un"]):
            S2 = _side(kf)
            m12, md = search_for_triangulation(S1, S2, kc, has1, np.asarray(kf["has_map_point"]).astype(bool), th_low, n_levels, ties=ties)
            for i1 in np.flatnonzero(m12 >= 0):
                outcome[i1], branch[i1], x3d[i1] = triangulate(S1, S2, P1, f32(cur["mb"]), kc, i1, int(m12[i1]), cam, bf, scale_factor)
        out.append(dict(match_idx2=m12, match_dist=md, outcome=outcome, branch=branch, x3d=x3d, gate=kc["gate"], ties=ties))
    return out


def create_new_map_points(cur, kfs, cam, bf, th_low=TH_LOW, n_levels=pm.N_LEVELS, scale_factor=SCALE_FACTOR):
    """the sequential chain -> (per neighbour dict(created_idx1, created_idx2, n_created, gate), owner, n_new)"""
    S1 = _side(cur); P1 = pose(cur["Tcw"]); n1 = S1["n"]
    has1 = np.asarray(cur["has_map_point"]).astype(bool).copy()
    owner = np.full(n1, -1, np.int32); out = []
    for j, kf in enumerate(kfs):
        kc = neighbour_constants(cam, P1, kf)
        c1, c2 = [], []
        if kc["gate"] == GATE_SEARCHED and n1 and len(kf["kp_un"]):
            S2 = _side(kf)
            m12, _ = search_for_triangulation(S1, S2, kc, has1, np.asarray(kf["has_map_point"]).astype(bool), th_low, n_levels)
            for i1 in np.flatnonzero(m12 >= 0):                      # vMatchedPairs: ascending idx1
                o, _, _ = triangulate(S1, S2, P1, f32(cur["mb"]), kc, i1, int(m12[i1]), cam, bf, scale_factor)
                if o == CREATED:
                    has1[i1] = True                                  # mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
                    owner[i1] = j; c1.append(int(i1)); c2.append(int(m12[i1]))
        out.append(dict(created_idx1=np.array(c1, np.int32), created_idx2=np.array(c2, np.int32), n_created=len(c1), gate=kc["gate"]))
    return out, owner, int((owner >= 0).sum())


def full(cur, kfs, cam, bf, **kw):
    """what the library returns: per neighbour the pair results merged with the chain's lists, and the summary"""
    pairs = pairs_under_initial_occupancy(cur, kfs, cam, bf, **kw)
    chain, owner, n_new = create_new_map_points(cur, kfs, cam, bf, **kw)
    return [dict(p, **c, status=0) for p, c in zip(pairs, chain)], dict(owner=owner, n_new=n_new)


# ---- scenes ----
BASE = np.arange(32, dtype=np.uint8) * 7 + 3
SCENE_SEED = 23                                        # the random scene's seed: change it, never a condition of vacuity()
CAM = pm.CAM                                           # TUM3: fx, fy, cx, cy, bf = 40
MB = float(F32(F32(CAM[4]) / F32(CAM[0])))


def flip(k, base=BASE, start=0):
    """base with k bits flipped from bit `start`: Hamming distance k"""
    bits = np.unpackbits(base); bits[start:start + k] ^= 1
    return np.packbits(bits)


def Tcw_of(R, C):
    """the pose of a camera with world-to-camera rotation R at centre C"""
    R = np.asarray(R, np.float64); t = -R @ np.asarray(C, np.float64)
    return np.concatenate([R, t[:, None]], axis=1).astype(np.float32)


def yaw(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


IDENTITY = Tcw_of(np.eye(3), (0, 0, 0))
SCENE_POSES = ((np.eye(3), (0, 0, 0.25)), (yaw(0.05), (0.1, 0, 0)), (np.eye(3), (0.05, 0, 0)), (np.eye(3), (0.3, 0, 0)))


def observe(rng, Pw, Tcw, cam=CAM, noise=0.5, depth_noise=0.01, no_depth=0.15, octave=None):
    """a key frame's features of the world points Pw: pixel noise, depth noise, a share without depth"""
    n = len(Pw); T = np.asarray(Tcw, np.float64)
    Pc = Pw @ T[:, :3].T + T[:, 3]
    kp = np.zeros(n, KP_DT); kp["size"] = 31; kp["class_id"] = -1
    kp["x"] = cam[0] * Pc[:, 0] / Pc[:, 2] + cam[2] + rng.normal(0, noise, n); kp["y"] = cam[1] * Pc[:, 1] / Pc[:, 2] + cam[3] + rng.normal(0, noise, n)
    kp["octave"] = rng.choice(8, n, p=[0.26, 0.2, 0.16, 0.12, 0.1, 0.07, 0.05, 0.04]) if octave is None else octave
    depth = (Pc[:, 2] * (1 + rng.normal(0, depth_noise, n))).astype(np.float32)
    ur = (kp["x"] - F32(cam[4]) / depth).astype(np.float32)
    mono = rng.rand(n) < no_depth
    depth[mono] = -1; ur[mono] = -1
    return kp, ur, depth


def random_scene(n=1000, seed=SCENE_SEED, poses=SCENE_POSES, per_node=8, other_node=0.05, twins=20, occupied=0.25, skip=()):
    """the current key frame at the identity with n features of world points uniform in [-3, 3] x [-2, 2] x [0.5, 8] m and one neighbour per
    pose that sees the same points in another feature order.  Descriptor pairs lie 0 .. 6 bits apart; a pair shares its node (per_node points
    per node) except for the share other_node; `twins` neighbour features get a copy (same descriptor, 0.3 px aside) at a higher index: a tie
    on the distance; a quarter of the current features and a tenth of a neighbour's hold a map point"""
    rng = np.random.RandomState(seed)
    Pw = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 8, n)], axis=1)
    kp, ur, depth = observe(rng, Pw, IDENTITY)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    node = (np.arange(n) // per_node).astype(np.int32) * 3 + 5
    cur = dict(kp_un=kp, kp=None, uright=ur, depth=depth, desc=desc, node_id=node, has_map_point=(rng.rand(n) < occupied).astype(np.uint8), Tcw=IDENTITY, mb=MB)
    kfs = []
    for j, (R, C) in enumerate(poses):
        T = Tcw_of(R, C)
        perm = rng.permutation(n)
        kp2, ur2, dp2 = observe(rng, Pw[perm], T, octave=kp["octave"][perm])
        d2 = desc[perm].copy()
        for i in range(n):
            for b in rng.choice(256, rng.randint(0, 7), replace=False): d2[i, b >> 3] ^= 1 << (b & 7)
        nd2 = node[perm].copy()
        moved = rng.rand(n) < other_node
        nd2[moved] += 1                                              # a node the current key frame does not use
        has2 = (rng.rand(n) < 0.1).astype(np.uint8)
        if twins and n:
            tw = rng.choice(n, min(twins, n), replace=False)
            k2 = kp2[tw].copy(); k2["x"] += F32(0.3)
            kp2 = np.concatenate([kp2, k2]); ur2 = np.concatenate([ur2, np.where(ur2[tw] >= 0, ur2[tw] + F32(0.3), ur2[tw]).astype(np.float32)]); dp2 = np.concatenate([dp2, dp2[tw]])
            d2 = np.concatenate([d2, d2[tw]]); nd2 = np.concatenate([nd2, nd2[tw]]); has2 = np.concatenate([has2, has2[tw]])
        kfs.append(dict(kp_un=kp2, kp=None, uright=ur2, depth=dp2, desc=d2, node_id=nd2.astype(np.int32), has_map_point=has2, Tcw=T, mb=MB, skip=1 if j in skip else 0))
    return cur, kfs


RAGGED = (65, 0, 300, 1, 17)                            # the feature counts the five neighbours of ragged_scene are cut to
RAGGED_CREATED, FULL_SIZE_CREATED = (39, 0, 156, 0, 0), 2563      # what the restatement creates on ragged_scene and on full_size_scene


def cut(side, n):
    """the first n features of a key frame"""
    return dict(side, **{k: (None if side.get(k) is None else side[k][:n]) for k in ("kp_un", "kp", "uright", "depth", "desc", "node_id", "has_map_point")})


def ragged_scene():
    """one call whose neighbours differ in everything the staging pads or leaves out: 65, 0, 300, 1 and 17 features (the stride is the
    largest count), an empty neighbour inside the list, neighbour 2 monocular, neighbour 0 alone with raw key points (a quarter pixel off its
    undistorted ones, so that the unprojection of its stereo branch reads them)"""
    poses = (SCENE_POSES[0], SCENE_POSES[1], SCENE_POSES[3], (np.eye(3), (-0.2, 0.1, 0)), (yaw(0.01), (0.15, 0, 0.05)))
    cur, kfs = random_scene(n=300, seed=11, poses=poses, twins=5)
    kfs = [cut(k, n) for k, n in zip(kfs, RAGGED)]
    kfs[2] = dict(kfs[2], uright=None, depth=None)
    raw = kfs[0]["kp_un"].copy(); raw["x"] += F32(0.25)
    kfs[0] = dict(kfs[0], kp=raw)
    return cur, kfs


def full_size_scene():
    """4096 features on both sides in 64 nodes of 64: the CSR sort fills its 32 KB of keys and the search key's 16-bit position is largest"""
    return random_scene(n=MAX_FEATURES, seed=12, poses=SCENE_POSES[:1], per_node=64, twins=0)


def neighbours_of_frame(kp_un, uright, depth, desc, node_id, poses, cam, seed, mb):
    """neighbours that see a real frame's features: each feature is unprojected at its depth (a feature without depth at a drawn one) from
    the identity pose and observed from every pose of `poses`, in reversed feature order, with up to six descriptor bits flipped"""
    rng = np.random.RandomState(seed)
    n = len(kp_un)
    z = np.where(np.asarray(depth) > 0, np.asarray(depth, np.float64), rng.uniform(1.0, 4.0, n))
    Pw = np.stack([(kp_un["x"] - cam[2]) * z / cam[0], (kp_un["y"] - cam[3]) * z / cam[1], z], axis=1)
    kfs = []
    for R, C in poses:
        T = Tcw_of(R, C)
        perm = np.arange(n)[::-1]
        kp2, ur2, dp2 = observe(rng, Pw[perm], T, cam=cam, noise=0.3, octave=kp_un["octave"][perm])
        d2 = np.asarray(desc)[perm].copy()
        for i in range(n):
            for b in rng.choice(256, rng.randint(0, 7), replace=False): d2[i, b >> 3] ^= 1 << (b & 7)
        kfs.append(dict(kp_un=kp2, kp=None, uright=ur2, depth=dp2, desc=d2, node_id=np.asarray(node_id, np.int32)[perm].copy(),
                        has_map_point=(rng.rand(n) < 0.1).astype(np.uint8), Tcw=T, mb=mb, skip=0))
    return kfs


def vacuity(res, summ, n):
    """the random scene says something: asserted on the restatement's own output before the device is compared with it"""
    br = np.concatenate([r["branch"][r["outcome"] == CREATED] for r in res])
    assert all((br == b).sum() >= 20 for b in (1, 2, 3)), np.bincount(br, minlength=4)
    oc = np.concatenate([r["outcome"] for r in res])
    assert (oc == LOW_PARALLAX).any() and (oc == NO_MATCH).any() and (oc == OCCUPIED).any() and ((oc == REPROJ_1) | (oc == REPROJ_2)).any(), np.bincount(oc, minlength=12)
    ncreated = sum((r["outcome"] == CREATED).astype(int) for r in res)
    assert ((summ["owner"] >= 0) & (ncreated >= 2)).sum() >= 100
    assert sum(len(r["ties"]) for r in res) >= 1
    assert any(r["gate"] != GATE_SEARCHED for r in res)


# ---- crafted pairs: CAM2 = (512, 512, 320, 240, 64), the current key frame at the identity, the neighbour 0.25 m to the right.  Every step of
# ComputeF12 is exact there: F12 = [[0, 0, 0], [0, 0, -1/2048], [0, 1/2048, 0]], the line of (x1, y1) is y2 = y1 and dsqr = (y2 - y1)^2 ----
CAM2 = pm.CAM2
MB2 = 0.125                                            # bf / fx
T_RIGHT = Tcw_of(np.eye(3), (0.25, 0, 0))


def feats(rows):
    """rows of (x, y, octave, uright, depth, node, descriptor, has_map_point) -> the arrays of one side"""
    n = len(rows)
    kp = np.zeros(n, KP_DT); kp["size"] = 31; kp["class_id"] = -1
    kp["x"] = [r[0] for r in rows]; kp["y"] = [r[1] for r in rows]; kp["octave"] = [r[2] for r in rows]
    return dict(kp_un=kp, kp=None, uright=np.array([r[3] for r in rows], np.float32), depth=np.array([r[4] for r in rows], np.float32),
                desc=np.array([r[6] for r in rows], np.uint8).reshape(n, 32), node_id=np.array([r[5] for r in rows], np.int32),
                has_map_point=np.array([r[7] for r in rows], np.uint8))


def side(rows, Tcw=IDENTITY, mb=MB2, skip=0, mono=False):
    s = feats(rows); s.update(Tcw=np.asarray(Tcw, np.float32), mb=mb, skip=skip)
    if mono: s["uright"] = s["depth"] = None
    return s


def pt(X, Y, Z, octave=0, node=1, desc=BASE, has=0, stereo=True, Tcw=IDENTITY, cam=CAM2, dx=0.0, dy=0.0, depth=None):
    """the feature row of the world point (X, Y, Z) seen from Tcw, exact where the numbers allow"""
    T = np.asarray(Tcw, np.float64); Pc = T[:, :3] @ np.array([X, Y, Z], np.float64) + T[:, 3]
    x = cam[0] * Pc[0] / Pc[2] + cam[2] + dx; y = cam[1] * Pc[1] / Pc[2] + cam[3] + dy
    z = Pc[2] if depth is None else depth
    return (x, y, octave, (x - cam[4] / z) if stereo else -1.0, z if stereo else -1.0, node, desc, has)


def search_cases():
    """(name, current rows, neighbour rows, expected match_idx2, expected match_dist): mono features at depth 2 m on y = 240 + 16 k lines"""
    P = lambda k, **kw: pt(0.1 * k, 0.0625 * k, 2.0, stereo=False, **kw)
    N = lambda k, **kw: pt(0.1 * k, 0.0625 * k, 2.0, stereo=False, Tcw=T_RIGHT, **kw)
    c = []
    c.append(("equal distances: the last in index order wins", [P(1)], [N(1, desc=flip(7)), N(1, desc=flip(7, start=40)), N(1, desc=flip(9))], [1], [7]))
    c.append(("a closer candidate fails the epipolar gate, the farther one after it is taken", [P(1)], [N(1, desc=flip(3), dy=2.0), N(1, desc=flip(9))], [1], [9]))
    c.append(("a farther passing candidate after a closer passing one is refused", [P(1)], [N(1, desc=flip(3)), N(1, desc=flip(9))], [0], [3]))
    c.append(("a closer passing candidate after a farther one replaces it", [P(1)], [N(1, desc=flip(9)), N(1, desc=flip(3))], [1], [3]))
    c.append(("dist 50 and 51", [P(1), P(2, node=2)], [N(1, desc=flip(50)), N(2, node=2, desc=flip(51))], [0, -1], [50, 256]))
    c.append(("dy = 1 passes 3.84, dy = 2 does not", [P(1), P(2, node=2)], [N(1, dy=1.0), N(2, node=2, dy=2.0)], [0, -1], [0, 256]))
    c.append(("two idx1 take the same idx2", [P(1), P(1, dx=0.5)], [N(1, desc=flip(2))], [0, 0], [2, 2]))
    c.append(("node_id == -1; a node on one side only", [P(1, node=-1), P(2, node=4), P(3, node=6)], [N(1, node=-1), N(2, node=5), N(3, node=6)], [-1, -1, 2], [256, 256, 0]))
    c.append(("an occupied idx1 is not searched, an occupied idx2 is no candidate", [P(1, has=1), P(2, node=2)], [N(1), N(2, node=2, has=1), N(2, node=2, desc=flip(5))], [-1, 2], [256, 5]))
    c.append(("an octave outside the pyramid refuses the pair", [P(1, octave=-1), P(2, node=2), P(3, node=3, octave=8)],
              [N(1), N(2, node=2, octave=-1), N(2, node=2, desc=flip(4), octave=1), N(3, node=3)], [-1, 2, -1], [256, 4, 256]))
    return c


def epipole_case():
    """both features monocular: the neighbour 0.25 m AHEAD has its epipole at (320, 240); candidates sqrt(100 * 1.0) = 10 px from it are excluded
    (<), at exactly 10 px taken.  Features on the line x = 320: the epipolar line of (320, y1) is x2 = 320"""
    T = Tcw_of(np.eye(3), (0, 0, 0.25))
    row_ = lambda y, node, **kw: (320.0, y, 0, -1.0, -1.0, node, kw.get("desc", BASE), 0)
    st = lambda y, node: (320.0, y, 0, 300.0, 2.0, node, BASE, 0)
    cur = [row_(246.0, 1), row_(247.0, 2), row_(246.0, 3)]
    nb = [row_(249.75, 1), row_(250.0, 2), st(249.75, 3)]             # 9.75 px: excluded; 10 px: not excluded; stereo: the test does not run
    return cur, nb, T, [-1, 1, 2]


def node_size_case(sizes=(1, 15, 16, 17, 65, 200)):
    """one node per size: the current feature's partner is the LAST but one of the node's candidates, the last one lies a bit farther"""
    cur, nb, want = [], [], []
    for k, s in enumerate(sizes):
        node = 10 + k
        cur.append(pt(0.05 * k, 0.0625 * k, 2.0, stereo=False, node=node))
        for q in range(s):
            d = flip(3) if q == max(0, s - 2) else flip(20 + q % 20, start=64)
            nb.append(pt(0.05 * k, 0.0625 * k, 2.0, stereo=False, Tcw=T_RIGHT, node=node, desc=d))
        want.append(len(nb) - s + max(0, s - 2))
    return cur, nb, want


def bound_case():
    """the epipolar bound: candidates whose dsqr lies as close to 3.84 as a float y2 allows, on either side (y1 = 2, so y2 moves in steps of
    2.4e-7 and dsqr in steps of about 9e-7).  -> rows and the two dsqr values"""
    y1 = 2.0
    lo = F32(y1 + math.sqrt(3.84))
    while float(lo - F32(y1)) ** 2 >= 3.84: lo = np.nextafter(lo, F32(0))
    while float(np.nextafter(lo, F32(9)) - F32(y1)) ** 2 < 3.84: lo = np.nextafter(lo, F32(9))
    hi = np.nextafter(lo, F32(9))
    mk = lambda y, node: (300.0, float(y), 0, -1.0, -1.0, node, BASE, 0)
    return [mk(y1, 1), mk(y1, 2)], [mk(lo, 1), mk(hi, 2)], [0, -1]


def triangulation_cases():
    """(name, current row, neighbour row, neighbour Tcw, mb1, mb2, expected outcome, expected branch).  mb = 1 gives a stereo feature the
    smaller parallax cosine, so its UnprojectStereo is taken instead of the linear triangulation"""
    L = T_RIGHT
    c = []
    both = lambda X, Y, Z, T=L, **kw: (pt(X, Y, Z, **kw.get("a", {})), pt(X, Y, Z, Tcw=T, **kw.get("b", {})))
    add = lambda name, a, b, o, br, T=L, mb1=MB2, mb2=MB2: c.append((name, a, b, T, mb1, mb2, o, br))
    a, b = both(0.25, 0.125, 2.0); add("linear triangulation of two stereo features", a, b, CREATED, 1)
    a, b = both(0.25, 0.125, 2.0, a=dict(stereo=False), b=dict(stereo=False)); add("linear triangulation of two mono features", a, b, CREATED, 1)
    a, b = both(0.25, 0.125, 16.0); add("far point: UnprojectStereo of the current key frame", a, b, CREATED, 2, mb1=1.0)
    A = Tcw_of(np.eye(3), (0, 0, 1.0))                            # 1 m ahead: the baseline is not below mb2 = 1, and the rays of a point near the axis are almost parallel
    a, b = both(0.25, 0.125, 16.0, T=A, a=dict(stereo=False)); add("far point, current mono: UnprojectStereo of the neighbour", a, b, CREATED, 3, T=A, mb2=1.0)
    a, b = both(0.25, 0.125, 16.0, T=A); add("both stereo, the neighbour's cosine would be the smaller one: bStereo1 decides first and the current key frame is unprojected", a, b, CREATED, 2, T=A, mb2=1.0)
    a, b = both(0.25, 0.125, 400.0, a=dict(stereo=False), b=dict(stereo=False)); add("no stereo and very low parallax", a, b, LOW_PARALLAX, 0)
    a, b = both(0.25, 0.125, 16.0); a = a[:3] + (100.0, 0.0) + a[5:]; add("UnprojectStereo with z = 0", a, b, NO_DEPTH, 2, mb1=1.0)
    a, b = both(0.25, 0.125, 16.0, T=A, a=dict(stereo=False)); b = b[:3] + (100.0, -1.0) + b[5:]; add("UnprojectStereo of the neighbour with z < 0", a, b, NO_DEPTH, 3, T=A, mb2=1.0)
    a, b = both(0.25, 0.125, 2.0, a=dict(stereo=False), b=dict(stereo=False)); b = (a[0] + 64.0,) + b[1:]; add("rays that meet behind the cameras", a, b, BEHIND_1, 1)
    a = pt(0.25, 0.125, 2.0); add("in front of the current key frame, behind the neighbour 4 m ahead", a, (256.0, 208.0, 0, -1.0, -1.0, 1, BASE, 0), BEHIND_2, 2,
                                  T=Tcw_of(np.eye(3), (0, 0, 4.0)), mb1=1.0)
    a, b = both(0.25, 0.125, 16.0); a = a[:3] + (a[3] + 3.0,) + a[4:]; add("the current key frame's u_r is 3 px off: 9 > 7.8", a, b, REPROJ_1, 2, mb1=1.0)
    a, b = both(0.25, 0.125, 16.0); b = (b[0] + 3.0,) + b[1:]; add("the neighbour's x is 3 px off: 9 > 7.8", a, b, REPROJ_2, 2, mb1=1.0)
    a, b = both(0.25, 0.125, 16.0, b=dict(stereo=False)); b = (b[0] + 2.5,) + b[1:]; add("the mono neighbour's x is 2.5 px off: 6.25 > 5.991", a, b, REPROJ_2, 2, mb1=1.0)
    a, b = both(0.25, 0.125, 16.0, a=dict(octave=4), b=dict(octave=0)); add("octaves 4 and 0 at equal distance: ratioDist > ratioOctave * ratioFactor is false, the other side fires", a, b, SCALE, 2, mb1=1.0)
    a, b = both(0.25, 0.125, 16.0, a=dict(octave=0), b=dict(octave=4)); add("octaves 0 and 4 at equal distance", a, b, SCALE, 2, mb1=1.0)
    a, b = both(0.25, 0.125, 16.0, a=dict(octave=3), b=dict(octave=0)); add("octaves 3 and 0: 1.728 < 1.8 passes", a, b, CREATED, 2, mb1=1.0)
    return c


CAM4 = (512.0, 512.0, 0.0, 0.0, 64.0)                 # cx = cy = 0: a point on the optical axis projects to (0, 0), so a coordinate IS its error
T_LEFT = Tcw_of(np.eye(3), (-1.0, 0, 0))             # 1 m to the left: the baseline is not below mb2 = 1


def reproj_bound_cases():
    """the chi-square gates on the bound and one float step beyond, where every other number is exact (CAM4, depth 2 m, v = 0 everywhere so
    the epipolar distance is 0).  The point comes from UnprojectStereo of a stereo side with mb = 1.  A mono side under test sees it at u = 0
    and its feature's x is the error; a stereo side under test sees it at u = 32, u_r = 0, and its feature's mvuRight is the error.  The side
    under test has octave 1 (sigma2 = 1.44 in float).  -> as triangulation_cases()"""
    c = []
    s2 = float(SIGMA2[1])

    def step(limit):
        """the largest float e with (float)(e * e) <= limit, and the next float"""
        e = F32(math.sqrt(limit))
        while float(F32(e * e)) > limit: e = np.nextafter(e, F32(0))
        while float(F32(np.nextafter(e, F32(9)) * np.nextafter(e, F32(9)))) <= limit: e = np.nextafter(e, F32(9))
        return float(e), float(np.nextafter(e, F32(9)))

    f = lambda x, ur, o=0: (x, 0.0, o, ur, 2.0 if ur >= 0 else -1.0, 1, BASE, 0)
    on, off = step(7.8 * s2)
    for e, o, w in ((on, CREATED, "on the bound"), (off, REPROJ_1, "one float step beyond")):
        c.append(("current, stereo 7.8: " + w, f(32.0, e, 1), f(-32.0, -1.0), T_RIGHT, 1.0, MB2, o, 2))
    for e, o, w in ((on, CREATED, "on the bound"), (off, REPROJ_2, "one float step beyond")):
        c.append(("neighbour, stereo 7.8: " + w, f(96.0, 64.0), f(32.0, e, 1), T_RIGHT, 1.0, MB2, o, 2))
    on, off = step(5.991 * s2)
    for e, o, w in ((on, CREATED, "on the bound"), (off, REPROJ_1, "one float step beyond")):
        c.append(("current, mono 5.991: " + w, f(e, -1.0, 1), f(256.0, 224.0), T_LEFT, MB2, 1.0, o, 3))
    for e, o, w in ((on, CREATED, "on the bound"), (off, REPROJ_2, "one float step beyond")):
        c.append(("neighbour, mono 5.991: " + w, f(64.0, 32.0), f(e, -1.0, 1), T_RIGHT, 1.0, MB2, o, 2))
    return c


def degenerate_cases():
    """W_ZERO and ZERO_DIST lie behind gates that a rigid pose never lets them pass (a zero column of A needs parallel rays, which the parallax
    test refuses; x3D == Ow1 gives z1 = 0).  The call computes what the text computes on any twelve floats, so two poses that are no
    rotations reach them.  -> (name, current row, current Tcw, neighbour row, neighbour Tcw, mb1, mb2, expected outcome, expected branch)"""
    c = []
    # Rcw = diag(0, 1, 1) on both sides: the world x is unobservable, column 0 of A is exactly zero, x = e0 and w = 0.  The neighbour is 1 m ahead
    D = np.diag([0.0, 1.0, 1.0])
    T1 = np.concatenate([D, [[0.125], [0.0], [0.0]]], axis=1).astype(np.float32); T2 = np.concatenate([D, [[-0.25], [0.0], [-1.0]]], axis=1).astype(np.float32)
    a = (352.0, 272.25, 0, -1.0, -1.0, 1, BASE, 0); b = (192.0, 304.0, 0, -1.0, -1.0, 1, BASE, 0)
    c.append(("column 0 of A is zero: the null vector has w = 0", a, T1, b, T2, MB2, MB2, W_ZERO, 1))
    # Rcw1 = diag(1, 1, 0.5), tcw1 = (0, 0, 4): Ow1 = (0, 0, -2) and z1(Ow1) = 3.  The neighbour at (0.25, 0, -4) unprojects its feature to (0, 0, -2) exactly
    T1 = np.concatenate([np.diag([1.0, 1.0, 0.5]), [[0.0], [0.0], [4.0]]], axis=1).astype(np.float32)
    a = (320.0, 240.0, 0, -1.0, -1.0, 1, BASE, 0); b = (256.0, 240.0, 0, 224.0, 2.0, 1, BASE, 0)
    c.append(("x3D == Ow1 in front of a key frame whose pose is no rotation", a, T1, b, Tcw_of(np.eye(3), (0.25, 0, -4.0)), MB2, 1.0, ZERO_DIST, 3))
    return c


def run_pair(a, b, T, cam=CAM2, bf=None, mb1=MB2, mb2=MB2, T1=IDENTITY, **kw):
    """one current feature against one neighbour feature in node 1 -> the two sides, the neighbour's result dict and the summary"""
    cur = side([a], Tcw=T1, mb=mb1); nb = side([b], Tcw=T, mb=mb2)
    res, summ = full(cur, [nb], cam, cam[4] if bf is None else bf, **kw)
    return cur, nb, res[0], summ
