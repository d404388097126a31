"""CPU restatement of LocalMapping::CreateNewMapLinesConstraint (reference src/LocalMapping.cc:1064-1565) with
LSDmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, true) (src/LSDmatcher.cpp:1195-1231), LSDmatcher::FrameBFMatch (:942-966) and
LSDmatcher::lineDescriptorMAD (:1110-1135).  Test infrastructure only, and THE DEFINITION of the readings csrc/line_triang.hip states at its
head.  Python floats are IEEE doubles, f32() rounds to float (a double result of + - * / sqrt of two floats rounds to the same float as the
float operation), one step per step of the reference.  The readings of tests/new_points_ref.py are reused as they stand: dot3f, dotd, normd,
inv3, mul3, pose and the Jacobi reading svd4_last of cv::SVD::compute.

create_new_map_lines() runs the SEQUENTIAL loops as written: the compacted list of match vectors, key frames read by list position (or,
with pairing = ALIGNED, the searched neighbour itself), every triple in (a, b, ikl) order under the occupancy as it stands, the three
occupancy bytes set when a line is created.  triples_under_initial_occupancy() evaluates every (pair, ikl) alone, as the device does.

The float / double reading of every expression (LocalMapping.cc line numbers):
  :1115 baseline              cv::norm returns double, narrowed by the assignment to `const float`; the difference Ow2 - Ow1 in float
  :1223-1226 F21              R21 = Rcw2 Rwc1 by dot3f; t21 = Rcw2 (Rwc2 tcw2 - Rwc1 tcw1): dot3f, dot3f, a float subtraction, dot3f;
                              inv() is OpenCV's closed 3 x 3 form; ((K2^T.inv() t21x) R21) K1.inv() left to right by dot3f
  :1221 lineVector2, klF      the double line function narrowed to float per element
  :1227-1232 Result1 / 2      F21 ray by dot3f; Mat::dot on float matrices accumulates in double, norm is double, the quotient is narrowed
                              by the assignment to `float`; abs on a float; compared as a double with 0.996
  :1242-1255 L, tWorldVector  K.inv() (x, y, 1) by dot3f; cross: two float products and a float subtraction per element; R12 L2 by dot3f
  :1256-1263 norm_, CosSita   float norm_ = cv::norm (narrowed); Mat /= norm_ scales by the double reciprocal, rounded to float; L1.dot is a
                              double, abs of it a double, narrowed by `float CosSita`; compared as a double with 0.0087 (a NaN passes on)
  :1274-1283 M, A             M = K Tcw by dot3f; A.row(0) = klF3^T M3 and A.row(1) = klF2^T M2 by dot3f; rows 2 and 3 one float product
                              then one float subtraction per element
  :1286-1312 s3D, e3D         svd4_last; w == 0 refuses; x_k * (1.0 / w) in double rounded to float
  :1317-1345 cosParallax      normal = p - Ow in float; dist = (float)cv::norm; dot in double; dist1 * dist2 is a FLOAT product; the double
                              quotient narrowed to float; >= 0.99998 as doubles
  :1347-1364 ratios           float distance / float median depth; < 0.3 as doubles; ratio3 > 1 in float
  :1366-1388 SZC ..           Mat::dot (double) + (double)tcw, narrowed to float; <= 0 refuses, a NaN passes on
  :1391-1458 reprojection     x, y as SZC; invz = (float)(1.0 / (double)z); u = fx * x * invz + cx left to right in float; err = fn0 * u +
                              fn1 * v + fn2 are double products of the double line function with float pixels; err * err > 3.84 * sigma2
                              with sigma2 a float (mvLevelSigma2Line: sf[0] = 1, sf[l] = sf[l - 1] * scale, sigma2[l] = sf[l] * sf[l], in float)
  :1460-1539 overlap          fabs(angle) as a double against 3.0 * PI / 4.0 and 1.0 * PI / 4.0 with PI = 3.1415926; std::min(a, b) = b < a ? b : a
                              and std::max(a, b) = a < b ? b : a on floats; the ratios in float; < 0.85 as doubles.  A zero-length segment
                              makes a ratio inf or NaN: the comparison is false and the triple passes on
An octave outside [0, n_levels) refuses the triple after the occupancy tests (the reference would read mvLevelSigma2Line out of range)."""
import math

import numpy as np

from new_points_ref import f32, ddiv, dot3f, dotd, normd, pose, col, inv3, mul3, svd4_last, Tcw_of, yaw, flip, BASE, IDENTITY

F32 = np.float32
KL_DT = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
                  ("sx", "<f4"), ("sy", "<f4"), ("ex", "<f4"), ("ey", "<f4"), ("sox", "<f4"), ("soy", "<f4"), ("eox", "<f4"), ("eoy", "<f4"),
                  ("length", "<f4"), ("num_pixels", "<i4")])
MAX_LINES, MAX_NEIGHBOURS = 2048, 16
TH_HIGH, NN_RATIO = 80, 0.85
N_LEVELS, SCALE_FACTOR = 8, 1.2
PI = 3.1415926
AS_WRITTEN, ALIGNED = 0, 1
(CREATED, NO_MATCH, IDX_RANGE, OCCUPIED_1, OCCUPIED_2, OCCUPIED_3, BAD_OCTAVE, EPI_PARALLEL, NORM_ZERO_23, NORM_ZERO_1, NOT_COPLANAR, W_ZERO_S, W_ZERO_E,
 PARALLAX_S, PARALLAX_E, RATIO_1, RATIO_2, RATIO_3) = range(18)
BEHIND, REPROJ = 18, 24                               # + 0 .. 5: 1S, 1E, 2S, 2E, 3S, 3E
DISJOINT_1, OVERLAP_1, DISJOINT_2, OVERLAP_2, DISJOINT_3, OVERLAP_3 = range(30, 36)
N_CODES = 36
GATE_SEARCHED, GATE_SKIP, GATE_BASELINE = 0, 1, 2
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_ERR = dict(all="ignore")


def sigma2_table(n_levels=N_LEVELS, scale=SCALE_FACTOR):
    """LINEextractor's constructor: mvScaleFactor and mvLevelSigma2 are vector<float>, scale a float"""
    sf = [1.0]
    for _ in range(1, n_levels): sf.append(f32(sf[-1] * f32(scale)))
    return [f32(s * s) for s in sf]


def dot2d(a, b):
    return a[0] * b[0] + a[1] * b[1]


def cross(a, b):
    return [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])), f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]


def keyframe_constants(kf, cur=None):
    """everything one key frame contributes; cur: the current key frame's constants (None for itself)"""
    with np.errstate(**_ERR):
        R, t, Ow = pose(kf["Tcw"])
        fx, fy, cx, cy = (f32(v) for v in kf["cam"][:4])
        K = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]; Kt = [[fx, 0.0, 0.0], [0.0, fy, 0.0], [cx, cy, 1.0]]
        T = [R[r] + [t[r]] for r in range(3)]
        c = dict(R=R, t=t, Ow=Ow, cam=(fx, fy, cx, cy), Ki=inv3(K), M=[[dot3f(K[r], [T[0][q], T[1][q], T[2][q]]) for q in range(4)] for r in range(3)],
                 med=f32(kf.get("median_depth", 1.0)), n=len(kf["kl"]))
        if cur is None: return c
        R1, t1 = cur["R"], cur["t"]
        R21 = [[dot3f(R[r], R1[q]) for q in range(3)] for r in range(3)]
        c["R1k"] = [[dot3f(R1[r], R[q]) for q in range(3)] for r in range(3)]
        d = [f32(dot3f(col(R, r), t) - dot3f(col(R1, r), t1)) for r in range(3)]
        t21 = [dot3f(R[r], d) for r in range(3)]
        tx = [[0.0, -t21[2], t21[1]], [t21[2], 0.0, -t21[0]], [-t21[1], t21[0], 0.0]]
        c["F21"] = mul3(mul3(mul3(inv3(Kt), tx), R21), cur["Ki"])
        baseline = f32(normd([f32(Ow[k] - cur["Ow"][k]) for k in range(3)]))
        c["baseline"] = baseline
        c["gate"] = GATE_SKIP if kf.get("skip") else (GATE_BASELINE if baseline < f32(kf.get("mb", 0.0)) else GATE_SEARCHED)
    return c


# ---- the search ----
def knn2(q, t):
    """cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2): per query the two smallest (distance, train index)"""
    d = _POP[q[:, None, :] ^ t[None, :, :]].sum(axis=2).astype(np.int64)
    key = d * 65536 + np.arange(len(t))[None, :]
    o = np.sort(key, axis=1)[:, :2]
    return o % 65536, o // 65536


def frame_bf_match(d1, d2, th=TH_HIGH, nn_ratio=NN_RATIO):
    """LSDmatcher.cpp:942-966.  Fewer than two train descriptors: knnMatch(k = 2) cannot rank and nothing matches (the project's reading)"""
    n1 = len(d1)
    m = np.full(n1, -1, np.int32)
    if n1 == 0 or len(d2) < 2: return m
    idx, dist = knn2(d1, d2)
    v1 = [f32(float(dist[i, 1]) - float(dist[i, 0])) for i in range(n1)]
    k = n1 // 2
    med = sorted(v1, reverse=True)[k]                                 # conpare_descriptor_by_NN12_dist sorts descending
    v2 = [f32(abs(f32(v - med))) for v in v1]
    th12 = 1.4826 * sorted(v2)[k]
    th12 = th12 * 0.5
    for i in range(n1):
        d0, d1_ = float(dist[i, 0]), float(dist[i, 1])
        if f32(d1_ - d0) > th12 and d0 < f32(th) and d0 < f32(f32(nn_ratio) * d1_): m[i] = idx[i, 0]
    return m


def search_for_triangulation(desc1, desc2, has1, has2, th=TH_HIGH, nn_ratio=NN_RATIO):
    """LSDmatcher.cpp:1195-1231 with isDouble -> (vMatchedPairs, nmatches)"""
    n1 = len(desc1)
    out = np.full(n1, -1, np.int32)
    if n1 == 0 or len(desc2) == 0: return out, 0
    m12 = frame_bf_match(desc1, desc2, th, nn_ratio); m21 = frame_bf_match(desc2, desc1, th, nn_ratio)
    n = 0
    for i in range(n1):
        j = int(m12[i])
        if j >= 0:
            if m21[j] != i: continue
            if has1[i] or has2[j]: continue
            out[i] = j; n += 1
    return out, n


# ---- one triple ----
def plane_normal(Ki, l):
    s = [dot3f(Ki[r], [float(l["sx"]), float(l["sy"]), 1.0]) for r in range(3)]; e = [dot3f(Ki[r], [float(l["ex"]), float(l["ey"]), 1.0]) for r in range(3)]
    return cross(s, e)


def epi_cos(F, x, y, lv):
    th0 = dot3f(F[0], [x, y, 1.0]); th1 = dot3f(F[1], [x, y, 1.0])
    a = [-th1, th0]
    return abs(f32(ddiv(dot2d(a, lv), math.sqrt(dot2d(a, a)) * math.sqrt(dot2d(lv, lv)))))


def front(k1, k2, k3, l1, l2, l3, f2, n_levels=N_LEVELS, trace=None):
    """the gates before the two solves (:1221-1268) -> an outcome code or None"""
    with np.errstate(**_ERR):
        for l in (l1, l2, l3):
            if int(l["octave"]) < 0 or int(l["octave"]) >= n_levels: return BAD_OCTAVE
        lv = [-f32(f2[1]), f32(f2[0])]
        r1 = epi_cos(k2["F21"], float(l1["sx"]), float(l1["sy"]), lv); r2 = epi_cos(k2["F21"], float(l1["ex"]), float(l1["ey"]), lv)
        if trace is not None: trace.update(result1=r1, result2=r2)
        if r1 > 0.996 or r2 > 0.996: return EPI_PARALLEL
        L1, L2, L3 = plane_normal(k1["Ki"], l1), plane_normal(k2["Ki"], l2), plane_normal(k3["Ki"], l3)
        tw = cross([dot3f(k2["R1k"][r], L2) for r in range(3)], [dot3f(k3["R1k"][r], L3) for r in range(3)])
        norm_ = f32(normd(tw))
        if norm_ == 0.0: return NORM_ZERO_23
        inv = ddiv(1.0, norm_); tw = [f32(v * inv) for v in tw]
        norm_ = f32(normd(L1))
        if norm_ == 0.0: return NORM_ZERO_1
        inv = ddiv(1.0, norm_); L1 = [f32(v * inv) for v in L1]
        cos_sita = f32(abs(dotd(L1, tw)))
        if trace is not None: trace.update(cos_sita=cos_sita)
        if cos_sita > 0.0087: return NOT_COPLANAR
    return None


def systems(k1, k2, k3, l1, f2, f3):
    """the two 4 x 4 matrices (:1274-1301)"""
    g3 = [f32(v) for v in f3]; g2 = [f32(v) for v in f2]
    colm = lambda M, c: [M[0][c], M[1][c], M[2][c]]
    A0 = [dot3f(g3, colm(k3["M"], c)) for c in range(4)]; A1 = [dot3f(g2, colm(k2["M"], c)) for c in range(4)]
    M1 = k1["M"]
    out = []
    for px, py in ((float(l1["sx"]), float(l1["sy"])), (float(l1["ex"]), float(l1["ey"]))):
        out.append([A0, A1, [f32(f32(px * M1[2][c]) - M1[0][c]) for c in range(4)], [f32(f32(py * M1[2][c]) - M1[1][c]) for c in range(4)]])
    return out


def cam_row(k, r, p):
    return f32(dotd(k["R"][r], p) + k["t"][r])


def project(k, p, z):
    fx, fy, cx, cy = k["cam"]
    x = cam_row(k, 0, p); y = cam_row(k, 1, p)
    invz = f32(ddiv(1.0, z))
    return f32(f32(f32(fx * x) * invz) + cx), f32(f32(f32(fy * y) * invz) + cy)


def overlap(l, us, vs, ue, ve, trace=None):
    """:1460-1485 for one view: 0 passes, 1 the segments are disjoint, 2 a ratio is below 0.85"""
    fa = abs(float(l["angle"]))
    vert = fa < 3.0 * PI / 4.0 and fa > 1.0 * PI / 4.0
    pe, ps = (ve, vs) if vert else (ue, us)
    ks, ke = (float(l["sy"]), float(l["ey"])) if vert else (float(l["sx"]), float(l["ex"]))
    minp = ps if ps < pe else pe; maxp = ps if pe < ps else pe
    maxk = ke if ks < ke else ks; mink = ke if ke < ks else ks
    if minp > maxk or mink > maxp: return 1
    hi = maxk if maxk < maxp else maxp; lo = mink if minp < mink else minp
    r1 = f32(ddiv(f32(hi - lo), f32(maxp - minp))); r2 = f32(ddiv(f32(hi - lo), f32(maxk - mink)))
    if trace is not None: trace.setdefault("ratios", []).append((r1, r2))
    return 2 if (r1 < 0.85 or r2 < 0.85) else 0


def tail(k1, k2, k3, l1, l2, l3, f1, f2, f3, S, E, sigma2, trace=None):
    """the gates after the two solves (:1314-1539) -> an outcome code"""
    with np.errstate(**_ERR):
        dS = None
        for e, p in enumerate((S, E)):
            n1 = [f32(p[k] - k1["Ow"][k]) for k in range(3)]; n2 = [f32(p[k] - k2["Ow"][k]) for k in range(3)]; n3 = [f32(p[k] - k3["Ow"][k]) for k in range(3)]
            d1, d2, d3 = f32(normd(n1)), f32(normd(n2)), f32(normd(n3))
            c12 = f32(ddiv(dotd(n1, n2), f32(d1 * d2))); c13 = f32(ddiv(dotd(n1, n3), f32(d1 * d3)))
            if c12 >= 0.99998 or c13 >= 0.99998: return PARALLAX_E if e else PARALLAX_S
            if e == 0: dS = (d1, d2)
        med = k2["med"]
        if f32(ddiv(dS[0], med)) < 0.3: return RATIO_1
        if f32(ddiv(dS[1], med)) < 0.3: return RATIO_2
        d3 = f32(normd([f32(E[k] - S[k]) for k in range(3)]))
        if f32(ddiv(d3, med)) > 1.0: return RATIO_3
        z = []
        for v, k in enumerate((k1, k2, k3)):
            for e, p in enumerate((S, E)):
                z.append(cam_row(k, 2, p))
                if z[-1] <= 0.0: return BEHIND + 2 * v + e
        uv = []
        for v, (k, l, f) in enumerate(((k1, l1, f1), (k2, l2, f2), (k3, l3, f3))):
            sg = float(sigma2[int(l["octave"])])
            for e, p in enumerate((S, E)):
                u, w = project(k, p, z[2 * v + e])
                err = (float(f[0]) * u + float(f[1]) * w) + float(f[2])
                if trace is not None: trace.setdefault("err", []).append(err)
                if err * err > 3.84 * sg: return REPROJ + 2 * v + e
                uv.append((u, w))
        for v, l in enumerate((l1, l2, l3)):
            o = overlap(l, uv[2 * v][0], uv[2 * v][1], uv[2 * v + 1][0], uv[2 * v + 1][1], trace)
            if o: return DISJOINT_1 + 2 * v + o - 1
    return CREATED


def triple(k1, k2, k3, l1, l2, l3, f1, f2, f3, sigma2, n_levels=N_LEVELS, trace=None, solve=svd4_last):
    """one (pair, ikl) after the index and occupancy tests -> (outcome, line3D as six floats: zeros where not reached)"""
    zero = (0.0, 0.0, 0.0)
    o = front(k1, k2, k3, l1, l2, l3, f2, n_levels, trace)
    if o is not None: return o, zero + zero
    with np.errstate(**_ERR):
        pts = []
        for e, A in enumerate(systems(k1, k2, k3, l1, f2, f3)):
            x = solve(A)
            if trace is not None: trace.setdefault("A", []).append(A)
            if x[3] == 0.0: return (W_ZERO_E if e else W_ZERO_S), tuple(pts[0] if pts else zero) + zero
            iw = ddiv(1.0, x[3])
            pts.append(tuple(f32(x[k] * iw) for k in range(3)))
    S, E = pts
    return tail(k1, k2, k3, l1, l2, l3, f1, f2, f3, S, E, sigma2, trace), S + E


# ---- the call ----
def _prepare(cur, kfs, th_high, nn_ratio, pairing):
    k1 = keyframe_constants(cur)
    kc = [keyframe_constants(k, k1) for k in kfs]
    S = [j for j, c in enumerate(kc) if c["gate"] == GATE_SEARCHED] if len(kfs) >= 2 else []
    pairs = []
    if len(S) >= 2 and len(cur["kl"]):
        for a in range(len(S) - 1):
            for b in range(a + 1, len(S)):
                pairs.append((a, b, S[a], S[b]) if pairing == AS_WRITTEN else (S[a], S[b], S[a], S[b]))
    return k1, kc, S, pairs


def _triple_of(cur, kfs, k1, kc, pr, ikl, idx1, idx2, has1, has, sigma2, n_levels):
    kf2, kf3 = pr[0], pr[1]
    zero = (0.0,) * 6
    if idx1 == -1 or idx2 == -1: return NO_MATCH, zero
    if idx1 >= kc[kf2]["n"] or idx2 >= kc[kf3]["n"]: return IDX_RANGE, zero
    if has1[ikl]: return OCCUPIED_1, zero
    if has[kf2][idx1]: return OCCUPIED_2, zero
    if has[kf3][idx2]: return OCCUPIED_3, zero
    return triple(k1, kc[kf2], kc[kf3], cur["kl"][ikl], kfs[kf2]["kl"][idx1], kfs[kf3]["kl"][idx2], cur["linefn"][ikl], kfs[kf2]["linefn"][idx1], kfs[kf3]["linefn"][idx2],
                  sigma2, n_levels)


def _occ(k):
    return np.asarray(k["has_map_line"]).astype(bool).copy()


def _search_all(cur, kfs, kc, S, has1, has, th_high, nn_ratio):
    n1 = len(cur["kl"])
    M = [np.full(n1, -1, np.int32) for _ in kfs]; nm = [0] * len(kfs)
    for j in S:
        M[j], nm[j] = search_for_triangulation(np.asarray(cur["desc"], np.uint8).reshape(-1, 32), np.asarray(kfs[j]["desc"], np.uint8).reshape(-1, 32), has1, has[j], th_high, nn_ratio)
    return M, nm


def triples_under_initial_occupancy(cur, kfs, th_high=TH_HIGH, nn_ratio=NN_RATIO, n_levels=N_LEVELS, scale_factor=SCALE_FACTOR, pairing=AS_WRITTEN):
    """every (pair, ikl) alone -> (matches: dict(match_idx, n_matched, gate) per neighbour; pairs: dict(kf2, kf3, mv2, mv3, outcome, line3d))"""
    k1, kc, S, pairs = _prepare(cur, kfs, th_high, nn_ratio, pairing)
    n1 = len(cur["kl"]); sigma2 = sigma2_table(n_levels, scale_factor)
    has1 = _occ(cur); has = [_occ(k) for k in kfs]
    M, nm = _search_all(cur, kfs, kc, S if pairs else [], has1, has, th_high, nn_ratio)
    matches = [dict(match_idx=M[j], n_matched=nm[j], gate=kc[j]["gate"]) for j in range(len(kfs))]
    out = []
    for pr in pairs:
        oc = np.zeros(n1, np.int8); x = np.zeros((n1, 6), np.float32)
        for ikl in range(n1):
            oc[ikl], x[ikl] = _triple_of(cur, kfs, k1, kc, pr, ikl, int(M[pr[2]][ikl]), int(M[pr[3]][ikl]), has1, has, sigma2, n_levels)
        out.append(dict(kf2=pr[0], kf3=pr[1], mv2=pr[2], mv3=pr[3], outcome=oc, line3d=x))
    return matches, out


def create_new_map_lines(cur, kfs, th_high=TH_HIGH, nn_ratio=NN_RATIO, n_levels=N_LEVELS, scale_factor=SCALE_FACTOR, pairing=AS_WRITTEN):
    """the sequential loops -> (per pair dict(created_idx0, created_idx1, created_idx2, n_created), owner_pair, n_new)"""
    k1, kc, S, pairs = _prepare(cur, kfs, th_high, nn_ratio, pairing)
    n1 = len(cur["kl"]); sigma2 = sigma2_table(n_levels, scale_factor)
    has1 = _occ(cur); has = [_occ(k) for k in kfs]
    M, nm = _search_all(cur, kfs, kc, S if pairs else [], has1, has, th_high, nn_ratio)      # the searches all run before the pair loops
    owner = np.full(n1, -1, np.int32); out = []
    for p, pr in enumerate(pairs):
        c0, c1, c2 = [], [], []
        if nm[pr[2]] != 0 and nm[pr[3]] != 0:                          # nTotalMatched[i] == 0: the pair is skipped
            for ikl in range(n1):
                idx1, idx2 = int(M[pr[2]][ikl]), int(M[pr[3]][ikl])
                o, _ = _triple_of(cur, kfs, k1, kc, pr, ikl, idx1, idx2, has1, has, sigma2, n_levels)
                if o == CREATED:
                    has1[ikl] = True; has[pr[0]][idx1] = True; has[pr[1]][idx2] = True      # the three AddMapLine
                    owner[ikl] = p; c0.append(ikl); c1.append(idx1); c2.append(idx2)
        out.append(dict(created_idx0=np.array(c0, np.int32), created_idx1=np.array(c1, np.int32), created_idx2=np.array(c2, np.int32), n_created=len(c0)))
    return out, owner, int((owner >= 0).sum())


def full(cur, kfs, **kw):
    """what the library returns: (matches, pairs merged with the chain's lists, summary)"""
    matches, pairs = triples_under_initial_occupancy(cur, kfs, **kw)
    chain, owner, n_new = create_new_map_lines(cur, kfs, **kw)
    return matches, [dict(p, **c, status=0) for p, c in zip(pairs, chain)], dict(owner_pair=owner, n_new=n_new, n_pairs=len(pairs))


# ---- scenes ----
CAM2 = (512.0, 512.0, 320.0, 240.0)
SCENE_SEED = 31                                        # the random scene's seed: change it, never a condition of the vacuity test
SCENE_POSES = ((np.eye(3), (0.3, 0.0, 0.0)), (yaw(0.04), (-0.25, 0.05, 0.0)), (np.eye(3), (0.0, 0.3, 0.05)), (yaw(-0.03), (0.2, -0.25, 0.0)))


def line_fn(sx, sy, ex, ey):
    """the line through the two end points, (a, b) of unit length"""
    a, b, c = sy - ey, ex - sx, sx * ey - ex * sy
    n = math.hypot(a, b)
    return (a / n, b / n, c / n) if n > 0 else (0.0, 0.0, 0.0)


def keyline(sx, sy, ex, ey, octave=0, angle=None):
    k = np.zeros((), KL_DT)
    k["sx"], k["sy"], k["ex"], k["ey"] = sx, sy, ex, ey
    k["sox"], k["soy"], k["eox"], k["eoy"] = sx, sy, ex, ey
    k["angle"] = math.atan2(ey - sy, ex - sx) if angle is None else angle
    k["octave"] = octave; k["class_id"] = -1; k["pt_x"] = (sx + ex) / 2; k["pt_y"] = (sy + ey) / 2; k["length"] = math.hypot(ex - sx, ey - sy)
    return k


def side(lines, Tcw=IDENTITY, cam=CAM2, mb=0.0, median_depth=2.0, skip=0):
    """lines: rows of (sx, sy, ex, ey, octave, descriptor, has_map_line[, angle[, line function]])"""
    n = len(lines)
    kl = np.zeros(n, KL_DT); fn = np.zeros((n, 3)); desc = np.zeros((n, 32), np.uint8); has = np.zeros(n, np.uint8)
    for i, r in enumerate(lines):
        kl[i] = keyline(r[0], r[1], r[2], r[3], r[4], r[7] if len(r) > 7 else None)
        fn[i] = r[8] if len(r) > 8 else line_fn(*[float(kl[i][k]) for k in ("sx", "sy", "ex", "ey")])
        desc[i] = r[5]; has[i] = r[6]
    return dict(kl=kl, linefn=fn, desc=desc, has_map_line=has, Tcw=np.asarray(Tcw, np.float32), cam=cam, mb=mb, median_depth=median_depth, skip=skip)


def see(Ps, Pe, Tcw, cam=CAM2, octave=0, desc=BASE, has=0, d=(0.0, 0.0, 0.0, 0.0)):
    """the line row of the 3-D segment Ps - Pe seen from Tcw, its end points moved by d pixels"""
    T = np.asarray(Tcw, np.float64)
    px = []
    for P in (Ps, Pe):
        Pc = T[:, :3] @ np.asarray(P, np.float64) + T[:, 3]
        px += [cam[0] * Pc[0] / Pc[2] + cam[2], cam[1] * Pc[1] / Pc[2] + cam[3]]
    return (px[0] + d[0], px[1] + d[1], px[2] + d[2], px[3] + d[3], octave, desc, has)


T_R, T_L = Tcw_of(np.eye(3), (0.25, 0, 0)), Tcw_of(np.eye(3), (-0.25, 0, 0))
PS, PE = (0.25, -0.25, 2.0), (0.25, 0.25, 2.0)       # the base segment: x = 384 / 320 / 448, y = 176 .. 304 in the three views, exactly
FILL = [flip(100 + 7 * k, start=16 * k) for k in range(1, 4)]      # lines that match nothing: a side needs two for knnMatch(k = 2) to rank


def filler(k, y=20.0):
    return (10.0 + 40 * k, y, 30.0 + 40 * k, y + 60.0, 0, FILL[k], 0)


def base_triple(c=None, n2=None, n3=None, T2=T_R, T3=T_L, med=2.0, **kw):
    """the current key frame and two neighbours, each with the base segment as line 0 and two lines that match nothing"""
    c = see(PS, PE, IDENTITY) if c is None else c
    n2 = see(PS, PE, T2) if n2 is None else n2; n3 = see(PS, PE, T3) if n3 is None else n3
    pad = lambda r, k: [r, filler(k), filler((k + 1) % 3, 300.0)]
    return side(pad(c, 0)), [side(pad(n2, 1), Tcw=T2, median_depth=med, **kw), side(pad(n3, 2), Tcw=T3, median_depth=med)]


def with_(row, **kw):
    """a line row with fields replaced: sx, sy, ex, ey, octave, desc, has, angle, fn"""
    names = ("sx", "sy", "ex", "ey", "octave", "desc", "has", "angle", "fn")
    r = list(row) + [None] * (9 - len(row))
    for k, v in kw.items(): r[names.index(k)] = v
    if r[8] is None: r = r[:8]
    if len(r) == 8 and r[7] is None: r = r[:7]
    return tuple(r)


def full_call_cases():
    """(name, cur, kfs, expected outcome of (pair 0, line 0)): one whole call per outcome code.  The call takes any key lines, line
    functions, angles and twelve-float poses, so a case may give a view a line function or an angle that is not its segment's.  With
    idx_range_scene() and occupied_shift_scenes() every code is reached by a call but two: OCCUPIED_1 (SearchForTriangulation already drops
    a match of an occupied current line: the index test fires first) and W_ZERO_E (the two systems share rows 0 and 1 and the current key
    frame's M; the only exact w == 0 found, a zero column, fires at the start point): direct_cases()"""
    c = []
    add = lambda name, want, *a, **kw: c.append((name,) + base_triple(*a, **kw) + (want,))
    b1, b2, b3 = see(PS, PE, IDENTITY), see(PS, PE, T_R), see(PS, PE, T_L)
    add("the base segment, 2 m away, seen 0.25 m to either side", CREATED)
    add("neighbour 3 holds no partner", NO_MATCH, n3=with_(b3, desc=FILL[0]))
    add("octave 8 of an 8-level pyramid in view 2", BAD_OCTAVE, n2=with_(b2, octave=8))
    hs, he = (0.0, 0.25, 2.0), (0.25, 0.25, 2.0)
    add("a segment parallel to the sideways baseline lies on its epipolar line", EPI_PARALLEL, c=see(hs, he, IDENTITY), n2=see(hs, he, T_R), n3=see(hs, he, T_L))
    add("both neighbours at one pose see one line: the two planes are one", NORM_ZERO_23, T3=T_R, n3=see(PS, PE, T_R))
    add("a current line of zero length", NORM_ZERO_1, c=with_(b1, ex=b1[0], ey=b1[1]))
    add("the current line tilted by 2 px over 128", NOT_COPLANAR, c=with_(b1, ex=b1[2] + 2.0))
    far_s, far_e = (0.25, -50.0, 400.0), (0.25, 50.0, 400.0)
    add("400 m away: the rays are parallel", PARALLAX_S, c=see(far_s, far_e, IDENTITY), n2=see(far_s, far_e, T_R), n3=see(far_s, far_e, T_L), med=400.0)
    mid_e = (0.25, 50.0, 400.0)
    add("the end point 400 m away", PARALLAX_E, c=see(PS, mid_e, IDENTITY), n2=see(PS, mid_e, T_R), n3=see(PS, mid_e, T_L), med=400.0)
    add("median depth 10 m: the start point is closer than 0.3 of it", RATIO_1, med=10.0)
    add("median depth 6.75 m: 2.0156 / 6.75 < 0.3 <= 2.0310 / 6.75", RATIO_2, med=6.75)
    add("median depth 0.4 m: the segment is longer", RATIO_3, med=0.4)
    add("the neighbours' observations swapped: the planes meet 2 m behind the cameras", BEHIND + 0, n2=with_(b3, desc=BASE), n3=with_(b2, desc=BASE))
    add("the current line 3 px aside, octave 0", REPROJ + 0, c=with_(b1, sx=b1[0] + 3.0, ex=b1[2] + 3.0))
    wide = dict(sx=b1[0] + 7.0, ex=b1[2] + 7.0, octave=7)              # the errors are 4.67, -2.29, -2.39 px: octave 7 bears |err| < 7.0, octave 0 1.96
    add("the current line 7 px aside on octave 7: view 2 is the first to refuse", REPROJ + 2, c=with_(b1, **wide))
    add("the same with view 2 on octave 7 too: view 3 refuses", REPROJ + 4, c=with_(b1, **wide), n2=with_(b2, octave=7))
    add("view 2 observes another stretch of the line", DISJOINT_2, n2=with_(b2, sy=400.0, ey=470.0))
    add("view 2 observes 40 px more than is projected", OVERLAP_2, n2=with_(b2, ey=b2[3] + 40.0))
    add("view 3 observes another stretch of the line", DISJOINT_3, n3=with_(b3, sy=10.0, ey=100.0))
    add("view 3 observes half of what is projected", OVERLAP_3, n3=with_(b3, ey=b3[1] + 64.0))
    views = lambda S, E, T2=T_R, T3=T_L: dict(c=see(S, E, IDENTITY), n2=see(S, E, T2), n3=see(S, E, T3), T2=T2, T3=T3)
    add("the end point half a metre behind the current key frame", BEHIND + 1, med=4.0, **views(PS, (0.25, 0.25, -0.5)))
    T_A, T_B = Tcw_of(np.eye(3), (0.3, 0.1, 1.0)), Tcw_of(np.eye(3), (0.0, 0.3, 1.0))      # one metre ahead
    add("the start point behind neighbour 2, one metre ahead", BEHIND + 2, med=1.5, **views((0.25, -0.25, 0.5), (0.25, 0.25, 1.7), T2=T_A))
    add("the end point behind neighbour 2", BEHIND + 3, med=1.5, **views(PS, (0.25, 0.25, 0.9), T2=T_B))
    add("the start point behind neighbour 3", BEHIND + 4, med=1.5, **views((0.25, -0.25, 0.9), PE, T3=T_B))
    add("the end point behind neighbour 3", BEHIND + 5, med=1.5, **views(PS, (0.25, 0.25, 0.9), T3=T_B))
    tilt = lambda row, d: line_fn(row[0], row[1], row[2] + d, row[3])    # the line function of the segment with its end d px aside
    add("the current line's function runs 3 px off its end point (it is read by the distance test only)", REPROJ + 1, c=with_(b1, fn=tilt(b1, 3.0)))
    # a tilted function in view 2 or 3 tilts that view's plane: of 13 px a sixth stays as that view's error at the end point, a third as view 1's
    add("view 2's function 13 px off at the end, views 1 and 3 on octave 7", REPROJ + 3, c=with_(b1, octave=7), n2=with_(b2, fn=tilt(b2, 13.0)), n3=with_(b3, octave=7))
    add("view 3's function 13 px off at the end, views 1 and 2 on octave 7", REPROJ + 5, c=with_(b1, octave=7), n2=with_(b2, octave=7), n3=with_(b3, fn=tilt(b3, 13.0)))
    o7 = lambda row, **kw: with_(row, octave=7, **kw)
    add("the current line flagged horizontal by its angle, views 2 and 3 see the line 4 px aside: x = 384 is beside the projection", DISJOINT_1,
        c=o7(b1, angle=0.0), n2=o7(b2, sx=b2[0] + 4.0, ex=b2[2] + 4.0), n3=o7(b3, sx=b3[0] + 4.0, ex=b3[2] + 4.0))
    add("the current line 1 px wide in x and flagged horizontal: the projection covers a third of it", OVERLAP_1, c=o7(b1, ex=b1[2] + 1.0, angle=0.0), n2=o7(b2), n3=o7(b3))
    c.append(("poses with Rcw = diag(0, 1, 1): column 0 of both systems is zero, the null vector is e0",) + w_zero_scene() + (W_ZERO_S,))
    return c


def w_zero_scene():
    """the call computes what the text computes on any twelve floats: three poses whose rotation block is diag(0, 1, 1) make the world x
    unobservable, column 0 of every M and of both 4 x 4 systems is exactly zero, no Jacobi rotation touches it and w == 0.  The lines are
    horizontal (L1 has no x component, so CosSita is 0) at three heights (the planes of views 2 and 3 differ)"""
    D = np.diag([0.0, 1.0, 1.0])
    Td = lambda t: np.concatenate([D, np.array(t, np.float64)[:, None]], axis=1).astype(np.float32)
    pad = lambda r, k: [r, filler(k), filler((k + 1) % 3, 300.0)]
    rows = ((300.0, 200.0, 420.0, 200.0, 0, BASE, 0), (280.0, 260.0, 400.0, 260.0, 0, BASE, 0), (310.0, 150.0, 450.0, 150.0, 0, BASE, 0))
    return side(pad(rows[0], 0), Tcw=Td((0.1, 0.0, 0.0))), [side(pad(rows[1], 1), Tcw=Td((0.2, 0.1, 0.0))), side(pad(rows[2], 2), Tcw=Td((-0.3, -0.1, 0.1)))]


def bisect_float(lo, hi, fails):
    """adjacent floats lo < hi with fails(lo) False and fails(hi) True (fails is monotone between the two given values)"""
    lo, hi = F32(lo), F32(hi)
    assert not fails(float(lo)) and fails(float(hi))
    while np.nextafter(lo, F32(np.inf)) < hi:
        mid = F32((float(lo) + float(hi)) / 2)
        if mid <= lo or mid >= hi: mid = np.nextafter(lo, F32(np.inf))
        if fails(float(mid)): hi = mid
        else: lo = mid
    return float(lo), float(hi)


def outcome00(cur, kfs, **kw):
    return int(full(cur, kfs, **kw)[1][0]["outcome"][0])


def bound_cases():
    """the CosSita, chi-square and 0.85 bounds approached from both sides by adjacent floats of one input coordinate ->
    (name, cur, kfs, expected) in pairs: the last passing value, the first refused one"""
    b1, b2 = see(PS, PE, IDENTITY), see(PS, PE, T_R)
    c = []

    def pair(name, want, make, lo, hi):
        f = lambda v: outcome00(*make(v)) == want
        a, b = bisect_float(lo, hi, f)
        c.append((name + ": the last float that passes", ) + make(a) + (outcome00(*make(a)),))
        c.append((name + ": the next float", ) + make(b) + (want,))
    pair("CosSita 0.0087, the current line's end x", NOT_COPLANAR, lambda v: base_triple(c=with_(b1, ex=v, octave=7), n2=with_(b2, octave=7), n3=with_(see(PS, PE, T_L), octave=7)), b1[2], b1[2] + 2.0)
    pair("chi-square 3.84, the current line's x", REPROJ + 0, lambda v: base_triple(c=with_(b1, sx=v, ex=v)), b1[0], b1[0] + 3.0)
    pair("overlap 0.85, view 2's observed end y", OVERLAP_2, lambda v: base_triple(n2=with_(b2, ey=v)), b2[3], b2[3] + 40.0)
    return c


def direct_cases():
    """(name, keyword arguments of direct(), expected): what no whole call reaches, given to the gate functions themselves"""
    c = []
    add = lambda name, want, **kw: c.append((name, kw, want))
    add("the three occupancy bytes in the text's order", OCCUPIED_1, occupied=(1, 1, 1))
    add("pKF2's line holds a map line", OCCUPIED_2, occupied=(0, 1, 1))
    add("pKF3's line holds a map line", OCCUPIED_3, occupied=(0, 0, 1))
    add("a null vector with w == 0 at the start point", W_ZERO_S, w_zero=0)
    add("a null vector with w == 0 at the end point", W_ZERO_E, w_zero=1)
    return c


def direct(occupied=None, w_zero=None):
    """the base triple with occupancy bytes given by hand, or with the solve's w replaced by 0 at one end point -> the outcome"""
    rows = [see(PS, PE, T) for T in (IDENTITY, T_R, T_L)]
    cur = side([rows[0]]); kfs = [side([rows[1]], Tcw=T_R, median_depth=2.0), side([rows[2]], Tcw=T_L, median_depth=2.0)]
    k1 = keyframe_constants(cur); kc = [keyframe_constants(k, k1) for k in kfs]
    sg = sigma2_table()
    if occupied is not None:
        has = [np.array([occupied[1]], bool), np.array([occupied[2]], bool)]
        return _triple_of(cur, kfs, k1, kc, (0, 1, 0, 1), 0, 0, 0, np.array([occupied[0]], bool), has, sg, N_LEVELS)[0]
    a = (k1, kc[0], kc[1], cur["kl"][0], kfs[0]["kl"][0], kfs[1]["kl"][0], cur["linefn"][0], kfs[0]["linefn"][0], kfs[1]["linefn"][0])
    calls = []

    def solve(A):
        calls.append(1)
        x = svd4_last(A)
        return [x[0], x[1], x[2], 0.0] if len(calls) - 1 == w_zero else x
    return triple(*a, sg, solve=solve)[0]


def nan_overlap_case():
    """a triangulated segment along the camera's x axis, every line flagged vertical by its angle and observed with sy == ey: on the y axis
    both the projected and the observed segment have zero length, both ratios are 0 / 0, both comparisons with 0.85 are false and the triple
    passes -> (the outcome, the ratios met)"""
    S, E = (0.125, 0.25, 2.0), (0.375, 0.25, 2.0)
    T2, T3 = Tcw_of(np.eye(3), (0, 0.25, 0)), Tcw_of(np.eye(3), (0, -0.25, 0))
    rows = [with_(see(S, E, T), angle=math.pi / 2) for T in (IDENTITY, T2, T3)]
    cur = side([rows[0]]); kfs = [side([rows[1]], Tcw=T2), side([rows[2]], Tcw=T3)]
    k1 = keyframe_constants(cur); kc = [keyframe_constants(k, k1) for k in kfs]
    tr = {}
    o = tail(k1, kc[0], kc[1], cur["kl"][0], kfs[0]["kl"][0], kfs[1]["kl"][0], cur["linefn"][0], kfs[0]["linefn"][0], kfs[1]["linefn"][0], S, E, sigma2_table(), tr)
    return o, tr.get("ratios", [])


def nan_overlap_scene():
    """the same through a whole call: the two solves return the planted end points exactly, so every view projects both on one row -> (cur, kfs)"""
    S, E = (0.125, 0.25, 2.0), (0.375, 0.25, 2.0)
    T2, T3 = Tcw_of(np.eye(3), (0, 0.25, 0)), Tcw_of(np.eye(3), (0, -0.25, 0))
    rows = [with_(see(S, E, T), angle=math.pi / 2) for T in (IDENTITY, T2, T3)]
    return base_triple(c=rows[0], n2=rows[1], n3=rows[2], T2=T2, T3=T3)


def search_cases():
    """(name, current descriptors, neighbour descriptors, has1, has2, th_high, nn_ratio, expected vMatchedIndices).  Rows are BASE-like
    descriptors far from each other (FAR[k]) with bits flipped"""
    far = lambda k: flip(128, base=np.roll(BASE, 3 * k) ^ np.uint8(17 * k), start=(37 * k) % 128)
    z = lambda n: np.zeros(n, np.uint8)
    c = []
    A, B, Cc, D = far(0), far(1), far(2), far(3)
    c.append(("three clean partners", [A, B, Cc], [B, Cc, A], z(3), z(3), 80, 0.85, [2, 0, 1]))
    # line 0 and line 1 of the current side both prefer neighbour line 0; that line prefers current line 0
    c.append(("a one-way match that the mutual check removes", [A, flip(6, A, 200), Cc], [flip(2, A), Cc, D], z(3), z(3), 80, 0.85, [0, -1, 1]))
    c.append(("distance 79 is taken, 80 is not (d0 < TH)", [A, B, Cc], [flip(79, A), flip(80, B), Cc], z(3), z(3), 80, 0.85, [0, -1, 2]))
    c.append(("an occupied line on either side", [A, B, Cc], [A, B, Cc], np.array([1, 0, 0], np.uint8), np.array([0, 1, 0], np.uint8), 80, 0.85, [-1, -1, 2]))
    return c


def _far(k):
    """descriptors about 128 bits from each other"""
    return np.random.RandomState(1000 + k).randint(0, 256, 32).astype(np.uint8)


def ratio_case():
    """d0 < 0.85f * d1 on either side of the bound.  Every current line k has two candidates of its own: its base with `best` bits flipped and
    the base with 100 other bits flipped.  0.85f * 100 = 84.99999..: best = 84 passes, 85 does not (and 85 < 80 fails anyway, so th_high is
    255 here) -> (current descriptors, neighbour descriptors, th_high, expected)"""
    d1, d2, want = [], [], []
    for k, best in enumerate((84, 85, 20)):
        q = _far(k)
        d1.append(q); d2 += [flip(best, q, 0), flip(100, q, 128)]
        want.append(2 * k if best < 85 else -1)
    return d1, d2, 255, want


def mad_cases():
    """lineDescriptorMAD's threshold with tied gaps.  Five current lines, each with candidates of its own at distances (best, best + gap).
    Gaps 40, 40, 40, 12, 90: element 2 of the descending order is 40, the deviations 0, 0, 0, 28, 50 have the median 0 and `dist_12 > 0` keeps
    all five.  Gaps 40, 30, 20, 7, 90: the median gap is 30, the deviations 10, 0, 10, 23, 60 have the median 10, the threshold is
    1.4826 * 10 * 0.5 = 7.413: the gap of 7 fails, a gap of 8 in its place passes -> list of (d1, d2, expected)"""
    out = []
    for gaps, keep in (((40, 40, 40, 12, 90), (1, 1, 1, 1, 1)), ((40, 30, 20, 7, 90), (1, 1, 1, 0, 1)), ((40, 30, 20, 8, 90), (1, 1, 1, 1, 1))):
        d1, d2, want = [], [], []
        for k, g in enumerate(gaps):
            q = _far(10 + k)
            d1.append(q); d2 += [flip(5, q, 0), flip(5 + g, q, 100)]
            want.append(2 * k if keep[k] else -1)
        out.append((d1, d2, want))
    return out


def gated_middle_scene(n_extra=0):
    """three neighbours, the middle one gated by its baseline: AS_WRITTEN pairs match vector 2 with key frame 1"""
    T_U = Tcw_of(np.eye(3), (0.0, 0.01, 0.0))                          # 1 cm away: baseline < mb = 0.05
    c = see(PS, PE, IDENTITY)
    pad = lambda r, k: [r, filler(k), filler((k + 1) % 3, 300.0)]
    cur = side(pad(c, 0))
    kfs = [side(pad(see(PS, PE, T_R), 1), Tcw=T_R), side([see(PS, PE, T_U)], Tcw=T_U, mb=0.05), side(pad(see(PS, PE, T_L), 2), Tcw=T_L)]
    return cur, kfs


def idx_range_scene():
    """as gated_middle_scene, with the partner in neighbour 2 at index 2: the gated key frame 1 has one line, so AS_WRITTEN refuses idx2 >= NL"""
    cur, kfs = gated_middle_scene()
    k = kfs[2]
    order = [1, 2, 0]
    kfs[2] = dict(k, kl=k["kl"][order], linefn=k["linefn"][order], desc=k["desc"][order], has_map_line=k["has_map_line"][order])
    return cur, kfs


def occupied_shift_scenes():
    """OCCUPIED_2 and OCCUPIED_3 are reached by a shifted pair only (the search drops a match whose own line is occupied): a gated key frame
    at position 0, resp. 1, whose line 0 holds a map line, is read by AS_WRITTEN in place of the searched neighbour -> (cur, kfs, expected)"""
    out = []
    cur, kfs = gated_middle_scene()
    k = kfs[1]
    occ = dict(k, has_map_line=np.ones(len(k["kl"]), np.uint8))
    out.append((cur, [kfs[0], occ, kfs[2]], OCCUPIED_3))               # pairs (kf2, kf3, mv2, mv3) = (0, 1, 0, 2)
    out.append((cur, [occ, kfs[0], kfs[2]], OCCUPIED_2))               # (0, 1, 1, 2)
    return out


def random_scene(n=200, seed=SCENE_SEED, poses=SCENE_POSES, noise=0.25, occupied=0.1, cam=(535.4, 539.2, 320.1, 247.6), skip=(), mb=0.05, spare=0.15):
    """n planted 3-D segments seen from the current pose (the identity) and from every pose of `poses`, each neighbour in its own line order,
    with pixel noise, up to six descriptor bits flipped, a share of segments replaced by unrelated lines, and occupancy on every side"""
    rng = np.random.RandomState(seed)
    mid = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)], axis=1)
    dirs = rng.normal(size=(n, 3)); dirs[:, 2] *= 0.3
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    half = rng.uniform(0.15, 0.5, n)[:, None]
    Ps, Pe = mid - dirs * half, mid + dirs * half
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    octv = rng.choice(3, n, p=[0.6, 0.3, 0.1])

    def view(T, perm, flips, cut):
        rows = []
        for i in perm:
            d = desc[i].copy()
            for b in rng.choice(256, rng.randint(0, flips + 1), replace=False): d[b >> 3] ^= 1 << (b & 7)
            if rng.rand() < spare: d = rng.randint(0, 256, 32).astype(np.uint8)
            nz = rng.normal(0, noise * (6.0 if rng.rand() < 0.15 else 1.0), 4)      # (a share of badly localised lines)
            s, e = (Ps[i], Pe[i])
            u = rng.rand()
            if u < cut: e = s + (e - s) * rng.uniform(0.3, 0.9)               # the view sees a part of the segment only
            elif u < 1.25 * cut: s, e = e, e + (e - s) * 0.5                  # or the stretch beyond it
            rows.append(see(s, e, T, cam=cam, octave=int(octv[i]), desc=d, has=int(rng.rand() < occupied), d=tuple(nz)))
        return rows
    cur = side(view(IDENTITY, np.arange(n), 0, 0.0), cam=cam)
    kfs = []
    for j, (R, C) in enumerate(poses):
        T = Tcw_of(R, C)
        kfs.append(side(view(T, rng.permutation(n), 6, 0.2), Tcw=T, cam=cam, mb=mb, median_depth=4.0, skip=1 if j in skip else 0))
    return cur, kfs


def cut(side_, n):
    """the first n lines of a key frame"""
    return dict(side_, **{k: side_[k][:n] for k in ("kl", "linefn", "desc", "has_map_line")})


def neighbours_of_frame(kl, desc, poses, cam, seed, mb=0.05, median_depth=3.0):
    """neighbours that see a real frame's key lines: each line's end points are unprojected at drawn depths from the identity pose and the
    3-D segment is observed from every pose of `poses`, in reversed line order, with up to six descriptor bits flipped"""
    rng = np.random.RandomState(seed)
    n = len(kl)
    zs, ze = rng.uniform(2.0, 4.0, n), rng.uniform(2.0, 4.0, n)
    un = lambda x, y, z: ((float(x) - cam[2]) * z / cam[0], (float(y) - cam[3]) * z / cam[1], z)
    kfs = []
    for R, C in poses:
        T = Tcw_of(R, C)
        rows = []
        for i in range(n - 1, -1, -1):
            d = np.asarray(desc[i], np.uint8).copy()
            for b in rng.choice(256, rng.randint(0, 7), replace=False): d[b >> 3] ^= 1 << (b & 7)
            rows.append(see(un(kl["sx"][i], kl["sy"][i], zs[i]), un(kl["ex"][i], kl["ey"][i], ze[i]), T, cam=cam, octave=int(kl["octave"][i]), desc=d, has=int(rng.rand() < 0.1),
                            d=tuple(rng.normal(0, 0.2, 4))))
        kfs.append(side(rows, Tcw=T, cam=cam, mb=mb, median_depth=median_depth))
    return kfs


def toy_desc(k):
    """the toy map's descriptor k: 32 bytes of a linear congruential sequence (examples/create_map_lines.cpp has the same)"""
    v = ((k + 1) * 2654435761) & 0xFFFFFFFF
    out = []
    for _ in range(32):
        v = (v * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(v >> 24)
    return np.array(out, np.uint8)


TOY_X = (-0.5, -0.25, 0.25, 0.5, 0.75, 1.0)
TOY_C = (0.25, -0.25, 0.5)


def toy_map():
    """the map of examples/create_map_lines.cpp: six vertical segments 2 m away, the current key frame at the origin and three neighbours
    beside it, each with the lines in reversed order; neighbour 0 lacks lines 2 and 3, the current line 5 holds a map line"""
    seg = lambda i: ((TOY_X[i], -0.25, 2.0), (TOY_X[i], 0.25, 2.0))
    cur = side([see(*seg(i), IDENTITY, desc=toy_desc(i), has=int(i == 5)) for i in range(6)])
    kfs = []
    for j, cx in enumerate(TOY_C):
        T = Tcw_of(np.eye(3), (cx, 0.0, 0.0))
        kfs.append(side([see(*seg(i), T, desc=toy_desc(100 + i if (j == 0 and i in (2, 3)) else i)) for i in range(5, -1, -1)], Tcw=T, median_depth=2.0))
    return cur, kfs
