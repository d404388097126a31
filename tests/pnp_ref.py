"""CPU restatement of the relocalisation PnP solver (csrc/pnp.hip, csrc/pnp_core.inc): PnPsolver's EPnP RANSAC, reference
src/PnPsolver.cc:67-950, under the readings include/hvo.h states.  Vectorised over hypotheses (axis 0) with numpy: every float
operation is one IEEE + - * / sqrt on float64 (float32 in CheckInliers) in the order the device code performs it, so results are
compared bit for bit.  Also here: a LITERAL transcription of iterate() / Refine() (a loop with state, `LiteralSolver`) that the
events formulation (`events_from_counts` + hvo_amd.pnp_iterate) is checked against."""
import math
import numpy as np

SEQ_ROWS, EIG_SWEEPS, SVD_SWEEPS = 64, 12, 12
PAIRS12 = [(a, b) for a in range(12) for b in range(a, 12)]
PAIRS3 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
F64 = np.float64


def default_params(**kw):
    p = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5, th2=5.991, seed=1, extra_iterations=8, max_events=8)
    p.update(kw)
    return p


def _clog(x):
    return np.float64(math.log(x)) if x > 0 else (np.float64(-np.inf) if x == 0 else np.float64(np.nan))


def set_ransac(P, N):
    """SetRansacParameters (:121-157) -> dict(N, min_inliers, max_its, epsilon, T, no_more)"""
    eps = np.float32(P["epsilon"])
    n_min = int(np.float32(N) * eps)
    n_min = max(n_min, P["min_inliers"], P["min_set"])
    if N > 0 and eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    if n_min == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):                          # IEEE log / division like C: log(0) = -inf, log(< 0) = nan
            v = np.ceil(_clog(1 - P["probability"]) / _clog(1 - math.pow(float(eps), 3)))
        n_it = P["max_iterations"] if not (v < P["max_iterations"]) else (1 if v < 1 else int(v))
    max_its = max(1, min(n_it, P["max_iterations"]))
    no_more = N < n_min
    return dict(N=N, min_inliers=n_min, max_its=max_its, epsilon=eps, T=0 if no_more else max_its + P["extra_iterations"], no_more=no_more)


def xs32(s):
    s ^= (s << 13) & 0xFFFFFFFF
    s ^= s >> 17
    s ^= (s << 5) & 0xFFFFFFFF
    return s


def draw_sample(seed, j, it, N, min_set):
    """the min-set of hypothesis (candidate j, iteration it = 1..T): xorshift32, x % s, swap-with-last (:188-201)"""
    rs = (seed ^ ((0x9E3779B9 * (j * 1024 + it)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    if rs == 0:
        rs = 0x6D2B79F5
    avail = list(range(N)); out = []
    for _ in range(min_set):
        rs = xs32(rs)
        r = rs % len(avail)
        out.append(avail[r])
        avail[r] = avail[-1]; avail.pop()
    return out


def rsum(terms):
    """terms (H, nr, K) -> (H, K): ascending sum for up to 64 rows, the fixed tree above"""
    H, nr, K = terms.shape
    if nr <= SEQ_ROWS:
        s = np.zeros((H, K), F64)
        for r in range(nr):
            s = s + terms[:, r, :]
        return s
    P = np.zeros((H, 256, K), F64)
    for b in range(0, nr, 256):
        ch = terms[:, b:b + 256, :]
        P[:, :ch.shape[1], :] = P[:, :ch.shape[1], :] + ch
    P = P.reshape(H, 4, 64, K)
    off = 32
    while off > 0:
        P[:, :, :off, :] = P[:, :, :off, :] + P[:, :, off:2 * off, :]
        off >>= 1
    return ((P[:, 0, 0] + P[:, 1, 0]) + P[:, 2, 0]) + P[:, 3, 0]


def rot(num, den2):
    with np.errstate(all="ignore"):
        z = den2 == 0.0
        th = num / np.where(z, 1.0, den2)
        at = np.abs(th)
        tt = 1.0 / (at + np.sqrt(th * th + 1.0))
        tt = np.where(th < 0.0, -tt, tt)
        cc = 1.0 / np.sqrt(tt * tt + 1.0)
        return np.where(z, 1.0, cc), np.where(z, 0.0, tt * cc), np.where(z, 0.0, tt)


def jacobi_eig(A):
    """A (H, n, n) symmetric -> d (H, n) |eigenvalues| in descending eigenvalue, Ut (H, n, n) eigenvectors as rows"""
    A = A.copy(); H, n, _ = A.shape
    V = np.tile(np.eye(n), (H, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(EIG_SWEEPS):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    app, aqq, apq = A[:, p, p].copy(), A[:, q, q].copy(), A[:, p, q].copy()
                    c, s, t = rot(aqq - app, 2.0 * apq)
                    ap, aq = A[:, :, p].copy(), A[:, :, q].copy()
                    nwp = c[:, None] * ap - s[:, None] * aq; nwq = s[:, None] * ap + c[:, None] * aq
                    A[:, :, p] = nwp; A[:, p, :] = nwp; A[:, :, q] = nwq; A[:, q, :] = nwq
                    A[:, p, p] = app - t * apq; A[:, q, q] = aqq + t * apq; A[:, p, q] = 0.0; A[:, q, p] = 0.0
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = c[:, None] * vp - s[:, None] * vq; V[:, :, q] = s[:, None] * vp + c[:, None] * vq
    d = np.einsum("hii->hi", A)
    dd = np.zeros((H, n), F64); Ut = np.zeros((H, n, n), F64)
    idx = np.arange(n)
    for i in range(n):
        gt = (d > d[:, i:i + 1]) | ((d == d[:, i:i + 1]) & (idx[None, :] < i))
        rank = gt.sum(1)
        dd[np.arange(H), rank] = np.abs(d[:, i])
        Ut[np.arange(H), rank, :] = V[:, :, i]
    return dd, Ut


def hestenes(W):
    """W (H, m, n) -> W rotated, Vh (H, n, n), s2 (H, n) squared column norms with the cut ones set to 0"""
    W = W.copy(); H, m, n = W.shape
    Vh = np.tile(np.eye(n), (H, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(SVD_SWEEPS):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    al = np.zeros(H); be = np.zeros(H); ga = np.zeros(H)
                    for i in range(m):
                        wp, wq = W[:, i, p], W[:, i, q]
                        al = al + wp * wp; be = be + wq * wq; ga = ga + wp * wq
                    c, s, _ = rot(be - al, 2.0 * ga)
                    wp, wq = W[:, :, p].copy(), W[:, :, q].copy()
                    W[:, :, p] = c[:, None] * wp - s[:, None] * wq; W[:, :, q] = s[:, None] * wp + c[:, None] * wq
                    vp, vq = Vh[:, :, p].copy(), Vh[:, :, q].copy()
                    Vh[:, :, p] = c[:, None] * vp - s[:, None] * vq; Vh[:, :, q] = s[:, None] * vp + c[:, None] * vq
        s2 = np.zeros((H, n)); tot = np.zeros(H)
        for j in range(n):
            a = np.zeros(H)
            for i in range(m):
                a = a + W[:, i, j] * W[:, i, j]
            s2[:, j] = a; tot = tot + np.sqrt(a)
        cut = 2.0 * 2.220446049250313e-16 * tot
        s2 = np.where(np.sqrt(s2) > cut[:, None], s2, 0.0)
    return W, Vh, s2


def backsub(W, Vh, s2, rhs):
    H, m, n = W.shape
    x = np.zeros((H, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            dt = np.zeros(H)
            for i in range(m):
                dt = dt + W[:, i, j] * rhs[:, i]
            skip = s2[:, j] == 0.0
            cf = dt / np.where(skip, 1.0, s2[:, j])
            x = np.where(skip[:, None], x, x + Vh[:, :, j] * cf[:, None])
    return x


def qr_solve(A, b):
    """qr_solve (:860-950) on A (H, 6, 4), b (H, 6): x (H, 4); a zero column makes the step zero"""
    A = A.copy(); b = b.copy(); H = A.shape[0]; nr, nc = 6, 4
    dead = np.zeros(H, bool); A1 = np.zeros((H, nc)); A2 = np.zeros((H, nc))
    with np.errstate(all="ignore"):
        for k in range(nc):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, nr):
                elt = np.abs(A[:, i - 1, k])
                eta = np.where(eta < elt, elt, eta)
            dead = dead | (eta == 0.0)
            inv_eta = 1.0 / eta
            sm = np.zeros(H)
            for i in range(k, nr):
                A[:, i, k] = A[:, i, k] * inv_eta
                sm = sm + A[:, i, k] * A[:, i, k]
            sigma = np.sqrt(sm)
            sigma = np.where(A[:, k, k] < 0.0, -sigma, sigma)
            A[:, k, k] = A[:, k, k] + sigma
            A1[:, k] = sigma * A[:, k, k]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, nc):
                s = np.zeros(H)
                for i in range(k, nr):
                    s = s + A[:, i, k] * A[:, i, j]
                tau = s / A1[:, k]
                for i in range(k, nr):
                    A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
        for j in range(nc):
            tau = np.zeros(H)
            for i in range(j, nr):
                tau = tau + A[:, i, j] * b[:, i]
            tau = tau / A1[:, j]
            for i in range(j, nr):
                b[:, i] = b[:, i] - tau * A[:, i, j]
        X = np.zeros((H, nc))
        X[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
        for i in range(nc - 2, -1, -1):
            s = np.zeros(H)
            for j in range(i + 1, nc):
                s = s + A[:, i, j] * X[:, j]
            X[:, i] = (b[:, i] - s) / A2[:, i]
    return np.where(dead[:, None], 0.0, X)


def alphas_of(pw, c0, ci):
    d = pw - c0[:, None, :]
    a = [None] * 4
    for j in range(3):
        a[1 + j] = ci[:, 3 * j, None] * d[:, :, 0] + ci[:, 3 * j + 1, None] * d[:, :, 1] + ci[:, 3 * j + 2, None] * d[:, :, 2]
    a[0] = 1.0 - a[1] - a[2] - a[3]
    return np.stack(a, 2)                                        # (H, n, 4)


def pcs_of(al, ccs):
    """(H, n, 4), (H, 12) -> (H, n, 3)"""
    return np.stack([al[:, :, 0] * ccs[:, None, j] + al[:, :, 1] * ccs[:, None, 3 + j] + al[:, :, 2] * ccs[:, None, 6 + j] + al[:, :, 3] * ccs[:, None, 9 + j]
                     for j in range(3)], 2)


def epnp(pw, us, cam, want=None):
    """compute_pose (:477-525) for H problems of n correspondences each: pw (H, n, 3), us (H, n, 2) float64, cam = (fu, fv, uc, vc).
    Returns R (H, 3, 3), t (H, 3).  want: a dict that receives intermediate values (tests)."""
    pw = np.asarray(pw, F64); us = np.asarray(us, F64)
    H, n, _ = pw.shape
    fu, fv, uc, vc = [float(np.float32(v)) for v in cam]
    nd = float(n)
    with np.errstate(all="ignore"):
        c0 = rsum(pw) / nd
        d = pw - c0[:, None, :]
        r = rsum(np.stack([d[:, :, a] * d[:, :, b] for a, b in PAIRS3], 2))
        A = np.zeros((H, 3, 3))
        for k, (a, b) in enumerate(PAIRS3):
            A[:, a, b] = r[:, k]; A[:, b, a] = r[:, k]
        dc, uct = jacobi_eig(A)
        cws = np.zeros((H, 4, 3)); cws[:, 0] = c0
        for i in range(1, 4):
            k = np.sqrt(dc[:, i - 1] / nd)
            cws[:, i] = c0 + k[:, None] * uct[:, i - 1, :]
        CC = np.zeros((H, 3, 3))
        for i in range(3):
            for j in range(1, 4):
                CC[:, i, j - 1] = cws[:, j, i] - c0[:, i]
        W, Vh, s2 = hestenes(CC)
        ci = np.zeros((H, 9))
        for col in range(3):
            rhs = np.zeros((H, 3)); rhs[:, col] = 1.0
            x = backsub(W, Vh, s2, rhs)
            for i in range(3):
                ci[:, 3 * i + col] = x[:, i]
        rho = np.zeros((H, 6)); a, b = 0, 1
        for i in range(6):
            p1, p2 = cws[:, a], cws[:, b]
            rho[:, i] = (p1[:, 0] - p2[:, 0]) * (p1[:, 0] - p2[:, 0]) + (p1[:, 1] - p2[:, 1]) * (p1[:, 1] - p2[:, 1]) + (p1[:, 2] - p2[:, 2]) * (p1[:, 2] - p2[:, 2])
            b += 1
            if b > 3:
                a += 1; b = a + 1
        al = alphas_of(pw, c0, ci)
        M = np.zeros((H, 2 * n, 12))
        for ai in range(4):
            M[:, 0::2, 3 * ai] = al[:, :, ai] * fu
            M[:, 0::2, 3 * ai + 2] = al[:, :, ai] * (uc - us[:, :, 0])
            M[:, 1::2, 3 * ai + 1] = al[:, :, ai] * fv
            M[:, 1::2, 3 * ai + 2] = al[:, :, ai] * (vc - us[:, :, 1])
        r = rsum(np.stack([M[:, :, a] * M[:, :, b] for a, b in PAIRS12], 2))
        MtM = np.zeros((H, 12, 12))
        for k, (a, b) in enumerate(PAIRS12):
            MtM[:, a, b] = r[:, k]; MtM[:, b, a] = r[:, k]
        dm, ut = jacobi_eig(MtM)
        if want is not None:
            want.update(MtM=MtM, d=dm, ut=ut, cws=cws, alphas=al)
        L = np.zeros((H, 6, 10))
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        for i, (a, b) in enumerate(pairs):
            col = 0
            for q in range(4):
                for p in range(q + 1):
                    vp, vq = ut[:, 11 - p], ut[:, 11 - q]
                    dp = [vp[:, 3 * a + k] - vp[:, 3 * b + k] for k in range(3)]
                    dq = [vq[:, 3 * a + k] - vq[:, 3 * b + k] for k in range(3)]
                    dt = dp[0] * dq[0] + dp[1] * dq[1] + dp[2] * dq[2]
                    L[:, i, col] = dt if p == q else 2.0 * dt
                    col += 1
        ccs = []
        for bi in range(3):
            cols = [0, 1, 3, 6] if bi == 0 else ([0, 1, 2] if bi == 1 else [0, 1, 2, 3, 4])
            W, Vh, s2 = hestenes(L[:, :, cols])
            x = backsub(W, Vh, s2, rho)
            be = np.zeros((H, 4)); neg = x[:, 0] < 0
            be[:, 0] = np.sqrt(np.where(neg, -x[:, 0], x[:, 0]))
            if bi == 0:
                for k in (1, 2, 3):
                    be[:, k] = np.where(neg, -x[:, k], x[:, k]) / be[:, 0]
            else:
                be[:, 1] = np.where(neg, np.where(x[:, 2] < 0, np.sqrt(np.abs(x[:, 2])), 0.0), np.where(x[:, 2] > 0, np.sqrt(np.abs(x[:, 2])), 0.0))
                be[:, 0] = np.where(x[:, 1] < 0, -be[:, 0], be[:, 0])
                if bi == 2:
                    be[:, 2] = x[:, 3] / be[:, 0]
            for _ in range(5):
                ga = np.zeros((H, 6, 4)); gb = np.zeros((H, 6))
                b0, b1, b2, b3 = be[:, 0], be[:, 1], be[:, 2], be[:, 3]
                for i in range(6):
                    rl = [L[:, i, k] for k in range(10)]
                    ga[:, i, 0] = 2 * rl[0] * b0 + rl[1] * b1 + rl[3] * b2 + rl[6] * b3
                    ga[:, i, 1] = rl[1] * b0 + 2 * rl[2] * b1 + rl[4] * b2 + rl[7] * b3
                    ga[:, i, 2] = rl[3] * b0 + rl[4] * b1 + 2 * rl[5] * b2 + rl[8] * b3
                    ga[:, i, 3] = rl[6] * b0 + rl[7] * b1 + rl[8] * b2 + 2 * rl[9] * b3
                    gb[:, i] = rho[:, i] - (rl[0] * b0 * b0 + rl[1] * b0 * b1 + rl[2] * b1 * b1 + rl[3] * b0 * b2 + rl[4] * b1 * b2 +
                                            rl[5] * b2 * b2 + rl[6] * b0 * b3 + rl[7] * b1 * b3 + rl[8] * b2 * b3 + rl[9] * b3 * b3)
                be = be + qr_solve(ga, gb)
            cc = np.zeros((H, 12))
            for i in range(4):
                cc = cc + be[:, i, None] * ut[:, 11 - i, :]
            pc00 = pcs_of(al[:, :1, :], cc)[:, 0, 2]
            cc = np.where((pc00 < 0.0)[:, None], -cc, cc)
            ccs.append(cc)
        pcs = [pcs_of(al, cc) for cc in ccs]
        pc0 = [rsum(p) / nd for p in pcs]
        Rs, ts, errs = [], [], []
        for bi in range(3):
            dpc = pcs[bi] - pc0[bi][:, None, :]
            abt = rsum(np.stack([dpc[:, :, j] * d[:, :, m] for j in range(3) for m in range(3)], 2)).reshape(H, 3, 3)
            W, Vh, s2 = hestenes(abt)
            sg = np.sqrt(s2)
            U = np.where(s2[:, None, :] == 0.0, 0.0, W / np.where(sg == 0.0, 1.0, sg)[:, None, :])
            R = np.zeros((H, 3, 3))
            for i in range(3):
                for j in range(3):
                    R[:, i, j] = U[:, i, 0] * Vh[:, j, 0] + U[:, i, 1] * Vh[:, j, 1] + U[:, i, 2] * Vh[:, j, 2]
            det = (R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1] -
                   R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] - R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1])
            R[:, 2, :] = np.where((det < 0)[:, None], -R[:, 2, :], R[:, 2, :])
            t = np.stack([pc0[bi][:, i] - (R[:, i, 0] * c0[:, 0] + R[:, i, 1] * c0[:, 1] + R[:, i, 2] * c0[:, 2]) for i in range(3)], 1)
            Xc = R[:, None, 0, 0] * pw[:, :, 0] + R[:, None, 0, 1] * pw[:, :, 1] + R[:, None, 0, 2] * pw[:, :, 2] + t[:, None, 0]
            Yc = R[:, None, 1, 0] * pw[:, :, 0] + R[:, None, 1, 1] * pw[:, :, 1] + R[:, None, 1, 2] * pw[:, :, 2] + t[:, None, 1]
            iz = 1.0 / (R[:, None, 2, 0] * pw[:, :, 0] + R[:, None, 2, 1] * pw[:, :, 1] + R[:, None, 2, 2] * pw[:, :, 2] + t[:, None, 2])
            ue = uc + fu * Xc * iz; ve = vc + fv * Yc * iz
            u, v = us[:, :, 0], us[:, :, 1]
            err = rsum(np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))[:, :, None])[:, 0] / nd
            Rs.append(R); ts.append(t); errs.append(err)
        sel = np.zeros(H, int); eN = errs[0].copy()
        m = errs[1] < errs[0]; sel[m] = 1; eN[m] = errs[1][m]
        m = errs[2] < eN; sel[m] = 2
        R = np.where((sel == 0)[:, None, None], Rs[0], np.where((sel == 1)[:, None, None], Rs[1], Rs[2]))
        t = np.where((sel == 0)[:, None], ts[0], np.where((sel == 1)[:, None], ts[1], ts[2]))
    return R, t


def check_inliers(R, t, p3d, p2d, max_err, cam, want_err=False):
    """CheckInliers (:308-339): R (H, 3, 3), t (H, 3) float64; p3d (N, 3), p2d (N, 2), max_err (N) float32 -> mask (H, N) uint8, count (H)"""
    fu, fv, uc, vc = [float(np.float32(v)) for v in cam]
    X, Y, Z = [p3d[None, :, k].astype(F64) for k in range(3)]
    with np.errstate(all="ignore"):
        Xc = (R[:, 0, 0, None] * X + R[:, 0, 1, None] * Y + R[:, 0, 2, None] * Z + t[:, 0, None]).astype(np.float32)
        Yc = (R[:, 1, 0, None] * X + R[:, 1, 1, None] * Y + R[:, 1, 2, None] * Z + t[:, 1, None]).astype(np.float32)
        iz = (1.0 / (R[:, 2, 0, None] * X + R[:, 2, 1, None] * Y + R[:, 2, 2, None] * Z + t[:, 2, None])).astype(np.float32)
        ue = uc + fu * Xc.astype(F64) * iz.astype(F64); ve = vc + fv * Yc.astype(F64) * iz.astype(F64)
        dx = (p2d[None, :, 0].astype(F64) - ue).astype(np.float32); dy = (p2d[None, :, 1].astype(F64) - ve).astype(np.float32)
        e2 = dx * dx + dy * dy
        finite = (np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1))[:, None]
        mask = ((e2 < max_err[None, :]) & finite).astype(np.uint8)
    if want_err:
        return mask, mask.sum(1).astype(np.int32), e2
    return mask, mask.sum(1).astype(np.int32)


def tcw32(R, t):
    return np.concatenate([R, t[:, None]], 1).astype(np.float32).reshape(12)


def events_from_counts(counts, min_inliers, refine_count, max_events):
    """k_pnp_scan + k_pnp_events on the host: counts (T), refine_count(record_iteration0) -> the refined count of that record.
    Returns dict(records (iteration0 list, all of them), hyp_event (T), best, best_it0)"""
    best, best_it, recs = 0, -1, []
    hyp_rec = np.full(len(counts), -1, np.int32)
    for it, c in enumerate(counts):
        if c >= min_inliers:
            if c > best:
                best, best_it = int(c), it; recs.append(it)
            hyp_rec[it] = len(recs) - 1
    ne = min(len(recs), max_events)
    rc = [refine_count(it) for it in recs[:ne]]
    hyp_event = np.array([r if (0 <= r < ne and rc[r] > min_inliers) else -1 for r in hyp_rec], np.int32)
    return dict(records=recs, ref_counts=rc, hyp_event=hyp_event, best=best, best_it=best_it, overflow=len(recs) > max_events)


def solve(problem, cam, P, j=0, want_err=False):
    """one candidate, everything hvo_pnp_ransac returns for it.  problem: dict(p3d, p2d, sigma2, feature_index, n_features)"""
    p3d = np.ascontiguousarray(problem["p3d"], np.float32).reshape(-1, 3); p2d = np.ascontiguousarray(problem["p2d"], np.float32).reshape(-1, 2)
    N = len(p3d); nf = int(problem["n_features"]); fi = np.asarray(problem["feature_index"], np.int64)
    max_err = np.asarray(problem["sigma2"], np.float32) * np.float32(P["th2"])
    S = set_ransac(P, N); T = S["T"]; ms = P["min_set"]
    out = dict(S, n_features=nf, hyp_inliers=np.zeros(T, np.int32), hyp_event=np.full(T, -1, np.int32), hyp_sample=np.zeros((T, ms), np.int32), events=[],
               best_n_inliers=0, best_valid=False, best_iteration=0, best_Tcw=np.zeros(12, np.float32), best_inliers=np.zeros(nf, np.uint8), status=0, err2=[])
    if T == 0:
        return out
    samp = np.array([draw_sample(P["seed"], j, it, N, ms) for it in range(1, T + 1)], np.int32)
    R, t = epnp(p3d[samp].astype(F64), p2d[samp].astype(F64), cam)
    res = check_inliers(R, t, p3d, p2d, max_err, cam, want_err)
    mask, cnt = res[0], res[1]
    if want_err:
        out["err2"].append(res[2])
    refined = {}

    def refine(it0):
        idx = np.nonzero(mask[it0])[0]
        Rr, tr = epnp(p3d[idx][None].astype(F64), p2d[idx][None].astype(F64), cam)
        rr = check_inliers(Rr, tr, p3d, p2d, max_err, cam, want_err)
        if want_err:
            out["err2"].append(rr[2])
        refined[it0] = (rr[0][0], int(rr[1][0]), tcw32(Rr[0], tr[0]))
        return refined[it0][1]
    ev = events_from_counts(cnt, S["min_inliers"], refine, P["max_events"])
    out.update(hyp_inliers=cnt, hyp_sample=samp, hyp_event=ev["hyp_event"], status=-5 if ev["overflow"] else 0, hyp_mask=mask)
    for it0 in ev["records"][:P["max_events"]]:
        m, c, T12 = refined[it0]
        inl = np.zeros(nf, np.uint8); inl[fi[m != 0]] = 1
        hin = np.zeros(nf, np.uint8); hin[fi[mask[it0] != 0]] = 1
        out["events"].append(dict(iteration=it0 + 1, n_inliers=c, success=c > S["min_inliers"], Tcw=T12, inliers=inl,
                                  hyp_n_inliers=int(cnt[it0]), hyp_Tcw=tcw32(R[it0], t[it0]), hyp_inliers=hin))
    if ev["best_it"] >= 0:
        b = ev["best_it"]
        inl = np.zeros(nf, np.uint8); inl[fi[mask[b] != 0]] = 1
        out.update(best_n_inliers=ev["best"], best_valid=ev["best"] >= S["min_inliers"], best_iteration=b + 1, best_Tcw=tcw32(R[b], t[b]), best_inliers=inl)
    return out


class LiteralSolver:
    """iterate() (:165-258) and Refine() (:260-305) as written, a loop with state.  hyp(it) -> (count, mask, Tcw) is hypothesis it = 1, 2, ...
    (None past the last one that exists: the replay's bNoMore), refine(mask) -> (count, mask, Tcw)."""

    def __init__(self, N, min_inliers, max_its, hyp, refine):
        self.N, self.min_inliers, self.max_its, self.hyp, self.refine = N, min_inliers, max_its, hyp, refine
        self.mnIterations = 0; self.mnBestInliers = 0; self.mvbBestInliers = None; self.mBestTcw = None

    def iterate(self, nIterations):
        """-> (Tcw or None, bNoMore, inlier mask or None, nInliers)"""
        if self.N < self.min_inliers:
            return None, True, None, 0
        nCurrentIterations = 0
        while self.mnIterations < self.max_its or nCurrentIterations < nIterations:
            nCurrentIterations += 1
            self.mnIterations += 1
            h = self.hyp(self.mnIterations)
            if h is None:
                return None, True, None, 0
            count, mask, Tcw = h
            if count >= self.min_inliers:
                if count > self.mnBestInliers:
                    self.mvbBestInliers = mask; self.mnBestInliers = count; self.mBestTcw = Tcw
                rc, rmask, rT = self.refine(self.mvbBestInliers)
                if rc > self.min_inliers:
                    return rT, False, rmask, rc
        if self.mnIterations >= self.max_its:
            if self.mnBestInliers >= self.min_inliers:
                return self.mBestTcw, True, self.mvbBestInliers, self.mnBestInliers
            return None, True, None, 0
        return None, False, None, 0


def planted_scene(seed, N, outlier_frac=0.0, coplanar=False, noise=0.0, n_features=None, dup=0):
    """a camera pose, N world points in front of it and their projections (float32), a fraction of them replaced by gross outliers"""
    rng = np.random.RandomState(seed)
    cam = (517.3, 516.5, 318.6, 255.3)
    ax = rng.randn(3); ax /= np.linalg.norm(ax); ang = 0.3 * rng.rand() + 0.1
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
    t = rng.randn(3) * 0.3
    uv = np.stack([rng.uniform(20, 620, N), rng.uniform(20, 460, N)], 1)
    z = rng.uniform(1.0, 4.0, N)
    pc = np.stack([(uv[:, 0] - cam[2]) / cam[0] * z, (uv[:, 1] - cam[3]) / cam[1] * z, z], 1)
    pw = (pc - t) @ R                                            # R^T (pc - t)
    if coplanar:                                                 # the world plane Z = 0, exactly: PW0tPW0 has a zero eigenvalue, CC a zero column
        pw = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), np.zeros(N)], 1)
        t = np.array([0.1, -0.05, 4.0]) + 0.1 * rng.randn(3)
    p3d = pw.astype(np.float32)
    pcf = p3d.astype(F64) @ R.T + t
    p2d = np.stack([cam[0] * pcf[:, 0] / pcf[:, 2] + cam[2], cam[1] * pcf[:, 1] / pcf[:, 2] + cam[3]], 1) + noise * rng.randn(N, 2)
    n_out = int(round(outlier_frac * N))
    if n_out:
        who = rng.permutation(N)[:n_out]
        p2d[who] += rng.choice([-1, 1], (n_out, 2)) * rng.uniform(30, 120, (n_out, 2))
    for k in range(dup):
        p3d[N - 1 - k] = p3d[k]; p2d[N - 1 - k] = p2d[k]
    nf = n_features or N + 7
    fi = np.sort(rng.permutation(nf)[:N]).astype(np.int32)
    sigma2 = (np.float32(1.2) ** rng.randint(0, 8, N).astype(np.float32)) ** 2
    return dict(p3d=p3d, p2d=p2d.astype(np.float32), sigma2=sigma2.astype(np.float32), feature_index=fi, n_features=nf,
                Tcw=np.concatenate([R, t[:, None]], 1).reshape(12), cam=cam)


def write_problem_file(path, problems, cam, P):
    """the input of tools/pnp_host.cpp"""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<6iI6fd", len(problems), P["min_set"], P["min_inliers"], P["max_iterations"], P["extra_iterations"], P["max_events"], P["seed"],
                            P["epsilon"], P["th2"], cam[0], cam[1], cam[2], cam[3], P["probability"]))
        for pr in problems:
            p3d = np.ascontiguousarray(pr["p3d"], np.float32).reshape(-1, 3)
            f.write(struct.pack("<2i", len(p3d), pr["n_features"]))
            f.write(p3d.tobytes()); f.write(np.ascontiguousarray(pr["p2d"], np.float32).tobytes())
            f.write(np.ascontiguousarray(pr["sigma2"], np.float32).tobytes()); f.write(np.ascontiguousarray(pr["feature_index"], np.int32).tobytes())


def read_host_result(path, n_kf, min_set):
    """the output of tools/pnp_host.cpp: per candidate dict(N, min_inliers, max_its, T, no_more, epsilon, hyp_inliers, hyp_sample, hyp_Tcw, hyp_mask, records)"""
    b = open(path, "rb").read(); o = 0; out = []

    def take(dt, n):
        nonlocal o
        a = np.frombuffer(b, dt, n, o); o += a.nbytes
        return a
    for _ in range(n_kf):
        N, mi, mx, T, nm = [int(v) for v in take(np.int32, 5)]
        eps = take(np.float32, 1)[0]
        r = dict(N=N, min_inliers=mi, max_its=mx, T=T, no_more=bool(nm), epsilon=eps, hyp_inliers=take(np.int32, T), hyp_sample=take(np.int32, T * min_set).reshape(T, min_set),
                 hyp_Tcw=take(np.float32, 12 * T).reshape(T, 12), hyp_mask=take(np.uint8, T * N).reshape(T, N), records=[])
        for _ in range(int(take(np.int32, 1)[0])):
            it0, c = [int(v) for v in take(np.int32, 2)]
            r["records"].append(dict(it0=it0, count=c, Tcw=take(np.float32, 12), mask=take(np.uint8, N)))
        out.append(r)
    assert o == len(b)
    return out


def two_pose_scene(seed, n_a=10, n_b=11):
    """n_a points that agree with one pose and n_b that agree with another: a record of exactly min_inliers whose Refine cannot pass
    the strict > (:292), and a larger one whose Refine does"""
    a = planted_scene(seed, n_a, n_features=64); b = planted_scene(seed + 1000, n_b, n_features=64)
    rng = np.random.RandomState(seed)
    order = rng.permutation(n_a + n_b)
    cat = lambda k: np.concatenate([a[k], b[k]])[order]
    return dict(p3d=cat("p3d"), p2d=cat("p2d"), sigma2=np.ones(n_a + n_b, np.float32), feature_index=np.sort(rng.permutation(64)[:n_a + n_b]).astype(np.int32),
                n_features=64, cam=a["cam"], Tcw_a=a["Tcw"], Tcw_b=b["Tcw"], is_b=(order >= n_a))


def exact_inlier_scene(seed, n_in, n_out):
    """exactly n_in exact correspondences and n_out gross outliers"""
    N = n_in + n_out
    return planted_scene(seed, N, outlier_frac=n_out / N)


CAM = (517.3, 516.5, 318.6, 255.3)
TWO_POSE_SEED = 3


def cases():
    """name -> dict(problems, P): the crafted GPU cases; tests/test_pnp.py asserts on the CPU that each reaches its path"""
    C = {}
    C["clean40"] = dict(problems=[planted_scene(1, 40)], P=default_params())
    for n in (9, 10, 15, 63, 64, 65, 130):
        C["edge%d" % n] = dict(problems=[planted_scene(10 + n, n, 0.4)], P=default_params(seed=9))
    C["coplanar"] = dict(problems=[planted_scene(6, 50, coplanar=True)], P=default_params(seed=2))
    C["duplicates"] = dict(problems=[planted_scene(8, 30, 0.2, dup=6)], P=default_params(seed=3))
    C["two_pose"] = dict(problems=[two_pose_scene(TWO_POSE_SEED)], P=default_params(seed=5))
    C["overflow"] = dict(problems=[two_pose_scene(TWO_POSE_SEED)], P=default_params(seed=5, max_events=1))
    C["refine280"] = dict(problems=[planted_scene(4, 400, 0.3)], P=default_params())
    for n in (32, 33, 64, 65):
        C["rows%d" % n] = dict(problems=[exact_inlier_scene(20 + n, n, n // 4)], P=default_params(seed=9))
    C["minset5"] = dict(problems=[planted_scene(3, 65, 0.4)], P=default_params(min_set=5))
    C["minset64"] = dict(problems=[planted_scene(5, 100)], P=default_params(min_set=64, extra_iterations=0))
    return C


def multi_problems(n_kf):
    """n_kf candidates of different N for one call"""
    sizes = [40, 9, 130, 15, 64, 33, 10, 65, 22, 100, 12, 63, 31, 48, 17, 80, 25]
    return [planted_scene(100 + j, sizes[j], 0.3 if sizes[j] >= 20 else 0.0) for j in range(n_kf)]
