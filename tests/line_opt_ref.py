"""CPU restatement (numpy float64) of the two per-frame steps between the Frame constructor and Track() in Tracking::GrabImageRGBD_wh
(reference src/Tracking.cc:270-335), and a deterministic scene generator.  g2o cannot be built here (no Eigen), so tests/test_line_opt.py
pins this file by known answers worked by hand.

What is restated, with the files it was written from:
  part 1       Manhattan::computeStructConstrains(frame, idx, par, perp) (src/Manhattan.cpp:107-161) with computeAngle / computeAngle2D
               (:1054-1087) and the thresholds of Manhattan::Manhattan (:28-30); the row rules of src/Tracking.cc:280 and :401
  graph        Optimizer::LineOptStruct, src/Optimizer.cc:1542-1707: which lines get vertices, which list entries get edges
  edges        ParEptsNVector3DSingleFrame / PerpEptsNVector3DSingleFrame over ComputeAngle3D (include/g2oMSC.h:25-34, 123-190)
  Jacobians    g2o's numeric rule for a binary edge: central differences, delta 1e-9, per vertex and coordinate, times 1 / (2 delta)
  quadratic    the binary edge's constructQuadraticForm with RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91); rows 1 and 2 of
               the error are zero, so a line's block is rho' J0^T J0 and b is -rho' J0 e0
  Levenberg    core/optimization_algorithm_levenberg.cpp:61-164 with one lambda over all blocks; SparseOptimizer::optimize stops a round at the
               first iteration that is not OK, and returns before computing anything when no vertex is active
  rounds       Optimizer.cc:1711-1831, the final rejection :1834-1851, the write-back :1858-1874 with its vertex(0) test
Readings (the same in csrc/line_opt.hip): the Hessian is block-diagonal, one 6 x 6 block per line (start, end), solved
by LDL^T without pivoting; the solve fails when any block has a pivot that is exactly 0 or not finite, and the step of a failed solve is
taken as zero (tempChi = DBL_MAX rejects the trial either way); a stored _error is never kept per edge: classification re-evaluates an active
edge at the end points of the round's last computeActiveErrors (the last trial, accepted or not) and a flagged edge at the estimate, the
same arithmetic on the same inputs."""
import numpy as np

DELTA = 1e-9
F32 = np.float32
DBL_MAX = np.finfo(np.float64).max


def default_params(**kw):
    p = dict(cos_par=np.cos(3 * 0.0174533), cos_perp=np.cos((90.0 - 3) * 0.0174533), huber_delta=float(F32(np.sqrt(0.02))),
             chi2_reject=0.02, chi2_round=(F32(0.02), F32(0.01)), min_constraints=5, iterations=5, row_rule=0)
    p.update(kw)
    return p


class Ops:
    """arithmetic that may differ between two correct implementations: the order of the sums, and the libm results (sqrt, pow) when
    ulp_seed is set: each moved by one ulp in a pseudo-random direction"""
    def __init__(self, order="seq", ulp_seed=None):
        self.order = order
        self.rng = np.random.RandomState(ulp_seed) if ulp_seed is not None else None

    def _nudge(self, v):
        if self.rng is None:
            return v
        v = np.asarray(v, np.float64)
        d = self.rng.randint(0, 2, size=v.shape) * 2 - 1
        return np.nextafter(v, np.where(d > 0, np.inf, -np.inf))

    def sqrt(self, x):
        with np.errstate(invalid="ignore"):
            return self._nudge(np.sqrt(x))

    def pow3(self, x):
        return float(self._nudge(np.float64(x ** 3.0)))

    def sum_lines(self, a):
        """sum of one value per line (index = line).  seq: a running sum.  tree: the kernel's -- thread t of 256 adds lines t, t + 256, ...
        in order, a wave halves its 64 lanes (lane i += lane i + 32, 16, ... 1), waves 0..3 are added in order."""
        a = np.asarray(a, np.float64)
        if a.shape[0] == 0:
            return 0.0
        if self.order == "seq":
            return float(np.cumsum(a)[-1])
        n = a.shape[0]; k = (n + 255) // 256
        p = np.zeros(k * 256); p[:n] = a
        p = np.cumsum(p.reshape(k, 256), axis=0)[-1].reshape(4, 64)
        off = 32
        while off:
            p[:, :off] = p[:, :off] + p[:, off:2 * off]; off //= 2
        return float(((p[0, 0] + p[1, 0]) + p[2, 0]) + p[3, 0])

    def sum_edges_of_line(self, rows, partner):
        """sum over one line's edges of rows (edges x columns).  seq: in insertion order (the parallel list, then the perpendicular list).
        tree: lane l of 64 adds the edges with partner l, l + 64, ... in order, then the lanes are halved."""
        if self.order == "seq":
            return np.cumsum(rows, axis=0)[-1]
        lanes = np.zeros((64, rows.shape[1]))
        o = np.argsort(partner, kind="stable")
        rows, partner = rows[o], partner[o]
        for c in np.unique(partner // 64):
            s = (partner // 64) == c
            lanes[partner[s] % 64] = lanes[partner[s] % 64] + rows[s]
        off = 32
        while off:
            lanes[:off] = lanes[:off] + lanes[off:2 * off]; off //= 2
        return lanes[0]


# ---------------------------------------------------------------- part 1
def struct_constraints(linefn, line_eq, params=None):
    """rel (n x n int8): row k = line k's lists, 1 parallel, 2 perpendicular.  linefn: mvKeyLineFunctions (n x 3 doubles); line_eq: mvLineEq
    (n x 3 floats)."""
    p = params or default_params()
    fn = np.asarray(linefn, np.float64).reshape(-1, 3); q32 = np.asarray(line_eq, F32).reshape(-1, 3); q = q32.astype(np.float64)
    n = len(fn)
    rel = np.zeros((n, n), np.int8)
    if n == 0:
        return rel
    with np.errstate(all="ignore"):
        x, y = fn[:, 0] / fn[:, 2], fn[:, 1] / fn[:, 2]
        kx, ky, ix, iy = x[:, None], y[:, None], x[None, :], y[None, :]
        a2 = np.abs((ix * kx + iy * ky) / (np.sqrt(ix * ix + iy * iy) * np.sqrt(kx * kx + ky * ky)))
        k0, k1, k2 = (q[:, j][:, None] for j in range(3)); i0, i1, i2 = (q[:, j][None, :] for j in range(3))
        a3 = np.abs(((i0 * k0 + i1 * k1) + i2 * k2) / (np.sqrt((i0 * i0 + i1 * i1) + i2 * i2) * np.sqrt((k0 * k0 + k1 * k1) + k2 * k2)))
        perp = (a2 < p["cos_perp"]) & (a3 < p["cos_perp"])
        par = ~perp & (a2 > p["cos_par"]) & (a3 > p["cos_par"])
    rel[par] = 1; rel[perp] = 2
    if p["row_rule"] == 1:
        skip = q32[:, 2] == 0.0
    else:
        skip = (q32[:, 0] == -1.0) & (q32[:, 1] == -1.0) & (q32[:, 2] == -1.0)
    rel[skip, :] = 0
    rel[np.arange(n), np.arange(n)] = 0
    return rel


def lists_of(rel_row):
    """(mvParLinesIdx[k], mvPerpLinesIdx[k]): partner indices in ascending order, -1 in a slot LineOptStruct rejected"""
    r = np.asarray(rel_row)
    ip, iq = np.nonzero(np.abs(r) == 1)[0], np.nonzero(np.abs(r) == 2)[0]
    return np.where(r[ip] > 0, ip, -1).tolist(), np.where(r[iq] > 0, iq, -1).tolist()


# ---------------------------------------------------------------- part 2
class Result:
    pass


def huber_v(e, delta):
    dsqr = delta * delta
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(e)
        inl = e <= dsqr
        return np.where(inl, e, 2 * s * delta - dsqr), np.where(inl, 1.0, delta / s)


def ldlt_blocks(H, b):
    """x of H x = b for a stack of 6 x 6 blocks by LDL^T without pivoting; ok per block: no pivot exactly 0 or not finite"""
    n = len(H)
    L = np.zeros((n, 6, 6)); D = np.zeros((n, 6)); y = np.zeros((n, 6)); x = np.zeros((n, 6)); ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = H[:, j, j].copy()
            for k in range(j): s = s - L[:, j, k] * L[:, j, k] * D[:, k]
            D[:, j] = s; ok &= ~((s == 0.0) | ~np.isfinite(s))
            for i in range(j + 1, 6):
                s2 = H[:, i, j].copy()
                for k in range(j): s2 = s2 - L[:, i, k] * L[:, j, k] * D[:, k]
                L[:, i, j] = s2 / D[:, j]
        for i in range(6):
            s = b[:, i].copy()
            for k in range(i): s = s - L[:, i, k] * y[:, k]
            y[:, i] = s
        for i in range(5, -1, -1):
            s = y[:, i] / D[:, i]
            for k in range(i + 1, 6): s = s - L[:, k, i] * x[:, k]
            x[:, i] = s
    return x, ok


class _Graph:
    def __init__(self, rel, A, B, line_eq, p, ops):
        self.ops = ops; self.p = p
        rel = np.asarray(rel, np.int8); n = len(rel); self.n = n
        A = np.asarray(A, np.float64).reshape(n, 3); B = np.asarray(B, np.float64).reshape(n, 3)
        q32 = np.asarray(line_eq, F32).reshape(n, 3); q = q32.astype(np.float64)
        cnt = (rel != 0).sum(axis=1)                                         # list sizes, slots holding -1 included
        ent = cnt >= p["min_constraints"]
        ent &= ~((A[:, 2] == 0.0) | (A[:, 0] == -1.0) | (B[:, 2] == 0.0) | (B[:, 0] == -1.0))
        ent &= ~((np.abs(B[:, 0] - A[:, 0]) < 0.00001) & (np.abs(B[:, 1] - A[:, 1]) < 0.00001))
        ent &= ~(np.isnan(A).any(axis=1) | np.isnan(B).any(axis=1))
        self.entered = ent
        valid = ~((q[:, 2] == 0.0) | (q[:, 0] == -1.0))                       # a partner's mvLineEq that gives an edge (:1591)
        ek, ei, kind = [], [], []
        for k in np.nonzero(ent)[0]:
            for kd in (1, 2):                                                # the parallel list, then the perpendicular list
                ii = np.nonzero((rel[k] == kd) & valid)[0]
                ek += [k] * len(ii); ei += ii.tolist(); kind += [kd] * len(ii)
        self.ek = np.array(ek, np.int64); self.ei = np.array(ei, np.int64); self.kind = np.array(kind, np.int64)
        self.E = len(ek)
        self.m = q[self.ei] if self.E else np.zeros((0, 3))
        self.nm = ops.sqrt((self.m[:, 0] * self.m[:, 0] + self.m[:, 1] * self.m[:, 1]) + self.m[:, 2] * self.m[:, 2])
        self.P0 = np.concatenate([A, B], axis=1)

    def err(self, P):
        m, k = self.m, self.ek
        with np.errstate(all="ignore"):
            l0, l1, l2 = P[k, 3] - P[k, 0], P[k, 4] - P[k, 1], P[k, 5] - P[k, 2]
            dot = (m[:, 0] * l0 + m[:, 1] * l1) + m[:, 2] * l2
            nl = self.ops.sqrt((l0 * l0 + l1 * l1) + l2 * l2)
            c = np.abs(dot / (self.nm * nl))
        return np.where(self.kind == 1, 1 - c, c)

    def line_sums(self, rows, active):
        """per line: the sum of rows over the line's active edges -> (n x columns)"""
        out = np.zeros((self.n, rows.shape[1]))
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            return out
        ks = self.ek[idx]
        for k in np.unique(ks):
            s = idx[ks == k]
            out[k] = self.ops.sum_edges_of_line(rows[s], self.ei[s])
        return out


def line_opt_struct(rel, A, B, line_eq, params=None, ops=None):
    """Optimizer::LineOptStruct on the lists held in rel (values 0, +-1, +-2) -> Result: rel (rejections marked), lines (n x 6: A, B after the
    call), the counters of hvo_line_opt_result, and for `accepted`: round_chi2 (per round the chi2 of every edge as the classification read
    it), final_chi2"""
    p = params or default_params(); ops = ops or Ops()
    G = _Graph(rel, A, B, line_eq, p, ops)
    n, E = G.n, G.E
    R = Result()
    R.rel = np.array(rel, np.int8).reshape(n, n).copy()
    R.n_lines = n; R.n_lines_to_opt = int(G.entered.sum()); R.n_edges = E
    R.n_par_edges = int((G.kind == 1).sum()); R.n_perp_edges = int((G.kind == 2).sum())
    R.iterations = [0, 0]; R.trials = [0, 0]; R.lam = [0.0, 0.0]; R.chi2 = [0.0, 0.0]; R.n_flagged = [0, 0]; R.rounds = 0
    R.round_chi2 = []; R.final_chi2 = np.zeros(E); R.graph = G
    est = G.P0.copy(); last = est.copy()
    level1 = np.zeros(E, bool)
    delta = p["huber_delta"]
    for rnd in range(2):
        active = ~level1
        act_line = np.zeros(n, bool); act_line[G.ek[active]] = True
        lam = 0.0; ni = 2.0; nbad = 0; its = 0; trials = 0; chi_final = 0.0

        def chi_of(P):
            e = G.err(P); r0, _ = huber_v(e * e, delta)
            if ops.order == "seq":
                return float(np.cumsum(r0[active])[-1]) if active.any() else 0.0
            return ops.sum_lines(G.line_sums(r0[:, None], active)[:, 0])

        if act_line.any():
            for it in range(p["iterations"]):
                e0 = G.err(est); r0, r1 = huber_v(e0 * e0, delta)
                J = np.zeros((E, 6))
                for d in range(6):
                    Pp = est.copy(); Pp[:, d] = est[:, d] + DELTA
                    Pm = est.copy(); Pm[:, d] = est[:, d] - DELTA
                    J[:, d] = (1.0 / (2 * DELTA)) * (G.err(Pp) - G.err(Pm))
                cols = []
                for a in range(6):
                    for b in range(a, 6): cols.append(J[:, a] * r1 * J[:, b])
                for a in range(6): cols.append(-(r1 * (J[:, a] * e0)))
                cols.append(r0)
                S = G.line_sums(np.stack(cols, axis=1), active)
                H = np.zeros((n, 6, 6)); h = 0
                for a in range(6):
                    for b in range(a, 6): H[:, a, b] = S[:, h]; H[:, b, a] = S[:, h]; h += 1
                bv = S[:, 21:27]
                cur = float(np.cumsum(r0[active])[-1]) if ops.order == "seq" else ops.sum_lines(S[:, 27])
                ini = cur
                if it == 0:
                    lam = 1e-5 * float(np.abs(H[act_line][:, np.arange(6), np.arange(6)]).max()); ni = 2.0; nbad = 0
                rho = 0.0; q = 0
                while True:
                    Hl = H[act_line].copy(); Hl[:, np.arange(6), np.arange(6)] = Hl[:, np.arange(6), np.arange(6)] + lam
                    x = np.zeros((n, 6)); xa, ok = ldlt_blocks(Hl, bv[act_line]); x[act_line] = xa
                    fail = not ok.all()
                    if fail: x[:] = 0.0
                    trial = est.copy(); trial[act_line] = est[act_line] + x[act_line]
                    with np.errstate(all="ignore"):
                        if ops.order == "seq":
                            scale = 0.0
                            for k in np.nonzero(act_line)[0]:
                                for j in range(6): scale += x[k, j] * (lam * x[k, j] + bv[k, j])
                        else:
                            sc = np.zeros(n)
                            for j in range(6): sc = sc + x[:, j] * (lam * x[:, j] + bv[:, j])
                            sc[~act_line] = 0.0
                            scale = ops.sum_lines(sc)
                        tmp = chi_of(trial); last = trial; trials += 1
                        if fail: tmp = DBL_MAX
                        scale += 1e-3
                        rho = (cur - tmp) / scale
                    if rho > 0 and np.isfinite(tmp):
                        alpha = 1.0 - ops.pow3(2 * rho - 1)
                        alpha = min(alpha, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha); ni = 2.0; cur = tmp; est = trial
                    else:
                        lam *= ni; ni *= 2
                    q += 1
                    if not (rho < 0 and q < 10): break
                its += 1; chi_final = cur
                if q == 10 or rho == 0: break
                if (ini - cur) * 1e3 < ini: nbad += 1
                else: nbad = 0
                if nbad >= 3: break
        R.iterations[rnd] = its; R.trials[rnd] = trials; R.lam[rnd] = lam if its else 0.0; R.chi2[rnd] = chi_final; R.rounds = rnd + 1
        # classification: a flagged edge is recomputed at the estimate, the others hold the last trial's error
        e = np.where(level1, G.err(est), G.err(last))
        chi = e * e
        R.round_chi2.append(chi.copy()); R.final_chi2 = chi
        with np.errstate(invalid="ignore"):
            level1 = chi.astype(F32) > p["chi2_round"][rnd]
        R.n_flagged[rnd] = int(level1.sum())
        if E < 10: break
    with np.errstate(invalid="ignore"):
        good = (R.final_chi2 >= 0.0) & (R.final_chi2 <= p["chi2_reject"])
    R.rel[G.ek[~good], G.ei[~good]] = -G.kind[~good]
    R.written_back = int(n > 0 and bool(G.entered[0]))
    R.lines = G.P0.copy()
    if R.written_back: R.lines[G.entered] = est[G.entered]
    R.est = est
    return R


def run_both(linefn, A, B, line_eq, params=None, ops=None):
    p = params or default_params()
    return line_opt_struct(struct_constraints(linefn, line_eq, p), A, B, line_eq, p, ops)


# ---------------------------------------------------------------- scenes
CAM = (535.4, 539.2, 320.1, 247.6)


def rot_vec(w):
    th = np.linalg.norm(w)
    if th < 1e-12: return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def make_scene(seed, n_lines=200, clutter=0.15, noise_deg=1.0, invalid=0.06, corrupt=0.0, cam=CAM):
    """a box room seen from inside: lines along three orthogonal axes plus oblique clutter, the direction of every line disturbed by
    noise_deg (as depth noise on the end points would), a share of invalid records ((-1,-1,-1), zero end points, c == 0 line functions).
    corrupt > 0: that share of the list entries of the returned rel are wrong on purpose (kinds swapped, entries between unrelated lines
    added), for part 2 alone.  -> dict(linefn, A, B, line_eq, rel)"""
    rng = np.random.RandomState(seed)
    Rw = rot_vec(rng.uniform(-0.4, 0.4, 3))
    A = np.zeros((n_lines, 3)); B = np.zeros((n_lines, 3))
    for i in range(n_lines):
        if rng.rand() < clutter:
            d = rng.normal(size=3); d /= np.linalg.norm(d)
        else:
            d = Rw[:, rng.randint(3)] * (1 if rng.rand() < 0.5 else -1)
        d = rot_vec(np.deg2rad(noise_deg) * rng.normal(size=3)) @ d
        c = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(2.0, 5.0)])
        half = rng.uniform(0.15, 0.6)
        A[i] = c - half * d; B[i] = c + half * d
    fx, fy, cx, cy = cam
    pa = np.stack([A[:, 0] / A[:, 2] * fx + cx, A[:, 1] / A[:, 2] * fy + cy, np.ones(n_lines)], axis=1)
    pb = np.stack([B[:, 0] / B[:, 2] * fx + cx, B[:, 1] / B[:, 2] * fy + cy, np.ones(n_lines)], axis=1)
    le = np.cross(pa, pb); linefn = le / np.sqrt(le[:, 0] ** 2 + le[:, 1] ** 2)[:, None]
    d = B - A; line_eq = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)
    for i in np.nonzero(rng.rand(n_lines) < invalid)[0]:
        kind = rng.randint(4)
        if kind == 0: line_eq[i] = -1.0; A[i] = 0.0; B[i] = 0.0               # no 3-D line was fitted
        elif kind == 1: line_eq[i, 2] = 0.0                                   # a direction in the image plane
        elif kind == 2: linefn[i, 2] = 0.0                                    # a key line through the origin: a / 0
        else: A[i] = 0.0; B[i] = 0.0                                          # zero end points under a set mvLineEq
    S = dict(linefn=linefn, A=A, B=B, line_eq=line_eq, seed=seed)
    rel = struct_constraints(linefn, line_eq)
    if corrupt > 0:
        k, i = np.nonzero(rel)
        s = rng.rand(len(k)) < corrupt
        rel[k[s], i[s]] = 3 - rel[k[s], i[s]]                                 # parallel <-> perpendicular
        z = (rel == 0) & (rng.rand(n_lines, n_lines) < 0.3 * corrupt)
        z[np.arange(n_lines), np.arange(n_lines)] = False
        rel[z] = rng.randint(1, 3, size=int(z.sum())).astype(np.int8)
    S["rel"] = rel
    return S


def run_scene(S, ops=None, params=None):
    return line_opt_struct(S["rel"], S["A"], S["B"], S["line_eq"], params, ops)


BAND = 0.02     # a scene is accepted when no edge's chi2 lies within +-2 % of a threshold at any classification or at the final rejection


def accepted(R, params=None, band=BAND):
    p = params or default_params()
    with np.errstate(invalid="ignore"):
        for rnd, chi in enumerate(R.round_chi2):
            t = float(p["chi2_round"][rnd])
            if np.any(np.abs(chi - t) <= band * t) or np.any(~np.isfinite(chi)):
                return False
        t = p["chi2_reject"]
        if np.any(np.abs(R.final_chi2 - t) <= band * t):
            return False
    return True


def accepted_scenes(count, seed0=2000, **kw):
    """(scenes, generated): (scene, Result) in seed order that pass `accepted`; more than half of the generated scenes rejected is an error"""
    out, gen, s = [], 0, seed0
    while len(out) < count:
        S = make_scene(s, **kw); s += 1; gen += 1
        R = run_scene(S)
        if accepted(R): out.append((S, R))
        assert gen <= 2 * max(len(out), 2) + 2 and gen < 200, "more than half of the generated scenes rejected"
    return out, gen


def directions(lines):
    d = lines[:, 3:6] - lines[:, 0:3]
    with np.errstate(all="ignore"):
        return d / np.linalg.norm(d, axis=1)[:, None]


def measured_D(scenes, seed=7):
    """D of tests/test_line_opt_gpu.py: the largest difference of any end-point coordinate between the restatement with g2o's edge-order
    sums and numpy's libm, and with the kernel's tree order and every sqrt / pow result moved by one ulp in a pseudo-random direction"""
    D = 0.0
    for S, R in scenes:
        b = run_scene(S, Ops("tree", seed))
        D = max(D, float(np.abs(R.lines - b.lines).max()))
    return D


def to_records(S, line3d_dt):
    l3 = np.zeros(len(S["A"]), line3d_dt)
    l3["A"] = S["A"]; l3["B"] = S["B"]; l3["line_eq"] = S["line_eq"]
    return l3


# ---------------------------------------------------------------- crafted problems (known answers, tests/test_line_opt.py)
TILT = rot_vec(np.array([0.3, -0.2, 0.1]))


def crafted(dirs, partners=(), mids=None):
    """lines of unit length along TILT dirs through (i / 4, 0, 3) (or mids), mvLineEq = the float direction; rel from partners: (k, i, kind)
    entries.  The fixed tilt keeps axis directions away from z == 0, which would make a partner invalid (Optimizer.cc:1591)."""
    dirs = np.asarray(dirs, np.float64) @ TILT.T; n = len(dirs)
    mid = np.stack([np.arange(n) * 0.25, np.zeros(n), np.full(n, 3.0)], axis=1) if mids is None else np.asarray(mids, np.float64)
    A = mid - 0.5 * dirs; B = mid + 0.5 * dirs
    rel = np.zeros((n, n), np.int8)
    for k, i, kind in partners: rel[k, i] = kind
    return dict(A=A, B=B, line_eq=dirs.astype(F32), rel=rel, linefn=np.tile([0.0, 1.0, 1.0], (n, 1)))


def crafted_families(seed=5, nx=8, ny=8, start_deg=2.0, meas_deg=0.3, line0=True):
    """two families along X and Y: mvLineEq (the measurements) within meas_deg of the axis, the end points start_deg off; every line is
    parallel to its family and perpendicular to the other.  line0 False: row 0 is emptied, so line 0 gets no vertices."""
    rng = np.random.RandomState(seed)
    axes = [np.array([1.0, 0, 0])] * nx + [np.array([0, 1.0, 0])] * ny
    n = nx + ny
    meas = np.array([rot_vec(np.deg2rad(meas_deg) * rng.normal(size=3)) @ a for a in axes])
    start = np.array([rot_vec(np.deg2rad(start_deg) * rng.normal(size=3)) @ a for a in axes])
    S = crafted(start, [(k, i, 1 if (k < nx) == (i < nx) else 2) for k in range(n) for i in range(n) if i != k])
    S["line_eq"] = (meas @ TILT.T).astype(F32); S["axes"] = np.array(axes) @ TILT.T
    if not line0: S["rel"][0, :] = 0
    return S
