// pnp_core.inc -- EPnP and CheckInliers of PnPsolver (reference src/PnPsolver.cc:308-339 and :375-950) as one text for three callers:
// the hypothesis kernel (G = 16 lanes of a wave work on one hypothesis), the refine kernel (G = 256, one workgroup) and the plain
// single-thread host restatement tools/pnp_host.cpp (G = 1).  csrc/pnp.hip includes it with PNP_HD = __device__ and PNP_SYNC = __syncthreads(); the host tool with both empty.
//
// The rules that make the three produce the same bits (tests/pnp_ref.py restates them a fourth time, in numpy):
//   * only + - * / sqrt on doubles (floats in CheckInliers), no contraction (-ffp-contract=off), every sum in a written order;
//   * a sum over the rows of a correspondence matrix (rows = correspondences; for MtM, the 2 n rows of M) is `0 + r0 + r1 + ...` in
//     ascending row order for up to PNP_SEQ_ROWS rows.  Above that it is one fixed tree: 256 partial sums, partial t = rows t, t + 256, ...
//     in ascending order; each run of 64 partials is halved (l += l + 32, + 16, ... + 1); the four run totals are added in order;
//   * cvSVD of a symmetric matrix (3 x 3 and 12 x 12) is a cyclic two-sided Jacobi eigen-iteration: pairs (p, q) in row-major order,
//     PNP_EIG_SWEEPS sweeps, never fewer (the stopping rule is the count); an off-diagonal element that is exactly zero gives the identity
//     rotation (c = 1, s = 0), applied through the same formulas.  Eigenpairs leave in descending eigenvalue, ties by index; the
//     singular value is |eigenvalue|;
//   * cvSVD of the 3 x 3 ABt, cvInvert(CV_SVD) and cvSolve(CV_SVD) (6 x 4, 6 x 3, 6 x 5) are one-sided (Hestenes) Jacobi on the columns,
//     PNP_SVD_SWEEPS sweeps, pairs in row-major order; a singular value at or below 2 DBL_EPSILON (sum of the singular values) is cut
//     (its term of the pseudo-inverse is zero, its left vector is zero), so coplanar points take the pseudo-inverse, not a division by 0;
//   * qr_solve as written (the pivot scan looks at rows k .. nr-2); where it returns early on a zero column the step is zero.
// Nothing here indexes a private array with a run-time index: every array lives in the workspace (LDS on the device).
#ifndef PNP_HD
#define PNP_HD
#endif
#ifndef PNP_SYNC
#define PNP_SYNC() ((void)0)
#endif

#define PNP_SEQ_ROWS 64
#define PNP_EIG_SWEEPS 12
#define PNP_SVD_SWEEPS 12
#define PNP_TREE_BATCH 8           // sums that go through the tree together (PNP_TREE_BATCH x 256 doubles of workspace)

struct PnpCorr {                   // correspondence i of the problem at hand is entry (sel ? sel[i] : i) of the candidate's arrays
    const float *p3d, *p2d; const int *sel; int n;
    double fu, fv, uc, vc;
};

struct PnpBetaWs {                 // what one of the three beta approximations needs (one lane each)
    double W[36], Vh[25], s2[5], x[5], rhs[6];
    double ga[24], gb[6], gx[4], A1[4], A2[4];
    double betas[4], ccs[12], pc0[3], abt[9], R[9], t[3], rep;
};

struct PnpWs {
    double A[144], V[144], Ut[144], d[12];
    double red[80];
    double c0[3], cws[12], ci[9], L[60], rho[6];
    PnpBetaWs bt[3];
    double R[9], t[3];
    int cnt[256];
};

static PNP_HD inline double pnp_pw(const PnpCorr &c, int i, int k) { const int id = c.sel ? c.sel[i] : i; return (double)c.p3d[3 * id + k]; }
static PNP_HD inline double pnp_us(const PnpCorr &c, int i, int k) { const int id = c.sel ? c.sel[i] : i; return (double)c.p2d[2 * id + k]; }

// compute_barycentric_coordinates' inner part (:423-433)
static PNP_HD inline void pnp_alphas(const PnpCorr &c, const PnpWs *w, int i, double a[4])
{
    const double d0 = pnp_pw(c, i, 0) - w->c0[0], d1 = pnp_pw(c, i, 1) - w->c0[1], d2 = pnp_pw(c, i, 2) - w->c0[2];
    a[1] = w->ci[0] * d0 + w->ci[1] * d1 + w->ci[2] * d2;
    a[2] = w->ci[3] * d0 + w->ci[4] * d1 + w->ci[5] * d2;
    a[3] = w->ci[6] * d0 + w->ci[7] * d1 + w->ci[8] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];                            // a[0] = 1.0f - ... (:432): the float constant widens exactly
}
// compute_pcs (:466-475) for one correspondence and one coordinate
static PNP_HD inline double pnp_pc(const double a[4], const double *ccs, int j) { return a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j]; }

// The terms of the sums over rows.  kind 0: pws (3); 1: PW0tPW0 upper (6); 2: MtM upper (78, rows of M); 3: pcs of the three betas (9);
// 4: ABt of the three betas (27); 5: the reprojection error of the three betas (3)
static PNP_HD inline double pnp_term(const PnpCorr &c, const PnpWs *w, int kind, int r, int k)
{
    if (kind == 0) return pnp_pw(c, r, k);
    if (kind == 1) {
        const int a = k < 3 ? 0 : (k < 5 ? 1 : 2), b = k < 3 ? k : (k < 5 ? k - 2 : 2);
        return (pnp_pw(c, r, a) - w->c0[a]) * (pnp_pw(c, r, b) - w->c0[b]);
    }
    if (kind == 2) {                                            // fill_M (:436-451) and one row's product of cvMulTransposed (:492)
        int a = 0, kk = k;
        while (kk >= 12 - a) { kk -= 12 - a; a++; }
        const int b = a + kk, i = r >> 1, row = r & 1;
        double al[4]; pnp_alphas(c, w, i, al);
        const double u = pnp_us(c, i, row);
        const double f = row ? c.fv : c.fu, cc = row ? c.vc : c.uc;
        const int ai = a / 3, ac = a - 3 * ai, bi = b / 3, bc = b - 3 * bi;
        const double aa = ai == 0 ? al[0] : (ai == 1 ? al[1] : (ai == 2 ? al[2] : al[3]));
        const double ab = bi == 0 ? al[0] : (bi == 1 ? al[1] : (bi == 2 ? al[2] : al[3]));
        const double ea = ac == 2 ? aa * (cc - u) : (ac == row ? aa * f : 0.0);
        const double eb = bc == 2 ? ab * (cc - u) : (bc == row ? ab * f : 0.0);
        return ea * eb;
    }
    double al[4]; pnp_alphas(c, w, r, al);
    if (kind == 3) { const int b = k / 3, j = k - 3 * b; return pnp_pc(al, w->bt[b].ccs, j); }
    if (kind == 4) {                                            // estimate_R_and_t's ABt (:597-606)
        const int b = k / 9, j = (k - 9 * b) / 3, m = k - 9 * b - 3 * j;
        return (pnp_pc(al, w->bt[b].ccs, j) - w->bt[b].pc0[j]) * (pnp_pw(c, r, m) - w->c0[m]);
    }
    const PnpBetaWs *B = &w->bt[k];                             // reprojection_error (:550-567)
    const double p0 = pnp_pw(c, r, 0), p1 = pnp_pw(c, r, 1), p2 = pnp_pw(c, r, 2);
    const double Xc = B->R[0] * p0 + B->R[1] * p1 + B->R[2] * p2 + B->t[0];
    const double Yc = B->R[3] * p0 + B->R[4] * p1 + B->R[5] * p2 + B->t[1];
    const double inv_Zc = 1.0 / (B->R[6] * p0 + B->R[7] * p1 + B->R[8] * p2 + B->t[2]);
    const double ue = c.uc + c.fu * Xc * inv_Zc, ve = c.vc + c.fv * Yc * inv_Zc;
    const double u = pnp_us(c, r, 0), v = pnp_us(c, r, 1);
    return sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}

// w->red[k] = the sum over rows 0 .. nr-1 of term(kind, r, k), k < K, by the rule at the top.  tbuf: PNP_TREE_BATCH x 256 doubles (used when nr > 64)
template <int G> static PNP_HD inline void pnp_reduce(const PnpCorr &c, PnpWs *w, double *tbuf, int lane, int kind, int nr, int K)
{
    if (nr <= PNP_SEQ_ROWS) {
        for (int k = lane; k < K; k += G) {
            double s = 0.0;
            for (int r = 0; r < nr; r++) s += pnp_term(c, w, kind, r, k);
            w->red[k] = s;
        }
        PNP_SYNC();
        return;
    }
    for (int k0 = 0; k0 < K; k0 += PNP_TREE_BATCH) {
        const int kb = K - k0 < PNP_TREE_BATCH ? K - k0 : PNP_TREE_BATCH;
        for (int x = lane; x < kb * 256; x += G) {
            const int kk = x >> 8, t = x & 255;
            double s = 0.0;
            for (int r = t; r < nr; r += 256) s += pnp_term(c, w, kind, r, k0 + kk);
            tbuf[x] = s;
        }
        PNP_SYNC();
        for (int off = 32; off > 0; off >>= 1) {
            for (int x = lane; x < kb * 4 * off; x += G) {
                const int kk = x / (4 * off), y = x - kk * 4 * off, wv = y / off, l = y - wv * off;
                double *p = tbuf + kk * 256 + wv * 64 + l;
                p[0] = p[0] + p[off];
            }
            PNP_SYNC();
        }
        for (int kk = lane; kk < kb; kk += G) { const double *p = tbuf + kk * 256; w->red[k0 + kk] = ((p[0] + p[64]) + p[128]) + p[192]; }
        PNP_SYNC();
    }
}

static PNP_HD inline void pnp_rot(double num, double den2, double *c, double *s, double *t)
{
    // the rotation that zeroes the pair: theta = num / den2 (den2 = twice the off-diagonal term), t = sign(theta) / (|theta| + sqrt(theta^2 + 1))
    if (den2 * 0.5 == 0.0) { *c = 1.0; *s = 0.0; *t = 0.0; return; }
    const double th = num / den2;
    const double at = th < 0.0 ? -th : th;
    double tt = 1.0 / (at + sqrt(th * th + 1.0));
    if (th < 0.0) tt = -tt;
    const double cc = 1.0 / sqrt(tt * tt + 1.0);
    *c = cc; *s = tt * cc; *t = tt;
}

// cvSVD(A symmetric n x n, D, Ut, CV_SVD_U_T): w->A (row-major, stride n) is destroyed, w->d gets the n values, w->Ut the vectors as rows
template <int G> static PNP_HD inline void pnp_eig(PnpWs *w, int n, int lane)
{
    for (int x = lane; x < n * n; x += G) w->V[x] = (x / n == x % n) ? 1.0 : 0.0;
    PNP_SYNC();
    for (int sw = 0; sw < PNP_EIG_SWEEPS; sw++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                const double app = w->A[p * n + p], aqq = w->A[q * n + q], apq = w->A[p * n + q];
                PNP_SYNC();
                double c, s, t; pnp_rot(aqq - app, 2.0 * apq, &c, &s, &t);
                for (int k = lane; k < n; k += G) {
                    if (k == p) { w->A[p * n + p] = app - t * apq; w->A[p * n + q] = 0.0; }
                    else if (k == q) { w->A[q * n + q] = aqq + t * apq; w->A[q * n + p] = 0.0; }
                    else {
                        const double akp = w->A[k * n + p], akq = w->A[k * n + q];
                        const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                        w->A[k * n + p] = np_; w->A[p * n + k] = np_; w->A[k * n + q] = nq_; w->A[q * n + k] = nq_;
                    }
                    const double vkp = w->V[k * n + p], vkq = w->V[k * n + q];
                    w->V[k * n + p] = c * vkp - s * vkq; w->V[k * n + q] = s * vkp + c * vkq;
                }
                PNP_SYNC();
            }
    for (int i = lane; i < n; i += G) {                          // descending eigenvalue, ties by index
        const double di = w->A[i * n + i];
        int rank = 0;
        for (int j = 0; j < n; j++) { const double dj = w->A[j * n + j]; if (dj > di || (dj == di && j < i)) rank++; }
        w->d[rank] = di < 0.0 ? -di : di;
        for (int k = 0; k < n; k++) w->Ut[rank * n + k] = w->V[k * n + i];
    }
    PNP_SYNC();
}

// one-sided Jacobi on the columns of B->W (m x n, row-major, stride n); B->Vh (n x n) collects the rotations, B->s2 the squared column norms
static PNP_HD inline void pnp_hestenes(PnpBetaWs *B, int m, int n)
{
    for (int x = 0; x < n * n; x++) B->Vh[x] = (x / n == x % n) ? 1.0 : 0.0;
    for (int sw = 0; sw < PNP_SVD_SWEEPS; sw++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int i = 0; i < m; i++) { const double wp = B->W[i * n + p], wq = B->W[i * n + q]; al += wp * wp; be += wq * wq; ga += wp * wq; }
                double c, s, t; pnp_rot(be - al, 2.0 * ga, &c, &s, &t);
                for (int i = 0; i < m; i++) { const double wp = B->W[i * n + p], wq = B->W[i * n + q]; B->W[i * n + p] = c * wp - s * wq; B->W[i * n + q] = s * wp + c * wq; }
                for (int i = 0; i < n; i++) { const double vp = B->Vh[i * n + p], vq = B->Vh[i * n + q]; B->Vh[i * n + p] = c * vp - s * vq; B->Vh[i * n + q] = s * vp + c * vq; }
            }
    double tot = 0.0;
    for (int j = 0; j < n; j++) { double s2 = 0.0; for (int i = 0; i < m; i++) s2 += B->W[i * n + j] * B->W[i * n + j]; B->s2[j] = s2; tot += sqrt(s2); }
    const double cut = 2.0 * 2.220446049250313e-16 * tot;
    for (int j = 0; j < n; j++) if (!(sqrt(B->s2[j]) > cut)) B->s2[j] = 0.0;      // cut (a NaN norm is cut too)
}
// x = pinv(W0) rhs after pnp_hestenes: sum over the kept columns j of Vh[:, j] (W[:, j] . rhs) / s2[j]
static PNP_HD inline void pnp_svd_backsub(PnpBetaWs *B, int m, int n)
{
    for (int i = 0; i < n; i++) B->x[i] = 0.0;
    for (int j = 0; j < n; j++) {
        if (B->s2[j] == 0.0) continue;
        double dt = 0.0;
        for (int i = 0; i < m; i++) dt += B->W[i * n + j] * B->rhs[i];
        const double cf = dt / B->s2[j];
        for (int i = 0; i < n; i++) B->x[i] += B->Vh[i * n + j] * cf;
    }
}

// qr_solve (:860-950) on B->ga (6 x 4), B->gb -> B->gx
static PNP_HD inline void pnp_qr_solve(PnpBetaWs *B)
{
    const int nr = 6, nc = 4;
    double *A = B->ga, *b = B->gb, *X = B->gx;
    for (int i = 0; i < nc; i++) X[i] = 0.0;
    for (int k = 0; k < nc; k++) {
        double eta = A[k * nc + k]; eta = eta < 0.0 ? -eta : eta;
        for (int i = k + 1; i < nr; i++) { double elt = A[(i - 1) * nc + k]; elt = elt < 0.0 ? -elt : elt; if (eta < elt) eta = elt; }   // rows k .. nr-2, as written
        if (eta == 0.0) return;                                  // the reference leaves X stale here; the step is zero
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < nr; i++) { A[i * nc + k] *= inv_eta; sum += A[i * nc + k] * A[i * nc + k]; }
        double sigma = sqrt(sum);
        if (A[k * nc + k] < 0.0) sigma = -sigma;
        A[k * nc + k] += sigma;
        B->A1[k] = sigma * A[k * nc + k];
        B->A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double sm = 0.0;
            for (int i = k; i < nr; i++) sm += A[i * nc + k] * A[i * nc + j];
            const double tau = sm / B->A1[k];
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {
        double tau = 0.0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= B->A1[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / B->A2[nc - 1];
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0.0;
        for (int j = i + 1; j < nc; j++) sum += A[i * nc + j] * X[j];
        X[i] = (b[i] - sum) / B->A2[i];
    }
}

// find_betas_approx_{1,2,3} (:667-758), gauss_newton (:812-858), compute_ccs (:453-464) and solve_for_sign (:636-649) of approximation b
static PNP_HD inline void pnp_beta(const PnpCorr &c, PnpWs *w, int b)
{
    PnpBetaWs *B = &w->bt[b];
    const int n = b == 0 ? 4 : (b == 1 ? 3 : 5);
    for (int i = 0; i < 6; i++) {
        for (int j = 0; j < n; j++) { const int col = b == 0 ? (j == 0 ? 0 : (j == 1 ? 1 : (j == 2 ? 3 : 6))) : j; B->W[i * n + j] = w->L[10 * i + col]; }
        B->rhs[i] = w->rho[i];
    }
    pnp_hestenes(B, 6, n);
    pnp_svd_backsub(B, 6, n);
    double *be = B->betas; const double *x = B->x;
    if (b == 0) {
        if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = -x[1] / be[0]; be[2] = -x[2] / be[0]; be[3] = -x[3] / be[0]; }
        else { be[0] = sqrt(x[0]); be[1] = x[1] / be[0]; be[2] = x[2] / be[0]; be[3] = x[3] / be[0]; }
    } else {
        if (x[0] < 0) { be[0] = sqrt(-x[0]); be[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0; }
        else { be[0] = sqrt(x[0]); be[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0; }
        if (x[1] < 0) be[0] = -be[0];
        be[2] = b == 1 ? 0.0 : x[3] / be[0];
        be[3] = 0.0;
    }
    for (int it = 0; it < 5; it++) {
        for (int i = 0; i < 6; i++) {
            const double *rl = w->L + 10 * i; double *ra = B->ga + 4 * i;
            ra[0] = 2 * rl[0] * be[0] + rl[1] * be[1] + rl[3] * be[2] + rl[6] * be[3];
            ra[1] = rl[1] * be[0] + 2 * rl[2] * be[1] + rl[4] * be[2] + rl[7] * be[3];
            ra[2] = rl[3] * be[0] + rl[4] * be[1] + 2 * rl[5] * be[2] + rl[8] * be[3];
            ra[3] = rl[6] * be[0] + rl[7] * be[1] + rl[8] * be[2] + 2 * rl[9] * be[3];
            B->gb[i] = w->rho[i] - (rl[0] * be[0] * be[0] + rl[1] * be[0] * be[1] + rl[2] * be[1] * be[1] + rl[3] * be[0] * be[2] + rl[4] * be[1] * be[2] +
                                    rl[5] * be[2] * be[2] + rl[6] * be[0] * be[3] + rl[7] * be[1] * be[3] + rl[8] * be[2] * be[3] + rl[9] * be[3] * be[3]);
        }
        pnp_qr_solve(B);
        for (int i = 0; i < 4; i++) be[i] += B->gx[i];
    }
    for (int i = 0; i < 12; i++) B->ccs[i] = 0.0;
    for (int i = 0; i < 4; i++) { const double *v = w->Ut + 12 * (11 - i); for (int j = 0; j < 12; j++) B->ccs[j] += be[i] * v[j]; }
    double al[4]; pnp_alphas(c, w, 0, al);
    if (pnp_pc(al, B->ccs, 2) < 0.0) for (int i = 0; i < 12; i++) B->ccs[i] = -B->ccs[i];
}

// estimate_R_and_t after the sums (:608-626)
static PNP_HD inline void pnp_rt(PnpWs *w, int b)
{
    PnpBetaWs *B = &w->bt[b];
    for (int i = 0; i < 9; i++) B->W[i] = B->abt[i];
    pnp_hestenes(B, 3, 3);
    for (int j = 0; j < 3; j++) {                                // U[:, j] = W[:, j] / sigma_j, zero when cut
        const double sg = sqrt(B->s2[j]);
        for (int i = 0; i < 3; i++) B->W[i * 3 + j] = B->s2[j] == 0.0 ? 0.0 : B->W[i * 3 + j] / sg;
    }
    double *R = B->R;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = B->W[3 * i] * B->Vh[3 * j] + B->W[3 * i + 1] * B->Vh[3 * j + 1] + B->W[3 * i + 2] * B->Vh[3 * j + 2];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int i = 0; i < 3; i++) B->t[i] = B->pc0[i] - (R[3 * i] * w->c0[0] + R[3 * i + 1] * w->c0[1] + R[3 * i + 2] * w->c0[2]);
}

// compute_pose (:477-525): w->R, w->t.  Every lane of the group calls it with the same arguments.
template <int G> static PNP_HD inline void pnp_epnp(const PnpCorr &c, PnpWs *w, double *tbuf, int lane)
{
    const int n = c.n;
    // choose_control_points (:375-409)
    pnp_reduce<G>(c, w, tbuf, lane, 0, n, 3);
    if (lane == 0) for (int j = 0; j < 3; j++) w->c0[j] = w->red[j] / n;
    PNP_SYNC();
    pnp_reduce<G>(c, w, tbuf, lane, 1, n, 6);
    if (lane == 0) {
        const double *r = w->red;
        w->A[0] = r[0]; w->A[1] = r[1]; w->A[2] = r[2]; w->A[3] = r[1]; w->A[4] = r[3]; w->A[5] = r[4]; w->A[6] = r[2]; w->A[7] = r[4]; w->A[8] = r[5];
    }
    PNP_SYNC();
    pnp_eig<G>(w, 3, lane);
    if (lane == 0) {
        for (int j = 0; j < 3; j++) w->cws[j] = w->c0[j];
        for (int i = 1; i < 4; i++) { const double k = sqrt(w->d[i - 1] / n); for (int j = 0; j < 3; j++) w->cws[3 * i + j] = w->c0[j] + k * w->Ut[3 * (i - 1) + j]; }
        // compute_barycentric_coordinates' cvInvert(CC, CC_inv, CV_SVD) (:417-421)
        PnpBetaWs *B = &w->bt[0];
        for (int i = 0; i < 3; i++) for (int j = 1; j < 4; j++) B->W[3 * i + j - 1] = w->cws[3 * j + i] - w->c0[i];
        pnp_hestenes(B, 3, 3);
        for (int col = 0; col < 3; col++) {
            for (int i = 0; i < 3; i++) B->rhs[i] = i == col ? 1.0 : 0.0;
            pnp_svd_backsub(B, 3, 3);
            for (int i = 0; i < 3; i++) w->ci[3 * i + col] = B->x[i];
        }
        // compute_rho (:802-810)
        int a = 0, b = 1;
        for (int i = 0; i < 6; i++) {
            const double *p1 = w->cws + 3 * a, *p2 = w->cws + 3 * b;
            w->rho[i] = (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
            b++; if (b > 3) { a++; b = a + 1; }
        }
    }
    PNP_SYNC();
    pnp_reduce<G>(c, w, tbuf, lane, 2, 2 * n, 78);
    for (int k = lane; k < 78; k += G) {
        int a = 0, kk = k;
        while (kk >= 12 - a) { kk -= 12 - a; a++; }
        const int b = a + kk;
        w->A[a * 12 + b] = w->red[k]; w->A[b * 12 + a] = w->red[k];
    }
    PNP_SYNC();
    pnp_eig<G>(w, 12, lane);
    // compute_L_6x10 (:760-800): row i on lane i
    for (int i = lane; i < 6; i += G) {
        const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
        double *row = w->L + 10 * i;
        int col = 0;
        for (int q = 0; q < 4; q++)
            for (int p = 0; p <= q; p++) {
                const double *vp = w->Ut + 12 * (11 - p), *vq = w->Ut + 12 * (11 - q);
                const double p0 = vp[3 * a] - vp[3 * b], p1 = vp[3 * a + 1] - vp[3 * b + 1], p2 = vp[3 * a + 2] - vp[3 * b + 2];
                const double q0 = vq[3 * a] - vq[3 * b], q1 = vq[3 * a + 1] - vq[3 * b + 1], q2 = vq[3 * a + 2] - vq[3 * b + 2];
                const double dt = p0 * q0 + p1 * q1 + p2 * q2;
                row[col++] = p == q ? dt : 2.0 * dt;               // [B11 B12 B22 B13 B23 B33 B14 B24 B34 B44]
            }
    }
    PNP_SYNC();
    for (int b = lane; b < 3; b += G) pnp_beta(c, w, b);
    PNP_SYNC();
    pnp_reduce<G>(c, w, tbuf, lane, 3, n, 9);
    for (int k = lane; k < 9; k += G) w->bt[k / 3].pc0[k % 3] = w->red[k] / n;
    PNP_SYNC();
    pnp_reduce<G>(c, w, tbuf, lane, 4, n, 27);
    for (int k = lane; k < 27; k += G) w->bt[k / 9].abt[k % 9] = w->red[k];
    PNP_SYNC();
    for (int b = lane; b < 3; b += G) pnp_rt(w, b);
    PNP_SYNC();
    pnp_reduce<G>(c, w, tbuf, lane, 5, n, 3);
    if (lane == 0) {
        const double e1 = w->red[0] / n, e2 = w->red[1] / n, e3 = w->red[2] / n;
        int N = 0; double eN = e1;
        if (e2 < e1) { N = 1; eN = e2; }
        if (e3 < eN) N = 2;
        for (int i = 0; i < 9; i++) w->R[i] = w->bt[N].R[i];
        for (int i = 0; i < 3; i++) w->t[i] = w->bt[N].t[i];
    }
    PNP_SYNC();
}

// CheckInliers (:308-339) of correspondence i of the candidate against w->R, w->t; the mix of float and double is the reference's
static PNP_HD inline int pnp_check_one(const PnpWs *w, const float *p3d, const float *p2d, const float *max_err, double fu, double fv, double uc, double vc, int i)
{
    const float X = p3d[3 * i], Y = p3d[3 * i + 1], Z = p3d[3 * i + 2];
    const float Xc = (float)(w->R[0] * X + w->R[1] * Y + w->R[2] * Z + w->t[0]);
    const float Yc = (float)(w->R[3] * X + w->R[4] * Y + w->R[5] * Z + w->t[1]);
    const float invZc = (float)(1 / (w->R[6] * X + w->R[7] * Y + w->R[8] * Z + w->t[2]));
    const double ue = uc + fu * Xc * invZc, ve = vc + fv * Yc * invZc;
    const float distX = (float)(p2d[2 * i] - ue), distY = (float)(p2d[2 * i + 1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err[i] ? 1 : 0;
}
static PNP_HD inline int pnp_pose_finite(const PnpWs *w)
{
    int ok = 1;
    for (int i = 0; i < 9; i++) { const double v = w->R[i] - w->R[i]; if (!(v == 0.0)) ok = 0; }
    for (int i = 0; i < 3; i++) { const double v = w->t[i] - w->t[i]; if (!(v == 0.0)) ok = 0; }
    return ok;
}
