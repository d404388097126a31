// Optimizer::LocalMapOptimization (reference src/Optimizer.cc:3014-3940): local bundle adjustment over the covisibility window.
//
// Formulation (tests/local_ba_ref.py is the definition): no edge joins two different lines, so a line's
// (start, end) pair is ONE 6-dimensional landmark beside the 3-dimensional points.  Every landmark block (plus lambda) is eliminated
// and the dense reduced system over the free key frames (6 x n_free <= 384) is factored by LDL^T without pivoting.
//
// Launches of one linearisation:  k_lba_poses (R, t of every key frame and of its 12 perturbed poses), k_lba_edges<true> (one thread per
// edge: error, robust weight, Jacobians -- analytic for the point edge, g2o's central differences with delta 1e-9 for the line edges),
// k_lba_pairs (one thread per (landmark, free key frame) pair: pose block, pose gradient, pose-landmark block), k_lba_build (one thread
// per landmark: its Hessian block and gradient), k_lba_diag (one wave per free key frame: its diagonal block), k_lba_sum (chi2, scale, largest diagonal).
// Launches of one trial:  k_lba_invert (landmark blocks + lambda inverted, Y = W Hll^-1), k_lba_reduce (one wave per key-frame pair:
// the reduced block, pairs walked observer-major in landmark order), k_lba_solve (one workgroup), k_lba_update (back-substitution and
// oplus into the trial state), k_lba_poses, k_lba_edges<false>, k_lba_sum.  Every sum has a fixed order: no atomics.
//
// chi2() of the erase tests is the error an edge HOLDS (reading 2): chi_held[e] is written by every evaluation of an ACTIVE edge and
// by nothing else, so a level-1 edge keeps round 1's last evaluation.  The classification and the flags are host code.
#include "hvo_internal.hpp"
#include "se3quat.hpp"        // quat_from_R .. se3_map, huber, wave_sum_down
#include <math.h>
#include <cmath>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>

#define LBA_DELTA 1e-9
#define LBA_THREADS 256

static_assert(sizeof(hvo_local_ba_params) == 88 && sizeof(hvo_local_ba_graph) == 208 && sizeof(hvo_local_ba_result) == 200, "the layouts the Python binding mirrors");

enum { LBA_PT = 0, LBA_START = 1, LBA_END = 2, LBA_MANH = 3, LBA_PAR = 4, LBA_PERP = 5 };

struct LbEdge { int kind, lm, kf, pair; double m[3], info, delta, cam[4]; };   // pair: -1 when the key frame is fixed or there is none
struct LbPair { int lm, f, e0, e1; };                                          // f: index among the free key frames

struct LbArgs {
    int n_kf, n_free, n_pts, n_lm, n_edges, n_pairs, n6, robust;
    // the graph (read only)
    const int *kf_free;             // n_kf: free index or -1
    const LbEdge *edge; const LbPair *pair;
    const int *lm_e0, *lm_p0;       // n_lm + 1
    const int *kf_p0, *kf_pairs;    // n_free + 1, n_pairs: a free key frame's pairs in landmark order
    const uint8_t *level;           // n_edges
    // the state: [pose n_kf x 8 | landmark n_lm x 6], estimate and trial
    double *est, *trial;
    double *Rt;                     // n_kf x 13 x 12
    // per edge
    double *Jl, *Jp, *ew, *rho, *chi_held;      // x 12, x 12, x 4 (e0 e1 rho' info), x 1, x 1
    // per pair
    double *A, *bp, *W, *Y; int *pair_act;      // x 36, x 6, x 36 (pose row, landmark column), x 36
    // per landmark
    double *Hll, *bl, *Hinv, *lm_maxd; int *lm_act;
    // per free key frame
    double *Hpp, *bfull, *kf_maxd; int *kf_act;
    // the reduced system
    double *S, *rhs, *dx;
    double *sc;                     // n_lm + n_free: the terms of computeScale
    double *out;                    // chi2, scale, ok, largest diagonal
};

// R, t of every key frame's pose (slot 0) and, with full != 0, of exp(+-delta e_d) * pose for the free ones (slots 1 + 2 d, 2 + 2 d)
__global__ __launch_bounds__(LBA_THREADS) void k_lba_poses(LbArgs a, int trial, int full)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int kf = t / 13, s = t % 13;
    if (kf >= a.n_kf) return;
    if (s > 0 && (!full || a.kf_free[kf] < 0)) return;
    const double *P = (trial ? a.trial : a.est) + (size_t)kf * 8;
    double p[7];
    if (s == 0) { for (int i = 0; i < 7; i++) p[i] = P[i]; }
    else {
        double u[6] = { 0, 0, 0, 0, 0, 0 };
        u[(s - 1) >> 1] = ((s - 1) & 1) ? -LBA_DELTA : LBA_DELTA;
        double e[7]; se3_exp(u, e);
        double b[7]; for (int i = 0; i < 7; i++) b[i] = P[i];
        se3_mul(e, b, p);
    }
    double *Rt = a.Rt + ((size_t)kf * 13 + s) * 12;
    double R[9]; quat_to_R(p, R);
    for (int i = 0; i < 9; i++) Rt[i] = R[i];
    Rt[9] = p[4]; Rt[10] = p[5]; Rt[11] = p[6];
}

// computeError of the five edge types: X holds the landmark (3 or 6 doubles), Rt the observer's pose; err[1] is 0 for the line edges
static __device__ __forceinline__ void lb_project(const double *Rt, const double *X, const double *cam, double *uv)
{
    double Y[3]; se3_map(Rt, X, Y);
    uv[0] = Y[0] / Y[2] * cam[0] + cam[2];
    uv[1] = Y[1] / Y[2] * cam[1] + cam[3];
}
static __device__ void lb_error(const LbEdge &E, const double *Rt, const double *X, double *err)
{
    err[1] = 0.0;
    if (E.kind == LBA_PT) {
        double uv[2]; lb_project(Rt, X, E.cam, uv);
        err[0] = E.m[0] - uv[0]; err[1] = E.m[1] - uv[1];
    } else if (E.kind == LBA_START || E.kind == LBA_END) {
        double uv[2]; lb_project(Rt, X + (E.kind == LBA_END ? 3 : 0), E.cam, uv);
        err[0] = (E.m[0] * uv[0] + E.m[1] * uv[1]) + E.m[2];                       // g2oMSC.h:576
    } else if (E.kind == LBA_MANH) {
        const double d[3] = { X[3] - X[0], X[4] - X[1], X[5] - X[2] };          // ComputeAngle3D(line_eq, axis), g2oMSC.h:25-34
        const double dot = (E.m[0] * d[0] + E.m[1] * d[1]) + E.m[2] * d[2];
        const double ma = sqrt((E.m[0] * E.m[0] + E.m[1] * E.m[1]) + E.m[2] * E.m[2]);
        const double mb = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        err[0] = 1 - fabs(dot / (ma * mb));
    } else {
        double ps[2], pe[2]; lb_project(Rt, X, E.cam, ps); lb_project(Rt, X + 3, E.cam, pe);
        const double lb[2] = { pe[0] - ps[0], pe[1] - ps[1] };                    // ComputeAngle2D(measurement, line_eq), g2oMSC.h:11-23
        const double la[2] = { E.m[0] / E.m[2], E.m[1] / E.m[2] };
        const double dot = lb[0] * la[0] + lb[1] * la[1];
        const double ma = sqrt(lb[0] * lb[0] + lb[1] * lb[1]);
        const double mb = sqrt(la[0] * la[0] + la[1] * la[1]);
        const double ang = fabs(dot / (ma * mb));
        err[0] = E.kind == LBA_PAR ? 1 - ang : ang;
    }
}

// one thread per edge.  LIN: the linearisation at the estimate; else the evaluation at the trial state
template <bool LIN>
__global__ __launch_bounds__(LBA_THREADS) void k_lba_edges(LbArgs a)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_edges) return;
    double *Jl = a.Jl + (size_t)e * 12, *Jp = a.Jp + (size_t)e * 12, *ew = a.ew + (size_t)e * 4;
    if (a.level[e]) {                                                           // not in the active set: nothing is evaluated
        a.rho[e] = 0.0;
        if (LIN) { for (int i = 0; i < 12; i++) { Jl[i] = 0.0; Jp[i] = 0.0; } ew[0] = ew[1] = ew[2] = ew[3] = 0.0; }
        return;
    }
    const LbEdge E = a.edge[e];
    const double *state = LIN ? a.est : a.trial;
    const double *Xp = state + (size_t)a.n_kf * 8 + (size_t)E.lm * 6;
    double X[6]; for (int i = 0; i < 6; i++) X[i] = Xp[i];
    const double *Rt = a.Rt + (size_t)(E.kf < 0 ? 0 : E.kf) * 13 * 12;
    double err[2]; lb_error(E, Rt, X, err);
    const double chi = E.info * err[0] * err[0] + E.info * err[1] * err[1];
    a.chi_held[e] = chi;
    double r0 = chi, r1 = 1.0;
    if (a.robust || E.kind == LBA_MANH) huber(chi, E.delta, r0, r1);            // the Manhattan edge keeps its kernel in round 2
    a.rho[e] = r0;
    if (!LIN) return;
    ew[0] = err[0]; ew[1] = err[1]; ew[2] = r1; ew[3] = E.info;
    for (int i = 0; i < 12; i++) { Jl[i] = 0.0; Jp[i] = 0.0; }
    const bool free_kf = E.pair >= 0;
    if (E.kind == LBA_PT) {                                                     // EdgeSE3ProjectXYZ::linearizeOplus
        double Y[3]; se3_map(Rt, X, Y);
        const double x = Y[0], y = Y[1], z = Y[2], z_2 = z * z, fx = E.cam[0], fy = E.cam[1];
        const double c = -1. / z;
        const double t0[3] = { c * fx, c * 0.0, c * (-x / z * fx) }, t1[3] = { c * 0.0, c * fy, c * (-y / z * fy) };
        for (int j = 0; j < 3; j++) {
            Jl[j] = (t0[0] * Rt[j] + t0[1] * Rt[3 + j]) + t0[2] * Rt[6 + j];
            Jl[6 + j] = (t1[0] * Rt[j] + t1[1] * Rt[3 + j]) + t1[2] * Rt[6 + j];
        }
        if (free_kf) {
            Jp[0] = x * y / z_2 * fx; Jp[1] = -(1 + (x * x / z_2)) * fx; Jp[2] = y / z * fx; Jp[3] = -1. / z * fx; Jp[4] = 0; Jp[5] = x / z_2 * fx;
            Jp[6] = (1 + y * y / z_2) * fy; Jp[7] = -x * y / z_2 * fy; Jp[8] = -x / z * fy; Jp[9] = 0; Jp[10] = -1. / z * fy; Jp[11] = y / z_2 * fy;
        }
        return;
    }
    // g2o's numeric Jacobian (base_binary_edge.hpp:147, base_multi_edge.hpp:72): per non-fixed vertex, central differences
    const double scalar = 1.0 / (2 * LBA_DELTA);
    const int d0 = E.kind == LBA_END ? 3 : 0, d1 = E.kind == LBA_START ? 3 : 6;
    for (int d = d0; d < d1; d++) {
        const double keep = X[d];
        double ea[2], eb[2];
        X[d] = keep + LBA_DELTA; lb_error(E, Rt, X, ea);
        X[d] = keep + (-LBA_DELTA); lb_error(E, Rt, X, eb);
        X[d] = keep;
        Jl[d] = scalar * (ea[0] - eb[0]);
    }
    if (free_kf)
        for (int d = 0; d < 6; d++) {
            double ea[2], eb[2];
            lb_error(E, Rt + (1 + 2 * d) * 12, X, ea);
            lb_error(E, Rt + (2 + 2 * d) * 12, X, eb);
            Jp[d] = scalar * (ea[0] - eb[0]);
        }
}

// b -= J^T (rho' (Omega e)),  H += J^T (rho' Omega) J  (base_binary_edge.hpp constructQuadraticForm), edge after edge
static __device__ __forceinline__ void lb_add_edge(const double *Ja, const double *Jb, const double *ew, double *H, double *b)
{
    const double w = ew[2] * ew[3], we0 = ew[3] * ew[0], we1 = ew[3] * ew[1];
    for (int i = 0; i < 6; i++) {
        if (b) b[i] = b[i] - ew[2] * (Ja[i] * we0 + Ja[6 + i] * we1);
        for (int j = 0; j < 6; j++) H[6 * i + j] = H[6 * i + j] + (Ja[i] * w * Jb[j] + Ja[6 + i] * w * Jb[6 + j]);
    }
}

// one thread per (landmark, free key frame) pair: A = sum Jp^T w Jp, bp, W = sum Jp^T w Jl over the pair's edges in order
__global__ __launch_bounds__(64) void k_lba_pairs(LbArgs a)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n_pairs) return;
    const LbPair P = a.pair[p];
    double A[36], W[36], b[6];
    for (int i = 0; i < 36; i++) { A[i] = 0.0; W[i] = 0.0; }
    for (int i = 0; i < 6; i++) b[i] = 0.0;
    int act = 0;
    for (int e = P.e0; e < P.e1; e++) {
        if (a.level[e]) continue;
        act = 1;
        const double *Jl = a.Jl + (size_t)e * 12, *Jp = a.Jp + (size_t)e * 12, *ew = a.ew + (size_t)e * 4;
        lb_add_edge(Jp, Jp, ew, A, b);
        lb_add_edge(Jp, Jl, ew, W, nullptr);
    }
    for (int i = 0; i < 36; i++) { a.A[(size_t)p * 36 + i] = A[i]; a.W[(size_t)p * 36 + i] = W[i]; }
    for (int i = 0; i < 6; i++) a.bp[(size_t)p * 6 + i] = b[i];
    a.pair_act[p] = act;
}

// one thread per landmark: its Hessian block and gradient over its edges in order
__global__ __launch_bounds__(64) void k_lba_build(LbArgs a)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_lm) return;
    double H[36], b[6];
    for (int i = 0; i < 36; i++) H[i] = 0.0;
    for (int i = 0; i < 6; i++) b[i] = 0.0;
    int act = 0;
    for (int e = a.lm_e0[t]; e < a.lm_e0[t + 1]; e++) {
        if (a.level[e]) continue;
        act = 1;
        const double *Jl = a.Jl + (size_t)e * 12;
        lb_add_edge(Jl, Jl, a.ew + (size_t)e * 4, H, b);
    }
    double md = 0.0;
    for (int i = 0; i < 6; i++) md = fmax(fabs(H[7 * i]), md);
    for (int i = 0; i < 36; i++) a.Hll[(size_t)t * 36 + i] = H[i];
    for (int i = 0; i < 6; i++) a.bl[(size_t)t * 6 + i] = b[i];
    a.lm_act[t] = act; a.lm_maxd[t] = md;
}

// one wave per free key frame: its diagonal block (lanes 0..35) and gradient (lanes 36..41), each entry added over the key frame's pairs
// in landmark order
__global__ __launch_bounds__(64) void k_lba_diag(LbArgs a)
{
    __shared__ double h[42];
    const int f = blockIdx.x, t = threadIdx.x;
    double v = 0.0; int act = 0;
    for (int k = a.kf_p0[f]; k < a.kf_p0[f + 1]; k++) {
        const int p = a.kf_pairs[k];
        if (!a.pair_act[p]) continue;
        act = 1;
        if (t < 36) v = v + a.A[(size_t)p * 36 + t];
        else if (t < 42) v = v + a.bp[(size_t)p * 6 + t - 36];
    }
    if (t < 42) h[t] = v;
    if (t < 36) a.Hpp[(size_t)f * 36 + t] = v;
    else if (t < 42) a.bfull[(size_t)f * 6 + t - 36] = v;
    __syncthreads();
    if (t == 0) {
        double md = 0.0;
        for (int i = 0; i < 6; i++) md = fmax(fabs(h[7 * i]), md);
        a.kf_act[f] = act; a.kf_maxd[f] = md;
    }
}

// one thread per landmark: (Hll + lambda I)^-1 by LDL^T without pivoting, column by column, and Y = W Hll^-1 for its pairs.
// Not ldlt6_solve (se3quat.hpp), though the recurrences are the same: the order is 3 or 6 at run time, lambda is added while the diagonal
// is read, no pivot is judged, and one factorisation serves `dim` right-hand sides.
__global__ __launch_bounds__(64) void k_lba_invert(LbArgs a, double lambda)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= a.n_lm || !a.lm_act[l]) return;
    const int dim = l < a.n_pts ? 3 : 6;
    double L[36], D[6], Hi[36];
    const double *H = a.Hll + (size_t)l * 36;
    for (int j = 0; j < dim; j++) {
        double s = H[6 * j + j] + lambda;
        for (int k = 0; k < j; k++) s = s - L[6 * j + k] * L[6 * j + k] * D[k];
        D[j] = s;
        for (int i = j + 1; i < dim; i++) {
            double s2 = H[6 * i + j];
            for (int k = 0; k < j; k++) s2 = s2 - L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = s2 / D[j];
        }
    }
    for (int i = 0; i < 36; i++) Hi[i] = 0.0;
    for (int c = 0; c < dim; c++) {
        double y[6], x[6];
        for (int i = 0; i < dim; i++) { double s = i == c ? 1.0 : 0.0; for (int k = 0; k < i; k++) s = s - L[6 * i + k] * y[k]; y[i] = s; }
        for (int i = dim - 1; i >= 0; i--) { double s = y[i] / D[i]; for (int k = i + 1; k < dim; k++) s = s - L[6 * k + i] * x[k]; x[i] = s; }
        for (int i = 0; i < dim; i++) Hi[6 * i + c] = x[i];
    }
    for (int i = 0; i < 36; i++) a.Hinv[(size_t)l * 36 + i] = Hi[i];
    for (int p = a.lm_p0[l]; p < a.lm_p0[l + 1]; p++) {
        const double *W = a.W + (size_t)p * 36; double *Y = a.Y + (size_t)p * 36;
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 6; c++) {
                double s = 0.0;
                for (int k = 0; k < dim; k++) s = s + W[6 * r + k] * Hi[6 * k + c];
                Y[6 * r + c] = s;
            }
    }
}

// one wave per (free key frame i, free key frame j >= i): lanes 0..35 own the block's entries, lanes 36..41 (i == j) the gradient.
// The common landmarks are found by walking both observer-major pair lists, which are in landmark order.
__global__ __launch_bounds__(64) void k_lba_reduce(LbArgs a, double lambda)
{
    const int i = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
    if (j < i || t >= 42 || (t >= 36 && i != j)) return;
    const int n6 = a.n6;
    if (i == j && !a.kf_act[i]) {                                               // no active edge: the key frame keeps its estimate
        if (t < 36) a.S[(size_t)(6 * i + t / 6) * n6 + 6 * i + t % 6] = t / 6 == t % 6 ? 1.0 : 0.0;
        else a.rhs[6 * i + t - 36] = 0.0;
        return;
    }
    const int r = t < 36 ? t / 6 : t - 36, c = t % 6;
    int ki = a.kf_p0[i], kj = a.kf_p0[j];
    const int ei = a.kf_p0[i + 1], ej = a.kf_p0[j + 1];
    double acc = 0.0;
    while (ki < ei && kj < ej) {
        const int pi = a.kf_pairs[ki], pj = a.kf_pairs[kj];
        const int li = a.pair[pi].lm, lj = a.pair[pj].lm;
        if (li < lj) { ki++; continue; }
        if (lj < li) { kj++; continue; }
        ki++; kj++;
        if (!a.lm_act[li] || !a.pair_act[pi] || !a.pair_act[pj]) continue;
        const double *Y = a.Y + (size_t)pi * 36 + 6 * r;
        double s = 0.0;
        if (t < 36) { const double *W = a.W + (size_t)pj * 36 + 6 * c; for (int k = 0; k < 6; k++) s = s + Y[k] * W[k]; }
        else { const double *bl = a.bl + (size_t)li * 6; for (int k = 0; k < 6; k++) s = s + Y[k] * bl[k]; }
        acc = acc + s;
    }
    if (t >= 36) { a.rhs[6 * i + r] = a.bfull[(size_t)i * 6 + r] - acc; return; }
    double v = -acc;
    if (i == j) { v = a.Hpp[(size_t)i * 36 + t] - acc; if (r == c) v = v + lambda; }
    a.S[(size_t)(6 * i + r) * n6 + 6 * j + c] = v;
    a.S[(size_t)(6 * j + c) * n6 + 6 * i + r] = v;
}

// one workgroup: S = L D L^T in place without pivoting (right-looking, the lower triangle), then the two substitutions column by column.
// out[2] = 1 when every pivot was positive.  Exempt from the budget test's LDS and register limits by design: it runs once per trial.
__global__ __launch_bounds__(LBA_THREADS) void k_lba_solve(LbArgs a)
{
    __shared__ double raw[6 * HVO_LBA_MAX_FREE_KF], l[6 * HVO_LBA_MAX_FREE_KF], y[6 * HVO_LBA_MAX_FREE_KF];
    __shared__ int bad;
    const int n = a.n6, t = threadIdx.x;
    double *S = a.S;
    if (t == 0) bad = 0;
    for (int i = t; i < n; i += LBA_THREADS) y[i] = a.rhs[i];
    __syncthreads();
    for (int j = 0; j < n; j++) {
        const double d = S[(size_t)j * n + j];
        if (t == 0 && !(d > 0)) bad = 1;
        for (int i = j + 1 + t; i < n; i += LBA_THREADS) { const double v = S[(size_t)i * n + j]; raw[i] = v; l[i] = v / d; }
        __syncthreads();
        for (int i = j + 1 + (t >> 4); i < n; i += LBA_THREADS / 16)            // 16 x 16 tiles over the trailing lower triangle
            for (int k = j + 1 + (t & 15); k <= i; k += 16) S[(size_t)i * n + k] = S[(size_t)i * n + k] - l[i] * raw[k];
        for (int i = j + 1 + t; i < n; i += LBA_THREADS) S[(size_t)i * n + j] = l[i];
        __syncthreads();
    }
    for (int j = 0; j < n; j++) {                                               // L y = rhs
        const double yj = y[j];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += LBA_THREADS) y[i] = y[i] - S[(size_t)i * n + j] * yj;
        __syncthreads();
    }
    for (int i = t; i < n; i += LBA_THREADS) y[i] = y[i] / S[(size_t)i * n + i];
    __syncthreads();
    for (int j = n - 1; j >= 0; j--) {                                          // L^T x = D^-1 y
        const double xj = y[j];
        __syncthreads();
        for (int i = t; i < j; i += LBA_THREADS) y[i] = y[i] - S[(size_t)j * n + i] * xj;
        __syncthreads();
    }
    for (int i = t; i < n; i += LBA_THREADS) a.dx[i] = y[i];
    if (t == 0) a.out[2] = bad ? 0.0 : 1.0;
}

// threads 0 .. n_lm - 1: back-substitution into a landmark and oplus (estimate += update); the next n_kf threads: a key frame's oplus
// (exp(update) * estimate).  Writes the trial state and the vertex's terms of computeScale.
__global__ __launch_bounds__(64) void k_lba_update(LbArgs a, double lambda)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_lm + a.n_kf) return;
    if (t < a.n_lm) {
        const double *X = a.est + (size_t)a.n_kf * 8 + (size_t)t * 6; double *Xt = a.trial + (size_t)a.n_kf * 8 + (size_t)t * 6;
        double sc = 0.0;
        if (!a.lm_act[t]) { for (int i = 0; i < 6; i++) Xt[i] = X[i]; a.sc[t] = 0.0; return; }
        const int dim = t < a.n_pts ? 3 : 6;
        double v[6];
        for (int i = 0; i < 6; i++) v[i] = a.bl[(size_t)t * 6 + i];
        for (int p = a.lm_p0[t]; p < a.lm_p0[t + 1]; p++) {
            if (!a.pair_act[p]) continue;
            const double *W = a.W + (size_t)p * 36, *dx = a.dx + 6 * a.pair[p].f;
            for (int c = 0; c < dim; c++) {
                double s = 0.0;
                for (int r = 0; r < 6; r++) s = s + W[6 * r + c] * dx[r];
                v[c] = v[c] - s;
            }
        }
        const double *Hi = a.Hinv + (size_t)t * 36;
        for (int i = 0; i < 6; i++) {
            double s = 0.0;
            if (i < dim) for (int k = 0; k < dim; k++) s = s + Hi[6 * i + k] * v[k];
            Xt[i] = i < dim ? X[i] + s : X[i];
            if (i < dim) sc = sc + s * (lambda * s + a.bl[(size_t)t * 6 + i]);
        }
        a.sc[t] = sc;
        return;
    }
    const int kf = t - a.n_lm, f = a.kf_free[kf];
    const double *P = a.est + (size_t)kf * 8; double *Pt = a.trial + (size_t)kf * 8;
    if (f < 0 || !a.kf_act[f]) { for (int i = 0; i < 8; i++) Pt[i] = P[i]; if (f >= 0) a.sc[a.n_lm + f] = 0.0; return; }
    double u[6], e[7], b[7], o[7], sc = 0.0;
    for (int i = 0; i < 6; i++) { u[i] = a.dx[6 * f + i]; sc = sc + u[i] * (lambda * u[i] + a.bfull[(size_t)f * 6 + i]); }
    for (int i = 0; i < 7; i++) b[i] = P[i];
    se3_exp(u, e); se3_mul(e, b, o);
    for (int i = 0; i < 7; i++) Pt[i] = o[i];
    Pt[7] = 0.0;
    a.sc[a.n_lm + f] = sc;
}

// one workgroup: out[0] = sum of rho over the edges, out[1] = sum of the computeScale terms, out[3] = largest Hessian diagonal of the
// active vertices.  The tree: thread t adds items t, t + 256, ... in order, a wave halves its lanes, the four waves are added in order.
static __device__ double lb_tree(const double *v, int n, double *red)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double x = 0.0;
    for (int i = t; i < n; i += LBA_THREADS) x = x + v[i];
    x = wave_sum_down(x);
    __syncthreads();
    if (lane == 0) red[wave] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(LBA_THREADS) void k_lba_sum(LbArgs a)
{
    __shared__ double red[4];
    __shared__ double mx[LBA_THREADS];
    const int t = threadIdx.x;
    const double chi = lb_tree(a.rho, a.n_edges, red);
    const double sc = lb_tree(a.sc, a.n_lm + a.n_free, red);
    double m = 0.0;
    for (int i = t; i < a.n_lm; i += LBA_THREADS) if (a.lm_act[i]) m = fmax(m, a.lm_maxd[i]);
    for (int i = t; i < a.n_free; i += LBA_THREADS) if (a.kf_act[i]) m = fmax(m, a.kf_maxd[i]);
    mx[t] = m;
    __syncthreads();
    for (int off = LBA_THREADS / 2; off > 0; off >>= 1) { if (t < off) mx[t] = fmax(mx[t], mx[t + off]); __syncthreads(); }
    if (t == 0) { a.out[0] = chi; a.out[1] = sc; a.out[3] = mx[0]; }
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------
struct hvo_local_ba {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evg[4] = { nullptr, nullptr, nullptr, nullptr };   // the call; a group of launches; the factorisation
    std::string last_error;
    float last_ms = 0.f, prof_ms[4] = { 0.f, 0.f, 0.f, 0.f };      // linearisations, trials, of the trials the factorisation, the whole call
    int prof_n[2] = { 0, 0 };
    char *d_in = nullptr, *d_work = nullptr, *h_pin = nullptr;
    size_t in_cap = 0, work_cap = 0, pin_cap = 0;
};

static int lb_fail(hvo_local_ba *B, int rc, const std::string &why) { B->last_error = why; return rc; }
#define LB_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return lb_fail(B, HVO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

static int lb_reserve(hvo_local_ba *B, char **p, size_t *cap, size_t bytes, bool pinned)
{
    if (*cap >= bytes) return HVO_OK;
    const size_t want = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
    if (*p) { if (pinned) LB_HIP(hipHostFree(*p)); else LB_HIP(hipFree(*p)); *p = nullptr; *cap = 0; }
    if (pinned) LB_HIP(hipHostMalloc((void **)p, want, hipHostMallocDefault)); else LB_HIP(hipMalloc((void **)p, want));
    *cap = want;
    return HVO_OK;
}

struct LbLayout {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

extern "C" {

void hvo_local_ba_default_params(hvo_local_ba_params *p)
{
    if (!p) return;
    p->iterations[0] = 5; p->iterations[1] = 10; p->max_trials = 10; p->stop_at_poll = -1;
    p->huber_delta[0] = (double)(float)sqrt(5.991); p->huber_delta[1] = (double)(float)sqrt(3.84); p->huber_delta[2] = (double)(float)sqrt(0.08);
    p->chi2_gate[0] = 5.991; p->chi2_gate[1] = 3.84; p->chi2_gate[2] = 0.13;
    p->inv_sigma[0] = 0.3; p->inv_sigma[1] = 0.3; p->inv_sigma[2] = 0.5;
}

int hvo_local_ba_create(int device, hvo_local_ba **ba)
{
    if (!ba || device < 0) return HVO_ERR_INVALID_ARG;
    *ba = nullptr;
    if (hipSetDevice(device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HVO_ERR_NO_DEVICE;        // the code object is gfx950 only
    hvo_local_ba *B = new hvo_local_ba();
    B->device = device;
    if (hipStreamCreateWithFlags(&B->st, hipStreamNonBlocking) != hipSuccess) { B->st = nullptr; hvo_local_ba_destroy(B); return HVO_ERR_HIP; }
    if (hipEventCreate(&B->ev0) != hipSuccess || hipEventCreate(&B->ev1) != hipSuccess) { hvo_local_ba_destroy(B); return HVO_ERR_HIP; }
    for (int i = 0; i < 4; i++) if (hipEventCreate(&B->evg[i]) != hipSuccess) { B->evg[i] = nullptr; hvo_local_ba_destroy(B); return HVO_ERR_HIP; }
    *ba = B;
    return HVO_OK;
}

void hvo_local_ba_destroy(hvo_local_ba *B)
{
    if (!B) return;
    (void)hipSetDevice(B->device);
    if (B->st) { (void)hipStreamSynchronize(B->st); (void)hipStreamDestroy(B->st); }
    if (B->ev0) (void)hipEventDestroy(B->ev0);
    if (B->ev1) (void)hipEventDestroy(B->ev1);
    for (int i = 0; i < 4; i++) if (B->evg[i]) (void)hipEventDestroy(B->evg[i]);
    if (B->d_in) (void)hipFree(B->d_in);
    if (B->d_work) (void)hipFree(B->d_work);
    if (B->h_pin) (void)hipHostFree(B->h_pin);
    delete B;
}

const char *hvo_local_ba_last_error(const hvo_local_ba *B) { return B ? B->last_error.c_str() : ""; }

int hvo_local_ba_last_ms(const hvo_local_ba *B, float *ms)
{
    if (!B || !ms) return HVO_ERR_INVALID_ARG;
    *ms = B->last_ms;
    return HVO_OK;
}

int hvo_local_ba_last_profile(const hvo_local_ba *B, float ms[4], int32_t n[2])
{
    if (!B || !ms || !n) return HVO_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++) ms[i] = B->prof_ms[i];
    n[0] = B->prof_n[0]; n[1] = B->prof_n[1];
    return HVO_OK;
}

}  // extern "C"

namespace {

struct LbHost {                       // the graph in launch order and where every flag goes back to
    std::vector<LbEdge> edge; std::vector<int> src;          // src: the observation / entry / line index of the edge's flag
    std::vector<LbPair> pair;
    std::vector<int> lm_e0, lm_p0, kf_free, free_kf, kf_p0, kf_pairs, lm_line;     // lm_line: landmark -> line index (points: -1)
    std::vector<uint8_t> level;
    std::vector<double> state;        // pose n_kf x 8 | landmark n_lm x 6
    std::vector<int> ln_start_edge, ln_end_edge, par_edge, perp_edge, manh_edge, pt_edge;   // per observation / entry / line: edge or -1
};

bool lb_nan3(const double *v) { return std::isnan(v[0]) || std::isnan(v[1]) || std::isnan(v[2]); }

struct LbPoll {
    const volatile int *stop; int at, count = 0, first = -1;
    bool operator()() {
        const int k = count++;
        const bool s = (at >= 0 && k >= at) || (stop && *stop);
        if (s && first < 0) first = k;
        return s;
    }
};

}  // namespace

extern "C" int hvo_local_ba_optimize(hvo_local_ba *B, const hvo_local_ba_params *params, const hvo_local_ba_graph *G, const volatile int *stop,
                                     hvo_local_ba_result *R)
{
    if (!B) return HVO_ERR_INVALID_ARG;
    B->last_error.clear(); B->last_ms = 0.f;
    for (int i = 0; i < 4; i++) B->prof_ms[i] = 0.f;
    B->prof_n[0] = B->prof_n[1] = 0;
    if (!G || !R) return lb_fail(B, HVO_ERR_INVALID_ARG, "graph or result is NULL");
    hvo_local_ba_params P;
    if (params) P = *params; else hvo_local_ba_default_params(&P);
    const int nkf = G->n_kf, np = G->n_points, nl = G->n_lines;
    if (nkf < 0 || np < 0 || nl < 0) return lb_fail(B, HVO_ERR_INVALID_ARG, "a negative count");
    if (P.iterations[0] < 0 || P.iterations[1] < 0 || P.max_trials < 1) return lb_fail(B, HVO_ERR_INVALID_ARG, "iterations or max_trials");
    if (nkf > HVO_LBA_MAX_KF) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 1024 key frames");
    if (np > HVO_LBA_MAX_POINTS) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 65536 points");
    if (nl > HVO_LBA_MAX_LINES) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 16384 lines");
    if ((nkf && (!G->Tcw || !G->fixed || !G->cam)) || (np && (!G->pt_pos || !G->pt_obs_start)) ||
        (nl && (!G->ln_pos || !G->ln_manh_idx || !G->ln_obs_start || !G->par_start || !G->perp_start || !G->par_map_size || !G->perp_map_size)))
        return lb_fail(B, HVO_ERR_INVALID_ARG, "a NULL array of the graph");
    if ((nkf && (!R->Tcw_f || !R->Tcw_d)) || (np && (!R->pt_f || !R->pt_d)) || (nl && (!R->ln_f || !R->ln_d || !R->manh_erase || !R->line_made)))
        return lb_fail(B, HVO_ERR_INVALID_ARG, "a NULL array of the result");
    const int n_pt_obs = np ? G->pt_obs_start[np] : 0, n_ln_obs = nl ? G->ln_obs_start[nl] : 0;
    const int n_par = nl ? G->par_start[nl] : 0, n_perp = nl ? G->perp_start[nl] : 0;
    auto csr_ok = [](const int32_t *s, int n) { if (!n) return true; if (s[0] != 0) return false; for (int i = 0; i < n; i++) if (s[i + 1] < s[i]) return false; return true; };
    if (!csr_ok(G->pt_obs_start, np) || !csr_ok(G->ln_obs_start, nl) || !csr_ok(G->par_start, nl) || !csr_ok(G->perp_start, nl))
        return lb_fail(B, HVO_ERR_INVALID_ARG, "a start array that does not begin at 0 or decreases");
    if (n_pt_obs > HVO_LBA_MAX_PT_OBS) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 2^20 point observations");
    if (n_ln_obs > HVO_LBA_MAX_LN_OBS) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 2^18 line observations");
    if ((long long)n_par + n_perp > HVO_LBA_MAX_STRUCT) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 2^18 par plus perp entries");
    if ((n_pt_obs && (!G->pt_obs_kf || !G->pt_obs_uv || !G->pt_obs_inv_sigma2 || !R->pt_erase)) || (n_ln_obs && (!G->ln_obs_kf || !G->ln_obs_fn || !R->ln_erase)) ||
        (n_par && (!G->par_kf || !G->par_idx || !G->par_fn || !R->par_erase || !R->par_made)) ||
        (n_perp && (!G->perp_kf || !G->perp_idx || !G->perp_fn || !R->perp_erase || !R->perp_made)))
        return lb_fail(B, HVO_ERR_INVALID_ARG, "a NULL observation array");
    if (G->manh_available && !G->manh_axis) return lb_fail(B, HVO_ERR_INVALID_ARG, "manh_available without manh_axis");

    LbHost H;
    H.kf_free.assign(nkf, -1);
    for (int k = 0; k < nkf; k++) if (!G->fixed[k]) { H.kf_free[k] = (int)H.free_kf.size(); H.free_kf.push_back(k); }
    const int nf = (int)H.free_kf.size();
    if (nf > HVO_LBA_MAX_FREE_KF) return lb_fail(B, HVO_ERR_UNSUPPORTED, "more than 64 free key frames");
    auto kf_ok = [&](const int32_t *kf, int n) { for (int i = 0; i < n; i++) if (kf[i] < 0 || kf[i] >= nkf) return false; return true; };
    if (!kf_ok(G->pt_obs_kf, n_pt_obs) || !kf_ok(G->ln_obs_kf, n_ln_obs) || !kf_ok(G->par_kf, n_par) || !kf_ok(G->perp_kf, n_perp))
        return lb_fail(B, HVO_ERR_UNSUPPORTED, "a key-frame index outside the call's list");
    {
        std::vector<int> stamp(nkf, -1);
        for (int i = 0; i < np; i++)
            for (int o = G->pt_obs_start[i]; o < G->pt_obs_start[i + 1]; o++) {
                if (stamp[G->pt_obs_kf[o]] == i) return lb_fail(B, HVO_ERR_UNSUPPORTED, "a key frame observes one point twice");
                stamp[G->pt_obs_kf[o]] = i;
            }
        for (int i = 0; i < nl; i++)
            for (int o = G->ln_obs_start[i]; o < G->ln_obs_start[i + 1]; o++) {
                if (stamp[G->ln_obs_kf[o]] == np + i) return lb_fail(B, HVO_ERR_UNSUPPORTED, "a key frame observes one line twice");
                stamp[G->ln_obs_kf[o]] = np + i;
            }
    }

    // ---- the graph in launch order: landmark-major, a landmark's edges grouped by key frame ----
    const double cam0[4] = { nkf ? (double)G->cam[0] : 0, nkf ? (double)G->cam[1] : 0, nkf ? (double)G->cam[2] : 0, nkf ? (double)G->cam[3] : 0 };
    H.pt_edge.assign(n_pt_obs, -1); H.ln_start_edge.assign(n_ln_obs, -1); H.ln_end_edge.assign(n_ln_obs, -1);
    H.par_edge.assign(n_par, -1); H.perp_edge.assign(n_perp, -1); H.manh_edge.assign(nl, -1);
    std::vector<uint8_t> line_made(nl, 0);
    std::vector<double> lm_pos;
    int cnt[6] = { 0, 0, 0, 0, 0, 0 };
    auto open_lm = [&](const double *X, int line) { H.lm_e0.push_back((int)H.edge.size()); H.lm_p0.push_back((int)H.pair.size()); H.lm_line.push_back(line); for (int i = 0; i < 6; i++) lm_pos.push_back(X[i]); };
    auto add_edge = [&](int kind, int kf, const double *m, double info, double delta, const double *cam, int src) {
        LbEdge E; memset(&E, 0, sizeof E);
        E.kind = kind; E.lm = (int)H.lm_line.size() - 1; E.kf = kf; E.pair = -1;
        for (int i = 0; i < 3; i++) E.m[i] = m[i];
        E.info = info; E.delta = delta;
        for (int i = 0; i < 4; i++) E.cam[i] = cam[i];
        if (kf >= 0 && H.kf_free[kf] >= 0) {
            if (H.pair.empty() || H.pair.back().lm != E.lm || H.pair.back().f != H.kf_free[kf]) H.pair.push_back({ E.lm, H.kf_free[kf], (int)H.edge.size(), (int)H.edge.size() });
            E.pair = (int)H.pair.size() - 1; H.pair.back().e1 = (int)H.edge.size() + 1;
        }
        H.edge.push_back(E); H.src.push_back(src); cnt[kind]++;
        return (int)H.edge.size() - 1;
    };
    for (int i = 0; i < np; i++) {
        const double X[6] = { (double)G->pt_pos[3 * i], (double)G->pt_pos[3 * i + 1], (double)G->pt_pos[3 * i + 2], 0, 0, 0 };
        open_lm(X, -1);
        for (int o = G->pt_obs_start[i]; o < G->pt_obs_start[i + 1]; o++) {
            const int kf = G->pt_obs_kf[o];
            const double m[3] = { (double)G->pt_obs_uv[2 * o], (double)G->pt_obs_uv[2 * o + 1], 0 };
            const double cam[4] = { (double)G->cam[4 * kf], (double)G->cam[4 * kf + 1], (double)G->cam[4 * kf + 2], (double)G->cam[4 * kf + 3] };
            H.pt_edge[o] = add_edge(LBA_PT, kf, m, (double)G->pt_obs_inv_sigma2[o], P.huber_delta[0], cam, o);
        }
    }
    struct Item { int kf, kind, src; };
    std::vector<Item> items;
    for (int i = 0; i < nl; i++) {
        const double *X = G->ln_pos + 6 * (size_t)i;
        if (lb_nan3(X) || lb_nan3(X + 3) || fabs(X[3] - X[0]) < 0.00001) continue;                    // :3358-3366
        line_made[i] = 1;
        open_lm(X, i);
        if (G->manh_available && G->ln_manh_idx[i] > 0 && G->ln_manh_idx[i] <= 3) {
            const int c = G->ln_manh_idx[i] - 1;
            const double m[3] = { G->manh_axis[c], G->manh_axis[3 + c], G->manh_axis[6 + c] };
            H.manh_edge[i] = add_edge(LBA_MANH, -1, m, P.inv_sigma[1], P.huber_delta[2], cam0, i);
        }
        items.clear();
        for (int o = G->ln_obs_start[i]; o < G->ln_obs_start[i + 1]; o++) { items.push_back({ G->ln_obs_kf[o], LBA_START, o }); items.push_back({ G->ln_obs_kf[o], LBA_END, o }); }
        for (int s = 0; s < 2; s++) {
            const int32_t *st = s ? G->perp_start : G->par_start, *kfv = s ? G->perp_kf : G->par_kf, *idx = s ? G->perp_idx : G->par_idx;
            const double *fn = s ? G->perp_fn : G->par_fn;
            for (int o = st[i]; o < st[i + 1]; o++) {
                const double *l = fn + 3 * (size_t)o;
                if (idx[o] < 0 || l[0] == 0.0 || l[0] == -1.0 || lb_nan3(l)) continue;                   // :3484-3501
                items.push_back({ kfv[o], s ? LBA_PERP : LBA_PAR, o });
            }
        }
        std::stable_sort(items.begin(), items.end(), [](const Item &x, const Item &y) { return x.kf < y.kf; });
        for (const Item &it : items) {
            const int kf = it.kf;
            const double camk[4] = { (double)G->cam[4 * kf], (double)G->cam[4 * kf + 1], (double)G->cam[4 * kf + 2], (double)G->cam[4 * kf + 3] };
            if (it.kind == LBA_START) H.ln_start_edge[it.src] = add_edge(LBA_START, kf, G->ln_obs_fn + 3 * (size_t)it.src, P.inv_sigma[0], P.huber_delta[1], camk, it.src);
            else if (it.kind == LBA_END) H.ln_end_edge[it.src] = add_edge(LBA_END, kf, G->ln_obs_fn + 3 * (size_t)it.src, P.inv_sigma[0], P.huber_delta[1], cam0, it.src);   // reading 1
            else if (it.kind == LBA_PAR) H.par_edge[it.src] = add_edge(LBA_PAR, kf, G->par_fn + 3 * (size_t)it.src, P.inv_sigma[2] + G->par_map_size[i] / 10.0, P.huber_delta[2], cam0, it.src);
            else H.perp_edge[it.src] = add_edge(LBA_PERP, kf, G->perp_fn + 3 * (size_t)it.src, P.inv_sigma[2] + G->perp_map_size[i] / 10.0, P.huber_delta[2], cam0, it.src);
        }
    }
    const int nlm = (int)H.lm_line.size(), nE = (int)H.edge.size(), nP = (int)H.pair.size();
    H.lm_e0.push_back(nE); H.lm_p0.push_back(nP);
    // observer-major pair lists: pairs are created landmark-major, so a stable bucket by key frame keeps landmark order
    H.kf_p0.assign(nf + 1, 0);
    for (const LbPair &p : H.pair) H.kf_p0[p.f + 1]++;
    for (int f = 0; f < nf; f++) H.kf_p0[f + 1] += H.kf_p0[f];
    H.kf_pairs.assign(nP, 0);
    { std::vector<int> at(H.kf_p0.begin(), H.kf_p0.end() - 1); for (int p = 0; p < nP; p++) H.kf_pairs[at[H.pair[p].f]++] = p; }
    // the estimates: Converter::toSE3Quat(GetPose())
    H.state.assign((size_t)nkf * 8 + (size_t)nlm * 6, 0.0);
    for (int k = 0; k < nkf; k++) {
        const float *T = G->Tcw + 12 * (size_t)k;
        const double Rm[9] = { T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10] };
        double *p = &H.state[(size_t)k * 8];
        quat_from_R(Rm, p); quat_normalize(p);
        p[4] = T[3]; p[5] = T[7]; p[6] = T[11];
    }
    for (size_t i = 0; i < lm_pos.size(); i++) H.state[(size_t)nkf * 8 + i] = lm_pos[i];
    H.level.assign(nE, 0);

    // ---- from here on outputs are written ----
    auto write_inputs = [&]() {
        for (size_t i = 0; i < (size_t)nkf * 12; i++) { R->Tcw_f[i] = G->Tcw[i]; R->Tcw_d[i] = (double)G->Tcw[i]; }
        for (size_t i = 0; i < (size_t)np * 3; i++) { R->pt_f[i] = G->pt_pos[i]; R->pt_d[i] = (double)G->pt_pos[i]; }
        for (size_t i = 0; i < (size_t)nl * 6; i++) { R->ln_f[i] = (float)G->ln_pos[i]; R->ln_d[i] = G->ln_pos[i]; }
    };
    auto write_counts = [&]() {
        for (int i = 0; i < n_pt_obs; i++) R->pt_erase[i] = 0;
        for (int i = 0; i < n_ln_obs; i++) R->ln_erase[i] = 0;
        for (int i = 0; i < nl; i++) { R->manh_erase[i] = 0; R->line_made[i] = line_made[i]; }
        for (int i = 0; i < n_par; i++) { R->par_erase[i] = 0; R->par_made[i] = H.par_edge[i] >= 0; }
        for (int i = 0; i < n_perp; i++) { R->perp_erase[i] = 0; R->perp_made[i] = H.perp_edge[i] >= 0; }
        for (int r = 0; r < 2; r++) { R->iterations[r] = R->trials[r] = 0; R->lambda[r] = R->chi2[r] = 0.0; }
        R->n_free_kf = nf; R->n_pt_edges = cnt[LBA_PT]; R->n_line_obs = cnt[LBA_START]; R->n_manh_edges = cnt[LBA_MANH];
        R->n_par_edges = cnt[LBA_PAR]; R->n_perp_edges = cnt[LBA_PERP]; R->n_lines_made = nlm - np; R->rounds = 0; R->stopped_at = -1;
    };
    if (nf == 0 || nE == 0) { write_inputs(); write_counts(); R->status = HVO_LBA_NOTHING; return HVO_OK; }
    LbPoll poll{ stop, P.stop_at_poll };
    if (poll()) { write_inputs(); write_counts(); R->stopped_at = poll.first; R->status = HVO_LBA_STOPPED; return HVO_OK; }      // :3641

    if (hipSetDevice(B->device) != hipSuccess) return lb_fail(B, HVO_ERR_NO_DEVICE, "hipSetDevice");
    const int n6 = 6 * nf;
    // the upload block
    LbLayout Li;
    const size_t o_kf_free = Li.take(sizeof(int) * nkf), o_edge = Li.take(sizeof(LbEdge) * nE), o_pair = Li.take(sizeof(LbPair) * std::max(nP, 1));
    const size_t o_lm_e0 = Li.take(sizeof(int) * (nlm + 1)), o_lm_p0 = Li.take(sizeof(int) * (nlm + 1));
    const size_t o_kf_p0 = Li.take(sizeof(int) * (nf + 1)), o_kf_pairs = Li.take(sizeof(int) * std::max(nP, 1));
    const size_t o_state = Li.take(sizeof(double) * H.state.size()), o_level = Li.take(nE);
    // the work block
    LbLayout Lw;
    const size_t state_bytes = sizeof(double) * H.state.size();
    const size_t w_est = Lw.take(state_bytes), w_trial = Lw.take(state_bytes), w_Rt = Lw.take(sizeof(double) * nkf * 13 * 12);
    const size_t w_Jl = Lw.take(sizeof(double) * 12 * nE), w_Jp = Lw.take(sizeof(double) * 12 * nE), w_ew = Lw.take(sizeof(double) * 4 * nE);
    const size_t w_rho = Lw.take(sizeof(double) * nE), w_chi = Lw.take(sizeof(double) * nE);
    const size_t nP1 = std::max(nP, 1);
    const size_t w_A = Lw.take(sizeof(double) * 36 * nP1), w_bp = Lw.take(sizeof(double) * 6 * nP1), w_W = Lw.take(sizeof(double) * 36 * nP1), w_Y = Lw.take(sizeof(double) * 36 * nP1);
    const size_t w_pact = Lw.take(sizeof(int) * nP1);
    const size_t w_Hll = Lw.take(sizeof(double) * 36 * nlm), w_bl = Lw.take(sizeof(double) * 6 * nlm), w_Hinv = Lw.take(sizeof(double) * 36 * nlm);
    const size_t w_lmd = Lw.take(sizeof(double) * nlm), w_lact = Lw.take(sizeof(int) * nlm);
    const size_t w_Hpp = Lw.take(sizeof(double) * 36 * nf), w_bfull = Lw.take(sizeof(double) * 6 * nf), w_kmd = Lw.take(sizeof(double) * nf), w_kact = Lw.take(sizeof(int) * nf);
    const size_t w_S = Lw.take(sizeof(double) * n6 * n6), w_rhs = Lw.take(sizeof(double) * n6), w_dx = Lw.take(sizeof(double) * n6);
    const size_t w_sc = Lw.take(sizeof(double) * (nlm + nf)), w_out = Lw.take(sizeof(double) * 4);
    // the pinned block: the upload image, then the downloads (four scalars, the state, the held chi2)
    LbLayout Lp;
    const size_t p_in = Lp.take(Li.off), p_out = Lp.take(sizeof(double) * 4), p_state = Lp.take(state_bytes), p_chi = Lp.take(sizeof(double) * nE);
    int rc;
    if ((rc = lb_reserve(B, &B->d_in, &B->in_cap, Li.off, false)) || (rc = lb_reserve(B, &B->d_work, &B->work_cap, Lw.off, false)) ||
        (rc = lb_reserve(B, &B->h_pin, &B->pin_cap, Lp.off, true))) return rc;
    char *hp = B->h_pin + p_in;
    memcpy(hp + o_kf_free, H.kf_free.data(), sizeof(int) * nkf);
    memcpy(hp + o_edge, H.edge.data(), sizeof(LbEdge) * nE);
    if (nP) memcpy(hp + o_pair, H.pair.data(), sizeof(LbPair) * nP);
    memcpy(hp + o_lm_e0, H.lm_e0.data(), sizeof(int) * (nlm + 1));
    memcpy(hp + o_lm_p0, H.lm_p0.data(), sizeof(int) * (nlm + 1));
    memcpy(hp + o_kf_p0, H.kf_p0.data(), sizeof(int) * (nf + 1));
    if (nP) memcpy(hp + o_kf_pairs, H.kf_pairs.data(), sizeof(int) * nP);
    memcpy(hp + o_state, H.state.data(), state_bytes);
    memcpy(hp + o_level, H.level.data(), nE);
    hipStream_t st = B->st;
    LB_HIP(hipEventRecord(B->ev0, st));
    LB_HIP(hipMemcpyAsync(B->d_in, hp, Li.off, hipMemcpyHostToDevice, st));
    LbArgs a; memset(&a, 0, sizeof a);
    a.n_kf = nkf; a.n_free = nf; a.n_pts = np; a.n_lm = nlm; a.n_edges = nE; a.n_pairs = nP; a.n6 = n6; a.robust = 1;
    a.kf_free = (const int *)(B->d_in + o_kf_free); a.edge = (const LbEdge *)(B->d_in + o_edge); a.pair = (const LbPair *)(B->d_in + o_pair);
    a.lm_e0 = (const int *)(B->d_in + o_lm_e0); a.lm_p0 = (const int *)(B->d_in + o_lm_p0);
    a.kf_p0 = (const int *)(B->d_in + o_kf_p0); a.kf_pairs = (const int *)(B->d_in + o_kf_pairs); a.level = (const uint8_t *)(B->d_in + o_level);
    char *w = B->d_work;
    a.est = (double *)(w + w_est); a.trial = (double *)(w + w_trial); a.Rt = (double *)(w + w_Rt);
    a.Jl = (double *)(w + w_Jl); a.Jp = (double *)(w + w_Jp); a.ew = (double *)(w + w_ew); a.rho = (double *)(w + w_rho); a.chi_held = (double *)(w + w_chi);
    a.A = (double *)(w + w_A); a.bp = (double *)(w + w_bp); a.W = (double *)(w + w_W); a.Y = (double *)(w + w_Y); a.pair_act = (int *)(w + w_pact);
    a.Hll = (double *)(w + w_Hll); a.bl = (double *)(w + w_bl); a.Hinv = (double *)(w + w_Hinv); a.lm_maxd = (double *)(w + w_lmd); a.lm_act = (int *)(w + w_lact);
    a.Hpp = (double *)(w + w_Hpp); a.bfull = (double *)(w + w_bfull); a.kf_maxd = (double *)(w + w_kmd); a.kf_act = (int *)(w + w_kact);
    a.S = (double *)(w + w_S); a.rhs = (double *)(w + w_rhs); a.dx = (double *)(w + w_dx); a.sc = (double *)(w + w_sc); a.out = (double *)(w + w_out);
    LB_HIP(hipMemcpyAsync(a.est, B->d_in + o_state, state_bytes, hipMemcpyDeviceToDevice, st));
    LB_HIP(hipMemcpyAsync(a.trial, B->d_in + o_state, state_bytes, hipMemcpyDeviceToDevice, st));
    LB_HIP(hipMemsetAsync(a.chi_held, 0, sizeof(double) * nE, st));                     // an edge never evaluated holds a zero error
    LB_HIP(hipMemsetAsync(a.sc, 0, sizeof(double) * (nlm + nf), st));
    LB_HIP(hipMemsetAsync(a.out, 0, sizeof(double) * 4, st));
    LB_HIP(hipMemsetAsync(a.Y, 0, sizeof(double) * 36 * nP1, st));
    LB_HIP(hipMemsetAsync(a.Hinv, 0, sizeof(double) * 36 * nlm, st));

    double *h_out = (double *)(B->h_pin + p_out), *h_state = (double *)(B->h_pin + p_state), *h_chi = (double *)(B->h_pin + p_chi);
    auto blocks = [](long long n, int per) { return dim3((unsigned)std::max<long long>((n + per - 1) / per, 1)); };
    auto fetch_out = [&]() -> int {
        LB_HIP(hipMemcpyAsync(h_out, a.out, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
        LB_HIP(hipStreamSynchronize(st));
        return HVO_OK;
    };
    auto fetch_held = [&]() -> int {
        LB_HIP(hipMemcpyAsync(h_chi, a.chi_held, sizeof(double) * nE, hipMemcpyDeviceToHost, st));
        LB_HIP(hipMemcpyAsync(h_state, a.est, state_bytes, hipMemcpyDeviceToHost, st));
        LB_HIP(hipStreamSynchronize(st));
        return HVO_OK;
    };
    // EdgeSE3ProjectXYZ::isDepthPositive at the estimate in h_state
    auto depth_positive = [&](int e) {
        const LbEdge &E = H.edge[e];
        double Rt[12]; const double *p = h_state + (size_t)E.kf * 8;
        quat_to_R(p, Rt); Rt[9] = p[4]; Rt[10] = p[5]; Rt[11] = p[6];
        double Y[3]; se3_map(Rt, h_state + (size_t)nkf * 8 + (size_t)E.lm * 6, Y);
        return Y[2] > 0.0;
    };
    write_counts();
    bool stopped_between = false;
    for (int rnd = 0; rnd < 2; rnd++) {
        int n_active = 0;
        for (int e = 0; e < nE; e++) n_active += !H.level[e];
        a.robust = rnd == 0;
        double lambda = 0.0, ni = 2.0, cur = 0.0; int nbad = 0, its = 0, trials = 0; bool ok = true;
        for (int it = 0; n_active > 0 && it < P.iterations[rnd]; it++) {
            if (poll()) break;                                                  // sparse_optimizer.cpp:376
            if (!ok) break;
            // ---- linearise at the estimate
            LB_HIP(hipEventRecord(B->evg[0], st));
            k_lba_poses<<<blocks((long long)nkf * 13, LBA_THREADS), LBA_THREADS, 0, st>>>(a, 0, 1);
            k_lba_edges<true><<<blocks(nE, LBA_THREADS), LBA_THREADS, 0, st>>>(a);
            if (nP) k_lba_pairs<<<blocks(nP, 64), 64, 0, st>>>(a);
            k_lba_build<<<blocks(nlm, 64), 64, 0, st>>>(a);
            k_lba_diag<<<nf, 64, 0, st>>>(a);
            k_lba_sum<<<1, LBA_THREADS, 0, st>>>(a);
            LB_HIP(hipEventRecord(B->evg[1], st));
            if ((rc = fetch_out())) return rc;
            { float ms = 0.f; (void)hipEventElapsedTime(&ms, B->evg[0], B->evg[1]); B->prof_ms[0] += ms; B->prof_n[0]++; }
            cur = h_out[0];
            const double ini = cur;
            if (it == 0) { lambda = 1e-5 * h_out[3]; ni = 2.0; nbad = 0; }
            double rho = 0.0; int q = 0;
            while (true) {
                LB_HIP(hipEventRecord(B->evg[0], st));
                k_lba_invert<<<blocks(nlm, 64), 64, 0, st>>>(a, lambda);
                k_lba_reduce<<<dim3(nf, nf), 64, 0, st>>>(a, lambda);
                LB_HIP(hipEventRecord(B->evg[2], st));
                k_lba_solve<<<1, LBA_THREADS, 0, st>>>(a);
                LB_HIP(hipEventRecord(B->evg[3], st));
                k_lba_update<<<blocks(nlm + nkf, 64), 64, 0, st>>>(a, lambda);
                k_lba_poses<<<blocks((long long)nkf * 13, LBA_THREADS), LBA_THREADS, 0, st>>>(a, 1, 0);
                k_lba_edges<false><<<blocks(nE, LBA_THREADS), LBA_THREADS, 0, st>>>(a);
                k_lba_sum<<<1, LBA_THREADS, 0, st>>>(a);
                LB_HIP(hipEventRecord(B->evg[1], st));
                if ((rc = fetch_out())) return rc;
                { float ms = 0.f; (void)hipEventElapsedTime(&ms, B->evg[0], B->evg[1]); B->prof_ms[1] += ms; (void)hipEventElapsedTime(&ms, B->evg[2], B->evg[3]); B->prof_ms[2] += ms; B->prof_n[1]++; }
                trials++;
                double tmp = h_out[0];
                if (!(h_out[2] > 0.5)) tmp = 1.7976931348623157e308;
                const double scale = h_out[1] + 1e-3;
                rho = (cur - tmp) / scale;
                if (rho > 0 && std::isfinite(tmp)) {
                    double alpha = 1. - pow(2 * rho - 1, 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha); ni = 2.0; cur = tmp;
                    LB_HIP(hipMemcpyAsync(a.est, a.trial, state_bytes, hipMemcpyDeviceToDevice, st));
                } else { lambda *= ni; ni *= 2; }
                q++;
                if (!(rho < 0 && q < P.max_trials && !poll())) break;             // optimization_algorithm_levenberg.cpp:149
            }
            its++;
            if (q == P.max_trials || rho == 0) { ok = false; continue; }
            if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
            if (nbad >= 3) ok = false;
        }
        R->iterations[rnd] = its; R->trials[rnd] = trials; R->lambda[rnd] = lambda; R->chi2[rnd] = cur; R->rounds = rnd + 1;
        if (rnd == 1) break;
        if (poll()) { stopped_between = true; break; }                          // :3650
        // ---- the classification of :3656-3743
        if ((rc = fetch_held())) return rc;
        for (int o = 0; o < n_pt_obs; o++) { const int e = H.pt_edge[o]; if (h_chi[e] > P.chi2_gate[0] || !depth_positive(e)) H.level[e] = 1; }
        for (int o = 0; o < n_ln_obs; o++) {
            const int e1 = H.ln_start_edge[o], e2 = H.ln_end_edge[o];
            if (e1 < 0) continue;
            if (h_chi[e1] > P.chi2_gate[1] || h_chi[e2] > P.chi2_gate[1]) { H.level[e1] = 1; H.level[e2] = 1; }
        }
        for (int o = 0; o < n_par; o++) { const int e = H.par_edge[o]; if (e >= 0 && h_chi[e] > P.chi2_gate[2]) H.level[e] = 1; }
        for (int o = 0; o < n_perp; o++) { const int e = H.perp_edge[o]; if (e >= 0 && h_chi[e] > P.chi2_gate[2]) H.level[e] = 1; }
        memcpy(B->h_pin + p_in + o_level, H.level.data(), nE);
        LB_HIP(hipMemcpyAsync(B->d_in + o_level, B->h_pin + p_in + o_level, nE, hipMemcpyHostToDevice, st));
    }
    (void)stopped_between;
    // ---- the erase tests of :3753-3847 and the write-back of :3903-3939
    if ((rc = fetch_held())) return rc;
    LB_HIP(hipEventRecord(B->ev1, st));
    LB_HIP(hipEventSynchronize(B->ev1));
    (void)hipEventElapsedTime(&B->prof_ms[3], B->ev0, B->ev1);
    B->last_ms = B->prof_ms[0] + B->prof_ms[1];
    for (int o = 0; o < n_pt_obs; o++) { const int e = H.pt_edge[o]; R->pt_erase[o] = h_chi[e] > P.chi2_gate[0] || !depth_positive(e); }
    for (int o = 0; o < n_ln_obs; o++) { const int e = H.ln_start_edge[o]; R->ln_erase[o] = e >= 0 && h_chi[e] > P.chi2_gate[1]; }        // reading 3
    for (int i = 0; i < nl; i++) { const int e = H.manh_edge[i]; R->manh_erase[i] = e >= 0 && h_chi[e] > P.chi2_gate[2]; }
    for (int o = 0; o < n_par; o++) { const int e = H.par_edge[o]; R->par_erase[o] = e >= 0 && h_chi[e] > P.chi2_gate[2]; }
    for (int o = 0; o < n_perp; o++) { const int e = H.perp_edge[o]; R->perp_erase[o] = e >= 0 && h_chi[e] > P.chi2_gate[2]; }
    for (int k = 0; k < nkf; k++) {
        const double *p = h_state + (size_t)k * 8;
        double Rm[9]; quat_to_R(p, Rm);
        double *T = R->Tcw_d + 12 * (size_t)k;
        for (int r = 0; r < 3; r++) { T[4 * r] = Rm[3 * r]; T[4 * r + 1] = Rm[3 * r + 1]; T[4 * r + 2] = Rm[3 * r + 2]; T[4 * r + 3] = p[4 + r]; }
        for (int i = 0; i < 12; i++) R->Tcw_f[12 * (size_t)k + i] = (float)T[i];
    }
    const double *X = h_state + (size_t)nkf * 8;
    for (size_t i = 0; i < (size_t)nl * 6; i++) { R->ln_f[i] = (float)G->ln_pos[i]; R->ln_d[i] = G->ln_pos[i]; }
    for (int l = 0; l < nlm; l++) {
        const int line = H.lm_line[l];
        if (line < 0) for (int i = 0; i < 3; i++) { R->pt_d[3 * (size_t)l + i] = X[6 * (size_t)l + i]; R->pt_f[3 * (size_t)l + i] = (float)X[6 * (size_t)l + i]; }
        else for (int i = 0; i < 6; i++) { R->ln_d[6 * (size_t)line + i] = X[6 * (size_t)l + i]; R->ln_f[6 * (size_t)line + i] = (float)X[6 * (size_t)l + i]; }
    }
    R->stopped_at = poll.first;
    R->status = HVO_LBA_OPTIMISED;
    return HVO_OK;
}
