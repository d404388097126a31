// line_opt.hip -- the two per-frame steps between the Frame constructor and Track() (reference src/Tracking.cc:270-335):
//   k_ls_pairs   Manhattan::computeStructConstrains(frame, k, par, perp) for every key line k (src/Manhattan.cpp:107-161, computeAngle /
//                computeAngle2D :1054-1087): one thread per ordered pair (k, i) writes one byte of the dense relation matrix
//   k_line_opt   Optimizer::LineOptStruct(Frame *) (src/Optimizer.cc:1480-1876): one workgroup of LS_THREADS threads per frame, the
//                whole call in one launch.  The Hessian is block-diagonal, one 6 x 6 block per line (both end points of a line against
//                fixed measurements), coupled only by Levenberg's global lambda and chi2:
//     system pass   a wave takes lines wave, wave + 4, ...; its lanes take the line's edges (lane l scans partners l, l + 64, ... of
//                   the row); the line's 12 perturbed end-point pairs (+-1e-9 per coordinate, core/base_binary_edge.hpp) are the
//                   same for every edge of the line; upper H (21), b (6), robust chi2 (1) are added per lane in partner order and
//                   halved over the wave with __shfl_down
//     trial         thread t solves the blocks of lines t, t + 256, ... (LDL^T without pivoting) and forms the trial end points; the
//                   chi pass is the system pass without Jacobians
//     sums          chi2 and computeScale over the lines: thread t adds lines t, t + 256, ... in order, a wave halves, the four waves
//                   are added in order -- the same bytes give the same result on every run and in all three forms
//   Per-line state (estimate, trial, H | b) lies in the call's device scratch, edge levels in a byte matrix beside rel.
// All arithmetic in double, uncontracted.  Readings (tests/line_opt_ref.py restates the same): a solve fails when a
// pivot is exactly 0 or not finite, in any line's block; the step of a failed solve is taken as zero (the trial is rejected either way);
// classification re-evaluates an edge at the end points of the round's last computeActiveErrors instead of storing _error.
#include "frame_view.hpp"
#include "staged_call.hpp"
#include "se3quat.hpp"        // huber, wave_sum_down
#include <math.h>
#include <cmath>
#include <string.h>
#include <string>
#include <vector>

#define LS_THREADS 256
#define LS_WAVES (LS_THREADS / 64)
#define LS_MAX_LINES 4096
#define LS_DELTA 1e-9

struct LsFrame {                       // one frame, every pointer a device pointer
    int n_cap;                         // the caller's n_lines: the side (and row stride) of rel
    const int *d_nkl;                  // resident count that caps it (may be null)
    const double *linefn; hvo_line3d *l3d;
    int8_t *rel; uint8_t *lev;         // n_cap x n_cap: the relation, and per pair 0 no edge / 1 active edge / 2 edge at level 1
    double *est, *trial, *Hb;          // n_cap x 6, n_cap x 6, n_cap x 27
    uint8_t *ent;                      // n_cap x 2: the line has vertices, the line is active in this round
    double *out6;                      // n_cap x 6 (may be null)
};

struct LsArgs {
    const LsFrame *frames; hvo_line_opt_result *res;
    double cos_par, cos_perp, delta, chi2_reject;
    float chi2_round[2];
    int min_constraints, iterations, row_rule;
};

static __device__ __forceinline__ int ls_count(const LsFrame &F)
{
    int n = F.n_cap;
    if (F.d_nkl) { const int c = *F.d_nkl; n = n < c ? n : (c < 0 ? 0 : c); }
    return n;
}

// ---- part 1 ----
__global__ __launch_bounds__(256) void k_ls_pairs(LsArgs A)
{
    const LsFrame &F = A.frames[blockIdx.x];
    const int n = ls_count(F), cap = F.n_cap;
    const long long total = (long long)cap * cap;
    for (long long p = (long long)blockIdx.y * 256 + threadIdx.x; p < total; p += (long long)gridDim.y * 256) {
        const int k = (int)(p / cap), i = (int)(p - (long long)k * cap);
        int8_t r = 0;
        if (k < n && i < n && i != k) {
            const float *qk = F.l3d[k].line_eq, *qi = F.l3d[i].line_eq;
            const bool skip = A.row_rule == HVO_LINE_STRUCT_ROW_Z0 ? (qk[2] == 0.0f) : (qk[0] == -1.0f && qk[1] == -1.0f && qk[2] == -1.0f);
            if (!skip) {
                const double *fk = F.linefn + 3 * (size_t)k, *fi = F.linefn + 3 * (size_t)i;
                const double kx = fk[0] / fk[2], ky = fk[1] / fk[2], ix = fi[0] / fi[2], iy = fi[1] / fi[2];
                const double a2 = fabs((ix * kx + iy * ky) / (sqrt(ix * ix + iy * iy) * sqrt(kx * kx + ky * ky)));
                const double k0 = qk[0], k1 = qk[1], k2 = qk[2], i0 = qi[0], i1 = qi[1], i2 = qi[2];
                const double a3 = fabs(((i0 * k0 + i1 * k1) + i2 * k2) / (sqrt((i0 * i0 + i1 * i1) + i2 * i2) * sqrt((k0 * k0 + k1 * k1) + k2 * k2)));
                if (a2 < A.cos_perp && a3 < A.cos_perp) r = 2;
                else if (a2 > A.cos_par && a3 > A.cos_par) r = 1;
            }
        }
        F.rel[p] = r;
    }
}

// ---- part 2 ----
struct LsShared {
    double lv[LS_MAX_LINES];           // one double per line, summed by ls_reduce_lines
    double red[LS_WAVES];
    double sum;
    int cnt[4];
    int go, fail, accept;
};

// ComputeAngle3D of l = end - start against m (include/g2oMSC.h:25-34); nm = |m|
static __device__ __forceinline__ double ls_cos(const double *s, const double *e, const double *m, double nm)
{
    const double l0 = e[0] - s[0], l1 = e[1] - s[1], l2 = e[2] - s[2];
    const double dot = (m[0] * l0 + m[1] * l1) + m[2] * l2;
    const double nl = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
    return fabs(dot / (nm * nl));
}
static __device__ __forceinline__ double ls_err(int kind, const double *p, const double *m, double nm)
{
    const double c = ls_cos(p, p + 3, m, nm);
    return kind == 1 ? 1 - c : c;
}
static __device__ __forceinline__ void ls_meas(const LsFrame &F, int i, double *m, double &nm)
{
    const float *q = F.l3d[i].line_eq;
    m[0] = (double)q[0]; m[1] = (double)q[1]; m[2] = (double)q[2];
    nm = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
}
// sum of sh.lv[0..n) -> return value on every thread: thread t adds lines t, t + 256, ... in order, a wave halves, the waves in order
static __device__ double ls_reduce_lines(LsShared &sh, int n)
{
    const int tid = threadIdx.x;
    double x = 0.0;
    for (int k = tid; k < n; k += LS_THREADS) x = x + sh.lv[k];
    x = wave_sum_down(x);
    __syncthreads();
    if ((tid & 63) == 0) sh.red[tid >> 6] = x;
    __syncthreads();
    if (tid == 0) sh.sum = ((sh.red[0] + sh.red[1]) + sh.red[2]) + sh.red[3];
    __syncthreads();
    const double r = sh.sum;
    __syncthreads();
    return r;
}

// robust chi2 of line k's active edges at the end points p -> sh.lv[k] (0 for a line that is not active); with_sys: H | b to F.Hb too
template <bool with_sys>
static __device__ void ls_line_pass(const LsArgs &A, const LsFrame &F, LsShared &sh, int n, const double *pts)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cap = F.n_cap;
    for (int k = wave; k < n; k += LS_WAVES) {
        if (!F.ent[2 * k] || (!with_sys && !F.ent[2 * k + 1])) { if (lane == 0) sh.lv[k] = 0.0; continue; }
        double p[6];
        for (int j = 0; j < 6; j++) p[j] = pts[6 * (size_t)k + j];
        double acc[28]; int cnt = 0;
        for (int j = 0; j < 28; j++) acc[j] = 0.0;
        for (int i = lane; i < n; i += 64) {
            if (F.lev[(size_t)k * cap + i] != 1) continue;
            const int kind = F.rel[(size_t)k * cap + i] < 0 ? -F.rel[(size_t)k * cap + i] : F.rel[(size_t)k * cap + i];
            double m[3], nm; ls_meas(F, i, m, nm);
            const double e0 = ls_err(kind, p, m, nm);
            const double c = e0 * e0;
            double r0, r1; huber(c, A.delta, r0, r1);
            acc[27] = acc[27] + r0; cnt++;
            if (with_sys) {
                double J[6];
                const double scalar = 1.0 / (2 * LS_DELTA);
                for (int d = 0; d < 6; d++) {                                // central differences, vertex 0 then vertex 1
                    double q[6];
                    for (int j = 0; j < 6; j++) q[j] = p[j];
                    q[d] = p[d] + LS_DELTA; const double e1 = ls_err(kind, q, m, nm);
                    q[d] = p[d] - LS_DELTA; const double e2 = ls_err(kind, q, m, nm);
                    J[d] = scalar * (e1 - e2);
                }
                int h = 0;
                for (int a = 0; a < 6; a++) {
                    for (int b = a; b < 6; b++, h++) acc[h] = acc[h] + J[a] * r1 * J[b];
                    acc[21 + a] = acc[21 + a] - r1 * (J[a] * e0);
                }
            }
        }
        for (int j = with_sys ? 0 : 27; j < 28; j++) acc[j] = wave_sum_down(acc[j]);
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if (lane == 0) {
            sh.lv[k] = acc[27];
            if (with_sys) {
                for (int j = 0; j < 27; j++) F.Hb[27 * (size_t)k + j] = acc[j];
                F.ent[2 * k + 1] = cnt > 0;
            }
        }
    }
    __syncthreads();
}

// one line's block: (H + lam I) x = b by LDL^T without pivoting; false when a pivot is exactly 0 or not finite
static __device__ bool ls_solve6(const double *Hb, double lam, double *x)
{
    double H[36], L[36], D[6], y[6]; bool ok = true;
    int h = 0;
    for (int i = 0; i < 6; i++) for (int j = i; j < 6; j++, h++) { H[6 * i + j] = Hb[h]; H[6 * j + i] = Hb[h]; }
    for (int j = 0; j < 6; j++) H[7 * j] = H[7 * j] + lam;
    // ldlt6_solve's text (se3quat.hpp) with this call's pivot rule, kept in place: through the shared function k_line_opt is scheduled
    // differently and its 256-frame batch measured above both parent runs (profiles/shared_readings.txt)
    for (int j = 0; j < 6; j++) {
        double s = H[6 * j + j];
        for (int k = 0; k < j; k++) s = s - L[6 * j + k] * L[6 * j + k] * D[k];
        D[j] = s;
        if (s == 0.0 || !isfinite(s)) ok = false;
        for (int i = j + 1; i < 6; i++) {
            double s2 = H[6 * i + j];
            for (int k = 0; k < j; k++) s2 = s2 - L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = s2 / D[j];
        }
    }
    const double *b = Hb + 21;
    for (int i = 0; i < 6; i++) { double s = b[i]; for (int k = 0; k < i; k++) s = s - L[6 * i + k] * y[k]; y[i] = s; }
    for (int i = 5; i >= 0; i--) { double s = y[i] / D[i]; for (int k = i + 1; k < 6; k++) s = s - L[6 * k + i] * x[k]; x[i] = s; }
    return ok;
}

__global__ __launch_bounds__(LS_THREADS) void k_line_opt(LsArgs A)
{
    __shared__ LsShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LsFrame &F = A.frames[blockIdx.x];
    hvo_line_opt_result *res = A.res + blockIdx.x;
    const int n = ls_count(F), cap = F.n_cap;
    if (tid == 0) { sh.cnt[0] = sh.cnt[1] = sh.cnt[2] = sh.cnt[3] = 0; sh.go = sh.fail = sh.accept = 0; }
    __syncthreads();

    // ---- the graph (Optimizer.cc:1542-1707): a wave per line, its lanes over the row ----
    for (int k = wave; k < n; k += LS_WAVES) {
        int c = 0;
        for (int i = lane; i < n; i += 64) c += F.rel[(size_t)k * cap + i] != 0;
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        c = __shfl(c, 0, 64);
        const hvo_line3d &R = F.l3d[k];
        const double s0 = R.A[0], s1 = R.A[1], s2 = R.A[2], e0 = R.B[0], e1 = R.B[1], e2 = R.B[2];
        bool in = c >= A.min_constraints;
        if (s2 == 0.0 || s0 == -1.0 || e2 == 0.0 || e0 == -1.0) in = false;
        if (fabs(e0 - s0) < 0.00001 && fabs(e1 - s1) < 0.00001) in = false;
        if (isnan(s0) || isnan(s1) || isnan(s2) || isnan(e0) || isnan(e1) || isnan(e2)) in = false;
        int npar = 0, nperp = 0;
        for (int i = lane; i < n; i += 64) {
            const int8_t r = F.rel[(size_t)k * cap + i];
            uint8_t lv = 0;
            if (in && r > 0) {                                               // a slot holding -1 gives no edge (:1585)
                const float *q = F.l3d[i].line_eq;
                if (!((double)q[2] == 0.0 || (double)q[0] == -1.0)) { lv = 1; if (r == 1) npar++; else nperp++; }
            }
            F.lev[(size_t)k * cap + i] = lv;
        }
        for (int off = 32; off > 0; off >>= 1) { npar += __shfl_down(npar, off, 64); nperp += __shfl_down(nperp, off, 64); }
        if (lane == 0) {
            F.ent[2 * k] = in; F.ent[2 * k + 1] = 0;
            F.est[6 * (size_t)k + 0] = s0; F.est[6 * (size_t)k + 1] = s1; F.est[6 * (size_t)k + 2] = s2;
            F.est[6 * (size_t)k + 3] = e0; F.est[6 * (size_t)k + 4] = e1; F.est[6 * (size_t)k + 5] = e2;
            for (int j = 0; j < 6; j++) F.trial[6 * (size_t)k + j] = F.est[6 * (size_t)k + j];
            atomicAdd(&sh.cnt[0], in ? 1 : 0); atomicAdd(&sh.cnt[1], npar); atomicAdd(&sh.cnt[2], nperp);
        }
    }
    __syncthreads();
    const int n_to_opt = sh.cnt[0], n_par = sh.cnt[1], n_perp = sh.cnt[2], n_edges = n_par + n_perp;
    if (tid == 0) {
        memset(res, 0, sizeof(*res));
        res->n_lines = n; res->n_lines_to_opt = n_to_opt; res->n_edges = n_edges; res->n_par_edges = n_par; res->n_perp_edges = n_perp;
        res->status = HVO_OK;
    }
    __syncthreads();

    for (int rnd = 0; rnd < 2; rnd++) {
        double lam = 0.0, ni = 2.0; int nbad_it = 0, its = 0, trials = 0; double chi_final = 0.0;      // thread 0's
        for (int it = 0; it < A.iterations; it++) {
            ls_line_pass<true>(A, F, sh, n, F.est);                          // computeActiveErrors + buildSystem
            int n_act = 0;
            double md = 0.0;
            for (int k = tid; k < n; k += LS_THREADS) if (F.ent[2 * k] && F.ent[2 * k + 1]) {
                n_act++;
                const double *Hb = F.Hb + 27 * (size_t)k;
                md = fmax(fabs(Hb[0]), md); md = fmax(fabs(Hb[6]), md); md = fmax(fabs(Hb[11]), md);
                md = fmax(fabs(Hb[15]), md); md = fmax(fabs(Hb[18]), md); md = fmax(fabs(Hb[20]), md);
            }
            if (it == 0) {                                                   // the active set and computeLambdaInit (tau = 1e-5): a maximum, any order
                for (int off = 32; off > 0; off >>= 1) { md = fmax(md, __shfl_down(md, off, 64)); n_act += __shfl_down(n_act, off, 64); }
                if (lane == 0) { sh.red[wave] = md; atomicAdd(&sh.cnt[3], n_act); }
                __syncthreads();
                if (tid == 0) { lam = 1e-5 * fmax(fmax(sh.red[0], sh.red[1]), fmax(sh.red[2], sh.red[3])); ni = 2.0; nbad_it = 0; }
                n_act = sh.cnt[3];
                __syncthreads();
                if (tid == 0) sh.cnt[3] = 0;
                __syncthreads();
                if (n_act == 0) break;                                       // "0 vertices to optimize": optimize() returns before anything is computed
            }
            const double ini = ls_reduce_lines(sh, n);
            double cur = ini;
            double rho = 0.0; int q = 0;
            while (true) {                                                   // uniform: every thread follows sh.go
                if (tid == 0) { sh.sum = lam; sh.fail = 0; }
                __syncthreads();
                const double lm = sh.sum;
                __syncthreads();
                bool bad = false;
                for (int k = tid; k < n; k += LS_THREADS) {
                    double sc = 0.0;
                    if (F.ent[2 * k] && F.ent[2 * k + 1]) {
                        double x[6];
                        const double *Hb = F.Hb + 27 * (size_t)k;
                        if (!ls_solve6(Hb, lm, x)) bad = true;
                        for (int j = 0; j < 6; j++) { F.trial[6 * (size_t)k + j] = F.est[6 * (size_t)k + j] + x[j]; sc = sc + x[j] * (lm * x[j] + Hb[21 + j]); }
                    }
                    sh.lv[k] = sc;
                }
                if (bad) atomicOr(&sh.fail, 1);
                __syncthreads();
                const int fail = sh.fail;
                if (fail) for (int k = tid; k < n; k += LS_THREADS) {         // the step of a failed solve is zero
                    for (int j = 0; j < 6; j++) F.trial[6 * (size_t)k + j] = F.est[6 * (size_t)k + j];
                    sh.lv[k] = 0.0;
                }
                __syncthreads();
                double scale = ls_reduce_lines(sh, n);                       // computeScale
                ls_line_pass<false>(A, F, sh, n, F.trial);
                double tmp = ls_reduce_lines(sh, n);
                if (tid == 0) {
                    if (fail) tmp = 1.7976931348623157e308;
                    scale = scale + 1e-3;
                    rho = (cur - tmp) / scale;
                    if (rho > 0 && isfinite(tmp)) {
                        double alpha = 1.0 - pow(2 * rho - 1, 3.0);
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lam = lam * fmax(1.0 / 3.0, alpha); ni = 2.0; cur = tmp; sh.accept = 1;
                    } else { lam = lam * ni; ni = ni * 2; sh.accept = 0; }
                    q++; trials++;
                    sh.go = (rho < 0 && q < 10) ? 1 : 0;
                }
                __syncthreads();
                const int go = sh.go;
                if (sh.accept) for (int k = tid; k < n; k += LS_THREADS) if (F.ent[2 * k] && F.ent[2 * k + 1])
                    for (int j = 0; j < 6; j++) F.est[6 * (size_t)k + j] = F.trial[6 * (size_t)k + j];
                __syncthreads();
                if (!go) break;
            }
            if (tid == 0) {
                its++; chi_final = cur;
                int ok = 1;
                if (q == 10 || rho == 0) ok = 0;
                else {
                    if ((ini - cur) * 1e3 < ini) nbad_it++; else nbad_it = 0;
                    if (nbad_it >= 3) ok = 0;
                }
                sh.go = ok;
            }
            __syncthreads();
            const int go = sh.go;
            __syncthreads();
            if (!go) break;
        }
        // ---- classification (Optimizer.cc:1727-1792) and, on the same _error, the final rejection (:1834-1851) ----
        int flagged = 0;
        for (int k = wave; k < n; k += LS_WAVES) {
            if (!F.ent[2 * k]) continue;
            for (int i = lane; i < n; i += 64) {
                const uint8_t lv = F.lev[(size_t)k * cap + i];
                if (!lv) continue;
                const int8_t r = F.rel[(size_t)k * cap + i];
                const int kind = r < 0 ? -r : r;
                double m[3], nm; ls_meas(F, i, m, nm);
                const double e0 = ls_err(kind, (lv == 1 ? F.trial : F.est) + 6 * (size_t)k, m, nm);
                const double chi = e0 * e0;
                const bool bad = (float)chi > A.chi2_round[rnd];
                flagged += bad;
                F.lev[(size_t)k * cap + i] = bad ? 2 : 1;
                F.rel[(size_t)k * cap + i] = (int8_t)((chi >= 0.0 && chi <= A.chi2_reject) ? kind : -kind);
            }
        }
        for (int off = 32; off > 0; off >>= 1) flagged += __shfl_down(flagged, off, 64);
        if (lane == 0) atomicAdd(&sh.cnt[3], flagged);
        __syncthreads();
        if (tid == 0) {
            res->iterations[rnd] = its; res->trials[rnd] = trials; res->lambda[rnd] = its ? lam : 0.0; res->chi2[rnd] = chi_final;
            res->n_flagged[rnd] = sh.cnt[3]; res->rounds = rnd + 1;
            sh.cnt[3] = 0;
        }
        __syncthreads();
        if (n_edges < 10) break;                                             // optimizer.edges().size() < 10
    }

    // ---- write-back (Optimizer.cc:1858-1874): the second operand asks for vertex 0 ----
    const int wb = n > 0 && F.ent[0];
    if (tid == 0) res->written_back = wb;
    for (int k = tid; k < cap; k += LS_THREADS) {
        double o[6] = { 0, 0, 0, 0, 0, 0 };
        if (k < n) {
            hvo_line3d &R = F.l3d[k];
            if (wb && F.ent[2 * k]) {
                for (int j = 0; j < 3; j++) { R.A[j] = F.est[6 * (size_t)k + j]; R.B[j] = F.est[6 * (size_t)k + 3 + j]; }
            }
            for (int j = 0; j < 3; j++) { o[j] = R.A[j]; o[3 + j] = R.B[j]; }
        }
        if (F.out6) for (int j = 0; j < 6; j++) F.out6[6 * (size_t)k + j] = o[j];
    }
}

// k_line_opt's tail for a call without part 2: the end points as they are
__global__ void k_ls_copy6(LsArgs A)
{
    const LsFrame &F = A.frames[blockIdx.x];
    const int n = ls_count(F);
    if (threadIdx.x == 0) { hvo_line_opt_result *res = A.res + blockIdx.x; memset(res, 0, sizeof(*res)); res->n_lines = n; res->status = HVO_OK; }
    for (int k = threadIdx.x; k < F.n_cap; k += blockDim.x) {
        if (!F.out6) break;
        for (int j = 0; j < 3; j++) { F.out6[6 * (size_t)k + j] = k < n ? F.l3d[k].A[j] : 0.0; F.out6[6 * (size_t)k + 3 + j] = k < n ? F.l3d[k].B[j] : 0.0; }
    }
}

// ---- host side ----
extern "C" int hvo_line_struct_default_params(hvo_line_struct_params *p)
{
    if (!p) return HVO_ERR_INVALID_ARG;
    memset(p, 0, sizeof(*p));
    const double deg_th = 3;                                                 // src/Manhattan.cpp:28-30
    p->cos_par = cos(deg_th * 0.0174533); p->cos_perp = cos((90.0 - deg_th) * 0.0174533);
    p->huber_delta = (double)(float)sqrt(0.02);                              // const float thHuberLine = sqrt(0.02)
    p->chi2_reject = 0.02; p->chi2_round[0] = 0.02f; p->chi2_round[1] = 0.01f;
    p->min_constraints = 5; p->iterations = 5; p->row_rule = HVO_LINE_STRUCT_ROW_UNSET;
    p->mode = HVO_LINE_STRUCT_CONSTRAINTS | HVO_LINE_STRUCT_OPTIMIZE;
    return HVO_OK;
}

// Layout of one call in the context's call arena / pinned staging block:
//   [LsFrame x n | per frame: (host form) linefn, records | rel]  up to here the upload (rel only when the caller's is read)
//   [per frame: rel | out6] [results]                              the download; then the kernel's own scratch (lev, est, trial, Hb, ent)
int ls_run(hvo_ctx *ctx, hipStream_t st, const hvo_line_struct_params *params, int n, const int32_t *n_lines, const hvo_line_struct_problem *prob,
           const FrameView *fr, int8_t *const *rel, double *const *l3d_out, hvo_line_opt_result *res, std::string *err)
{
    hvo_line_struct_params P;
    if (params) P = *params; else hvo_line_struct_default_params(&P);
    const bool part1 = (P.mode & HVO_LINE_STRUCT_CONSTRAINTS) != 0, part2 = (P.mode & HVO_LINE_STRUCT_OPTIMIZE) != 0;
    if (!part1 && !part2) { *err = "line structure: mode selects neither part"; return HVO_ERR_INVALID_ARG; }
    if (P.iterations < 0 || (P.row_rule != HVO_LINE_STRUCT_ROW_UNSET && P.row_rule != HVO_LINE_STRUCT_ROW_Z0)) { *err = "line structure: bad params"; return HVO_ERR_INVALID_ARG; }
    struct Pieces { StagePiece<double> fn, out6, est, trial, Hb; StagePiece<hvo_line3d> rec; StagePiece<int8_t> rel; StagePiece<uint8_t> lev, ent; };
    std::vector<Pieces> O((size_t)n);
    StageCarver C(64);
    const auto frames = C.take<LsFrame>((size_t)n);
    int cap_max = 0;
    for (int f = 0; f < n; f++) {
        const int c = n_lines[f];
        if (c < 0) { *err = "line structure: n_lines < 0"; return HVO_ERR_INVALID_ARG; }
        if (c > LS_MAX_LINES) { *err = "line structure: at most 4096 lines per frame"; return HVO_ERR_UNSUPPORTED; }
        if (c && (!rel || !rel[f])) { *err = "line structure: rel is NULL"; return HVO_ERR_INVALID_ARG; }
        if (c && !fr && (!prob[f].lines3d || (part1 && !prob[f].linefn))) { *err = "line structure: a needed array is NULL"; return HVO_ERR_INVALID_ARG; }
        cap_max = c > cap_max ? c : cap_max;
        if (!fr) { O[f].fn = C.take<double>((size_t)c, 3); O[f].rec = C.take<hvo_line3d>((size_t)c); }
    }
    const size_t down0 = C.mark();                                           // rel is the first thing that comes down, and goes up when it is the caller's
    for (int f = 0; f < n; f++) O[f].rel = C.take<int8_t>((size_t)n_lines[f], (size_t)n_lines[f]);
    const size_t up_end = part1 ? down0 : C.mark();
    for (int f = 0; f < n; f++) O[f].out6 = C.take<double>((size_t)n_lines[f], 6);
    const auto results = C.take<hvo_line_opt_result>((size_t)n);
    const size_t down_end = C.mark();
    for (int f = 0; f < n; f++) {
        const size_t c = (size_t)n_lines[f];
        O[f].lev = C.take<uint8_t>(part2 ? c : 0, c); O[f].est = C.take<double>(c, 6); O[f].trial = C.take<double>(c, 6); O[f].Hb = C.take<double>(c, 27);
        O[f].ent = C.take<uint8_t>(c, 2);
    }
    StagedCall sc(ctx, st, "line structure: ", err); int rc;
    if ((rc = sc.begin(C.mark(), up_end, down_end - down0, false))) return rc;     // every piece is copied whole: nothing relies on zero padding
    char *const d = sc.d, *const h = sc.h;
    for (int f = 0; f < n; f++) {
        const size_t c = (size_t)n_lines[f];
        LsFrame &F = *frames.host(h, f); memset(&F, 0, sizeof(F));
        F.n_cap = (int)c;
        if (fr) { F.d_nkl = fr[f].d_nkl; F.linefn = fr[f].fn; F.l3d = fr[f].l3d; }
        else {
            if (c && prob[f].linefn) memcpy(O[f].fn.host(h), prob[f].linefn, c * 24);
            if (c) memcpy(O[f].rec.host(h), prob[f].lines3d, c * sizeof(hvo_line3d));
            F.linefn = O[f].fn.dev(d); F.l3d = O[f].rec.dev(d);
        }
        if (!part1 && c) {
            for (size_t i = 0; i < c * c; i++) { const int8_t v = rel[f][i]; if (v < -2 || v > 2) { *err = "line structure: rel holds a value outside -2 .. 2"; return HVO_ERR_INVALID_ARG; } }
            memcpy(O[f].rel.host(h), rel[f], c * c);
        }
        F.rel = O[f].rel.dev(d); F.lev = O[f].lev.dev(d);
        F.est = O[f].est.dev(d); F.trial = O[f].trial.dev(d); F.Hb = O[f].Hb.dev(d); F.ent = O[f].ent.dev(d);
        F.out6 = O[f].out6.dev(d);
    }
    LsArgs A; memset(&A, 0, sizeof(A));
    A.frames = frames.dev(d); A.res = results.dev(d);
    A.cos_par = P.cos_par; A.cos_perp = P.cos_perp; A.delta = P.huber_delta; A.chi2_reject = P.chi2_reject;
    A.chi2_round[0] = P.chi2_round[0]; A.chi2_round[1] = P.chi2_round[1];
    A.min_constraints = P.min_constraints; A.iterations = P.iterations; A.row_rule = P.row_rule;
    if ((rc = sc.up(0, up_end))) return rc;
    sc.tick();
    if (part1 && cap_max > 0) {
        const long long blocks = ((long long)cap_max * cap_max + 255) / 256;
        hipLaunchKernelGGL(k_ls_pairs, dim3(n, (unsigned)(blocks < 64 ? blocks : 64)), dim3(256), 0, st, A);
    }
    sc.tick();
    if (part2) hipLaunchKernelGGL(k_line_opt, dim3(n), dim3(LS_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_ls_copy6, dim3(n), dim3(256), 0, st, A);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(down0, down_end, &b))) return rc;
    ctx->ls_ms[0] = part1 ? sc.ms[0] : 0.f; ctx->ls_ms[1] = part2 ? sc.ms[1] : 0.f;
    memcpy(res, results.down(b), results.bytes());
    for (int f = 0; f < n; f++) {
        const size_t c = (size_t)n_lines[f];
        if (c) memcpy(rel[f], O[f].rel.down(b), c * c);
        if (c && l3d_out && l3d_out[f]) memcpy(l3d_out[f], O[f].out6.down(b), c * 48);
    }
    return HVO_OK;
}
