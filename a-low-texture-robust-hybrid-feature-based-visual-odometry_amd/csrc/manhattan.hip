// manhattan.hip -- Tracking::TrackManhattanFrame (reference src/Tracking.cc:1172-1348, with ProjectSN2Conic 953-1026, ProjectSN2MF
// 1028-1150 and MeanShift 1152-1170): the Manhattan-frame rotation of every tracked frame from the frame's surface normals
// (vSurfaceNormal = hvo_surface_normals, HVO_STAGE_PLANE_TAIL) and its 3-D lines (mVF3DLines = the good entries of hvo_lines_3d,
// HVO_STAGE_LINES3D).
//
// One workgroup per frame, MF_THREADS threads.  The device function mf_frame runs the whole call:
//   cone pass       per element and axis the ProjectSN2Conic test against R_last (sin 0.2018 for normals, sin 0.1018 for lines);
//                   numInCone counts the normals (ballot + popcount per wave, one LDS slot per wave)
//   threshold       minNumOfSN = size / 20, or (b + a) / 2 of the sorted counts when the middle one is below it (one lane)
//   mean shift      per axis, in axis order: the cone's elements (recomputed, not stored) through the sin 0.2518 test against the
//                   CURRENT R_cm_update, m_j in double, the sums of k, k m_x, k m_y in double over a fixed tree (each thread sums its
//                   own elements in index order, then a halving tree in LDS), then one lane finishes the axis and writes the column
//   completion      the missing column of two found axes and the 3 x 3 polar factor, one lane
//   membership      (only when asked) bit a-1 of an element when it enters ProjectSN2MF's lists for axis a
// The reference's R_cm is a shallow cv::Mat copy of R_cm_update (Tracking.cc:1181), so the mean shift of axis 2 and 3 reads the columns
// that the earlier axes replaced, and fewer than two found axes return R_last with the one found column replaced.
// Float steps use the _rn intrinsics on top of -ffp-contract=off; the readings of OpenCV's arithmetic are DESIGN.md's "Manhattan
// tracking readings".  The host, stream and batch forms launch this kernel alone, so the three give bit-identical results.
#include "hvo_internal.hpp"
#include <math.h>

#define MF_THREADS 512
#define MF_WAVES (MF_THREADS / 64)

struct MfArgs {
    const hvo_surface_normal *sn; int nn; size_t sn_stride;      // normals of frame f at (char *)sn + f * sn_stride
    const hvo_line3d *l3d; int nl; size_t l3d_stride;            // key lines' 3-D lines of frame f; nl = count, or a cap when d_nl is set
    const int *d_nl;                                             // per-frame key-line counts (batch), may be null
    int nframes;
    float R0[9];                                                 // R_last of frame 0, row-major
    double sin_n, sin_l, sin_ms;                                 // sin(0.2018), sin(0.1018), sin(0.2518)
    hvo_mf_result *res;                                          // nframes results
    uint8_t *normal_axes, *line_axes;                            // membership bits of frame 0 (single-frame forms only), may be null
};

struct MfShared {
    float R0[9], R[9], Rax[3][9];      // R_last, R_cm_update, and R_cm as each axis's mean shift read it
    double red[3][MF_THREADS];
    int redc[MF_THREADS];
    int cone[MF_WAVES][3];
    int thr, nl;
};

// n_ini of an element for axis a (x: column a mod 3, y: column (a + 1) mod 3, z: column a - 1 of R, Tracking.cc:1189-1201 + 970-978)
static __device__ __forceinline__ void mf_proj_f(const float *R, int a, float n0, float n1, float n2, float &x, float &y, float &z)
{
    const int cx = a % 3, cy = (a + 1) % 3, cz = a - 1;
    x = __fadd_rn(__fadd_rn(__fmul_rn(R[cx], n0), __fmul_rn(R[3 + cx], n1)), __fmul_rn(R[6 + cx], n2));
    y = __fadd_rn(__fadd_rn(__fmul_rn(R[cy], n0), __fmul_rn(R[3 + cy], n1)), __fmul_rn(R[6 + cy], n2));
    z = __fadd_rn(__fadd_rn(__fmul_rn(R[cz], n0), __fmul_rn(R[3 + cz], n1)), __fmul_rn(R[6 + cz], n2));
}
// the line form: float entries times a double direction, summed in double, stored into a Point3f (Tracking.cc:994-1002)
static __device__ __forceinline__ void mf_proj_d(const float *R, int a, const double d[3], float &x, float &y, float &z)
{
    const int cx = a % 3, cy = (a + 1) % 3, cz = a - 1;
    x = (float)__dadd_rn(__dadd_rn(__dmul_rn((double)R[cx], d[0]), __dmul_rn((double)R[3 + cx], d[1])), __dmul_rn((double)R[6 + cx], d[2]));
    y = (float)__dadd_rn(__dadd_rn(__dmul_rn((double)R[cy], d[0]), __dmul_rn((double)R[3 + cy], d[1])), __dmul_rn((double)R[6 + cy], d[2]));
    z = (float)__dadd_rn(__dadd_rn(__dmul_rn((double)R[cz], d[0]), __dmul_rn((double)R[3 + cz], d[1])), __dmul_rn((double)R[6 + cz], d[2]));
}
// lambda = sqrt(x x + y y) on floats (std::sqrt(float))
static __device__ __forceinline__ float mf_lambda(float x, float y) { return __fsqrt_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y))); }

// RandomLine3d::director = (A - B) / sqrt((A - B).(A - B)) (LineExtractor.cpp:321)
static __device__ __forceinline__ void mf_director(const hvo_line3d &L, double d[3])
{
    const double dx = __dsub_rn(L.A[0], L.B[0]), dy = __dsub_rn(L.A[1], L.B[1]), dz = __dsub_rn(L.A[2], L.B[2]);
    const double s = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
    d[0] = __ddiv_rn(dx, s); d[1] = __ddiv_rn(dy, s); d[2] = __ddiv_rn(dz, s);
}

// an element that passed the sin 0.2518 test: m_j (ProjectSN2MF, Tracking.cc:1062-1069) and its MeanShift weight (1161-1165)
static __device__ __forceinline__ bool mf_mj(float x, float y, float z, float lam, double &k, double &mx, double &my)
{
    const double l = (double)lam;
    const double tan_alfa = __ddiv_rn(l, (double)fabsf(z));
    const double alfa = asin(l);
    const double q = __ddiv_rn(alfa, tan_alfa);
    mx = __ddiv_rn(__dmul_rn(q, (double)x), (double)z);
    my = __ddiv_rn(__dmul_rn(q, (double)y), (double)z);
    if (isnan(mx) || isnan(my)) return false;
    const double nrm = __dsqrt_rn(__dadd_rn(__dmul_rn(mx, mx), __dmul_rn(my, my)));
    k = exp(__dmul_rn(__dmul_rn(-20.0, nrm), nrm));
    return true;
}

static __device__ __forceinline__ void mf_cross(const float *u, const float *v, float *w)
{
    w[0] = __fsub_rn(__fmul_rn(u[1], v[2]), __fmul_rn(u[2], v[1]));
    w[1] = __fsub_rn(__fmul_rn(u[2], v[0]), __fmul_rn(u[0], v[2]));
    w[2] = __fsub_rn(__fmul_rn(u[0], v[1]), __fmul_rn(u[1], v[0]));
}
// cv::determinant of a 3 x 3 CV_32F: cofactor expansion along row 0 in double
static __device__ double mf_det(const float *M)
{
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    const double c0 = __dsub_rn(__dmul_rn(m11, m22), __dmul_rn(m12, m21));
    const double c1 = __dsub_rn(__dmul_rn(m10, m22), __dmul_rn(m12, m20));
    const double c2 = __dsub_rn(__dmul_rn(m10, m21), __dmul_rn(m11, m20));
    return __dadd_rn(__dsub_rn(__dmul_rn(m00, c0), __dmul_rn(m01, c1)), __dmul_rn(m02, c2));
}
// U V^T of the SVD of a nonsingular 3 x 3 = its orthogonal polar factor: Newton's iteration X <- (X + X^-T) / 2 in double
static __device__ void mf_polar(float *M)
{
    double X[9];
    for (int i = 0; i < 9; i++) X[i] = M[i];
    for (int it = 0; it < 64; it++) {
        double C[9];                                             // cofactor matrix: X^-T = C / det
        C[0] = X[4] * X[8] - X[5] * X[7]; C[1] = X[5] * X[6] - X[3] * X[8]; C[2] = X[3] * X[7] - X[4] * X[6];
        C[3] = X[2] * X[7] - X[1] * X[8]; C[4] = X[0] * X[8] - X[2] * X[6]; C[5] = X[1] * X[6] - X[0] * X[7];
        C[6] = X[1] * X[5] - X[2] * X[4]; C[7] = X[2] * X[3] - X[0] * X[5]; C[8] = X[0] * X[4] - X[1] * X[3];
        const double det = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
        double d = 0.0;
        for (int i = 0; i < 9; i++) {
            const double y = 0.5 * (X[i] + C[i] / det);
            d = fmax(d, fabs(y - X[i]));
            X[i] = y;
        }
        if (!(d > 1e-15)) break;                                 // converged (or NaN)
    }
    for (int i = 0; i < 9; i++) M[i] = (float)X[i];
}

// sum of v over the workgroup: each thread's value into LDS, then a halving tree (the same tree for every call)
static __device__ __forceinline__ void mf_tree(MfShared &sh, int tid)
{
    for (int s = MF_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            sh.red[0][tid] = sh.red[0][tid] + sh.red[0][tid + s];
            sh.red[1][tid] = sh.red[1][tid] + sh.red[1][tid + s];
            sh.red[2][tid] = sh.red[2][tid] + sh.red[2][tid + s];
            sh.redc[tid] += sh.redc[tid + s];
        }
        __syncthreads();
    }
}

// Tracking::TrackManhattanFrame for one frame.  sh.R0 holds R_last on entry; sh.R holds the returned R on exit.
static __device__ void mf_frame(MfShared &sh, const MfArgs &a, const hvo_surface_normal *sn, int nn, const hvo_line3d *l3d, int nl,
                                hvo_mf_result *res, uint8_t *nax, uint8_t *lax)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 9) sh.R[tid] = sh.R0[tid];
    __syncthreads();

    // ---- numInCone: the normals in each axis's sin 0.2018 cone (ProjectSN2Conic, Tracking.cc:967-990) ----
    int cnt[3] = { 0, 0, 0 };
    for (int base = 0; base < nn; base += MF_THREADS) {
        const int i = base + tid;
        bool in[3] = { false, false, false };
        if (i < nn) {
            const float n0 = sn[i].normal[0], n1 = sn[i].normal[1], n2 = sn[i].normal[2];
            for (int ax = 1; ax <= 3; ax++) {
                float x, y, z; mf_proj_f(sh.R0, ax, n0, n1, n2, x, y, z);
                in[ax - 1] = (double)mf_lambda(x, y) < a.sin_n;
            }
        }
        for (int k = 0; k < 3; k++) cnt[k] += __popcll(__ballot(in[k]));
    }
    if (lane == 0) { sh.cone[wave][0] = cnt[0]; sh.cone[wave][1] = cnt[1]; sh.cone[wave][2] = cnt[2]; }
    __syncthreads();
    if (tid == 0) {
        int c[3] = { 0, 0, 0 };
        for (int w = 0; w < MF_WAVES; w++) for (int k = 0; k < 3; k++) c[k] += sh.cone[w][k];
        for (int k = 0; k < 3; k++) res->n_in_cone[k] = c[k];
        int thr = nn / 20;                                       // minNumOfSN (Tracking.cc:1215-1226)
        int s0 = c[0], s1 = c[1], s2 = c[2], t;
        if (s0 > s1) { t = s0; s0 = s1; s1 = t; }
        if (s1 > s2) { t = s1; s1 = s2; s2 = t; }
        if (s0 > s1) { t = s0; s0 = s1; s1 = t; }
        if (s1 < thr) thr = (s1 + s0) / 2;
        sh.thr = thr; res->min_num_sn = thr;
    }
    __syncthreads();
    const int thr = sh.thr;

    // ---- per axis: ProjectSN2MF + MeanShift over the cone's normals, then its lines ----
    int n_found = 0; int found[3] = { 0, 0, 0 };
    for (int ax = 1; ax <= 3; ax++) {
        if (tid < 9) sh.Rax[ax - 1][tid] = sh.R[tid];
        __syncthreads();
        const float *Rc = sh.Rax[ax - 1];
        double sk = 0.0, skx = 0.0, sky = 0.0; int kept = 0;
        const int ne = nn + nl;
        for (int e = tid; e < ne; e += MF_THREADS) {
            float x, y, z;
            if (e < nn) {
                const float n0 = sn[e].normal[0], n1 = sn[e].normal[1], n2 = sn[e].normal[2];
                mf_proj_f(sh.R0, ax, n0, n1, n2, x, y, z);
                if (!((double)mf_lambda(x, y) < a.sin_n)) continue;
                mf_proj_f(Rc, ax, n0, n1, n2, x, y, z);
            } else {
                const hvo_line3d &L = l3d[e - nn];
                if (!L.good) continue;
                double d[3]; mf_director(L, d);
                mf_proj_d(sh.R0, ax, d, x, y, z);
                if (!((double)mf_lambda(x, y) < a.sin_l)) continue;
                mf_proj_d(Rc, ax, d, x, y, z);
            }
            const float lam = mf_lambda(x, y);
            if (!((double)lam < a.sin_ms)) continue;
            double k, mx, my;
            if (!mf_mj(x, y, z, lam, k, mx, my)) continue;
            kept++;
            sk = sk + k; skx = skx + k * mx; sky = sky + k * my;
        }
        sh.red[0][tid] = sk; sh.red[1][tid] = skx; sh.red[2][tid] = sky; sh.redc[tid] = kept;
        __syncthreads();
        mf_tree(sh, tid);
        if (tid == 0) {
            const int cntk = sh.redc[0];
            res->n_selected[ax - 1] = cntk;
            float rec[3] = { 0.f, 0.f, 0.f }; float den = 0.f;
            if (cntk > thr) {
                const double Sk = sh.red[0][0];
                const double cx = sh.red[1][0] / Sk, cy = sh.red[2][0] / Sk;       // centerOfShift = nominator / denominator
                den = (float)(Sk / (double)cntk);                                   // density = denominator / numPoint
                const float alfa = (float)__dsqrt_rn(__dadd_rn(__dmul_rn(cx, cx), __dmul_rn(cy, cy)));   // float alfa = norm(s_j)
                const float t = __fdiv_rn(tanf(alfa), alfa);                       // tan(float) / float
                const float ma_x = (float)__dmul_rn((double)t, cx), ma_y = (float)__dmul_rn((double)t, cy);
                const int cxi = ax % 3, cyi = (ax + 1) % 3, czi = ax - 1;
                float v[3];
                for (int r = 0; r < 3; r++)                                         // R_mc * (ma_x, ma_y, 1)
                    v[r] = (float)__dadd_rn(__dadd_rn(__dmul_rn((double)Rc[3 * r + cxi], (double)ma_x), __dmul_rn((double)Rc[3 * r + cyi], (double)ma_y)),
                                            (double)Rc[3 * r + czi]);
                const double nv = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)v[0], (double)v[0]), __dmul_rn((double)v[1], (double)v[1])),
                                                       __dmul_rn((double)v[2], (double)v[2])));
                for (int r = 0; r < 3; r++) rec[r] = (float)__ddiv_rn((double)v[r], nv);
            }
            // sum(R_cm_Rec)[0] != 0 (Tracking.cc:1258)
            const bool f = __dadd_rn(__dadd_rn((double)rec[0], (double)rec[1]), (double)rec[2]) != 0.0;
            res->density[ax - 1] = f ? den : 0.f;
            for (int r = 0; r < 3; r++) res->axis_vec[ax - 1][r] = f ? rec[r] : 0.f;
            if (f) for (int r = 0; r < 3; r++) sh.R[3 * r + ax - 1] = rec[r];
            res->found[ax - 1] = f ? 1 : 0;
        }
        __syncthreads();
    }

    // ---- completion (Tracking.cc:1283-1340) ----
    if (tid == 0) {
        for (int k = 0; k < 3; k++) { found[k] = res->found[k]; n_found += found[k]; }
        float *M = sh.R;
        if (n_found >= 2) {
            if (n_found == 2) {
                float c0[3] = { M[0], M[3], M[6] }, c1[3] = { M[1], M[4], M[7] }, c2[3] = { M[2], M[5], M[8] }, w[3];
                int col;
                if (found[0] && found[1]) { mf_cross(c0, c1, w); col = 2; }          // v3 = v1 x v2
                else if (found[1] && found[2]) { mf_cross(c2, c1, w); col = 0; }     // v1 = v3 x v2
                else { mf_cross(c0, c2, w); col = 1; }                               // v2 = v1 x v3
                for (int r = 0; r < 3; r++) M[3 * r + col] = w[r];
                if (fabs(mf_det(M) + 1.0) < 0.5) for (int r = 0; r < 3; r++) M[3 * r + col] = -w[r];
            }
            mf_polar(M);
        }
        for (int i = 0; i < 9; i++) res->R[i] = M[i];
        res->n_found = n_found;
        res->tracked = n_found >= 2 ? 1 : 0;
        res->status = HVO_OK;
    }
    __syncthreads();

    // ---- membership: bit a-1 where the element enters ProjectSN2MF's lists for axis a (Tracking.cc:1058-1060, 1070-1119) ----
    if (nax)
        for (int i = tid; i < nn; i += MF_THREADS) {
            const float n0 = sn[i].normal[0], n1 = sn[i].normal[1], n2 = sn[i].normal[2];
            unsigned m = 0;
            for (int ax = 1; ax <= 3; ax++) {
                float x, y, z; mf_proj_f(sh.R0, ax, n0, n1, n2, x, y, z);
                if (!((double)mf_lambda(x, y) < a.sin_n)) continue;
                mf_proj_f(sh.Rax[ax - 1], ax, n0, n1, n2, x, y, z);
                if ((double)mf_lambda(x, y) < a.sin_ms) m |= 1u << (ax - 1);
            }
            nax[i] = (uint8_t)m;
        }
    if (lax)
        for (int j = tid; j < nl; j += MF_THREADS) {
            unsigned m = 0;
            if (l3d[j].good) {
                double d[3]; mf_director(l3d[j], d);
                for (int ax = 1; ax <= 3; ax++) {
                    float x, y, z; mf_proj_d(sh.R0, ax, d, x, y, z);
                    if (!((double)mf_lambda(x, y) < a.sin_l)) continue;
                    mf_proj_d(sh.Rax[ax - 1], ax, d, x, y, z);
                    if ((double)mf_lambda(x, y) < a.sin_ms) m |= 1u << (ax - 1);
                }
            }
            lax[j] = (uint8_t)m;
        }
}

// one workgroup walks the frames in order: frame f starts from frame f - 1's R (frame 0 from a.R0)
__global__ __launch_bounds__(MF_THREADS) void k_mf_track(MfArgs a)
{
    __shared__ MfShared sh;
    const int tid = threadIdx.x;
    if (tid < 9) sh.R0[tid] = a.R0[tid];
    __syncthreads();
    for (int f = 0; f < a.nframes; f++) {
        const hvo_surface_normal *sn = (const hvo_surface_normal *)((const char *)a.sn + (size_t)f * a.sn_stride);
        const hvo_line3d *l3d = (const hvo_line3d *)((const char *)a.l3d + (size_t)f * a.l3d_stride);
        if (tid == 0) { int nl = a.nl; if (a.d_nl) { nl = a.d_nl[f]; nl = nl < 0 ? 0 : (nl > a.nl ? a.nl : nl); } sh.nl = nl; }
        __syncthreads();
        const int nl = sh.nl;
        mf_frame(sh, a, sn, a.nn, l3d, nl, a.res + f, f == 0 ? a.normal_axes : nullptr, f == 0 ? a.line_axes : nullptr);
        __syncthreads();                                         // the membership pass reads sh.R0
        if (tid < 9) sh.R0[tid] = sh.R[tid];
        __syncthreads();
    }
}

// enqueue the chain over nframes frames laid out at the given strides; R_last of frame 0 by value
int mf_enqueue(hipStream_t st, const hvo_surface_normal *d_sn, int nn, size_t sn_stride, const hvo_line3d *d_l3d, int nl, size_t l3d_stride,
               const int *d_nl, int nframes, const float R_last[9], hvo_mf_result *d_res, uint8_t *d_normal_axes, uint8_t *d_line_axes)
{
    if (nframes < 1 || nn < 0 || nl < 0 || (nn > 0 && !d_sn) || (nl > 0 && !d_l3d) || !d_res) return HVO_ERR_INVALID_ARG;
    MfArgs a;
    a.sn = d_sn; a.nn = nn; a.sn_stride = sn_stride;
    a.l3d = d_l3d; a.nl = nl; a.l3d_stride = l3d_stride; a.d_nl = d_nl;
    a.nframes = nframes;
    for (int i = 0; i < 9; i++) a.R0[i] = R_last[i];
    a.sin_n = sin(0.2018); a.sin_l = sin(0.1018); a.sin_ms = sin(0.2518);
    a.res = d_res; a.normal_axes = d_normal_axes; a.line_axes = d_line_axes;
    hipLaunchKernelGGL(k_mf_track, dim3(1), dim3(MF_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? HVO_OK : HVO_ERR_HIP;
}
