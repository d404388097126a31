// pose_opt.hip -- Optimizer::PoseOptimization(Frame *) for the RGB-D tracker (reference src/Optimizer.cc:590-1478): the motion-only
// optimisation of one pose vertex over the frame's point, line end-point, vanishing-direction and plane correspondences, the four rounds
// of g2o's Levenberg loop with the outlier classification between them.
//
// One workgroup of PO_THREADS threads per frame, the whole call in one launch:
//   edges        the index space [points | line start/end pairs | vanishing directions | planes | parallel | vertical] in the reference's
//                insertion order; thread t owns edges t, t + PO_THREADS, ... for the whole call and reloads their few words per pass (they
//                stay in the vector cache); the outlier flags (= the edges' levels) live in LDS
//   iteration    thread 0 keeps the estimate as unit quaternion + translation like SE3Quat; 12 threads form the perturbed poses
//                exp(+-1e-9 e_d) * estimate (Thirdparty/g2o/g2o/core/base_unary_edge.hpp:82-130) once for all edges; every thread adds
//                its edges' upper H (21), b (6) and robust chi2 (1) in edge order, the workgroup reduces them over a fixed tree
//                (__shfl_down within a wave, waves added in order), thread 0 runs the 6 x 6 LDL^T solve and the lambda logic
//                (core/optimization_algorithm_levenberg.cpp:61-189); a trial is one error pass and the reduction of one double
//   rounds       Optimizer.cc:1183-1466: restart from the initial pose, classify on chi2() as float, robust kernels off after round 2
// All arithmetic in double, uncontracted (-ffp-contract=off).  Readings and defined behaviours (tests/pose_opt_ref.py
// restates the same): points and planes are mapped with the quaternion's rotation matrix; the solve is LDL^T without pivoting and fails on
// a pivot <= 0; an evaluation of DistVp2VpOnlyPose (include/g2oMSC.h:766-846) that takes its early return yields error 0 -- the reference
// keeps a stale or uninitialised _error -- and flags the edge when a round's classification reads that evaluation; classification
// re-evaluates an unflagged edge at the pose of the round's last computeActiveErrors (the last trial, accepted or not) instead of storing
// _error per edge.  The host and stream forms launch this kernel alone on the same bytes, so they give bit-identical results.
#include "frame_view.hpp"
#include "staged_call.hpp"
#include "se3quat.hpp"        // quat_from_R .. se3_map, huber, ldlt6_solve
#include <math.h>
#include <cmath>
#include <string.h>
#include <string>
#include <vector>

#define PO_THREADS 256
#define PO_WAVES (PO_THREADS / 64)
#define PO_MAX_POINTS 8192
#define PO_MAX_LINES 4096
#define PO_MAX_PLANES 64
#define PO_DELTA 1e-9

struct PoFrame {                       // one frame's problem, every pointer a device pointer
    float Tcw[12];
    int n_pts, n_lines, n_planes, planes_from_tail;
    const int *d_nkp, *d_nkl;          // resident counts that cap n_pts / n_lines (may be null)
    const hvo_keypoint *kp_un; const float *uright; const float *inv_sigma2;     // inv_sigma2 null: the level table by octave
    const uint16_t *depth; int pitch, w, h; float dfac, bf32;                    // depth set (resident batch): mvuRight is formed here like k_stereo_from_rgbd
    const double *linefn; const hvo_line3d *l3d;
    const float *pl_coef; const hvo_plane_cloud *pclouds;                        // frame planes: n x 4 floats, or the plane tail's 64 records
    const uint8_t *pt_has; const float *pt_xyz;
    const uint8_t *ln_has; const double *ln_xyz;
    const uint8_t *pl_has; const float *pl_map;                                  // n_planes x 3 flags, n_planes x 3 x 4 world coefficients
    uint8_t *pt_out, *ln_out, *vp_out, *pl_out;                                  // outlier flags: n_pts, n_lines, n_lines, n_planes x 3
};

struct PoArgs {
    const PoFrame *frames; hvo_pose_result *res; int nframes;
    double fx, fy, cx, cy, bf;
    double info_angle, info_dis, info_par, info_ver, chi_plane, chi_vp;
    double d_mono, d_stereo, d_line, d_plane, d_vpl;     // Huber deltas (floats in the reference)
    float inv_level_sigma2[HVO_MAX_LEVELS];
};

struct PoPose { double q[4], t[3]; };  // se3quat.hpp's pose, passed as .q: seven doubles in a row
static_assert(offsetof(PoPose, t) == 4 * sizeof(double) && sizeof(PoPose) == 7 * sizeof(double), "q then t, no padding");

struct PoShared {
    double P[13][12];                  // R (row-major) and t of the estimate [0] and the 12 perturbed poses
    double Plast[12], Pest[12];        // the last trial's pose and the estimate, for the classification
    double red[PO_WAVES][28];
    double sum[28];
    PoPose est, trial;
    float plane[PO_MAX_PLANES][4];     // the frame planes' coefficients
    int n_pts, n_lines, n_planes, cnt[4];
    int go, robust;
    uint8_t f_pt[PO_MAX_POINTS], f_ln[PO_MAX_LINES], f_vp[PO_MAX_LINES], f_pl[3 * PO_MAX_PLANES];
};

// ---- Plane3D (g2oAddition/Plane3D.h) ----
static __device__ void po_plane_normalize(double *c)                        // :175-180
{
    const double n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]), s = 1.0 / n;
    c[0] = c[0] * s; c[1] = c[1] * s; c[2] = c[2] * s; c[3] = c[3] * s;
    if (c[3] < 0.0) { c[0] = -c[0]; c[1] = -c[1]; c[2] = -c[2]; c[3] = -c[3]; }
}
static __device__ void po_plane_transform(const double *Rt, const double *c, double *o)   // operator*(Isometry3D, Plane3D) :186-199
{
    o[0] = (c[0] * Rt[0] + c[1] * Rt[1]) + c[2] * Rt[2];
    o[1] = (c[0] * Rt[3] + c[1] * Rt[4]) + c[2] * Rt[5];
    o[2] = (c[0] * Rt[6] + c[1] * Rt[7]) + c[2] * Rt[8];
    o[3] = c[3] - ((Rt[9] * o[0] + Rt[10] * o[1]) + Rt[11] * o[2]);
    if (o[3] < 0.0) { o[0] = -o[0]; o[1] = -o[1]; o[2] = -o[2]; o[3] = -o[3]; }
    po_plane_normalize(o);
}
// (azimuth, elevation) of rotation(v)^T m, rotation(v) = Rz(azimuth(v)) Ry(-elevation(v)) (:46-82)
static __device__ void po_rot_T_apply(const double *v, const double *m, double *ae)
{
    const double az = atan2(v[1], v[0]), el = atan2(v[2], sqrt(v[0] * v[0] + v[1] * v[1]));
    const double ca = cos(az), sa = sin(az), ce = cos(-el), se = sin(-el);
    const double n0 = (ca * ce * m[0] + sa * ce * m[1]) - se * m[2];
    const double n1 = -sa * m[0] + ca * m[1];
    const double n2 = (ca * se * m[0] + sa * se * m[1]) + ce * m[2];
    ae[0] = atan2(n1, n0); ae[1] = atan2(n2, sqrt(n0 * n0 + n1 * n1));
}

// ---- one edge ----
enum { PO_NONE = 0, PO_MONO, PO_STEREO, PO_LINEPT, PO_VP, PO_PLANE, PO_PAR, PO_VER };
struct PoEdge { int kind; double a[6], m[4], info[3], delta; };

// the edge at index e of the frame's index space; kind PO_NONE where the reference inserts none
static __device__ void po_load(const PoArgs &A, const PoFrame &F, const PoShared &sh, int e, PoEdge &E)
{
    const int n = sh.n_pts, nl = sh.n_lines, m = sh.n_planes;
    E.kind = PO_NONE; E.info[0] = E.info[1] = E.info[2] = 0.0; E.delta = 0.0;
    if (e < n) {
        if (!F.pt_has[e]) return;
        const hvo_keypoint kp = F.kp_un[e];
        float ur = F.uright ? F.uright[e] : -1.f;
        if (F.depth) {                                                       // Frame::ComputeStereoFromRGBD (src/Frame.cc:1940-1961), k1 == 0: mvKeysUn = mvKeys
            const int v = (int)kp.y, u = (int)kp.x;
            if (u >= 0 && v >= 0 && u < F.w && v < F.h) {
                const float d = __fmul_rn((float)F.depth[(size_t)v * F.pitch + u], F.dfac);
                if (d > 0 && (double)d < 7.0) ur = __fsub_rn(kp.x, __fdiv_rn(F.bf32, d));
            }
        }
        float s2;
        if (F.inv_sigma2) s2 = F.inv_sigma2[e];
        else { int o = kp.octave; o = o < 0 ? 0 : (o >= HVO_MAX_LEVELS ? HVO_MAX_LEVELS - 1 : o); s2 = A.inv_level_sigma2[o]; }
        E.kind = ur < 0 ? PO_MONO : PO_STEREO;                               // Optimizer.cc:646
        for (int k = 0; k < 3; k++) E.a[k] = (double)F.pt_xyz[3 * e + k];
        E.m[0] = (double)kp.x; E.m[1] = (double)kp.y; E.m[2] = (double)ur;
        E.info[0] = E.info[1] = (double)s2; E.info[2] = E.kind == PO_STEREO ? (double)s2 : 0.0;
        E.delta = E.kind == PO_STEREO ? A.d_stereo : A.d_mono;
        return;
    }
    e -= n;
    if (e < 2 * nl) {
        const int i = e >> 1;
        if (!F.ln_has[i]) return;
        E.kind = PO_LINEPT;
        for (int k = 0; k < 3; k++) { E.a[k] = F.ln_xyz[6 * i + 3 * (e & 1) + k]; E.m[k] = F.linefn[3 * i + k]; }
        E.info[0] = E.info[1] = E.info[2] = 1.0; E.delta = A.d_line;
        return;
    }
    e -= 2 * nl;
    if (e < nl) {
        if (!F.ln_has[e]) return;
        const hvo_line3d &L = F.l3d[e];
        for (int k = 0; k < 3; k++) { E.m[k] = L.B[k] - L.A[k]; E.a[k] = F.ln_xyz[6 * e + k]; E.a[3 + k] = F.ln_xyz[6 * e + 3 + k]; }
        if (E.m[0] == 0.0 || E.m[1] == 0.0 || E.m[2] == 0.0) return;        // Optimizer.cc:827
        if (E.a[3] - E.a[0] == 0.0 || E.a[4] - E.a[1] == 0.0 || E.a[5] - E.a[2] == 0.0) return;   // :853
        E.kind = PO_VP; E.info[0] = E.info[1] = E.info[2] = 1.0; E.delta = A.d_line;
        return;
    }
    e -= nl;
    if (e < 3 * m) {
        const int r = e / m, i = e - r * m;
        if (!F.pl_has[3 * i + r]) return;
        for (int k = 0; k < 4; k++) { E.a[k] = (double)F.pl_map[(3 * i + r) * 4 + k]; E.m[k] = (double)sh.plane[i][k]; }
        po_plane_normalize(E.a); po_plane_normalize(E.m);                   // Converter::toPlane3D -> Plane3D(v)
        if (r == 0) { E.kind = PO_PLANE; E.info[0] = E.info[1] = A.info_angle; E.info[2] = A.info_dis; E.delta = A.d_plane; }
        else { E.kind = r == 1 ? PO_PAR : PO_VER; E.info[0] = E.info[1] = r == 1 ? A.info_par : A.info_ver; E.delta = A.d_vpl; }
    }
}

// computeError at the pose Rt; returns true when DistVp2VpOnlyPose takes its early return (err = 0: the defined behaviour)
static __device__ bool po_error(const PoArgs &A, const PoEdge &E, const double *Rt, double *err)
{
    err[0] = err[1] = err[2] = 0.0;
    switch (E.kind) {
    case PO_MONO: {
        double X[3]; se3_map(Rt, E.a, X);
        err[0] = E.m[0] - (X[0] / X[2] * A.fx + A.cx); err[1] = E.m[1] - (X[1] / X[2] * A.fy + A.cy);
        return false; }
    case PO_STEREO: {
        double X[3]; se3_map(Rt, E.a, X);
        const double iz = (double)(float)(1.0 / X[2]);                      // const float invz = 1.0f / trans_xyz[2]
        const double u = X[0] * iz * A.fx + A.cx;
        err[0] = E.m[0] - u; err[1] = E.m[1] - (X[1] * iz * A.fy + A.cy); err[2] = E.m[2] - (u - A.bf * iz);
        return false; }
    case PO_LINEPT: {
        double X[3]; se3_map(Rt, E.a, X);
        const double u = X[0] / X[2] * A.fx + A.cx, v = X[1] / X[2] * A.fy + A.cy;
        err[0] = (E.m[0] * u + E.m[1] * v) + E.m[2];
        return false; }
    case PO_VP: {
        double S[3], T[3]; se3_map(Rt, E.a, S); se3_map(Rt, E.a + 3, T);
        double dc[3] = { T[0] - S[0], T[1] - S[1], T[2] - S[2] };
        const double *m = E.m;
        const double dot = (m[0] * dc[0] + m[1] * dc[1]) + m[2] * dc[2];
        const double den = sqrt((dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2]) * sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        if (dot / den < 0.0) { dc[0] = S[0] - T[0]; dc[1] = S[1] - T[1]; dc[2] = S[2] - T[2]; }
        const double a2 = m[2], b2 = dc[2];
        if (a2 == 0.0 || b2 == 0.0) return true;
        double a0 = (A.fx * m[0] + A.cx * m[2]) / a2, a1 = (A.fy * m[1] + A.cy * m[2]) / a2;
        double b0 = (A.fx * dc[0] + A.cx * dc[2]) / b2, b1 = (A.fy * dc[1] + A.cy * dc[2]) / b2;
        const double na = sqrt(a0 * a0 + a1 * a1), nb = sqrt(b0 * b0 + b1 * b1);
        a0 = a0 / na; a1 = a1 / na; b0 = b0 / nb; b1 = b1 / nb;
        const double d0 = a0 - b0, d1 = a1 - b1;
        err[0] = sqrt(d0 * d0 + d1 * d1);
        return false; }
    case PO_PLANE: {
        double l[4]; po_plane_transform(Rt, E.a, l);
        po_rot_T_apply(l, E.m, err);
        err[2] = (-l[3]) - (-E.m[3]);
        return false; }
    case PO_PAR: {
        double l[4]; po_plane_transform(Rt, E.a, l);
        if ((E.m[0] * l[0] + E.m[1] * l[1]) + E.m[2] * l[2] < 0) { l[0] = -l[0]; l[1] = -l[1]; l[2] = -l[2]; }
        po_rot_T_apply(l, E.m, err);
        return false; }
    case PO_VER: {
        double n[4]; po_plane_transform(Rt, E.a, n);
        const double *m = E.m;
        const double v[3] = { n[1] * m[2] - n[2] * m[1], n[2] * m[0] - n[0] * m[2], n[0] * m[1] - n[1] * m[0] };
        const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        const double ax[3] = { v[0] / vn, v[1] / vn, v[2] / vn };
        const double s = 1.0, c = 6.123233995736766e-17;                    // sin, cos of M_PI / 2 as Eigen::AngleAxisd takes them
        const double sa[3] = { s * ax[0], s * ax[1], s * ax[2] }, ca[3] = { (1 - c) * ax[0], (1 - c) * ax[1], (1 - c) * ax[2] };
        const double t01 = ca[0] * ax[1], t02 = ca[0] * ax[2], t12 = ca[1] * ax[2];
        const double b[3] = { ((ca[0] * ax[0] + c) * n[0] + (t01 - sa[2]) * n[1]) + (t02 + sa[1]) * n[2],
                              ((t01 + sa[2]) * n[0] + (ca[1] * ax[1] + c) * n[1]) + (t12 - sa[0]) * n[2],
                              ((t02 - sa[1]) * n[0] + (t12 + sa[0]) * n[1]) + (ca[2] * ax[2] + c) * n[2] };
        po_rot_T_apply(b, m, err);
        return false; }
    }
    return false;
}

static __device__ __forceinline__ double po_chi2(const PoEdge &E, const double *err)
{
    return (E.info[0] * err[0] * err[0] + E.info[1] * err[1] * err[1]) + E.info[2] * err[2] * err[2];
}
static __device__ __forceinline__ bool po_level1(const PoShared &sh, int e)
{
    const int n = sh.n_pts, nl = sh.n_lines;
    if (e < n) return sh.f_pt[e];
    e -= n; if (e < 2 * nl) return sh.f_ln[e >> 1];
    e -= 2 * nl; if (e < nl) return sh.f_vp[e];
    return sh.f_pl[e - nl];                                                  // role-major: r * n_planes + i
}

// sum of v[0..cnt) over the workgroup into sh.sum: __shfl_down halving within a wave, then the waves in order
static __device__ void po_reduce(PoShared &sh, double *v, int cnt)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k < cnt; k++) {
        double x = v[k];
        for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, 64);   // wave_sum_down's text (se3quat.hpp), kept in place: as a call
        if (lane == 0) sh.red[wave][k] = x;                                        // it reorders k_pose_opt (profiles/shared_readings.txt)
    }
    __syncthreads();
    if (tid < cnt) sh.sum[tid] = ((sh.red[0][tid] + sh.red[1][tid]) + sh.red[2][tid]) + sh.red[3][tid];
    __syncthreads();
}

// robust chi2 of the active edges at pose Rt -> sh.sum[0]
static __device__ void po_chi_pass(const PoArgs &A, const PoFrame &F, PoShared &sh, const double *Rt, int nE)
{
    double acc = 0.0;
    for (int e = threadIdx.x; e < nE; e += PO_THREADS) {
        if (po_level1(sh, e)) continue;
        PoEdge E; po_load(A, F, sh, e, E);
        if (E.kind == PO_NONE) continue;
        double err[3]; po_error(A, E, Rt, err);
        double c = po_chi2(E, err), r0 = c, r1;
        if (sh.robust) huber(c, E.delta, r0, r1);
        acc = acc + r0;
    }
    po_reduce(sh, &acc, 1);
}

// computeActiveErrors + buildSystem at sh.P[0] with the perturbed poses sh.P[1..12]: H (upper, 21), b (6), robust chi2 -> sh.sum
static __device__ void po_sys_pass(const PoArgs &A, const PoFrame &F, PoShared &sh, int nE)
{
    double acc[28];
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    for (int e = threadIdx.x; e < nE; e += PO_THREADS) {
        if (po_level1(sh, e)) continue;
        PoEdge E; po_load(A, F, sh, e, E);
        if (E.kind == PO_NONE) continue;
        double err[3]; po_error(A, E, sh.P[0], err);
        const double c = po_chi2(E, err);
        double r0 = c, r1 = 1.0;
        if (sh.robust) huber(c, E.delta, r0, r1);
        double J[3][6];
        if (E.kind <= PO_STEREO) {                                           // types_six_dof_expmap.cpp:266-288, :335-364
            double X[3]; se3_map(sh.P[0], E.a, X);
            const double x = X[0], y = X[1], invz = 1.0 / X[2], iz2 = invz * invz, fx = A.fx, fy = A.fy;
            J[0][0] = x * y * iz2 * fx; J[0][1] = -(1 + (x * x * iz2)) * fx; J[0][2] = y * invz * fx; J[0][3] = -invz * fx; J[0][4] = 0; J[0][5] = x * iz2 * fx;
            J[1][0] = (1 + y * y * iz2) * fy; J[1][1] = -x * y * iz2 * fy; J[1][2] = -x * invz * fy; J[1][3] = 0; J[1][4] = -invz * fy; J[1][5] = y * iz2 * fy;
            if (E.kind == PO_STEREO) {
                J[2][0] = J[0][0] - A.bf * y * iz2; J[2][1] = J[0][1] + A.bf * x * iz2; J[2][2] = J[0][2]; J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - A.bf * iz2;
            } else for (int d = 0; d < 6; d++) J[2][d] = 0.0;
        } else {
            const double scalar = 1.0 / (2 * PO_DELTA);
            for (int d = 0; d < 6; d++) {
                double e1[3], e2[3];
                po_error(A, E, sh.P[1 + 2 * d], e1); po_error(A, E, sh.P[2 + 2 * d], e2);
                for (int k = 0; k < 3; k++) J[k][d] = scalar * (e1[k] - e2[k]);
            }
        }
        int h = 0;
        for (int i = 0; i < 6; i++) {
            for (int j = i; j < 6; j++, h++) {
                double s = 0.0;
                for (int k = 0; k < 3; k++) s = s + J[k][i] * (r1 * E.info[k]) * J[k][j];
                acc[h] = acc[h] + s;
            }
            double g = 0.0;
            for (int k = 0; k < 3; k++) g = g + J[k][i] * (E.info[k] * err[k]);
            acc[21 + i] = acc[21 + i] - r1 * g;
        }
        acc[27] = acc[27] + r0;
    }
    po_reduce(sh, acc, 28);
}

__global__ __launch_bounds__(PO_THREADS) void k_pose_opt(PoArgs A)
{
    __shared__ PoShared sh;
    const int tid = threadIdx.x;
    const PoFrame &F = A.frames[blockIdx.x];
    hvo_pose_result *res = A.res + blockIdx.x;

    if (tid == 0) {
        int n = F.n_pts, nl = F.n_lines;
        if (F.d_nkp) { const int c = *F.d_nkp; n = n < c ? n : (c < 0 ? 0 : c); }
        if (F.d_nkl) { const int c = *F.d_nkl; nl = nl < c ? nl : (c < 0 ? 0 : c); }
        sh.n_pts = n < PO_MAX_POINTS ? n : PO_MAX_POINTS; sh.n_lines = nl < PO_MAX_LINES ? nl : PO_MAX_LINES;
        int m = 0;
        if (F.planes_from_tail) {                                            // the valid records, in order = mvPlaneCoefficients
            for (int i = 0; i < PO_MAX_PLANES && m < F.n_planes; i++)
                if (F.pclouds[i].valid) { for (int k = 0; k < 4; k++) sh.plane[m][k] = F.pclouds[i].coef[k]; m++; }
        } else {
            m = F.n_planes < PO_MAX_PLANES ? F.n_planes : PO_MAX_PLANES;
            for (int i = 0; i < m; i++) for (int k = 0; k < 4; k++) sh.plane[i][k] = F.pl_coef[4 * i + k];
        }
        sh.n_planes = m;
        sh.cnt[0] = sh.cnt[1] = sh.cnt[2] = sh.cnt[3] = 0;
        sh.robust = 1;
    }
    __syncthreads();
    const int n = sh.n_pts, nl = sh.n_lines, m = sh.n_planes, nE = n + 3 * nl + 3 * m;
    for (int i = tid; i < n; i += PO_THREADS) sh.f_pt[i] = 0;
    for (int i = tid; i < nl; i += PO_THREADS) { sh.f_ln[i] = 0; sh.f_vp[i] = 0; }
    for (int i = tid; i < 3 * m; i += PO_THREADS) sh.f_pl[i] = 0;

    // nInitialCorrespondences (points + planes of the three roles) and the graph's edge count
    {
        int c_init = 0, c_edges = 0;
        for (int e = tid; e < nE; e += PO_THREADS) {
            PoEdge E; po_load(A, F, sh, e, E);
            if (E.kind == PO_NONE) continue;
            c_edges++;
            if (E.kind <= PO_STEREO || E.kind >= PO_PLANE) c_init++;
        }
        atomicAdd(&sh.cnt[0], c_init); atomicAdd(&sh.cnt[1], c_edges);
    }
    __syncthreads();
    const int n_init = sh.cnt[0], n_edges = sh.cnt[1];
    __syncthreads();

    double T0[12];
    for (int i = 0; i < 12; i++) T0[i] = (double)F.Tcw[i];                    // finite: the host checked
    if (tid == 0) {
        memset(res, 0, sizeof(*res));
        for (int i = 0; i < 12; i++) { res->Tcw[i] = F.Tcw[i]; res->Tcw_d[i] = T0[i]; }
        res->n_initial = n_init; res->n_edges = n_edges;
        res->status = HVO_OK;
    }
    int n_bad = 0, n_line_bad = 0;
    if (n_init >= 3) {                                          // Optimizer.cc:1170
        PoPose init;
        {
            const double R[9] = { T0[0], T0[1], T0[2], T0[4], T0[5], T0[6], T0[8], T0[9], T0[10] };
            quat_from_R(R, init.q); quat_normalize(init.q);            // Converter::toSE3Quat
            init.t[0] = T0[3]; init.t[1] = T0[7]; init.t[2] = T0[11];
        }
        for (int rnd = 0; rnd < 4; rnd++) {
            if (tid == 0) sh.est = init;                                     // setEstimate(pFrame->mTcw), every round
            __syncthreads();
            double lam = 0.0, ni = 2.0; int nbad_it = 0, its = 0, trials = 0; double chi_final = 0.0;     // thread 0's
            for (int it = 0; it < 10; it++) {
                if (tid == 0) se3_Rt(sh.est.q, sh.P[0]);
                else if (tid <= 12) {
                    const int d = (tid - 1) >> 1;
                    double u[6] = { 0, 0, 0, 0, 0, 0 }; u[d] = ((tid - 1) & 1) ? -PO_DELTA : PO_DELTA;
                    PoPose ex, p; se3_exp(u, ex.q); se3_mul(ex.q, sh.est.q, p.q); se3_Rt(p.q, sh.P[tid]);
                }
                __syncthreads();
                po_sys_pass(A, F, sh, nE);
                double H[36], b[6], cur = 0.0, ini = 0.0;
                if (tid == 0) {
                    int h = 0;
                    for (int i = 0; i < 6; i++) for (int j = i; j < 6; j++, h++) { H[6 * i + j] = sh.sum[h]; H[6 * j + i] = sh.sum[h]; }
                    for (int i = 0; i < 6; i++) b[i] = sh.sum[21 + i];
                    cur = ini = sh.sum[27];
                    if (it == 0) {                                           // computeLambdaInit: tau = 1e-5
                        double md = 0.0;
                        for (int j = 0; j < 6; j++) md = fmax(fabs(H[7 * j]), md);
                        lam = 1e-5 * md; ni = 2.0; nbad_it = 0;
                    }
                }
                double rho = 0.0; int q = 0;
                while (true) {                                               // uniform: every thread follows sh.go
                    double x[6]; bool ok2 = true; double scale = 0.0;
                    if (tid == 0) {
                        double Hl[36];
                        for (int i = 0; i < 36; i++) Hl[i] = H[i];
                        for (int j = 0; j < 6; j++) Hl[7 * j] = Hl[7 * j] + lam;
                        ok2 = ldlt6_solve(Hl, b, x, [](double s) { return !(s > 0); });             // fails on a pivot <= 0 or NaN
                        PoPose ex; se3_exp(x, ex.q); se3_mul(ex.q, sh.est.q, sh.trial.q);
                        se3_Rt(sh.trial.q, sh.Plast);
                        for (int j = 0; j < 6; j++) scale = scale + x[j] * (lam * x[j] + b[j]);
                    }
                    __syncthreads();
                    po_chi_pass(A, F, sh, sh.Plast, nE);
                    if (tid == 0) {
                        double tmp = sh.sum[0];
                        if (!ok2) tmp = 1.7976931348623157e308;
                        scale = scale + 1e-3;
                        rho = (cur - tmp) / scale;
                        if (rho > 0 && isfinite(tmp)) {
                            double alpha = 1.0 - pow(2 * rho - 1, 3.0);
                            alpha = fmin(alpha, 2.0 / 3.0);
                            lam = lam * fmax(1.0 / 3.0, alpha); ni = 2.0; cur = tmp; sh.est = sh.trial;
                        } else { lam = lam * ni; ni = ni * 2; }
                        q++; trials++;
                        sh.go = (rho < 0 && q < 10) ? 1 : 0;
                    }
                    __syncthreads();
                    const int go = sh.go;
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
            if (tid == 0) {
                res->iterations[rnd] = its; res->trials[rnd] = trials; res->lambda[rnd] = lam; res->chi2[rnd] = chi_final; res->rounds = rnd + 1;
                se3_Rt(sh.est.q, sh.Pest);
                sh.cnt[2] = sh.cnt[3] = 0;
            }
            __syncthreads();
            // ---- classification (Optimizer.cc:1188-1458) ----
            const float th_mono = 5.991f, th_stereo = 7.815f, th_line = 3.84f;
            int c_bad = 0, c_lbad = 0;
            for (int i = tid; i < n; i += PO_THREADS) {
                PoEdge E; po_load(A, F, sh, i, E);
                if (E.kind == PO_NONE) continue;
                double err[3]; po_error(A, E, sh.f_pt[i] ? sh.Pest : sh.Plast, err);
                const float chi = (float)po_chi2(E, err);
                const bool bad = chi > (E.kind == PO_STEREO ? th_stereo : th_mono);
                sh.f_pt[i] = bad; c_bad += bad;
            }
            for (int i = tid; i < nl; i += PO_THREADS) {
                PoEdge E; double err[3];
                po_load(A, F, sh, n + 2 * i, E);
                if (E.kind != PO_NONE) {
                    const double *Rt = sh.f_ln[i] ? sh.Pest : sh.Plast;
                    po_error(A, E, Rt, err); const float cs = (float)po_chi2(E, err);
                    po_load(A, F, sh, n + 2 * i + 1, E);
                    po_error(A, E, Rt, err); const float ce = (float)po_chi2(E, err);
                    const bool bad = cs > th_line && ce > th_line;
                    sh.f_ln[i] = bad; c_lbad += bad;
                }
                po_load(A, F, sh, n + 2 * nl + i, E);
                if (E.kind != PO_NONE) {
                    const bool early = po_error(A, E, sh.f_vp[i] ? sh.Pest : sh.Plast, err);
                    const float chi = (float)po_chi2(E, err);
                    sh.f_vp[i] = early || (double)chi > 3.84;               // vanishing-direction outliers count nowhere
                }
            }
            for (int e = tid; e < 3 * m; e += PO_THREADS) {
                PoEdge E; po_load(A, F, sh, n + 3 * nl + e, E);
                if (E.kind == PO_NONE) continue;
                double err[3]; po_error(A, E, sh.f_pl[e] ? sh.Pest : sh.Plast, err);
                const float chi = (float)po_chi2(E, err);
                const bool bad = (double)chi > (E.kind == PO_PLANE ? A.chi_plane : A.chi_vp);
                sh.f_pl[e] = bad; c_bad += bad;
            }
            atomicAdd(&sh.cnt[2], c_bad); atomicAdd(&sh.cnt[3], c_lbad);
            __syncthreads();
            n_bad = sh.cnt[2]; n_line_bad = sh.cnt[3];
            if (tid == 0 && rnd == 2) sh.robust = 0;                         // setRobustKernel(0) on every edge
            __syncthreads();
            if (n_edges < 10) break;                                         // optimizer.edges().size() < 10
        }
        if (tid == 0) {
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { res->Tcw_d[4 * r + c] = sh.Pest[3 * r + c]; res->Tcw[4 * r + c] = (float)sh.Pest[3 * r + c]; }
            for (int r = 0; r < 3; r++) { res->Tcw_d[4 * r + 3] = sh.Pest[9 + r]; res->Tcw[4 * r + 3] = (float)sh.Pest[9 + r]; }
            res->n_bad = n_bad; res->n_line_bad = n_line_bad;
            res->ret = n_init - n_bad - n_line_bad;
        }
    }
    __syncthreads();
    for (int i = tid; i < F.n_pts; i += PO_THREADS) F.pt_out[i] = i < n ? sh.f_pt[i] : 0;
    for (int i = tid; i < F.n_lines; i += PO_THREADS) { F.ln_out[i] = i < nl ? sh.f_ln[i] : 0; F.vp_out[i] = i < nl ? sh.f_vp[i] : 0; }
    for (int e = tid; e < 3 * F.n_planes; e += PO_THREADS) {                 // out: n_planes x 3, plane-major
        const int i = e / 3, r = e - 3 * i;
        F.pl_out[e] = i < m ? sh.f_pl[r * m + i] : 0;
    }
}

// ---- host side ----
static const hvo_pose_plane_params k_po_default_pp = { 0.5, 50.0, 0.1, 0.1, 100.0, 50.0 };    // TUM3.yaml

// where one frame's host arrays lie in the one upload (the frame side only when it is not resident) and its flags in the download
struct PoPieces {
    StagePiece<uint8_t> pt_has, ln_has, pl_has, pt_out, ln_out, vp_out, pl_out;
    StagePiece<float> pt_xyz, pl_map, uright, inv_sigma2, pl_coef;
    StagePiece<double> ln_xyz, linefn;
    StagePiece<hvo_keypoint> kp_un; StagePiece<hvo_line3d> l3d;
};

// A staged call (staged_call.hpp): the context's pinned block holds the upload and receives the download, the device side is the context's
// call arena: nothing is allocated by a call once both have grown.
int po_run(hvo_ctx *ctx, hipStream_t st, const hvo_camera *cam, const hvo_pose_plane_params *pp,
           int n, const hvo_pose_problem *prob, const FrameView *fr, hvo_pose_result *res, const hvo_pose_flags *flags, std::string *err)
{
    if (!pp) pp = &k_po_default_pp;
    StageCarver C(64);
    const auto frames = C.take<PoFrame>((size_t)n);
    std::vector<PoPieces> pieces((size_t)n);
    for (int f = 0; f < n; f++) {
        const hvo_pose_problem &p = prob[f];
        if (p.n_points < 0 || p.n_lines < 0 || p.n_planes < 0 || p.n_points > PO_MAX_POINTS || p.n_lines > PO_MAX_LINES || p.n_planes > PO_MAX_PLANES) {
            *err = "pose optimisation: at most 8192 points, 4096 lines and 64 planes per frame"; return HVO_ERR_UNSUPPORTED;
        }
        for (int i = 0; i < 12; i++) if (!std::isfinite(p.Tcw[i])) { *err = "pose optimisation: the initial pose is not finite"; return HVO_ERR_INVALID_ARG; }
        const bool r = fr != nullptr;
        const bool planes_ok = p.plane_map ? (p.slot_match || p.slot_parallel || p.slot_vertical) : (p.pl_has && p.pl_coef_w);
        if ((p.n_points && (!p.pt_has || !p.pt_xyz || (!r && !p.kp_un))) ||
            (p.n_lines && (!p.ln_has || !p.ln_xyz || (!r && (!p.linefn || !p.lines3d)))) ||
            (p.n_planes && (!planes_ok || (!r && !p.plane_coef)))) { *err = "pose optimisation: a needed array is NULL"; return HVO_ERR_INVALID_ARG;
        }
        const size_t np = (size_t)p.n_points, nl = (size_t)p.n_lines, m = (size_t)p.n_planes;
        PoPieces &L = pieces[f];
        L.pt_has = C.take<uint8_t>(np); L.pt_xyz = C.take<float>(np, 3); L.ln_has = C.take<uint8_t>(nl); L.ln_xyz = C.take<double>(nl, 6);
        L.pl_has = C.take<uint8_t>(m, 3); L.pl_map = C.take<float>(m, 12);
        if (!r) {
            L.kp_un = C.take<hvo_keypoint>(np); L.uright = C.take<float>(p.uright ? np : 0); L.inv_sigma2 = C.take<float>(p.inv_sigma2 ? np : 0);
            L.linefn = C.take<double>(nl, 3); L.l3d = C.take<hvo_line3d>(nl); L.pl_coef = C.take<float>(m, 4);
        }
    }
    const size_t up = C.mark(), down0 = up;                                  // [0, up) goes up, [down0, total) comes down
    for (int f = 0; f < n; f++) {
        const hvo_pose_problem &p = prob[f];
        PoPieces &L = pieces[f];
        L.pt_out = C.take<uint8_t>((size_t)p.n_points); L.ln_out = C.take<uint8_t>((size_t)p.n_lines); L.vp_out = C.take<uint8_t>((size_t)p.n_lines);
        L.pl_out = C.take<uint8_t>((size_t)p.n_planes, 3);
    }
    const auto results = C.take<hvo_pose_result>((size_t)n);
    const size_t total = C.mark();
    StagedCall sc(ctx, st, "pose optimisation: ", err); int rc;
    if ((rc = sc.begin(total, up, total - down0, false))) return rc;     // every piece is copied whole: nothing relies on zero padding
    char *const d = sc.d, *const h = sc.h;
    for (int f = 0; f < n; f++) {
        const hvo_pose_problem &p = prob[f];
        const PoPieces &L = pieces[f];
        const size_t m = (size_t)p.n_planes;
        PoFrame &F = *frames.host(h, f); memset(&F, 0, sizeof(F));
        memcpy(F.Tcw, p.Tcw, sizeof(F.Tcw));
        F.n_pts = p.n_points; F.n_lines = p.n_lines; F.n_planes = p.n_planes;
        auto put = [&](const auto &piece, const void *src) { if (piece.bytes()) memcpy(piece.host(h), src, piece.bytes()); return piece.dev(d); };
        F.pt_has = put(L.pt_has, p.pt_has); F.pt_xyz = put(L.pt_xyz, p.pt_xyz);
        F.ln_has = put(L.ln_has, p.ln_has); F.ln_xyz = put(L.ln_xyz, p.ln_xyz);
        if (p.plane_map) {                                                   // an hvo_plane_match result as it is: slots, -1 = none; coefficients from the map
            uint8_t *has = L.pl_has.host(h); float *cw = L.pl_map.host(h);
            const int32_t *sl[3] = { p.slot_match, p.slot_parallel, p.slot_vertical };
            for (size_t i = 0; i < m; i++) for (int r = 0; r < 3; r++) {
                const int slot = sl[r] ? sl[r][i] : -1;
                float *c = cw + (3 * i + r) * 4; c[0] = c[1] = c[2] = c[3] = 0.f;
                has[3 * i + r] = 0;
                if (slot < 0) continue;
                if (hvo_plane_map_slot(p.plane_map, slot, c, nullptr, nullptr)) { *err = "pose optimisation: no such slot in the plane map"; return HVO_ERR_INVALID_ARG; }
                has[3 * i + r] = 1;
            }
            F.pl_has = L.pl_has.dev(d); F.pl_map = L.pl_map.dev(d);
        } else {
            F.pl_has = put(L.pl_has, p.pl_has); F.pl_map = put(L.pl_map, p.pl_coef_w);
        }
        if (fr) {
            const FrameView &R = fr[f];
            F.kp_un = R.kp_un; F.uright = R.uright; F.inv_sigma2 = nullptr; F.linefn = R.fn; F.l3d = R.l3d; F.pclouds = R.pclouds;
            F.planes_from_tail = 1; F.d_nkp = R.d_nkp; F.d_nkl = R.d_nkl;
            F.depth = R.depth; F.pitch = R.pitch; F.w = R.w; F.h = R.h; F.dfac = R.dfac; F.bf32 = cam->bf;
        } else {
            F.kp_un = put(L.kp_un, p.kp_un);
            F.uright = p.uright ? put(L.uright, p.uright) : nullptr;
            F.inv_sigma2 = p.inv_sigma2 ? put(L.inv_sigma2, p.inv_sigma2) : nullptr;
            F.linefn = put(L.linefn, p.linefn); F.l3d = put(L.l3d, p.lines3d);
            F.pl_coef = put(L.pl_coef, p.plane_coef);
        }
        F.pt_out = L.pt_out.dev(d); F.ln_out = L.ln_out.dev(d); F.vp_out = L.vp_out.dev(d); F.pl_out = L.pl_out.dev(d);
    }
    PoArgs A; memset(&A, 0, sizeof(A));
    A.frames = frames.dev(d); A.res = results.dev(d); A.nframes = n;
    A.fx = cam->fx; A.fy = cam->fy; A.cx = cam->cx; A.cy = cam->cy; A.bf = cam->bf;
    A.info_angle = 3282.8 / (pp->angle_info * pp->angle_info); A.info_dis = pp->distance_info * pp->distance_info;
    A.info_par = 3282.8 / (pp->parallel_info * pp->parallel_info); A.info_ver = 3282.8 / (pp->vertical_info * pp->vertical_info);
    A.chi_plane = pp->chi; A.chi_vp = pp->vp_chi;
    A.d_mono = (double)(float)sqrt(5.991); A.d_stereo = (double)(float)sqrt(7.815); A.d_line = (double)(float)sqrt(3.84);     // Optimizer.cc:631-633
    A.d_plane = (double)(float)sqrt(pp->chi); A.d_vpl = (double)(float)sqrt(pp->vp_chi);                                      // :963, :966
    frame_level_sigma2(ctx, nullptr, A.inv_level_sigma2);
    if ((rc = sc.up(0, up))) return rc;
    sc.tick();
    hipLaunchKernelGGL(k_pose_opt, dim3(n), dim3(PO_THREADS), 0, st, A);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(down0, total, &b))) return rc;
    ctx->po_ms = sc.ms[0];
    memcpy(res, results.down(b), results.bytes());
    // the reference writes a flag only where there is a correspondence (Optimizer.cc:650, :757, :976): the caller's other entries stay
    for (int f = 0; flags && f < n; f++) {
        const hvo_pose_problem &p = prob[f];
        const hvo_pose_flags &G = flags[f];
        const uint8_t *o_pt = pieces[f].pt_out.down(b), *o_ln = pieces[f].ln_out.down(b), *o_vp = pieces[f].vp_out.down(b), *o_pl = pieces[f].pl_out.down(b);
        for (int i = 0; G.pt_outlier && i < p.n_points; i++) if (p.pt_has[i]) G.pt_outlier[i] = o_pt[i];
        for (int i = 0; G.ln_outlier && i < p.n_lines; i++) if (p.ln_has[i]) G.ln_outlier[i] = o_ln[i];
        for (int i = 0; G.vp_outlier && i < p.n_lines; i++) G.vp_outlier[i] = o_vp[i];
        for (int i = 0; G.pl_outlier && i < 3 * p.n_planes; i++) {
            bool has;
            if (p.plane_map) { const int32_t *sl = i % 3 == 0 ? p.slot_match : (i % 3 == 1 ? p.slot_parallel : p.slot_vertical); has = sl && sl[i / 3] >= 0; }
            else has = p.pl_has[i] != 0;
            if (has) G.pl_outlier[i] = o_pl[i];
        }
    }
    return HVO_OK;
}
