// se3quat.hpp -- the g2o arithmetic the three optimisers share (pose_opt.hip, local_ba.hip, line_opt.hip), each reading stated once
// (tests/pose_opt_ref.py restates the same in numpy).  All of it in double, in the written order, uncontracted.
// A pose is seven doubles: the unit quaternion (w, x, y, z), then the translation.  Plain C++ up to the wave sum: a host compiler can
// include this header (tools/se3quat_host.cpp does), and local_ba.hip calls the quaternion functions on the host.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define SE3_HD __host__ __device__
#else
#define SE3_HD
#endif

// ---- SE3Quat (Thirdparty/g2o/g2o/types/se3quat.h) ----
static SE3_HD void quat_from_R(const double *m, double *q)                  // Eigen::Quaterniond(Matrix3d): (w, x, y, z)
{
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0); q[0] = 0.5 * t; t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t; q[2] = (m[2] - m[6]) * t; q[3] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0); q[1 + i] = 0.5 * t; t = 0.5 / t;
        q[0] = (m[3 * k + j] - m[3 * j + k]) * t; q[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t; q[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}
static SE3_HD void quat_normalize(double *q)                                // SE3Quat::normalizeRotation
{
    if (q[0] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}
static SE3_HD void quat_to_R(const double *q, double *R)                    // Eigen's toRotationMatrix
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
static SE3_HD void mat3(const double *A, const double *B, double *C)
{
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
// SE3Quat::exp(update) (se3quat.h:229-263)
static SE3_HD void se3_exp(const double *u, double *o)
{
    const double th = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    const double Om[9] = { 0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0 };
    double Om2[9]; mat3(Om, Om, Om2);
    double R[9], V[9];
    if (th < 0.00001) {
        for (int i = 0; i < 9; i++) { R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + Om[i]) + Om2[i]; V[i] = R[i]; }
    } else {
        const double s = sin(th), c = cos(th);
        const double a = s / th, b = (1 - c) / (th * th), g = (th - s) / (th * th * th);
        for (int i = 0; i < 9; i++) {
            const double I = i % 4 == 0 ? 1.0 : 0.0;
            R[i] = (I + a * Om[i]) + b * Om2[i];
            V[i] = (I + b * Om[i]) + g * Om2[i];
        }
    }
    quat_from_R(R, o); quat_normalize(o);
    for (int i = 0; i < 3; i++) o[4 + i] = (V[3 * i] * u[3] + V[3 * i + 1] * u[4]) + V[3 * i + 2] * u[5];
}
// SE3Quat::operator*; o may be a or b
static SE3_HD void se3_mul(const double *a, const double *b, double *o)
{
    const double *p = a, *q = b;
    double r[4];
    r[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
    r[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
    r[2] = p[0] * q[2] + p[2] * q[0] + p[3] * q[1] - p[1] * q[3];
    r[3] = p[0] * q[3] + p[3] * q[0] + p[1] * q[2] - p[2] * q[1];
    double Ra[9]; quat_to_R(a, Ra);
    double t[3];
    for (int i = 0; i < 3; i++) t[i] = a[4 + i] + ((Ra[3 * i] * b[4] + Ra[3 * i + 1] * b[5]) + Ra[3 * i + 2] * b[6]);
    quat_normalize(r);
    for (int i = 0; i < 4; i++) o[i] = r[i];
    for (int i = 0; i < 3; i++) o[4 + i] = t[i];
}
// the pose as R (row-major, 9) and t (3); points and planes are mapped with the quaternion's rotation matrix
static SE3_HD void se3_Rt(const double *p, double *Rt) { quat_to_R(p, Rt); Rt[9] = p[4]; Rt[10] = p[5]; Rt[11] = p[6]; }
static SE3_HD inline __attribute__((always_inline)) void se3_map(const double *Rt, const double *X, double *Y)
{
    Y[0] = ((Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2]) + Rt[9];
    Y[1] = ((Rt[3] * X[0] + Rt[4] * X[1]) + Rt[5] * X[2]) + Rt[10];
    Y[2] = ((Rt[6] * X[0] + Rt[7] * X[1]) + Rt[8] * X[2]) + Rt[11];
}

// RobustKernelHuber::robustify (core/robust_kernel_impl.cpp:78-91): rho and rho'.  A NaN takes the square-root branch.
static SE3_HD inline __attribute__((always_inline)) void huber(double e, double delta, double &r0, double &r1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) { r0 = e; r1 = 1.0; }
    else { const double s = sqrt(e); r0 = 2 * s * delta - dsqr; r1 = delta / s; }
}

// H x = b (H 6 x 6, row-major, its lower triangle read) by LDL^T without pivoting.  bad_pivot(D[j]) is the caller's rule for a failed
// solve; the factorisation and both substitutions run to the end either way.  Returns false when any pivot was bad.
template <class BadPivot>
static SE3_HD bool ldlt6_solve(const double *H, const double *b, double *x, BadPivot bad_pivot)
{
    double L[36], D[6], y[6]; bool ok = true;
    for (int j = 0; j < 6; j++) {
        double s = H[6 * j + j];
        for (int k = 0; k < j; k++) s = s - L[6 * j + k] * L[6 * j + k] * D[k];
        D[j] = s;
        if (bad_pivot(s)) ok = false;
        for (int i = j + 1; i < 6; i++) {
            double s2 = H[6 * i + j];
            for (int k = 0; k < j; k++) s2 = s2 - L[6 * i + k] * L[6 * j + k] * D[k];
            L[6 * i + j] = s2 / D[j];
        }
    }
    for (int i = 0; i < 6; i++) { double s = b[i]; for (int k = 0; k < i; k++) s = s - L[6 * i + k] * y[k]; y[i] = s; }
    for (int i = 5; i >= 0; i--) { double s = y[i] / D[i]; for (int k = i + 1; k < 6; k++) s = s - L[6 * k + i] * x[k]; x[i] = s; }
    return ok;
}

#ifdef __HIPCC__
// the sum over a wave's 64 lanes into lane 0: __shfl_down halving 32, 16, .., 1.  The callers keep their own order across waves.
static __device__ __forceinline__ double wave_sum_down(double x)
{
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, 64);
    return x;
}
#endif
