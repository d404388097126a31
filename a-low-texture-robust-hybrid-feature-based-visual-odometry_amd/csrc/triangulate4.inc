// triangulate4.inc -- the float / double readings that the two triangulating calls share (included by new_points.hip, line_triang.hip
// and, for cv::norm, map_refresh.hip): the 3-term sums, cv::norm, OpenCV's closed 3 x 3 inverse, the float 3 x 3 product and the 4 x 4
// cv::SVD::compute of a linear triangulation.  The readings themselves are stated at the head of new_points.hip; tests/new_points_ref.py is
// their definition.  Only + - * / sqrt in the written order: the including file is compiled with -ffp-contract=off.
#pragma once

#define NP_SWEEPS 12

static __host__ __device__ __forceinline__ float np_dot3f(float a0, float a1, float a2, float b0, float b1, float b2)
{
    float s = a0 * b0; s = s + a1 * b1; s = s + a2 * b2;
    return s;
}
static __host__ __device__ __forceinline__ float np_row(float a0, float a1, float a2, float b0, float b1, float b2, float c)
{
    return (float)((double)np_dot3f(a0, a1, a2, b0, b1, b2) * 1.0 + (double)c * 1.0);
}
static __host__ __device__ __forceinline__ double np_dotd(float a0, float a1, float a2, float b0, float b1, float b2)
{
    double s = (double)a0 * (double)b0; s = s + (double)a1 * (double)b1; s = s + (double)a2 * (double)b2;
    return s;
}
static __host__ __device__ __forceinline__ double np_normd(float a0, float a1, float a2) { return sqrt(np_dotd(a0, a1, a2, a0, a1, a2)); }

// pnp_core.inc's pnp_rot: the rotation that zeroes the pair
static __host__ __device__ __forceinline__ void np_rot(double num, double den2, double *c, double *s)
{
    if (den2 * 0.5 == 0.0) { *c = 1.0; *s = 0.0; return; }
    const double th = num / den2;
    const double at = th < 0.0 ? -th : th;
    double tt = 1.0 / (at + sqrt(th * th + 1.0));
    if (th < 0.0) tt = -tt;
    const double cc = 1.0 / sqrt(tt * tt + 1.0);
    *c = cc; *s = tt * cc;
}

// the right singular vector of the smallest singular value of the 4 x 4 float A, rounded to float once.  Every index is a compile-time
// constant once the loops unroll, so W and V live in registers.
static __host__ __device__ __forceinline__ void np_svd4(const float (&A)[4][4], float (&x)[4])
{
    double W[4][4], V[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) { W[r][c] = (double)A[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sw = 0; sw < NP_SWEEPS; sw++) {
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) { const double wp = W[r][p], wq = W[r][q]; al = al + wp * wp; be = be + wq * wq; ga = ga + wp * wq; }
                double c, s; np_rot(be - al, 2.0 * ga, &c, &s);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const double wp = W[r][p], wq = W[r][q], vp = V[r][p], vq = V[r][q];
                    W[r][p] = c * wp - s * wq; W[r][q] = s * wp + c * wq;
                    V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
                }
            }
        }
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        double s2 = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) { const double w = W[r][c]; s2 = s2 + w * w; }
        if (c == 0 || s2 <= best) {                                  // the highest index among equals (a NaN norm never wins over column 0)
            best = s2;
#pragma unroll
            for (int r = 0; r < 4; r++) x[r] = (float)V[r][c];
        }
    }
}

// OpenCV's closed form of a 3 x 3 inverse on float entries
static void np_inv3(const float *m, float *o)
{
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5], a20 = m[6], a21 = m[7], a22 = m[8];
    double d = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    d = 1.0 / d;
    o[0] = (float)((a11 * a22 - a12 * a21) * d); o[1] = (float)((a02 * a21 - a01 * a22) * d); o[2] = (float)((a01 * a12 - a02 * a11) * d);
    o[3] = (float)((a12 * a20 - a10 * a22) * d); o[4] = (float)((a00 * a22 - a02 * a20) * d); o[5] = (float)((a02 * a10 - a00 * a12) * d);
    o[6] = (float)((a10 * a21 - a11 * a20) * d); o[7] = (float)((a01 * a20 - a00 * a21) * d); o[8] = (float)((a00 * a11 - a01 * a10) * d);
}
static void np_mul3(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) C[3 * r + c] = np_dot3f(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
