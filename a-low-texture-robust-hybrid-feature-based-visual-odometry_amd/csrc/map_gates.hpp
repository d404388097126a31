// map_gates.hpp -- the atoms the matchers' projection gates and searches share, each stated once.  Only the atoms: how
// a call orders its gates, what a NaN does in its in-image test, and where it reads the reference differently stay with the call, which
// says so against the name here.  No contraction: everything is written with the __f*_rn / __d*_rn intrinsics.
#pragma once
#include "hvo_internal.hpp"

// ORBmatcher::DescriptorDistance on a 256-bit descriptor (src/ORBmatcher.cc:1676-1692): the sum of popcount(xor) over 4 x u64
static __device__ __forceinline__ int ham256(const ulonglong4 &a, const ulonglong4 &b)
{
    return __popcll(a.x ^ b.x) + __popcll(a.y ^ b.y) + __popcll(a.z ^ b.z) + __popcll(a.w ^ b.w);
}
// a descriptor's 32 bytes as 4 x u64: four 8-byte loads, which is all the alignment the callers' arrays promise
static __device__ __forceinline__ ulonglong4 ld256(const uint8_t *p)
{
    const unsigned long long *q = reinterpret_cast<const unsigned long long *>(p);
    return make_ulonglong4(q[0], q[1], q[2], q[3]);
}

// the predicted level's conversion to int: saturating, NaN -> 0
static __device__ __forceinline__ int sm_level(float lv)
{
    return lv != lv ? 0 : lv >= 2147483648.0f ? 2147483647 : lv <= -2147483648.0f ? (-2147483647 - 1) : (int)lv;
}

// MapPoint::PredictScale / MapLine::PredictScale before the clamp (src/MapPoint.cc:383-398 and :400-415, src/MapLine.cpp:557): float
// ratio, logf, float division, ceilf (sm_predict_lv, the float the text forms), then sm_level's conversion
static __device__ __forceinline__ float sm_predict_lv(float mfMax, float dist, float logsf)
{
    return ceilf(__fdiv_rn(logf(__fdiv_rn(mfMax, dist)), logsf));
}
static __device__ __forceinline__ int sm_predict_level(float mfMax, float dist, float logsf)
{
    return sm_level(sm_predict_lv(mfMax, dist, logsf));
}
// ... and its clamp to [0, n_levels - 1] (MapPoint.cc:392-395, :409-412)
static __device__ __forceinline__ int sm_clamp_level(int l, int n_levels)
{
    return l < 0 ? 0 : l >= n_levels ? n_levels - 1 : l;
}

// cv::norm of the entry's offset from the camera centre: sqrt of the double sum of squares, left to right, stored to float
static __device__ __forceinline__ float sm_dist3(double d0, double d1, double d2)
{
    return (float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2)));
}
// GetMaxDistanceInvariance / GetMinDistanceInvariance: float products
static __device__ __forceinline__ void sm_dist_band(float mfMax, float mfMin, float *maxD, float *minD)
{
    *maxD = __fmul_rn(1.2f, mfMax); *minD = __fmul_rn(0.8f, mfMin);
}

// u = fx * xc * invz + cx in float, left to right
static __device__ __forceinline__ float sm_pinhole(float f, float xc, float invz, float c)
{
    return __fadd_rn(__fmul_rn(__fmul_rn(f, xc), invz), c);
}
