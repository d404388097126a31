// map_refresh.hip -- MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (reference src/MapPoint.cc:240-305, 328-369) and
// MapLine::ComputeDistinctiveDescriptors + UpdateAverageDir (src/MapLine.cpp:331-396, 404-455) for n features in one call with one
// synchronisation (a staged call: staged_call.hpp).
//
// No feature reads another's result, so the call is one launch: ONE WAVE (a work group of 64 lanes) PER FEATURE.
//   k_mr_points / k_mr_lines   the feature's good observers (kf_bad == 0) are listed in order by ballots; their descriptors are gathered
//                              into LDS (at most 256 x 32 B).  Lane l owns rows l, l + 64, ... of the N x N Hamming matrix and holds its
//                              row's descriptor in registers; the other rows are LDS broadcasts.  The row's median is the element at rank
//                              k = (N - 1) / 2 of the sorted row: the least v in 0 .. 256 with count(d <= v) >= k + 1, by nine bisection
//                              steps over the row -- no sort.  For N <= 64 the row's distances sit in LDS (written and read by the same
//                              lane, one column each, no bank conflict); above that they are recomputed in every step.  The winner is the
//                              wave minimum of median << 16 | index by shuffles: the least median, the first index among equals.
//                              Geometry: every lane forms the unit vectors of its observations into LDS, lane 0 adds them IN LIST ORDER
//                              (an ordered chain, float for points and double for lines) and writes the feature.
// A quarter-wave per feature would fit the typical N of 5 - 30 more tightly; nobody has measured either against the other, so no number
// favours this choice (profiles/map_refresh.txt has this form's times only).  No atomic is used.
//
// The slot forms write the map's device arrays in the same kernel; the host then copies the downloaded result into the map's mirror.
//
// Readings (tests/map_refresh_ref.py is the definition).  Only + - * / sqrt in the written order, nothing contracted.
//   the list                vDescriptors holds the rows of the observers that are not bad, in the map's order; N = its size
//   median                  vDists[0.5 * (N - 1)]: the double product truncated by the conversion to size_t = (N - 1) / 2; of the full
//                           row, the self-distance 0 included.  `median < BestMedian` keeps the first of equal medians
//   points: normali         mWorldPos - Owi in float; cv::norm a double sum of squares left to right, sqrt in double; Mat / scalar
//                           multiplies by the double reciprocal and rounds each element to float; `normal + ...` adds in float
//           normal / n      (float)((double)normal * (1.0 / (double)n)); n counts every observation, bad observers included
//           dist            (float)cv::norm(Pos - Ow_ref), the difference in float
//   lines:  middlePos       0.5 * (head + tail) in double; normali = middlePos - (double)Owi; norm() = sqrt((x x + y y) + z z);
//                           normali / norm() and normal / n are true double divisions
//           SP, EP          (float)Pos(k).  MP = 0.5 * (SP + EP): OpenCV is not in the reference tree, so this is a choice
//                           made here: the MatExpr a + b scaled by 0.5 is addWeighted(SP, 0.5, EP, 0.5), evaluated as
//                           (float)((double)SP * 0.5 + (double)EP * 0.5), one rounding.  Rounding the float sum first and halving it gives
//                           the same float unless SP + EP overflows or the result is subnormal
//           mWorldVector    head - tail in double.  Eigen is not in the reference tree either; normalize() is taken as Eigen 3.3's
//                           `z = squaredNorm(); if (z > 0) *this /= sqrt(z)`: a zero (or NaN) vector is left as it is, where Eigen 3.2
//                           would divide by zero
//   distance range          mfMaxDistance = dist * sf[level] and mfMinDistance = mfMaxDistance / sf[n_levels - 1], float.  sf is the
//                           context's ORB table for points; for lines sf[0] = 1, sf[l] = sf[l - 1] * scale_factor in float
#include "hvo_internal.hpp"
#include "slot_map.hpp"
#include "staged_call.hpp"
#include "triangulate4.inc"                 // np_normd
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#define MR_MAXOBS HVO_MR_MAX_OBS

struct MrDev {
    int n, n_levels, what, cap;                                  // cap: the map's capacity (slot form)
    const int32_t *obs_start; const uint8_t *obs_desc; const float *obs_Ow; const uint8_t *kf_bad;
    const float *ref_Ow; const int32_t *ref_level; const uint8_t *skip;
    const int32_t *slots;                                        // null: host-array form, pos is packed per feature
    const void *pos;                                             // points: float, lines: double; slot form: the map's component-major array
    const float *sf;
    int32_t *best_obs, *best_median; uint8_t *desc; void *normal; double *wvec; float *maxd, *mind; uint8_t *status;       // the staged result
    void *m_nrm; double *m_wvec; float *m_maxd, *m_mind; uint8_t *m_desc; const uint8_t *m_flags;                            // the map (slot form)
};

// ham256 (map_gates.hpp) over 32-bit words: the rows lie in LDS as uint32_t and are read word by word; ham256's 64-bit operands would change those loads
static __device__ __forceinline__ int mr_ham(const uint32_t *d, const uint32_t *e)
{
    int h = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) h += __popc(d[w] ^ e[w]);
    return h;
}

template <bool LINE> static __device__ __forceinline__ void mr_feature(const MrDev &a)
{
    typedef typename std::conditional<LINE, double, float>::type real;
    __shared__ uint32_t s_desc[MR_MAXOBS * 8];
    __shared__ uint16_t s_dist[64 * 64];                          // [j * 64 + lane]: the distance of the lane's row to row j (N <= 64)
    __shared__ uint8_t s_idx[MR_MAXOBS];                          // good observer -> its place in the feature's list
    __shared__ real s_unit[MR_MAXOBS * 3];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int s0 = a.obs_start[f], N = a.obs_start[f + 1] - s0;
    const int slot = a.slots ? a.slots[f] : f;
    const bool skip = a.skip[f] != 0 || (a.slots && (a.m_flags[slot] & SM_BAD));
    if (skip || N <= 0 || N > MR_MAXOBS) {                        // (uniform; N > 256 is refused by the host)
        if (lane == 0) { a.status[f] = skip ? HVO_MR_SKIPPED : HVO_MR_NO_OBS; a.best_obs[f] = -1; a.best_median[f] = -1; }
        return;
    }
    int status = HVO_MR_REFRESHED, best_obs = -1, best_median = -1;
    if (a.what & HVO_MR_DESCRIPTOR) {
        int ng = 0;
        for (int c0 = 0; c0 < N; c0 += 64) {
            const int i = c0 + lane;
            const bool good = i < N && a.kf_bad[s0 + i] == 0;
            const unsigned long long bm = __ballot(good);
            if (good) s_idx[ng + __popcll(bm & ((1ull << lane) - 1ull))] = (uint8_t)i;
            ng += __popcll(bm);
        }
        __syncthreads();
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.obs_desc);
        for (int w = lane; w < ng * 8; w += 64) s_desc[w] = src[(size_t)(s0 + s_idx[w >> 3]) * 8 + (w & 7)];
        __syncthreads();
        if (ng == 0) status = HVO_MR_DESC_KEPT;
        else {
            const int k = (ng - 1) >> 1;
            unsigned best = 0xFFFFFFFFu;
            for (int r0 = 0; r0 < ng; r0 += 64) {
                const int i = r0 + lane;
                const bool have = i < ng;
                uint32_t d[8];
#pragma unroll
                for (int w = 0; w < 8; w++) d[w] = s_desc[(have ? i : 0) * 8 + w];
                if (ng <= 64)
                    for (int j = 0; j < ng; j++) s_dist[j * 64 + lane] = (uint16_t)mr_ham(d, s_desc + j * 8);
                // the least v with count(d <= v) >= k + 1.  count(d <= 256) = ng holds at entry; an interval of 257 values is one
                // value after nine halvings, and a step on a one-value interval changes nothing
                int lo = 0, hi = 256;
                for (int s = 0; s < 9; s++) {
                    const int mid = (lo + hi) >> 1;
                    int cnt = 0;
                    if (ng <= 64) for (int j = 0; j < ng; j++) cnt += s_dist[j * 64 + lane] <= mid ? 1 : 0;
                    else for (int j = 0; j < ng; j++) cnt += mr_ham(d, s_desc + j * 8) <= mid ? 1 : 0;
                    if (cnt >= k + 1) hi = mid; else lo = mid + 1;
                }
                const unsigned key = ((unsigned)lo << 16) | (unsigned)i;
                if (have && key < best) best = key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { const unsigned v = __shfl_xor(best, o); best = v < best ? v : best; }
            const int bi = (int)(best & 0xFFFFu);
            best_obs = s_idx[bi]; best_median = (int)(best >> 16);
            if (lane < 8) {
                const uint32_t w = s_desc[bi * 8 + lane];
                reinterpret_cast<uint32_t *>(a.desc)[(size_t)f * 8 + lane] = w;
                if (a.slots) reinterpret_cast<uint32_t *>(a.m_desc)[(size_t)slot * 8 + lane] = w;
            }
        }
    }
    if (a.what & HVO_MR_GEOMETRY) {
        const size_t cap = (size_t)a.cap;
        real P[LINE ? 6 : 3];
#pragma unroll
        for (int c = 0; c < (LINE ? 6 : 3); c++) P[c] = a.slots ? ((const real *)a.pos)[c * cap + slot] : ((const real *)a.pos)[(size_t)f * (LINE ? 6 : 3) + c];
        real M[3];                                                // what the viewing directions start from
#pragma unroll
        for (int c = 0; c < 3; c++) { if constexpr (LINE) M[c] = 0.5 * (P[c] + P[3 + c]); else M[c] = P[c]; }
        for (int i = lane; i < N; i += 64) {
            const float *O = a.obs_Ow + 3 * (size_t)(s0 + i);
            if constexpr (LINE) {
                const double x = M[0] - (double)O[0], y = M[1] - (double)O[1], z = M[2] - (double)O[2];
                const double nn = sqrt((x * x + y * y) + z * z);
                s_unit[3 * i] = x / nn; s_unit[3 * i + 1] = y / nn; s_unit[3 * i + 2] = z / nn;
            } else {
                const float x = M[0] - O[0], y = M[1] - O[1], z = M[2] - O[2];
                const double inv = 1.0 / np_normd(x, y, z);
                s_unit[3 * i] = (float)((double)x * inv); s_unit[3 * i + 1] = (float)((double)y * inv); s_unit[3 * i + 2] = (float)((double)z * inv);
            }
        }
        __syncthreads();
        const int level = a.ref_level[f];
        const bool lvl_ok = level >= 0 && level < a.n_levels;
        if (!lvl_ok && status == HVO_MR_REFRESHED) status = HVO_MR_BAD_LEVEL;
        if (lane == 0) {
            real sx = 0, sy = 0, sz = 0;
            for (int i = 0; i < N; i++) { sx = sx + s_unit[3 * i]; sy = sy + s_unit[3 * i + 1]; sz = sz + s_unit[3 * i + 2]; }
            const float *Or = a.ref_Ow + 3 * (size_t)f;
            float cm[3];
            if constexpr (LINE) {
                const double dn = (double)N;
                sx = sx / dn; sy = sy / dn; sz = sz / dn;
#pragma unroll
                for (int c = 0; c < 3; c++) { const float sp = (float)P[c], ep = (float)P[3 + c]; cm[c] = (float)((double)sp * 0.5 + (double)ep * 0.5) - Or[c]; }
                double wx = P[0] - P[3], wy = P[1] - P[4], wz = P[2] - P[5];
                const double z = (wx * wx + wy * wy) + wz * wz;
                if (z > 0.0) { const double r = sqrt(z); wx = wx / r; wy = wy / r; wz = wz / r; }
                a.wvec[3 * (size_t)f] = wx; a.wvec[3 * (size_t)f + 1] = wy; a.wvec[3 * (size_t)f + 2] = wz;
                if (a.slots) { a.m_wvec[slot] = wx; a.m_wvec[cap + slot] = wy; a.m_wvec[2 * cap + slot] = wz; }
            } else {
                const double in = 1.0 / (double)N;
                sx = (float)((double)sx * in); sy = (float)((double)sy * in); sz = (float)((double)sz * in);
#pragma unroll
                for (int c = 0; c < 3; c++) cm[c] = P[c] - Or[c];
            }
            real *nrm = (real *)a.normal + 3 * (size_t)f;
            nrm[0] = sx; nrm[1] = sy; nrm[2] = sz;
            if (a.slots) { real *mn = (real *)a.m_nrm; mn[slot] = sx; mn[cap + slot] = sy; mn[2 * cap + slot] = sz; }
            if (lvl_ok) {
                const float dist = (float)np_normd(cm[0], cm[1], cm[2]);
                const float mx = dist * a.sf[level], mi = mx / a.sf[a.n_levels - 1];
                a.maxd[f] = mx; a.mind[f] = mi;
                if (a.slots) { a.m_maxd[slot] = mx; a.m_mind[slot] = mi; }
            }
        }
    }
    if (lane == 0) { a.status[f] = (uint8_t)status; a.best_obs[f] = best_obs; a.best_median[f] = best_median; }
}

__global__ __launch_bounds__(64) void k_mr_points(MrDev a) { mr_feature<false>(a); }
__global__ __launch_bounds__(64) void k_mr_lines(MrDev a) { mr_feature<true>(a); }

// What the two calls share.  m null: the host-array form on pos.  The map's arrays are named by their indices in the slot map's table
struct MrMapCols { int pos, nrm, wvec, maxd, mind, desc; };
struct MrOut { int32_t *best_obs, *best_median; uint8_t *desc; void *normal; double *wvec; float *maxd, *mind; uint8_t *status; float *kernel_ms; };

template <bool LINE> static int mr_run(hvo_ctx *ctx, hvo_slot_map *m, const MrMapCols &col, const int32_t *slots, const hvo_mr_params *P, const hvo_mr_input *in,
                                       const void *pos, const MrOut &out, std::string *err)
{
    typedef typename std::conditional<LINE, double, float>::type real;
    const char *who = LINE ? "refresh map lines: " : "refresh map points: ";
    const int n = in->n;
    // ---- refusals: whole, before anything is written ----
    if (n < 0) { *err = std::string(who) + "n < 0"; return HVO_ERR_INVALID_ARG; }
    if (P->what == 0 || (P->what & ~(HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY))) { *err = std::string(who) + "what is 0 or has unknown bits"; return HVO_ERR_INVALID_ARG; }
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { *err = std::string(who) + "n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (!LINE && P->n_levels > ctx->p.orb_nlevels) { *err = std::string(who) + "n_levels beyond the context's ORB pyramid"; return HVO_ERR_INVALID_ARG; }
    if (m && m->device != ctx->device) { *err = std::string(who) + "the map lives on another device"; return HVO_ERR_INVALID_ARG; }
    if (n == 0) { *out.kernel_ms = 0.f; return HVO_OK; }
    if (n > HVO_MR_MAX_FEATURES) { *err = std::string(who) + std::to_string(n) + " features (limit " + std::to_string(HVO_MR_MAX_FEATURES) + "); nothing was written"; return HVO_ERR_UNSUPPORTED; }
    if (!in->obs_start || !in->ref_Ow || !in->ref_level || (m ? !slots : !pos)) { *err = std::string(who) + "a missing array"; return HVO_ERR_INVALID_ARG; }
    if (in->obs_start[0] != 0) { *err = std::string(who) + "obs_start[0] is not 0"; return HVO_ERR_INVALID_ARG; }
    int most = 0;
    for (int i = 0; i < n; i++) {
        const int64_t c = (int64_t)in->obs_start[i + 1] - (int64_t)in->obs_start[i];
        if (c < 0) { *err = std::string(who) + "obs_start decreases at feature " + std::to_string(i); return HVO_ERR_INVALID_ARG; }
        most = std::max<int64_t>(most, std::min<int64_t>(c, INT_MAX));
    }
    const size_t no = (size_t)in->obs_start[n];
    if (no > 0 && (!in->obs_desc || !in->obs_Ow)) { *err = std::string(who) + "a missing array"; return HVO_ERR_INVALID_ARG; }
    if (m) {
        std::vector<uint8_t> seen((size_t)m->n_slots, 0);
        for (int i = 0; i < n; i++) {
            if (slots[i] < 0 || slots[i] >= m->n_slots) { *err = std::string(who) + "slot " + std::to_string(slots[i]) + " is outside the map"; return HVO_ERR_INVALID_ARG; }
            if (seen[(size_t)slots[i]]) { *err = std::string(who) + "slot " + std::to_string(slots[i]) + " is listed twice"; return HVO_ERR_INVALID_ARG; }
            seen[(size_t)slots[i]] = 1;
        }
    }
    if (most > MR_MAXOBS) { *err = std::string(who) + std::to_string(most) + " observations of one feature (limit " + std::to_string(MR_MAXOBS) + "); nothing was written"; return HVO_ERR_UNSUPPORTED; }
    if (no > HVO_MR_MAX_OBS_TOTAL) { *err = std::string(who) + std::to_string(no) + " observations (limit " + std::to_string(HVO_MR_MAX_OBS_TOTAL) + "); nothing was written"; return HVO_ERR_UNSUPPORTED; }
    *out.kernel_ms = 0.f;
    // ---- one carve of the context's arena: what goes up, then what is cleared and comes down ----
    const size_t N = (size_t)n, npos = LINE ? 6 : 3;
    hipStream_t st = ctx->stream;
    StageCarver C(256);
    const auto u_start = C.take<int32_t>(N + 1); const auto u_desc = C.take<uint8_t>(no * 32); const auto u_ow = C.take<float>(no * 3); const auto u_bad = C.take<uint8_t>(no);
    const auto u_row = C.take<float>(N * 3); const auto u_lvl = C.take<int32_t>(N); const auto u_skip = C.take<uint8_t>(N); const auto u_sf = C.take<float>(HVO_MAX_LEVELS);
    const auto u_slot = C.take<int32_t>(m ? N : 0); const auto u_pos = C.take<real>(m ? 0 : N * npos);
    const size_t up_end = C.mark(), r0 = up_end;                  // [r0, r1) is zeroed and comes down
    const auto r_bo = C.take<int32_t>(N), r_bm = C.take<int32_t>(N); const auto r_desc = C.take<uint8_t>(N * 32); const auto r_nrm = C.take<real>(N * 3);
    const auto r_wv = C.take<double>(LINE ? N * 3 : 0); const auto r_mx = C.take<float>(N), r_mi = C.take<float>(N); const auto r_st = C.take<uint8_t>(N);
    const size_t r1 = C.mark();
    StagedCall sc(ctx, st, who, err); int rc;
    if ((rc = sc.begin(r1, up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    memcpy(u_start.host(h), in->obs_start, (N + 1) * 4);
    if (no) { memcpy(u_desc.host(h), in->obs_desc, no * 32); memcpy(u_ow.host(h), in->obs_Ow, no * 12); if (in->kf_bad) memcpy(u_bad.host(h), in->kf_bad, no); }
    memcpy(u_row.host(h), in->ref_Ow, N * 12); memcpy(u_lvl.host(h), in->ref_level, N * 4);
    if (in->skip) memcpy(u_skip.host(h), in->skip, N);
    float *sf = u_sf.host(h), v = 1.0f;
    for (int l = 0; l < HVO_MAX_LEVELS; l++) {
        if (LINE) { if (l > 0 && l < P->n_levels) v = v * P->scale_factor; sf[l] = l < P->n_levels ? v : 1.0f; }
        else sf[l] = l < P->n_levels ? ctx->scale[l] : 1.0f;
    }
    if (m) memcpy(u_slot.host(h), slots, N * 4); else memcpy(u_pos.host(h), pos, N * npos * sizeof(real));
    if ((rc = sc.up(0, up_end)) || (rc = sc.clear(r0, r1))) return rc;
    sc.tick();
    MrDev a; memset(&a, 0, sizeof(a));
    a.n = n; a.n_levels = P->n_levels; a.what = P->what;
    a.obs_start = u_start.dev(d); a.obs_desc = u_desc.dev(d); a.obs_Ow = u_ow.dev(d); a.kf_bad = u_bad.dev(d);
    a.ref_Ow = u_row.dev(d); a.ref_level = u_lvl.dev(d); a.skip = u_skip.dev(d); a.sf = u_sf.dev(d);
    a.best_obs = r_bo.dev(d); a.best_median = r_bm.dev(d); a.desc = r_desc.dev(d); a.normal = r_nrm.dev(d); a.wvec = r_wv.dev(d);
    a.maxd = r_mx.dev(d); a.mind = r_mi.dev(d); a.status = r_st.dev(d);
    if (m) {
        a.slots = u_slot.dev(d); a.cap = m->cap; a.pos = m->arr[col.pos].d; a.m_nrm = m->arr[col.nrm].d; a.m_wvec = LINE ? (double *)m->arr[col.wvec].d : nullptr;
        a.m_maxd = (float *)m->arr[col.maxd].d; a.m_mind = (float *)m->arr[col.mind].d; a.m_desc = (uint8_t *)m->arr[col.desc].d; a.m_flags = m->d_flags();
    } else a.pos = u_pos.dev(d);
    if (LINE) hipLaunchKernelGGL(k_mr_lines, dim3((unsigned)n), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(k_mr_points, dim3((unsigned)n), dim3(64), 0, st, a);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    *out.kernel_ms = sc.ms[0];
    // ---- what the status says was written goes to the caller's arrays and, in the slot form, to the map's mirror ----
    const int32_t *bo = r_bo.down(b), *bm = r_bm.down(b); const uint8_t *ds = r_desc.down(b), *stt = r_st.down(b);
    const real *nr = r_nrm.down(b); const double *wv = LINE ? r_wv.down(b) : nullptr; const float *mx = r_mx.down(b), *mi = r_mi.down(b);
    const size_t cap = m ? (size_t)m->cap : 0;
    for (size_t i = 0; i < N; i++) {
        const int s = stt[i];
        const bool alive = s != HVO_MR_SKIPPED && s != HVO_MR_NO_OBS, geo = alive && (P->what & HVO_MR_GEOMETRY);
        const bool dsc = bo[i] >= 0, rng = geo && in->ref_level[i] >= 0 && in->ref_level[i] < P->n_levels;
        const size_t j = m ? (size_t)slots[i] : 0;
        if (out.status) out.status[i] = (uint8_t)s;
        if (out.best_obs) out.best_obs[i] = bo[i];
        if (out.best_median) out.best_median[i] = bm[i];
        if (dsc) {
            if (out.desc) memcpy(out.desc + 32 * i, ds + 32 * i, 32);
            if (m) memcpy(m->arr[col.desc].h.data() + 32 * j, ds + 32 * i, 32);
        }
        if (geo) {
            if (out.normal) memcpy((real *)out.normal + 3 * i, nr + 3 * i, 3 * sizeof(real));
            if (LINE && out.wvec) memcpy(out.wvec + 3 * i, wv + 3 * i, 24);
            if (m) for (int c = 0; c < 3; c++) {
                ((real *)m->arr[col.nrm].h.data())[c * cap + j] = nr[3 * i + c];
                if (LINE) ((double *)m->arr[col.wvec].h.data())[c * cap + j] = wv[3 * i + c];
            }
        }
        if (rng) {
            if (out.maxd) out.maxd[i] = mx[i];
            if (out.mind) out.mind[i] = mi[i];
            if (m) { ((float *)m->arr[col.maxd].h.data())[j] = mx[i]; ((float *)m->arr[col.mind].h.data())[j] = mi[i]; }
        }
    }
    return HVO_OK;
}

static MrOut mr_out(hvo_mr_point_out *o) { return MrOut{ o->best_obs, o->best_median, o->desc, o->normal, nullptr, o->max_dist, o->min_dist, o->status, &o->kernel_ms }; }
static MrOut mr_out(hvo_mr_line_out *o) { return MrOut{ o->best_obs, o->best_median, o->desc, o->normal, o->wvec, o->max_dist, o->min_dist, o->status, &o->kernel_ms }; }

extern "C" {

int hvo_refresh_map_points(hvo_ctx *ctx, const hvo_mr_params *params, const hvo_mr_input *in, const float *pos, hvo_mr_point_out *out)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!params || !in || !out) { ctx->last_error = "refresh map points: a null argument"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return mr_run<false>(ctx, nullptr, MrMapCols{}, nullptr, params, in, pos, mr_out(out), &ctx->last_error);
}

int hvo_refresh_map_lines(hvo_ctx *ctx, const hvo_mr_params *params, const hvo_mr_input *in, const double *pos, hvo_mr_line_out *out)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!params || !in || !out) { ctx->last_error = "refresh map lines: a null argument"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return mr_run<true>(ctx, nullptr, MrMapCols{}, nullptr, params, in, pos, mr_out(out), &ctx->last_error);
}

int hvo_point_map_refresh(hvo_ctx *ctx, hvo_point_map *m, const int32_t *slots, const hvo_mr_params *params, const hvo_mr_input *in, hvo_mr_point_out *out)
{
    if (!ctx || !m) return HVO_ERR_INVALID_ARG;
    if (!params || !in || !out) { m->last_error = ctx->last_error = "refresh map points: a null argument"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const MrMapCols col = { m->POS, m->NRM, -1, m->MAXD, m->MIND, m->DESC };
    const int rc = mr_run<false>(ctx, m, col, slots, params, in, nullptr, mr_out(out), &ctx->last_error);
    if (rc) m->last_error = ctx->last_error;
    return rc;
}

int hvo_line_map_refresh(hvo_ctx *ctx, hvo_line_map *m, const int32_t *slots, const hvo_mr_params *params, const hvo_mr_input *in, hvo_mr_line_out *out)
{
    if (!ctx || !m) return HVO_ERR_INVALID_ARG;
    if (!params || !in || !out) { m->last_error = ctx->last_error = "refresh map lines: a null argument"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const MrMapCols col = { m->POS, m->NRM, m->WVEC, m->MAXD, m->MIND, m->DESC };
    const int rc = mr_run<true>(ctx, m, col, slots, params, in, nullptr, mr_out(out), &ctx->last_error);
    if (rc) m->last_error = ctx->last_error;
    return rc;
}

}   // extern "C"
