// local_points.hip -- the point side of Tracking::TrackLocalMapWithLines against map points that stay on the device (hvo_point_map):
//   Tracking::SearchLocalPoints (reference src/Tracking.cc:3227-3277) with Frame::isInFrustum(MapPoint *, 0.5) (src/Frame.cc:1371-1427),
//   MapPoint::PredictScale (src/MapPoint.cc:400-415) and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-132)
//   through the search core of match.hip, unchanged (k_track_windows, k_search_by_projection, k_sbp_epilogue in map_mode).
//
// The map.  Per slot (= position in mvpLocalMapPoints): GetWorldPos() and GetNormal() (3 floats each, both CV_32F), mfMaxDistance and
// mfMinDistance (raw floats), GetDescriptor() (32 bytes) and one flag byte (bit 0 bad, bit 1 Observations() > 0).  Every component is an
// array of its own over the slots, as in the line map (local_lines.hip): the frustum kernel runs one lane per slot, so a wave's load of one
// component covers 256 contiguous bytes.  The descriptor is consumed whole, 32 bytes by one lane of the gather, and stays packed.  The host
// mirror is the truth; storage grows only, by a new allocation and one upload of the mirror.
//
// The call, the same kernels for the host, stream and batch forms (bit-identical results):
//   k_lp_mark      per frame feature: a held slot that is bad becomes -1; t_occupied = the feature holds an observed point (a slot with the
//                  observed flag, or HVO_HELD_FOREIGN_OBSERVED); the held slots and the caller's seen_extra slots are marked seen
//   k_lp_frustum   one lane per slot, the slot loaded ONCE and tested under every frame's pose: bad / seen skip, isInFrustum as written,
//                  PredictScale with its clamp; per (frame, slot) a pass flag and the projection, per (frame, block) the survivors
//   k_lp_compact   the survivors in ASCENDING SLOT ORDER: position = (sum of the counts of the blocks before) + (wave ballot prefix inside
//                  the block).  No atomic decides an order.  u, v, ur, level, view cosine, descriptor and observation flag are gathered
//                  by slot straight into the arrays SbpDev names.
//   -- the in-view counts come down here: the search core's grid is one wave per query, so the host has to know them; more than 16384
//      in view is refused (HVO_ERR_UNSUPPORTED) with `held` untouched --
//   k_track_windows, k_search_by_projection, k_sbp_epilogue (match.hip, unchanged) on the device-resident queries
//   k_lp_assign    F.mvpMapPoints[bestIdx] = pMP in query order: the LAST query that matched a feature keeps it (two unobserved points may
//                  take one feature), taken as an atomicMax of the query index per feature (a maximum does not depend on operand order)
//   k_lp_apply     held[i] = the slot of the winning query
//
// Readings (OpenCV is not in the reference tree; DESIGN.md section 7, tests/point_map_ref.py restates the same):
//   mRcw * P + mtcw              as k_project_last (match.hip): the row's three products summed in FLOAT left to right, then
//                                (float)((double)sum * 1.0 + (double)t * 1.0)
//   PcZ < 0.0f                   as written: z == 0 and -0.0 pass and divide; a NaN projection passes the four bounds tests
//   invz, u, v, ur               one float division; fx * PcX * invz + cx in float, left to right; u - mbf * invz
//   mOw                          -Rcw^T tcw with double sums, times -1.0, rounded to float (match_project_setup's twc)
//   P - mOw                      float, element-wise
//   cv::norm                     sqrt of the double sum of squares, stored to float
//   PO.dot(Pn) / dist            Mat::dot accumulates in double; / the float dist in double; rounded to the float viewCos
//   PredictScale                 float ratio; MapPoint.cc writes unique_lock<mutex> unqualified, so it sits under `using namespace std` with
//                                <cmath> reached through its headers, as MapLine.cpp does: log and ceil are the FLOAT overloads, the division
//                                by mfLogScaleFactor is float; the conversion to int saturates (NaN -> 0) and the clamp to
//                                [0, mnScaleLevels - 1] is part of the function.  The search reads the level (radius, band).
// No contraction (-ffp-contract=off, __f*_rn).
#include "hvo_internal.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#define LP_BLOCK 256
#define LP_BAD 1
#define LP_OBS 2
#define LP_MAXQ 16384             // points in view per call (SBP_MAXQ of match.hip)
#define LP_MAXT 65535             // frame features (the search core's keys hold the feature in 16 bits)

struct hvo_point_map {
    int device = 0;
    hipStream_t st = nullptr;                                    // the map's own uploads
    int n_slots = 0, cap = 0;
    std::vector<float> h_pos, h_nrm;                             // component-major: component c of slot j at [c * cap + j]
    std::vector<float> h_maxd, h_mind;
    std::vector<uint8_t> h_desc, h_flags;
    float *d_pos = nullptr, *d_nrm = nullptr, *d_maxd = nullptr, *d_mind = nullptr;
    uint8_t *d_desc = nullptr, *d_flags = nullptr;
    char *d_a = nullptr, *d_b = nullptr; size_t a_bytes = 0, b_bytes = 0;    // the calls' scratch (before / after the in-view counts), grow-only
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    std::string last_error;
};

#define PM_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { m->last_error = std::string(#call) + ": " + hipGetErrorString(e_); return HVO_ERR_HIP; } } while (0)

static size_t lp_al(size_t v) { return (v + 255) & ~(size_t)255; }

static void pm_free_device(hvo_point_map *m)
{
    void *p[] = { m->d_pos, m->d_nrm, m->d_maxd, m->d_mind, m->d_desc, m->d_flags };
    for (void *q : p) if (q) (void)hipFree(q);
    m->d_pos = m->d_nrm = m->d_maxd = m->d_mind = nullptr; m->d_desc = m->d_flags = nullptr;
}

// slots [first, first + n) of the host mirror -> device
static int pm_upload(hvo_point_map *m, int first, int n)
{
    if (n <= 0) return HVO_OK;
    const size_t cap = (size_t)m->cap, f = (size_t)first, c = (size_t)n;
    for (int k = 0; k < 3; k++) PM_HIP(hipMemcpyAsync(m->d_pos + k * cap + f, m->h_pos.data() + k * cap + f, c * 4, hipMemcpyHostToDevice, m->st));
    for (int k = 0; k < 3; k++) PM_HIP(hipMemcpyAsync(m->d_nrm + k * cap + f, m->h_nrm.data() + k * cap + f, c * 4, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipMemcpyAsync(m->d_maxd + f, m->h_maxd.data() + f, c * 4, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipMemcpyAsync(m->d_mind + f, m->h_mind.data() + f, c * 4, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipMemcpyAsync(m->d_desc + f * 32, m->h_desc.data() + f * 32, c * 32, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipMemcpyAsync(m->d_flags + f, m->h_flags.data() + f, c, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipStreamSynchronize(m->st));
    return HVO_OK;
}

// room for `want` slots.  The new device arrays are allocated first: when one allocation fails nothing of the map has changed.  After a
// regrowth (*regrown) the device arrays are empty and the caller uploads every slot in use.
static int pm_reserve(hvo_point_map *m, int want, bool *regrown)
{
    *regrown = false;
    if (want <= m->cap) return HVO_OK;
    int cap = std::max(m->cap, 64);
    while (cap < want) cap *= 2;
    const size_t c = (size_t)cap;
    const size_t bytes[6] = { c * 12, c * 12, c * 4, c * 4, c * 32, c };
    void *nd[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    for (int k = 0; k < 6; k++)
        if (hipMalloc(&nd[k], bytes[k]) != hipSuccess) {
            for (int q = 0; q < k; q++) (void)hipFree(nd[q]);
            m->last_error = "point map: hipMalloc of the slot arrays"; return HVO_ERR_HIP;
        }
    // the mirror moves to the new component stride
    auto regrid = [&](std::vector<float> &v) {
        std::vector<float> nv((size_t)3 * cap, 0.f);
        for (int k = 0; k < 3; k++) for (int j = 0; j < m->n_slots; j++) nv[(size_t)k * cap + j] = v[(size_t)k * m->cap + j];
        v.swap(nv);
    };
    regrid(m->h_pos); regrid(m->h_nrm);
    m->h_maxd.resize(cap, 0.f); m->h_mind.resize(cap, 0.f); m->h_desc.resize((size_t)cap * 32, 0); m->h_flags.resize(cap, LP_BAD);
    pm_free_device(m);
    m->d_pos = (float *)nd[0]; m->d_nrm = (float *)nd[1]; m->d_maxd = (float *)nd[2]; m->d_mind = (float *)nd[3];
    m->d_desc = (uint8_t *)nd[4]; m->d_flags = (uint8_t *)nd[5];
    m->cap = cap; *regrown = true;
    return HVO_OK;
}

extern "C" {

hvo_point_map *hvo_point_map_create(int device, int slots)
{
    if (device < 0 || slots < 0 || slots > HVO_POINT_MAP_MAX_SLOTS) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hvo_point_map *m = new hvo_point_map();
    m->device = device;
    if (hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) != hipSuccess) { m->st = nullptr; hvo_point_map_destroy(m); return nullptr; }
    for (int k = 0; k < 4; k++) if (hipEventCreate(&m->ev[k]) != hipSuccess) { m->ev[k] = nullptr; hvo_point_map_destroy(m); return nullptr; }
    bool regrown;
    if (pm_reserve(m, std::max(slots, 1), &regrown)) { hvo_point_map_destroy(m); return nullptr; }
    return m;
}

void hvo_point_map_destroy(hvo_point_map *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->st) { (void)hipStreamSynchronize(m->st); (void)hipStreamDestroy(m->st); }
    for (int k = 0; k < 4; k++) if (m->ev[k]) (void)hipEventDestroy(m->ev[k]);
    pm_free_device(m);
    if (m->d_a) (void)hipFree(m->d_a);
    if (m->d_b) (void)hipFree(m->d_b);
    delete m;
}

int hvo_point_map_set_many(hvo_point_map *m, int first, int n, const float *pos, const float *normal, const float *max_dist, const float *min_dist,
                           const uint8_t *desc, const uint8_t *observed, const uint8_t *bad)
{
    if (!m || first < 0 || n < 0) return HVO_ERR_INVALID_ARG;
    if ((int64_t)first + n > HVO_POINT_MAP_MAX_SLOTS) { m->last_error = "point map: more than HVO_POINT_MAP_MAX_SLOTS slots"; return HVO_ERR_UNSUPPORTED; }
    if (n == 0) return HVO_OK;
    if (!pos || !normal || !max_dist || !min_dist || !desc) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    int rc; bool regrown;
    if ((rc = pm_reserve(m, first + n, &regrown))) return rc;
    const size_t cap = (size_t)m->cap;
    for (int i = 0; i < n; i++) {
        const size_t j = (size_t)first + i;
        for (int k = 0; k < 3; k++) { m->h_pos[k * cap + j] = pos[3 * (size_t)i + k]; m->h_nrm[k * cap + j] = normal[3 * (size_t)i + k]; }
        m->h_maxd[j] = max_dist[i]; m->h_mind[j] = min_dist[i];
        memcpy(&m->h_desc[j * 32], desc + 32 * (size_t)i, 32);
        m->h_flags[j] = (uint8_t)(((bad && bad[i]) ? LP_BAD : 0) | ((!observed || observed[i]) ? LP_OBS : 0));
    }
    const int old = m->n_slots;                                  // the slots skipped over stay bad (the mirror's default)
    if (first + n > m->n_slots) m->n_slots = first + n;
    if (regrown) return pm_upload(m, 0, m->n_slots);             // fresh device arrays: every slot in use, once
    const int lo = std::min(first, old), hi = first + n;
    return pm_upload(m, lo, hi - lo);
}

int hvo_point_map_set(hvo_point_map *m, int slot, const float pos[3], const float normal[3], float max_dist, float min_dist, const uint8_t desc[32],
                      int observed)
{
    const uint8_t o = observed ? 1 : 0;
    return hvo_point_map_set_many(m, slot, 1, pos, normal, &max_dist, &min_dist, desc, &o, nullptr);
}

static int pm_set_flag(hvo_point_map *m, int slot, int bit, int on)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    m->h_flags[slot] = (uint8_t)(on ? (m->h_flags[slot] | bit) : (m->h_flags[slot] & ~bit));
    PM_HIP(hipMemcpyAsync(m->d_flags + slot, &m->h_flags[slot], 1, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipStreamSynchronize(m->st));
    return HVO_OK;
}

int hvo_point_map_set_bad(hvo_point_map *m, int slot, int bad) { return pm_set_flag(m, slot, LP_BAD, bad); }
int hvo_point_map_set_observed(hvo_point_map *m, int slot, int observed) { return pm_set_flag(m, slot, LP_OBS, observed); }

int hvo_point_map_counts(const hvo_point_map *m, int *n_slots, int *n_good, int *n_observed)
{
    if (!m) return HVO_ERR_INVALID_ARG;
    int g = 0, o = 0;
    for (int j = 0; j < m->n_slots; j++) { g += (m->h_flags[j] & LP_BAD) ? 0 : 1; o += (m->h_flags[j] & LP_OBS) ? 1 : 0; }
    if (n_slots) *n_slots = m->n_slots;
    if (n_good) *n_good = g;
    if (n_observed) *n_observed = o;
    return HVO_OK;
}

int hvo_point_map_slot(const hvo_point_map *m, int slot, float pos[3], float normal[3], float *max_dist, float *min_dist, uint8_t desc[32], int *bad,
                       int *observed)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    const size_t cap = (size_t)m->cap, j = (size_t)slot;
    if (pos) for (int k = 0; k < 3; k++) pos[k] = m->h_pos[k * cap + j];
    if (normal) for (int k = 0; k < 3; k++) normal[k] = m->h_nrm[k * cap + j];
    if (max_dist) *max_dist = m->h_maxd[j];
    if (min_dist) *min_dist = m->h_mind[j];
    if (desc) memcpy(desc, &m->h_desc[j * 32], 32);
    if (bad) *bad = (m->h_flags[j] & LP_BAD) ? 1 : 0;
    if (observed) *observed = (m->h_flags[j] & LP_OBS) ? 1 : 0;
    return HVO_OK;
}

const char *hvo_point_map_last_error(const hvo_point_map *m) { return m ? m->last_error.c_str() : ""; }

}  // extern "C"

// ---------------------------------------------------------------- kernels ----------------------------------------------------------------

struct LpPose { float R[9], t[3], Ow[3], pad; };

struct LpDev {
    int ns, cap, nframes, nblocks, capq, n_levels;
    const float *pos, *nrm, *maxd, *mind; const uint8_t *desc, *flags;
    const LpPose *pose;                              // nframes
    float fx, fy, cx, cy, bf, minX, maxX, minY, maxY, logsf, vclimit;
    const uint8_t *seen;                             // nframes x ns
    uint8_t *pass; float4 *s_proj; int *s_lvl;       // nframes x ns, by slot: (u, v, ur, viewCos), level
    int *blockcnt;                                   // nframes x nblocks
    int *nview, *ntested;                            // nframes
    int *q_slot; float *q_u, *q_v, *q_ur, *q_vc, *q_proj; int *q_lvl; uint8_t *q_desc, *q_blocks;   // frame f's queries at f * capq (q_proj: u, v, ur packed, for the caller)
};

// one row of Rcw * X + tcw: the reading of k_project_last (match.hip's gemm3_row)
static __device__ __forceinline__ float lp_row(const float *a, float b0, float b1, float b2, float c)
{
    float t = __fmul_rn(a[0], b0); t = __fadd_rn(t, __fmul_rn(a[1], b1)); t = __fadd_rn(t, __fmul_rn(a[2], b2));
    return (float)((double)t * 1.0 + (double)c * 1.0);
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_mark(int nt, int ns, const uint8_t *__restrict__ flags, int32_t *__restrict__ held, uint8_t *__restrict__ t_occ,
                                                        const int32_t *__restrict__ extra, int n_extra, uint8_t *__restrict__ seen)
{
    const int i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i < nt) {
        int h = held[i];
        if (h >= ns) h = -1;                                       // (refused on the host before the launch)
        if (h >= 0 && (flags[h] & LP_BAD)) h = -1;                 // Tracking.cc:3235-3238
        held[i] = h;
        t_occ[i] = ((h >= 0 && (flags[h] & LP_OBS)) || h == HVO_HELD_FOREIGN_OBSERVED) ? 1 : 0;    // ORBmatcher.cc:88-90
        if (h >= 0) seen[h] = 1;                                   // mnLastFrameSeen = mCurrentFrame.mnId (3242)
    } else if (i - nt < n_extra) {
        const int e = extra[i - nt];
        if (e >= 0 && e < ns) seen[e] = 1;
    }
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_frustum(LpDev a)
{
    const int j = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool in = j < a.ns;
    const size_t cap = (size_t)a.cap, jj = in ? (size_t)j : 0;
    const float X = a.pos[jj], Y = a.pos[cap + jj], Z = a.pos[2 * cap + jj];
    const float n0 = a.nrm[jj], n1 = a.nrm[cap + jj], n2 = a.nrm[2 * cap + jj];
    const float mfMax = a.maxd[jj], mfMin = a.mind[jj];
    const bool good = in && !(a.flags[jj] & LP_BAD);
    for (int f = 0; f < a.nframes; f++) {
        const LpPose &P = a.pose[f];
        const size_t o = (size_t)f * a.ns + jj;
        const bool tested = good && !a.seen[o];
        bool pass = false;
        if (tested) {
            const float xc = lp_row(P.R, X, Y, Z, P.t[0]), yc = lp_row(P.R + 3, X, Y, Z, P.t[1]), zc = lp_row(P.R + 6, X, Y, Z, P.t[2]);
            if (!(zc < 0.0f)) {                                    // Frame.cc:1385: z == 0 and -0.0 pass and divide
                const float invz = __fdiv_rn(1.0f, zc);
                const float u = __fadd_rn(__fmul_rn(__fmul_rn(a.fx, xc), invz), a.cx), v = __fadd_rn(__fmul_rn(__fmul_rn(a.fy, yc), invz), a.cy);
                const bool out = (u < a.minX || u > a.maxX) || (v < a.minY || v > a.maxY);       // (a NaN compares false four times)
                if (!out) {
                    const float maxD = __fmul_rn(1.2f, mfMax), minD = __fmul_rn(0.8f, mfMin);
                    const double d0 = __fsub_rn(X, P.Ow[0]), d1 = __fsub_rn(Y, P.Ow[1]), d2 = __fsub_rn(Z, P.Ow[2]);
                    const float dist = (float)sqrt((d0 * d0 + d1 * d1) + d2 * d2);
                    if (!(dist < minD || dist > maxD)) {
                        const double dot = (d0 * (double)n0 + d1 * (double)n1) + d2 * (double)n2;
                        const float vc = (float)(dot / (double)dist);
                        if (!(vc < a.vclimit)) {
                            const float ratio = __fdiv_rn(mfMax, dist);
                            const float lv = ceilf(__fdiv_rn(logf(ratio), a.logsf));
                            int l = lv != lv ? 0 : lv >= 2147483648.0f ? 2147483647 : lv <= -2147483648.0f ? (-2147483647 - 1) : (int)lv;
                            if (l < 0) l = 0; else if (l >= a.n_levels) l = a.n_levels - 1;      // MapPoint.cc:409-412
                            pass = true;
                            a.s_proj[o] = make_float4(u, v, __fsub_rn(u, __fmul_rn(a.bf, invz)), vc);
                            a.s_lvl[o] = l;
                        }
                    }
                }
            }
        }
        if (in) a.pass[o] = pass ? 1 : 0;
        const int np = __syncthreads_count(pass), nt = __syncthreads_count(tested);
        if (threadIdx.x == 0) { a.blockcnt[(size_t)f * a.nblocks + blockIdx.x] = np; if (nt) atomicAdd(&a.ntested[f], nt); }
    }
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_compact(LpDev a)
{
    __shared__ int red[LP_BLOCK / 64], wcnt[LP_BLOCK / 64];
    const int f = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // survivors of the blocks before this one (an integer sum: any order)
    int s = 0;
    for (int k = tid; k < b; k += LP_BLOCK) s += a.blockcnt[(size_t)f * a.nblocks + k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const int j = b * LP_BLOCK + tid;
    const size_t src = (size_t)f * a.ns + (j < a.ns ? j : 0);
    const bool p = j < a.ns && a.pass[src];
    const unsigned long long bm = __ballot(p);
    if (lane == 0) { red[wave] = s; wcnt[wave] = __popcll(bm); }
    __syncthreads();
    int off = 0, before = 0, total = 0;
    for (int w = 0; w < LP_BLOCK / 64; w++) { off += red[w]; before += w < wave ? wcnt[w] : 0; total += wcnt[w]; }
    if (b == a.nblocks - 1 && tid == 0) a.nview[f] = off + total;
    const int q = off + before + __popcll(bm & ((1ull << lane) - 1ull));
    if (p && q < a.capq) {
        const size_t d = (size_t)f * a.capq + q;
        const float4 pr = a.s_proj[src];
        a.q_slot[d] = j;
        a.q_u[d] = pr.x; a.q_v[d] = pr.y; a.q_ur[d] = pr.z; a.q_vc[d] = pr.w; a.q_lvl[d] = a.s_lvl[src];
        a.q_proj[3 * d] = pr.x; a.q_proj[3 * d + 1] = pr.y; a.q_proj[3 * d + 2] = pr.z;
        *(ulonglong4 *)(a.q_desc + 32 * d) = *(const ulonglong4 *)(a.desc + 32 * (size_t)j);
        a.q_blocks[d] = (a.flags[j] & LP_OBS) ? 1 : 0;
    }
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_fill(int n, int32_t *__restrict__ idx, int32_t *__restrict__ dist)
{
    const int i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i < n) { idx[i] = -1; dist[i] = 256; }
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_assign(int nq, int nt, const int32_t *__restrict__ match_idx, int *__restrict__ win)
{
    const int q = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (q >= nq) return;
    const int j = match_idx[q];
    if (j >= 0 && j < nt) atomicMax(&win[j], q);
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_apply(int nt, int nq, const int *__restrict__ win, const int *__restrict__ q_slot, int32_t *__restrict__ held)
{
    const int i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= nt) return;
    const int w = win[i];
    if (w >= 0 && w < nq) held[i] = q_slot[w];                     // F.mvpMapPoints[bestIdx] = pMP, the last one in query order
}

// ---------------------------------------------------------------- the call ----------------------------------------------------------------

static int lp_grow(hvo_point_map *m, hipStream_t st, char **p, size_t *have, size_t want)
{
    if (*have >= want) return HVO_OK;
    PM_HIP(hipStreamSynchronize(st));
    if (*p) (void)hipFree(*p);
    *p = nullptr; *have = 0;
    size_t c = 1 << 20;
    while (c < want) c *= 2;
    PM_HIP(hipMalloc((void **)p, c));
    *have = c;
    return HVO_OK;
}

int lp_map_device(const hvo_point_map *m) { return m->device; }
const char *lp_map_error(const hvo_point_map *m) { return m->last_error.c_str(); }

static std::string lp_limit_text(int nq, int nt)
{
    return "local points: " + std::to_string(nq) + " points in view, " + std::to_string(nt) + " frame features (limits: " + std::to_string(LP_MAXQ) + ", " +
           std::to_string(LP_MAXT) + "); nothing was written";
}

int lp_run(hipStream_t st, hvo_point_map *m, const hvo_camera *cam, const hvo_local_points_params *P, const float bounds[4], const float *sf, int nframes,
           const LpFrameDev *fr, const float *Tcw, hvo_local_points_io *io, hvo_local_points_result *res)
{
    const int ns = m->n_slots, nblocks = std::max(1, (ns + LP_BLOCK - 1) / LP_BLOCK), capq = std::max(1, std::min(ns, LP_MAXQ));
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { m->last_error = "local points: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) { m->last_error = "local points: empty image bounds"; return HVO_ERR_INVALID_ARG; }
    for (int f = 0; f < nframes; f++) {
        memset(&res[f], 0, sizeof(res[f]));
        if (fr[f].nt > LP_MAXT) { m->last_error = lp_limit_text(0, fr[f].nt); res[f].status = HVO_ERR_UNSUPPORTED; return HVO_ERR_UNSUPPORTED; }
        if (fr[f].nt > io[f].n_kp) { m->last_error = "local points: held is shorter than the frame's key-point count"; return HVO_ERR_INVALID_ARG; }
        if ((fr[f].nt > 0 && !io[f].held) || !io[f].in_view_slot || io[f].n_seen_extra < 0 || (io[f].n_seen_extra > 0 && !io[f].seen_extra)) {
            m->last_error = "local points: held or in_view_slot missing"; return HVO_ERR_INVALID_ARG;
        }
        for (int i = 0; i < fr[f].nt; i++)
            if (io[f].held[i] >= ns || io[f].held[i] < HVO_HELD_FOREIGN_UNOBSERVED) { m->last_error = "local points: held names a slot beyond the map or an unknown value"; return HVO_ERR_INVALID_ARG; }
        for (int i = 0; i < io[f].n_seen_extra; i++) if (io[f].seen_extra[i] < 0 || io[f].seen_extra[i] >= ns) { m->last_error = "local points: seen_extra names a slot beyond the map"; return HVO_ERR_INVALID_ARG; }
    }
    // ---- scratch A: everything whose size is known before the in-view counts ----
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += lp_al(bytes); return at; };
    const size_t F = (size_t)nframes, NS = (size_t)std::max(ns, 1);
    const size_t o_pose = take(F * sizeof(LpPose)), o_seen = take(F * NS), o_pass = take(F * NS), o_sp = take(F * NS * 16), o_slv = take(F * NS * 4);
    const size_t o_bc = take(F * nblocks * 4), o_cnt = take(F * 2 * 4);
    const size_t o_qs = take(F * capq * 4), o_qu = take(F * capq * 4), o_qv = take(F * capq * 4), o_qr = take(F * capq * 4), o_qc = take(F * capq * 4),
                 o_ql = take(F * capq * 4), o_qd = take(F * capq * 32), o_qb = take(F * capq), o_qp = take(F * capq * 12);
    const size_t o_rad = take(F * capq * 4), o_min = take(F * capq * 4), o_max = take(F * capq * 4);
    const size_t o_mi = take(F * capq * 4), o_md = take(F * capq * 4);
    std::vector<size_t> o_held(F), o_occ(F), o_ex(F), o_win(F), o_k(F), o_ur(F);
    for (int f = 0; f < nframes; f++) {
        const size_t nt = (size_t)std::max(fr[f].nt, 1);
        o_held[f] = take(nt * 4); o_occ[f] = take(nt); o_ex[f] = take((size_t)std::max(io[f].n_seen_extra, 1) * 4); o_win[f] = take(nt * 4);
        o_k[f] = take(4);                                          // n_matches
        o_ur[f] = fr[f].depth ? take(2 * nt * 4) : 0;              // mvuRight, mvDepth formed from the depth image
    }
    int rc;
    if ((rc = lp_grow(m, st, &m->d_a, &m->a_bytes, o))) return rc;
    char *A = m->d_a;
    std::vector<LpPose> pose(F);
    for (int f = 0; f < nframes; f++) {
        const float *T = Tcw + 12 * (size_t)f; LpPose &p = pose[f];
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) p.R[3 * r + c] = T[4 * r + c]; p.t[r] = T[4 * r + 3]; }
        for (int r = 0; r < 3; r++) {                              // mOw = -Rcw^T tcw
            double s0 = 0;
            for (int k = 0; k < 3; k++) s0 += (double)p.R[3 * k + r] * (double)p.t[k];
            p.Ow[r] = (float)(s0 * -1.0);
        }
        p.pad = 0.f;
    }
    PM_HIP(hipMemcpyAsync(A + o_pose, pose.data(), F * sizeof(LpPose), hipMemcpyHostToDevice, st));
    PM_HIP(hipMemsetAsync(A + o_seen, 0, F * NS, st));
    PM_HIP(hipMemsetAsync(A + o_cnt, 0, F * 8, st));
    for (int f = 0; f < nframes; f++) {
        const int nt = fr[f].nt, ne = io[f].n_seen_extra;
        if (nt) PM_HIP(hipMemcpyAsync(A + o_held[f], io[f].held, (size_t)nt * 4, hipMemcpyHostToDevice, st));
        if (ne) PM_HIP(hipMemcpyAsync(A + o_ex[f], io[f].seen_extra, (size_t)ne * 4, hipMemcpyHostToDevice, st));
        PM_HIP(hipMemsetAsync(A + o_win[f], 0xFF, (size_t)std::max(nt, 1) * 4, st));
        PM_HIP(hipMemsetAsync(A + o_k[f], 0, 4, st));
    }
    LpDev a; memset(&a, 0, sizeof(a));
    a.ns = ns; a.cap = m->cap; a.nframes = nframes; a.nblocks = nblocks; a.capq = capq; a.n_levels = P->n_levels;
    a.pos = m->d_pos; a.nrm = m->d_nrm; a.maxd = m->d_maxd; a.mind = m->d_mind; a.desc = m->d_desc; a.flags = m->d_flags;
    a.pose = (const LpPose *)(A + o_pose);
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.bf = P->bf; a.minX = bounds[0]; a.maxX = bounds[1]; a.minY = bounds[2]; a.maxY = bounds[3];
    a.logsf = P->log_scale_factor; a.vclimit = P->view_cos_limit;
    a.seen = (const uint8_t *)(A + o_seen); a.pass = (uint8_t *)(A + o_pass); a.s_proj = (float4 *)(A + o_sp); a.s_lvl = (int *)(A + o_slv);
    a.blockcnt = (int *)(A + o_bc); a.nview = (int *)(A + o_cnt); a.ntested = a.nview + nframes;
    a.q_slot = (int *)(A + o_qs); a.q_u = (float *)(A + o_qu); a.q_v = (float *)(A + o_qv); a.q_ur = (float *)(A + o_qr); a.q_vc = (float *)(A + o_qc);
    a.q_lvl = (int *)(A + o_ql); a.q_proj = (float *)(A + o_qp); a.q_desc = (uint8_t *)(A + o_qd); a.q_blocks = (uint8_t *)(A + o_qb);
    PM_HIP(hipEventRecord(m->ev[0], st));
    for (int f = 0; f < nframes; f++) {
        const int n = fr[f].nt + io[f].n_seen_extra;
        if (n > 0 && ns > 0)
            hipLaunchKernelGGL(k_lp_mark, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, fr[f].nt, ns, m->d_flags, (int32_t *)(A + o_held[f]),
                               (uint8_t *)(A + o_occ[f]), (const int32_t *)(A + o_ex[f]), io[f].n_seen_extra, (uint8_t *)(A + o_seen) + (size_t)f * ns);
        else if (fr[f].nt > 0)
            PM_HIP(hipMemsetAsync(A + o_occ[f], 0, (size_t)fr[f].nt, st));
    }
    if (ns > 0) {
        hipLaunchKernelGGL(k_lp_frustum, dim3(nblocks), dim3(LP_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_lp_compact, dim3(nblocks, nframes), dim3(LP_BLOCK), 0, st, a);
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "local points: frustum launch"; return HVO_ERR_HIP; }
    PM_HIP(hipEventRecord(m->ev[1], st));
    std::vector<int> cnt(2 * F, 0);
    PM_HIP(hipMemcpyAsync(cnt.data(), A + o_cnt, F * 8, hipMemcpyDeviceToHost, st));
    PM_HIP(hipStreamSynchronize(st));
    size_t sb = 0;
    for (int f = 0; f < nframes; f++) {
        res[f].n_slots_tested = cnt[nframes + f]; res[f].n_in_view = cnt[f];
        if (cnt[f] > LP_MAXQ) {                                    // refused whole: nothing of the caller's is written
            res[f].status = HVO_ERR_UNSUPPORTED; m->last_error = lp_limit_text(cnt[f], fr[f].nt); return HVO_ERR_UNSUPPORTED;
        }
        if (cnt[f] > 0 && fr[f].nt > 0) sb = std::max(sb, match_sbp_scratch_bytes(cnt[f]));
    }
    // ---- scratch B: the search's key rows (the frames' searches run one after the other on the stream and share them) ----
    if ((rc = lp_grow(m, st, &m->d_b, &m->b_bytes, lp_al(sb) + 256))) return rc;
    ProjDev W; memset(&W, 0, sizeof(W));
    for (int l = 0; l < HVO_MAX_LEVELS; l++) W.sf[l] = sf[l];
    for (int f = 0; f < nframes; f++) {
        const int nq = cnt[f], nt = fr[f].nt;
        const size_t q0 = (size_t)f * capq;
        int32_t *d_mi = (int32_t *)(A + o_mi) + q0, *d_md = (int32_t *)(A + o_md) + q0;
        if (nq > 0 && nt > 0) {                                    // nToMatch > 0 (Tracking.cc:3266)
            const float *d_uright = fr[f].uright;
            if (fr[f].depth) {                                     // Frame::ComputeStereoFromRGBD on the resident key points (mvKeysUn = mvKeys)
                float *ur = (float *)(A + o_ur[f]);
                if ((rc = match_stereo_enqueue(st, fr[f].kp_un, fr[f].kp_un, nullptr, nt, fr[f].depth, fr[f].pitch, fr[f].w, fr[f].h, fr[f].dfac, P->bf, ur, ur + nt))) {
                    m->last_error = "local points: mvuRight launch"; return rc;
                }
                d_uright = ur;
            }
            float *d_rad = (float *)(A + o_rad) + q0; int *d_min = (int *)(A + o_min) + q0, *d_max = (int *)(A + o_max) + q0;
            hipLaunchKernelGGL(k_track_windows, dim3((nq + 255) / 256), dim3(256), 0, st, nq, (const int *)(a.q_lvl + q0), (const float *)(a.q_vc + q0), P->th,
                               P->th != 1.0f ? 1 : 0, W, d_rad, d_min, d_max);
            SbpDev s; memset(&s, 0, sizeof(s));
            s.q_desc = a.q_desc + 32 * q0; s.q_desc_index = nullptr;
            s.q_u = a.q_u + q0; s.q_v = a.q_v + q0; s.q_ur = a.q_ur + q0; s.q_radius = d_rad; s.q_min_level = d_min; s.q_max_level = d_max; s.q_angle = nullptr;
            s.q_blocks = a.q_blocks + q0;
            s.t_kp = fr[f].kp_un; s.t_uright = d_uright; s.t_occ = (const uint8_t *)(A + o_occ[f]); s.t_desc = fr[f].desc;
            s.nq = nq; s.nt = nt; s.mnMinX = bounds[0]; s.mnMaxX = bounds[1]; s.mnMinY = bounds[2]; s.mnMaxY = bounds[3];
            s.th_high = P->th_high; s.check_orientation = 0; s.map_mode = 1; s.nn_ratio = P->nn_ratio;
            s.match_idx = d_mi; s.match_dist = d_md; s.n_matches = (int *)(A + o_k[f]);
            if ((rc = match_sbp_enqueue(st, s, m->d_b))) { m->last_error = rc == HVO_ERR_UNSUPPORTED ? lp_limit_text(nq, nt) : "local points: search launch"; return rc; }
        } else if (nq > 0)
            hipLaunchKernelGGL(k_lp_fill, dim3((nq + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, nq, d_mi, d_md);
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "local points: search launch"; return HVO_ERR_HIP; }
    PM_HIP(hipEventRecord(m->ev[2], st));
    for (int f = 0; f < nframes; f++) {
        const int nq = cnt[f], nt = fr[f].nt;
        if (nt < 1 || nq < 1) continue;
        const size_t q0 = (size_t)f * capq;
        int *d_win = (int *)(A + o_win[f]);
        hipLaunchKernelGGL(k_lp_assign, dim3((nq + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, nq, nt, (const int32_t *)(A + o_mi) + q0, d_win);
        hipLaunchKernelGGL(k_lp_apply, dim3((nt + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, nt, nq, d_win, a.q_slot + q0, (int32_t *)(A + o_held[f]));
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "local points: assignment launch"; return HVO_ERR_HIP; }
    PM_HIP(hipEventRecord(m->ev[3], st));
    std::vector<int> kk(F, 0);
    for (int f = 0; f < nframes; f++) {
        const size_t nq = (size_t)cnt[f], nt = (size_t)fr[f].nt, q0 = (size_t)f * capq;
        hvo_local_points_io &I = io[f];
        PM_HIP(hipMemcpyAsync(&kk[f], A + o_k[f], 4, hipMemcpyDeviceToHost, st));
        if (nt && ns > 0) PM_HIP(hipMemcpyAsync(I.held, A + o_held[f], nt * 4, hipMemcpyDeviceToHost, st));
        if (nq) {
            PM_HIP(hipMemcpyAsync(I.in_view_slot, a.q_slot + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.proj) PM_HIP(hipMemcpyAsync(I.proj, a.q_proj + 3 * q0, nq * 12, hipMemcpyDeviceToHost, st));
            if (I.view_cos) PM_HIP(hipMemcpyAsync(I.view_cos, a.q_vc + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.level) PM_HIP(hipMemcpyAsync(I.level, a.q_lvl + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.match_idx) PM_HIP(hipMemcpyAsync(I.match_idx, (int32_t *)(A + o_mi) + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.match_dist) PM_HIP(hipMemcpyAsync(I.match_dist, (int32_t *)(A + o_md) + q0, nq * 4, hipMemcpyDeviceToHost, st));
        }
    }
    PM_HIP(hipStreamSynchronize(st));
    float ms[3] = { 0.f, 0.f, 0.f };
    for (int k = 0; k < 3; k++) if (hipEventElapsedTime(&ms[k], m->ev[k], m->ev[k + 1]) != hipSuccess) ms[k] = 0.f;
    for (int f = 0; f < nframes; f++) {
        res[f].n_matches = kk[f]; res[f].status = HVO_OK;
        for (int k = 0; k < 3; k++) res[f].kernel_ms[k] = ms[k];
    }
    return HVO_OK;
}
