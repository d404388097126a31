// new_keyframe.hip -- the new map points and map lines of Tracking::CreateNewKeyFrame (reference src/Tracking.cc:3032-3187), of
// Tracking::StereoInitialization (1364-1400) and the temporal points of Tracking::UpdateLastFrame (2194-2246), made from a frame's own arrays
// and written into the resident point map and line map in one call: one launch sequence, one download, one synchronisation.
//
// The selection is a rank by counting: keys (depth, index) are unique, so the place of an entry in the reference's sorted vector is the number
// of candidates with a smaller key, and every counter of the sequential loops has a closed form over those counts (tests/new_keyframe_ref.py
// states the loops as written and tests/test_new_keyframe.py checks the closed forms against them):
//   points    M candidates (depth > 0), c of them with depth <= thDepth.  nPoints counts every processed entry and the break is tested after
//             the increment: the entries of rank <= max(c, 100) are processed.  Everything in front of a processed entry is processed, so the
//             creation rank of a created entry is the number of creatable candidates with a smaller key
//   lines     the counter runs inside `if (bCreateNew)`: over the creatable candidates alone, c' of them with z <= thDepth; those of rank <=
//             max(c', 100) AMONG THE CREATABLE are created, and that rank is the creation rank
//   init      index order and no limit: the same counts with every key 0 (the index decides) and an unbounded limit
// No atomic is used, and two calls on the same bytes return the same bytes.
//   k_nkf_keys     one lane per feature and per key line: the key, the candidate / creatable / level flags, the world direction of every
//                  frame line for the structure pass; a NaN line key raises the call's refusal word (a plain store of 1: every writer stores
//                  the same value) and the later kernels return at once
//   k_nkf_points   one lane per feature; the keys and flags of all features pass through LDS in tiles of 256 and every lane counts its own
//   k_nkf_lines    ranks; a selected lane forms its entry, writes it to the result block and, where a first slot is given, to the map's
//                  component-major device arrays in place (as map_refresh.hip does)
//   k_nkf_struct   Manhattan::computeStructConstrains(Frame &, MapLine *, ..) (src/Manhattan.cpp:66-105) of every new line: one work group
//                  row per entry, one lane per frame line
// The handle owns its workspace (a device block, a pinned block, two events), grow-only, like hvo_local_ba; nothing of a context's arena
// is used.
//
// Readings (tests/new_keyframe_ref.py is the definition).  Only + - * / sqrt in the written order, nothing contracted.
//   UnprojectStereo     x = (u - cx) * z * invfx in float, left to right, invfx = 1.0f / fx; mRwc * x3Dc + mOw by the row reading of sm_row
//                       (slot_map.hpp); mRwc = Rcw^T, mOw = -Rcw^T tcw as match_project_setup forms twc (double sums, times -1.0, to float)
//   point normal        key frame / init: UpdateNormalAndDepth with the key frame as sole observer: 0 + (float)(d * (1 / |d|)), then times
//                       1.0 / 1: a -0.0 component becomes +0.0.  Temporal: the Frame constructor's (src/MapPoint.cc:45-69): d / |d| as
//                       Mat / scalar, no sum: -0.0 stays.  The distance range is the same text in both
//   PtToWorldCoord      Rwc and Ow widened to double; ((r0 p0 + r1 p1) + r2 p2) + Ow per row
//   line geometry       line_geometry = 1: UpdateAverageDir for the sole observer (Tracking.cc:3171 uncommented): normal = (0 + n / |n|) / 1 in
//                       double, the distance range of map_refresh.hip with the key line's octave.  0: normal 0 and both distances 0, the
//                       members MapLine(Vector6d &, int &, KeyFrame *, Map *) leaves unwritten read as zero: never in view until a refresh
//   line key            z = (float)(sz > ez ? sz : ez); a candidate whose key is NaN refuses the call
//   computeAngle        |dot / (|a| |b|)| in double, sums left to right (tests/line_map_ref.py struct_rel); < cos_perp: 2, else > cos_par: 1
#include "hvo_internal.hpp"
#include "slot_map.hpp"
#include "frame_view.hpp"
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>

#define NKF_BLOCK 256
#define NKF_CAND  1          // flag bits of a feature
#define NKF_CREAT 2
#define NKF_LEVEL 4
#define NKF_STRUCT 8         // lines: mvLines3D[i].first[0] != 0.0, the gate of computeStructConstrains

struct NkfSide {             // one of the two feature kinds: where its keys, its results and its map live
    int n, first, cap, ns;   // features; first slot (-1: none); the map's component stride and slot count
    const int32_t *held; const uint8_t *flags;           // uploaded held; the map's flag bytes (null: no map)
    float *key; uint8_t *fl;                             // scratch
    int32_t *o_held, *o_index, *o_slot; uint8_t *o_status, *o_desc; void *o_pos, *o_nrm; double *o_wvec; float *o_maxd, *o_mind;      // the result block
    void *m_pos, *m_nrm; double *m_wvec; float *m_maxd, *m_mind; uint8_t *m_desc, *m_flags;                                  // the map's arrays
};

struct NkfDev {
    int mode, n_levels, ln_levels, line_geometry;
    float th, cx, cy, invfx, invfy;
    float Rwc[9], Ow[3], sf[HVO_MAX_LEVELS], lsf[HVO_MAX_LEVELS];
    double cos_par, cos_perp;
    const hvo_keypoint *kp_un; const float *depth; const uint8_t *desc; const hvo_keyline *kl; const uint8_t *ldesc; const hvo_line3d *l3d;
    int32_t *hdr;            // [0] the refusal word (1: a NaN line key), [1] point candidates, [2] line candidates
    double *ldir;            // scratch: n_kl x 3, end - start of every frame line in the world
    uint8_t *rel;            // result: entries x n_kl
    NkfSide p, l;
};

static __device__ __forceinline__ bool nkf_creatable(int mode, int h, const uint8_t *flags)
{
    if (mode == HVO_KFI_INIT) return true;
    if (h >= 0) return !(flags[h] & SM_OBS);
    return h == -1 || h == HVO_HELD_FOREIGN_UNOBSERVED;
}

static __device__ __forceinline__ void nkf_to_world(const NkfDev &a, const double *P, double *W)
{
#pragma unroll
    for (int r = 0; r < 3; r++) W[r] = (((double)a.Rwc[3 * r] * P[0] + (double)a.Rwc[3 * r + 1] * P[1]) + (double)a.Rwc[3 * r + 2] * P[2]) + (double)a.Ow[r];
}

static __device__ __forceinline__ double nkf_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

__global__ __launch_bounds__(NKF_BLOCK) void k_nkf_keys(NkfDev a)
{
    const int i = blockIdx.x * NKF_BLOCK + threadIdx.x;
    if (i < a.p.n) {
        const float z = a.depth[i];
        const int h = a.p.held[i], lvl = a.kp_un[i].octave;
        int f = z > 0 ? NKF_CAND : 0;
        if (nkf_creatable(a.mode, h, a.p.flags)) f |= NKF_CREAT;
        if (lvl >= 0 && lvl < a.n_levels) f |= NKF_LEVEL;
        a.p.key[i] = a.mode == HVO_KFI_INIT ? 0.0f : z;
        a.p.fl[i] = (uint8_t)f;
        a.p.o_held[i] = a.mode == HVO_KFI_INIT ? -1 : h;
    }
    if (i < a.l.n) {
        const hvo_line3d &L = a.l3d[i];
        const int h = a.l.held[i], lvl = a.kl[i].octave;
        int f = 0; float z = 0.0f;
        if (a.mode == HVO_KFI_INIT) { if (a.kl[i].sx > 0.0 && L.A[0] != 0) f |= NKF_CAND; }
        else {
            if (!(L.A[2] == 0 || L.B[2] == 0)) f |= NKF_CAND;
            const double sz = L.A[2], ez = L.B[2];
            z = (float)(sz > ez ? sz : ez);
            if ((f & NKF_CAND) && z != z) a.hdr[0] = 1;
        }
        if (nkf_creatable(a.mode, h, a.l.flags)) f |= NKF_CREAT;
        if (!a.line_geometry || (lvl >= 0 && lvl < a.ln_levels)) f |= NKF_LEVEL;
        if (L.A[0] != 0.0) {
            f |= NKF_STRUCT;
            double S[3], E[3];
            nkf_to_world(a, L.A, S); nkf_to_world(a, L.B, E);
            a.ldir[3 * (size_t)i] = E[0] - S[0]; a.ldir[3 * (size_t)i + 1] = E[1] - S[1]; a.ldir[3 * (size_t)i + 2] = E[2] - S[2];
        }
        a.l.key[i] = z;
        a.l.fl[i] = (uint8_t)f;
        a.l.o_held[i] = a.mode == HVO_KFI_INIT ? -1 : h;
    }
}

// The counts of lane i over all n features (tiles of NKF_BLOCK through LDS): is it selected, its place e among the entries and its creation
// rank k (the entries in front of it whose level is inside the table).  *total: the candidates.
template <bool LINE> static __device__ __forceinline__ bool nkf_select(const NkfDev &a, const NkfSide &s, int i, int *e_out, int *k_out, int *total)
{
    __shared__ float t_key[NKF_BLOCK];
    __shared__ uint8_t t_fl[NKF_BLOCK];
    const bool in = i < s.n;
    const float zi = in ? s.key[i] : 0.0f;
    const int fi = in ? s.fl[i] : 0;
    int rank = 0, crank = 0, krank = 0, c = 0, M = 0;
    for (int j0 = 0; j0 < s.n; j0 += NKF_BLOCK) {
        const int j = j0 + (int)threadIdx.x;
        __syncthreads();
        t_key[threadIdx.x] = j < s.n ? s.key[j] : 0.0f;
        t_fl[threadIdx.x] = j < s.n ? s.fl[j] : 0;
        __syncthreads();
        const int m = min(NKF_BLOCK, s.n - j0);
        for (int q = 0; q < m; q++) {
            const float zj = t_key[q]; const int fj = t_fl[q];
            const bool cand = fj & NKF_CAND, creat = cand && (fj & NKF_CREAT);
            const bool lt = cand && (zj < zi || (zj == zi && j0 + q < i));          // pair<float, int>'s operator<
            const bool counted = LINE ? creat : cand;
            M += cand ? 1 : 0;
            c += (counted && zj <= a.th) ? 1 : 0;
            rank += lt ? 1 : 0;
            crank += (lt && creat) ? 1 : 0;
            krank += (lt && creat && (fj & NKF_LEVEL)) ? 1 : 0;
        }
    }
    *total = M; *e_out = crank; *k_out = krank;
    const int limit = a.mode == HVO_KFI_INIT ? INT_MAX : max(c, 100);
    return (fi & NKF_CAND) && (fi & NKF_CREAT) && (LINE ? crank : rank) <= limit;
}

__global__ __launch_bounds__(NKF_BLOCK) void k_nkf_points(NkfDev a)
{
    const NkfSide &s = a.p;
    const int i = blockIdx.x * NKF_BLOCK + threadIdx.x;
    int e, k, M;
    if (a.hdr[0] == 1) return;                                   // (uniform: written by the launch before)
    const bool sel = nkf_select<false>(a, s, i, &e, &k, &M);
    if (i == 0) a.hdr[1] = M;
    if (!sel) return;
    const bool temporal = a.mode == HVO_KFI_TEMPORAL;
    s.o_index[e] = i;
    if (!(s.fl[i] & NKF_LEVEL)) {
        s.o_status[e] = HVO_KFI_BAD_LEVEL; s.o_slot[e] = -1;
        if (!temporal) s.o_held[i] = -1;                         // Tracking.cc:3077: cleared before the constructor would run
        return;
    }
    const hvo_keypoint kp = a.kp_un[i];
    const float z = a.depth[i];
    const float x = (kp.x - a.cx) * z * a.invfx, y = (kp.y - a.cy) * z * a.invfy;
    float P[3], d[3], nrm[3];
#pragma unroll
    for (int r = 0; r < 3; r++) { P[r] = sm_row(a.Rwc + 3 * r, x, y, z, a.Ow[r]); d[r] = P[r] - a.Ow[r]; }
    const double nn = nkf_norm3(d[0], d[1], d[2]), inv = 1.0 / nn;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float u = (float)((double)d[r] * inv);
        nrm[r] = temporal ? u : (float)((double)(0.0f + u) * (1.0 / 1.0));
    }
    const float dist = (float)nn, mx = dist * a.sf[kp.octave], mi = mx / a.sf[a.n_levels - 1];
    const int slot = (s.first >= 0 && !temporal) ? s.first + k : -1;
    s.o_status[e] = HVO_KFI_CREATED; s.o_slot[e] = slot;
    float *op = (float *)s.o_pos + 3 * (size_t)e, *on = (float *)s.o_nrm + 3 * (size_t)e;
#pragma unroll
    for (int r = 0; r < 3; r++) { op[r] = P[r]; on[r] = nrm[r]; }
    s.o_maxd[e] = mx; s.o_mind[e] = mi;
    const ulonglong4 dsc = *(const ulonglong4 *)(a.desc + 32 * (size_t)i);
    *(ulonglong4 *)(s.o_desc + 32 * (size_t)e) = dsc;
    s.o_held[i] = slot >= 0 ? slot : (temporal ? HVO_HELD_FOREIGN_UNOBSERVED : HVO_HELD_FOREIGN_OBSERVED);
    if (slot >= 0) {
        const size_t cap = (size_t)s.cap;
        float *mp = (float *)s.m_pos, *mn = (float *)s.m_nrm;
#pragma unroll
        for (int r = 0; r < 3; r++) { mp[r * cap + slot] = P[r]; mn[r * cap + slot] = nrm[r]; }
        s.m_maxd[slot] = mx; s.m_mind[slot] = mi;
        *(ulonglong4 *)(s.m_desc + 32 * (size_t)slot) = dsc;
        s.m_flags[slot] = SM_OBS;
    }
}

__global__ __launch_bounds__(NKF_BLOCK) void k_nkf_lines(NkfDev a)
{
    const NkfSide &s = a.l;
    const int i = blockIdx.x * NKF_BLOCK + threadIdx.x;
    int e, k, M;
    if (a.hdr[0] == 1) return;
    const bool sel = nkf_select<true>(a, s, i, &e, &k, &M);
    if (i == 0) a.hdr[2] = M;
    if (!sel) return;
    s.o_index[e] = i;
    if (!(s.fl[i] & NKF_LEVEL)) { s.o_status[e] = HVO_KFI_BAD_LEVEL; s.o_slot[e] = -1; s.o_held[i] = -1; return; }
    const hvo_line3d &L = a.l3d[i];
    double P[6], w[3], nrm[3] = { 0.0, 0.0, 0.0 };
    nkf_to_world(a, L.A, P); nkf_to_world(a, L.B, P + 3);
#pragma unroll
    for (int r = 0; r < 3; r++) w[r] = P[r] - P[3 + r];
    const double zz = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    if (zz > 0.0) { const double rt = sqrt(zz); w[0] = w[0] / rt; w[1] = w[1] / rt; w[2] = w[2] / rt; }
    float mx = 0.0f, mi = 0.0f;
    if (a.line_geometry) {
        double dd[3]; float cm[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            dd[r] = 0.5 * (P[r] + P[3 + r]) - (double)a.Ow[r];
            const float sp = (float)P[r], ep = (float)P[3 + r];
            cm[r] = (float)((double)sp * 0.5 + (double)ep * 0.5) - a.Ow[r];
        }
        const double nn = sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);
#pragma unroll
        for (int r = 0; r < 3; r++) nrm[r] = (0.0 + dd[r] / nn) / 1.0;
        const float dist = (float)nkf_norm3(cm[0], cm[1], cm[2]);
        mx = dist * a.lsf[a.kl[i].octave]; mi = mx / a.lsf[a.ln_levels - 1];
    }
    const int slot = s.first >= 0 ? s.first + k : -1;
    s.o_status[e] = HVO_KFI_CREATED; s.o_slot[e] = slot;
    double *op = (double *)s.o_pos + 6 * (size_t)e, *on = (double *)s.o_nrm + 3 * (size_t)e, *ow = s.o_wvec + 3 * (size_t)e;
#pragma unroll
    for (int r = 0; r < 6; r++) op[r] = P[r];
#pragma unroll
    for (int r = 0; r < 3; r++) { on[r] = nrm[r]; ow[r] = w[r]; }
    s.o_maxd[e] = mx; s.o_mind[e] = mi;
    const ulonglong4 dsc = *(const ulonglong4 *)(a.ldesc + 32 * (size_t)i);
    *(ulonglong4 *)(s.o_desc + 32 * (size_t)e) = dsc;
    s.o_held[i] = slot >= 0 ? slot : HVO_HELD_FOREIGN_OBSERVED;
    if (slot >= 0) {
        const size_t cap = (size_t)s.cap;
        double *mp = (double *)s.m_pos, *mn = (double *)s.m_nrm;
#pragma unroll
        for (int r = 0; r < 6; r++) mp[r * cap + slot] = P[r];
#pragma unroll
        for (int r = 0; r < 3; r++) { mn[r * cap + slot] = nrm[r]; s.m_wvec[r * cap + slot] = w[r]; }
        s.m_maxd[slot] = mx; s.m_mind[slot] = mi;
        *(ulonglong4 *)(s.m_desc + 32 * (size_t)slot) = dsc;
        s.m_flags[slot] = SM_OBS;
    }
}

// grid (ceil(n_kl / NKF_BLOCK), n_kl): row e exists when entry e does (a row past the entries returns whole)
__global__ __launch_bounds__(NKF_BLOCK) void k_nkf_struct(NkfDev a)
{
    const int e = blockIdx.y, i = blockIdx.x * NKF_BLOCK + threadIdx.x;
    if (a.hdr[0] == 1 || a.l.o_index[e] < 0 || i >= a.l.n) return;
    uint8_t rel = 0;
    if (a.l.o_status[e] == HVO_KFI_CREATED && (a.l.fl[i] & NKF_STRUCT)) {
        const double *P = (const double *)a.l.o_pos + 6 * (size_t)e, *le = a.ldir + 3 * (size_t)i;
        const double m0 = P[3] - P[0], m1 = P[4] - P[1], m2 = P[5] - P[2];
        const double dot = (le[0] * m0 + le[1] * m1) + le[2] * m2;
        const double ma = sqrt((le[0] * le[0] + le[1] * le[1]) + le[2] * le[2]), mb = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
        const double ang = fabs(dot / (ma * mb));
        rel = ang < a.cos_perp ? 2 : (ang > a.cos_par ? 1 : 0);
    }
    a.rel[(size_t)e * a.l.n + i] = rel;
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------
struct hvo_kf_insert {
    int device = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    char *d_ws = nullptr, *h_pin = nullptr; size_t ws_cap = 0, pin_cap = 0;
    std::string last_error;
};

static int kf_fail(hvo_kf_insert *K, int rc, const std::string &why) { K->last_error = "create key-frame features: " + why; return rc; }
#define KF_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return kf_fail(K, HVO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// grow-only; the call's stream is drained before a block that a pending copy may still read is freed
static int kf_reserve(hvo_kf_insert *K, hipStream_t st, char **p, size_t *cap, size_t bytes, bool pinned)
{
    if (*cap >= bytes) return HVO_OK;
    const size_t want = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095;
    if (*p) { KF_HIP(hipStreamSynchronize(st)); if (pinned) KF_HIP(hipHostFree(*p)); else KF_HIP(hipFree(*p)); *p = nullptr; *cap = 0; }
    if (pinned) KF_HIP(hipHostMalloc((void **)p, want, hipHostMallocDefault)); else KF_HIP(hipMalloc((void **)p, want));
    *cap = want;
    return HVO_OK;
}

struct KfCarve { size_t off = 0; size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; } };

struct KfSideLayout { size_t held, key, fl, o_held, o_index, o_slot, o_status, o_desc, o_pos, o_nrm, o_wvec, o_maxd, o_mind; };

static int kf_check_held(hvo_kf_insert *K, const char *what, const int32_t *held, int n, const hvo_slot_map *m)
{
    const int ns = m ? m->n_slots : 0;
    for (int i = 0; i < n; i++)
        if (held[i] < HVO_HELD_FOREIGN_UNOBSERVED || held[i] >= ns) return kf_fail(K, HVO_ERR_INVALID_ARG, std::string(what) + " names a slot beyond the map or an unknown value");
    return HVO_OK;
}

// room for `bound` slots behind `first`, before the launch: the kernels write the device arrays in place
static int kf_make_room(hvo_kf_insert *K, hvo_slot_map *m, int first, int bound)
{
    if (!m || first < 0 || bound < 1) return HVO_OK;
    bool regrown = false;
    int rc = sm_set_begin(m, first, bound, true, &regrown);
    if (rc == HVO_OK && regrown) rc = sm_set_end(m, m->n_slots, 0, true);      // fresh device arrays: every slot in use goes up again, n_slots stays
    if (rc) return kf_fail(K, rc, m->last_error);
    return HVO_OK;
}

static void kf_side_map(NkfSide &s, hvo_slot_map *m, int col_pos, int col_nrm, int col_wvec, int col_maxd, int col_mind, int col_desc)
{
    if (!m) return;
    s.cap = m->cap; s.ns = m->n_slots; s.flags = m->d_flags();
    s.m_pos = m->arr[col_pos].d; s.m_nrm = m->arr[col_nrm].d; s.m_wvec = col_wvec >= 0 ? (double *)m->arr[col_wvec].d : nullptr;
    s.m_maxd = (float *)m->arr[col_maxd].d; s.m_mind = (float *)m->arr[col_mind].d; s.m_desc = (uint8_t *)m->arr[col_desc].d; s.m_flags = m->d_flags();
}

struct KfOut { int32_t *held, *index, *slot; uint8_t *status; void *pos, *nrm; double *wvec; float *maxd, *mind; };
struct KfCols { int pos, nrm, wvec, maxd, mind, desc; };

// One side of the block that came down (h: the pinned block): the dense prefix of entries goes to the caller's arrays, and what the kernel
// wrote into the map's device arrays goes into the map's mirror from the same values; held comes back whole
template <class real> static void kf_finish(const char *h, const KfSideLayout &y, int n, int npos, int first, hvo_slot_map *m, const KfCols &col, const KfOut &o,
                                            int32_t *n_entries, int32_t *n_created)
{
    const int32_t *idx = (const int32_t *)(h + y.o_index), *slot = (const int32_t *)(h + y.o_slot); const uint8_t *stt = (const uint8_t *)(h + y.o_status);
    const real *pos = (const real *)(h + y.o_pos), *nrm = (const real *)(h + y.o_nrm); const double *wv = (const double *)(h + y.o_wvec);
    const float *mx = (const float *)(h + y.o_maxd), *mi = (const float *)(h + y.o_mind); const uint8_t *ds = (const uint8_t *)(h + y.o_desc);
    int ne = 0, nc = 0;
    while (ne < n && idx[ne] >= 0) ne++;
    const size_t cap = m ? (size_t)m->cap : 0, np = (size_t)npos;
    for (int e = 0; e < ne; e++) {
        const size_t E = (size_t)e;
        if (o.index) o.index[e] = idx[e];
        if (o.slot) o.slot[e] = slot[e];
        if (o.status) o.status[e] = stt[e];
        if (stt[e] != HVO_KFI_CREATED) continue;
        nc++;
        if (o.pos) memcpy((real *)o.pos + np * E, pos + np * E, np * sizeof(real));
        if (o.nrm) memcpy((real *)o.nrm + 3 * E, nrm + 3 * E, 3 * sizeof(real));
        if (o.wvec && col.wvec >= 0) memcpy(o.wvec + 3 * E, wv + 3 * E, 24);
        if (o.maxd) o.maxd[e] = mx[e];
        if (o.mind) o.mind[e] = mi[e];
        if (slot[e] < 0 || !m) continue;
        const size_t j = (size_t)slot[e];
        for (size_t c = 0; c < np; c++) m->host<real>(col.pos)[c * cap + j] = pos[np * E + c];
        for (size_t c = 0; c < 3; c++) {
            m->host<real>(col.nrm)[c * cap + j] = nrm[3 * E + c];
            if (col.wvec >= 0) m->host<double>(col.wvec)[c * cap + j] = wv[3 * E + c];
        }
        m->host<float>(col.maxd)[j] = mx[e]; m->host<float>(col.mind)[j] = mi[e];
        memcpy(m->host<uint8_t>(col.desc) + 32 * j, ds + 32 * E, 32);
        m->h_flags()[j] = SM_OBS;
    }
    *n_entries = ne; *n_created = nc;
    if (n > 0) memcpy(o.held, h + y.o_held, (size_t)n * 4);
    if (m && first >= 0 && nc > 0 && first + nc > m->n_slots) m->n_slots = first + nc;
}

// fr: the frame on the device (the resident form) or null: `host` goes up.  sf: mvScaleFactors of the context, orb_levels of them
static int kf_run(hvo_kf_insert *K, hipStream_t st, hvo_point_map *pm, hvo_line_map *lm, const hvo_camera *cam, const float *Tcw, const hvo_kfi_params *P,
                  const FrameView *fr, const hvo_kfi_frame *host, const float *sf, int orb_levels, hvo_kfi_io *io, hvo_kfi_result *res)
{
    memset(res, 0, sizeof(*res));
    const int mode = P->mode;
    const bool temporal = mode == HVO_KFI_TEMPORAL;
    const int n_kp = fr ? fr->n_kp : host->n_kp, n_kl = temporal ? 0 : (fr ? fr->n_kl : host->n_kl);
    res->n_kp = n_kp; res->n_kl = n_kl;
    // ---- refusals: whole, before anything is written ----
    if (mode != HVO_KFI_KEYFRAME && mode != HVO_KFI_INIT && mode != HVO_KFI_TEMPORAL) return kf_fail(K, HVO_ERR_INVALID_ARG, "unknown mode");
    if (n_kp < 0 || n_kl < 0) return kf_fail(K, HVO_ERR_INVALID_ARG, "a negative count");
    if (n_kp > HVO_KFI_MAX_FEATURES || n_kl > HVO_KFI_MAX_LINES)
        return kf_fail(K, HVO_ERR_UNSUPPORTED, std::to_string(n_kp) + " features, " + std::to_string(n_kl) + " key lines (limits: " + std::to_string(HVO_KFI_MAX_FEATURES) + ", " +
                       std::to_string(HVO_KFI_MAX_LINES) + "); nothing was written");
    if (P->n_levels < 1 || P->n_levels > orb_levels || P->n_levels > HVO_MAX_LEVELS) return kf_fail(K, HVO_ERR_INVALID_ARG, "n_levels outside the context's ORB pyramid");
    if (P->line_n_levels < 1 || P->line_n_levels > HVO_MAX_LEVELS) return kf_fail(K, HVO_ERR_INVALID_ARG, "line_n_levels outside 1 .. 16");
    if (P->first_point_slot < -1 || P->first_line_slot < -1) return kf_fail(K, HVO_ERR_INVALID_ARG, "a first slot below -1");
    const int first_p = temporal ? -1 : P->first_point_slot, first_l = temporal ? -1 : P->first_line_slot;
    if ((first_p >= 0 && !pm) || (first_l >= 0 && n_kl > 0 && !lm)) return kf_fail(K, HVO_ERR_INVALID_ARG, "a first slot without its map");
    if ((pm && pm->device != K->device) || (lm && lm->device != K->device)) return kf_fail(K, HVO_ERR_INVALID_ARG, "a map lives on another device");
    if ((pm && first_p > pm->n_slots) || (lm && first_l > lm->n_slots)) return kf_fail(K, HVO_ERR_INVALID_ARG, "a first slot beyond the map's slots");
    if (n_kp > io->n_kp || n_kl > io->n_kl) return kf_fail(K, HVO_ERR_INVALID_ARG, "held is shorter than the frame's count");
    if ((n_kp > 0 && !io->held_points) || (n_kl > 0 && !io->held_lines)) return kf_fail(K, HVO_ERR_INVALID_ARG, "held missing");
    if (!fr && ((n_kp > 0 && (!host->kp_un || !host->depth || !host->desc)) || (n_kl > 0 && (!host->keylines || !host->ldesc || !host->lines3d))))
        return kf_fail(K, HVO_ERR_INVALID_ARG, "a missing frame array");
    int rc;
    if (mode != HVO_KFI_INIT) {
        if ((rc = kf_check_held(K, "held_points", io->held_points, n_kp, pm)) || (rc = kf_check_held(K, "held_lines", io->held_lines, n_kl, lm))) return rc;
    }
    if (n_kp == 0 && n_kl == 0) return HVO_OK;
    if ((rc = kf_make_room(K, pm, first_p, n_kp)) || (rc = kf_make_room(K, lm, first_l, n_kl))) return rc;
    // ---- the workspace: what goes up, the scratch, then what is cleared and comes down ----
    const size_t NP = (size_t)n_kp, NL = (size_t)n_kl;
    KfCarve C; KfSideLayout lp, ll;
    lp.held = C.take(NP * 4); ll.held = C.take(NL * 4);
    size_t u_kp = 0, u_z = 0, u_desc = 0, u_kl = 0, u_ldesc = 0, u_l3d = 0;
    if (!fr) {
        u_kp = C.take(NP * sizeof(hvo_keypoint)); u_z = C.take(NP * 4); u_desc = C.take(NP * 32);
        u_kl = C.take(NL * sizeof(hvo_keyline)); u_ldesc = C.take(NL * 32); u_l3d = C.take(NL * sizeof(hvo_line3d));
    }
    const size_t up_end = C.off;
    lp.key = C.take(NP * 4); lp.fl = C.take(NP); ll.key = C.take(NL * 4); ll.fl = C.take(NL);
    const size_t o_ldir = C.take(NL * 24);
    const size_t r0 = C.off, o_hdr = C.take(16);
    lp.o_held = C.take(NP * 4); lp.o_index = C.take(NP * 4); lp.o_slot = C.take(NP * 4); lp.o_status = C.take(NP); lp.o_pos = C.take(NP * 12); lp.o_nrm = C.take(NP * 12);
    lp.o_maxd = C.take(NP * 4); lp.o_mind = C.take(NP * 4); lp.o_desc = C.take(NP * 32); lp.o_wvec = 0;
    ll.o_held = C.take(NL * 4); ll.o_index = C.take(NL * 4); ll.o_slot = C.take(NL * 4); ll.o_status = C.take(NL); ll.o_pos = C.take(NL * 48); ll.o_nrm = C.take(NL * 24);
    ll.o_wvec = C.take(NL * 24); ll.o_maxd = C.take(NL * 4); ll.o_mind = C.take(NL * 4); ll.o_desc = C.take(NL * 32);
    const bool want_rel = mode == HVO_KFI_KEYFRAME && n_kl > 0;
    const size_t o_rel = C.take(want_rel ? NL * NL : 0), r1 = C.off;
    if ((rc = kf_reserve(K, st, &K->d_ws, &K->ws_cap, r1, false)) || (rc = kf_reserve(K, st, &K->h_pin, &K->pin_cap, r1, true))) return rc;
    char *const d = K->d_ws, *const h = K->h_pin;
    if (n_kp) memcpy(h + lp.held, io->held_points, NP * 4);
    if (n_kl) memcpy(h + ll.held, io->held_lines, NL * 4);
    if (!fr) {
        if (n_kp) { memcpy(h + u_kp, host->kp_un, NP * sizeof(hvo_keypoint)); memcpy(h + u_z, host->depth, NP * 4); memcpy(h + u_desc, host->desc, NP * 32); }
        if (n_kl) { memcpy(h + u_kl, host->keylines, NL * sizeof(hvo_keyline)); memcpy(h + u_ldesc, host->ldesc, NL * 32); memcpy(h + u_l3d, host->lines3d, NL * sizeof(hvo_line3d)); }
    }
    KF_HIP(hipMemcpyAsync(d, h, up_end, hipMemcpyHostToDevice, st));
    KF_HIP(hipMemsetAsync(d + r0, 0xFF, r1 - r0, st));             // index -1, status 255, the refusal word -1
    NkfDev a; memset(&a, 0, sizeof(a));
    a.mode = mode; a.n_levels = P->n_levels; a.ln_levels = P->line_n_levels; a.line_geometry = P->line_geometry ? 1 : 0;
    a.th = P->th_depth; a.cx = cam->cx; a.cy = cam->cy; a.invfx = 1.0f / cam->fx; a.invfy = 1.0f / cam->fy;
    a.cos_par = P->cos_par; a.cos_perp = P->cos_perp;
    {   // mRwc = Rcw^T; mOw = -Rcw^T tcw as match_project_setup forms twc
        const float Rcw[9] = { Tcw[0], Tcw[1], Tcw[2], Tcw[4], Tcw[5], Tcw[6], Tcw[8], Tcw[9], Tcw[10] }, tcw[3] = { Tcw[3], Tcw[7], Tcw[11] };
        for (int r = 0; r < 3; r++) {
            double s0 = 0; for (int q = 0; q < 3; q++) { a.Rwc[3 * r + q] = Rcw[3 * q + r]; s0 += (double)Rcw[3 * q + r] * (double)tcw[q]; }
            a.Ow[r] = (float)(s0 * -1.0);
        }
    }
    float v = 1.0f;
    for (int l = 0; l < HVO_MAX_LEVELS; l++) {
        a.sf[l] = l < P->n_levels ? sf[l] : 1.0f;
        if (l > 0 && l < P->line_n_levels) v = v * P->line_scale_factor;
        a.lsf[l] = l < P->line_n_levels ? v : 1.0f;
    }
    if (fr) { a.kp_un = fr->kp_un; a.depth = fr->zdepth; a.desc = fr->desc; a.kl = fr->kl; a.ldesc = fr->ldesc; a.l3d = fr->l3d; }
    else {
        a.kp_un = (const hvo_keypoint *)(d + u_kp); a.depth = (const float *)(d + u_z); a.desc = (const uint8_t *)(d + u_desc);
        a.kl = (const hvo_keyline *)(d + u_kl); a.ldesc = (const uint8_t *)(d + u_ldesc); a.l3d = (const hvo_line3d *)(d + u_l3d);
    }
    a.hdr = (int32_t *)(d + o_hdr); a.ldir = (double *)(d + o_ldir); a.rel = (uint8_t *)(d + o_rel);
    const KfSideLayout *lay[2] = { &lp, &ll }; NkfSide *side[2] = { &a.p, &a.l };
    for (int q = 0; q < 2; q++) {
        NkfSide &s = *side[q]; const KfSideLayout &y = *lay[q];
        s.n = q ? n_kl : n_kp; s.first = q ? first_l : first_p;
        s.held = (const int32_t *)(d + y.held); s.key = (float *)(d + y.key); s.fl = (uint8_t *)(d + y.fl);
        s.o_held = (int32_t *)(d + y.o_held); s.o_index = (int32_t *)(d + y.o_index); s.o_slot = (int32_t *)(d + y.o_slot); s.o_status = (uint8_t *)(d + y.o_status); s.o_desc = (uint8_t *)(d + y.o_desc);
        s.o_pos = d + y.o_pos; s.o_nrm = d + y.o_nrm; s.o_wvec = (double *)(d + y.o_wvec); s.o_maxd = (float *)(d + y.o_maxd); s.o_mind = (float *)(d + y.o_mind);
    }
    kf_side_map(a.p, pm, hvo_point_map::POS, hvo_point_map::NRM, -1, hvo_point_map::MAXD, hvo_point_map::MIND, hvo_point_map::DESC);
    kf_side_map(a.l, lm, hvo_line_map::POS, hvo_line_map::NRM, hvo_line_map::WVEC, hvo_line_map::MAXD, hvo_line_map::MIND, hvo_line_map::DESC);
    KF_HIP(hipEventRecord(K->ev0, st));
    const int nmax = std::max(n_kp, n_kl);
    hipLaunchKernelGGL(k_nkf_keys, dim3((nmax + NKF_BLOCK - 1) / NKF_BLOCK), dim3(NKF_BLOCK), 0, st, a);
    if (n_kp) hipLaunchKernelGGL(k_nkf_points, dim3((n_kp + NKF_BLOCK - 1) / NKF_BLOCK), dim3(NKF_BLOCK), 0, st, a);
    if (n_kl) hipLaunchKernelGGL(k_nkf_lines, dim3((n_kl + NKF_BLOCK - 1) / NKF_BLOCK), dim3(NKF_BLOCK), 0, st, a);
    if (want_rel) hipLaunchKernelGGL(k_nkf_struct, dim3((n_kl + NKF_BLOCK - 1) / NKF_BLOCK, n_kl), dim3(NKF_BLOCK), 0, st, a);
    if (hipGetLastError() != hipSuccess) return kf_fail(K, HVO_ERR_HIP, "kernel launch");
    KF_HIP(hipEventRecord(K->ev1, st));
    KF_HIP(hipMemcpyAsync(h + r0, d + r0, r1 - r0, hipMemcpyDeviceToHost, st));
    KF_HIP(hipStreamSynchronize(st));
    KF_HIP(hipEventElapsedTime(&res->kernel_ms, K->ev0, K->ev1));
    // ---- the one block that came down: the caller's arrays and the maps' mirrors ----
    const int32_t *hdr = (const int32_t *)(h + o_hdr);
    if (hdr[0] == 1) return kf_fail(K, HVO_ERR_INVALID_ARG, "a line depth is NaN: the order of the reference's sort is undefined; nothing was written");
    res->n_point_candidates = n_kp ? hdr[1] : 0; res->n_line_candidates = n_kl ? hdr[2] : 0;
    const KfOut po = { io->held_points, io->pt_index, io->pt_slot, io->pt_status, io->pt_pos, io->pt_normal, nullptr, io->pt_max_dist, io->pt_min_dist };
    const KfOut lo = { io->held_lines, io->ln_index, io->ln_slot, io->ln_status, io->ln_pos, io->ln_normal, io->ln_wvec, io->ln_max_dist, io->ln_min_dist };
    const KfCols pc = { hvo_point_map::POS, hvo_point_map::NRM, -1, hvo_point_map::MAXD, hvo_point_map::MIND, hvo_point_map::DESC };
    const KfCols lc = { hvo_line_map::POS, hvo_line_map::NRM, hvo_line_map::WVEC, hvo_line_map::MAXD, hvo_line_map::MIND, hvo_line_map::DESC };
    kf_finish<float>(h, lp, n_kp, 3, first_p, pm, pc, po, &res->n_point_entries, &res->n_points_created);
    kf_finish<double>(h, ll, n_kl, 6, first_l, lm, lc, lo, &res->n_line_entries, &res->n_lines_created);
    if (want_rel && io->ln_rel) memcpy(io->ln_rel, h + o_rel, (size_t)res->n_line_entries * NL);
    return HVO_OK;
}

extern "C" {

void hvo_kfi_default_params(hvo_kfi_params *p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->mode = HVO_KFI_KEYFRAME; p->th_depth = 3.0f; p->n_levels = 8; p->line_n_levels = 1; p->line_scale_factor = 1.2f; p->line_geometry = 1;
    p->cos_par = cos(3.0 * 0.0174533); p->cos_perp = cos((90.0 - 3.0) * 0.0174533);
    p->first_point_slot = -1; p->first_line_slot = -1;
}

hvo_kf_insert *hvo_kf_insert_create(int device)
{
    if (device < 0 || hipSetDevice(device) != hipSuccess) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) return nullptr;      // the code object is gfx950 only
    hvo_kf_insert *K = new hvo_kf_insert();
    K->device = device;
    if (hipEventCreate(&K->ev0) != hipSuccess) { K->ev0 = nullptr; hvo_kf_insert_destroy(K); return nullptr; }
    if (hipEventCreate(&K->ev1) != hipSuccess) { K->ev1 = nullptr; hvo_kf_insert_destroy(K); return nullptr; }
    return K;
}

void hvo_kf_insert_destroy(hvo_kf_insert *K)
{
    if (!K) return;
    (void)hipSetDevice(K->device);
    (void)hipDeviceSynchronize();                                // the calls ran on their callers' streams
    if (K->ev0) (void)hipEventDestroy(K->ev0);
    if (K->ev1) (void)hipEventDestroy(K->ev1);
    if (K->d_ws) (void)hipFree(K->d_ws);
    if (K->h_pin) (void)hipHostFree(K->h_pin);
    delete K;
}

const char *hvo_kf_insert_last_error(const hvo_kf_insert *K) { return K ? K->last_error.c_str() : ""; }

int hvo_create_keyframe_features(hvo_kf_insert *K, hvo_ctx *ctx, hvo_point_map *pmap, hvo_line_map *lmap, const hvo_camera *cam, const float Tcw[12],
                                 const hvo_kfi_params *params, const hvo_kfi_frame *frame, hvo_kfi_io *io, hvo_kfi_result *res)
{
    if (!K || !ctx) return HVO_ERR_INVALID_ARG;
    if (!cam || !Tcw || !params || !frame || !io || !res) return kf_fail(K, HVO_ERR_INVALID_ARG, "a null argument");
    if (ctx->device != K->device) return kf_fail(K, HVO_ERR_INVALID_ARG, "the context lives on another device");
    if (hipSetDevice(K->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const int rc = kf_run(K, ctx->stream, pmap, lmap, cam, Tcw, params, nullptr, frame, ctx->scale, ctx->p.orb_nlevels, io, res);
    res->status = rc;
    if (rc) ctx->last_error = K->last_error;
    return rc;
}

int hvo_stream_create_keyframe_features(hvo_kf_insert *K, hvo_stream *s, hvo_point_map *pmap, hvo_line_map *lmap, int64_t cur, const hvo_camera *cam,
                                        const float Tcw[12], const hvo_kfi_params *params, hvo_kfi_io *io, hvo_kfi_result *res)
{
    if (!K || !s) return HVO_ERR_INVALID_ARG;
    if (!cam || !Tcw || !params || !io || !res) return kf_fail(K, HVO_ERR_INVALID_ARG, "a null argument");
    FrameView B; int rc;   // (the host waits for ev_orb and ev_lsd: the counts arrived with the frame's download)
    if ((rc = stream_view(s, cur, need_new_keyframe, s->s_match, B))) { K->last_error = s->last_error; return rc; }
    if (s->p.device != K->device) { s->last_error = "create key-frame features: the stream lives on another device"; K->last_error = s->last_error; return HVO_ERR_INVALID_ARG; }
    rc = kf_run(K, s->s_match, pmap, lmap, cam, Tcw, params, &B, nullptr, B.ctx->scale, B.ctx->p.orb_nlevels, io, res);
    res->status = rc;
    if (rc) s->last_error = K->last_error;
    return rc;
}

// Test door, not product API and not in include/hvo.h: the workspace's two blocks, at the sizes they have, set to fill_byte
int hvo_debug_kf_insert_fill(hvo_kf_insert *K, int fill_byte)
{
    if (!K || fill_byte < 0 || fill_byte > 255) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(K->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    KF_HIP(hipDeviceSynchronize());
    if (K->d_ws) KF_HIP(hipMemset(K->d_ws, fill_byte, K->ws_cap));
    if (K->h_pin) memset(K->h_pin, fill_byte, K->pin_cap);
    return HVO_OK;
}

}   // extern "C"
