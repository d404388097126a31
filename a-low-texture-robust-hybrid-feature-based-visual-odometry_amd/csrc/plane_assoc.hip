// plane_assoc.hip -- PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:10-68, PointDistanceFromPlane :69-81,
// Frame::ComputePlaneWorldCoeff src/Frame.cc:2275-2280) against a plane map that stays on the device (hvo_plane_map).
//
// The map.  Per slot: world coefficients (float4), a bad flag, and the cloud's coordinates in one pool of floats.  A slot's room is a power
// of two of points (64 at least); its cloud lies there as three arrays, x at [first, first + cap), y and z one and two caps further, padded
// with NaN to a multiple of four points.  Three arrays, not packed xyz: the distance pass reads whole points into a lane's registers, and
// with 12-byte points a 16-byte load per lane either straddles points or leaves the wave's 64 loads 48 bytes apart; per coordinate every
// global_load_dwordx4 of a wave covers 1024 contiguous bytes and hands the lane four points (cdna_hip_programming.md, global-load width).
// hvo_plane_map_set transposes on the host, at key-frame rate.  A cloud that outgrows its room gets new room at the pool's end; rooms
// double, so the abandoned ones never exceed the live ones and nothing is compacted; the pool itself grows by one device copy.
//
// The match, the same four kernels for the host, stream and batch forms (bit-identical results):
//   k_pa_prep    one wave per frame: the valid planes in order (ballot + rank), pM = Tcw^T coef in double -> float, result defaults
//   k_pa_gate    one thread per (frame, slot): the angle of every frame plane (float, left to right, not contracted), the distance row
//                preset to 100, and the 64-bit mask of the frame planes whose |angle| passes aTh for that slot (0 for a bad slot)
//   k_pa_dist    one wave per chunk of 1024 points of one slot (work is balanced by points, not by slots): the chunk is loaded ONCE into
//                registers (3 x 4 dwordx4 per lane), then evaluated against every gated frame plane of every frame: three multiplies and
//                three adds per point as PointDistanceFromPlane writes them, |.|, a minimum that ignores NaN (v_min_f32 returns the other
//                operand), a wave reduction, and one atomicMin on the float's bits per (frame plane, slot) -- distances are >= 0, so the
//                unsigned order is the float order, and a minimum does not depend on the order of its operands
//   k_pa_decide  one wave per frame plane walks the finished row 64 slots at a time.  The three running thresholds of the reference's loop
//                are exclusive prefix minima / maxima: slot j is consumed by the association iff it is gated and its distance is below
//                min(dTh, gated distances before j); it becomes the vertical plane iff it is not consumed and |angle| is inside
//                min(verTh, such |angle| before j); else the parallel plane iff |angle| is outside max(parTh, such |angle| before j).
//                Strict comparisons against an exclusive prefix: the first slot wins a tie, as in the loop.
#include "hvo_internal.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#include "plane_map.hpp"

static size_t pa_al(size_t v) { return (v + 255) & ~(size_t)255; }

int pm_reserve_slots(hvo_plane_map *m, int want)
{
    if (want <= m->slot_cap) return HVO_OK;
    int cap = std::max(m->slot_cap, 64);
    while (cap < want) cap *= 2;
    float *nc = nullptr; int32_t *nb = nullptr;
    PM_HIP(hipMalloc((void **)&nc, (size_t)cap * 16));
    if (hipMalloc((void **)&nb, (size_t)cap * 4) != hipSuccess) { (void)hipFree(nc); m->last_error = "hipMalloc of the slot table"; return HVO_ERR_HIP; }
    m->h_coef.resize((size_t)cap * 4, 0.f); m->h_bad.resize(cap, 1); m->slot.resize(cap);
    // the host mirror is the truth: the whole table goes up again
    hipError_t e = hipMemcpyAsync(nc, m->h_coef.data(), (size_t)cap * 16, hipMemcpyHostToDevice, m->st);
    if (e == hipSuccess) e = hipMemcpyAsync(nb, m->h_bad.data(), (size_t)cap * 4, hipMemcpyHostToDevice, m->st);
    if (e == hipSuccess) e = hipStreamSynchronize(m->st);
    if (e != hipSuccess) { (void)hipFree(nc); (void)hipFree(nb); m->last_error = "slot table upload"; return HVO_ERR_HIP; }
    if (m->d_coef) (void)hipFree(m->d_coef);
    if (m->d_bad) (void)hipFree(m->d_bad);
    m->d_coef = nc; m->d_bad = nb; m->slot_cap = cap;
    return HVO_OK;
}

int pm_reserve_pool(hvo_plane_map *m, size_t want)
{
    if (want <= m->pool_cap) return HVO_OK;
    size_t cap = std::max(m->pool_cap, (size_t)3 * 4096);
    while (cap < want) cap *= 2;
    float *np = nullptr;
    PM_HIP(hipMalloc((void **)&np, cap * 4));
    if (m->pool_used) {
        hipError_t e = hipMemcpyAsync(np, m->d_pool, m->pool_used * 4, hipMemcpyDeviceToDevice, m->st);
        if (e == hipSuccess) e = hipStreamSynchronize(m->st);
        if (e != hipSuccess) { (void)hipFree(np); m->last_error = "point pool copy"; return HVO_ERR_HIP; }
    }
    if (m->d_pool) (void)hipFree(m->d_pool);
    m->d_pool = np; m->pool_cap = cap;
    return HVO_OK;
}

int pm_scratch(hvo_plane_map *m, hipStream_t st, size_t dbytes, size_t hbytes)
{
    if (m->scr_bytes < dbytes) {
        size_t cap = std::max(m->scr_bytes, (size_t)1 << 16);
        while (cap < dbytes) cap *= 2;
        PM_HIP(hipStreamSynchronize(st));
        if (m->d_scr) (void)hipFree(m->d_scr);
        m->d_scr = nullptr; m->scr_bytes = 0;
        PM_HIP(hipMalloc((void **)&m->d_scr, cap));
        m->scr_bytes = cap;
    }
    if (m->hscr_bytes < hbytes) {
        size_t cap = std::max(m->hscr_bytes, (size_t)1 << 14);
        while (cap < hbytes) cap *= 2;
        PM_HIP(hipStreamSynchronize(st));
        if (m->h_scr) (void)hipHostFree(m->h_scr);
        m->h_scr = nullptr; m->hscr_bytes = 0;
        PM_HIP(hipHostMalloc((void **)&m->h_scr, cap, hipHostMallocDefault));
        m->hscr_bytes = cap;
    }
    return HVO_OK;
}

extern "C" {

hvo_plane_map *hvo_plane_map_create(int device, int slots, int64_t points)
{
    if (device < 0 || slots < 0 || points < 0 || slots > HVO_PLANE_MAP_MAX_SLOTS) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hvo_plane_map *m = new hvo_plane_map();
    m->device = device;
    if (hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) != hipSuccess) { m->st = nullptr; hvo_plane_map_destroy(m); return nullptr; }
    if (pm_reserve_slots(m, std::max(slots, 1)) || pm_reserve_pool(m, (size_t)3 * (size_t)std::max<int64_t>(points, 1))) { hvo_plane_map_destroy(m); return nullptr; }
    return m;
}

void hvo_plane_map_destroy(hvo_plane_map *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->st) { (void)hipStreamSynchronize(m->st); (void)hipStreamDestroy(m->st); }
    if (m->d_coef) (void)hipFree(m->d_coef);
    if (m->d_bad) (void)hipFree(m->d_bad);
    if (m->d_pool) (void)hipFree(m->d_pool);
    if (m->h_stage) (void)hipHostFree(m->h_stage);
    if (m->d_chunks) (void)hipFree(m->d_chunks);
    if (m->d_scr) (void)hipFree(m->d_scr);
    if (m->h_scr) (void)hipHostFree(m->h_scr);
    delete m;
}

int hvo_plane_map_set(hvo_plane_map *m, int slot, const float coef[4], const float *xyz, int n_points)
{
    if (!m || !coef || slot < 0 || slot >= HVO_PLANE_MAP_MAX_SLOTS || n_points < 0 || (n_points > 0 && !xyz)) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    int rc;
    if ((rc = pm_reserve_slots(m, slot + 1))) return rc;
    PaSlot &S = m->slot[slot];
    const size_t n4 = ((size_t)n_points + 3) & ~(size_t)3;
    if ((size_t)S.cap < n4) {                                    // new room at the pool's end; the old room is abandoned
        size_t cap = 64;
        while (cap < n4) cap *= 2;
        if ((rc = pm_reserve_pool(m, m->pool_used + 3 * cap))) return rc;
        S.first = m->pool_used; S.cap = (int)cap; m->pool_used += 3 * cap;
    }
    if (n4) {
        if (m->stage_cap < 3 * n4) {
            size_t c = std::max((size_t)3 * 4096, m->stage_cap);
            while (c < 3 * n4) c *= 2;
            if (m->h_stage) (void)hipHostFree(m->h_stage);
            m->h_stage = nullptr; m->stage_cap = 0;
            PM_HIP(hipHostMalloc((void **)&m->h_stage, c * 4, hipHostMallocDefault));
            m->stage_cap = c;
        }
        float *x = m->h_stage, *y = x + n4, *z = y + n4;
        for (int i = 0; i < n_points; i++) { x[i] = xyz[3 * i]; y[i] = xyz[3 * i + 1]; z[i] = xyz[3 * i + 2]; }
        for (size_t i = n_points; i < n4; i++) x[i] = y[i] = z[i] = NAN;
        PM_HIP(hipMemcpyAsync(m->d_pool + S.first, x, n4 * 4, hipMemcpyHostToDevice, m->st));
        PM_HIP(hipMemcpyAsync(m->d_pool + S.first + S.cap, y, n4 * 4, hipMemcpyHostToDevice, m->st));
        PM_HIP(hipMemcpyAsync(m->d_pool + S.first + 2 * (size_t)S.cap, z, n4 * 4, hipMemcpyHostToDevice, m->st));
    }
    S.npts = n_points;
    for (int k = 0; k < 4; k++) m->h_coef[(size_t)slot * 4 + k] = coef[k];
    if (slot >= m->n_slots) {                                    // a new slot starts good; the ones skipped over stay bad and empty
        m->h_bad[slot] = 0;
        PM_HIP(hipMemcpyAsync(m->d_bad + slot, &m->h_bad[slot], 4, hipMemcpyHostToDevice, m->st));
        m->n_slots = slot + 1;
    }
    PM_HIP(hipMemcpyAsync(m->d_coef + (size_t)slot * 4, &m->h_coef[(size_t)slot * 4], 16, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipStreamSynchronize(m->st));
    m->chunks_dirty = true;
    return HVO_OK;
}

int hvo_plane_map_set_bad(hvo_plane_map *m, int slot, int bad)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    m->h_bad[slot] = bad ? 1 : 0;
    PM_HIP(hipMemcpyAsync(m->d_bad + slot, &m->h_bad[slot], 4, hipMemcpyHostToDevice, m->st));
    PM_HIP(hipStreamSynchronize(m->st));
    m->chunks_dirty = true;
    return HVO_OK;
}

int hvo_plane_map_counts(const hvo_plane_map *m, int *n_slots, int *n_good, int64_t *n_points)
{
    if (!m) return HVO_ERR_INVALID_ARG;
    int g = 0; int64_t p = 0;
    for (int j = 0; j < m->n_slots; j++) { g += m->h_bad[j] ? 0 : 1; p += m->slot[j].npts; }
    if (n_slots) *n_slots = m->n_slots;
    if (n_good) *n_good = g;
    if (n_points) *n_points = p;
    return HVO_OK;
}

int hvo_plane_map_slot(const hvo_plane_map *m, int slot, float coef[4], int *n_points, int *bad)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    if (coef) for (int k = 0; k < 4; k++) coef[k] = m->h_coef[(size_t)slot * 4 + k];
    if (n_points) *n_points = m->slot[slot].npts;
    if (bad) *bad = m->h_bad[slot];
    return HVO_OK;
}

const char *hvo_plane_map_last_error(const hvo_plane_map *m) { return m ? m->last_error.c_str() : ""; }

}  // extern "C"

// ---------------------------------------------------------------- kernels ----------------------------------------------------------------

struct PaArgs {
    const float *coef;                       // host form: n x 4 camera-frame coefficients, else null
    int n;                                   //            their count
    const hvo_plane_cloud *pc; size_t pc_stride;   // resident forms: frame f's 64 records at (char *)pc + f * pc_stride
    const float *tcw;                        // nframes x 12
    int nframes, nslots;
    float dTh, aTh, verTh, parTh;
    const float *m_coef; const int32_t *m_bad; const float *pool;
    const PaChunk *chunks; int nchunks;
    hvo_plane_match *res;                    // nframes
    unsigned long long *gate;                // nframes x nslots
    float *angle, *dist;                     // nframes x 64 x nslots
};

// Frame::ComputePlaneWorldCoeff: (Tcw^T coef)[c] = sum over r = 0..3 of Tcw[r][c] coef[r], products and sums in double, left to right;
// row 3 of Tcw is (0, 0, 0, 1)
__global__ __launch_bounds__(64) void k_pa_prep(PaArgs a)
{
    const int f = blockIdx.x, l = threadIdx.x;
    hvo_plane_match *R = a.res + f;
    bool valid; float c[4];
    if (a.coef) {
        valid = l < a.n;
        for (int k = 0; k < 4; k++) c[k] = valid ? a.coef[l * 4 + k] : 0.f;
    } else {
        const hvo_plane_cloud *pc = (const hvo_plane_cloud *)((const char *)a.pc + (size_t)f * a.pc_stride) + l;
        valid = pc->valid != 0;
        for (int k = 0; k < 4; k++) c[k] = pc->coef[k];
    }
    const unsigned long long vm = __ballot(valid);
    const int rank = __popcll(vm & ((1ull << l) - 1ull)), n = __popcll(vm);
    R->match[l] = -1; R->vertical[l] = -1; R->parallel[l] = -1; R->dist[l] = 100.f;
    if (l >= n) { R->plane_idx[l] = -1; for (int k = 0; k < 4; k++) R->pM[l][k] = 0.f; }
    if (l == 0) { R->n_planes = n; R->n_matches = 0; }
    if (valid) {
        const float *T = a.tcw + f * 12;
        for (int k = 0; k < 4; k++) {
            const double last = k == 3 ? 1.0 : 0.0;
            double s = __dmul_rn((double)T[k], (double)c[0]);
            s = __dadd_rn(s, __dmul_rn((double)T[4 + k], (double)c[1]));
            s = __dadd_rn(s, __dmul_rn((double)T[8 + k], (double)c[2]));
            s = __dadd_rn(s, __dmul_rn(last, (double)c[3]));
            R->pM[rank][k] = (float)s;
        }
        R->plane_idx[rank] = l;
    }
}

__global__ __launch_bounds__(256) void k_pa_gate(PaArgs a)
{
    __shared__ float pm[PA_MAXP][3];
    const int f = blockIdx.y, tid = threadIdx.x;
    const hvo_plane_match *R = a.res + f;
    const int n = R->n_planes;
    if (tid < PA_MAXP * 3) pm[tid / 3][tid % 3] = R->pM[tid / 3][tid % 3];
    __syncthreads();
    const int j = blockIdx.x * 256 + tid;
    if (j >= a.nslots) return;
    const float4 w = ((const float4 *)a.m_coef)[j];
    const bool good = a.m_bad[j] == 0;
    unsigned long long mask = 0;
    const size_t row0 = (size_t)f * PA_MAXP * a.nslots + j;
    for (int i = 0; i < n; i++) {
        const float ang = __fadd_rn(__fadd_rn(__fmul_rn(pm[i][0], w.x), __fmul_rn(pm[i][1], w.y)), __fmul_rn(pm[i][2], w.z));
        a.angle[row0 + (size_t)i * a.nslots] = ang;
        a.dist[row0 + (size_t)i * a.nslots] = 100.f;
        if (good && (ang > a.aTh || ang < -a.aTh)) mask |= 1ull << i;
    }
    a.gate[(size_t)f * a.nslots + j] = mask;
}

// |pM0 x + pM1 y + pM2 z + pM3| folded into the running minimum; a NaN distance leaves m as it is (fminf returns the other operand)
static __device__ __forceinline__ float pa_fold(float m, float p0, float p1, float p2, float p3, float x, float y, float z)
{
    const float d = fabsf(__fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(p0, x), __fmul_rn(p1, y)), __fmul_rn(p2, z)), p3));
    return fminf(m, d);
}

__global__ __launch_bounds__(64 * PA_DIST_WAVES) void k_pa_dist(PaArgs a)
{
    const int lane = threadIdx.x & 63;
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * PA_DIST_WAVES + (threadIdx.x >> 6));
    if (c >= a.nchunks) return;
    const PaChunk ch = a.chunks[c];
    const float qnan = __builtin_nanf("");
    float4 X[4], Y[4], Z[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int p = (k * 64 + lane) * 4;
        if (p < ch.count) {                                      // count and cap are multiples of 4 and the room is padded with NaN
            const float *q = a.pool + ch.xoff + p;
            X[k] = *(const float4 *)q; Y[k] = *(const float4 *)(q + ch.cap); Z[k] = *(const float4 *)(q + 2 * (size_t)ch.cap);
        } else {
            X[k] = Y[k] = Z[k] = make_float4(qnan, qnan, qnan, qnan);
        }
    }
    for (int f = 0; f < a.nframes; f++) {
        unsigned long long mask = a.gate[(size_t)f * a.nslots + ch.slot];
        const hvo_plane_match *R = a.res + f;
        while (mask) {
            const int i = __builtin_ctzll(mask);
            mask &= mask - 1;
            const float p0 = R->pM[i][0], p1 = R->pM[i][1], p2 = R->pM[i][2], p3 = R->pM[i][3];
            float m = 100.f;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                m = pa_fold(m, p0, p1, p2, p3, X[k].x, Y[k].x, Z[k].x);
                m = pa_fold(m, p0, p1, p2, p3, X[k].y, Y[k].y, Z[k].y);
                m = pa_fold(m, p0, p1, p2, p3, X[k].z, Y[k].z, Z[k].z);
                m = pa_fold(m, p0, p1, p2, p3, X[k].w, Y[k].w, Z[k].w);
            }
            for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
            if (lane == 0 && m < 100.f)
                atomicMin((unsigned *)&a.dist[((size_t)f * PA_MAXP + i) * a.nslots + ch.slot], __float_as_uint(m));
        }
    }
}

static __device__ __forceinline__ float pa_scan_min_excl(float v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(v, o); if (lane >= o) v = fminf(v, t); }
    const float e = __shfl_up(v, 1);
    return lane == 0 ? INFINITY : e;
}
static __device__ __forceinline__ float pa_scan_max_excl(float v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(v, o); if (lane >= o) v = fmaxf(v, t); }
    const float e = __shfl_up(v, 1);
    return lane == 0 ? -INFINITY : e;
}

__global__ __launch_bounds__(64) void k_pa_decide(PaArgs a)
{
    const int i = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    hvo_plane_match *R = a.res + f;
    if (i >= R->n_planes) return;
    const size_t row = ((size_t)f * PA_MAXP + i) * a.nslots;
    float ld = a.dTh, lv = a.verTh, lp = a.parTh, md = 100.f;
    int mi = -1, vi = -1, pi = -1;
    for (int base = 0; base < a.nslots; base += 64) {
        const int j = base + lane;
        const bool in = j < a.nslots;
        const float ang = in ? a.angle[row + j] : 0.f, d = in ? a.dist[row + j] : 100.f;
        const bool ok = in && a.m_bad[j] == 0;
        const float aa = fabsf(ang);
        // association: consumed iff gated and below every gated distance before it (and below dTh)
        const bool gated = ok && (ang > a.aTh || ang < -a.aTh);
        float t = fminf(ld, pa_scan_min_excl(gated && d < ld ? d : INFINITY, lane));
        const bool consumed = gated && d < t;
        unsigned long long bm = __ballot(consumed);
        if (bm) { const int last = 63 - __builtin_clzll(bm); mi = base + last; md = __shfl(d, last); ld = md; }
        // vertical: of the slots the association did not consume
        const bool cand = ok && !consumed;
        t = fminf(lv, pa_scan_min_excl(cand && ang < lv && ang > -lv ? aa : INFINITY, lane));
        const bool vup = cand && ang < t && ang > -t;
        bm = __ballot(vup);
        if (bm) { const int last = 63 - __builtin_clzll(bm); vi = base + last; lv = __shfl(aa, last); }
        // parallel: of the rest
        const bool rest = cand && !vup;
        t = fmaxf(lp, pa_scan_max_excl(rest && (ang > lp || ang < -lp) ? aa : -INFINITY, lane));
        const bool pup = rest && (ang > t || ang < -t);
        bm = __ballot(pup);
        if (bm) { const int last = 63 - __builtin_clzll(bm); pi = base + last; lp = __shfl(aa, last); }
    }
    if (lane == 0) {
        R->match[i] = mi; R->vertical[i] = vi; R->parallel[i] = pi; R->dist[i] = md;
        if (mi >= 0) atomicAdd(&R->n_matches, 1);
    }
}

// ---------------------------------------------------------------- the call ----------------------------------------------------------------

static int pa_refresh_chunks(hvo_plane_map *m)
{
    if (!m->chunks_dirty) return HVO_OK;
    m->chunks.clear();
    for (int j = 0; j < m->n_slots; j++) {
        const PaSlot &S = m->slot[j];
        if (m->h_bad[j] || S.npts <= 0) continue;
        const int n4 = (S.npts + 3) & ~3;
        for (int o = 0; o < n4; o += PA_CHUNK) {
            PaChunk c; c.xoff = (long long)S.first + o; c.cap = S.cap; c.count = std::min(PA_CHUNK, n4 - o); c.slot = j; c.pad = 0;
            m->chunks.push_back(c);
        }
    }
    if (m->chunks.size() > m->chunk_cap) {
        size_t cap = std::max(m->chunk_cap, (size_t)1024);
        while (cap < m->chunks.size()) cap *= 2;
        if (m->d_chunks) (void)hipFree(m->d_chunks);
        m->d_chunks = nullptr; m->chunk_cap = 0;
        PM_HIP(hipMalloc((void **)&m->d_chunks, cap * sizeof(PaChunk)));
        m->chunk_cap = cap;
    }
    if (!m->chunks.empty()) {
        PM_HIP(hipMemcpyAsync(m->d_chunks, m->chunks.data(), m->chunks.size() * sizeof(PaChunk), hipMemcpyHostToDevice, m->st));
        PM_HIP(hipStreamSynchronize(m->st));
    }
    m->chunks_dirty = false;
    return HVO_OK;
}

// SearchMapByCoefficients of nframes frames against the map on stream st, results in res (host) when the call returns.  Frame planes: the
// host array coef (n x 4, one frame) or the resident plane_clouds records.  dist_mat / angle_mat: host, n x slots (host form only).
int pa_match(hipStream_t st, hvo_plane_map *m, const float *coef, int n, const hvo_plane_cloud *d_pc, size_t pc_stride, int nframes, const float *Tcw,
             const float th[4], hvo_plane_match *res, float *dist_mat, float *angle_mat)
{
    static const float th_default[4] = { 0.1f, 0.86f, 0.08716f, 0.9962f };          // include/PlaneMatcher.h:17
    if (!th) th = th_default;
    for (int k = 0; k < 4; k++) if (th[k] != th[k]) { m->last_error = "plane association: a threshold is NaN"; return HVO_ERR_INVALID_ARG; }
    int rc;
    if ((rc = pa_refresh_chunks(m))) return rc;
    const int ns = m->n_slots;
    const size_t b_in = pa_al((size_t)nframes * 48 + PA_MAXP * 16), b_res = pa_al((size_t)nframes * sizeof(hvo_plane_match)),
                 b_gate = pa_al((size_t)nframes * ns * 8), b_mat = pa_al((size_t)nframes * PA_MAXP * ns * 4);
    const size_t bytes = b_in + b_res + b_gate + 2 * b_mat, hbytes = b_in + b_res;
    if ((rc = pm_scratch(m, st, bytes, hbytes))) return rc;
    float *h_in = (float *)m->h_scr;
    memcpy(h_in, Tcw, (size_t)nframes * 48);
    if (coef && n) memcpy(h_in + (size_t)nframes * 12, coef, (size_t)n * 16);
    PM_HIP(hipMemcpyAsync(m->d_scr, h_in, (size_t)nframes * 48 + (coef ? (size_t)n * 16 : 0), hipMemcpyHostToDevice, st));
    PaArgs a;
    a.coef = coef ? (const float *)m->d_scr + (size_t)nframes * 12 : nullptr; a.n = n;
    a.pc = d_pc; a.pc_stride = pc_stride;
    a.tcw = (const float *)m->d_scr; a.nframes = nframes; a.nslots = ns;
    a.dTh = th[0]; a.aTh = th[1]; a.verTh = th[2]; a.parTh = th[3];
    a.m_coef = m->d_coef; a.m_bad = m->d_bad; a.pool = m->d_pool;
    a.chunks = m->d_chunks; a.nchunks = (int)m->chunks.size();
    a.res = (hvo_plane_match *)(m->d_scr + b_in);
    a.gate = (unsigned long long *)(m->d_scr + b_in + b_res);
    a.angle = (float *)(m->d_scr + b_in + b_res + b_gate); a.dist = (float *)(m->d_scr + b_in + b_res + b_gate + b_mat);
    hipLaunchKernelGGL(k_pa_prep, dim3(nframes), dim3(64), 0, st, a);
    if (ns > 0) {
        hipLaunchKernelGGL(k_pa_gate, dim3((ns + 255) / 256, nframes), dim3(256), 0, st, a);
        if (a.nchunks > 0)
            hipLaunchKernelGGL(k_pa_dist, dim3((a.nchunks + PA_DIST_WAVES - 1) / PA_DIST_WAVES), dim3(64 * PA_DIST_WAVES), 0, st, a);
        hipLaunchKernelGGL(k_pa_decide, dim3(PA_MAXP, nframes), dim3(64), 0, st, a);
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "plane association launch"; return HVO_ERR_HIP; }
    hvo_plane_match *h_res = (hvo_plane_match *)(m->h_scr + b_in);
    PM_HIP(hipMemcpyAsync(h_res, a.res, (size_t)nframes * sizeof(hvo_plane_match), hipMemcpyDeviceToHost, st));
    if (ns > 0 && n > 0 && dist_mat) PM_HIP(hipMemcpyAsync(dist_mat, a.dist, (size_t)n * ns * 4, hipMemcpyDeviceToHost, st));
    if (ns > 0 && n > 0 && angle_mat) PM_HIP(hipMemcpyAsync(angle_mat, a.angle, (size_t)n * ns * 4, hipMemcpyDeviceToHost, st));
    PM_HIP(hipStreamSynchronize(st));
    memcpy(res, h_res, (size_t)nframes * sizeof(hvo_plane_match));
    return HVO_OK;
}

int pa_map_device(const hvo_plane_map *m) { return m->device; }
const char *pa_map_error(const hvo_plane_map *m) { return m->last_error.c_str(); }
