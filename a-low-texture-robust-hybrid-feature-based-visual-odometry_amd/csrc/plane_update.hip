// plane_update.hip -- MapPlane::UpdateCoefficientsAndPoints on the resident plane map (reference src/MapPlane.cc:337-368 with a frame,
// :300-335 without; called from src/Tracking.cc:796-804 for every matched plane of every tracked frame, and :3208-3213 / :1407 on a new plane).
//
// One operation = one workgroup of k_pu_update (PU_THREADS threads); the operations of one launch touch different slots.
//   gather   the frame plane's voxel cloud (packed xyz where the plane tail left it) under the twelve doubles of the operation, then the
//            slot's cloud from its room (MERGE only), into three scratch arrays; a point that is not finite is marked; the float bounding box
//   grid     min_b / div_b as pcl::VoxelGrid forms them; the refusals (index overflow) leave before anything of the map is written
//   keys     (voxel index << 32 | point) per point, all ones for a dropped point and for the padding up to a power of two
//   sort     a bitonic network over the keys: every stage whose partner lies within PU_TILE keys runs in LDS, the others through global
//            scratch.  The keys are distinct, so the order is total and the network's instability does not matter
//   reduce   a head is a key whose voxel differs from its predecessor's; the heads' inclusive count is the voxel's rank = its place in the
//            result (ascending index).  Every point adds its 2^-24 m fixed-point coordinates to its voxel's 64-bit sums: integer
//            addition, so no order shows in the result
//   emit     (float)((double)sum / ((double)n * 2^24)) per voxel into the slot's room: x, y, z one cap apart, NaN up to a multiple of four
// Work and scratch follow the points (N log^2 N compare-exchanges, 12 + 8 + 32 bytes a point), never the bounding box's cells.
//
// The room is chosen on the host before the launch from the only bound it has, frame points + slot points: a cloud that could outgrow
// its room moves to the pool's end (rooms double, as in hvo_plane_map_set).  The gather has read the whole old room into scratch before
// the emission writes, so a slot that keeps its room is rewritten in place.
// Operations on the same slot go into successive launches: the second one's sizes are the first one's result.
#include "plane_map.hpp"
#include "frame_view.hpp"
#include "plane_update_xform.inc"
#include <math.h>
#include <string.h>
#include <algorithm>

#define PU_THREADS 1024
#define PU_TILE 4096                // keys of one LDS tile (32 KiB)

struct PuOp {
    double M[12];                   // the points' transform
    float T[12];                    // Tcw: ComputePlaneWorldCoeff of an INSERT
    float coef[4];                  // the frame plane's record coefficients (camera frame): ComputePlaneWorldCoeff of an INSERT
    const float *src;               // the frame plane's cloud, packed xyz
    long long old_first, new_first; // pool indices of the rooms
    size_t s_pts, s_keys, s_acc;    // byte offsets into the scratch
    int n_frame, n_before, old_cap, new_cap, p2, op, pad0, pad1;
};
struct PuRes { int status, n_after; float coef[4]; };

static __device__ __forceinline__ bool pu_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and the infinities

static __device__ __forceinline__ void pu_cas(unsigned long long &a, unsigned long long &b, bool up)
{
    if ((a > b) == up) { const unsigned long long t = a; a = b; b = t; }
}

__global__ __launch_bounds__(PU_THREADS) void k_pu_update(const PuOp *ops, PuRes *res, float *pool, char *scr)
{
    __shared__ unsigned long long tile[PU_TILE];
    __shared__ float red[6][PU_THREADS / 64];
    __shared__ int wsum[PU_THREADS / 64];
    __shared__ int s_carry;
    const PuOp &o = ops[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = o.n_frame + o.n_before, P2 = o.p2;
    float *px = (float *)(scr + o.s_pts), *py = px + N, *pz = py + N;
    unsigned long long *keys = (unsigned long long *)(scr + o.s_keys);
    long long *acc = (long long *)(scr + o.s_acc);

    // ---- gather, bounding box
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    int nvalid = 0;
    for (int i = tid; i < N; i += PU_THREADS) {
        float x, y, z;
        if (i < o.n_frame) {
            const double a = (double)o.src[3 * (size_t)i], b = (double)o.src[3 * (size_t)i + 1], c = (double)o.src[3 * (size_t)i + 2];
            x = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(o.M[0], a), __dmul_rn(o.M[1], b)), __dmul_rn(o.M[2], c)), o.M[3]);
            y = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(o.M[4], a), __dmul_rn(o.M[5], b)), __dmul_rn(o.M[6], c)), o.M[7]);
            z = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(o.M[8], a), __dmul_rn(o.M[9], b)), __dmul_rn(o.M[10], c)), o.M[11]);
        } else {
            const float *q = pool + o.old_first + (i - o.n_frame);
            x = q[0]; y = q[o.old_cap]; z = q[2 * (size_t)o.old_cap];
        }
        const bool ok = pu_finite(x) && pu_finite(y) && pu_finite(z);
        if (ok) {
            nvalid++;
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
            mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        } else {
            x = __builtin_nanf("");                              // the mark of a dropped point
        }
        px[i] = x; py[i] = y; pz[i] = z;
    }
    for (int k = 0; k < 3; k++)
        for (int s = 32; s > 0; s >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], s)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], s)); }
    for (int s = 32; s > 0; s >>= 1) nvalid += __shfl_xor(nvalid, s);
    if (lane == 0) { for (int k = 0; k < 3; k++) { red[k][wv] = mn[k]; red[3 + k][wv] = mx[k]; } wsum[wv] = nvalid; }
    if (tid == 0) s_carry = 0;
    __syncthreads();
    nvalid = 0;
    for (int w = 0; w < PU_THREADS / 64; w++) {
        for (int k = 0; k < 3; k++) { mn[k] = fminf(mn[k], red[k][w]); mx[k] = fmaxf(mx[k], red[3 + k][w]); }
        nvalid += wsum[w];
    }
    __syncthreads();                                             // wsum is used again below

    // ---- the grid, and the refusals
    const float inv_leaf = 1.0f / 0.1f;
    float fmin_b[3] = { 0.f, 0.f, 0.f }; long long div[3] = { 1, 1, 1 };
    bool refuse = false;
    if (nvalid > 0) {
        for (int k = 0; k < 3; k++) {
            const float lo = floorf(__fmul_rn(mn[k], inv_leaf)), hi = floorf(__fmul_rn(mx[k], inv_leaf));
            if (!(lo >= -2147483648.f && lo < 2147483648.f && hi >= -2147483648.f && hi < 2147483648.f)) { refuse = true; continue; }
            const int min_b = (int)lo, max_b = (int)hi;
            fmin_b[k] = (float)min_b; div[k] = (long long)max_b - (long long)min_b + 1;
        }
        if (!refuse) {
            if (div[0] > 2147483647ll || div[1] > 2147483647ll || div[2] > 2147483647ll) refuse = true;
            else if (div[0] * div[1] > 2147483647ll || div[0] * div[1] * div[2] > 2147483647ll) refuse = true;
        }
    }
    if (refuse) {                                                // uniform: every thread leaves; nothing of the map was written
        if (tid == 0) { res[blockIdx.x].status = HVO_ERR_UNSUPPORTED; res[blockIdx.x].n_after = o.n_before; }
        return;
    }

    // ---- keys; the sums start at zero
    for (int i = tid; i < P2; i += PU_THREADS) {
        unsigned long long key = ~0ull;
        if (i < N) {
            const float x = px[i];
            if (x == x) {
                const int i0 = (int)__fsub_rn(floorf(__fmul_rn(x, inv_leaf)), fmin_b[0]), i1 = (int)__fsub_rn(floorf(__fmul_rn(py[i], inv_leaf)), fmin_b[1]),
                          i2 = (int)__fsub_rn(floorf(__fmul_rn(pz[i], inv_leaf)), fmin_b[2]);
                const long long idx = (long long)i0 + (long long)i1 * div[0] + (long long)i2 * div[0] * div[1];
                key = ((unsigned long long)(unsigned)idx << 32) | (unsigned)i;
            }
        }
        keys[i] = key;
    }
    for (int i = tid; i < 4 * N; i += PU_THREADS) __hip_atomic_store(acc + i, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();

    // ---- bitonic sort, ascending
    const int T = P2 < PU_TILE ? P2 : PU_TILE;                   // a power of two
    for (int base = 0; base < P2; base += T) {                   // every k up to T inside the tile
        for (int i = tid; i < T; i += PU_THREADS) tile[i] = keys[base + i];
        __syncthreads();
        for (int k = 2; k <= T; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int p = tid; p < T / 2; p += PU_THREADS) {
                    const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1)), b = a | j;
                    pu_cas(tile[a], tile[b], ((base + a) & k) == 0);
                }
                __syncthreads();
            }
        for (int i = tid; i < T; i += PU_THREADS) keys[base + i] = tile[i];
        __syncthreads();
    }
    for (int k = 2 * T; k <= P2; k <<= 1) {
        for (int j = k >> 1; j >= T; j >>= 1) {                  // partners further than a tile apart: through global scratch
            for (int p = tid; p < P2 / 2; p += PU_THREADS) {
                const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1)), b = a | j;
                unsigned long long u = keys[a], v = keys[b];
                if ((u > v) == ((a & k) == 0)) { keys[a] = v; keys[b] = u; }
            }
            __syncthreads();
        }
        for (int base = 0; base < P2; base += T) {               // the rest of this k inside the tile
            for (int i = tid; i < T; i += PU_THREADS) tile[i] = keys[base + i];
            __syncthreads();
            for (int j = T >> 1; j > 0; j >>= 1) {
                for (int p = tid; p < T / 2; p += PU_THREADS) {
                    const int a = ((p & ~(j - 1)) << 1) | (p & (j - 1)), b = a | j;
                    pu_cas(tile[a], tile[b], ((base + a) & k) == 0);
                }
                __syncthreads();
            }
            for (int i = tid; i < T; i += PU_THREADS) keys[base + i] = tile[i];
            __syncthreads();
        }
    }

    // ---- heads, ranks, sums: the valid keys are the first nvalid of the sorted array
    for (int base = 0; base < nvalid; base += PU_THREADS) {
        const int p = base + tid;
        const bool in = p < nvalid;
        const unsigned long long key = in ? keys[p] : 0ull;
        const bool head = in && (p == 0 || (unsigned)(keys[p - 1] >> 32) != (unsigned)(key >> 32));
        const unsigned long long bm = __ballot(head);
        const int incl = __popcll(bm & ((2ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(bm);
        __syncthreads();
        int before = s_carry, all = 0;
        for (int w = 0; w < PU_THREADS / 64; w++) { if (w < wv) before += wsum[w]; all += wsum[w]; }
        if (in) {
            const int rank = before + incl - 1;
            const unsigned i = (unsigned)key;
            atomicAdd((unsigned long long *)(acc + 4 * (size_t)rank), (unsigned long long)__double2ll_rn(__dmul_rn((double)px[i], 16777216.0)));
            atomicAdd((unsigned long long *)(acc + 4 * (size_t)rank + 1), (unsigned long long)__double2ll_rn(__dmul_rn((double)py[i], 16777216.0)));
            atomicAdd((unsigned long long *)(acc + 4 * (size_t)rank + 2), (unsigned long long)__double2ll_rn(__dmul_rn((double)pz[i], 16777216.0)));
            atomicAdd((unsigned long long *)(acc + 4 * (size_t)rank + 3), 1ull);
        }
        __syncthreads();
        if (tid == 0) s_carry += all;
        __syncthreads();
    }
    const int nseg = s_carry;                                    // <= nvalid <= N <= new_cap

    // ---- emission into the room
    float *ox = pool + o.new_first, *oy = ox + o.new_cap, *oz = oy + o.new_cap;
    const int n4 = (nseg + 3) & ~3;
    for (int s = tid; s < n4; s += PU_THREADS) {
        float x, y, z;
        if (s < nseg) {
            const long long sx = __hip_atomic_load(acc + 4 * (size_t)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                            sy = __hip_atomic_load(acc + 4 * (size_t)s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                            sz = __hip_atomic_load(acc + 4 * (size_t)s + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                            n = __hip_atomic_load(acc + 4 * (size_t)s + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const double den = __dmul_rn((double)n, 16777216.0);
            x = (float)__ddiv_rn((double)sx, den); y = (float)__ddiv_rn((double)sy, den); z = (float)__ddiv_rn((double)sz, den);
        } else {
            x = y = z = __builtin_nanf("");
        }
        ox[s] = x; oy[s] = y; oz[s] = z;
    }
    if (tid == 0) {
        PuRes &R = res[blockIdx.x];
        R.status = HVO_OK; R.n_after = nseg;
        if (o.op == HVO_PLANE_UPDATE_INSERT) {                   // Frame::ComputePlaneWorldCoeff, as k_pa_prep writes it
            float c[4];
            for (int k = 0; k < 4; k++) c[k] = o.coef[k];
            for (int k = 0; k < 4; k++) {
                const double last = k == 3 ? 1.0 : 0.0;
                double s = __dmul_rn((double)o.T[k], (double)c[0]);
                s = __dadd_rn(s, __dmul_rn((double)o.T[4 + k], (double)c[1]));
                s = __dadd_rn(s, __dmul_rn((double)o.T[8 + k], (double)c[2]));
                s = __dadd_rn(s, __dmul_rn(last, (double)c[3]));
                R.coef[k] = (float)s;
            }
        }
    }
}

// ---------------------------------------------------------------- the call ----------------------------------------------------------------

static size_t pu_al(size_t v) { return (v + 255) & ~(size_t)255; }

static int pu_bad(hvo_plane_map *m, const char *why) { m->last_error = std::string("plane map update: ") + why; return HVO_ERR_INVALID_ARG; }

// The update of hvo_update_map_planes / hvo_stream_update_map_planes on stream st.  rec: the frame's records on the host (n_rec of them; the
// stream form's came down with the frame).  The cloud (n_cloud points, packed xyz): d_cloud on the device, or h_cloud on the host, which
// goes up with the descriptors.
int pu_run(hipStream_t st, hvo_plane_map *m, const hvo_plane_cloud *rec, int n_rec, const float *d_cloud, const float *h_cloud,
           int n_cloud, const float Tcw[12], const float Twc[12], const hvo_plane_update *upd, hvo_plane_update_result *res)
{
    // ---- the whole list is checked before anything is touched
    if (upd->n < 0 || upd->n > 64) return pu_bad(m, "n outside 0..64");
    int valid[PA_MAXP], nv = 0;
    for (int r = 0; r < n_rec && r < PA_MAXP; r++) if (rec[r].valid) valid[nv++] = r;
    int sim_slots = m->n_slots;
    for (int k = 0; k < upd->n; k++) {
        if (upd->plane[k] < 0 || upd->plane[k] >= nv) return pu_bad(m, "a plane index is not below the frame's valid planes");
        const hvo_plane_cloud &R = rec[valid[upd->plane[k]]];
        if (R.first < 0 || R.n_points < 0 || (long long)R.first + R.n_points > n_cloud) return pu_bad(m, "a plane's cloud lies outside the frame's cloud");
        if (upd->slot[k] < 0 || upd->slot[k] >= HVO_PLANE_MAP_MAX_SLOTS) return pu_bad(m, "a slot outside the map's range");
        if (upd->op[k] == HVO_PLANE_UPDATE_MERGE) {
            if (upd->slot[k] >= sim_slots) return pu_bad(m, "a MERGE into a slot that does not exist");
        } else if (upd->op[k] == HVO_PLANE_UPDATE_INSERT) {
            if (!Twc) return pu_bad(m, "an INSERT without Twc");
            sim_slots = std::max(sim_slots, upd->slot[k] + 1);
        } else return pu_bad(m, "an unknown op");
    }
    memset(res, 0, sizeof(*res));
    double Mmerge[12], Minsert[12];
    hvo_pu_transform(Tcw, Mmerge);
    for (int k = 0; k < 12; k++) Minsert[k] = Twc ? (double)Twc[k] : 0.0;

    // ---- rounds: the operations of one launch must not depend on one another.  Operation k waits for an earlier operation j when both
    // name the same slot, and when j is an INSERT past k's slot while k's slot lies past the map's end: whether k's slot exists at k's
    // turn (as a skipped, bad and empty slot) hangs on j's outcome, which only the kernel knows.  With that, every round's results are
    // taken into the map in list order and the whole list behaves as if applied one by one.  Appending several new planes in ascending
    // slot order, the usual case, stays one round.
    int round[64], n_rounds = 0;
    const int n0 = m->n_slots;
    for (int k = 0; k < upd->n; k++) {
        round[k] = 0;
        for (int j = 0; j < k; j++)
            if (upd->slot[j] == upd->slot[k] || (upd->op[j] == HVO_PLANE_UPDATE_INSERT && upd->slot[k] >= n0 && upd->slot[j] > upd->slot[k]))
                round[k] = std::max(round[k], round[j] + 1);
        n_rounds = std::max(n_rounds, round[k] + 1);
    }
    int rc;
    const size_t b_cloud = h_cloud ? pu_al((size_t)n_cloud * 12) : 0, b_ops = pu_al(64 * sizeof(PuOp)), b_res = pu_al(64 * sizeof(PuRes));
    for (int r = 0; r < n_rounds; r++) {
        int idx[64], n = 0;
        PuOp ops[64];
        size_t off = b_cloud + b_ops + b_res;
        const size_t pool_mark = m->pool_used;                   // the new rooms of this round lie behind it, in the order of ops[]
        for (int k = 0; k < upd->n; k++) {
            if (round[k] != r) continue;
            const hvo_plane_cloud &R = rec[valid[upd->plane[k]]];
            const int slot = upd->slot[k];
            const bool insert = upd->op[k] == HVO_PLANE_UPDATE_INSERT;
            // (a MERGE's slot exists by now unless the INSERT that was to make it was refused: then the MERGE is refused with it)
            const bool there = slot < m->n_slots;
            const int n_before = insert || !there ? 0 : m->slot[slot].npts;
            res->n_frame[k] = R.n_points; res->n_before[k] = n_before; res->n_after[k] = n_before;
            const long long N = (long long)R.n_points + n_before;
            if (N > HVO_PLANE_UPDATE_MAX_POINTS || (!insert && !there)) { res->status[k] = HVO_ERR_UNSUPPORTED; continue; }
            if ((rc = pm_reserve_slots(m, slot + 1))) return rc;
            const PaSlot &S = m->slot[slot];
            PuOp &o = ops[n];
            memset(&o, 0, sizeof(o));
            memcpy(o.M, insert ? Minsert : Mmerge, sizeof(o.M)); memcpy(o.T, Tcw, sizeof(o.T)); memcpy(o.coef, R.coef, sizeof(o.coef));
            o.src = nullptr;                                     // set below: the scratch may still move
            o.n_frame = R.n_points; o.n_before = n_before; o.op = upd->op[k];
            o.old_first = (long long)S.first; o.old_cap = S.cap;
            const size_t n4 = ((size_t)N + 3) & ~(size_t)3;
            if ((size_t)S.cap < n4) {                            // new room at the pool's end; kept only when the operation succeeds (below)
                size_t cap = 64;
                while (cap < n4) cap *= 2;
                if ((rc = pm_reserve_pool(m, m->pool_used + 3 * cap))) return rc;
                o.new_first = (long long)m->pool_used; o.new_cap = (int)cap; m->pool_used += 3 * cap;
            } else { o.new_first = o.old_first; o.new_cap = o.old_cap; }
            int p2 = 1;
            while (p2 < N) p2 *= 2;
            o.p2 = p2;
            o.s_pts = off; off += pu_al((size_t)N * 12);
            o.s_keys = off; off += pu_al((size_t)p2 * 8);
            o.s_acc = off; off += pu_al((size_t)N * 32);
            idx[n++] = k;
        }
        if (!n) continue;
        if ((rc = pm_scratch(m, st, off, b_cloud + b_ops + b_res))) return rc;
        const float *cloud = h_cloud ? (const float *)m->d_scr : d_cloud;
        for (int j = 0; j < n; j++) ops[j].src = cloud + 3 * (size_t)rec[valid[upd->plane[idx[j]]]].first;
        if (h_cloud && n_cloud) memcpy(m->h_scr, h_cloud, (size_t)n_cloud * 12);
        memcpy(m->h_scr + b_cloud, ops, (size_t)n * sizeof(PuOp));
        PM_HIP(hipMemcpyAsync(m->d_scr, m->h_scr, b_cloud + (size_t)n * sizeof(PuOp), hipMemcpyHostToDevice, st));
        PuRes *d_res = (PuRes *)(m->d_scr + b_cloud + b_ops), *h_res = (PuRes *)(m->h_scr + b_cloud + b_ops);
        hipLaunchKernelGGL(k_pu_update, dim3(n), dim3(PU_THREADS), 0, st, (const PuOp *)(m->d_scr + b_cloud), d_res, m->d_pool, m->d_scr);
        if (hipGetLastError() != hipSuccess) { m->last_error = "plane map update launch"; return HVO_ERR_HIP; }
        PM_HIP(hipMemcpyAsync(h_res, d_res, (size_t)n * sizeof(PuRes), hipMemcpyDeviceToHost, st));
        PM_HIP(hipStreamSynchronize(st));
        // ---- a refused operation's new room goes back to the pool when it lies at the pool's end (the kernel wrote nothing there): the rooms
        // were handed out in the order of ops[], so the walk goes backwards and stops at the first new room that is kept.  A refused room
        // with a kept one behind it stays abandoned, like a room a slot has outgrown.
        for (int j = n - 1; j >= 0; j--) {
            if (ops[j].new_first < (long long)pool_mark || ops[j].new_first == ops[j].old_first) continue;      // the slot kept its room
            if (h_res[j].status == HVO_OK) break;
            m->pool_used = (size_t)ops[j].new_first;
        }
        // ---- the host mirror, in list order
        bool table = false;
        for (int j = 0; j < n; j++) {
            const int k = idx[j], slot = upd->slot[k];
            res->status[k] = h_res[j].status;
            if (h_res[j].status != HVO_OK) continue;
            PaSlot &S = m->slot[slot];
            S.first = (size_t)ops[j].new_first; S.cap = ops[j].new_cap; S.npts = h_res[j].n_after;
            res->n_after[k] = h_res[j].n_after; res->n_done++;
            if (ops[j].op == HVO_PLANE_UPDATE_INSERT) {
                for (int c = 0; c < 4; c++) m->h_coef[(size_t)slot * 4 + c] = h_res[j].coef[c];
                PM_HIP(hipMemcpyAsync(m->d_coef + (size_t)slot * 4, &m->h_coef[(size_t)slot * 4], 16, hipMemcpyHostToDevice, st));
                if (slot >= m->n_slots) {                        // a new slot starts good; the ones skipped over stay bad and empty
                    m->h_bad[slot] = 0;
                    PM_HIP(hipMemcpyAsync(m->d_bad + slot, &m->h_bad[slot], 4, hipMemcpyHostToDevice, st));
                    m->n_slots = slot + 1;
                }
                table = true;
            }
        }
        if (table) PM_HIP(hipStreamSynchronize(st));
        m->chunks_dirty = true;
    }
    return HVO_OK;
}

extern "C" {

int hvo_plane_update_transform(const float Tcw[12], double M[12])
{
    if (!Tcw || !M) return HVO_ERR_INVALID_ARG;
    hvo_pu_transform(Tcw, M);
    return HVO_OK;
}

int hvo_plane_map_get_points(const hvo_plane_map *cm, int slot, float *xyz, int cap, int *n)
{
    hvo_plane_map *m = const_cast<hvo_plane_map *>(cm);          // the copy runs on the map's stream and reports through its last error
    if (!m || slot < 0 || slot >= m->n_slots || cap < 0 || (cap > 0 && !xyz)) return HVO_ERR_INVALID_ARG;
    const PaSlot &S = m->slot[slot];
    if (n) *n = S.npts;
    if (S.npts > cap) { m->last_error = "plane map points: cap is below the slot's count"; return HVO_ERR_CAPACITY; }
    if (!S.npts) return HVO_OK;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    std::vector<float> t((size_t)3 * S.npts);
    for (int k = 0; k < 3; k++)
        PM_HIP(hipMemcpyAsync(t.data() + (size_t)k * S.npts, m->d_pool + S.first + (size_t)k * S.cap, (size_t)S.npts * 4, hipMemcpyDeviceToHost, m->st));
    PM_HIP(hipStreamSynchronize(m->st));
    for (int i = 0; i < S.npts; i++) for (int k = 0; k < 3; k++) xyz[3 * (size_t)i + k] = t[(size_t)k * S.npts + i];
    return HVO_OK;
}

int hvo_update_map_planes(hvo_ctx *ctx, hvo_plane_map *m, const hvo_plane_cloud *records, int n_records, const float *cloud_xyz, int n_cloud,
                          const float Tcw[12], const float Twc[12], const hvo_plane_update *upd, hvo_plane_update_result *res)
{
    if (!ctx || !m || !Tcw || !upd || !res || n_records < 0 || n_records > 64 || n_cloud < 0 || (n_records > 0 && !records) || (n_cloud > 0 && !cloud_xyz))
        return HVO_ERR_INVALID_ARG;
    if (m->device != ctx->device) { ctx->last_error = "plane map update: the map lives on another device"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    static const float none[3] = { 0.f, 0.f, 0.f };
    const int rc = pu_run(ctx->stream, m, records, n_records, nullptr, n_cloud ? cloud_xyz : none, n_cloud, Tcw, Twc, upd, res);
    if (rc) ctx->last_error = m->last_error;
    return rc;
}

int hvo_stream_update_map_planes(hvo_stream *s, hvo_plane_map *m, int64_t cur, const float Tcw[12], const float Twc[12], const hvo_plane_update *upd,
                                 hvo_plane_update_result *res)
{
    if (!s || !m || !Tcw || !upd || !res) return HVO_ERR_INVALID_ARG;
    FrameView B; int rc;   // (the need's host count makes the host wait for the plane chain: the records and the cloud's count have come down)
    if ((rc = stream_view(s, cur, need_plane_update, s->s_match, B))) return rc;
    if (m->device != s->p.device) { s->last_error = "plane map update: the map lives on another device"; return HVO_ERR_INVALID_ARG; }
    rc = pu_run(s->s_match, m, B.h_pclouds, PA_MAXP, B.cloud_xyz, nullptr, B.n_cloud, Tcw, Twc, upd, res);
    if (rc) s->last_error = m->last_error;
    return rc;
}

}  // extern "C"
