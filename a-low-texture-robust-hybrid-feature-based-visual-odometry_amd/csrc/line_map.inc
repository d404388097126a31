// line_map.inc -- the local-map line search (included by match.hip after line_track.inc, whose window walk it shares).
//
//   LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th)       reference src/LSDmatcher.cpp:709-801 (RadiusByViewingCos 1436-1442)
//       over Frame::GetFeaturesInAreaForLine with its defaults           reference src/Frame.cc:1557-1627, include/Frame.h:131 (TH = 0.998f)
//       called every frame by Tracking::SearchLocalLines                 reference src/Tracking.cc:3279-3355
//   One query per map line in view (mbTrackInView && !isBad(), in vpMapLines order; the caller filters).  Radius 5 when mTrackViewCos > 0.998
//   (a float against a double), else 8, times th when th != 1; the predicted level is never read (GetFeaturesInAreaForLine ignores min/maxLevel)
//   and neither is eval_orient.  Per window line that is not held by a map line with observations: the 3-D gate -- the frame's camera-frame
//   direction mvLines3D[idx].first - .second (hvo_line3d A - B) against the map line's WORLD vector, |dot / (|f| |ml|)| in float against
//   cos 15 degrees in double (a NaN, from a line without a fitted 3-D line or a zero world vector, passes) -- then the descriptor distance into
//   two slots with strict '<': the two smallest (distance, visit position).  Accepted when best <= 95, unless the two octaves are equal and
//   best > nn_ratio * second (a float product).
//
//   k_lsbp_map_keys (one wave per query, all queries in parallel): lsbp_window's visit positions, the gates, and the query's candidates written
//       COMPACTED to the head of its key row (key = distance << 40 | visit position << 16 | index, as in k_lsbp_keys); lines occupied before the
//       call (t_occupied) never enter.  The wave also takes the LSBP_MAP_TOPK smallest keys (per lane a sorted short list, then repeated wave
//       minima) and stores them in order with their octaves (LsbpTop).
//   k_lsbp_map_epilogue (ONE wave, the queries in order): the claims of this call are bits in LDS.  Claims only take lines away, so the first
//       two unclaimed keys of the stored smallest ones are the two smallest free keys whenever there are two of them (or the stored keys are
//       all the query's candidates): the per-query work is LSBP_MAP_TOPK LDS bit tests.  Otherwise the wave takes the two smallest free keys of
//       the query's compacted list (its window's candidates, not all nt lines) with a 64-lane pair reduction and loads the two winners' octaves.
//       A claim bit is set only for a query with observations (q_blocks): a claim by a map line without observations can be overwritten.
// Float arithmetic as written there, no contraction (-ffp-contract=off); Eigen's dot product is taken as ((x x') + (y y')) + z z'.

#define LSBP_MAP_DIR_TH 0.998f    // GetFeaturesInAreaForLine's default TH (include/Frame.h:131)

#define LSBP_MAP_TOPK 4           // smallest keys kept per query: the epilogue falls back to the query's list only when fewer than two are unclaimed

struct LsbpTop { unsigned long long k[LSBP_MAP_TOPK]; int cnt, o[LSBP_MAP_TOPK], pad[3]; };   // per query: the smallest keys in order, #candidates, octaves

static __device__ __forceinline__ void top2_insert(unsigned long long &b1, unsigned long long &b2, unsigned long long k)
{
    const bool lt1 = k < b1, lt2 = k < b2;                       // (selects: no pointer to a slot, so both stay in registers)
    b2 = lt1 ? b1 : lt2 ? k : b2;
    b1 = lt1 ? k : b1;
}

// (b1 <= b2) of every lane -> the two smallest keys of the wave, in every lane (keys are distinct except LSBP_NONE)
static __device__ __forceinline__ void top2_wave(unsigned long long &b1, unsigned long long &b2)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long o1 = __shfl_xor(b1, o), o2 = __shfl_xor(b2, o);
        const bool lt = o1 < b1;
        b2 = lt ? (o2 < b1 ? o2 : b1) : (o1 < b2 ? o1 : b2);
        b1 = lt ? o1 : b1;
    }
}

// sorted (l0 <= l1 <= l2 <= l3) + k
static __device__ __forceinline__ void top4_insert(unsigned long long &l0, unsigned long long &l1, unsigned long long &l2, unsigned long long &l3, unsigned long long k)
{
    const bool c0 = k < l0, c1 = k < l1, c2 = k < l2, c3 = k < l3;
    l3 = c2 ? l2 : c3 ? k : l3;
    l2 = c1 ? l1 : c2 ? k : l2;
    l1 = c0 ? l0 : c1 ? k : l1;
    l0 = c0 ? k : l0;
}

// the smallest head of the wave's sorted lists, popped from the list that holds it (keys are distinct except LSBP_NONE)
static __device__ __forceinline__ unsigned long long top4_pop(unsigned long long &l0, unsigned long long &l1, unsigned long long &l2, unsigned long long &l3)
{
    unsigned long long m = l0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(m, o); m = v < m ? v : m; }
    const bool mine = l0 == m;
    l0 = mine ? l1 : l0; l1 = mine ? l2 : l1; l2 = mine ? l3 : l2; l3 = mine ? LSBP_NONE : l3;
    return m;
}

static __device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int i)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, i), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), i);
    return ((unsigned long long)hi << 32) | lo;
}

// the acceptance of LSDmatcher.cpp:782-790 on the two smallest keys and the winners' octaves: the accepted distance, or 256.  A distance of 256
// never enters the reference's slots (strict '<' against the initial 256), so such a second leaves bestLevel2 = -1.
static __device__ __forceinline__ int lsbp_map_accept(unsigned long long k1, unsigned long long k2, int o1, int o2, float nn_ratio)
{
    const int d1 = k1 == LSBP_NONE ? 256 : (int)(k1 >> 40), d2 = k2 == LSBP_NONE ? 256 : (int)(k2 >> 40);
    if (d1 > 95) return 256;
    const int l2 = d2 < 256 ? o2 : -1;
    if (o1 == l2 && (float)d1 > __fmul_rn(nn_ratio, (float)d2)) return 256;
    return d1;
}

__global__ __launch_bounds__(64) void k_lsbp_map_keys(LsbpMapDev a)
{
    __shared__ unsigned rank[LSBP_MAXT];
    const int q = blockIdx.x, lane = threadIdx.x, nt = a.nt;
    for (int j = lane; j < nt; j += 64) rank[j] = 0xFFFFFFFFu;
    __syncthreads();
    float r = (double)a.q_view_cos[q] > 0.998 ? 5.0f : 8.0f;    // RadiusByViewingCos; not scaled by level
    if (a.th != 1.0f) r = __fmul_rn(r, a.th);
    lsbp_window(rank, a.q_xyxy + 4 * (size_t)q, r, LSBP_MAP_DIR_TH, a.cell_start, a.cell_items, a.n_items, a.t_kl, a.t_fn, nt,
                a.mnMinX, a.mnMaxX, a.mnMinY, a.mnMaxY, lane);
    __syncthreads();
    const double wx = a.q_wvec[3 * (size_t)q], wy = a.q_wvec[3 * (size_t)q + 1], wz = a.q_wvec[3 * (size_t)q + 2];
    const float mag_ml = (float)sqrt(wx * wx + wy * wy + wz * wz);
    const ulonglong4 qd = *reinterpret_cast<const ulonglong4 *>(a.q_desc + 32 * (size_t)q);
    unsigned long long *K = a.keys + (size_t)q * nt;
    unsigned long long l0 = LSBP_NONE, l1 = LSBP_NONE, l2 = LSBP_NONE, l3 = LSBP_NONE;
    int cnt = 0;                                                 // candidates written so far (uniform)
    for (int j0 = 0; j0 < nt; j0 += 64) {
        const int j = j0 + lane;
        unsigned long long key = LSBP_NONE;
        const unsigned rk = j < nt ? rank[j] : 0xFFFFFFFFu;
        if (rk != 0xFFFFFFFFu && !(a.t_occ && a.t_occ[j])) {
            const hvo_line3d &L = a.t_l3d[j];
            const double vx = L.A[0] - L.B[0], vy = L.A[1] - L.B[1], vz = L.A[2] - L.B[2];
            const float dot = (float)(vx * wx + vy * wy + vz * wz);
            const float mag_f = (float)sqrt(vx * vx + vy * vy + vz * vz);
            const float angle = fabsf(dot / __fmul_rn(mag_f, mag_ml));
            if (!((double)angle < a.cos_normal)) {                // (a NaN passes)
                const int d = ham256(qd, *reinterpret_cast<const ulonglong4 *>(a.t_desc + 32 * (size_t)j));
                key = ((unsigned long long)d << 40) | ((unsigned long long)(rk & 0xFFFFFFu) << 16) | (unsigned long long)j;
            }
        }
        const unsigned long long m = __ballot(key != LSBP_NONE);
        if (key != LSBP_NONE) {
            K[cnt + __popcll(m & ((1ull << lane) - 1ull))] = key;
            top4_insert(l0, l1, l2, l3, key);
        }
        cnt += __popcll(m);
    }
    static_assert(LSBP_MAP_TOPK == 4, "top4_insert / top4_pop");
    unsigned long long k[LSBP_MAP_TOPK];
#pragma unroll
    for (int r = 0; r < LSBP_MAP_TOPK; r++) k[r] = top4_pop(l0, l1, l2, l3);
    if (lane == 0) {
        LsbpTop t;
        t.cnt = cnt; t.pad[0] = t.pad[1] = t.pad[2] = 0;
#pragma unroll
        for (int r = 0; r < LSBP_MAP_TOPK; r++) { t.k[r] = k[r]; t.o[r] = k[r] != LSBP_NONE ? a.t_kl[k[r] & 0xFFFFu].octave : -1; }
        a.top[q] = t;
    }
}

// the reference's loop over the map lines, by one wave; 64 queries' records are held one per lane and read with readlane
__global__ __launch_bounds__(64) void k_lsbp_map_epilogue(LsbpMapDev a)
{
    __shared__ unsigned occ[LSBP_MAXT / 32];                     // lines claimed in this call by map lines with observations
    const int lane = threadIdx.x, nt = a.nt;
    for (int wd = lane; wd < LSBP_MAXT / 32; wd += 64) occ[wd] = 0;
    __syncthreads();
    int nm = 0;
    for (int q0 = 0; q0 < a.nq; q0 += 64) {
        const int nb = min(64, a.nq - q0), qq = q0 + lane;
        LsbpTop t; t.cnt = 0;
#pragma unroll
        for (int r = 0; r < LSBP_MAP_TOPK; r++) { t.k[r] = LSBP_NONE; t.o[r] = -1; }
        if (lane < nb) {
            const LsbpTop &g = a.top[qq];
            t.cnt = g.cnt;
#pragma unroll
            for (int r = 0; r < LSBP_MAP_TOPK; r++) { t.k[r] = g.k[r]; t.o[r] = g.o[r]; }
        }
        const int blk = (lane < nb && a.q_blocks) ? (int)a.q_blocks[qq] : 0;
        int out_j = -1, out_d = 256;
        for (int i = 0; i < nb; i++) {
            // the first two unclaimed of the query's smallest keys
            unsigned long long k1 = LSBP_NONE, k2 = LSBP_NONE;
            int o1 = -1, o2 = -1, nfree = 0;
#pragma unroll
            for (int r = 0; r < LSBP_MAP_TOPK; r++) {
                const unsigned long long k = readlane64(t.k[r], i);
                const int o = __builtin_amdgcn_readlane(t.o[r], i);
                const unsigned j = k == LSBP_NONE ? 0u : (unsigned)(k & 0xFFFFu);
                const bool f = k != LSBP_NONE && !((occ[j >> 5] >> (j & 31)) & 1u);
                if (f && nfree == 1) { k2 = k; o2 = o; }
                if (f && nfree == 0) { k1 = k; o1 = o; }
                nfree += f ? 1 : 0;
            }
            const int cnt = __builtin_amdgcn_readlane(t.cnt, i);
            if (nfree < 2 && cnt > LSBP_MAP_TOPK) {
                // claims took all but one of them: the two smallest free keys of the query's whole list
                const unsigned long long *K = a.keys + (size_t)(q0 + i) * nt;
                k1 = k2 = LSBP_NONE;
                for (int s = lane; s < cnt; s += 64) {
                    const unsigned long long k = K[s];
                    const unsigned j = (unsigned)(k & 0xFFFFu);
                    if (!((occ[j >> 5] >> (j & 31)) & 1u)) top2_insert(k1, k2, k);
                }
                top2_wave(k1, k2);                                   // (k1 <= k2 per lane from top2_insert)
                o1 = k1 != LSBP_NONE ? a.t_kl[k1 & 0xFFFFu].octave : -1;
                o2 = k2 != LSBP_NONE ? a.t_kl[k2 & 0xFFFFu].octave : -1;
            }
            const int d = lsbp_map_accept(k1, k2, o1, o2, a.nn_ratio);
            if (d < 256) {
                const unsigned j = (unsigned)(k1 & 0xFFFFu);
                nm++;
                if (lane == i) { out_j = (int)j; out_d = d; }
                if (__builtin_amdgcn_readlane(blk, i)) {
                    if (lane == 0) occ[j >> 5] |= 1u << (j & 31);
                    __syncthreads();
                }
            }
        }
        if (lane < nb) { a.match_idx[qq] = out_j; a.match_dist[qq] = out_d; }
    }
    if (lane == 0) *a.n_matches = nm;
}

size_t match_lsbp_map_scratch_bytes(int nq, int nt) { return AL((size_t)nq * (size_t)std::max(nt, 1), unsigned long long) + AL(nq, LsbpTop) + 64; }

// device-resident form: a.keys / a.top are carved from `scratch` (match_lsbp_map_scratch_bytes(nq, nt) bytes); nq or nt of 0 launches nothing
int match_lsbp_map_enqueue(hipStream_t st, LsbpMapDev a, void *scratch)
{
    if (a.nt > LSBP_MAXT || a.nq > LSBP_MAP_MAXQ || a.n_items >= (1 << 22)) return HVO_ERR_UNSUPPORTED;
    if (a.nq < 1 || a.nt < 1) return HVO_OK;
    a.keys = (unsigned long long *)scratch;
    a.top = (LsbpTop *)((char *)scratch + AL((size_t)a.nq * (size_t)a.nt, unsigned long long));
    hipLaunchKernelGGL(k_lsbp_map_keys, dim3(a.nq), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_lsbp_map_epilogue, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? HVO_OK : HVO_ERR_HIP;
}

const char *match_lsbp_map_limit_text(int nq, int nt)
{
    if (nt > LSBP_MAXT) return "local-map line search: more than 2048 current lines";
    if (nq > LSBP_MAP_MAXQ) return "local-map line search: more than 16384 map lines in one call";
    return "local-map line search: more than 2^22 line grid items";
}

// host-array form (hvo_search_lines_by_projection_map): stage, run, fetch
int match_search_lines_by_projection_map(hvo_ctx *ctx, int nq, const float *q_xyxy, const float *q_view_cos, const double *q_wvec, const uint8_t *q_desc,
                                         const uint8_t *q_blocks, const hvo_keyline *t_kl, const double *t_linefn, const hvo_line3d *t_l3d, const uint8_t *t_desc,
                                         const uint8_t *t_occupied, int nt, const int32_t *cell_start, const int32_t *cell_items, int n_items,
                                         const float *bounds4, float th, float nn_ratio, int32_t *match_idx, int32_t *match_dist, int *n_matches)
{
    if (nt > LSBP_MAXT || nq > LSBP_MAP_MAXQ || n_items >= (1 << 22)) { ctx->last_error = match_lsbp_map_limit_text(nq, nt); return HVO_ERR_UNSUPPORTED; }
    if (nq == 0 || nt == 0) return HVO_OK;
    const int ncell = HVO_GRID_COLS * HVO_GRID_ROWS + 1;
    const size_t in_b = AL(nq * 4, float) + AL(nq, float) + AL(nq * 3, double) + AL(nq * 32, char) + AL(nq, char) + AL(nt, hvo_keyline) + AL(nt * 3, double) +
                        AL(nt, hvo_line3d) + AL(nt * 32, char) + AL(nt, char) + AL(ncell, int32_t) + AL(n_items, int32_t);
    const size_t out_b = AL(2 * (size_t)nq + 1, int32_t), sb = match_lsbp_map_scratch_bytes(nq, nt);
    int rc = arena_begin(ctx, in_b + out_b + sb + 2048, in_b + out_b + 2048);
    if (rc) return rc;
    LsbpMapDev a; memset(&a, 0, sizeof(a));
    a.nq = nq; a.nt = nt;
    a.q_xyxy = arena_up(ctx, q_xyxy, (size_t)nq * 4); a.q_view_cos = arena_up(ctx, q_view_cos, (size_t)nq); a.q_wvec = arena_up(ctx, q_wvec, (size_t)nq * 3);
    a.q_desc = arena_up(ctx, q_desc, (size_t)nq * 32); a.q_blocks = arena_up(ctx, q_blocks, (size_t)nq);
    a.t_kl = arena_up(ctx, t_kl, (size_t)nt); a.t_fn = arena_up(ctx, t_linefn, (size_t)nt * 3); a.t_l3d = arena_up(ctx, t_l3d, (size_t)nt);
    a.t_desc = arena_up(ctx, t_desc, (size_t)nt * 32); a.t_occ = arena_up(ctx, t_occupied, (size_t)nt);
    a.cell_start = arena_up(ctx, cell_start, (size_t)ncell); a.cell_items = arena_up(ctx, cell_items, (size_t)n_items); a.n_items = n_items;
    a.mnMinX = bounds4[0]; a.mnMaxX = bounds4[1]; a.mnMinY = bounds4[2]; a.mnMaxY = bounds4[3]; a.th = th; a.nn_ratio = nn_ratio;
    a.cos_normal = cos(15.0 / 180.0 * M_PI);
    int32_t *dout = arena_dev<int32_t>(ctx, 2 * (size_t)nq + 1), *hout = arena_host<int32_t>(ctx, 2 * (size_t)nq + 1);
    a.match_idx = dout; a.match_dist = dout + nq; a.n_matches = dout + 2 * nq;
    void *scratch = arena_dev<char>(ctx, sb);
    if ((rc = match_lsbp_map_enqueue(ctx->stream, a, scratch))) { ctx->last_error = "local-map line search launch"; return rc; }
    HVO_HIP(hipMemcpyAsync(hout, dout, (2 * (size_t)nq + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HVO_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(match_idx, hout, (size_t)nq * sizeof(int32_t)); memcpy(match_dist, hout + nq, (size_t)nq * sizeof(int32_t));
    *n_matches = hout[2 * nq];
    return HVO_OK;
}
