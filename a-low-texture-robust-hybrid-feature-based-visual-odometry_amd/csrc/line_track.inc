// line_track.inc -- the line tracker's own two matching calls (round 5; included by match.hip, whose staging arena it uses).
//
//   LSDmatcher::SearchByGeomNApearance(Cur, Last, desc_th, matches_12)   reference src/LSDmatcher.cpp:36-108 (computeAngle2D 20-34)
//       = match() -> matchNNR on the two descriptor sets (k_hamming_knn2 + k_nnr_epilogue, above) and then, per pair, the 20-degree angle
//         gate on the in-octave end points and the "start OR end point within a tenth of the image bounds" gate: k_lines_geom_gate.
//   LSDmatcher::SearchByProjection(Cur, Last, th)                         reference src/LSDmatcher.cpp:561-662
//       over Frame::GetFeaturesInAreaForLine                               reference src/Frame.cc:1557-1627
//       One query per last-frame line whose map line is in view.  The reference collects the window's lines in a fixed order -- the three
//       sample points (start, middle, end), for each the grid cells of its window ix-major, a cell's lines in insertion order, a line
//       kept at its FIRST visit that passes the direction and the distance test for THAT sample point -- then walks them with a strict
//       minimum over the Hamming distance, so ties go to the earlier visit; and a current line claimed by an earlier query whose map line
//       has observations is passed over by later ones.  Restated as in k_search_by_projection: per query and in parallel (one wave per
//       query) every current line gets its key
//           key = distance << 40 | visit position << 16 | index        (or "none": not in the window, or a gate failed)
//       where the visit position is found by walking the window's CSR ranges with all lanes (a cell row of the grid is one contiguous
//       range of items; an LDS word per line keeps the smallest passing position), and k_lsbp_epilogue -- ONE wave -- walks the queries in
//       order with the occupancy bits in LDS: the smallest key among the free lines is what the reference's loop finds.
// Float arithmetic as written there (sqrt and / of floats are the correctly rounded ones under hipcc's defaults; the thresholds cos 10 / 20
// degrees come from the host's libm, like the oracle's); no contraction (-ffp-contract=off).

#define LSBP_MAXT 2048            // current-frame lines per call (a rank word and an occupancy bit each in LDS)
#define LSBP_NONE 0xFFFFFFFFFFFFFFFFull

// |cos| of the angle between the in-octave directions of two key lines (LSDmatcher::computeAngle2D on float differences widened to double)
static __device__ __forceinline__ double lt_angle2d(const hvo_keyline &a, const hvo_keyline &b)
{
    const double ax = (double)__fsub_rn(a.eox, a.sox), ay = (double)__fsub_rn(a.eoy, a.soy);
    const double bx = (double)__fsub_rn(b.eox, b.sox), by = (double)__fsub_rn(b.eoy, b.soy);
    double dot = 0.0; dot += ax * bx; dot += ay * by;
    const double ma = sqrt(ax * ax + ay * ay), mb = sqrt(bx * bx + by * by);
    return fabs(dot / (ma * mb));
}

// SearchByGeomNApearance's loop over matches_12 (src/LSDmatcher.cpp:54-105).  m12: matchNNR's result, edited in place.
__global__ __launch_bounds__(256) void k_lines_geom_gate(int32_t *__restrict__ m12, const hvo_keyline *__restrict__ kl_last, const uint8_t *__restrict__ has_ml, int n_last,
                                                         const hvo_keyline *__restrict__ kl_cur, double dW, double dH, double cos_th,
                                                         uint8_t *__restrict__ accepted, int *__restrict__ nmatch)
{
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i1 = threadIdx.x; i1 < n_last; i1 += 256) {
        bool acc = false;
        const int i2 = m12[i1];
        if ((!has_ml || has_ml[i1]) && i2 >= 0) {
            const hvo_keyline c = kl_cur[i2], l = kl_last[i1];
            if (!(c.sx == 0)) {
                if (lt_angle2d(c, l) < cos_th) m12[i1] = -1;
                else if (((double)fabsf(__fsub_rn(c.sox, l.sox)) > dW || (double)fabsf(__fsub_rn(c.soy, l.soy)) > dH) &&
                         ((double)fabsf(__fsub_rn(c.eox, l.eox)) > dW || (double)fabsf(__fsub_rn(c.eoy, l.eoy)) > dH)) m12[i1] = -1;
                else acc = true;
            }
        }
        accepted[i1] = acc ? 1 : 0;
        mine += acc;
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) *nmatch = s_cnt;
}


// Frame::GetFeaturesInAreaForLine's window walk (src/Frame.cc:1557-1627) by one wave: rank[j] (LDS, preset to ~0) receives the smallest visit
// position at which line j passes the direction test (|cos| >= dir_th; a NaN passes) and the distance test for that sample point; r is the radius.
static __device__ __forceinline__ void lsbp_window(unsigned *rank, const float *__restrict__ q4, float r, float dir_th, const int32_t *__restrict__ cell_start,
                                                   const int32_t *__restrict__ cell_items, int n_items, const hvo_keyline *__restrict__ t_kl,
                                                   const double *__restrict__ t_fn, int nt, float mnMinX, float mnMaxX, float mnMinY, float mnMaxY, int lane)
{
    const float x1 = q4[0], y1 = q4[1], x2 = q4[2], y2 = q4[3];
    const float xm = (float)((double)__fadd_rn(x1, x2) / 2.0), ym = (float)((double)__fadd_rn(y1, y2) / 2.0);      // the sample points: start, middle, end
    float d1x = __fsub_rn(x1, x2), d1y = __fsub_rn(y1, y2);
    const float n1 = sqrtf(__fadd_rn(__fmul_rn(d1x, d1x), __fmul_rn(d1y, d1y)));
    d1x = d1x / n1; d1y = d1y / n1;
    const float invW = (float)HVO_GRID_COLS / __fsub_rn(mnMaxX, mnMinX), invH = (float)HVO_GRID_ROWS / __fsub_rn(mnMaxY, mnMinY);
    unsigned base = 0;                                           // visits so far (uniform)
    for (int i = 0; i < 3; i++) {
        const float x = i == 0 ? x1 : i == 1 ? xm : x2, y = i == 0 ? y1 : i == 1 ? ym : y2;      // (selects: no stack array)
        int cx0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(x, mnMinX), r), invW)); if (cx0 < 0) cx0 = 0;
        if (cx0 >= HVO_GRID_COLS) continue;
        int cx1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(x, mnMinX), r), invW)); if (cx1 > HVO_GRID_COLS - 1) cx1 = HVO_GRID_COLS - 1;
        if (cx1 < 0) continue;
        int cy0 = (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(y, mnMinY), r), invH)); if (cy0 < 0) cy0 = 0;
        if (cy0 >= HVO_GRID_ROWS) continue;
        int cy1 = (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(y, mnMinY), r), invH)); if (cy1 > HVO_GRID_ROWS - 1) cy1 = HVO_GRID_ROWS - 1;
        if (cy1 < 0) continue;
        for (int ix = cx0; ix <= cx1; ix++) {
            // cells (ix, cy0 .. cy1) are neighbours in the CSR: one contiguous range of items, in the reference's visiting order
            const int k0 = cell_start[ix * HVO_GRID_ROWS + cy0], k1 = min(cell_start[ix * HVO_GRID_ROWS + cy1 + 1], n_items);
            for (int k = k0 + lane; k < k1; k += 64) {
                const int j = cell_items[k];
                if ((unsigned)j >= (unsigned)nt) continue;
                const hvo_keyline t = t_kl[j];
                float d2x = __fsub_rn(t.sx, t.ex), d2y = __fsub_rn(t.sy, t.ey);
                const float n2 = sqrtf(__fadd_rn(__fmul_rn(d2x, d2x), __fmul_rn(d2y, d2y)));
                d2x = d2x / n2; d2y = d2y / n2;
                const float cs = fabsf(__fadd_rn(__fmul_rn(d1x, d2x), __fmul_rn(d1y, d2y)));
                if (cs < dir_th) continue;                       // (a NaN passes, as in the reference)
                const double *fn = t_fn + 3 * (size_t)j;
                const float dist = (float)(fn[0] * (double)x + fn[1] * (double)y + fn[2]);
                if (fabsf(dist) < r) atomicMin(&rank[j], base + (unsigned)(k - k0));
            }
            base += (unsigned)max(k1 - k0, 0);
        }
    }
}

__global__ __launch_bounds__(64) void k_lsbp_keys(LsbpDev a)
{
    __shared__ unsigned rank[LSBP_MAXT];
    const int q = blockIdx.x, lane = threadIdx.x, nt = a.nt;
    for (int j = lane; j < nt; j += 64) rank[j] = 0xFFFFFFFFu;
    __syncthreads();
    lsbp_window(rank, a.q_xyxy + 4 * (size_t)q, a.th, 0.96f, a.cell_start, a.cell_items, a.n_items, a.t_kl, a.t_fn, nt, a.mnMinX, a.mnMaxX, a.mnMinY, a.mnMaxY, lane);
    __syncthreads();
    const int qi = a.q_index ? a.q_index[q] : q;
    const hvo_keyline ql = a.q_kl[qi];
    const ulonglong4 qd = *reinterpret_cast<const ulonglong4 *>(a.q_desc ? a.q_desc + 32 * (size_t)q : a.q_desc_all + 32 * (size_t)qi);
    unsigned long long *K = a.keys + (size_t)q * nt;
    for (int j = lane; j < nt; j += 64) {
        unsigned long long key = LSBP_NONE;
        const unsigned rk = rank[j];
        if (rk != 0xFFFFFFFFu) {
            const hvo_keyline t = a.t_kl[j];
            bool ok = !(lt_angle2d(t, ql) < a.cos_th);
            const float mx = ql.length < t.length ? t.length : ql.length, mn = t.length < ql.length ? t.length : ql.length;      // std::max(last, cur), std::min(last, cur)
            if ((double)(mn / mx) < 0.75) ok = false;
            if (ok) {
                const int d = ham256(qd, *reinterpret_cast<const ulonglong4 *>(a.t_desc + 32 * (size_t)j));
                key = ((unsigned long long)d << 40) | ((unsigned long long)(rk & 0xFFFFFFu) << 16) | (unsigned long long)j;
            }
        }
        K[j] = key;
    }
}

// the reference's loop over the queries, by one wave: occupancy bits in LDS, the smallest key among the free lines
__global__ __launch_bounds__(64) void k_lsbp_epilogue(LsbpDev a)
{
    __shared__ unsigned occ[LSBP_MAXT / 32];
    const int lane = threadIdx.x, nt = a.nt;
    for (int wd = lane; wd < LSBP_MAXT / 32; wd += 64) {
        unsigned m = 0;
        if (a.t_occ) for (int b = 0; b < 32; b++) { const int j = wd * 32 + b; if (j < nt && a.t_occ[j]) m |= 1u << b; }
        occ[wd] = m;
    }
    __syncthreads();
    int nm = 0;
    for (int q = 0; q < a.nq; q++) {
        const unsigned long long *K = a.keys + (size_t)q * nt;
        unsigned long long best = LSBP_NONE;
        for (int j = lane; j < nt; j += 64) {
            const unsigned long long k = K[j];
            if (k != LSBP_NONE && !((occ[j >> 5] >> (j & 31)) & 1u) && k < best) best = k;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long v = __shfl_xor(best, o); if (v < best) best = v; }
        const int d = best == LSBP_NONE ? 256 : (int)(best >> 40), j = (int)(best & 0xFFFFu);
        const bool acc = d <= 95;
        if (lane == 0) { a.match_idx[q] = acc ? j : -1; a.match_dist[q] = acc ? d : 256; }
        if (acc) {
            nm++;
            if (a.q_blocks && a.q_blocks[q] && lane == 0) occ[j >> 5] |= 1u << (j & 31);
        }
        __syncthreads();
    }
    if (lane == 0) *a.n_matches = nm;
}

size_t match_lsbp_scratch_bytes(int nq, int nt) { return AL((size_t)nq * (size_t)std::max(nt, 1), unsigned long long) + 64; }

// device-resident form: a.keys is carved from `scratch` (match_lsbp_scratch_bytes(nq, nt) bytes)
int match_lsbp_enqueue(hipStream_t st, LsbpDev a, void *scratch)
{
    if (a.nq < 1) return HVO_OK;
    if (a.nt > LSBP_MAXT || a.n_items >= (1 << 22)) return HVO_ERR_UNSUPPORTED;
    a.keys = (unsigned long long *)scratch;
    if (a.nt >= 1) hipLaunchKernelGGL(k_lsbp_keys, dim3(a.nq), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_lsbp_epilogue, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError() == hipSuccess ? HVO_OK : HVO_ERR_HIP;
}

// matchNNR + the gates, device-resident: m12 (n_last + 1 ints: the matches, then lmatches) and accepted (n_last bytes)
int match_lines_geom_enqueue(hipStream_t st, const uint8_t *d_last, const hvo_keyline *kl_last, const uint8_t *has_ml, int n_last,
                             const uint8_t *d_cur, const hvo_keyline *kl_cur, int n_cur, float desc_th, const float *bounds4,
                             void *scratch, int32_t *d_m12, uint8_t *d_acc)
{
    if (n_last < 1) return HVO_OK;
    int rc = match_lines_enqueue(st, d_last, n_last, d_cur, n_cur, 0.f, desc_th, 0, scratch, d_m12, d_m12 + n_last);
    if (rc) return rc;
    const double dW = (double)(bounds4[1] - bounds4[0]) * 0.1, dH = (double)(bounds4[3] - bounds4[2]) * 0.1;
    const double th_angle = 20.0, th_rad = th_angle / 180.0 * M_PI;
    hipLaunchKernelGGL(k_lines_geom_gate, dim3(1), dim3(256), 0, st, d_m12, kl_last, has_ml, n_last, kl_cur, dW, dH, cos(th_rad), d_acc, d_m12 + n_last);
    return hipGetLastError() == hipSuccess ? HVO_OK : HVO_ERR_HIP;
}

// host-array forms (hvo_match_lines_geom / hvo_search_lines_by_projection): stage, run, fetch
int match_lines_geom(hvo_ctx *ctx, const uint8_t *d_last, const hvo_keyline *kl_last, const uint8_t *has_ml, int n_last,
                     const uint8_t *d_cur, const hvo_keyline *kl_cur, int n_cur, float desc_th, const float *bounds4,
                     int32_t *m12, uint8_t *accepted, int *n_accepted)
{
    if (n_last > 65535 || n_cur > 65535) return HVO_ERR_UNSUPPORTED;
    const size_t sb = match_lines_scratch_bytes(n_last, n_cur);
    const size_t in_b = AL(n_last * 32, char) + AL(n_cur * 32, char) + AL(n_last, hvo_keyline) + AL(n_cur, hvo_keyline) + AL(n_last, char);
    const size_t out_b = AL(n_last + 1, int32_t) + AL(n_last, char);
    int rc = arena_begin(ctx, in_b + out_b + sb + 1024, in_b + out_b + 1024);
    if (rc) return rc;
    const uint8_t *a = arena_up(ctx, d_last, (size_t)n_last * 32), *b = arena_up(ctx, d_cur, (size_t)n_cur * 32), *hm = arena_up(ctx, has_ml, (size_t)n_last);
    const hvo_keyline *ka = arena_up(ctx, kl_last, (size_t)n_last), *kb = arena_up(ctx, kl_cur, (size_t)n_cur);
    void *scratch = arena_dev<char>(ctx, sb);
    int32_t *dm = arena_dev<int32_t>(ctx, (size_t)n_last + 1); uint8_t *da = arena_dev<uint8_t>(ctx, (size_t)n_last);
    int32_t *hmm = arena_host<int32_t>(ctx, (size_t)n_last + 1); uint8_t *ha = arena_host<uint8_t>(ctx, (size_t)n_last);
    // (fewer than two current lines: knnMatch(k = 2) has no second neighbour -- no matches, as hvo_match_nnr)
    HVO_HIP(hipMemsetAsync(dm, 0xFF, (size_t)n_last * 4, ctx->stream)); HVO_HIP(hipMemsetAsync(dm + n_last, 0, 4, ctx->stream)); HVO_HIP(hipMemsetAsync(da, 0, (size_t)n_last, ctx->stream));
    if (n_cur >= 2 && (rc = match_lines_geom_enqueue(ctx->stream, a, ka, hm, n_last, b, kb, n_cur, desc_th, bounds4, scratch, dm, da))) { ctx->last_error = "line matching launch"; return rc; }
    HVO_HIP(hipMemcpyAsync(hmm, dm, ((size_t)n_last + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HVO_HIP(hipMemcpyAsync(ha, da, (size_t)n_last, hipMemcpyDeviceToHost, ctx->stream));
    HVO_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(m12, hmm, (size_t)n_last * 4); memcpy(accepted, ha, (size_t)n_last);
    *n_accepted = hmm[n_last];
    return HVO_OK;
}

int match_search_lines_by_projection(hvo_ctx *ctx, int nq, const float *q_xyxy, const hvo_keyline *q_kl, const uint8_t *q_desc, const uint8_t *q_blocks,
                                     const hvo_keyline *t_kl, const double *t_linefn, const uint8_t *t_desc, const uint8_t *t_occupied, int nt,
                                     const int32_t *cell_start, const int32_t *cell_items, int n_items, const float *bounds4, float th,
                                     int32_t *match_idx, int32_t *match_dist, int *n_matches)
{
    if (nt > LSBP_MAXT || nq > 65535 || n_items >= (1 << 22)) { ctx->last_error = "guided line search: more than 2048 current lines, 65535 queries or 2^22 line grid items"; return HVO_ERR_UNSUPPORTED; }
    const int ncell = HVO_GRID_COLS * HVO_GRID_ROWS + 1;
    const size_t in_b = AL(nq * 4, float) + AL(nq, hvo_keyline) + AL(nq * 32, char) + AL(nq, char) + AL(nt, hvo_keyline) + AL(nt * 3, double) + AL(nt * 32, char) + AL(nt, char) +
                        AL(ncell, int32_t) + AL(n_items, int32_t);
    const size_t out_b = AL(2 * (size_t)nq + 1, int32_t), sb = match_lsbp_scratch_bytes(nq, nt);
    int rc = arena_begin(ctx, in_b + out_b + sb + 2048, in_b + out_b + 2048);
    if (rc) return rc;
    LsbpDev a; memset(&a, 0, sizeof(a));
    a.nq = nq; a.nt = nt;
    a.q_xyxy = arena_up(ctx, q_xyxy, (size_t)nq * 4); a.q_kl = arena_up(ctx, q_kl, (size_t)nq); a.q_index = nullptr;
    a.q_desc = arena_up(ctx, q_desc, (size_t)nq * 32); a.q_desc_all = nullptr; a.q_blocks = arena_up(ctx, q_blocks, (size_t)nq);
    a.t_kl = arena_up(ctx, t_kl, (size_t)nt); a.t_fn = arena_up(ctx, t_linefn, (size_t)nt * 3); a.t_desc = arena_up(ctx, t_desc, (size_t)nt * 32); a.t_occ = arena_up(ctx, t_occupied, (size_t)nt);
    a.cell_start = arena_up(ctx, cell_start, (size_t)ncell); a.cell_items = arena_up(ctx, cell_items, (size_t)n_items); a.n_items = n_items;
    a.mnMinX = bounds4[0]; a.mnMaxX = bounds4[1]; a.mnMinY = bounds4[2]; a.mnMaxY = bounds4[3]; a.th = th; a.cos_th = cos(10.0 / 180.0 * M_PI);
    int32_t *dout = arena_dev<int32_t>(ctx, 2 * (size_t)nq + 1), *hout = arena_host<int32_t>(ctx, 2 * (size_t)nq + 1);
    a.match_idx = dout; a.match_dist = dout + nq; a.n_matches = dout + 2 * nq;
    void *scratch = arena_dev<char>(ctx, sb);
    if ((rc = match_lsbp_enqueue(ctx->stream, a, scratch))) { ctx->last_error = "guided line search launch"; return rc; }
    HVO_HIP(hipMemcpyAsync(hout, dout, (2 * (size_t)nq + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HVO_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(match_idx, hout, (size_t)nq * sizeof(int32_t)); memcpy(match_dist, hout + nq, (size_t)nq * sizeof(int32_t));
    *n_matches = hout[2 * nq];
    return HVO_OK;
}
