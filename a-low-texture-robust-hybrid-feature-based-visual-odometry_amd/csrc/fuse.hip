// fuse.hip -- ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, float th) (reference src/ORBmatcher.cc:838-994), the
// matcher of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1567-1696), for n_kf key frames in one call with one synchronisation.
// With it: KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:627-666), KeyFrame::IsInImage (:780-783), MapPoint::PredictScale(dist, KeyFrame *)
// (src/MapPoint.cc:383-398).
//
// Fuse has no occupancy: an entry's best feature does not depend on what earlier entries took (pKF->GetMapPoint(bestIdx) is read after the
// search, to choose between Replace and AddObservation), so every (key frame, entry) pair is independent and one launch covers them all.
// The in-order pass of k_search_by_projection (match.hip) is not needed and is not used.
//
//   k_fuse_grid     one block per key frame: every feature's cell as Frame::PosInGrid computes it (round((x - mnMinX) * invW) on 64 x 48
//                   cells; a feature outside the grid is in no cell), a counting sort into a CSR that is STABLE in feature index and numbers
//                   the cells COLUMN-MAJOR (ix * 48 + iy).  GetFeaturesInArea visits ix outer, iy inner, then the cell's vector, which
//                   AssignFeaturesToGrid filled in index order: with this numbering that is ascending CSR position, and a query's cells of
//                   one ix are one contiguous run.  The record at a CSR position is (x, y, mvuRight or -1, octave); the feature index beside it.
//   k_fuse_project  one lane per (key frame, entry), blockIdx.y = key frame: the gates in the reference's order; u, v, ur, radius, level
//   k_fuse_search   16 lanes (a quarter wave) per entry: the lanes stride over the CSR runs of the window's columns; per candidate the two
//                   fabs tests, the level band [level - 1, level], the chi-square gate, the 256-bit Hamming distance against the entry's
//                   descriptor (kept in registers).  key = dist << 16 | CSR position, minimum over the group by shuffles: the strict
//                   `dist < bestDist` of the reference keeps the first of equal distances in visiting order = the lowest key.
//   k_fuse_compact  the entries with best_dist <= th_low in ascending entry order (sm_compact_pos: ballot + prefix per block, block offsets
//                   from the counts of the blocks before).  No atomic decides anything: integer atomics only count (cells, searched
//                   entries, fused entries per block).
//
// The key-frame side is host arrays (they go up) or a resident frame's arrays (FrameView: the stream form, one key frame).  The map side is
// host arrays, one set shared by all key frames or one per key frame (stored by component, so a wave's load is contiguous), or a list of
// slots of a resident hvo_point_map, whose device arrays are read in place.  Staging and scratch come from the context's call arena.
//
// Readings (OpenCV is not in the reference tree; DESIGN.md section 7, tests/fuse_ref.py restates the same):
//   Rcw * p3Dw + tcw       sm_row: the row's products summed in FLOAT left to right, then (float)((double)sum * 1.0 + (double)t * 1.0)
//   z < 0.0f               as written: z == 0 and -0.0 pass and divide
//   invz = 1 / z           ONE FLOAT division: the text has the int literal 1 (the siblings divide the double 1.0)
//   u = fx * x + cx        x = X * invz: two float products, NOT sm_pinhole (the siblings form fx * xc * invzc left to right)
//   IsInImage              u >= minX && u < maxX && v >= minY && v < maxY: a NaN FAILS (kf_search's four one-sided tests let it pass)
//   ur = u - bf * invz     float
//   Ow, p3Dw - Ow, norm    as kf_search: -Rcw^T tcw with double sums times -1.0 rounded to float; float difference; sm_dist3; the
//                          1.2 / 0.8 band is sm_dist_band
//   PO.dot(Pn)             cv::Mat::dot on CV_32F accumulates in double, in order; compared with the double 0.5 * dist3D
//   PredictScale           sm_predict_level, then sm_clamp_level (map_gates.hpp, shared with every sibling)
//   radius                 th * mvScaleFactors[level], a float product; the scale factors and mvInvLevelSigma2 are the context's
//   cell range             max(0, (int)floor((u - minX - r) * invW)) .. min(cols - 1, (int)ceil((u - minX + r) * invW)) with the four early
//                          returns, applied as written IN ADDITION to the fabs tests (float rounding can make the two disagree by a cell)
//   e2                     float, left to right; e2 * mvInvLevelSigma2[octave] a float product compared with the DOUBLE literals 7.8 / 5.99;
//                          mvuRight[idx] >= 0 chooses the gate (a NaN there takes the mono gate)
//   octave < 0             in no band (the reference would index mvInvLevelSigma2[-1] at level 0)
// No contraction (-ffp-contract=off, __f*_rn, __d*_rn).
#include "slot_map.hpp"
#include "frame_view.hpp"
#include "staged_call.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#define FU_BLOCK SM_BLOCK
#define FU_GROUP 16               // lanes per entry in the search
#define FU_MAXT 65535             // features per key frame (the search key holds the CSR position in 16 bits)
#define FU_MAXQ (1 << 20)         // entries per key frame
#define FU_MAXTOTAL (1 << 24)     // padded entries of all key frames of one call
#define FU_COLS 64
#define FU_ROWS 48
#define FU_CELLS (FU_COLS * FU_ROWS)
#define FU_NOKEY ((256u << 16) | 0xFFFFu)

struct FuKf { float R[9], t[3], Ow[3]; int n_feat, n_ent; const hvo_keypoint *kp; const float *ur; const uint8_t *desc; };
struct FuDev {
    const FuKf *kf; int cq, ct, n_levels, per_kf, nb;               // entry stride (a multiple of FU_BLOCK), feature stride, blocks of FU_BLOCK entries
    // the map side: arrays (component c of map side s at (3 s + c) * cq + i) or slots of a point map (component c of slot k at c * cstride + k)
    const float *pos, *nrm, *maxd, *mind; const uint8_t *mdesc, *flags; const int32_t *slots; size_t cstride;
    const uint8_t *skip; const float *tab;                           // tab: mvScaleFactors[16] then mvInvLevelSigma2[16]
    float fx, fy, cx, cy, bf, minX, maxX, minY, maxY, invW, invH, logsf, th; int th_low;
    int *cstart; float4 *rec; int32_t *item;                         // per key frame: FU_CELLS + 1 starts; ct records and feature indices in CSR order
    float *q_u, *q_v, *q_ur, *q_rad;
    float *proj; int32_t *level; int8_t *gate; int32_t *bi, *bd, *fe, *fi; uint8_t *pass; int *blockcnt, *nsearched, *nfused;
};

// Frame::PosInGrid (src/Frame.cc:1680-1690) -> ix * 48 + iy, or -1 (outside the grid; a NaN is outside)
static __device__ __forceinline__ int fu_cell(const FuDev &a, float x, float y)
{
    const float px = roundf(__fmul_rn(__fsub_rn(x, a.minX), a.invW)), py = roundf(__fmul_rn(__fsub_rn(y, a.minY), a.invH));
    if (!(px >= 0.f && px < (float)FU_COLS && py >= 0.f && py < (float)FU_ROWS)) return -1;
    return (int)px * FU_ROWS + (int)py;
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_grid(FuDev a)
{
    __shared__ int cnt[FU_CELLS];                                  // the cells' counts, then where each cell's next feature goes
    __shared__ int part[FU_BLOCK];
    __shared__ unsigned short cc[FU_BLOCK];
    const int j = blockIdx.x, tid = threadIdx.x;
    const FuKf &k = a.kf[j];
    const int n = k.n_feat;
    int *start = a.cstart + (size_t)j * (FU_CELLS + 1);
    float4 *rec = a.rec + (size_t)j * a.ct; int32_t *item = a.item + (size_t)j * a.ct;
    for (int c = tid; c < FU_CELLS; c += FU_BLOCK) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += FU_BLOCK) {
        const int c = fu_cell(a, k.kp[i].x, k.kp[i].y);
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan: lane t owns the cells [12 t, 12 t + 12)
    constexpr int PER = FU_CELLS / FU_BLOCK;
    int s = 0;
    for (int q = 0; q < PER; q++) s += cnt[PER * tid + q];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < FU_BLOCK; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int q = 0; q < PER; q++) { const int c = PER * tid + q, v = cnt[c]; cnt[c] = run; start[c] = run; run += v; }
    if (tid == FU_BLOCK - 1) start[FU_CELLS] = run;
    __syncthreads();
    // placement, stable in feature index: chunks of FU_BLOCK features in index order; inside a chunk a feature's place is its cell's next
    // position plus the chunk's lower-indexed features of the same cell
    for (int base = 0; base < n; base += FU_BLOCK) {
        const int i = base + tid;
        float x = 0.f, y = 0.f; int oct = 0;
        if (i < n) { x = k.kp[i].x; y = k.kp[i].y; oct = k.kp[i].octave; }
        const int c = i < n ? fu_cell(a, x, y) : -1;
        cc[tid] = (unsigned short)(c < 0 ? 0xFFFF : c);
        __syncthreads();
        int before = 0, total = 0;
        if (c >= 0) {
            const unsigned short me = (unsigned short)c;
            for (int q = 0; q < FU_BLOCK; q++) { const bool e = cc[q] == me; total += e ? 1 : 0; before += (e && q < tid) ? 1 : 0; }
            const int p = cnt[c] + before;                           // < n <= ct
            rec[p] = make_float4(x, y, k.ur ? k.ur[i] : -1.0f, __int_as_float(oct));
            item[p] = i;
        }
        __syncthreads();
        if (c >= 0 && before == 0) cnt[c] += total;                  // one lane per cell of the chunk
        __syncthreads();
    }
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_project(FuDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * FU_BLOCK + threadIdx.x;
    const FuKf &k = a.kf[j];
    const bool in = i < k.n_ent;
    const size_t cq = (size_t)a.cq, o = (size_t)j * cq + (in ? (size_t)i : 0);
    int g = HVO_FUSE_GATE_SKIP, lvl = -1;
    float u = 0.f, v = 0.f, ur = 0.f, radius = 0.f;
    if (in) {
        const size_t mb = a.per_kf ? (size_t)j : 0;
        const size_t e = a.slots ? (size_t)a.slots[i] : mb * cq + (size_t)i;               // the entry's scalars; its components start at p
        const size_t p = a.slots ? e : mb * 3 * cq + (size_t)i;
        const bool skip = a.skip[o] || (a.flags && (a.flags[e] & SM_BAD));
        if (!skip) {
            const float X = a.pos[p], Y = a.pos[p + a.cstride], Z = a.pos[p + 2 * a.cstride];
            const float xc = sm_row(k.R, X, Y, Z, k.t[0]), yc = sm_row(k.R + 3, X, Y, Z, k.t[1]), zc = sm_row(k.R + 6, X, Y, Z, k.t[2]);
            g = HVO_FUSE_GATE_BEHIND;
            if (!(zc < 0.0f)) {                                     // ORBmatcher.cc:869
                const float invz = __fdiv_rn(1.0f, zc);             // :872, the int literal 1: a float division
                const float x = __fmul_rn(xc, invz), y = __fmul_rn(yc, invz);
                u = __fadd_rn(__fmul_rn(a.fx, x), a.cx); v = __fadd_rn(__fmul_rn(a.fy, y), a.cy);
                g = HVO_FUSE_GATE_OUT_OF_IMAGE;
                if (u >= a.minX && u < a.maxX && v >= a.minY && v < a.maxY) {          // KeyFrame::IsInImage: a NaN fails
                    ur = __fsub_rn(u, __fmul_rn(a.bf, invz));
                    const float mfMax = a.maxd[e]; float maxD, minD; sm_dist_band(mfMax, a.mind[e], &maxD, &minD);
                    const double d0 = __fsub_rn(X, k.Ow[0]), d1 = __fsub_rn(Y, k.Ow[1]), d2 = __fsub_rn(Z, k.Ow[2]);
                    const float dist = sm_dist3(d0, d1, d2);
                    g = dist < minD ? HVO_FUSE_GATE_DIST_MIN : dist > maxD ? HVO_FUSE_GATE_DIST_MAX : 0;
                    if (g == 0) {
                        const double n0 = a.nrm[p], n1 = a.nrm[p + a.cstride], n2 = a.nrm[p + 2 * a.cstride];
                        const double dot = __dadd_rn(__dadd_rn(__dmul_rn(d0, n0), __dmul_rn(d1, n1)), __dmul_rn(d2, n2));
                        if (dot < __dmul_rn(0.5, (double)dist)) g = HVO_FUSE_GATE_VIEW_ANGLE;          // :897
                        else {
                            lvl = sm_clamp_level(sm_predict_level(mfMax, dist, a.logsf), a.n_levels);           // MapPoint.cc:383-398
                            radius = __fmul_rn(a.th, a.tab[lvl]);
                        }
                    }
                }
            }
        }
    }
    if (in) {
        a.q_u[o] = u; a.q_v[o] = v; a.q_ur[o] = ur; a.q_rad[o] = radius;
        a.proj[3 * o] = u; a.proj[3 * o + 1] = v; a.proj[3 * o + 2] = ur; a.level[o] = lvl; a.gate[o] = (int8_t)g;
        a.bi[o] = -1; a.bd[o] = 256;
    }
    const unsigned long long s = __ballot(in && g == 0);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&a.nsearched[j], __popcll(s));
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_search(FuDev a)
{
    const int j = blockIdx.y, sub = threadIdx.x & (FU_GROUP - 1);
    const int i = blockIdx.x * (FU_BLOCK / FU_GROUP) + (threadIdx.x / FU_GROUP);
    const FuKf &k = a.kf[j];
    if (i >= k.n_ent) return;                                        // (a whole group leaves together: the shuffles below stay inside a group)
    const size_t o = (size_t)j * a.cq + (size_t)i;
    if (a.gate[o] != 0) return;
    const float u = a.q_u[o], v = a.q_v[o], ur = a.q_ur[o], r = a.q_rad[o];
    const int lvl = a.level[o], lo = lvl > 0 ? lvl - 1 : 0;
    // KeyFrame::GetFeaturesInArea's cell range, as written (KeyFrame.cc:632-646)
    const float du = __fsub_rn(u, a.minX), dv = __fsub_rn(v, a.minY);
    int x0 = sm_level(floorf(__fmul_rn(__fsub_rn(du, r), a.invW))), x1 = sm_level(ceilf(__fmul_rn(__fadd_rn(du, r), a.invW)));
    int y0 = sm_level(floorf(__fmul_rn(__fsub_rn(dv, r), a.invH))), y1 = sm_level(ceilf(__fmul_rn(__fadd_rn(dv, r), a.invH)));
    x0 = x0 < 0 ? 0 : x0; x1 = x1 > FU_COLS - 1 ? FU_COLS - 1 : x1; y0 = y0 < 0 ? 0 : y0; y1 = y1 > FU_ROWS - 1 ? FU_ROWS - 1 : y1;
    if (x0 >= FU_COLS || x1 < 0 || y0 >= FU_ROWS || y1 < 0) return;  // vIndices.empty(): bestIdx stays -1
    const size_t e = a.slots ? (size_t)a.slots[i] : (a.per_kf ? (size_t)j * a.cq : 0) + (size_t)i;
    const ulonglong4 qd = ld256(a.mdesc + e * 32);
    const int *start = a.cstart + (size_t)j * (FU_CELLS + 1);
    const float4 *rec = a.rec + (size_t)j * a.ct; const int32_t *item = a.item + (size_t)j * a.ct;
    const float *isig = a.tab + HVO_MAX_LEVELS;
    unsigned best = FU_NOKEY;
    for (int ix = x0; ix <= x1; ix++) {
        const int p0 = start[ix * FU_ROWS + y0], p1 = start[ix * FU_ROWS + y1 + 1];     // y1 + 1 <= 48: the last index is FU_CELLS
        for (int p = p0 + sub; p < p1; p += FU_GROUP) {
            const float4 f = rec[p];
            if (!(fabsf(__fsub_rn(f.x, u)) < r && fabsf(__fsub_rn(f.y, v)) < r)) continue;    // KeyFrame.cc:656-659
            const int oct = __float_as_int(f.w);
            if (oct < lo || oct > lvl) continue;                     // ORBmatcher.cc:924
            const float ex = __fsub_rn(u, f.x), ey = __fsub_rn(v, f.y);
            float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
            double lim = 5.99;
            if (f.z >= 0.f) { const float er = __fsub_rn(ur, f.z); e2 = __fadd_rn(e2, __fmul_rn(er, er)); lim = 7.8; }
            if ((double)__fmul_rn(e2, isig[oct]) > lim) continue;    // :938, :949
            const unsigned dist = ham256(qd, ld256(k.desc + (size_t)item[p] * 32));
            const unsigned key = (dist << 16) | (unsigned)p;
            best = key < best ? key : best;
        }
    }
    for (int w = FU_GROUP / 2; w > 0; w >>= 1) { const unsigned other = (unsigned)__shfl_xor((int)best, w); best = other < best ? other : best; }
    if (sub == 0) {
        const int bd = (int)(best >> 16);
        if (bd < 256) { a.bi[o] = item[best & 0xFFFFu]; a.bd[o] = bd; }      // 256 never enters (dist < bestDist, bestDist = 256)
        if (bd <= a.th_low) { a.pass[o] = 1; atomicAdd(&a.blockcnt[(size_t)j * a.nb + (i / FU_BLOCK)], 1); }
    }
}

__global__ __launch_bounds__(FU_BLOCK) void k_fuse_compact(FuDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * FU_BLOCK + threadIdx.x;
    bool p;
    const int at = sm_compact_pos(a.blockcnt, a.nb, a.cq, j, a.pass, a.nfused, &p);
    if (p) { const size_t q0 = (size_t)j * a.cq; a.fe[q0 + at] = i; a.fi[q0 + at] = a.bi[q0 + i]; }
}

// what fuse_run serves: the key-frame side (host arrays kf[j], or the one resident frame fr with kf[0]'s Tcw and skip), the map side
// (host arrays maps[0] shared / maps[j], or n_slots slots of m)
static int fuse_run(hvo_ctx *ctx, hipStream_t st, const hvo_camera *cam, const hvo_fuse_params *P, const float bounds[4], const FrameView *fr,
             int n_kf, const hvo_fuse_keyframe *kf, const hvo_fuse_map *maps, hvo_point_map *m, int n_slots, const int32_t *slots,
             hvo_fuse_result *res, std::string *err)
{
    const bool per_kf = !m && P->map_per_keyframe != 0;
    // ---- refusals: whole, before anything is written ----
    if (P->th_low > 255) { *err = "fuse: th_low above 255 (bestDist starts at 256: the reference would accept bestIdx = -1)"; return HVO_ERR_INVALID_ARG; }
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { *err = "fuse: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) { *err = "fuse: empty image bounds"; return HVO_ERR_INVALID_ARG; }
    if (m) {
        if (P->map_per_keyframe) { *err = "fuse: the slot form has one slot list for all key frames (map_per_keyframe must be 0)"; return HVO_ERR_INVALID_ARG; }
        if (m->device != ctx->device) { *err = "fuse: the point map lives on another device"; return HVO_ERR_INVALID_ARG; }
        if (n_slots < 0 || (n_slots > 0 && !slots)) { *err = "fuse: n < 0 or no slot list"; return HVO_ERR_INVALID_ARG; }
        for (int i = 0; i < n_slots; i++) if (slots[i] < 0 || slots[i] >= m->n_slots) {
            *err = "fuse: entry " + std::to_string(i) + " names slot " + std::to_string(slots[i]) + " outside the map's " + std::to_string(m->n_slots) + " slots; nothing was written";
            return HVO_ERR_INVALID_ARG;
        }
    } else {
        for (int s = 0; s < (per_kf ? n_kf : 1); s++) {
            const hvo_fuse_map &M = maps[s];
            if (M.n < 0 || (M.n > 0 && (!M.pos || !M.normal || !M.max_dist || !M.min_dist || !M.desc))) { *err = "fuse: a map side with n < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
        }
    }
    int nmax = 0, tmax = 0;
    std::vector<int> n_ent((size_t)n_kf), n_feat((size_t)n_kf);
    for (int j = 0; j < n_kf; j++) {
        n_ent[j] = m ? n_slots : maps[per_kf ? j : 0].n;
        n_feat[j] = fr ? fr->n_kp : kf[j].n;
        if (n_feat[j] < 0 || (!fr && n_feat[j] > 0 && (!kf[j].kp_un || !kf[j].desc))) { *err = "fuse: a key frame with n < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
        if (!res[j].best_idx) { *err = "fuse: a result without best_idx"; return HVO_ERR_INVALID_ARG; }
        nmax = std::max(nmax, n_ent[j]); tmax = std::max(tmax, n_feat[j]);
    }
    const size_t cq = (size_t)std::max(FU_BLOCK, (nmax + FU_BLOCK - 1) / FU_BLOCK * FU_BLOCK), ct = (size_t)std::max(64, (tmax + 63) & ~63), F = (size_t)n_kf;
    if (tmax > FU_MAXT || nmax > FU_MAXQ || F * cq > FU_MAXTOTAL) {
        *err = "fuse: " + std::to_string(nmax) + " entries, " + std::to_string(tmax) + " features per key frame, " + std::to_string(F * cq) + " padded entries in all (limits: " +
               std::to_string(FU_MAXQ) + ", " + std::to_string(FU_MAXT) + ", " + std::to_string(FU_MAXTOTAL) + "); nothing was written";
        return HVO_ERR_UNSUPPORTED;
    }
    // ---- one carve of the context's arena: what goes up, the grid, the queries, what comes down ----
    const size_t S = m ? 0 : (per_kf ? F : 1), nb = cq / FU_BLOCK;
    StageCarver C(256);
    const size_t Fh = fr ? 0 : F;                                    // key-frame sides that go up
    const auto u_kf = C.take<FuKf>(F); const auto u_tab = C.take<float>(2 * HVO_MAX_LEVELS); const auto u_skip = C.take<uint8_t>(F, cq);
    const auto u_kp = C.take<hvo_keypoint>(Fh, ct); const auto u_ur = C.take<float>(Fh, ct); const auto u_fd = C.take<uint8_t>(Fh, ct * 32);
    const auto u_pos = C.take<float>(3 * S, cq), u_nrm = C.take<float>(3 * S, cq), u_maxd = C.take<float>(S, cq), u_mind = C.take<float>(S, cq);      // pos, nrm by component: row 3 s + q
    const auto u_md = C.take<uint8_t>(S, cq * 32); const auto u_slots = C.take<int32_t>(m ? cq : 0);
    const size_t up_end = C.mark();
    const auto g_start = C.take<int>(F, FU_CELLS + 1); const auto g_rec = C.take<float4>(F, ct); const auto g_item = C.take<int32_t>(F, ct);
    const auto q_u = C.take<float>(F, cq), q_v = C.take<float>(F, cq), q_ur = C.take<float>(F, cq), q_rad = C.take<float>(F, cq);
    const size_t z0 = C.mark();                                      // [z0, z1) is zeroed
    const auto s_pass = C.take<uint8_t>(F, cq); const auto s_bc = C.take<int>(F, nb);
    const size_t r0 = C.mark();                                      // [r0, r1) comes down; its head belongs to the zeroed range
    const auto r_cnt = C.take<int>(2, F);                            // row 0: searched, row 1: fused
    const size_t z1 = C.mark();
    const auto r_bi = C.take<int32_t>(F, cq), r_bd = C.take<int32_t>(F, cq), r_lvl = C.take<int32_t>(F, cq);
    const auto r_proj = C.take<float>(F, cq * 3); const auto r_gate = C.take<int8_t>(F, cq);
    const auto r_fe = C.take<int32_t>(F, cq), r_fi = C.take<int32_t>(F, cq);
    const size_t r1 = C.mark();
    StagedCall sc(ctx, st, "fuse: ", err); int rc;
    if ((rc = sc.begin(C.mark(), up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    float *tab = u_tab.host(h);
    for (int l = 0; l < HVO_MAX_LEVELS; l++) tab[l] = fr ? fr->sf[l] : ctx->scale[l];
    frame_level_sigma2(fr ? fr->ctx : ctx, nullptr, tab + HVO_MAX_LEVELS);
    for (int j = 0; j < n_kf; j++) {
        const hvo_fuse_keyframe &K = kf[j];
        FuKf &c = *u_kf.host(h, j);
        pose_split(K.Tcw, c.R, c.t, c.Ow);                         // Ow = -Rcw^T tcw (match_project_setup's twc)
        c.n_feat = n_feat[j]; c.n_ent = n_ent[j];
        if (fr) { c.kp = fr->kp_un; c.ur = fr->uright; c.desc = fr->desc; }
        else {
            const size_t nf = (size_t)n_feat[j];
            c.kp = u_kp.dev(d, j); c.ur = K.uright ? u_ur.dev(d, j) : nullptr; c.desc = u_fd.dev(d, j);
            if (nf) {
                memcpy(u_kp.host(h, j), K.kp_un, nf * sizeof(hvo_keypoint)); memcpy(u_fd.host(h, j), K.desc, nf * 32);
                if (K.uright) memcpy(u_ur.host(h, j), K.uright, nf * 4);
            }
        }
        if (K.skip && n_ent[j]) memcpy(u_skip.host(h, j), K.skip, (size_t)n_ent[j]);
    }
    for (size_t s = 0; s < S; s++) {
        const hvo_fuse_map &M = maps[s];
        const size_t n = (size_t)M.n;
        float *const hp[3] = { u_pos.host(h, 3 * s), u_pos.host(h, 3 * s + 1), u_pos.host(h, 3 * s + 2) };
        float *const hn[3] = { u_nrm.host(h, 3 * s), u_nrm.host(h, 3 * s + 1), u_nrm.host(h, 3 * s + 2) };
        for (size_t i = 0; i < n; i++) for (int q = 0; q < 3; q++) { hp[q][i] = M.pos[3 * i + q]; hn[q][i] = M.normal[3 * i + q]; }     // by component
        if (n) { memcpy(u_maxd.host(h, s), M.max_dist, n * 4); memcpy(u_mind.host(h, s), M.min_dist, n * 4); memcpy(u_md.host(h, s), M.desc, n * 32); }
    }
    if (m && n_slots) memcpy(u_slots.host(h), slots, (size_t)n_slots * 4);
    if ((rc = sc.up(0, up_end)) || (rc = sc.clear(z0, z1))) return rc;
    sc.tick();
    FuDev a; memset(&a, 0, sizeof(a));
    a.kf = u_kf.dev(d); a.cq = (int)cq; a.ct = (int)ct; a.n_levels = P->n_levels; a.per_kf = per_kf ? 1 : 0; a.nb = (int)nb;
    if (m) {
        a.pos = m->dev<float>(m->POS); a.nrm = m->dev<float>(m->NRM); a.maxd = m->dev<float>(m->MAXD); a.mind = m->dev<float>(m->MIND); a.mdesc = m->dev<uint8_t>(m->DESC);
        a.flags = m->d_flags(); a.slots = u_slots.dev(d); a.cstride = (size_t)m->cap;
    } else {
        a.pos = u_pos.dev(d); a.nrm = u_nrm.dev(d); a.maxd = u_maxd.dev(d); a.mind = u_mind.dev(d);
        a.mdesc = u_md.dev(d); a.cstride = cq;
    }
    a.skip = u_skip.dev(d); a.tab = u_tab.dev(d);
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.bf = P->bf;
    a.minX = bounds[0]; a.maxX = bounds[1]; a.minY = bounds[2]; a.maxY = bounds[3];
    a.invW = (float)FU_COLS / (bounds[1] - bounds[0]); a.invH = (float)FU_ROWS / (bounds[3] - bounds[2]);      // mfGridElementWidthInv / HeightInv (Frame.cc:184-185)
    a.logsf = P->log_scale_factor; a.th = P->th; a.th_low = P->th_low;
    a.cstart = g_start.dev(d); a.rec = g_rec.dev(d); a.item = g_item.dev(d);
    a.q_u = q_u.dev(d); a.q_v = q_v.dev(d); a.q_ur = q_ur.dev(d); a.q_rad = q_rad.dev(d);
    a.proj = r_proj.dev(d); a.level = r_lvl.dev(d); a.gate = r_gate.dev(d); a.bi = r_bi.dev(d); a.bd = r_bd.dev(d);
    a.fe = r_fe.dev(d); a.fi = r_fi.dev(d); a.pass = s_pass.dev(d); a.blockcnt = s_bc.dev(d);
    a.nsearched = r_cnt.dev(d, 0); a.nfused = r_cnt.dev(d, 1);
    hipLaunchKernelGGL(k_fuse_grid, dim3(n_kf), dim3(FU_BLOCK), 0, st, a);
    sc.tick();
    hipLaunchKernelGGL(k_fuse_project, dim3((unsigned)nb, n_kf), dim3(FU_BLOCK), 0, st, a);
    sc.tick();
    if (nmax > 0 && tmax > 0) hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)(cq / (FU_BLOCK / FU_GROUP)), n_kf), dim3(FU_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_fuse_compact, dim3((unsigned)nb, n_kf), dim3(FU_BLOCK), 0, st, a);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    for (int j = 0; j < n_kf; j++) {
        hvo_fuse_result &R = res[j];
        const size_t n = (size_t)n_ent[j];
        R.n_searched = r_cnt.down(b, 0)[j]; R.n_fused = r_cnt.down(b, 1)[j]; R.status = HVO_OK;
        for (int i = 0; i < 3; i++) R.kernel_ms[i] = sc.ms[i];
        if (!n) continue;
        memcpy(R.best_idx, r_bi.down(b, j), n * 4);
        if (R.best_dist) memcpy(R.best_dist, r_bd.down(b, j), n * 4);
        if (R.gate) memcpy(R.gate, r_gate.down(b, j), n);
        if (R.level) memcpy(R.level, r_lvl.down(b, j), n * 4);
        if (R.proj) memcpy(R.proj, r_proj.down(b, j), n * 12);
        const size_t nf = (size_t)std::max(0, std::min(R.n_fused, (int32_t)n));
        if (R.fused_entry) memcpy(R.fused_entry, r_fe.down(b, j), nf * 4);
        if (R.fused_idx) memcpy(R.fused_idx, r_fi.down(b, j), nf * 4);
    }
    return HVO_OK;
}

extern "C" {

int hvo_fuse_points(hvo_ctx *ctx, const hvo_camera *cam, const hvo_fuse_params *params, const hvo_fuse_map *map_side,
                    int n_kf, const hvo_fuse_keyframe *keyframes, hvo_fuse_result *results)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !map_side || !keyframes || !results || n_kf < 1) { ctx->last_error = "fuse: a null argument or n_kf < 1"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return fuse_run(ctx, ctx->stream, cam, params, params->bounds, nullptr, n_kf, keyframes, map_side, nullptr, 0, nullptr, results, &ctx->last_error);
}

int hvo_fuse_points_slots(hvo_ctx *ctx, hvo_point_map *m, int n, const int32_t *slots, const hvo_camera *cam, const hvo_fuse_params *params,
                          int n_kf, const hvo_fuse_keyframe *keyframes, hvo_fuse_result *results)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!m || !cam || !params || !keyframes || !results || n_kf < 1) { ctx->last_error = "fuse: a null argument or n_kf < 1"; if (m) m->last_error = ctx->last_error; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const int rc = fuse_run(ctx, ctx->stream, cam, params, params->bounds, nullptr, n_kf, keyframes, nullptr, m, n, slots, results, &ctx->last_error);
    if (rc) m->last_error = ctx->last_error;
    return rc;
}

int hvo_stream_fuse_points(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_fuse_params *params, const float Tcw[12], const uint8_t *skip,
                           const hvo_fuse_map *map_side, hvo_point_map *m, int n, const int32_t *slots, hvo_fuse_result *result)
{
    if (!s) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !Tcw || !result || (!map_side && !m)) { s->last_error = "fuse: a null argument or no map side"; return HVO_ERR_INVALID_ARG; }
    FrameView B; int rc;
    if ((rc = stream_view(s, cur, need_fuse, s->s_match, B))) return rc;
    hvo_fuse_keyframe K; memset(&K, 0, sizeof(K));
    memcpy(K.Tcw, Tcw, sizeof(K.Tcw)); K.skip = skip;
    hvo_fuse_params P = *params; P.map_per_keyframe = 0;
    rc = fuse_run(B.ctx, s->s_match, cam, &P, B.bounds, &B, 1, &K, map_side, map_side ? nullptr : m, n, slots, result, &s->last_error);
    if (rc && !map_side) m->last_error = s->last_error;
    return rc;
}

}   // extern "C"
