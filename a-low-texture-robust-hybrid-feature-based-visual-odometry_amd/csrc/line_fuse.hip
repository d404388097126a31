// line_fuse.hip -- LSDmatcher::Fuse(KeyFrame *pKF, const vector<MapLine *> &vpMapLines, float th) (reference src/LSDmatcher.cpp:1297-1434), the
// line matcher of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1651, :1677), for n_kf key frames in one call with one synchronisation.
// With it: KeyFrame::GetLinesInArea (src/KeyFrame.cc:668-702), KeyFrame::IsInImage, MapLine::PredictScale (src/MapLine.cpp:549-558).
// A staged call (staged_call.hpp) with one StageCarver layout.
//
// As in ORBmatcher::Fuse there is no occupancy: pKF->GetMapLine(bestIdx) is read after the search, so every (key frame, entry) pair is
// independent.  GetLinesInArea has no grid: it tests EVERY key line of the key frame for every entry, so the work is
// key frames x entries x lines and the search is a sweep, not a window walk.
//
//   k_lf_lines     one lane per (key frame, key line): the record GetLinesInArea needs of a line: its mid-point keyline.pt, its unit direction
//                  (start - end, normalised in float with the float sqrt: the operations of KeyFrame.cc:688-692 in their order, once per key
//                  frame instead of once per entry) and its octave
//   k_lf_project   one lane per (key frame, entry), blockIdx.y = key frame: the gates in the reference's order; u1 v1 u2 v2, level, radius
//   k_lf_search    16 lanes per searched entry: the key frame's records go through LDS in chunks of 256, the 16 groups of a block sweep each
//                  chunk (lane s of a group takes the records s, s + 16, ...); the entry's descriptor stays in registers; a candidate's 32
//                  bytes are gathered only after the mid-point gate, the cosine gate, the band and the row bound have passed.
//                  key = dist << 16 | line index, minimum over the group by shuffles: the strict `dist < bestDist` in ascending line index
//                  keeps the lowest index among equal distances = the lowest key
//   k_lf_count     per block of 256 entries: the fused flags (best_dist <= th_low), the behind flags, and the three counts
//   k_lf_compact   the fused entries and the behind entries in ascending order (sm_compact_pos), blockIdx.z chooses the list
// No atomic is used.  Every byte a kernel reads was written by the upload or by an earlier kernel of the call: nothing is cleared.
//
// THE READINGS (include/hvo.h, DESIGN.md section 7 and tests/line_fuse_ref.py state the same):
//   1. Which descriptors.  The text compares the map line's LBD descriptor with pKF->mDescriptors.row(idx): ORB rows under a line index
//      (it fetches mLineDescriptors into lineDesc and never uses it).  The call takes "the rows the candidates are compared with" as
//      n_desc_rows x 32 bytes per key frame: mLineDescriptors (the intended reading) or mDescriptors (as written).  A candidate
//      idx >= n_desc_rows is not compared (the reference would read past the matrix).  There is no flag.
//   2. The predicted level.  MapLine::PredictScale is ceil(log(mfMaxDistance / dist) / logScaleFactor), unclamped, and indexes
//      mvScaleFactorsLine.  HVO_LF_LEVEL_CLAMPED (default) clamps to [0, n_levels - 1] before the radius and the band, as
//      MapPoint::PredictScale does; HVO_LF_LEVEL_AS_WRITTEN keeps it, and an entry whose level is outside [0, n_levels) gets
//      HVO_LF_GATE_LEVEL and is not searched.  log_scale_factor is a parameter of its own (the reference passes the ORB factor's log);
//      the table is sf[0] = 1, sf[l] = sf[l - 1] * scale_factor in float.
//   3. `return false` on a negative depth (:1340-1341) stops the reference's call at the first entry that is still not skipped and lies
//      behind.  Which entry that is depends on the walk (a Replace can turn a later entry into a skipped one), so the device applies no
//      stop: every entry is evaluated, such an entry reports HVO_LF_GATE_BEHIND, and behind_entry / n_behind list them in ascending
//      order.  hvo::LSDmatcher::walkFused applies the stop (stop_on_behind) or not.
// Kept as written: the entry order (!pML and isBad() || IsInKeyFrame are the caller's skip byte, then both depths); IsInImage(u1, v1)
// before u2, v2 are computed, a NaN fails; the two distance gates (two codes); the double 0.5 * dist of the angle gate; the band
// [level - 1, level] on kl.octave (an octave of -1 is inside it at level 0); an empty vIndices is no match; strict `<`; bestDist <= th_low.
// Arithmetic: Mat_<float> << double rounds to float; Rcw * SP + tcw is sm_row (tests/fuse_ref.py: point_map_ref.transform); invz = 1.0f / z
// is one float division and u = fx * X * invz + cx is sm_pinhole (the literal is 1.0f here, and the products are not regrouped);
// 0.5 * (SP + EP) is f32(SP * 0.5 + EP * 0.5) with the products and the sum in double (tests/map_refresh_ref.py), minus Ow in float;
// cv::norm is sm_dist3, the band sm_dist_band, and Mat::dot accumulates in double (tests/fuse_ref.py);
// PredictScale is sm_predict_level, clamped by sm_clamp_level or gated as written (reading 2); the Hamming distance is ham256 (map_gates.hpp).
// Inside GetLinesInArea: the mid-point distance is formed in double (0.5 * (x1 + x2) has a double literal; x1 + x2 is a float sum) and
// rounded to the float `distance`; it is compared with the float product r * r with `>`; CosSita = fabsf of the float sum of two float
// products; `CosSita < 0.998f` continues, so a NaN (a projected or stored line of zero length) PASSES.  Nothing is contracted.
#include "hvo_internal.hpp"
#include "slot_map.hpp"
#include "frame_view.hpp"
#include "staged_call.hpp"
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#define LF_BLOCK SM_BLOCK
#define LF_GROUP 16                 // lanes per entry in the search
#define LF_CHUNK 256                // records per LDS chunk
#define LF_MAXL 2048                // lines per key frame
#define LF_MAXQ 65536               // entries per key frame
#define LF_MAXTOTAL (1 << 24)       // padded (key frame, entry) pairs of one call
#define LF_NOKEY ((256u << 16) | 0xFFFFu)

struct LfKf { float R[9], t[3], Ow[3], fx, fy, cx, cy, minX, maxX, minY, maxY; int n_lines, n_ent, n_rows; const hvo_keyline *kl; const uint8_t *desc; };
struct LfDev {
    const LfKf *kf; int cq, ct, n_levels, per_kf, nb, as_written;  // entry stride (a multiple of LF_BLOCK), line stride, blocks of LF_BLOCK entries
    // the map side: arrays (component c of map side s at (6 s + c) * cq + i; the normal's at (3 s + c) * cq + i) or slots of a line map
    // (component c of slot k at c * cstride + k)
    const double *pos, *nrm; const float *maxd, *mind; const uint8_t *mdesc, *flags; const int32_t *slots; size_t cstride;
    const uint8_t *skip; const float *tab;                          // tab: mvScaleFactorsLine
    float logsf, th; int th_low;
    float4 *rec; int32_t *oct; float *rad;                          // per key frame: ct records (pt.x, pt.y, unit direction) and octaves; per entry: the radius
    float *proj; int32_t *level; int8_t *gate; int32_t *bi, *bd, *fe, *fi, *be; uint8_t *passF, *passB; int *bcF, *bcB, *bcS, *nfused, *nbehind;
};

__global__ __launch_bounds__(LF_BLOCK) void k_lf_lines(LfDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * LF_BLOCK + threadIdx.x;
    const LfKf &k = a.kf[j];
    if (i >= k.n_lines) return;                                      // n_lines <= ct
    const hvo_keyline &l = k.kl[i];
    float dx = __fsub_rn(l.sx, l.ex), dy = __fsub_rn(l.sy, l.ey);    // KeyFrame.cc:688-692
    const float nd = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
    dx = __fdiv_rn(dx, nd); dy = __fdiv_rn(dy, nd);
    a.rec[(size_t)j * a.ct + i] = make_float4(l.pt_x, l.pt_y, dx, dy);
    a.oct[(size_t)j * a.ct + i] = l.octave;
}

__global__ __launch_bounds__(LF_BLOCK) void k_lf_project(LfDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * LF_BLOCK + threadIdx.x;      // i < cq: the grid covers the padded entries exactly
    const LfKf &k = a.kf[j];
    const bool in = i < k.n_ent;
    const size_t cq = (size_t)a.cq, o = (size_t)j * cq + (size_t)i;
    int g = HVO_LF_GATE_SKIP, lvl = -1;
    float u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f, radius = 0.f;
    if (in) {
        const size_t mb = a.per_kf ? (size_t)j : 0;
        const size_t e = a.slots ? (size_t)a.slots[i] : mb * cq + (size_t)i;               // the entry's scalars; its components start at p / pn
        const size_t p = a.slots ? e : mb * 6 * cq + (size_t)i, pn = a.slots ? e : mb * 3 * cq + (size_t)i;
        const bool skip = a.skip[o] || (a.flags && (a.flags[e] & SM_BAD));
        if (!skip) {
            float S[3], E[3];                                        // Mat_<float>(3, 1) << P(0), P(1), P(2)
            for (int c = 0; c < 3; c++) { S[c] = (float)a.pos[p + (size_t)c * a.cstride]; E[c] = (float)a.pos[p + (size_t)(3 + c) * a.cstride]; }
            const float sx = sm_row(k.R, S[0], S[1], S[2], k.t[0]), sy = sm_row(k.R + 3, S[0], S[1], S[2], k.t[1]), sz = sm_row(k.R + 6, S[0], S[1], S[2], k.t[2]);
            const float ex = sm_row(k.R, E[0], E[1], E[2], k.t[0]), ey = sm_row(k.R + 3, E[0], E[1], E[2], k.t[1]), ez = sm_row(k.R + 6, E[0], E[1], E[2], k.t[2]);
            g = HVO_LF_GATE_BEHIND;
            if (!(sz < 0.0f || ez < 0.0f)) {                         // LSDmatcher.cpp:1340
                const float invz1 = __fdiv_rn(1.0f, sz);
                u1 = sm_pinhole(k.fx, sx, invz1, k.cx); v1 = sm_pinhole(k.fy, sy, invz1, k.cy);
                g = HVO_LF_GATE_OUT_OF_IMAGE;
                if (u1 >= k.minX && u1 < k.maxX && v1 >= k.minY && v1 < k.maxY) {          // :1347, a NaN fails
                    const float invz2 = __fdiv_rn(1.0f, ez);
                    u2 = sm_pinhole(k.fx, ex, invz2, k.cx); v2 = sm_pinhole(k.fy, ey, invz2, k.cy);
                    if (u2 >= k.minX && u2 < k.maxX && v2 >= k.minY && v2 < k.maxY) {      // :1355
                        const float mfMax = a.maxd[e]; float maxD, minD; sm_dist_band(mfMax, a.mind[e], &maxD, &minD);
                        double d[3];                                 // OM = 0.5 * (SP + EP) - Ow, the midpoint in DOUBLE (local_lines.hip forms it in float)
                        for (int c = 0; c < 3; c++) {
                            const float mid = (float)__dadd_rn(__dmul_rn((double)S[c], 0.5), __dmul_rn((double)E[c], 0.5));
                            d[c] = (double)__fsub_rn(mid, k.Ow[c]);
                        }
                        const float dist = sm_dist3(d[0], d[1], d[2]);
                        g = dist < minD ? HVO_LF_GATE_DIST_MIN : dist > maxD ? HVO_LF_GATE_DIST_MAX : HVO_LF_GATE_SEARCHED;
                        if (g == HVO_LF_GATE_SEARCHED) {
                            const double n0 = (double)(float)a.nrm[pn], n1 = (double)(float)a.nrm[pn + a.cstride], n2 = (double)(float)a.nrm[pn + 2 * a.cstride];
                            const double dot = __dadd_rn(__dadd_rn(__dmul_rn(d[0], n0), __dmul_rn(d[1], n1)), __dmul_rn(d[2], n2));
                            if (dot < __dmul_rn(0.5, (double)dist)) g = HVO_LF_GATE_VIEW_ANGLE;        // :1371
                            else {
                                int l = sm_predict_level(mfMax, dist, a.logsf);                       // MapLine.cpp:557
                                if (a.as_written) { if (l < 0 || l >= a.n_levels) g = HVO_LF_GATE_LEVEL; }
                                else l = sm_clamp_level(l, a.n_levels);
                                lvl = l;
                                if (g == HVO_LF_GATE_SEARCHED) radius = __fmul_rn(a.th, a.tab[l]);
                            }
                        }
                    }
                }
            }
        }
    }
    a.proj[4 * o] = u1; a.proj[4 * o + 1] = v1; a.proj[4 * o + 2] = u2; a.proj[4 * o + 3] = v2;
    a.rad[o] = radius; a.level[o] = lvl; a.gate[o] = (int8_t)g; a.bi[o] = -1; a.bd[o] = 256;
}

__global__ __launch_bounds__(LF_BLOCK) void k_lf_search(LfDev a)
{
    __shared__ float4 s_rec[LF_CHUNK];
    __shared__ int s_oct[LF_CHUNK];
    const int j = blockIdx.y, tid = threadIdx.x, sub = tid & (LF_GROUP - 1);
    const int i = blockIdx.x * (LF_BLOCK / LF_GROUP) + tid / LF_GROUP;      // i < cq
    const LfKf &k = a.kf[j];
    const size_t o = (size_t)j * a.cq + (size_t)i;
    const bool act = i < k.n_ent && a.gate[o] == HVO_LF_GATE_SEARCHED;
    if (!__syncthreads_or(act)) return;                              // the whole block leaves together
    float d1x = 0.f, d1y = 0.f, rr = 0.f; double mx = 0.0, my = 0.0; int lvl = 0;
    unsigned long long q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    if (act) {
        const float x1 = a.proj[4 * o], y1 = a.proj[4 * o + 1], x2 = a.proj[4 * o + 2], y2 = a.proj[4 * o + 3], r = a.rad[o];
        d1x = __fsub_rn(x1, x2); d1y = __fsub_rn(y1, y2);            // KeyFrame.cc:674-678
        const float nd = sqrtf(__fadd_rn(__fmul_rn(d1x, d1x), __fmul_rn(d1y, d1y)));
        d1x = __fdiv_rn(d1x, nd); d1y = __fdiv_rn(d1y, nd);
        mx = __dmul_rn(0.5, (double)__fadd_rn(x1, x2)); my = __dmul_rn(0.5, (double)__fadd_rn(y1, y2));
        rr = __fmul_rn(r, r); lvl = a.level[o];
        const size_t e = a.slots ? (size_t)a.slots[i] : (a.per_kf ? (size_t)j * a.cq : 0) + (size_t)i;
        const ulonglong4 qd = ld256(a.mdesc + e * 32); q0 = qd.x; q1 = qd.y; q2 = qd.z; q3 = qd.w;
    }
    const float4 *rec = a.rec + (size_t)j * a.ct; const int32_t *oct = a.oct + (size_t)j * a.ct;
    const int n = k.n_lines, rows = k.n_rows;
    unsigned best = LF_NOKEY;
    for (int base = 0; base < n; base += LF_CHUNK) {
        const int m = n - base < LF_CHUNK ? n - base : LF_CHUNK;
        if (base) __syncthreads();                                   // the chunk before has been read by every group
        if (tid < m) { s_rec[tid] = rec[base + tid]; s_oct[tid] = oct[base + tid]; }
        __syncthreads();
        if (act) for (int p = sub; p < m; p += LF_GROUP) {
            const float4 f = s_rec[p];
            const double ex = __dsub_rn(mx, (double)f.x), ey = __dsub_rn(my, (double)f.y);
            const float distance = (float)__dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey));
            if (distance > rr) continue;                             // :685
            const float c = fabsf(__fadd_rn(__fmul_rn(d1x, f.z), __fmul_rn(d1y, f.w)));
            if (c < 0.998f) continue;                                // :695, a NaN passes
            const int oc = s_oct[p], idx = base + p;
            if (oc < lvl - 1 || oc > lvl) continue;                  // LSDmatcher.cpp:1395
            if (idx >= rows) continue;                               // no such row (reading 1)
            const unsigned dist = ham256(make_ulonglong4(q0, q1, q2, q3), ld256(k.desc + (size_t)idx * 32));
            const unsigned key = (dist << 16) | (unsigned)idx;
            best = key < best ? key : best;
        }
    }
    for (int w = LF_GROUP / 2; w > 0; w >>= 1) { const unsigned other = (unsigned)__shfl_xor((int)best, w); best = other < best ? other : best; }
    if (act && sub == 0) {
        const int bd = (int)(best >> 16);
        if (bd < 256) { a.bi[o] = (int)(best & 0xFFFFu); a.bd[o] = bd; }      // 256 never enters (dist < bestDist, bestDist = 256)
    }
}

__global__ __launch_bounds__(LF_BLOCK) void k_lf_count(LfDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * LF_BLOCK + threadIdx.x;      // i < cq; a padded entry is HVO_LF_GATE_SKIP with best_dist 256
    const size_t o = (size_t)j * a.cq + (size_t)i;
    const int g = a.gate[o];
    const bool s = g == HVO_LF_GATE_SEARCHED, f = s && a.bd[o] <= a.th_low, b = g == HVO_LF_GATE_BEHIND;
    a.passF[o] = f ? 1 : 0; a.passB[o] = b ? 1 : 0;
    const int nf = __syncthreads_count(f), nb = __syncthreads_count(b), ns = __syncthreads_count(s);
    if (threadIdx.x == 0) { const size_t q = (size_t)j * a.nb + blockIdx.x; a.bcF[q] = nf; a.bcB[q] = nb; a.bcS[q] = ns; }
}

__global__ __launch_bounds__(LF_BLOCK) void k_lf_compact(LfDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * LF_BLOCK + threadIdx.x, behind = blockIdx.z;
    bool p;
    const int at = sm_compact_pos(behind ? a.bcB : a.bcF, a.nb, a.cq, j, behind ? a.passB : a.passF, behind ? a.nbehind : a.nfused, &p);
    if (p) {
        const size_t q0 = (size_t)j * a.cq;
        if (behind) a.be[q0 + at] = i;
        else { a.fe[q0 + at] = i; a.fi[q0 + at] = a.bi[q0 + i]; }
    }
}

// what lf_run serves: the key-frame side (host arrays kf[j], or the one resident frame fr with kf[0]'s pose, camera, bounds and skip), the
// map side (host arrays maps[0] shared / maps[j], or n_slots slots of m)
static int lf_run(hvo_ctx *ctx, hipStream_t st, const hvo_lf_params *P, const FrameView *fr, int n_kf, const hvo_lf_keyframe *kf,
                  const hvo_lf_map *maps, hvo_line_map *m, int n_slots, const int32_t *slots, hvo_lf_result *res, std::string *err)
{
    const bool per_kf = !m && P->map_per_keyframe != 0;
    // ---- refusals: whole, before anything is written ----
    if (P->th_low > 255) { *err = "fuse lines: th_low above 255 (bestDist starts at 256: the reference would accept bestIdx = -1)"; return HVO_ERR_INVALID_ARG; }
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { *err = "fuse lines: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (P->level_rule != HVO_LF_LEVEL_CLAMPED && P->level_rule != HVO_LF_LEVEL_AS_WRITTEN) { *err = "fuse lines: unknown level_rule"; return HVO_ERR_INVALID_ARG; }
    if (m) {
        if (P->map_per_keyframe) { *err = "fuse lines: the slot form has one slot list for all key frames (map_per_keyframe must be 0)"; return HVO_ERR_INVALID_ARG; }
        if (m->device != ctx->device) { *err = "fuse lines: the line map lives on another device"; return HVO_ERR_INVALID_ARG; }
        if (n_slots < 0 || (n_slots > 0 && !slots)) { *err = "fuse lines: n < 0 or no slot list"; return HVO_ERR_INVALID_ARG; }
        for (int i = 0; i < n_slots; i++) if (slots[i] < 0 || slots[i] >= m->n_slots) {
            *err = "fuse lines: entry " + std::to_string(i) + " names slot " + std::to_string(slots[i]) + " outside the map's " + std::to_string(m->n_slots) + " slots; nothing was written";
            return HVO_ERR_INVALID_ARG;
        }
    } else {
        for (int s = 0; s < (per_kf ? n_kf : 1); s++) {
            const hvo_lf_map &M = maps[s];
            if (M.n < 0 || (M.n > 0 && (!M.pos || !M.normal || !M.max_distance || !M.min_distance || !M.desc))) { *err = "fuse lines: a map side with n < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
        }
    }
    int nmax = 0, tmax = 0;
    std::vector<int> n_ent((size_t)n_kf), n_line((size_t)n_kf), n_rows((size_t)n_kf);
    for (int j = 0; j < n_kf; j++) {
        const hvo_lf_keyframe &K = kf[j];
        if (!(K.bounds[1] > K.bounds[0]) || !(K.bounds[3] > K.bounds[2])) { *err = "fuse lines: empty image bounds"; return HVO_ERR_INVALID_ARG; }
        n_ent[j] = m ? n_slots : maps[per_kf ? j : 0].n;
        n_line[j] = fr ? fr->n_kl : K.n; n_rows[j] = fr ? fr->n_kl : K.n_desc_rows;
        if (n_line[j] < 0 || n_rows[j] < 0 || (!fr && ((n_line[j] > 0 && !K.kl) || (n_rows[j] > 0 && !K.desc_rows)))) { *err = "fuse lines: a key frame with n < 0, n_desc_rows < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
        if (!res[j].best_idx) { *err = "fuse lines: a result without best_idx"; return HVO_ERR_INVALID_ARG; }
        nmax = std::max(nmax, n_ent[j]); tmax = std::max(tmax, n_line[j]);
    }
    const size_t cq = (size_t)std::max(LF_BLOCK, (nmax + LF_BLOCK - 1) / LF_BLOCK * LF_BLOCK), ct = (size_t)std::max(64, (tmax + 63) & ~63), F = (size_t)n_kf;
    if (tmax > LF_MAXL || nmax > LF_MAXQ || F * cq > LF_MAXTOTAL) {
        *err = "fuse lines: " + std::to_string(nmax) + " entries, " + std::to_string(tmax) + " lines per key frame, " + std::to_string(F * cq) + " padded entries in all (limits: " +
               std::to_string(LF_MAXQ) + ", " + std::to_string(LF_MAXL) + ", " + std::to_string(LF_MAXTOTAL) + "); nothing was written";
        return HVO_ERR_UNSUPPORTED;
    }
    // ---- one carve of the context's arena: what goes up, the records and radii, the flags and counts, what comes down ----
    const size_t S = m ? 0 : (per_kf ? F : 1), nb = cq / LF_BLOCK, Fh = fr ? 0 : F;     // Fh: key-frame sides that go up
    size_t rmax = 0;
    for (int j = 0; j < n_kf; j++) rmax = std::max(rmax, (size_t)n_rows[j]);
    const size_t cr = std::max((size_t)64, (rmax + 63) & ~(size_t)63);
    StageCarver C(256);
    const auto u_kf = C.take<LfKf>(F); const auto u_tab = C.take<float>(HVO_MAX_LEVELS); const auto u_skip = C.take<uint8_t>(F, cq);
    const auto u_kl = C.take<hvo_keyline>(Fh, ct); const auto u_kd = C.take<uint8_t>(Fh, cr * 32);
    const auto u_pos = C.take<double>(6 * S, cq), u_nrm = C.take<double>(3 * S, cq); const auto u_maxd = C.take<float>(S, cq), u_mind = C.take<float>(S, cq);      // by component
    const auto u_md = C.take<uint8_t>(S, cq * 32); const auto u_slots = C.take<int32_t>(m ? cq : 0);
    const size_t up_end = C.mark();
    const auto g_rec = C.take<float4>(F, ct); const auto g_oct = C.take<int32_t>(F, ct); const auto q_rad = C.take<float>(F, cq);
    const auto s_pF = C.take<uint8_t>(F, cq), s_pB = C.take<uint8_t>(F, cq); const auto s_bcF = C.take<int>(F, nb), s_bcB = C.take<int>(F, nb);
    const size_t r0 = C.mark();                                      // [r0, r1) comes down
    const auto r_cnt = C.take<int>(2, F);                            // row 0: fused, row 1: behind
    const auto r_bcS = C.take<int>(F, nb);                           // searched entries per block of LF_BLOCK: summed here
    const auto r_bi = C.take<int32_t>(F, cq), r_bd = C.take<int32_t>(F, cq), r_lvl = C.take<int32_t>(F, cq);
    const auto r_proj = C.take<float>(F, cq * 4); const auto r_gate = C.take<int8_t>(F, cq);
    const auto r_fe = C.take<int32_t>(F, cq), r_fi = C.take<int32_t>(F, cq), r_be = C.take<int32_t>(F, cq);
    const size_t r1 = C.mark();
    StagedCall sc(ctx, st, "fuse lines: ", err); int rc;
    if ((rc = sc.begin(r1, up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    float *tab = u_tab.host(h), sf = 1.0f;
    for (int l = 0; l < HVO_MAX_LEVELS; l++) { if (l > 0 && l < P->n_levels) sf = sf * P->scale_factor; tab[l] = l < P->n_levels ? sf : 1.0f; }
    for (int j = 0; j < n_kf; j++) {
        const hvo_lf_keyframe &K = kf[j];
        LfKf &c = *u_kf.host(h, j);
        pose_split(K.Tcw, c.R, c.t, c.Ow);
        c.fx = K.fx; c.fy = K.fy; c.cx = K.cx; c.cy = K.cy; c.minX = K.bounds[0]; c.maxX = K.bounds[1]; c.minY = K.bounds[2]; c.maxY = K.bounds[3];
        c.n_lines = n_line[j]; c.n_ent = n_ent[j]; c.n_rows = n_rows[j];
        if (fr) { c.kl = fr->kl; c.desc = fr->ldesc; }
        else {
            c.kl = u_kl.dev(d, j); c.desc = u_kd.dev(d, j);
            if (n_line[j]) memcpy(u_kl.host(h, j), K.kl, (size_t)n_line[j] * sizeof(hvo_keyline));
            if (n_rows[j]) memcpy(u_kd.host(h, j), K.desc_rows, (size_t)n_rows[j] * 32);
        }
        if (K.skip && n_ent[j]) memcpy(u_skip.host(h, j), K.skip, (size_t)n_ent[j]);
    }
    for (size_t s = 0; s < S; s++) {
        const hvo_lf_map &M = maps[s];
        const size_t n = (size_t)M.n;
        for (int q = 0; q < 6; q++) { double *hp = u_pos.host(h, 6 * s + q); for (size_t i = 0; i < n; i++) hp[i] = M.pos[6 * i + q]; }      // by component
        for (int q = 0; q < 3; q++) { double *hn = u_nrm.host(h, 3 * s + q); for (size_t i = 0; i < n; i++) hn[i] = M.normal[3 * i + q]; }
        if (n) { memcpy(u_maxd.host(h, s), M.max_distance, n * 4); memcpy(u_mind.host(h, s), M.min_distance, n * 4); memcpy(u_md.host(h, s), M.desc, n * 32); }
    }
    if (m && n_slots) memcpy(u_slots.host(h), slots, (size_t)n_slots * 4);
    if ((rc = sc.up(0, up_end))) return rc;
    sc.tick();
    LfDev a; memset(&a, 0, sizeof(a));
    a.kf = u_kf.dev(d); a.cq = (int)cq; a.ct = (int)ct; a.n_levels = P->n_levels; a.per_kf = per_kf ? 1 : 0; a.nb = (int)nb;
    a.as_written = P->level_rule == HVO_LF_LEVEL_AS_WRITTEN ? 1 : 0;
    if (m) {
        a.pos = m->dev<double>(m->POS); a.nrm = m->dev<double>(m->NRM); a.maxd = m->dev<float>(m->MAXD); a.mind = m->dev<float>(m->MIND); a.mdesc = m->dev<uint8_t>(m->DESC);
        a.flags = m->d_flags(); a.slots = u_slots.dev(d); a.cstride = (size_t)m->cap;
    } else {
        a.pos = u_pos.dev(d); a.nrm = u_nrm.dev(d); a.maxd = u_maxd.dev(d); a.mind = u_mind.dev(d); a.mdesc = u_md.dev(d); a.cstride = cq;
    }
    a.skip = u_skip.dev(d); a.tab = u_tab.dev(d); a.logsf = P->log_scale_factor; a.th = P->th; a.th_low = P->th_low;
    a.rec = g_rec.dev(d); a.oct = g_oct.dev(d); a.rad = q_rad.dev(d);
    a.proj = r_proj.dev(d); a.level = r_lvl.dev(d); a.gate = r_gate.dev(d); a.bi = r_bi.dev(d); a.bd = r_bd.dev(d);
    a.fe = r_fe.dev(d); a.fi = r_fi.dev(d); a.be = r_be.dev(d); a.passF = s_pF.dev(d); a.passB = s_pB.dev(d);
    a.bcF = s_bcF.dev(d); a.bcB = s_bcB.dev(d); a.bcS = r_bcS.dev(d); a.nfused = r_cnt.dev(d, 0); a.nbehind = r_cnt.dev(d, 1);
    if (tmax > 0) hipLaunchKernelGGL(k_lf_lines, dim3((unsigned)((ct + LF_BLOCK - 1) / LF_BLOCK), n_kf), dim3(LF_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_lf_project, dim3((unsigned)nb, n_kf), dim3(LF_BLOCK), 0, st, a);
    sc.tick();
    if (nmax > 0 && tmax > 0) hipLaunchKernelGGL(k_lf_search, dim3((unsigned)(cq / (LF_BLOCK / LF_GROUP)), n_kf), dim3(LF_BLOCK), 0, st, a);
    sc.tick();
    hipLaunchKernelGGL(k_lf_count, dim3((unsigned)nb, n_kf), dim3(LF_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_lf_compact, dim3((unsigned)nb, n_kf, 2), dim3(LF_BLOCK), 0, st, a);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    for (int j = 0; j < n_kf; j++) {
        hvo_lf_result &R = res[j];
        const size_t n = (size_t)n_ent[j];
        int ns = 0;
        for (size_t q = 0; q < nb; q++) ns += r_bcS.down(b, j)[q];
        R.n_searched = ns; R.n_fused = r_cnt.down(b, 0)[j]; R.n_behind = r_cnt.down(b, 1)[j]; R.status = HVO_OK;
        for (int i = 0; i < 3; i++) R.kernel_ms[i] = sc.ms[i];
        if (!n) continue;
        memcpy(R.best_idx, r_bi.down(b, j), n * 4);
        if (R.best_dist) memcpy(R.best_dist, r_bd.down(b, j), n * 4);
        if (R.gate) memcpy(R.gate, r_gate.down(b, j), n);
        if (R.level) memcpy(R.level, r_lvl.down(b, j), n * 4);
        if (R.proj) memcpy(R.proj, r_proj.down(b, j), n * 16);
        const size_t nf = (size_t)std::max(0, std::min(R.n_fused, (int32_t)n)), nh = (size_t)std::max(0, std::min(R.n_behind, (int32_t)n));
        if (R.fused_entry) memcpy(R.fused_entry, r_fe.down(b, j), nf * 4);
        if (R.fused_idx) memcpy(R.fused_idx, r_fi.down(b, j), nf * 4);
        if (R.behind_entry) memcpy(R.behind_entry, r_be.down(b, j), nh * 4);
    }
    return HVO_OK;
}

extern "C" {

int hvo_fuse_lines(hvo_ctx *ctx, const hvo_lf_params *params, const hvo_lf_map *map_side, int n_kf, const hvo_lf_keyframe *keyframes, hvo_lf_result *results)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!params || !map_side || !keyframes || !results || n_kf < 1) { ctx->last_error = "fuse lines: a null argument or n_kf < 1"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return lf_run(ctx, ctx->stream, params, nullptr, n_kf, keyframes, map_side, nullptr, 0, nullptr, results, &ctx->last_error);
}

int hvo_fuse_lines_slots(hvo_ctx *ctx, hvo_line_map *m, int n, const int32_t *slots, const hvo_lf_params *params, int n_kf, const hvo_lf_keyframe *keyframes,
                         hvo_lf_result *results)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!m || !params || !keyframes || !results || n_kf < 1) { ctx->last_error = "fuse lines: a null argument or n_kf < 1"; if (m) m->last_error = ctx->last_error; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const int rc = lf_run(ctx, ctx->stream, params, nullptr, n_kf, keyframes, nullptr, m, n, slots, results, &ctx->last_error);
    if (rc) m->last_error = ctx->last_error;
    return rc;
}

int hvo_stream_fuse_lines(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_lf_params *params, const float Tcw[12], const uint8_t *skip,
                          const hvo_lf_map *map_side, hvo_line_map *m, int n, const int32_t *slots, hvo_lf_result *result)
{
    if (!s) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !Tcw || !result || (!map_side && !m)) { s->last_error = "fuse lines: a null argument or no map side"; return HVO_ERR_INVALID_ARG; }
    FrameView V; int rc;
    if ((rc = stream_view(s, cur, need_fuse_lines, s->s_match, V))) return rc;
    hvo_lf_keyframe K; memset(&K, 0, sizeof(K));
    memcpy(K.Tcw, Tcw, sizeof(K.Tcw)); K.skip = skip; K.fx = cam->fx; K.fy = cam->fy; K.cx = cam->cx; K.cy = cam->cy;
    for (int q = 0; q < 4; q++) K.bounds[q] = V.bounds[q];
    hvo_lf_params P = *params; P.map_per_keyframe = 0;
    rc = lf_run(V.ctx, s->s_match, &P, &V, 1, &K, map_side, map_side ? nullptr : m, n, slots, result, &s->last_error);
    if (rc && !map_side) m->last_error = s->last_error;
    return rc;
}

}   // extern "C"
