// kf_search.hip -- ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (reference src/ORBmatcher.cc:1499-1628), the
// refinement Tracking::Relocalization runs between its pose optimisations (src/Tracking.cc:3871 with (10, 100), :3885 with (3, 64)), for
// n_kf candidate key frames in one call, each under its own pose and its own occupancy of the frame's features.
//
//   k_kf_project   one launch for all candidates (blockIdx.y = candidate), one lane per key-frame entry: skip, projection, the four bounds
//                  tests, the distance range, MapPoint::PredictScale against the current frame (src/MapPoint.cc:400-415); it writes the query
//                  arrays SbpDev names (u, v, radius, band [level - 1, level + 1], blocks) and proj / level / gate for the caller.  An entry
//                  that fails a gate gets k_project_last's out-of-grid sentinel: the search core touches no train feature for it.
//   k_search_by_projection, k_sbp_epilogue (match.hip, unchanged, map_mode = 0) once per candidate: ranked window candidates, the in-order
//                  pass under the occupancy bit set (t_occ = occupied, q_blocks = 1 for every entry), the rescan, the 30-bin rotation
//                  histogram of kf angle - frame angle and ComputeThreeMaxima.  th_high = ORBdist: bestDist starts at 256, only strictly
//                  smaller distances enter, and bestDist <= ORBdist accepts -- no ratio test, no mvuRight gate (q_ur and t_uright are null).
//   k_kf_inverse   feature_kf[match_idx[i]] = i (every match blocks, so no feature is taken twice); an entry without a match gets distance 256
//
// The grid of every launch is sized by n, which the host knows: all candidates are enqueued before the call's single synchronisation.
// Staging (the candidates, and the frame's arrays in the host-array form) and scratch come from the context's call arena.
//
// What distinguishes this call from its siblings (k_project_last, k_lp_frustum):
//   no depth-sign test     a point behind the camera whose projection lands inside the bounds and whose distance is in range IS searched;
//                          z == 0 gives inf (a bounds gate) or NaN, and a NaN passes the four bounds tests and finds no candidate
//   every feature blocks   CurrentFrame.mvpMapPoints[i2] != NULL skips i2, whatever that point's observations; every accepted match is such
//                          a point for the entries after it, also one the rotation cull removes at the end
//   bestDist <= ORBdist    ORBdist > 255 would accept bestIdx2 = -1 and write mvpMapPoints[-1]: refused
//
// Readings (OpenCV is not in the reference tree; DESIGN.md section 7, tests/kf_search_ref.py restates the same):
//   Rcw * x3Dw + tcw       gemm3_row (match.hip; sm_row is the same text): the row's products summed in FLOAT left to right, then
//                          (float)((double)sum * 1.0 + (double)t * 1.0)
//   invzc = 1.0 / z        k_project_last's reading: the text divides the double 1.0, the quotient is rounded to float
//   u, v                   sm_pinhole: fx * xc * invzc + cx in float, left to right
//   Ow                     -Rcw^T tcw with double sums, times -1.0, rounded to float (match_project_setup's twc)
//   x3Dw - Ow              float, element-wise
//   cv::norm               sm_dist3: sqrt of the double sum of squares, stored to float
//   1.2f * mfMaxDistance   sm_dist_band: float products (GetMaxDistanceInvariance / GetMinDistanceInvariance)
//   PredictScale           sm_predict_level, then sm_clamp_level to [0, n_levels - 1] (map_gates.hpp, shared with every sibling)
//   radius                 th * mvScaleFactors[level], a float product; the scale factors are the context's
// No contraction (-ffp-contract=off, __f*_rn).
#include "slot_map.hpp"
#include "frame_view.hpp"
#include "staged_call.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#define KFS_BLOCK 256
#define KFS_MAXQ 16384            // entries per candidate (SBP_MAXQ of match.hip)
#define KFS_MAXT 65535            // frame features (the search core's keys hold the feature in 16 bits)

struct KfsCand { float R[9], t[3], Ow[3]; int n; };
struct KfsDev {
    const KfsCand *cand; int cq, n_levels;                       // candidate j's arrays start at j * cq (pos: component c at (3 j + c) * cq)
    const float *pos, *maxd, *mind; const uint8_t *skip;
    float fx, fy, cx, cy, minX, maxX, minY, maxY, logsf, th; float sf[HVO_MAX_LEVELS];
    float *q_u, *q_v, *q_rad; int *q_min, *q_max; uint8_t *q_blocks;
    float *proj; int32_t *level; int8_t *gate; int32_t *mi, *md; int *counters;     // counters: (n_matches, n_searched) per candidate
};

__global__ __launch_bounds__(KFS_BLOCK) void k_kf_project(KfsDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * KFS_BLOCK + threadIdx.x;
    const KfsCand &c = a.cand[j];
    const bool in = i < c.n;
    const size_t cq = (size_t)a.cq, o = (size_t)j * cq + (in ? (size_t)i : 0);
    int g = HVO_KF_GATE_SKIP, lvl = -1, lo = 0, hi = -1;
    float u = 1e30f, v = 1e30f, radius = 0.f, pu = 0.f, pv = 0.f;  // an entry that fails a gate: no grid cell, never searched (k_project_last)
    if (in && !a.skip[o]) {
        const size_t p = (size_t)j * 3 * cq + (size_t)i;
        const float X = a.pos[p], Y = a.pos[p + cq], Z = a.pos[p + 2 * cq];
        const float xc = sm_row(c.R, X, Y, Z, c.t[0]), yc = sm_row(c.R + 3, X, Y, Z, c.t[1]), zc = sm_row(c.R + 6, X, Y, Z, c.t[2]);
        const float invzc = (float)(1.0 / (double)zc);             // ORBmatcher.cc:1529; no sign test follows
        pu = sm_pinhole(a.fx, xc, invzc, a.cx); pv = sm_pinhole(a.fy, yc, invzc, a.cy);
        g = pu < a.minX ? HVO_KF_GATE_U_MIN : pu > a.maxX ? HVO_KF_GATE_U_MAX : pv < a.minY ? HVO_KF_GATE_V_MIN : pv > a.maxY ? HVO_KF_GATE_V_MAX : 0;   // (a NaN compares false four times)
        if (g == 0) {
            const float mfMax = a.maxd[o]; float maxD, minD; sm_dist_band(mfMax, a.mind[o], &maxD, &minD);
            const float dist = sm_dist3(__fsub_rn(X, c.Ow[0]), __fsub_rn(Y, c.Ow[1]), __fsub_rn(Z, c.Ow[2]));
            g = dist < minD ? HVO_KF_GATE_DIST_MIN : dist > maxD ? HVO_KF_GATE_DIST_MAX : 0;
            if (g == 0) {
                const int l = sm_clamp_level(sm_predict_level(mfMax, dist, a.logsf), a.n_levels);      // MapPoint.cc:400-415
                lvl = l; u = pu; v = pv; radius = __fmul_rn(a.th, a.sf[l]); lo = l - 1; hi = l + 1;
            }
        }
    }
    if (in) {
        a.q_u[o] = u; a.q_v[o] = v; a.q_rad[o] = radius; a.q_min[o] = lo; a.q_max[o] = hi; a.q_blocks[o] = 1;
        reinterpret_cast<float2 *>(a.proj)[o] = make_float2(pu, pv); a.level[o] = lvl; a.gate[o] = (int8_t)g;
        a.mi[o] = -1; a.md[o] = 256;                               // what stays where no search runs (a frame without features)
    }
    const unsigned long long s = __ballot(in && g == 0);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&a.counters[2 * j + 1], __popcll(s));
}

__global__ __launch_bounds__(KFS_BLOCK) void k_kf_inverse(int n, int nt, const int32_t *__restrict__ mi, int32_t *__restrict__ md, int32_t *__restrict__ fk)
{
    const int i = blockIdx.x * KFS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int m = mi[i];
    if (m >= 0 && m < nt) fk[m] = i;                               // CurrentFrame.mvpMapPoints[bestIdx2] = pMP
    else md[i] = 256;                                              // no match, or culled by the rotation histogram
}

static std::string kfs_limit_text(int n, int nt)
{
    return "key-frame search: " + std::to_string(n) + " key-frame entries, " + std::to_string(nt) + " frame features (limits: " + std::to_string(KFS_MAXQ) +
           ", " + std::to_string(KFS_MAXT) + "); nothing was written";
}

int kfs_run(hvo_ctx *ctx, hipStream_t st, const hvo_camera *cam, const hvo_kf_search_params *P, const FrameView *fr, const hvo_local_points_frame *host,
            int n_kf, const hvo_kf_search_candidate *kf, hvo_kf_search_result *res, std::string *err)
{
    const int nt = fr->n_kp;
    // ---- refusals: whole, before anything is written ----
    if (P->orb_dist > 255) { *err = "key-frame search: orb_dist above 255 (bestDist starts at 256: the reference would write mvpMapPoints[-1])"; return HVO_ERR_INVALID_ARG; }
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { *err = "key-frame search: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (!(fr->bounds[1] > fr->bounds[0]) || !(fr->bounds[3] > fr->bounds[2])) { *err = "key-frame search: empty image bounds"; return HVO_ERR_INVALID_ARG; }
    if (nt < 0 || (host && nt > 0 && (!host->kp_un || !host->desc))) { *err = "key-frame search: a frame with n < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
    int nmax = 0;
    for (int j = 0; j < n_kf; j++) {
        const hvo_kf_search_candidate &K = kf[j];
        if (K.n < 0 || (K.n > 0 && (!K.pos || !K.skip || !K.max_dist || !K.min_dist || !K.desc)) || !res[j].match_idx) {
            *err = "key-frame search: a candidate with n < 0, a null array or no match_idx"; return HVO_ERR_INVALID_ARG;
        }
        if (K.n > 0 && P->check_orientation && !K.angle) { *err = "key-frame search: check_orientation without the key frame's angles"; return HVO_ERR_INVALID_ARG; }
        nmax = std::max(nmax, (int)K.n);
    }
    for (int j = 0; j < n_kf; j++) if (kf[j].n > KFS_MAXQ || nt > KFS_MAXT) { *err = kfs_limit_text(kf[j].n, nt); return HVO_ERR_UNSUPPORTED; }
    // ---- one carve of the context's arena: what goes up, the queries, what comes down, the search's key rows ----
    const size_t cq = (size_t)std::max(64, (nmax + 63) & ~63), ntp = (size_t)std::max(64, (nt + 63) & ~63), F = (size_t)n_kf;
    StageCarver C(256);
    const auto u_cand = C.take<KfsCand>(F);
    const auto u_pos = C.take<float>(3 * F, cq), u_maxd = C.take<float>(F, cq), u_mind = C.take<float>(F, cq), u_ang = C.take<float>(F, cq);      // pos by component: row 3 j + k
    const auto u_desc = C.take<uint8_t>(F, cq * 32), u_skip = C.take<uint8_t>(F, cq), u_occ = C.take<uint8_t>(F, ntp);
    const auto u_kp = C.take<hvo_keypoint>(host ? ntp : 0); const auto u_fd = C.take<uint8_t>(host ? ntp * 32 : 0);
    const size_t up_end = C.mark();
    const auto q_u = C.take<float>(F, cq), q_v = C.take<float>(F, cq), q_rad = C.take<float>(F, cq);
    const auto q_min = C.take<int>(F, cq), q_max = C.take<int>(F, cq); const auto q_blk = C.take<uint8_t>(F, cq);
    const size_t r0 = C.mark();
    const auto r_cnt = C.take<int>(F, 2), r_fk = C.take<int32_t>(F, ntp), r_mi = C.take<int32_t>(F, cq), r_md = C.take<int32_t>(F, cq), r_lvl = C.take<int32_t>(F, cq);
    const auto r_proj = C.take<float>(F, cq * 2); const auto r_gate = C.take<int8_t>(F, cq);
    const size_t r1 = C.mark();                                  // [r0, r1) comes down
    const auto s_keys = C.take<char>(match_sbp_scratch_bytes((int)cq));  // the candidates' searches run one after the other on the stream and share the key rows
    StagedCall sc(ctx, st, "key-frame search: ", err); int rc;
    if ((rc = sc.begin(C.mark(), up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    for (int j = 0; j < n_kf; j++) {
        const hvo_kf_search_candidate &K = kf[j];
        KfsCand &c = *u_cand.host(h, j);
        pose_split(K.Tcw, c.R, c.t, c.Ow);                         // Ow = -Rcw^T tcw (match_project_setup's twc)
        c.n = K.n;
        const size_t n = (size_t)K.n;
        float *const hp[3] = { u_pos.host(h, 3 * j), u_pos.host(h, 3 * j + 1), u_pos.host(h, 3 * j + 2) };
        for (size_t i = 0; i < n; i++) if (!K.skip[i]) for (int k = 0; k < 3; k++) hp[k][i] = K.pos[3 * i + k];      // by component: a wave's load is contiguous
        if (n) {
            memcpy(u_maxd.host(h, j), K.max_dist, n * 4); memcpy(u_mind.host(h, j), K.min_dist, n * 4);
            if (K.angle) memcpy(u_ang.host(h, j), K.angle, n * 4);
            memcpy(u_desc.host(h, j), K.desc, n * 32); memcpy(u_skip.host(h, j), K.skip, n);
        }
        if (nt && K.occupied) memcpy(u_occ.host(h, j), K.occupied, (size_t)nt);
    }
    FrameView V = *fr;
    if (host) {
        if (nt) { memcpy(u_kp.host(h), host->kp_un, (size_t)nt * sizeof(hvo_keypoint)); memcpy(u_fd.host(h), host->desc, (size_t)nt * 32); }
        V.kp_un = u_kp.dev(d); V.desc = u_fd.dev(d);
    }
    if ((rc = sc.up(0, up_end)) || (rc = sc.clear(r_cnt.off, r_cnt.off + r_cnt.bytes())) || (rc = sc.clear(r_fk.off, r_fk.off + r_fk.bytes(), 0xFF))) return rc;
    sc.tick();
    KfsDev a; memset(&a, 0, sizeof(a));
    a.cand = u_cand.dev(d); a.cq = (int)cq; a.n_levels = P->n_levels;
    a.pos = u_pos.dev(d); a.maxd = u_maxd.dev(d); a.mind = u_mind.dev(d); a.skip = u_skip.dev(d);
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.minX = V.bounds[0]; a.maxX = V.bounds[1]; a.minY = V.bounds[2]; a.maxY = V.bounds[3]; a.logsf = P->log_scale_factor; a.th = P->th;
    for (int l = 0; l < HVO_MAX_LEVELS; l++) a.sf[l] = V.sf[l];
    a.q_u = q_u.dev(d); a.q_v = q_v.dev(d); a.q_rad = q_rad.dev(d); a.q_min = q_min.dev(d); a.q_max = q_max.dev(d); a.q_blocks = q_blk.dev(d);
    a.proj = r_proj.dev(d); a.level = r_lvl.dev(d); a.gate = r_gate.dev(d); a.mi = r_mi.dev(d); a.md = r_md.dev(d);
    a.counters = r_cnt.dev(d);
    if (nmax > 0) hipLaunchKernelGGL(k_kf_project, dim3((nmax + KFS_BLOCK - 1) / KFS_BLOCK, n_kf), dim3(KFS_BLOCK), 0, st, a);
    sc.tick();
    for (int j = 0; j < n_kf; j++) {
        const int n = kf[j].n;
        if (n < 1 || nt < 1) continue;
        SbpDev s; memset(&s, 0, sizeof(s));
        s.q_desc = u_desc.dev(d, j); s.q_desc_index = nullptr;
        s.q_u = q_u.dev(d, j); s.q_v = q_v.dev(d, j); s.q_radius = q_rad.dev(d, j); s.q_min_level = q_min.dev(d, j); s.q_max_level = q_max.dev(d, j); s.q_ur = nullptr;
        s.q_angle = u_ang.dev(d, j); s.q_blocks = q_blk.dev(d, j);
        s.t_kp = V.kp_un; s.t_uright = nullptr; s.t_occ = kf[j].occupied ? u_occ.dev(d, j) : nullptr; s.t_desc = V.desc;
        s.nq = n; s.nt = nt; s.mnMinX = V.bounds[0]; s.mnMaxX = V.bounds[1]; s.mnMinY = V.bounds[2]; s.mnMaxY = V.bounds[3];
        s.th_high = P->orb_dist; s.check_orientation = P->check_orientation ? 1 : 0; s.map_mode = 0; s.nn_ratio = 0.f;
        s.match_idx = r_mi.dev(d, j); s.match_dist = r_md.dev(d, j); s.n_matches = r_cnt.dev(d, j);
        if ((rc = match_sbp_enqueue(st, s, s_keys.dev(d)))) { *err = rc == HVO_ERR_UNSUPPORTED ? kfs_limit_text(n, nt) : "key-frame search: search launch"; return rc; }
        hipLaunchKernelGGL(k_kf_inverse, dim3((n + KFS_BLOCK - 1) / KFS_BLOCK), dim3(KFS_BLOCK), 0, st, n, nt, (const int32_t *)s.match_idx, s.match_dist, r_fk.dev(d, j));
    }
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    for (int j = 0; j < n_kf; j++) {
        hvo_kf_search_result &R = res[j];
        const size_t n = (size_t)kf[j].n;
        const int *cnt = r_cnt.down(b, j);
        R.n_matches = cnt[0]; R.n_searched = cnt[1]; R.status = HVO_OK; R.kernel_ms[0] = sc.ms[0]; R.kernel_ms[1] = sc.ms[1];
        if (n) {
            memcpy(R.match_idx, r_mi.down(b, j), n * 4);
            if (R.match_dist) memcpy(R.match_dist, r_md.down(b, j), n * 4);
            if (R.proj) memcpy(R.proj, r_proj.down(b, j), n * 8);
            if (R.level) memcpy(R.level, r_lvl.down(b, j), n * 4);
            if (R.gate) memcpy(R.gate, r_gate.down(b, j), n);
        }
        if (R.feature_kf && nt) memcpy(R.feature_kf, r_fk.down(b, j), (size_t)nt * 4);
    }
    return HVO_OK;
}

extern "C" {

int hvo_search_by_projection_keyframe(hvo_ctx *ctx, const hvo_camera *cam, const hvo_kf_search_params *params, const hvo_local_points_frame *frame,
                                      int n_kf, const hvo_kf_search_candidate *candidates, hvo_kf_search_result *results)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !frame || !candidates || !results || n_kf < 1) { ctx->last_error = "key-frame search: a null argument or n_kf < 1"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    FrameView F; memset(&F, 0, sizeof(F));
    F.ctx = ctx; F.n_kp = frame->n; F.sf = ctx->scale; memcpy(F.bounds, params->bounds, sizeof(F.bounds));
    return kfs_run(ctx, ctx->stream, cam, params, &F, frame, n_kf, candidates, results, &ctx->last_error);
}

int hvo_stream_search_by_projection_keyframe(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_kf_search_params *params,
                                             int n_kf, const hvo_kf_search_candidate *candidates, hvo_kf_search_result *results)
{
    if (!s) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !candidates || !results || n_kf < 1) { s->last_error = "key-frame search: a null argument or n_kf < 1"; return HVO_ERR_INVALID_ARG; }
    FrameView B; int rc;
    if ((rc = stream_view(s, cur, need_kf_search, s->s_match, B))) return rc;
    return kfs_run(B.ctx, s->s_match, cam, params, &B, nullptr, n_kf, candidates, results, &s->last_error);
}

}   // extern "C"
