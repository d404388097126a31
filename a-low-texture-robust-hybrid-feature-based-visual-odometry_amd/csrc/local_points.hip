// local_points.hip -- the point side of Tracking::TrackLocalMapWithLines against map points that stay on the device (hvo_point_map):
//   Tracking::SearchLocalPoints (reference src/Tracking.cc:3227-3277) with Frame::isInFrustum(MapPoint *, 0.5) (src/Frame.cc:1371-1427),
//   MapPoint::PredictScale (src/MapPoint.cc:400-415) and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-132)
//   through the search core of match.hip, unchanged (k_track_windows, k_search_by_projection, k_sbp_epilogue in map_mode).
//
// The map is a slot map (slot_map.hpp: the storage, its growth and uploads, the flag byte, the call's skeleton).  Per slot (= position in
// mvpLocalMapPoints) the point map keeps GetWorldPos() and GetNormal() (3 floats each, both CV_32F), mfMaxDistance and mfMinDistance (raw
// floats) and GetDescriptor() (32 bytes).  Every component is an array of its own over the slots, as in the line map (local_lines.hip): the
// frustum kernel runs one lane per slot, so a wave's load of one component covers 256 contiguous bytes.  The descriptor is consumed whole,
// 32 bytes by one lane of the gather, and stays packed.
//
// The call, the same kernels for the host, stream and batch forms (bit-identical results):
//   k_sm_mark      (slot_map.hip) held slots that are bad become -1; t_occupied = the feature holds an observed point (a slot with the
//                  observed flag, or HVO_HELD_FOREIGN_OBSERVED); held and seen_extra slots are marked seen
//   k_lp_frustum   one lane per slot, the slot loaded ONCE and tested under every frame's pose: bad / seen skip, isInFrustum as written,
//                  PredictScale with its clamp; per (frame, slot) a pass flag and the projection, per (frame, block) the survivors
//   k_lp_compact   the survivors in ASCENDING SLOT ORDER (sm_compact_pos).  u, v, ur, level, view cosine, descriptor and observation flag
//                  are gathered by slot straight into the arrays SbpDev names.
//   -- the in-view counts come down here: the search core's grid is one wave per query, so the host has to know them; more than 16384
//      in view is refused (HVO_ERR_UNSUPPORTED) with `held` untouched --
//   k_track_windows, k_search_by_projection, k_sbp_epilogue (match.hip, unchanged) on the device-resident queries
//   k_sm_assign    (slot_map.hip) per feature the LAST query in query order that matched it (two unobserved points may take one feature)
//   k_lp_apply     held[i] = the slot of the winning query
//
// Readings (OpenCV is not in the reference tree; DESIGN.md section 7, tests/point_map_ref.py restates the same):
//   mRcw * P + mtcw              as k_project_last (match.hip): the row's three products summed in FLOAT left to right, then
//                                (float)((double)sum * 1.0 + (double)t * 1.0)
//   PcZ < 0.0f                   as written: z == 0 and -0.0 pass and divide; a NaN projection passes the four bounds tests
//   invz, u, v, ur               one float division; sm_pinhole (fx * PcX * invz + cx in float, left to right); u - mbf * invz
//   mOw                          -Rcw^T tcw with double sums, times -1.0, rounded to float (match_project_setup's twc)
//   P - mOw                      float, element-wise
//   cv::norm                     sm_dist3: sqrt of the double sum of squares, stored to float; the 1.2 / 0.8 band is sm_dist_band
//   PO.dot(Pn) / dist            Mat::dot accumulates in double; / the float dist in double; rounded to the float viewCos
//   PredictScale                 sm_predict_level and sm_clamp_level (map_gates.hpp): float ratio; MapPoint.cc writes unique_lock<mutex> unqualified, so it sits under `using namespace std` with
//                                <cmath> reached through its headers, as MapLine.cpp does: log and ceil are the FLOAT overloads, the division
//                                by mfLogScaleFactor is float; the conversion to int saturates (NaN -> 0) and the clamp to
//                                [0, mnScaleLevels - 1] is part of the function.  The search reads the level (radius, band).
// No contraction (-ffp-contract=off, __f*_rn).
#include "slot_map.hpp"
#include "frame_view.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#define LP_BLOCK SM_BLOCK
#define LP_MAXQ 16384             // points in view per call (SBP_MAXQ of match.hip)
#define LP_MAXT 65535             // frame features (the search core's keys hold the feature in 16 bits)

extern "C" {

hvo_point_map *hvo_point_map_create(int device, int slots)
{
    if (device < 0 || slots < 0 || slots > HVO_POINT_MAP_MAX_SLOTS || hipSetDevice(device) != hipSuccess) return nullptr;
    hvo_point_map *m = new hvo_point_map();
    if (sm_init(m, device, slots)) { hvo_point_map_destroy(m); return nullptr; }
    return m;
}

void hvo_point_map_destroy(hvo_point_map *m) { if (m) { sm_release(m); delete m; } }

// test door, not product API and not in include/hvo.h
int hvo_debug_point_map_scratch(hvo_point_map *m, int fill_byte) { return sm_debug_fill_scratch(m, fill_byte); }

int hvo_point_map_set_many(hvo_point_map *m, int first, int n, const float *pos, const float *normal, const float *max_dist, const float *min_dist,
                           const uint8_t *desc, const uint8_t *observed, const uint8_t *bad)
{
    bool regrown;
    const int rc = sm_set_begin(m, first, n, pos && normal && max_dist && min_dist && desc, &regrown);
    if (rc || n == 0) return rc;
    const size_t cap = (size_t)m->cap;
    float *h_pos = m->host<float>(m->POS), *h_nrm = m->host<float>(m->NRM);
    for (int i = 0; i < n; i++) {
        const size_t j = (size_t)first + i;
        for (int k = 0; k < 3; k++) { h_pos[k * cap + j] = pos[3 * (size_t)i + k]; h_nrm[k * cap + j] = normal[3 * (size_t)i + k]; }
        m->host<float>(m->MAXD)[j] = max_dist[i]; m->host<float>(m->MIND)[j] = min_dist[i];
        memcpy(m->host<uint8_t>(m->DESC) + j * 32, desc + 32 * (size_t)i, 32);
        m->h_flags()[j] = sm_flag_byte(observed, bad, i);
    }
    return sm_set_end(m, first, n, regrown);
}

int hvo_point_map_set(hvo_point_map *m, int slot, const float pos[3], const float normal[3], float max_dist, float min_dist, const uint8_t desc[32],
                      int observed)
{
    const uint8_t o = observed ? 1 : 0;
    return hvo_point_map_set_many(m, slot, 1, pos, normal, &max_dist, &min_dist, desc, &o, nullptr);
}

int hvo_point_map_set_bad(hvo_point_map *m, int slot, int bad) { return sm_set_flag(m, slot, SM_BAD, bad); }
int hvo_point_map_set_observed(hvo_point_map *m, int slot, int observed) { return sm_set_flag(m, slot, SM_OBS, observed); }
int hvo_point_map_counts(const hvo_point_map *m, int *n_slots, int *n_good, int *n_observed) { return sm_counts(m, n_slots, n_good, n_observed); }

int hvo_point_map_slot(const hvo_point_map *m, int slot, float pos[3], float normal[3], float *max_dist, float *min_dist, uint8_t desc[32], int *bad,
                       int *observed)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    const size_t cap = (size_t)m->cap, j = (size_t)slot;
    if (pos) for (int k = 0; k < 3; k++) pos[k] = m->host<float>(m->POS)[k * cap + j];
    if (normal) for (int k = 0; k < 3; k++) normal[k] = m->host<float>(m->NRM)[k * cap + j];
    if (max_dist) *max_dist = m->host<float>(m->MAXD)[j];
    if (min_dist) *min_dist = m->host<float>(m->MIND)[j];
    if (desc) memcpy(desc, m->host<uint8_t>(m->DESC) + j * 32, 32);
    if (bad) *bad = (m->h_flags()[j] & SM_BAD) ? 1 : 0;
    if (observed) *observed = (m->h_flags()[j] & SM_OBS) ? 1 : 0;
    return HVO_OK;
}

const char *hvo_point_map_last_error(const hvo_point_map *m) { return m ? m->last_error.c_str() : ""; }

}  // extern "C"

// ---------------------------------------------------------------- kernels ----------------------------------------------------------------

struct LpDev {
    int ns, cap, nframes, nblocks, capq, n_levels;
    const float *pos, *nrm, *maxd, *mind; const uint8_t *desc, *flags;
    const SmPose *pose;                              // nframes
    float fx, fy, cx, cy, bf, minX, maxX, minY, maxY, logsf, vclimit;
    const uint8_t *seen;                             // nframes x ns
    uint8_t *pass; float4 *s_proj; int *s_lvl;       // nframes x ns, by slot: (u, v, ur, viewCos), level
    int *blockcnt;                                   // nframes x nblocks
    int *nview, *ntested;                            // nframes
    int *q_slot; float *q_u, *q_v, *q_ur, *q_vc, *q_proj; int *q_lvl; uint8_t *q_desc, *q_blocks;   // frame f's queries at f * capq (q_proj: u, v, ur packed, for the caller)
};

__global__ __launch_bounds__(LP_BLOCK) void k_lp_frustum(LpDev a)
{
    const int j = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool in = j < a.ns;
    const size_t cap = (size_t)a.cap, jj = in ? (size_t)j : 0;
    const float X = a.pos[jj], Y = a.pos[cap + jj], Z = a.pos[2 * cap + jj];
    const float n0 = a.nrm[jj], n1 = a.nrm[cap + jj], n2 = a.nrm[2 * cap + jj];
    const float mfMax = a.maxd[jj], mfMin = a.mind[jj];
    const bool good = in && !(a.flags[jj] & SM_BAD);
    for (int f = 0; f < a.nframes; f++) {
        const SmPose &P = a.pose[f];
        const size_t o = (size_t)f * a.ns + jj;
        const bool tested = good && !a.seen[o];
        bool pass = false;
        if (tested) {
            const float xc = sm_row(P.R, X, Y, Z, P.t[0]), yc = sm_row(P.R + 3, X, Y, Z, P.t[1]), zc = sm_row(P.R + 6, X, Y, Z, P.t[2]);
            if (!(zc < 0.0f)) {                                    // Frame.cc:1385: z == 0 and -0.0 pass and divide
                const float invz = __fdiv_rn(1.0f, zc);
                const float u = sm_pinhole(a.fx, xc, invz, a.cx), v = sm_pinhole(a.fy, yc, invz, a.cy);
                const bool out = (u < a.minX || u > a.maxX) || (v < a.minY || v > a.maxY);       // (a NaN compares false four times)
                if (!out) {
                    float maxD, minD; sm_dist_band(mfMax, mfMin, &maxD, &minD);
                    const double d0 = __fsub_rn(X, P.Ow[0]), d1 = __fsub_rn(Y, P.Ow[1]), d2 = __fsub_rn(Z, P.Ow[2]);
                    const float dist = sm_dist3(d0, d1, d2);
                    if (!(dist < minD || dist > maxD)) {
                        const double dot = (d0 * (double)n0 + d1 * (double)n1) + d2 * (double)n2;
                        const float vc = (float)(dot / (double)dist);
                        if (!(vc < a.vclimit)) {
                            const int l = sm_clamp_level(sm_predict_level(mfMax, dist, a.logsf), a.n_levels);     // MapPoint.cc:400-415
                            pass = true;
                            a.s_proj[o] = make_float4(u, v, __fsub_rn(u, __fmul_rn(a.bf, invz)), vc);
                            a.s_lvl[o] = l;
                        }
                    }
                }
            }
        }
        sm_frustum_tail(in, pass, tested, &a.pass[o], &a.blockcnt[(size_t)f * a.nblocks + blockIdx.x], &a.ntested[f]);
    }
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_compact(LpDev a)
{
    const int f = blockIdx.y, j = blockIdx.x * LP_BLOCK + threadIdx.x;
    bool p;
    const int q = sm_compact_pos(a.blockcnt, a.nblocks, a.ns, f, a.pass, a.nview, &p);
    if (p && q < a.capq) {
        const size_t d = (size_t)f * a.capq + q;
        const float4 pr = a.s_proj[(size_t)f * a.ns + j];
        a.q_slot[d] = j;
        a.q_u[d] = pr.x; a.q_v[d] = pr.y; a.q_ur[d] = pr.z; a.q_vc[d] = pr.w; a.q_lvl[d] = a.s_lvl[(size_t)f * a.ns + j];
        a.q_proj[3 * d] = pr.x; a.q_proj[3 * d + 1] = pr.y; a.q_proj[3 * d + 2] = pr.z;
        *(ulonglong4 *)(a.q_desc + 32 * d) = *(const ulonglong4 *)(a.desc + 32 * (size_t)j);
        a.q_blocks[d] = (a.flags[j] & SM_OBS) ? 1 : 0;
    }
}

__global__ __launch_bounds__(LP_BLOCK) void k_lp_apply(int nt, int nq, const int *__restrict__ win, const int *__restrict__ q_slot, int32_t *__restrict__ held)
{
    const int i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= nt) return;
    const int w = win[i];
    if (w >= 0 && w < nq) held[i] = q_slot[w];                     // F.mvpMapPoints[bestIdx] = pMP, the last one in query order
}

// ---------------------------------------------------------------- the call ----------------------------------------------------------------

int lp_map_device(const hvo_point_map *m) { return m->device; }
const char *lp_map_error(const hvo_point_map *m) { return m->last_error.c_str(); }

static std::string lp_limit_text(int nq, int nt)
{
    return "local points: " + std::to_string(nq) + " points in view, " + std::to_string(nt) + " frame features (limits: " + std::to_string(LP_MAXQ) + ", " +
           std::to_string(LP_MAXT) + "); nothing was written";
}

int lp_run(hipStream_t st, hvo_point_map *m, const hvo_camera *cam, const hvo_local_points_params *P, int nframes,
           const FrameView *fr, const float *Tcw, hvo_local_points_io *io, hvo_local_points_result *res)
{
    const int ns = m->n_slots, nblocks = std::max(1, (ns + LP_BLOCK - 1) / LP_BLOCK), capq = std::max(1, std::min(ns, LP_MAXQ));
    const float *bounds = fr[0].bounds, *sf = fr[0].sf;           // one call's frames share their geometry and pyramid
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { m->last_error = "local points: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (!(bounds[1] > bounds[0]) || !(bounds[3] > bounds[2])) { m->last_error = "local points: empty image bounds"; return HVO_ERR_INVALID_ARG; }
    std::vector<SmFrame> S(nframes);
    int rc;
    for (int f = 0; f < nframes; f++) {
        memset(&res[f], 0, sizeof(res[f]));
        if (fr[f].n_kp > LP_MAXT) { m->last_error = lp_limit_text(0, fr[f].n_kp); res[f].status = HVO_ERR_UNSUPPORTED; return HVO_ERR_UNSUPPORTED; }
        if (fr[f].n_kp > io[f].n_kp) { m->last_error = "local points: held is shorter than the frame's key-point count"; return HVO_ERR_INVALID_ARG; }
        if ((fr[f].n_kp > 0 && !io[f].held) || !io[f].in_view_slot || io[f].n_seen_extra < 0 || (io[f].n_seen_extra > 0 && !io[f].seen_extra)) {
            m->last_error = "local points: held or in_view_slot missing"; return HVO_ERR_INVALID_ARG;
        }
        S[f] = SmFrame{ fr[f].n_kp, io[f].n_seen_extra, io[f].held, io[f].seen_extra };
        if ((rc = sm_check_seen(m, "local points", "held names a slot beyond the map or an unknown value", HVO_HELD_FOREIGN_UNOBSERVED, S[f]))) return rc;
    }
    // ---- scratch A: everything whose size is known before the in-view counts ----
    SmCarve C;
    const size_t F = (size_t)nframes, NS = (size_t)std::max(ns, 1);
    const size_t o_pose = C.take(F * sizeof(SmPose)), o_seen = C.take(F * NS), o_pass = C.take(F * NS), o_sp = C.take(F * NS * 16), o_slv = C.take(F * NS * 4);
    const size_t o_bc = C.take(F * nblocks * 4), o_cnt = C.take(F * 2 * 4);
    const size_t o_qs = C.take(F * capq * 4), o_qu = C.take(F * capq * 4), o_qv = C.take(F * capq * 4), o_qr = C.take(F * capq * 4), o_qc = C.take(F * capq * 4),
                 o_ql = C.take(F * capq * 4), o_qd = C.take(F * capq * 32), o_qb = C.take(F * capq), o_qp = C.take(F * capq * 12);
    const size_t o_rad = C.take(F * capq * 4), o_min = C.take(F * capq * 4), o_max = C.take(F * capq * 4);
    const size_t o_mi = C.take(F * capq * 4), o_md = C.take(F * capq * 4);
    std::vector<size_t> o_k(F), o_ur(F);
    for (int f = 0; f < nframes; f++) {
        sm_carve_frame(C, S[f]);
        o_k[f] = C.take(4);                                        // n_matches
        o_ur[f] = fr[f].depth ? C.take(2 * (size_t)std::max(fr[f].n_kp, 1) * 4) : 0;      // mvuRight, mvDepth formed from the depth image
    }
    if ((rc = sm_grow(m, st, &m->d_a, &m->a_bytes, C.o))) return rc;
    char *A = m->d_a;
    if ((rc = sm_stage_in(m, st, A, o_pose, o_seen, o_cnt, S, Tcw))) return rc;
    for (int f = 0; f < nframes; f++) SM_HIP(hipMemsetAsync(A + o_k[f], 0, 4, st));
    if ((rc = sm_mark(m, st, A, o_seen, S, 1))) return rc;
    LpDev a; memset(&a, 0, sizeof(a));
    a.ns = ns; a.cap = m->cap; a.nframes = nframes; a.nblocks = nblocks; a.capq = capq; a.n_levels = P->n_levels;
    a.pos = m->dev<float>(m->POS); a.nrm = m->dev<float>(m->NRM); a.maxd = m->dev<float>(m->MAXD); a.mind = m->dev<float>(m->MIND); a.desc = m->dev<uint8_t>(m->DESC); a.flags = m->d_flags();
    a.pose = (const SmPose *)(A + o_pose);
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.bf = P->bf; a.minX = bounds[0]; a.maxX = bounds[1]; a.minY = bounds[2]; a.maxY = bounds[3];
    a.logsf = P->log_scale_factor; a.vclimit = P->view_cos_limit;
    a.seen = (const uint8_t *)(A + o_seen); a.pass = (uint8_t *)(A + o_pass); a.s_proj = (float4 *)(A + o_sp); a.s_lvl = (int *)(A + o_slv);
    a.blockcnt = (int *)(A + o_bc); a.nview = (int *)(A + o_cnt); a.ntested = a.nview + nframes;
    a.q_slot = (int *)(A + o_qs); a.q_u = (float *)(A + o_qu); a.q_v = (float *)(A + o_qv); a.q_ur = (float *)(A + o_qr); a.q_vc = (float *)(A + o_qc);
    a.q_lvl = (int *)(A + o_ql); a.q_proj = (float *)(A + o_qp); a.q_desc = (uint8_t *)(A + o_qd); a.q_blocks = (uint8_t *)(A + o_qb);
    if (ns > 0) {
        hipLaunchKernelGGL(k_lp_frustum, dim3(nblocks), dim3(LP_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_lp_compact, dim3(nblocks, nframes), dim3(LP_BLOCK), 0, st, a);
    }
    std::vector<int> cnt;
    if ((rc = sm_counts_down(m, st, "local points: frustum launch", A + o_cnt, nframes, cnt))) return rc;
    size_t sb = 0;
    for (int f = 0; f < nframes; f++) {
        res[f].n_slots_tested = cnt[nframes + f]; res[f].n_in_view = cnt[f];
        if (cnt[f] > LP_MAXQ) {                                    // refused whole: nothing of the caller's is written
            res[f].status = HVO_ERR_UNSUPPORTED; m->last_error = lp_limit_text(cnt[f], fr[f].n_kp); return HVO_ERR_UNSUPPORTED;
        }
        if (cnt[f] > 0 && fr[f].n_kp > 0) sb = std::max(sb, match_sbp_scratch_bytes(cnt[f]));
    }
    // ---- scratch B: the search's key rows (the frames' searches run one after the other on the stream and share them) ----
    if ((rc = sm_grow(m, st, &m->d_b, &m->b_bytes, stage_align(sb) + 256))) return rc;
    ProjDev W; memset(&W, 0, sizeof(W));
    for (int l = 0; l < HVO_MAX_LEVELS; l++) W.sf[l] = sf[l];
    for (int f = 0; f < nframes; f++) {
        const int nq = cnt[f], nt = fr[f].n_kp;
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
            s.t_kp = fr[f].kp_un; s.t_uright = d_uright; s.t_occ = (const uint8_t *)(A + S[f].o_occ); s.t_desc = fr[f].desc;
            s.nq = nq; s.nt = nt; s.mnMinX = bounds[0]; s.mnMaxX = bounds[1]; s.mnMinY = bounds[2]; s.mnMaxY = bounds[3];
            s.th_high = P->th_high; s.check_orientation = 0; s.map_mode = 1; s.nn_ratio = P->nn_ratio;
            s.match_idx = d_mi; s.match_dist = d_md; s.n_matches = (int *)(A + o_k[f]);
            if ((rc = match_sbp_enqueue(st, s, m->d_b))) { m->last_error = rc == HVO_ERR_UNSUPPORTED ? lp_limit_text(nq, nt) : "local points: search launch"; return rc; }
        } else if (nq > 0)
            sm_fill_enqueue(st, nq, d_mi, d_md);
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "local points: search launch"; return HVO_ERR_HIP; }
    SM_HIP(hipEventRecord(m->ev[2], st));
    for (int f = 0; f < nframes; f++) {
        const int nq = cnt[f], nt = fr[f].n_kp;
        if (nt < 1 || nq < 1) continue;
        const size_t q0 = (size_t)f * capq;
        int *d_win = (int *)(A + S[f].o_win);
        sm_assign_enqueue(st, nq, nt, (const int32_t *)(A + o_mi) + q0, d_win);
        hipLaunchKernelGGL(k_lp_apply, dim3((nt + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, nt, nq, d_win, a.q_slot + q0, (int32_t *)(A + S[f].o_held));
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "local points: assignment launch"; return HVO_ERR_HIP; }
    SM_HIP(hipEventRecord(m->ev[3], st));
    std::vector<int> kk(F, 0);
    for (int f = 0; f < nframes; f++) {
        const size_t nq = (size_t)cnt[f], nt = (size_t)fr[f].n_kp, q0 = (size_t)f * capq;
        hvo_local_points_io &I = io[f];
        SM_HIP(hipMemcpyAsync(&kk[f], A + o_k[f], 4, hipMemcpyDeviceToHost, st));
        if (nt && ns > 0) SM_HIP(hipMemcpyAsync(I.held, A + S[f].o_held, nt * 4, hipMemcpyDeviceToHost, st));
        if (nq) {
            SM_HIP(hipMemcpyAsync(I.in_view_slot, a.q_slot + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.proj) SM_HIP(hipMemcpyAsync(I.proj, a.q_proj + 3 * q0, nq * 12, hipMemcpyDeviceToHost, st));
            if (I.view_cos) SM_HIP(hipMemcpyAsync(I.view_cos, a.q_vc + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.level) SM_HIP(hipMemcpyAsync(I.level, a.q_lvl + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.match_idx) SM_HIP(hipMemcpyAsync(I.match_idx, (int32_t *)(A + o_mi) + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.match_dist) SM_HIP(hipMemcpyAsync(I.match_dist, (int32_t *)(A + o_md) + q0, nq * 4, hipMemcpyDeviceToHost, st));
        }
    }
    SM_HIP(hipStreamSynchronize(st));
    float ms[3];
    sm_kernel_ms(m, ms);
    for (int f = 0; f < nframes; f++) {
        res[f].n_matches = kk[f]; res[f].status = HVO_OK;
        for (int k = 0; k < 3; k++) res[f].kernel_ms[k] = ms[k];
    }
    return HVO_OK;
}
