// local_lines.hip -- the line side of Tracking::TrackLocalMapWithLines against map lines that stay on the device (hvo_line_map):
//   Tracking::SearchLocalLines (reference src/Tracking.cc:3279-3392) with Frame::isInFrustum(MapLine *, 0.5) (src/Frame.cc:1429-1499),
//   MapLine::PredictScale (src/MapLine.cpp:549-558), the search core of line_map.inc, the CosSita > 0.09 post-gate (3357-3386), and
//   Manhattan::computeStructConstInMap (src/Manhattan.cpp:163-224, rotCW 217-224, computeAngle 1054-1071).
//
// The map is a slot map (slot_map.hpp: the storage, its growth and uploads, the flag byte, the call's skeleton).  Per slot (= position in
// mvpLocalMapLines) the line map keeps GetWorldPos() (6 doubles), GetWorldVector() (3), GetNormal() (3), mfMaxDistance and mfMinDistance (raw
// floats) and GetDescriptor() (32 bytes).  Every component is an array of its own over the slots (pos: six arrays of `cap` doubles, and so
// on): the frustum kernel runs one lane per slot, so a wave's load of one component covers 512 contiguous bytes; packed 48-byte positions
// would put the lanes' loads 48 bytes apart and touch every line six times.  The descriptor is consumed whole, 32 bytes by one lane of the
// gather, and stays packed.
//
// The call, the same kernels for the host, stream and batch forms (bit-identical results):
//   k_sm_mark      (slot_map.hip) held slots that are bad become -1; t_occupied = held and the slot has observations; held and seen_extra
//                  slots are marked seen
//   k_ll_frustum   one lane per slot, the slot loaded ONCE and tested under every frame's pose: bad / seen skip, isInFrustum as written,
//                  PredictScale; per (frame, slot) a pass flag and the projections, per (frame, block) the number of survivors
//   k_ll_compact   the survivors in ASCENDING SLOT ORDER (sm_compact_pos).  The world vector, descriptor and observation flag are gathered
//                  by slot into the query arrays the search core reads.
//   -- the in-view counts come down here: the search core's grid is one wave per query, so the host has to know them; more than 16384
//      in view is refused (HVO_ERR_UNSUPPORTED) with `held` untouched --
//   k_lsbp_map_keys, k_lsbp_map_epilogue (line_map.inc, unchanged) on the device-resident queries; not run when nothing is in view
//   k_sm_assign    (slot_map.hip) per frame line the LAST query in query order that matched it
//   k_ll_gate      held[i] = the winning query's slot; then, only when the search matched something: for every line with held >= 0, lines
//                  held before the call included, CosSita
//   k_ll_struct    computeStructConstInMap: one thread per (frame line, in-view entry), the dense relation byte and the two counts
//
// Readings (OpenCV and Eigen are not in the reference tree; DESIGN.md section 7, tests/line_map_ref.py restates the same):
//   Mat_<float> << double        each entry rounded to float
//   mRcw * SP + mtcw             as k_project_last (match.hip): the row's three products summed in FLOAT left to right, then
//                                (float)((double)sum * 1.0 + (double)t * 1.0) -- gemm's small-matrix path with alpha = beta = 1
//   mOw                          -Rcw^T tcw with double sums, times -1.0, rounded to float (match_project_setup's twc)
//   0.5 * (SP + EP) - mOw        float, element-wise
//   cv::norm                     sm_dist3: sqrt of the double sum of squares, stored to float; the 1.2 / 0.8 band is sm_dist_band
//   Mat::dot on CV_32F           accumulates in double; / the float dist in double; rounded to the float viewCos
//   PredictScale                 sm_predict_level (map_gates.hpp), stored without sm_clamp_level: float ratio; log is the FLOAT overload (MapLine.cpp sees <cmath> and `using namespace std` through its
//                                headers, as DESIGN.md takes elsewhere); float division by logScaleFactor; ceil's float overload
//   K.inv() (3 x 3 CV_32F)       closed form, cofactors and determinant in double, each entry times 1/det rounded to float
//   K.inv() * tkl, Rcw * wvec    GEMM with a double work type: products and sums in double, left to right, rounded to float once
//   Mat::cross                   in float; NormalVector_ /= norm_: each element divided in double, rounded to float
//   rotCW                        Rcw converted to double times the double line equation, sums left to right (it multiplies by Rcw, as written)
// No contraction (-ffp-contract=off, __f*_rn).  The predicted level is reported and never read.
#include "slot_map.hpp"
#include "frame_view.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#define LL_BLOCK SM_BLOCK

extern "C" {

hvo_line_map *hvo_line_map_create(int device, int slots)
{
    if (device < 0 || slots < 0 || slots > HVO_LINE_MAP_MAX_SLOTS || hipSetDevice(device) != hipSuccess) return nullptr;
    hvo_line_map *m = new hvo_line_map();
    if (sm_init(m, device, slots)) { hvo_line_map_destroy(m); return nullptr; }
    return m;
}

void hvo_line_map_destroy(hvo_line_map *m) { if (m) { sm_release(m); delete m; } }

// test door, not product API and not in include/hvo.h
int hvo_debug_line_map_scratch(hvo_line_map *m, int fill_byte) { return sm_debug_fill_scratch(m, fill_byte); }

int hvo_line_map_set_many(hvo_line_map *m, int first, int n, const double *pos, const double *wvec, const double *normal, const float *max_dist,
                          const float *min_dist, const uint8_t *desc, const uint8_t *observed, const uint8_t *bad)
{
    bool regrown;
    const int rc = sm_set_begin(m, first, n, pos && wvec && normal && max_dist && min_dist && desc, &regrown);
    if (rc || n == 0) return rc;
    const size_t cap = (size_t)m->cap;
    double *h_pos = m->host<double>(m->POS), *h_wvec = m->host<double>(m->WVEC), *h_nrm = m->host<double>(m->NRM);
    for (int i = 0; i < n; i++) {
        const size_t j = (size_t)first + i;
        for (int k = 0; k < 6; k++) h_pos[k * cap + j] = pos[6 * (size_t)i + k];
        for (int k = 0; k < 3; k++) { h_wvec[k * cap + j] = wvec[3 * (size_t)i + k]; h_nrm[k * cap + j] = normal[3 * (size_t)i + k]; }
        m->host<float>(m->MAXD)[j] = max_dist[i]; m->host<float>(m->MIND)[j] = min_dist[i];
        memcpy(m->host<uint8_t>(m->DESC) + j * 32, desc + 32 * (size_t)i, 32);
        m->h_flags()[j] = sm_flag_byte(observed, bad, i);
    }
    return sm_set_end(m, first, n, regrown);
}

int hvo_line_map_set(hvo_line_map *m, int slot, const double pos[6], const double wvec[3], const double normal[3], float max_dist, float min_dist,
                     const uint8_t desc[32], int observed)
{
    const uint8_t o = observed ? 1 : 0;
    return hvo_line_map_set_many(m, slot, 1, pos, wvec, normal, &max_dist, &min_dist, desc, &o, nullptr);
}

int hvo_line_map_set_bad(hvo_line_map *m, int slot, int bad) { return sm_set_flag(m, slot, SM_BAD, bad); }
int hvo_line_map_set_observed(hvo_line_map *m, int slot, int observed) { return sm_set_flag(m, slot, SM_OBS, observed); }
int hvo_line_map_counts(const hvo_line_map *m, int *n_slots, int *n_good, int *n_observed) { return sm_counts(m, n_slots, n_good, n_observed); }

int hvo_line_map_slot(const hvo_line_map *m, int slot, double pos[6], double wvec[3], double normal[3], float *max_dist, float *min_dist,
                      uint8_t desc[32], int *bad, int *observed)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    const size_t cap = (size_t)m->cap, j = (size_t)slot;
    if (pos) for (int k = 0; k < 6; k++) pos[k] = m->host<double>(m->POS)[k * cap + j];
    if (wvec) for (int k = 0; k < 3; k++) wvec[k] = m->host<double>(m->WVEC)[k * cap + j];
    if (normal) for (int k = 0; k < 3; k++) normal[k] = m->host<double>(m->NRM)[k * cap + j];
    if (max_dist) *max_dist = m->host<float>(m->MAXD)[j];
    if (min_dist) *min_dist = m->host<float>(m->MIND)[j];
    if (desc) memcpy(desc, m->host<uint8_t>(m->DESC) + j * 32, 32);
    if (bad) *bad = (m->h_flags()[j] & SM_BAD) ? 1 : 0;
    if (observed) *observed = (m->h_flags()[j] & SM_OBS) ? 1 : 0;
    return HVO_OK;
}

const char *hvo_line_map_last_error(const hvo_line_map *m) { return m ? m->last_error.c_str() : ""; }

}  // extern "C"

// ---------------------------------------------------------------- kernels ----------------------------------------------------------------

struct LlDev {
    int ns, cap, nframes, nblocks, capq;
    const double *pos, *wvec, *nrm; const float *maxd, *mind; const uint8_t *desc, *flags;
    const SmPose *pose;                              // nframes
    float fx, fy, cx, cy, minX, maxX, minY, maxY, logsf;
    const uint8_t *seen;                             // nframes x ns
    uint8_t *pass; float4 *s_xyxy; float *s_vc; int *s_lvl;      // nframes x ns, by slot
    int *blockcnt;                                   // nframes x nblocks
    int *nview, *ntested;                            // nframes
    int *q_slot; float *q_xyxy; float *q_vc; int *q_lvl; double *q_wvec; uint8_t *q_desc, *q_blocks;   // frame f's queries at f * capq
};

__global__ __launch_bounds__(LL_BLOCK) void k_ll_frustum(LlDev a)
{
    const int j = blockIdx.x * LL_BLOCK + threadIdx.x;
    const bool in = j < a.ns;
    const size_t cap = (size_t)a.cap, jj = in ? (size_t)j : 0;
    float sp[3], ep[3], pn[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { sp[k] = (float)a.pos[k * cap + jj]; ep[k] = (float)a.pos[(k + 3) * cap + jj]; pn[k] = (float)a.nrm[k * cap + jj]; }
    const float mfMax = a.maxd[jj], mfMin = a.mind[jj];
    const bool good = in && !(a.flags[jj] & SM_BAD);
    for (int f = 0; f < a.nframes; f++) {
        const SmPose &P = a.pose[f];
        const size_t o = (size_t)f * a.ns + jj;
        const bool tested = good && !a.seen[o];
        bool pass = false;
        if (tested) {
            const float sx = sm_row(P.R, sp[0], sp[1], sp[2], P.t[0]), sy = sm_row(P.R + 3, sp[0], sp[1], sp[2], P.t[1]), sz = sm_row(P.R + 6, sp[0], sp[1], sp[2], P.t[2]);
            const float ex = sm_row(P.R, ep[0], ep[1], ep[2], P.t[0]), ey = sm_row(P.R + 3, ep[0], ep[1], ep[2], P.t[1]), ez = sm_row(P.R + 6, ep[0], ep[1], ep[2], P.t[2]);
            if (!(sz < 0.0f || ez < 0.0f)) {
                const float invz1 = __fdiv_rn(1.0f, sz);
                const float u1 = sm_pinhole(a.fx, sx, invz1, a.cx), v1 = sm_pinhole(a.fy, sy, invz1, a.cy);
                const float invz2 = __fdiv_rn(1.0f, ez);
                const float u2 = sm_pinhole(a.fx, ex, invz2, a.cx), v2 = sm_pinhole(a.fy, ey, invz2, a.cy);
                const bool out = (u1 < a.minX || u1 > a.maxX) || (v1 < a.minY || v1 > a.maxY) || (u2 < a.minX || u2 > a.maxX) || (v2 < a.minY || v2 > a.maxY);
                if (!out) {
                    float maxD, minD; sm_dist_band(mfMax, mfMin, &maxD, &minD);
                    float om[3];                                   // the midpoint in FLOAT (line_fuse.hip forms it in double)
#pragma unroll
                    for (int k = 0; k < 3; k++) om[k] = __fsub_rn(__fmul_rn(0.5f, __fadd_rn(sp[k], ep[k])), P.Ow[k]);
                    const double d0 = om[0], d1 = om[1], d2 = om[2];
                    const float dist = sm_dist3(d0, d1, d2);
                    if (!(dist < minD || dist > maxD)) {
                        const double dot = (d0 * (double)pn[0] + d1 * (double)pn[1]) + d2 * (double)pn[2];
                        const float vc = (float)(dot / (double)dist);
                        if (!(vc < 0.5f)) {
                            const float lv = sm_predict_lv(mfMax, dist, a.logsf);
                            pass = true;
                            a.s_xyxy[o] = make_float4(u1, v1, u2, v2); a.s_vc[o] = vc;
                            a.s_lvl[o] = sm_level(lv);                 // = sm_predict_level, unclamped (reported and never read), converted after the stores as before
                        }
                    }
                }
            }
        }
        sm_frustum_tail(in, pass, tested, &a.pass[o], &a.blockcnt[(size_t)f * a.nblocks + blockIdx.x], &a.ntested[f]);
    }
}

__global__ __launch_bounds__(LL_BLOCK) void k_ll_compact(LlDev a)
{
    const int f = blockIdx.y, j = blockIdx.x * LL_BLOCK + threadIdx.x;
    bool p;
    const int q = sm_compact_pos(a.blockcnt, a.nblocks, a.ns, f, a.pass, a.nview, &p);
    if (p && q < a.capq) {
        const size_t d = (size_t)f * a.capq + q, cap = (size_t)a.cap, src = (size_t)f * a.ns + j;
        a.q_slot[d] = j;
        *(float4 *)(a.q_xyxy + 4 * d) = a.s_xyxy[src]; a.q_vc[d] = a.s_vc[src]; a.q_lvl[d] = a.s_lvl[src];
        a.q_wvec[3 * d] = a.wvec[j]; a.q_wvec[3 * d + 1] = a.wvec[cap + j]; a.q_wvec[3 * d + 2] = a.wvec[2 * cap + j];
        *(ulonglong4 *)(a.q_desc + 32 * d) = *(const ulonglong4 *)(a.desc + 32 * (size_t)j);
        a.q_blocks[d] = (a.flags[j] & SM_OBS) ? 1 : 0;
    }
}

struct LlGate { float Ki[9], R[9]; };

__global__ __launch_bounds__(LL_BLOCK) void k_ll_gate(int nt, size_t cap, const double *__restrict__ wvec, const hvo_keyline *__restrict__ kl, const int *__restrict__ win,
                                                        const int *__restrict__ q_slot, const int *__restrict__ n_matches, LlGate G, int32_t *__restrict__ held,
                                                        int *__restrict__ n_gated)
{
    const int i = blockIdx.x * LL_BLOCK + threadIdx.x;
    if (i >= nt) return;
    int h = held[i];
    const int w = win[i];
    if (w >= 0) h = q_slot[w];                                     // F.mvpMapLines[bestIdx] = pML, the last one in query order
    if (*n_matches > 0 && h >= 0) {                                // Tracking.cc:3357-3386
        const float w0 = (float)wvec[h], w1 = (float)wvec[cap + h], w2 = (float)wvec[2 * cap + h];
        const hvo_keyline &L = kl[i];
        float S[3], E[3], C[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double k0 = G.Ki[3 * r], k1 = G.Ki[3 * r + 1], k2 = G.Ki[3 * r + 2], r0 = G.R[3 * r], r1 = G.R[3 * r + 1], r2 = G.R[3 * r + 2];
            S[r] = (float)((k0 * (double)L.sx + k1 * (double)L.sy) + k2 * 1.0);
            E[r] = (float)((k0 * (double)L.ex + k1 * (double)L.ey) + k2 * 1.0);
            C[r] = (float)((r0 * (double)w0 + r1 * (double)w1) + r2 * (double)w2);
        }
        float N[3] = { __fsub_rn(__fmul_rn(S[1], E[2]), __fmul_rn(S[2], E[1])), __fsub_rn(__fmul_rn(S[2], E[0]), __fmul_rn(S[0], E[2])),
                       __fsub_rn(__fmul_rn(S[0], E[1]), __fmul_rn(S[1], E[0])) };
        const double n0 = N[0], n1 = N[1], n2 = N[2];
        const double nrm = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
#pragma unroll
        for (int r = 0; r < 3; r++) N[r] = (float)((double)N[r] / nrm);
        const double cs = fabs(((double)N[0] * (double)C[0] + (double)N[1] * (double)C[1]) + (double)N[2] * (double)C[2]);
        if (cs > 0.09) { h = -1; atomicAdd(n_gated, 1); }
    }
    held[i] = h;
}

// computeStructConstInMap: grid (in-view chunks, frame lines)
__global__ __launch_bounds__(LL_BLOCK) void k_ll_struct(int nq, const hvo_line3d *__restrict__ l3d, const double *__restrict__ q_wvec, LlGate G, int8_t *__restrict__ rel,
                                                          int32_t *__restrict__ n_par, int32_t *__restrict__ n_perp)
{
    const int i = blockIdx.y, j = blockIdx.x * LL_BLOCK + threadIdx.x;
    const float *q = l3d[i].line_eq;
    const double e0 = q[0], e1 = q[1], e2 = q[2];
    double lw[3];
#pragma unroll
    for (int r = 0; r < 3; r++) lw[r] = ((double)G.R[3 * r] * e0 + (double)G.R[3 * r + 1] * e1) + (double)G.R[3 * r + 2] * e2;
    int r = 0;
    if (j < nq) {
        const double v0 = q_wvec[3 * (size_t)j], v1 = q_wvec[3 * (size_t)j + 1], v2 = q_wvec[3 * (size_t)j + 2];
        const double dot = (lw[0] * v0 + lw[1] * v1) + lw[2] * v2;
        const double ma = sqrt((lw[0] * lw[0] + lw[1] * lw[1]) + lw[2] * lw[2]), mb = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        const double ang = fabs(dot / (ma * mb));
        r = ang < 0.062 ? 2 : ang > 0.9985 ? 1 : 0;                // (a NaN compares false both ways)
        if (rel) rel[(size_t)i * nq + j] = (int8_t)r;
    }
    const int np = __syncthreads_count(r == 2), na = __syncthreads_count(r == 1);
    if (threadIdx.x == 0) { if (np) atomicAdd(&n_perp[i], np); if (na) atomicAdd(&n_par[i], na); }
}

// ---------------------------------------------------------------- the call ----------------------------------------------------------------

// K.inv() of the CV_32F camera matrix in closed form (double), entries rounded to float
static void ll_kinv(const hvo_camera *cam, float Ki[9])
{
    const double a00 = cam->fx, a01 = 0, a02 = cam->cx, a10 = 0, a11 = cam->fy, a12 = cam->cy, a20 = 0, a21 = 0, a22 = 1;
    const double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    const double d = 1.0 / det;
    const double t[9] = { (a11 * a22 - a12 * a21) * d, (a02 * a21 - a01 * a22) * d, (a01 * a12 - a02 * a11) * d,
                          (a12 * a20 - a10 * a22) * d, (a00 * a22 - a02 * a20) * d, (a02 * a10 - a00 * a12) * d,
                          (a10 * a21 - a11 * a20) * d, (a01 * a20 - a00 * a21) * d, (a00 * a11 - a01 * a10) * d };
    for (int k = 0; k < 9; k++) Ki[k] = (float)t[k];
}

int ll_map_device(const hvo_line_map *m) { return m->device; }
const char *ll_map_error(const hvo_line_map *m) { return m->last_error.c_str(); }

int ll_run(hipStream_t st, hvo_line_map *m, const hvo_camera *cam, const hvo_local_lines_params *P, int nframes,
           const FrameView *fr, const float *Tcw, hvo_local_lines_io *io, hvo_local_lines_result *res)
{
    const int ns = m->n_slots, nblocks = std::max(1, (ns + LL_BLOCK - 1) / LL_BLOCK), capq = std::max(1, std::min(ns, LSBP_MAP_MAXQ));
    const float *bounds = fr[0].bounds;                           // one call's frames share their geometry
    std::vector<SmFrame> S(nframes);
    int rc;
    for (int f = 0; f < nframes; f++) {
        memset(&res[f], 0, sizeof(res[f]));
        if (fr[f].n_kl > 2048) { m->last_error = match_lsbp_map_limit_text(0, fr[f].n_kl); res[f].status = HVO_ERR_UNSUPPORTED; return HVO_ERR_UNSUPPORTED; }
        if (fr[f].n_kl > io[f].n_kl) { m->last_error = "local lines: held is shorter than the frame's key-line count"; return HVO_ERR_INVALID_ARG; }
        if ((fr[f].n_kl > 0 && (!io[f].held || !io[f].n_par || !io[f].n_perp)) || !io[f].in_view_slot || io[f].n_seen_extra < 0 || (io[f].n_seen_extra > 0 && !io[f].seen_extra)) {
            m->last_error = "local lines: held, n_par, n_perp or in_view_slot missing"; return HVO_ERR_INVALID_ARG;
        }
        S[f] = SmFrame{ fr[f].n_kl, io[f].n_seen_extra, io[f].held, io[f].seen_extra };
        if ((rc = sm_check_seen(m, "local lines", "held names a slot beyond the map", INT32_MIN, S[f]))) return rc;
    }
    // ---- scratch A: everything whose size is known before the in-view counts ----
    SmCarve C;
    const size_t F = (size_t)nframes, NS = (size_t)std::max(ns, 1);
    const size_t o_pose = C.take(F * sizeof(SmPose)), o_seen = C.take(F * NS), o_pass = C.take(F * NS), o_sx = C.take(F * NS * 16), o_svc = C.take(F * NS * 4), o_slv = C.take(F * NS * 4);
    const size_t o_bc = C.take(F * nblocks * 4), o_cnt = C.take(F * 2 * 4);
    const size_t o_qs = C.take(F * capq * 4), o_qx = C.take(F * capq * 16), o_qv = C.take(F * capq * 4), o_ql = C.take(F * capq * 4), o_qw = C.take(F * capq * 24),
                 o_qd = C.take(F * capq * 32), o_qb = C.take(F * capq);
    const size_t o_mi = C.take(F * capq * 4), o_md = C.take(F * capq * 4);
    std::vector<size_t> o_np(F), o_nq(F), o_k(F);
    for (int f = 0; f < nframes; f++) {
        const size_t nt = (size_t)std::max(fr[f].n_kl, 1);
        sm_carve_frame(C, S[f]);
        o_np[f] = C.take(nt * 4); o_nq[f] = C.take(nt * 4); o_k[f] = C.take(2 * 4);        // n_matches, n_gated
    }
    if ((rc = sm_grow(m, st, &m->d_a, &m->a_bytes, C.o))) return rc;
    char *A = m->d_a;
    if ((rc = sm_stage_in(m, st, A, o_pose, o_seen, o_cnt, S, Tcw))) return rc;
    for (int f = 0; f < nframes; f++) {
        SM_HIP(hipMemsetAsync(A + o_np[f], 0, (size_t)std::max(fr[f].n_kl, 1) * 4, st));
        SM_HIP(hipMemsetAsync(A + o_nq[f], 0, (size_t)std::max(fr[f].n_kl, 1) * 4, st));
        SM_HIP(hipMemsetAsync(A + o_k[f], 0, 8, st));
    }
    if ((rc = sm_mark(m, st, A, o_seen, S, 0))) return rc;
    LlDev a; memset(&a, 0, sizeof(a));
    a.ns = ns; a.cap = m->cap; a.nframes = nframes; a.nblocks = nblocks; a.capq = capq;
    a.pos = m->dev<double>(m->POS); a.wvec = m->dev<double>(m->WVEC); a.nrm = m->dev<double>(m->NRM); a.maxd = m->dev<float>(m->MAXD); a.mind = m->dev<float>(m->MIND);
    a.desc = m->dev<uint8_t>(m->DESC); a.flags = m->d_flags();
    a.pose = (const SmPose *)(A + o_pose);
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.minX = bounds[0]; a.maxX = bounds[1]; a.minY = bounds[2]; a.maxY = bounds[3];
    a.logsf = P->log_scale_factor;
    a.seen = (const uint8_t *)(A + o_seen); a.pass = (uint8_t *)(A + o_pass); a.s_xyxy = (float4 *)(A + o_sx); a.s_vc = (float *)(A + o_svc); a.s_lvl = (int *)(A + o_slv);
    a.blockcnt = (int *)(A + o_bc); a.nview = (int *)(A + o_cnt); a.ntested = a.nview + nframes;
    a.q_slot = (int *)(A + o_qs); a.q_xyxy = (float *)(A + o_qx); a.q_vc = (float *)(A + o_qv); a.q_lvl = (int *)(A + o_ql); a.q_wvec = (double *)(A + o_qw);
    a.q_desc = (uint8_t *)(A + o_qd); a.q_blocks = (uint8_t *)(A + o_qb);
    if (ns > 0) {
        hipLaunchKernelGGL(k_ll_frustum, dim3(nblocks), dim3(LL_BLOCK), 0, st, a);
        hipLaunchKernelGGL(k_ll_compact, dim3(nblocks, nframes), dim3(LL_BLOCK), 0, st, a);
    }
    std::vector<int> cnt;
    if ((rc = sm_counts_down(m, st, "local lines: frustum launch", A + o_cnt, nframes, cnt))) return rc;
    size_t sb = 0, rb = 0;
    for (int f = 0; f < nframes; f++) {
        res[f].n_slots_tested = cnt[nframes + f]; res[f].n_in_view = cnt[f];
        if (cnt[f] > LSBP_MAP_MAXQ) {                              // refused whole: nothing of the caller's is written
            res[f].status = HVO_ERR_UNSUPPORTED; m->last_error = match_lsbp_map_limit_text(cnt[f], fr[f].n_kl); return HVO_ERR_UNSUPPORTED;
        }
        if (cnt[f] > 0 && fr[f].n_kl > 0) sb = std::max(sb, match_lsbp_map_scratch_bytes(cnt[f], fr[f].n_kl));
        if (io[f].rel_map) rb = std::max(rb, stage_align((size_t)cnt[f] * (size_t)fr[f].n_kl));
    }
    // ---- scratch B: the search's key rows and the relation matrix ----
    if ((rc = sm_grow(m, st, &m->d_b, &m->b_bytes, stage_align(sb) + F * rb + 256))) return rc;
    LlGate G;
    ll_kinv(cam, G.Ki);
    for (int f = 0; f < nframes; f++) {
        const int nq = cnt[f], nt = fr[f].n_kl;
        int32_t *d_mi = (int32_t *)(A + o_mi) + (size_t)f * capq, *d_md = (int32_t *)(A + o_md) + (size_t)f * capq;
        int *d_k = (int *)(A + o_k[f]);
        if (nq > 0) sm_fill_enqueue(st, nq, d_mi, d_md);
        if (nq > 0 && nt > 0) {                                    // nToMatch > 0 (Tracking.cc:3345)
            LsbpMapDev s; memset(&s, 0, sizeof(s));
            s.nq = nq; s.nt = nt;
            s.q_xyxy = a.q_xyxy + 4 * (size_t)f * capq; s.q_view_cos = a.q_vc + (size_t)f * capq; s.q_wvec = a.q_wvec + 3 * (size_t)f * capq;
            s.q_desc = a.q_desc + 32 * (size_t)f * capq; s.q_blocks = a.q_blocks + (size_t)f * capq;
            s.t_kl = fr[f].kl; s.t_fn = fr[f].fn; s.t_l3d = fr[f].l3d; s.t_desc = fr[f].ldesc; s.t_occ = (const uint8_t *)(A + S[f].o_occ);
            s.cell_start = fr[f].ln_start; s.cell_items = fr[f].ln_items; s.n_items = fr[f].n_ln_items;
            s.mnMinX = bounds[0]; s.mnMaxX = bounds[1]; s.mnMinY = bounds[2]; s.mnMaxY = bounds[3]; s.th = P->th; s.nn_ratio = P->nn_ratio;
            s.cos_normal = cos(15.0 / 180.0 * M_PI);
            s.match_idx = d_mi; s.match_dist = d_md; s.n_matches = d_k;
            if ((rc = match_lsbp_map_enqueue(st, s, m->d_b))) { m->last_error = rc == HVO_ERR_UNSUPPORTED ? match_lsbp_map_limit_text(nq, nt) : "local lines: search launch"; return rc; }
        }
        if (f == nframes - 1) SM_HIP(hipEventRecord(m->ev[2], st));
    }
    for (int f = 0; f < nframes; f++) {
        const int nq = cnt[f], nt = fr[f].n_kl;
        if (nt < 1) continue;
        const float *T = Tcw + 12 * (size_t)f;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) G.R[3 * r + c] = T[4 * r + c];
        int32_t *d_mi = (int32_t *)(A + o_mi) + (size_t)f * capq;
        int *d_k = (int *)(A + o_k[f]), *d_win = (int *)(A + S[f].o_win);
        int8_t *d_rel = io[f].rel_map ? (int8_t *)(m->d_b + stage_align(sb) + (size_t)f * rb) : nullptr;
        if (nq > 0) sm_assign_enqueue(st, nq, nt, d_mi, d_win);
        hipLaunchKernelGGL(k_ll_gate, dim3((nt + LL_BLOCK - 1) / LL_BLOCK), dim3(LL_BLOCK), 0, st, nt, (size_t)m->cap, a.wvec, fr[f].kl, d_win,
                           a.q_slot + (size_t)f * capq, d_k, G, (int32_t *)(A + S[f].o_held), d_k + 1);
        if (nq > 0)
            hipLaunchKernelGGL(k_ll_struct, dim3((nq + LL_BLOCK - 1) / LL_BLOCK, nt), dim3(LL_BLOCK), 0, st, nq, fr[f].l3d, a.q_wvec + 3 * (size_t)f * capq, G, d_rel,
                               (int32_t *)(A + o_np[f]), (int32_t *)(A + o_nq[f]));
    }
    if (hipGetLastError() != hipSuccess) { m->last_error = "local lines: post-gate launch"; return HVO_ERR_HIP; }
    SM_HIP(hipEventRecord(m->ev[3], st));
    std::vector<int> kk(2 * F, 0);
    for (int f = 0; f < nframes; f++) {
        const size_t nq = (size_t)cnt[f], nt = (size_t)fr[f].n_kl, q0 = (size_t)f * capq;
        hvo_local_lines_io &I = io[f];
        SM_HIP(hipMemcpyAsync(&kk[2 * f], A + o_k[f], 8, hipMemcpyDeviceToHost, st));
        if (nt) {
            SM_HIP(hipMemcpyAsync(I.held, A + S[f].o_held, nt * 4, hipMemcpyDeviceToHost, st));
            SM_HIP(hipMemcpyAsync(I.n_par, A + o_np[f], nt * 4, hipMemcpyDeviceToHost, st));
            SM_HIP(hipMemcpyAsync(I.n_perp, A + o_nq[f], nt * 4, hipMemcpyDeviceToHost, st));
        }
        if (nq) {
            SM_HIP(hipMemcpyAsync(I.in_view_slot, a.q_slot + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.proj) SM_HIP(hipMemcpyAsync(I.proj, a.q_xyxy + 4 * q0, nq * 16, hipMemcpyDeviceToHost, st));
            if (I.view_cos) SM_HIP(hipMemcpyAsync(I.view_cos, a.q_vc + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.level) SM_HIP(hipMemcpyAsync(I.level, a.q_lvl + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.match_idx) SM_HIP(hipMemcpyAsync(I.match_idx, (int32_t *)(A + o_mi) + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.match_dist) SM_HIP(hipMemcpyAsync(I.match_dist, (int32_t *)(A + o_md) + q0, nq * 4, hipMemcpyDeviceToHost, st));
            if (I.rel_map && nt) SM_HIP(hipMemcpyAsync(I.rel_map, m->d_b + stage_align(sb) + (size_t)f * rb, nq * nt, hipMemcpyDeviceToHost, st));
        }
    }
    SM_HIP(hipStreamSynchronize(st));
    float ms[3];
    sm_kernel_ms(m, ms);
    for (int f = 0; f < nframes; f++) {
        res[f].n_matches = kk[2 * f]; res[f].n_gated = kk[2 * f + 1]; res[f].status = HVO_OK;
        for (int k = 0; k < 3; k++) res[f].kernel_ms[k] = ms[k];
    }
    return HVO_OK;
}
