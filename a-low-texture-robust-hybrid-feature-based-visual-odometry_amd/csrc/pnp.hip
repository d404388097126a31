// pnp.hip -- the relocalisation PnP solver: PnPsolver's EPnP RANSAC (reference src/PnPsolver.cc) for every candidate key frame of a
// relocalisation in one call.  Restated: the constructor (:67-110), SetRansacParameters (:121-157), iterate (:165-258), Refine (:260-305),
// CheckInliers (:308-339) and EPnP (:342-950; csrc/pnp_core.inc holds that part, shared with tools/pnp_host.cpp).
//
// iterate() is sequential only through mnIterations, mnBestInliers and mvbBestInliers, and Refine() depends on nothing but the current best
// set.  So all T hypotheses of all candidates are evaluated at once and the host replays the loop over what comes back (include/hvo.h has
// the rules; hvo::PnPsolver::iterate and hvo_amd.pnp_iterate are the replay):
//   k_pnp_gather      (stream form) the constructor's compaction in ascending frame-feature index: ballot prefix per wave + wave counts
//   k_pnp_hypotheses  16 lanes per hypothesis, four hypotheses per wave: the draw, EPnP on the drawn set, CheckInliers over all N
//   k_pnp_scan        per candidate: the running best over the passing counts, the records, each iteration's latest record
//   k_pnp_refine      one workgroup per (candidate, record): the record's inliers in ascending index, EPnP on them, CheckInliers
//   k_pnp_events      per candidate: hyp_event, the events' and the end-of-run answer's inlier bytes indexed by frame feature
// No atomic decides an order: the same bytes in give the same bytes out, in both forms.
//
// Readings (OpenCV is not in the tree) and defined behaviours: the head of csrc/pnp_core.inc.  Random draws: the reference draws from the
// process-global rand() (DUtils::Random::RandomInt), shared by all solvers; here hypothesis (candidate j, iteration it = 1..T) has its own
// xorshift32 stream, state seed ^ (0x9E3779B9 * (j * 1024 + it)) (0 -> 0x6D2B79F5: the mixing of csrc/vps.hip), a draw from a set of size
// s is x % s, and removal is the reference's swap-with-last (:199-200).  A hypothesis whose pose is not finite has count 0.
// SetRansacParameters' log / pow / ceil run on the host (pnp_set_ransac below), so a restatement on the host calls the same libm.
#include "frame_view.hpp"
#include "staged_call.hpp"
#include <string.h>
#include <math.h>
#include <algorithm>

#define PNP_HD __device__
#define PNP_SYNC() __syncthreads()
#include "pnp_core.inc"

#define PNP_MAX_T 1024
#define PNP_MAX_N 4096
#define PNP_MAX_KF 256
#define PNP_MAX_SET 64
#define PNP_MAX_EVENTS 64
#define PNP_GROUP 16
#define PNP_ARENA_LIMIT ((size_t)1 << 30)

struct PnpCand { int N, min_inl, T, max_its, nfeat, no_more; float eps; int pad; };

struct PnpDev {
    const float *p3d, *p2d, *max_err; const int *fidx;          // candidate j's arrays at j * capN (* 3, * 2)
    const PnpCand *cand;
    int capN, Tcap, min_set, E, capF; unsigned seed;
    double fu, fv, uc, vc;
    int *hyp_inl; uint8_t *hyp_mask; float *hyp_pose; int *hyp_sample, *hyp_rec, *hyp_event;
    int *n_rec, *rec_it, *best;                                  // best: (count, iteration) per candidate
    int *idx; int *ref_cnt; float *ref_pose; uint8_t *ref_mask;
    uint8_t *ev_inl, *ev_hinl, *best_inl;                       // by frame feature: an event's refined inliers, its record's own inliers, the overall best's
};

// ------------------------------------------------------------------------------------------------ k_pnp_hypotheses
// block = one wave = four hypotheses of candidate blockIdx.y; a group past the candidate's T repeats hypothesis T - 1 and writes nothing
// (every lane of the block has to reach every barrier).  Dynamic LDS: the tree buffers, present only when 2 * min_set > 64 rows.
__global__ __launch_bounds__(64) void k_pnp_hypotheses(PnpDev D)
{
    extern __shared__ double pnp_dyn[];
    __shared__ PnpWs ws[4];
    __shared__ int samp[4][PNP_MAX_SET], ovp[4][PNP_MAX_SET], ovv[4][PNP_MAX_SET];
    const int j = blockIdx.y;
    const PnpCand cd = D.cand[j];
    if ((int)blockIdx.x * 4 >= cd.T) return;
    const int g = threadIdx.x / PNP_GROUP, lane = threadIdx.x % PNP_GROUP;
    const int it0 = blockIdx.x * 4 + g;
    const bool active = it0 < cd.T;
    const int it = active ? it0 : cd.T - 1;
    const int ms = D.min_set;
    if (lane == 0) {
        unsigned rs = D.seed ^ (0x9E3779B9u * (unsigned)(j * 1024 + it + 1)); if (rs == 0) rs = 0x6D2B79F5u;
        int size = cd.N, nov = 0;
        for (int s = 0; s < ms; s++) {
            const int r = (int)(xs32(rs) % (unsigned)size), last = size - 1;
            int idx = r, lv = last, found = -1;
            for (int q = 0; q < nov; q++) { if (ovp[g][q] == r) { idx = ovv[g][q]; found = q; } if (ovp[g][q] == last) lv = ovv[g][q]; }
            samp[g][s] = idx;
            if (found >= 0) ovv[g][found] = lv; else { ovp[g][nov] = r; ovv[g][nov] = lv; nov++; }
            size--;
        }
    }
    __syncthreads();
    PnpCorr c;
    c.p3d = D.p3d + (size_t)j * D.capN * 3; c.p2d = D.p2d + (size_t)j * D.capN * 2; c.sel = samp[g]; c.n = ms;
    c.fu = D.fu; c.fv = D.fv; c.uc = D.uc; c.vc = D.vc;
    PnpWs *w = &ws[g];
    pnp_epnp<PNP_GROUP>(c, w, pnp_dyn + (size_t)g * PNP_TREE_BATCH * 256, lane);
    const int finite = pnp_pose_finite(w);
    const float *me = D.max_err + (size_t)j * D.capN;
    const size_t h = (size_t)j * D.Tcap + it;
    uint8_t *mask = D.hyp_mask + h * D.capN;
    int cnt = 0;
    for (int i = lane; i < cd.N; i += PNP_GROUP) {
        const int in = finite ? pnp_check_one(w, c.p3d, c.p2d, me, D.fu, D.fv, D.uc, D.vc, i) : 0;
        if (active) mask[i] = (uint8_t)in;
        cnt += in;
    }
    w->cnt[lane] = cnt;
    __syncthreads();
    if (active && lane == 0) {
        int tot = 0;
        for (int l = 0; l < PNP_GROUP; l++) tot += w->cnt[l];
        D.hyp_inl[h] = tot;
        for (int q = 0; q < 3; q++) { for (int r = 0; r < 3; r++) D.hyp_pose[h * 12 + 4 * q + r] = (float)w->R[3 * q + r]; D.hyp_pose[h * 12 + 4 * q + 3] = (float)w->t[q]; }
    }
    if (active && D.hyp_sample) for (int s = lane; s < ms; s += PNP_GROUP) D.hyp_sample[h * ms + s] = samp[g][s];
}

// ------------------------------------------------------------------------------------------------ k_pnp_scan
// iterate()'s bookkeeping (:209-224) over the counts: a passing iteration (count >= minInliers) is a record when its count exceeds the
// running best; hyp_rec[it] = the latest record at a passing iteration, -1 otherwise.  Records past the capacity are counted, not kept.
// One thread per candidate on purpose: at most 1024 counts, a few dozen with the reference's parameters, beside a hypothesis kernel of
// tens of thousands of dependent steps; a wave-wide prefix maximum would save nothing that shows.
__global__ __launch_bounds__(64) void k_pnp_scan(PnpDev D)
{
    const int j = blockIdx.x;
    if (threadIdx.x != 0) return;
    const PnpCand cd = D.cand[j];
    int best = 0, best_it = -1, nrec = 0;
    for (int it = 0; it < cd.T; it++) {
        const int c = D.hyp_inl[(size_t)j * D.Tcap + it];
        int r = -1;
        if (c >= cd.min_inl) {
            if (c > best) { best = c; best_it = it; if (nrec < D.E) D.rec_it[j * D.E + nrec] = it; nrec++; }
            r = nrec - 1;
        }
        D.hyp_rec[(size_t)j * D.Tcap + it] = r;
    }
    D.n_rec[j] = nrec; D.best[2 * j] = best; D.best[2 * j + 1] = best_it;
}

// ------------------------------------------------------------------------------------------------ k_pnp_refine
// Refine() (:260-305) of record blockIdx.x of candidate blockIdx.y
__global__ __launch_bounds__(256) void k_pnp_refine(PnpDev D)
{
    __shared__ PnpWs w;
    __shared__ double tbuf[PNP_TREE_BATCH * 256];
    __shared__ int wcnt[4], base;
    const int j = blockIdx.y, e = blockIdx.x, tid = threadIdx.x;
    const PnpCand cd = D.cand[j];
    if (e >= min(D.n_rec[j], D.E)) return;
    const int it = D.rec_it[j * D.E + e];
    const uint8_t *hm = D.hyp_mask + ((size_t)j * D.Tcap + it) * D.capN;
    int *idx = D.idx + ((size_t)j * D.E + e) * D.capN;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < cd.N; i0 += 256) {                      // the inliers in ascending correspondence index
        const int i = i0 + tid;
        const bool p = i < cd.N && hm[i] != 0;
        const unsigned long long bm = __ballot(p);
        const int ln = tid & 63, wv = tid >> 6;
        if (ln == 0) wcnt[wv] = __popcll(bm);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wv; q++) off += wcnt[q];
        if (p) idx[off + __popcll(bm & ((1ull << ln) - 1ull))] = i;
        __syncthreads();
        if (tid == 0) base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    PnpCorr c;
    c.p3d = D.p3d + (size_t)j * D.capN * 3; c.p2d = D.p2d + (size_t)j * D.capN * 2; c.sel = idx; c.n = base;
    c.fu = D.fu; c.fv = D.fv; c.uc = D.uc; c.vc = D.vc;
    pnp_epnp<256>(c, &w, tbuf, tid);
    const int finite = pnp_pose_finite(&w);
    const float *me = D.max_err + (size_t)j * D.capN;
    const size_t r = (size_t)j * D.E + e;
    uint8_t *mask = D.ref_mask + r * D.capN;
    int cnt = 0;
    for (int i = tid; i < cd.N; i += 256) {
        const int in = finite ? pnp_check_one(&w, c.p3d, c.p2d, me, D.fu, D.fv, D.uc, D.vc, i) : 0;
        mask[i] = (uint8_t)in;
        cnt += in;
    }
    w.cnt[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int l = 0; l < 256; l++) tot += w.cnt[l];
        D.ref_cnt[r] = tot;
        for (int q = 0; q < 3; q++) { for (int k = 0; k < 3; k++) D.ref_pose[r * 12 + 4 * q + k] = (float)w.R[3 * q + k]; D.ref_pose[r * 12 + 4 * q + 3] = (float)w.t[q]; }
    }
}

// ------------------------------------------------------------------------------------------------ k_pnp_events
// hyp_event[it]: the record iterate() returns in iteration it (its Refine kept more than minInliers, :292), else -1; the inlier bytes of
// the events and of the end-of-run answer (:241-255) indexed by frame feature, as vbInliers is (:229-234)
__global__ __launch_bounds__(256) void k_pnp_events(PnpDev D)
{
    const int j = blockIdx.x, tid = threadIdx.x;
    const PnpCand cd = D.cand[j];
    const int ne = min(D.n_rec[j], D.E);
    for (int it = tid; it < cd.T; it += 256) {
        const int r = D.hyp_rec[(size_t)j * D.Tcap + it];
        D.hyp_event[(size_t)j * D.Tcap + it] = (r >= 0 && r < ne && D.ref_cnt[(size_t)j * D.E + r] > cd.min_inl) ? r : -1;
    }
    const int *fi = D.fidx + (size_t)j * D.capN;
    const int bit = D.best[2 * j + 1];
    for (int x = 0; x <= 2 * ne; x++) {                          // x == 2 ne: the best of all T; odd x: the record's own hypothesis (mvbBestInliers while it is the best)
        if (x == 2 * ne && bit < 0) break;
        const int e = x >> 1;
        uint8_t *out = x == 2 * ne ? D.best_inl + (size_t)j * D.capF : ((x & 1) ? D.ev_hinl : D.ev_inl) + ((size_t)j * D.E + e) * D.capF;
        const uint8_t *m = x == 2 * ne ? D.hyp_mask + ((size_t)j * D.Tcap + bit) * D.capN
                         : ((x & 1) ? D.hyp_mask + ((size_t)j * D.Tcap + D.rec_it[j * D.E + e]) * D.capN : D.ref_mask + ((size_t)j * D.E + e) * D.capN);
        for (int f = tid; f < cd.nfeat; f += 256) out[f] = 0;
        __syncthreads();
        for (int i = tid; i < cd.N; i += 256) if (m[i]) { const int f = fi[i]; if (f >= 0 && f < cd.nfeat) out[f] = 1; }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ k_pnp_gather
// The constructor (:78-101) for candidate blockIdx.x on a resident frame: feature i is kept when match[i] names a key-frame feature that is
// not bad; the kept ones leave in ascending i.  mvSigma2 = scale[octave]^2 (float), mvMaxError = mvSigma2 * th2 (:156).
struct PnpGather { const hvo_keypoint *kp_un; const int *match; const float *kf_pos; const uint8_t *kf_bad; const int *kf_n; int nf, capK; float sigma2[HVO_MAX_LEVELS]; float th2; };
__global__ __launch_bounds__(256) void k_pnp_gather(PnpGather G, int capN, float *p3d, float *p2d, float *max_err, int *fidx)
{
    __shared__ int wcnt[4], base;
    const int j = blockIdx.x, tid = threadIdx.x, ln = tid & 63, wv = tid >> 6;
    const int *match = G.match + (size_t)j * G.nf;
    const float *pos = G.kf_pos + (size_t)j * G.capK * 3;
    const uint8_t *bad = G.kf_bad + (size_t)j * G.capK;
    const int nk = G.kf_n[j];
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < G.nf; i0 += 256) {
        const int i = i0 + tid;
        int m = -1;
        if (i < G.nf) { m = match[i]; if (m < 0 || m >= nk || bad[m]) m = -1; }
        const bool p = m >= 0;
        const unsigned long long bm = __ballot(p);
        if (ln == 0) wcnt[wv] = __popcll(bm);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wv; q++) off += wcnt[q];
        const int o = off + __popcll(bm & ((1ull << ln) - 1ull));
        if (p && o < capN) {
            const hvo_keypoint kp = G.kp_un[i];
            const size_t d = (size_t)j * capN + o;
            p3d[d * 3] = pos[3 * m]; p3d[d * 3 + 1] = pos[3 * m + 1]; p3d[d * 3 + 2] = pos[3 * m + 2];
            p2d[d * 2] = kp.x; p2d[d * 2 + 1] = kp.y;
            const int oc = kp.octave < 0 ? 0 : (kp.octave >= HVO_MAX_LEVELS ? HVO_MAX_LEVELS - 1 : kp.octave);
            max_err[d] = __fmul_rn(G.sigma2[oc], G.th2);
            fidx[d] = i;
        }
        __syncthreads();
        if (tid == 0) base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ host
// SetRansacParameters (:121-157) for N correspondences, with the host's libm like the reference
static void pnp_set_ransac(const hvo_pnp_params *P, int N, PnpCand *c)
{
    float eps = P->epsilon;
    int nMin = (int)(N * eps);
    if (nMin < P->min_inliers) nMin = P->min_inliers;
    if (nMin < P->min_set) nMin = P->min_set;
    if (N > 0 && eps < (float)nMin / N) eps = (float)nMin / N;
    int nIt;
    if (nMin == N) nIt = 1;
    else {
        const double v = ceil(log(1 - P->probability) / log(1 - pow((double)eps, 3)));
        nIt = !(v < (double)P->max_iterations) ? P->max_iterations : (v < 1.0 ? 1 : (int)v);     // (a NaN or an overflowing quotient takes the cap; max(1, .) follows anyway)
    }
    c->N = N; c->min_inl = nMin; c->eps = eps; c->max_its = std::max(1, std::min(nIt, (int)P->max_iterations));
    c->no_more = N < nMin ? 1 : 0;                               // iterate (:173-177)
    c->T = c->no_more ? 0 : c->max_its + P->extra_iterations;
    c->pad = 0;
}

// fr null: prob's host arrays go up.  Else the frame side is the resident frame's key points at fr->kp_un, kf[j]'s map side goes up,
// N[j] is counted on the host (SetRansacParameters needs it before the launch) and k_pnp_gather compacts on the device.
int pnp_run(hvo_ctx *ctx, hipStream_t st, const hvo_camera *cam, const hvo_pnp_params *P, int n_kf, const hvo_pnp_problem *prob, const FrameView *fr,
            const hvo_pnp_keyframe_side *kf, hvo_pnp_result *res, std::string *err)
{
    if (P->min_set < 4) { *err = "pnp: min_set below 4"; return HVO_ERR_INVALID_ARG; }
    if (P->min_set > PNP_MAX_SET || n_kf > PNP_MAX_KF) { *err = "pnp: min_set above 64 or more than 256 candidates"; return HVO_ERR_UNSUPPORTED; }
    if (P->extra_iterations < 0 || P->max_events < 1 || P->max_iterations < 1 || P->min_inliers < 0) {
        *err = "pnp: extra_iterations < 0, max_events < 1, max_iterations < 1 or min_inliers < 0"; return HVO_ERR_INVALID_ARG;
    }
    if (P->max_events > PNP_MAX_EVENTS) { *err = "pnp: max_events above 64"; return HVO_ERR_UNSUPPORTED; }
    const int E = P->max_events, ms = P->min_set;
    std::vector<PnpCand> cand((size_t)n_kf);
    std::vector<int> Nj((size_t)n_kf), NFj((size_t)n_kf);
    int capN = 1, Tcap = 0, capF = 1, capK = 1;
    for (int j = 0; j < n_kf; j++) {
        int N, nfeat;
        if (fr) {
            const hvo_pnp_keyframe_side &K = kf[j];
            if (K.n < 0 || (K.n > 0 && (!K.pos || !K.bad)) || (fr->n_kp > 0 && !K.match_kf)) { *err = "pnp: a key-frame side with n < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
            N = 0;
            for (int i = 0; i < fr->n_kp; i++) { const int m = K.match_kf[i]; if (m >= 0 && m < K.n && !K.bad[m]) N++; }
            nfeat = fr->n_kp; capK = std::max(capK, (int)K.n);
        } else {
            const hvo_pnp_problem &Q = prob[j];
            if (Q.n < 0 || Q.n_features < 0 || (Q.n > 0 && (!Q.p3d || !Q.p2d || !Q.sigma2 || !Q.feature_index))) { *err = "pnp: a problem with n < 0, n_features < 0 or a null array"; return HVO_ERR_INVALID_ARG; }
            for (int i = 0; i < Q.n; i++) if (Q.feature_index[i] < 0 || Q.feature_index[i] >= Q.n_features) { *err = "pnp: feature_index outside [0, n_features)"; return HVO_ERR_INVALID_ARG; }
            N = Q.n; nfeat = Q.n_features;
        }
        if (N > PNP_MAX_N) { *err = "pnp: more than 4096 correspondences"; return HVO_ERR_UNSUPPORTED; }
        pnp_set_ransac(P, N, &cand[j]);
        cand[j].nfeat = nfeat;
        if (cand[j].T > PNP_MAX_T) { *err = "pnp: more than 1024 hypotheses per candidate (max_iterations + extra_iterations)"; return HVO_ERR_UNSUPPORTED; }
        Nj[j] = N; NFj[j] = nfeat;
        capN = std::max(capN, N); Tcap = std::max(Tcap, cand[j].T); capF = std::max(capF, nfeat);
        hvo_pnp_result &R = res[j];
        if (R.cap_hyp < cand[j].T || (cand[j].T > 0 && (!R.hyp_inliers || !R.hyp_event)) || !R.events || R.cap_events < E || (nfeat > 0 && !R.best_inliers)) {
            *err = "pnp: a result's arrays are missing or below the candidate's size"; return HVO_ERR_INVALID_ARG;
        }
        for (int e = 0; e < E; e++) if (nfeat > 0 && (!R.events[e].inliers || !R.events[e].hyp_inliers)) { *err = "pnp: an event's inlier arrays are missing"; return HVO_ERR_INVALID_ARG; }
    }
    bool want_sample = false;
    for (int j = 0; j < n_kf; j++) want_sample = want_sample || res[j].hyp_sample != nullptr;
    const int Tc = std::max(Tcap, 1);
    // one carve of the context's arena: what goes up, then the scratch and the results
    const size_t F = (size_t)n_kf, nkp = fr ? (size_t)std::max(fr->n_kp, 1) : 0, FE = F * E, FT = F * Tc;    // rows: a candidate, its event e at j E + e, its hypothesis at j Tc + it
    StageCarver C(256);
    const auto a_cand = C.take<PnpCand>(F);
    const auto a_p3d = C.take<float>(F, (size_t)capN * 3), a_p2d = C.take<float>(F, (size_t)capN * 2), a_me = C.take<float>(F, capN); const auto a_fi = C.take<int>(F, capN);
    const size_t up_host = C.mark(), Fr = fr ? F : 0;            // the host form uploads [0, up_host); the resident form adds the key-frame sides
    const auto g_match = C.take<int>(Fr, nkp); const auto g_pos = C.take<float>(Fr, (size_t)capK * 3); const auto g_bad = C.take<uint8_t>(Fr, capK); const auto g_n = C.take<int>(Fr);
    const size_t up_end = C.mark(), r0 = up_end;
    const auto a_inl = C.take<int>(F, Tc), a_rec = C.take<int>(F, Tc), a_evt = C.take<int>(F, Tc); const auto a_pose = C.take<float>(FT, 12);
    const auto a_nrec = C.take<int>(F), a_recit = C.take<int>(F, E), a_best = C.take<int>(F, 2), a_rcnt = C.take<int>(F, E); const auto a_rpose = C.take<float>(FE, 12);
    const auto a_evin = C.take<uint8_t>(FE, capF), a_evh = C.take<uint8_t>(FE, capF), a_bin = C.take<uint8_t>(F, capF);
    const auto a_samp = C.take<int>(want_sample ? F : 0, (size_t)Tc * ms);
    const size_t r1 = C.mark();                                  // [r0, r1) comes down
    const auto a_mask = C.take<uint8_t>(FT, capN); const auto a_idx = C.take<int>(FE, capN); const auto a_rmask = C.take<uint8_t>(FE, capN);
    const size_t total = C.mark();
    if (total > PNP_ARENA_LIMIT) { *err = "pnp: the call's device scratch would pass 1 GiB (candidates x hypotheses x correspondences)"; return HVO_ERR_UNSUPPORTED; }
    StagedCall sc(ctx, st, "pnp: ", err); int rc;
    ctx->pnp_ms[0] = ctx->pnp_ms[1] = 0.f;
    if ((rc = sc.begin(total, up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    memcpy(a_cand.host(h), cand.data(), a_cand.bytes());
    PnpGather G; memset(&G, 0, sizeof(G));
    if (fr) {
        for (int j = 0; j < n_kf; j++) {
            const hvo_pnp_keyframe_side &K = kf[j];
            if (fr->n_kp) memcpy(g_match.host(h, j), K.match_kf, (size_t)fr->n_kp * 4);
            if (K.n) { memcpy(g_pos.host(h, j), K.pos, (size_t)K.n * 12); memcpy(g_bad.host(h, j), K.bad, (size_t)K.n); }
            g_n.host(h)[j] = K.n;
        }
        G.kp_un = fr->kp_un; G.match = g_match.dev(d); G.kf_pos = g_pos.dev(d); G.kf_bad = g_bad.dev(d);
        G.kf_n = g_n.dev(d); G.nf = fr->n_kp; G.capK = capK; G.th2 = P->th2;
        frame_level_sigma2(ctx, G.sigma2, nullptr);
        if ((rc = sc.up(a_cand.off, a_cand.off + stage_align(a_cand.bytes()))) || (rc = sc.up(up_host, up_end))) return rc;
    } else {
        for (int j = 0; j < n_kf; j++) {
            const hvo_pnp_problem &Q = prob[j];
            if (!Q.n) continue;
            memcpy(a_p3d.host(h, j), Q.p3d, (size_t)Q.n * 12); memcpy(a_p2d.host(h, j), Q.p2d, (size_t)Q.n * 8);
            float *me = a_me.host(h, j);
            for (int i = 0; i < Q.n; i++) { volatile float m = Q.sigma2[i] * P->th2; me[i] = m; }       // mvMaxError (:156)
            memcpy(a_fi.host(h, j), Q.feature_index, (size_t)Q.n * 4);
        }
        if ((rc = sc.up(0, up_host))) return rc;
    }
    PnpDev D; memset(&D, 0, sizeof(D));
    D.p3d = a_p3d.dev(d); D.p2d = a_p2d.dev(d); D.max_err = a_me.dev(d); D.fidx = a_fi.dev(d);
    D.cand = a_cand.dev(d); D.capN = capN; D.Tcap = Tc; D.min_set = ms; D.E = E; D.capF = capF; D.seed = P->seed;
    D.fu = cam->fx; D.fv = cam->fy; D.uc = cam->cx; D.vc = cam->cy;
    D.hyp_inl = a_inl.dev(d); D.hyp_mask = a_mask.dev(d); D.hyp_pose = a_pose.dev(d); D.hyp_sample = want_sample ? a_samp.dev(d) : nullptr;
    D.hyp_rec = a_rec.dev(d); D.hyp_event = a_evt.dev(d); D.n_rec = a_nrec.dev(d); D.rec_it = a_recit.dev(d); D.best = a_best.dev(d);
    D.idx = a_idx.dev(d); D.ref_cnt = a_rcnt.dev(d); D.ref_pose = a_rpose.dev(d); D.ref_mask = a_rmask.dev(d);
    D.ev_inl = a_evin.dev(d); D.ev_hinl = a_evh.dev(d); D.best_inl = a_bin.dev(d);
    if ((rc = sc.clear(r0, r1))) return rc;
    if (fr && fr->n_kp > 0) hipLaunchKernelGGL(k_pnp_gather, dim3(n_kf), dim3(256), 0, st, G, capN, a_p3d.dev(d), a_p2d.dev(d), a_me.dev(d), a_fi.dev(d));
    sc.tick();
    if (Tcap > 0) {
        const size_t dyn = 2 * ms > PNP_SEQ_ROWS ? (size_t)4 * PNP_TREE_BATCH * 256 * sizeof(double) : 0;
        if (dyn && hvo_ensure_dyn_lds((const void *)k_pnp_hypotheses, dyn) != HVO_OK) { *err = "pnp: dynamic LDS"; return HVO_ERR_HIP; }
        hipLaunchKernelGGL(k_pnp_hypotheses, dim3((Tcap + 3) / 4, n_kf), dim3(64), dyn, st, D);
    }
    hipLaunchKernelGGL(k_pnp_scan, dim3(n_kf), dim3(1), 0, st, D);
    sc.tick();
    if (Tcap > 0) hipLaunchKernelGGL(k_pnp_refine, dim3(E, n_kf), dim3(256), 0, st, D);
    hipLaunchKernelGGL(k_pnp_events, dim3(n_kf), dim3(256), 0, st, D);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    ctx->pnp_ms[0] = sc.ms[0]; ctx->pnp_ms[1] = sc.ms[1];
    for (int j = 0; j < n_kf; j++) {
        hvo_pnp_result &R = res[j]; const PnpCand &c = cand[j];
        const int T = c.T, nrec = a_nrec.down(b)[j], ne = std::min(nrec, E);
        R.n = c.N; R.min_inliers = c.min_inl; R.max_its = c.max_its; R.epsilon = c.eps; R.n_hyp = T; R.no_more = c.no_more; R.n_features = NFj[j];
        R.n_events = ne; R.status = nrec > E ? HVO_ERR_CAPACITY : HVO_OK;
        if (nrec > E) rc = HVO_ERR_CAPACITY;
        if (T) {
            memcpy(R.hyp_inliers, a_inl.down(b, j), (size_t)T * 4);
            memcpy(R.hyp_event, a_evt.down(b, j), (size_t)T * 4);
            if (R.hyp_sample) memcpy(R.hyp_sample, a_samp.down(b, j), (size_t)T * ms * 4);
        }
        for (int e = 0; e < ne; e++) {
            hvo_pnp_event &V = R.events[e];
            const size_t je = (size_t)j * E + e;
            V.iteration = a_recit.down(b, j)[e] + 1;
            V.n_inliers = a_rcnt.down(b, j)[e];
            V.success = V.n_inliers > c.min_inl ? 1 : 0;
            memcpy(V.Tcw, a_rpose.down(b, je), 48);
            const int it0 = V.iteration - 1;
            V.hyp_n_inliers = a_inl.down(b, j)[it0];
            memcpy(V.hyp_Tcw, a_pose.down(b, (size_t)j * Tc + it0), 48);
            if (NFj[j]) { memcpy(V.inliers, a_evin.down(b, je), (size_t)NFj[j]); memcpy(V.hyp_inliers, a_evh.down(b, je), (size_t)NFj[j]); }
        }
        const int bc = a_best.down(b, j)[0], bit = a_best.down(b, j)[1];
        R.best_n_inliers = bc; R.best_valid = (bit >= 0 && bc >= c.min_inl) ? 1 : 0; R.best_iteration = bit + 1;
        if (bit >= 0) {
            memcpy(R.best_Tcw, a_pose.down(b, (size_t)j * Tc + bit), 48);
            if (NFj[j]) memcpy(R.best_inliers, a_bin.down(b, j), (size_t)NFj[j]);
        } else memset(R.best_Tcw, 0, 48);
    }
    if (rc == HVO_ERR_CAPACITY) *err = "pnp: a candidate has more records than max_events (its status says which)";
    return rc;
}

extern "C" {

void hvo_pnp_default_params(hvo_pnp_params *p)
{
    if (!p) return;
    p->probability = 0.99; p->min_inliers = 10; p->max_iterations = 300; p->min_set = 4; p->epsilon = 0.5f; p->th2 = 5.991f;   // src/Tracking.cc:3805
    p->seed = 1; p->extra_iterations = 8; p->max_events = 8;
}

int hvo_pnp_ransac(hvo_ctx *ctx, const hvo_camera *cam, const hvo_pnp_params *params, int n_kf, const hvo_pnp_problem *problems, hvo_pnp_result *results)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !problems || !results || n_kf < 1) { ctx->last_error = "pnp: a null argument or n_kf < 1"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return pnp_run(ctx, ctx->stream, cam, params, n_kf, problems, nullptr, nullptr, results, &ctx->last_error);
}

int hvo_pnp_last_kernel_ms(const hvo_ctx *ctx, float ms2[2])
{
    if (!ctx || !ms2) return HVO_ERR_INVALID_ARG;
    ms2[0] = ctx->pnp_ms[0]; ms2[1] = ctx->pnp_ms[1];
    return HVO_OK;
}

}   // extern "C"
