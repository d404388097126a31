// frame_view.hip -- the two builders of a FrameView (frame_view.hpp): where a resident frame's arrays live, and the refusals
#include "frame_view.hpp"
#include <string.h>
#include <algorithm>

// One row per resident operation: { what, stages, any LSD stage, depth, what a frame without depth lacks, mvuRight, bf, counts, events, the stages as the
// batch form's and the stream form's refusals name them }
static const char k_mf_list[] = "HVO_STAGE_PLANE_TAIL and HVO_STAGE_LINES3D", k_ls_list[] = "an LSD stage and HVO_STAGE_LINES3D",
                  k_ll_list[] = "an LSD stage, HVO_STAGE_GRIDS and HVO_STAGE_LINES3D", k_lines[] = "an LSD stage";
const FrameNeed need_manhattan     = { "Manhattan tracking", HVO_STAGE_PLANE_TAIL | HVO_STAGE_LINES3D, false, FV_DEPTH_STREAM, "no normals, no 3-D lines", false, false, 0, FV_EV_ORB | FV_EV_LSD, k_mf_list, k_mf_list };
const FrameNeed need_planes        = { "plane association", HVO_STAGE_PLANE_TAIL, false, FV_DEPTH_STREAM, "no planes", false, false, 0, FV_EV_PEAC, "HVO_STAGE_PLANE_TAIL", "HVO_STAGE_PLANE_TAIL" };
const FrameNeed need_pose          = { "pose optimisation", HVO_STAGE_ORB | HVO_STAGE_LINES3D | HVO_STAGE_PLANE_TAIL, true, FV_DEPTH, "no mvuRight, 3-D lines or planes", true, true, 0, FV_EV_ORB | FV_EV_LSD | FV_EV_PEAC,
                                       "HVO_STAGE_ORB, an LSD stage, HVO_STAGE_LINES3D and HVO_STAGE_PLANE_TAIL", "HVO_STAGE_ORB, HVO_STAGE_LINES3D and HVO_STAGE_PLANE_TAIL" };
const FrameNeed need_line_struct   = { "line structure", HVO_STAGE_LINES3D, true, FV_DEPTH, "no 3-D lines", false, false, 0, FV_EV_LSD, k_ls_list, k_ls_list };
const FrameNeed need_local_lines   = { "local lines", HVO_STAGE_GRIDS | HVO_STAGE_LINES3D, true, FV_DEPTH, "no 3-D lines", false, false, FV_N_KL | FV_N_LN, FV_EV_LSD, k_ll_list, k_ll_list };
const FrameNeed need_local_points  = { "local points", HVO_STAGE_ORB, false, 0, "", true, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
const FrameNeed need_bow           = { "bag of words", HVO_STAGE_ORB, false, 0, "", false, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
const FrameNeed need_bow_search    = { "search by bag of words", 0, false, 0, "", false, false, FV_N_KP, FV_EV_ORB, "", "" };     // (the frame's kept bag of words is the caller's check)
const FrameNeed need_pnp           = { "pnp", HVO_STAGE_ORB, false, 0, "", false, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
const FrameNeed need_kf_search     = { "key-frame search", HVO_STAGE_ORB, false, 0, "", false, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
const FrameNeed need_new_points    = { "create new map points", HVO_STAGE_ORB, false, 0, "", true, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
const FrameNeed need_fuse          = { "fuse", HVO_STAGE_ORB, false, 0, "", true, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
// the guided frame-to-frame matching of the stream
const FrameNeed need_guided_points = { "guided search", HVO_STAGE_ORB, false, 0, "", true, false, FV_N_KP, FV_EV_ORB, "HVO_STAGE_ORB", "HVO_STAGE_ORB" };
const FrameNeed need_line_match    = { "line matching", 0, true, 0, "", false, false, FV_N_KL, FV_EV_LSD, k_lines, k_lines };
const FrameNeed need_new_lines     = { "create new map lines", 0, true, 0, "", false, false, FV_N_KL, FV_EV_LSD, k_lines, k_lines };
const FrameNeed need_fuse_lines    = { "fuse lines", 0, true, 0, "", false, false, FV_N_KL, FV_EV_LSD, k_lines, k_lines };
const FrameNeed need_guided_lines  = { "guided line search", HVO_STAGE_GRIDS, true, 0, "", false, false, FV_N_KL | FV_N_LN, FV_EV_LSD, "an LSD stage and HVO_STAGE_GRIDS", "an LSD stage and HVO_STAGE_GRIDS" };
const FrameNeed need_map_lines     = { "local-map line search", HVO_STAGE_GRIDS | HVO_STAGE_LINES3D, true, FV_DEPTH_STREAM, "no 3-D lines", false, false, FV_N_KL | FV_N_LN, FV_EV_LSD,
                                       "HVO_STAGE_GRIDS and HVO_STAGE_LINES3D", "HVO_STAGE_GRIDS and HVO_STAGE_LINES3D" };

static const char k_pu_list[] = "HVO_STAGE_PLANES and HVO_STAGE_PLANE_TAIL";
const FrameNeed need_plane_update  = { "plane map update", HVO_STAGE_PLANES | HVO_STAGE_PLANE_TAIL, false, FV_DEPTH_STREAM, "no plane clouds", false, false, FV_N_PC, FV_EV_PEAC, k_pu_list, k_pu_list };

static const char k_kfi_list[] = "HVO_STAGE_ORB, an LSD stage and HVO_STAGE_LINES3D";
const FrameNeed need_new_keyframe  = { "create key-frame features", HVO_STAGE_ORB | HVO_STAGE_LINES3D, true, FV_DEPTH_STREAM, "no mvDepth, no 3-D lines", true, true, FV_N_KP | FV_N_KL,
                                       FV_EV_ORB | FV_EV_LSD, k_kfi_list, k_kfi_list };

static int refuse(std::string &err, const FrameNeed &nd, const char *a, const char *b = "", const char *c = "")
{
    err = std::string(nd.what) + ": " + a + b + c;
    return HVO_ERR_INVALID_ARG;
}

static bool stages_ok(const FrameNeed &nd, unsigned have)
{
    return (have & nd.stages) == nd.stages && (!nd.any_lsd || (have & (HVO_STAGE_LSD | HVO_STAGE_LSD_CULL)));
}

void frame_level_sigma2(const hvo_ctx *ctx, float *sigma2, float *inv_sigma2)
{
    for (int i = 0; i < HVO_MAX_LEVELS; i++) {
        if (sigma2) sigma2[i] = i < ctx->p.orb_nlevels ? ctx->scale[i] * ctx->scale[i] : 1.0f;
        if (inv_sigma2) inv_sigma2[i] = i < ctx->p.orb_nlevels ? 1.0f / (ctx->scale[i] * ctx->scale[i]) : 1.0f;
    }
}

void frame_view_counts(FrameView &v, unsigned which)
{
    if (!v.h_counts) return;
    if (which & FV_N_KP) v.n_kp = std::max(0, std::min(v.h_counts[0], v.kp_cap));
    if (which & FV_N_KL) v.n_kl = std::max(0, std::min(v.h_counts[4], v.nfeat));
}

int batch_views(hvo_ctx *ctx, int n, const FrameNeed &nd, std::vector<FrameView> &views, float bf)
{
    std::string &err = ctx->last_error;
    if (n > ctx->batch_n) return refuse(err, nd, "n beyond the resident batch");
    if (!stages_ok(nd, ctx->last_stages)) return refuse(err, nd, "the last hvo_batch_run must include ", nd.list_batch);
    if ((nd.depth & FV_DEPTH_BATCH) && !ctx->have_depth) return refuse(err, nd, "the batch was uploaded without depth (", nd.depth_why, ")");
    if (nd.bf && !(bf > 0)) return refuse(err, nd, "bf <= 0 (no mvuRight)");
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    // the plans: key lines where the operation needs an LSD stage or the 3-D lines, the depth image where it reads mvuRight
    const bool lines = nd.any_lsd || (nd.stages & HVO_STAGE_LINES3D);
    char *d_out = nullptr; TailLayout L; memset(&L, 0, sizeof(L));
    if ((nd.stages & (HVO_STAGE_LINES3D | HVO_STAGE_VP | HVO_STAGE_PLANE_TAIL | HVO_STAGE_GRIDS)) && tail_batch_view(ctx, &d_out, &L)) return refuse(err, nd, "no resident tail results");
    LsdView lv; PeacView pv; memset(&lv, 0, sizeof(lv)); memset(&pv, 0, sizeof(pv));
    const int plan = std::max(n, ctx->p.max_batch);
    int rc;
    if (lines && (rc = lsd_prepare(ctx, ctx->batch_w, ctx->batch_h, plan, ctx->last_cull, &lv))) return rc;
    if (nd.uright && ctx->have_depth && (rc = peac_prepare(ctx, ctx->batch_w, ctx->batch_h, plan, &pv))) return rc;
    // the resident counts, one copy for all n frames
    const OrbPlan &O = ctx->orb;
    const int *d_cnt = (nd.counts & FV_N_KP) ? O.d_nkp : ((nd.counts & FV_N_KL) ? lv.d_nkl : nullptr);
    std::vector<int> cnt((size_t)n, -1);
    if (d_cnt) {
        HVO_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    FrameView zero; memset(&zero, 0, sizeof(zero));
    views.assign((size_t)n, zero);
    for (int f = 0; f < n; f++) {
        FrameView &v = views[f];
        v.ctx = ctx; v.n_kp = v.n_kl = -1;
        v.kp = v.kp_un = O.d_kp + (size_t)f * O.kp_cap; v.desc = O.d_desc + (size_t)f * O.kp_cap * 32; v.d_nkp = O.d_nkp + f; v.kp_cap = O.kp_cap;
        if (nd.counts & FV_N_KP) v.n_kp = std::max(0, std::min(cnt[f], O.kp_cap));
        if (lines) {
            v.kl = lv.d_kl + (size_t)f * lv.nfeat; v.fn = lv.d_fn + (size_t)f * lv.nfeat * 3; v.ldesc = lv.d_desc + (size_t)f * lv.nfeat * 32; v.d_nkl = lv.d_nkl + f; v.nfeat = lv.nfeat;
            if (nd.counts & FV_N_KL) v.n_kl = std::max(0, std::min(cnt[f], lv.nfeat));
        }
        if (d_out) {
            char *o = d_out + (size_t)f * L.total;
            v.l3d = (hvo_line3d *)(o + L.lines3d); v.pclouds = (const hvo_plane_cloud *)(o + L.pclouds); v.normals = (const hvo_surface_normal *)(o + L.normals);
            v.cloud_xyz = (const float *)(o + L.cloud); v.cloud_cap = L.cloud_cap;
            v.n_normals = L.n_normals; v.ln_start = (const int32_t *)(o + L.ln_start); v.ln_items = (const int32_t *)(o + L.ln_items); v.n_ln_items = L.ln_cap;
        }
        if (pv.d_depth) { v.depth = pv.d_depth + (size_t)f * pv.dframe; v.pitch = pv.pitch; v.w = ctx->batch_w; v.h = ctx->batch_h; v.dfac = ctx->p.depth_map_factor; }
        v.sf = ctx->scale;
        v.bounds[0] = 0.f; v.bounds[1] = (float)ctx->batch_w; v.bounds[2] = 0.f; v.bounds[3] = (float)ctx->batch_h;      // as tail_batch_run builds the grids
    }
    return HVO_OK;
}

int stream_view(hvo_stream *s, int64_t ticket, const FrameNeed &nd, hipStream_t waits_on, FrameView &v)
{
    std::string &err = s->last_error;
    if (!stages_ok(nd, s->sp.stages)) return refuse(err, nd, "the stream must run ", nd.list_stream);
    if (nd.bf && !(s->sp.bf > 0)) return refuse(err, nd, "the stream was created with bf <= 0 (no mvuRight)");
    StreamSlot *B = slot_of(s, ticket);
    if (!B) return refuse(err, nd, "no such frame in the ring");
    if ((nd.depth & FV_DEPTH_STREAM) && !B->had_depth) return refuse(err, nd, "the frame was submitted without depth (", nd.depth_why, ")");
    if (hipSetDevice(s->p.device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const hipEvent_t ev[3] = { B->ev_orb, B->ev_lsd, B->ev_peac };
    for (int k = 0; k < 3; k++) {
        if (!(nd.events & (1u << k))) continue;
        if (nd.counts) ST_HIP(hipEventSynchronize(ev[k]));      // the counts arrived with the frame's download
        else ST_HIP(hipStreamWaitEvent(waits_on, ev[k], 0));
    }
    memset(&v, 0, sizeof(v));
    const OrbPlan &O = B->ctx->orb; const TailLayout &T = s->tl;
    v.ctx = B->ctx; v.n_kp = v.n_kl = -1;
    v.kp = O.d_kp; v.kp_un = B->d_kp_un; v.uright = (B->had_depth && s->sp.bf > 0) ? B->d_uright : nullptr; v.zdepth = v.uright ? B->d_zdepth : nullptr; v.desc = O.d_desc; v.d_nkp = O.d_nkp; v.kp_cap = s->kp_cap;
    v.kl = B->lv.d_kl; v.fn = B->lv.d_fn; v.ldesc = B->lv.d_desc; v.d_nkl = B->lv.d_nkl; v.nfeat = s->nfeat;
    if (B->d_tail) {
        v.l3d = (hvo_line3d *)(B->d_tail + T.lines3d); v.pclouds = (const hvo_plane_cloud *)(B->d_tail + T.pclouds); v.normals = (const hvo_surface_normal *)(B->d_tail + T.normals);
        v.cloud_xyz = (const float *)(B->d_tail + T.cloud); v.cloud_cap = T.cloud_cap;
        v.n_normals = T.n_normals; v.ln_start = (const int32_t *)(B->d_tail + T.ln_start); v.ln_items = (const int32_t *)(B->d_tail + T.ln_items);
    }
    v.sf = B->ctx->scale;
    for (int k = 0; k < 4; k++) v.bounds[k] = s->bounds[k];
    v.h_counts = (const int *)(B->h_out + s->lay.counts);
    frame_view_counts(v, nd.counts);
    if (nd.counts & FV_N_PC) {
        v.h_pclouds = (const hvo_plane_cloud *)(B->h_tail + T.pclouds);
        v.n_cloud = std::max(0, std::min(((const int *)(B->h_tail + T.counts))[0], T.cloud_cap));
    }
    if (nd.counts & FV_N_LN) {
        v.n_ln_items = ((const int *)(B->h_tail + T.counts))[3];
        if (v.n_ln_items < 0 || v.n_ln_items > T.ln_cap) { err = "line grid overflowed its capacity"; return HVO_ERR_CAPACITY; }
    }
    return HVO_OK;
}
