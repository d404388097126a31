// frame_view.hpp -- one resident frame as the resident operations see it, and the stream's ring the stream form is built from.
//
// A frame stays on the device in two shapes: frame f of a context's resident batch (hvo_batch_run) and a slot of a stream's ring
// (hvo_stream_submit).  Every resident operation -- Manhattan tracking, plane association, pose optimisation, line structure, the two
// local-map searches, bag of words, the PnP solver, the key-frame search, Fuse (points and lines), CreateNewMapPoints, CreateNewMapLinesConstraint, CreateNewKeyFrame's points and lines, the guided frame-to-frame matching -- reads the same arrays of it.  The two builders
// below are the only places that know where those arrays live in an OrbPlan, an LsdView, a PeacView, a TailLayout or a StreamSlot, and
// the only places that refuse a frame that lacks what an operation needs; the entry points and the *_run functions read a FrameView.
#pragma once
#include "hvo_internal.hpp"

struct FrameView {
    hvo_ctx *ctx;                           // owner: its call arena, pinned staging and timing events serve the *_run functions
    // key points: mvKeys, mvKeysUn (the batch carries no distortion: the same array), mvuRight (null: none held), descriptors
    const hvo_keypoint *kp, *kp_un; const float *uright, *zdepth; const uint8_t *desc; const int *d_nkp;   // zdepth: mvDepth beside mvuRight (stream only)
    int kp_cap, n_kp;                       // n_kp: host count clamped to [0, kp_cap]; -1: not fetched
    // key lines: records, line functions, descriptors
    const hvo_keyline *kl; const double *fn; const uint8_t *ldesc; const int *d_nkl;
    int nfeat, n_kl;                        // n_kl: host count clamped to [0, nfeat]; -1: not fetched
    // frame tail: 3-D lines (line structure rewrites A, B), plane records, surface normals, the line grid
    hvo_line3d *l3d; const hvo_plane_cloud *pclouds; const hvo_surface_normal *normals; int n_normals;
    const float *cloud_xyz; int cloud_cap;  // the plane tail's voxel clouds, packed xyz: record i's at [first, first + n_points)
    const hvo_plane_cloud *h_pclouds; int n_cloud;          // stream, with FV_N_PC: the records as they came down, and the cloud's point count clamped to cloud_cap
    const int32_t *ln_start, *ln_items; int n_ln_items;     // stream: the downloaded item count; batch: the list's capacity (its count lives on the device)
    // depth image (batch only: it holds no mvuRight, the kernels form it like k_stereo_from_rgbd)
    const uint16_t *depth; int pitch, w, h; float dfac;
    const float *sf;                        // mvScaleFactors of the owning context (HVO_MAX_LEVELS entries)
    float bounds[4];                        // mnMinX, mnMaxX, mnMinY, mnMaxY the grids were built with
    const int *h_counts;                    // stream: where the frame's downloaded counts land (frame_view_counts)
};

enum : unsigned { FV_N_KP = 1, FV_N_KL = 2, FV_N_LN = 4, FV_N_PC = 8 };     // host counts an operation reads (FV_N_PC: the plane records too)
enum : unsigned { FV_EV_ORB = 1, FV_EV_LSD = 2, FV_EV_PEAC = 4 };           // a slot's events an operation's inputs lie behind
enum : unsigned { FV_DEPTH_STREAM = 1, FV_DEPTH_BATCH = 2, FV_DEPTH = 3 };  // the forms that refuse a frame without depth

// What an operation needs of a frame: one row per operation, read by both builders.
struct FrameNeed {
    const char *what;                       // the head of every refusal: "<what>: ..."
    unsigned stages; bool any_lsd;          // HVO_STAGE_* bits that must all have run, and HVO_STAGE_LSD or HVO_STAGE_LSD_CULL
    unsigned depth; const char *depth_why;  // FV_DEPTH_*; what a frame without depth lacks
    bool uright, bf;                        // reads mvuRight where the frame has depth (batch: the depth image); refuses bf <= 0
    unsigned counts, events;                // FV_N_*: fetched to the host, which waits for the events; none: waits_on waits, the host does not
    const char *list_batch, *list_stream;   // the stages as the two forms' refusals name them
};

// the rows (frame_view.hip)
extern const FrameNeed need_manhattan, need_planes, need_pose, need_line_struct, need_local_lines, need_local_points, need_bow, need_bow_search, need_pnp, need_kf_search, need_fuse, need_new_points,
                       need_guided_points, need_line_match, need_new_lines, need_guided_lines, need_map_lines, need_plane_update, need_fuse_lines, need_new_keyframe;

// The first n frames of ctx's resident batch.  Refusals in the batch calls' order: n within the batch, stages, depth, bf; then
// hipSetDevice, the plan lookups and ONE count copy for all n frames.
int batch_views(hvo_ctx *ctx, int n, const FrameNeed &need, std::vector<FrameView> &views, float bf = 1.f);
// mvLevelSigma2 / mvInvLevelSigma2 (ORBextractor.cc:428-436) of ctx's pyramid; either may be null
void frame_level_sigma2(const hvo_ctx *ctx, float *sigma2, float *inv_sigma2);
// (re)read the host counts `which` of a stream view; the caller has waited for the frame's events
void frame_view_counts(FrameView &v, unsigned which);

// ---- the stream's ring (stream.hip) ----
#define ST_MAX_DEPTH 16

struct StreamSlot {
    hvo_ctx *ctx = nullptr;
    PeacView pv; LsdView lv;
    // pinned host
    uint8_t *h_gray = nullptr; uint16_t *h_depth = nullptr;
    char *h_out = nullptr;
    // device extras
    hvo_keypoint *d_kp_un = nullptr; float *d_uright = nullptr, *d_zdepth = nullptr;
    char *d_tail = nullptr, *d_tail_scratch = nullptr, *h_tail = nullptr;     // the Frame tail's result block (HBM + pinned copy) and scratch (tail.hip)
    hipEvent_t ev_gray = nullptr, ev_depth = nullptr, ev_orb = nullptr, ev_lsd = nullptr, ev_peac = nullptr;
    hipEvent_t ev_kern[3] = { nullptr, nullptr, nullptr };      // kernels done (before the downloads), per subsystem: latency accounting
    hipEvent_t ev_t0 = nullptr;
    int64_t ticket = -1; bool busy = false, had_depth = false;
    bool line_opt_done = false;            // hvo_stream_line_struct_optimize has rewritten this frame's 3-D lines
    BowState bow;                          // the frame's bag of words (hvo_stream_compute_bow), dropped when the slot takes its next frame
};

// layout of a slot's pinned result block
struct OutLayout {
    size_t counts, kp, desc, kp_un, uright, zdepth, kl, ldesc, fn, planes, labels, total;
};

struct hvo_stream {
    hvo_params p; hvo_stream_params sp;
    int depth = 0, w = 0, h = 0, kp_cap = 0, nfeat = 0;
    bool culled = false;
    StreamSlot slot[ST_MAX_DEPTH];
    OutLayout lay;
    int64_t next = 0;
    TailLayout tl; unsigned tail_stages = 0; double tail_dist_th = 0.05, tail_vp_th = 1.0 / 180.0 * 3.1415926535897932384626433832795;
    float bounds[4];                       // mnMinX, mnMaxX, mnMinY, mnMaxY (Frame::ComputeImageBounds)
    const float *bounds4() const { return bounds; }
    // matching scratch (device + pinned), sized for kp_cap queries
    char *d_ms = nullptr, *h_ms = nullptr; size_t ms_bytes = 0;
    // the local-map line search's scratch (hvo_stream_search_lines_by_projection_map): allocated on its first call, grow-only
    char *d_lm = nullptr, *h_lm = nullptr; size_t lm_dbytes = 0, lm_hbytes = 0;
    // Manhattan tracking's result block (hvo_stream_track_manhattan): allocated on its first call, grow-only
    char *d_mf = nullptr, *h_mf = nullptr; size_t mf_bytes = 0;
    hipStream_t s_match = nullptr;         // the matching calls run here, behind the two frames' events (not behind a frame's line chain)
    std::string last_error;
};

#define ST_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { s->last_error = std::string(#call) + ": " + hipGetErrorString(e_); return HVO_ERR_HIP; } } while (0)

static inline StreamSlot *slot_of(hvo_stream *s, int64_t ticket)
{
    if (ticket < 0 || ticket >= s->next || ticket < s->next - s->depth) return nullptr;
    StreamSlot &S = s->slot[ticket % s->depth];
    return S.ticket == ticket ? &S : nullptr;
}

// The frame `ticket` of the ring.  Refusals in the stream calls' order: stages, bf, the frame exists, depth; then hipSetDevice and the
// events: a need with host counts blocks the host on them (the counts arrived with the frame's download) and reads the counts, any other
// need only makes waits_on wait.
int stream_view(hvo_stream *s, int64_t ticket, const FrameNeed &need, hipStream_t waits_on, FrameView &view);
