/*
 * hvo.h -- C ABI of libhvo.so: the MI355X (gfx950) per-frame RGB-D front-end
 * (ORB + LSD/LBD lines + PEAC planes + Hamming matching) that replaces the bodies of
 *
 *   Frame::ExtractORB / ExtractORBNDepth   reference src/Frame.cc:886 / :874  (include/Frame.h:92-93)
 *       -> ORBextractor::operator()        reference src/ORBextractor.cc:1041 (include/ORBextractor.h:59-61)
 *   Frame::ExtractLSD                      reference src/Frame.cc:895          (include/Frame.h:96)
 *       -> LINEextractor::operator()       reference src/LineExtractor.cpp:329 (include/LineExtractor.h:193)
 *   Frame::ComputePlanes                   reference src/Frame.cc:2104         (include/Frame.h:415)
 *       -> PlaneDetection::readDepthImage / runPlaneDetection
 *                                          reference src/PlaneExtractor.cpp:26,60 (include/PlaneExtractor.h:50-54)
 *   ORBmatcher::DescriptorDistance         reference src/ORBmatcher.cc:1676    (include/ORBmatcher.h:44)
 *   LSDmatcher::match / matchNNR           reference src/LSDmatcher.cpp:828 / :803 (include/LSDmatcher.h:43)
 *   LSDmatcher::FrameBFMatch / SearchDouble reference src/LSDmatcher.cpp:942 / :902
 *   ORBmatcher::SearchByProjection         reference src/ORBmatcher.cc:1353 (frame to frame) and :45 (local map)
 * and, of the Frame constructor's post-processing:
 *   Frame::cullingLine                     reference src/Frame.cc:952
 *   Frame::UndistortKeyPoints / ComputeImageBounds / ComputeStereoFromRGBD / AssignFeaturesToGrid(ForLine)
 *                                          reference src/Frame.cc:1701 / 1733 / 1940 / 832 / 849
 *
 * The reference has no FFI of its own (single C++ process); INTEGRATION.md shows the
 * adaptor a maintainer adds to Frame.cc to call these entry points.
 *
 * Conventions
 *   - plain C types only; the caller owns every in/out buffer; nothing throws across the ABI
 *   - return value 0 = HVO_OK, negative = hvo_status; hvo_strerror() names it
 *   - empty image (NULL or w/h <= 0) -> *n = 0 and HVO_OK, like ORBextractor.cc:1044
 *   - a ctx is NOT thread-safe (neither is ORBextractor: mvImagePyramid is state); use one ctx
 *     per thread / per GPU.  Different ctx's may run concurrently (Frame.cc:210-215 pattern).
 *   - there is NO CPU fallback: every entry point fails with HVO_ERR_NO_DEVICE / HVO_ERR_HIP when
 *     the GPU or the gfx950 code object is unavailable.
 */
#ifndef HVO_H
#define HVO_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HVO_ABI_VERSION 3      /* 2: streamed-sequence entry points (hvo_stream_*), HVO_ERR_BUSY; 3: the Frame tail as pipeline stages
                                  (HVO_STAGE_LINES3D / _VP / _PLANE_TAIL / _GRIDS, hvo_frame_tail), hvo_stream_params grew three fields */

typedef enum {
    HVO_OK = 0,
    HVO_ERR_INVALID_ARG = -1,   /* NULL ctx/pointer, bad sizes */
    HVO_ERR_NO_DEVICE = -2,     /* no HIP device / wrong architecture */
    HVO_ERR_HIP = -3,           /* a HIP runtime call failed (hvo_last_error has the text) */
    HVO_ERR_UNSUPPORTED = -4,   /* image geometry outside what the kernels were sized for */
    HVO_ERR_CAPACITY = -5,      /* an internal fixed-capacity slab overflowed; results truncated */
    HVO_ERR_BAD_DTYPE = -6,     /* mirrors the CV_8UC1 assert (ORBextractor.cc:1048) and the
                                   CV_16U check (PlaneExtractor.cpp:34-38) */
    HVO_ERR_BUSY = -7           /* hvo_stream_submit: the ring slot still holds a frame that was not collected */
} hvo_status;

/* == cv::KeyPoint (28 bytes): what ORBextractor::operator() fills (ORBextractor.cc:1041-1103) */
typedef struct {
    float x, y;        /* pt, already multiplied by mvScaleFactor[octave] (ORBextractor.cc:1093-1099) */
    float size;        /* (int)(31 * scale) */
    float angle;       /* degrees [0,360), IC_Angle + fastAtan2 */
    float response;    /* FAST score */
    int32_t octave;
    int32_t class_id;  /* -1 */
} hvo_keypoint;

/* == cv::line_descriptor::KeyLine (68 bytes),
 * Thirdparty/line_descriptor/include/line_descriptor/descriptor_custom.hpp:105-144 */
typedef struct {
    float angle; int32_t class_id, octave;
    float pt_x, pt_y, response, size;
    float sx, sy, ex, ey;          /* startPointX/Y, endPointX/Y */
    float sox, soy, eox, eoy;      /* s/ePointInOctaveX/Y */
    float length; int32_t num_pixels;
} hvo_keyline;

/* one ahc::PlaneSeg of PlaneFitter::extractedPlanes (include/peac/AHCPlaneSeg.hpp:129-135) */
typedef struct {
    double normal[3], center[3], mse;
    int32_t n_points;   /* PlaneSeg::N */
    int32_t rid;        /* root block id */
} hvo_plane;

typedef struct {
    /* ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST): Tracking.cc:118-124,
     * Examples/RGB-D/TUM3.yaml:41-54 */
    int32_t orb_nfeatures;
    float   orb_scale_factor;
    int32_t orb_nlevels;
    int32_t orb_ini_th_fast;
    int32_t orb_min_th_fast;
    /* LINEextractor(numOctaves, scale, nLSDFeature, min_line_length): Tracking.cc:126-132,
     * TUM3.yaml:60-63.  NOTE the reference passes float scale into an int parameter (-> 1) and only
     * octave 0 runs for nLevels=1; num_octaves != 1 is HVO_ERR_UNSUPPORTED. */
    int32_t lsd_num_octaves;
    float   lsd_scale;
    int32_t lsd_nfeatures;
    /* camera / depth: TUM3.yaml:8-11,34; depth_map_factor = 1/DepthMapFactor as a float
     * (Tracking.cc:156-160) */
    float fx, fy, cx, cy;
    float depth_map_factor;
    /* execution */
    int32_t device;        /* HIP device ordinal */
    int32_t max_batch;     /* frames resident per batch call (>=1) */
} hvo_params;

typedef struct hvo_ctx hvo_ctx;

void        hvo_default_params(hvo_params *p);        /* TUM3.yaml values, device 0, max_batch 1 */
int         hvo_create(const hvo_params *p, hvo_ctx **out);
void        hvo_destroy(hvo_ctx *ctx);
const char *hvo_strerror(int status);
const char *hvo_last_error(const hvo_ctx *ctx);       /* text of the last HIP failure */
int         hvo_abi_version(void);

/* ---- single-frame entry points, host buffers (the drop-in boundary) ---- */

/* ORBextractor::operator()(image, mask(ignored), keypoints, descriptors).
 * gray: CV_8UC1 w x h, `stride` bytes per row.  kp/desc32: capacity `cap` entries (desc is cap x 32). */
int hvo_extract_orb(hvo_ctx *ctx, const uint8_t *gray, int w, int h, int stride,
                    hvo_keypoint *kp, uint8_t *desc32, int cap, int *n);

/* LINEextractor::operator()(image, mask(ignored), keylines, descriptors, lineVec2d).
 * linefn3: cap x 3 doubles (normalised 2-D line functions, LineExtractor.cpp:367-377). */
int hvo_extract_lsd(hvo_ctx *ctx, const uint8_t *gray, int w, int h, int stride,
                    hvo_keyline *kl, uint8_t *desc32, double *linefn3, int cap, int *n);

/* PlaneDetection::readDepthImage + runPlaneDetection on the raw 16-bit depth (Frame.cc:2104-2108).
 * depth: CV_16UC1, `stride` bytes per row.  labels: w*h int32 (PlaneFitter::membershipImg, -1 = none).
 * planes: extractedPlanes after refineDetails, sorted by N descending. */
int hvo_compute_planes(hvo_ctx *ctx, const uint16_t *depth, int w, int h, int stride,
                       int32_t *labels, hvo_plane *planes, int cap, int *n);

/* ---- Hamming matching (32-byte descriptors, row-major n x 32) ---- */
/* ORBmatcher::DescriptorDistance for every (q,t) pair */
int hvo_hamming_matrix(hvo_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, uint16_t *d);
/* cv::BFMatcher(NORM_HAMMING).knnMatch(q, t, 2) (LSDmatcher.cpp:811-812): two best train indices
 * per query, ascending distance, ties -> lower train index; -1 / INT32_MAX where nt < 2 */
int hvo_hamming_knn2(hvo_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt,
                     int32_t *idx2, int32_t *dist2);
/* LSDmatcher::matchNNR(desc1, desc2, nnr, matches_12): returns #matches in *n_matches */
int hvo_match_nnr(hvo_ctx *ctx, const uint8_t *d1, int n1, const uint8_t *d2, int n2, float nnr,
                  int32_t *matches12, int *n_matches);

/* LSDmatcher::FrameBFMatch(ldesc1, ldesc2, LineMatches, TH) (reference src/LSDmatcher.cpp:942-966): knnMatch(k = 2),
 * lineDescriptorMAD's nn12 threshold (1110-1135), accepted if d1 - d0 > threshold && d0 < th && d0 < nnratio * d1.
 * hvo_search_double = the core of LSDmatcher::SearchDouble / SearchByDescriptor (902-939, 865-899): FrameBFMatch in both
 * directions (the reference uses two threads), i -> j kept only if j -> i. */
int hvo_frame_bf_match(hvo_ctx *ctx, const uint8_t *d1, int n1, const uint8_t *d2, int n2, float th, float nnratio,
                       int32_t *matches12, int *n_matches);
int hvo_search_double(hvo_ctx *ctx, const uint8_t *d1, int n1, const uint8_t *d2, int n2, float th, float nnratio,
                      int32_t *matches12, int *n_matches);

/* LSDmatcher::SearchByGeomNApearance (reference src/LSDmatcher.cpp:36-108) on host arrays: see hvo_stream_match_lines_geom.  bounds4 = {mnMinX,
 * mnMaxX, mnMinY, mnMaxY} of the current frame; matches12 / accepted: n_last entries. */
int hvo_match_lines_geom(hvo_ctx *ctx, const uint8_t *d_last, const hvo_keyline *kl_last, const uint8_t *last_has_mapline, int n_last,
                         const uint8_t *d_cur, const hvo_keyline *kl_cur, int n_cur, float desc_th, const float bounds4[4],
                         int32_t *matches12, uint8_t *accepted, int *n_accepted);
/* LSDmatcher::SearchByProjection(Cur, Last, th) core (reference src/LSDmatcher.cpp:561-662, Frame::GetFeaturesInAreaForLine src/Frame.cc:1557-1627)
 * on host arrays: q_kl[i] = LastFrame.mvKeylinesUn of query i; t_linefn (nt x 3) = mvKeyLineFunctions; cell_start / cell_items = the current frame's
 * line grid as hvo_assign_lines_to_grid returns it; at most 2048 current lines and 65535 queries (HVO_ERR_UNSUPPORTED: match_idx / match_dist /
 * n_matches are left as they were).  See hvo_stream_search_lines_by_projection. */
int hvo_search_lines_by_projection(hvo_ctx *ctx, int nq, const float *q_xyxy, const hvo_keyline *q_kl, const uint8_t *q_desc, const uint8_t *q_blocks,
                                   const hvo_keyline *t_kl, const double *t_linefn, const uint8_t *t_desc, const uint8_t *t_occupied, int nt,
                                   const int32_t *cell_start, const int32_t *cell_items, const float bounds4[4], float th,
                                   int32_t *match_idx, int32_t *match_dist, int *n_matches);

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, mono) core (reference src/ORBmatcher.cc:1353-1497,
 * Frame::GetFeaturesInArea src/Frame.cc:1502-1555).  One query per last-frame map point that passed the
 * projection tests (:1381-1404): projected (u,v), radius = th * scale[octave], octave band [min,max] with
 * GetFeaturesInArea's conventions (min <= 0 and max < 0: no level check), ur = u - bf*invz (q_ur may be NULL),
 * key-point angle (rotation histogram) and q_blocks[i] != 0 when the map point has observations (the feature
 * it claims is then skipped by later queries, :1425-1427).  t_* describe the current frame: undistorted key
 * points, mvuRight (may be NULL), features already holding an observed map point (may be NULL), descriptors;
 * mnMin/Max are the frame's image bounds (64 x 48 grid).  match_idx[i] = current-frame index or -1.
 * At most 16384 queries and 65535 current-frame features (also for the _map and _tracked forms): more is HVO_ERR_UNSUPPORTED and
 * match_idx / match_dist are left as they were. */
int hvo_search_by_projection(hvo_ctx *ctx, const uint8_t *q_desc, int nq, const float *q_u, const float *q_v, const float *q_radius,
                             const int32_t *q_min_level, const int32_t *q_max_level, const float *q_ur, const float *q_angle,
                             const uint8_t *q_blocks, const hvo_keypoint *t_kp, const float *t_uright, const uint8_t *t_occupied,
                             const uint8_t *t_desc, int nt, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY,
                             int th_high, int check_orientation, int32_t *match_idx, int32_t *match_dist, int *n_matches);

/* Frame::ExtractLSD up to and including cullingLine (reference src/Frame.cc:895-934, 952-1116):
 * the LINEextractor output, then near-collinear segments merged (PointLineDistance / TwoLineAngle /
 * MergeTwoLines, 1117-1202), KeyLines rebuilt and re-sorted by response (class_id = rank), second LBD pass,
 * line functions.  isLineGood (the 3-D line fit with rand()) is not part of it.  Same conventions as
 * hvo_extract_lsd.  hvo_set_line_culling changes cullingLine's dis / angle (degrees) / endpoint_dis
 * (defaults 5, 2.5, 15: Frame.cc:934). */
int hvo_extract_lsd_culled(hvo_ctx *ctx, const uint8_t *gray, int w, int h, int stride,
                           hvo_keyline *kl, uint8_t *desc32, double *linefn3, int cap, int *n);
int hvo_set_line_culling(hvo_ctx *ctx, double dis, double angle_deg, double endpoint_dis);

/* Frame::isLineGood (reference src/Frame.cc:1205-1322): the 3-D line of every key line from the depth image --
 * <= 21 samples along the segment with nearest-pixel depth, LINEextractor::compPt3dCov (src/LineExtractor.cpp:44-97) and the RANSAC
 * on Mahalanobis point-line distances of LINEextractor::extract3dline_mahdist (220-327).  The reference draws from a time-seeded
 * rand(); here the caller passes a seed and every line draws from its own xorshift32 stream (seed, line index), so results are
 * reproducible and independent of the order of the lines.  depth / intrinsics as in hvo_stereo_from_rgbd. */
typedef struct {
    double A[3], B[3];          /* mvLines3D[i] (camera frame); zeros when no line was fitted */
    double line_nor[3];         /* mvLineNor[i] = A x B; (-1,-1,-1) when none */
    float  line_eq[3];          /* mvLineEq[i] = (B - A) / |B - A| (float); (-1,-1,-1) when none */
    int32_t good;               /* 1: |A - B| > 0.02: the line enters mVF3DLines */
    int32_t n_samples;          /* samples with a valid depth (<= 21) */
    int32_t n_inliers;          /* RandomLine3d::pts.size() */
    uint32_t inlier_mask;       /* bit j: valid sample j is an inlier */
    int32_t pad;
} hvo_line3d;
int hvo_lines_3d(hvo_ctx *ctx, const hvo_keyline *kl, int n, const uint16_t *depth, int w, int h, int stride, uint32_t seed, hvo_line3d *out);

/* LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th), the local-map line search (reference src/LSDmatcher.cpp:709-801 over
 * Frame::GetFeaturesInAreaForLine with its default direction gate 0.998, src/Frame.cc:1557-1627; called by Tracking::SearchLocalLines,
 * src/Tracking.cc:3279-3355) on host arrays.  One query per map line with mbTrackInView && !isBad(), in vpMapLines order (the caller filters):
 * q_xyxy[4 i ..] = (mTrackProjX1, mTrackProjY1, mTrackProjX2, mTrackProjY2), q_view_cos[i] = mTrackViewCos (radius 5 when > 0.998, else 8:
 * RadiusByViewingCos 1436-1442; times th when th != 1), q_wvec[3 i ..] = GetWorldVector(), q_desc (nq x 32) = GetDescriptor(), q_blocks[i] != 0
 * when Observations() > 0 (may be NULL: none).  mnTrackScaleLevel and eval_orient are not read by the reference.  t_l3d = the current frame's
 * mvLines3D (hvo_lines_3d): a line is skipped when |(A - B) . wvec| / (|A - B| |wvec|) < cos 15 degrees (NaN passes); t_occupied (may be NULL):
 * lines already holding a map line with observations.  Best and second best distance; accepted if best <= 95 and not (same octave && best >
 * nn_ratio * second).  match_idx[i] = the current line or -1, match_dist[i] = its distance or 256; the reference assigns F.mvpMapLines[match_idx[i]]
 * in query order (a later acceptance overwrites a claim by a map line without observations).  At most 2048 current lines and 16384 queries
 * (HVO_ERR_UNSUPPORTED: match_idx / match_dist / n_matches are left as they were).  See hvo_stream_search_lines_by_projection_map. */
int hvo_search_lines_by_projection_map(hvo_ctx *ctx, int nq, const float *q_xyxy, const float *q_view_cos, const double *q_wvec,
                                       const uint8_t *q_desc, const uint8_t *q_blocks,
                                       const hvo_keyline *t_kl, const double *t_linefn, const hvo_line3d *t_l3d, const uint8_t *t_desc, const uint8_t *t_occupied, int nt,
                                       const int32_t *cell_start, const int32_t *cell_items, const float bounds4[4], float th, float nn_ratio,
                                       int32_t *match_idx, int32_t *match_dist, int *n_matches);

/* The vanishing-point clustering of the key lines that the Frame constructor runs on every frame (reference src/Frame.cc:330-337,
 * SURVEY.md 8f.4): Frame::getVPHypVia2Lines (442-545: 105 random pairs of lines x 360 rotations = 37 800 hypotheses of three
 * orthogonal vanishing directions), getSphereGrids (546-650: the 90 x 360 grid of pairwise line intersections, weighted, 3x3
 * smoothed), getBestVpsHyp (651-707: the first hypothesis with the largest sum of its three cells) and line2Vps (708-778: the
 * cluster of every line, thAngle = 1 degree in Frame.h:365).  kl are the (undistorted) key lines (mvKeylinesUn), intrinsics
 * the context's.  The reference draws from a time-seeded rand(); the caller passes a seed, group i of 360 hypotheses draws its
 * pair of lines from its own xorshift32 stream (seed, i).  vp_idx[i] = 0..2 (isStructLine[i] = true) or 3 (none);
 * grid (optional) receives the 90 x 360 smoothed sphere grid.  n < 2: nothing is computed (as the reference), all vp_idx = 3.
 * This host-array form accepts 0 <= n <= 1024 lines; more is HVO_ERR_INVALID_ARG and nothing is launched.  The resident forms
 * (HVO_STAGE_VP below) are sized by the context's lsd_nfeatures instead and take every key line of the frame. */
typedef struct {
    double vps[3][3];           /* tmp_vps: the best hypothesis, three unit vectors (camera frame) */
    double score;               /* its summed grid length (0 when no hypothesis scored) */
    int32_t best;               /* its index, group * 360 + rotation */
    int32_t n_hypotheses;       /* 37 800 */
} hvo_vp_result;
int hvo_vanishing_points(hvo_ctx *ctx, const hvo_keyline *kl, int n, uint32_t seed, double th_angle,
                         hvo_vp_result *res, int32_t *vp_idx, double *grid);

/* The tail of Frame::ComputePlanes after the plane detector (reference src/Frame.cc:2110-2212) and Frame::MaxPointDistanceFromPlane
 * (2214-2274), SURVEY.md 8f.3.  labels / planes are the outputs of hvo_compute_planes for the same depth image.
 * hvo_plane_clouds: per plane the points of its pixels (float), pcl::VoxelGrid(0.1 m), the gate |n.p + d| <= dist_th
 * (Plane.DistanceThreshold of the settings file) and the pcl::SACSegmentation refit with the sign rule; valid planes are the
 * entries of mvPlanePoints / mvPlaneCoefficients, in order.  cloud_xyz (cap x 3 floats) receives every plane's voxel cloud,
 * plane i at [first, first + n_points).  PCL's semantics are restated (it is not vendored by the reference): oracle/planes_tail.c.
 * hvo_surface_normals: the 1/3-resolution cloud and pcl::IntegralImageNormalEstimation(AVERAGE_3D_GRADIENT, 0.05, 10) at the odd
 * grid positions = vSurfaceNormal (normal NaN where PCL leaves it undefined); needs (h/3/2) * (w/3/2) entries (80 x 107 for 640x480). */
typedef struct {
    float coef[4];              /* mvPlaneCoefficients entry when valid (refit, sign rule applied), else (n, -n.c) of the extracted plane */
    int32_t valid;              /* 1: passed the gate and the refit: the plane enters mvPlanePoints / mvPlaneCoefficients */
    int32_t gate_ok;            /* 1: no voxel point farther than dist_th from the extracted plane */
    int32_t first, n_points;    /* its voxel-grid cloud in cloud_xyz */
    int32_t n_pixels;           /* plane_vertices_[i].size() */
    int32_t n_inliers;          /* inliers of the refined model */
} hvo_plane_cloud;
typedef struct { float normal[3]; float position[3]; int32_t frame_x, frame_y; } hvo_surface_normal;   /* SurfaceNormal: normal, cameraPosition, FramePosition */
int hvo_plane_clouds(hvo_ctx *ctx, const uint16_t *depth, int w, int h, int stride, const int32_t *labels, const hvo_plane *planes, int n_planes,
                     double dist_th, float *cloud_xyz, int cap, hvo_plane_cloud *out, int *n_total);
int hvo_surface_normals(hvo_ctx *ctx, const uint16_t *depth, int w, int h, int stride, hvo_surface_normal *out, int cap, int *n);

/* Manhattan::computeNormalsLPVO (reference src/Manhattan.cpp:237-393, the second half of SURVEY.md 8f.4; run by the RGB-D Frame constructor
 * through Frame::ExtractMainImgPtNormals, src/Frame.cc:222, until the coarse Manhattan frame is initialised): surface normals from 10 x 10
 * box averages of the central-difference tangents at every 15th pixel.  The INTENDED reading is implemented -- depth in metres as CV_32F,
 * integral images with their zero row / column removed -- not what the reference binary computes: as compiled it reads the raw CV_16U image
 * through at<float> and moves half rows of its CV_64F integral images (undefined behaviour; csrc/lpvo.hip).
 * normals3: cap x 3 doubles (unit, or 0 when the cross product vanishes); depth_out: the sample's z; pixel2: (u, v).  *n = samples found. */
int hvo_normals_lpvo(hvo_ctx *ctx, const uint16_t *depth, int w, int h, int stride, double *normals3, float *depth_out, int32_t *pixel2, int cap, int *n);

/* ---- Frame post-processing of the outputs above ----------------------------------------
 * dist5 = {k1, k2, p1, p2, k3} (Camera.k1.. of the settings file; k3 = 0 when absent); the intrinsics are the
 * context's (hvo_params fx, fy, cx, cy).  The 64 x 48 grids (FRAME_GRID_COLS x FRAME_GRID_ROWS) are returned as
 * CSR: cell = col * 48 + row (the reference's mGrid[col][row]), cell_start has 64*48+1 entries, cell_items holds
 * feature indices in the reference's push order. */
#define HVO_GRID_COLS 64
#define HVO_GRID_ROWS 48
/* Frame::UndistortKeyPoints (reference src/Frame.cc:1701-1731): k1 == 0 copies the key points (1703-1707), else
 * cv::undistortPoints(pts, K, dist, Mat(), K) replaces x, y and keeps the other fields. */
int hvo_undistort_keypoints(hvo_ctx *ctx, const hvo_keypoint *kp, int n, const float dist5[5], hvo_keypoint *kp_un);
/* Frame::ComputeImageBounds (reference src/Frame.cc:1733-1762): bounds4 = {mnMinX, mnMaxX, mnMinY, mnMaxY} */
int hvo_image_bounds(hvo_ctx *ctx, int w, int h, const float dist5[5], float bounds4[4]);
/* Frame::AssignFeaturesToGrid (reference src/Frame.cc:832-847, PosInGrid 1680-1690); cell_items needs n entries */
int hvo_assign_features_to_grid(hvo_ctx *ctx, const hvo_keypoint *kp_un, int n, const float bounds4[4],
                                int32_t *cell_start, int32_t *cell_items, int *n_assigned);
/* Frame::AssignFeaturesToGridForLine (reference src/Frame.cc:849-872, src/lineIterator.cpp:34-76); a line enters
 * every cell its Bresenham walk visits; HVO_ERR_CAPACITY (with *n_items = the needed count) if cap is too small */
int hvo_assign_lines_to_grid(hvo_ctx *ctx, const hvo_keyline *kl, int n, const float bounds4[4],
                             int32_t *cell_start, int32_t *cell_items, int cap, int *n_items);

/* ORBmatcher::SearchByProjection(Frame &F, vpMapPoints, th) core (reference src/ORBmatcher.cc:45-132), the local-map
 * variant: one query per map point in view (projected u, v = mTrackProjX/Y; radius = RadiusByViewingCos * th *
 * scale[level]; levels [level-1, level]; ur = mTrackProjXR), best and second-best distance, accepted if best <= th_high
 * and not (both in the same octave && best > nn_ratio * second) (:117-124).  t_occupied / q_blocks as above. */
int hvo_search_by_projection_map(hvo_ctx *ctx, const uint8_t *q_desc, int nq, const float *q_u, const float *q_v, const float *q_radius,
                                 const int32_t *q_min_level, const int32_t *q_max_level, const float *q_ur, const uint8_t *q_blocks,
                                 const hvo_keypoint *t_kp, const float *t_uright, const uint8_t *t_occupied, const uint8_t *t_desc, int nt,
                                 float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, int th_high, float nn_ratio,
                                 int32_t *match_idx, int32_t *match_dist, int *n_matches);

/* The same search from the tracker's own per-point fields, its prologue (src/ORBmatcher.cc:55-70, RadiusByViewingCos 134-140) on the
 * device: one query per map point in view (mbTrackInView, not bad) with mTrackProjX / mTrackProjY / mTrackProjXR (may be NULL),
 * mnTrackScaleLevel and mTrackViewCos; radius = (viewCos > 0.998 ? 2.5 : 4.0) [* th when th != 1] * scale[level], levels
 * [level - 1, level].  Everything else as hvo_search_by_projection_map. */
int hvo_search_by_projection_tracked(hvo_ctx *ctx, const uint8_t *q_desc, int nq, const float *proj_x, const float *proj_y, const float *proj_xr,
                                     const int32_t *level, const float *view_cos, const uint8_t *q_blocks, float th,
                                     const hvo_keypoint *t_kp, const float *t_uright, const uint8_t *t_occupied, const uint8_t *t_desc, int nt,
                                     float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, int th_high, float nn_ratio,
                                     int32_t *match_idx, int32_t *match_dist, int *n_matches);

/* Frame::ComputeStereoFromRGBD (reference src/Frame.cc:1940-1961): uright[i] = kp_un[i].x - bf/d and zdepth[i] = d
 * where d = depth(v,u) * depth_map_factor at the truncated key-point position, if 0 < d < 7; else -1. */
int hvo_stereo_from_rgbd(hvo_ctx *ctx, const hvo_keypoint *kp, const hvo_keypoint *kp_un, int n,
                         const uint16_t *depth, int w, int h, int stride, float bf, float *uright, float *zdepth);

/* ---- batch entry points (config 4: independent frames; inputs stay resident in HBM) ---- */
#define HVO_STAGE_ORB    1u
#define HVO_STAGE_LSD    2u
#define HVO_STAGE_PLANES 4u
#define HVO_STAGE_ALL    7u
#define HVO_STAGE_LSD_CULL 8u    /* HVO_STAGE_LSD followed by Frame::cullingLine: the frame's kl / ldesc / linefn are the merged lines */
/* The rest of the Frame constructor (reference src/Frame.cc:205-233) as stages of the same pipelines: they read the key lines, depth image,
 * label image, planes and key points where the stages above left them in HBM (nothing is uploaded twice, nothing allocated per frame). */
#define HVO_STAGE_LINES3D    16u  /* Frame::isLineGood of every key line (src/Frame.cc:934-939, 1205-1322) = hvo_lines_3d; needs LSD + depth */
#define HVO_STAGE_VP         32u  /* vanishing points + line2Vps (src/Frame.cc:328-337, 442-778) = hvo_vanishing_points; needs LSD */
/* HVO_STAGE_VP runs on all of a frame's key lines, up to lsd_nfeatures: the 1024-line limit of hvo_vanishing_points does not apply (its
 * scratch is 20 bytes per PAIR of lsd_nfeatures lines and frame slot: 16 MB at 1280).  It returns no sphere grid. */
#define HVO_STAGE_PLANE_TAIL 64u  /* ComputePlanes' tail (src/Frame.cc:2110-2274) = hvo_plane_clouds + hvo_surface_normals; needs PLANES */
#define HVO_STAGE_GRIDS     128u  /* AssignFeaturesToGrid / ForLine (src/Frame.cc:832-872) = hvo_assign_*_to_grid; needs ORB + LSD */
#define HVO_STAGE_FRAME     (HVO_STAGE_ORB | HVO_STAGE_LSD_CULL | HVO_STAGE_LSD | HVO_STAGE_PLANES | HVO_STAGE_LINES3D | HVO_STAGE_VP | HVO_STAGE_PLANE_TAIL | HVO_STAGE_GRIDS)

typedef struct {
    const uint8_t  *gray;  int gray_stride;    /* bytes */
    const uint16_t *depth; int depth_stride;   /* bytes; may be NULL when planes are not requested */
} hvo_frame_in;

typedef struct {
    hvo_keypoint *kp; uint8_t *desc; int kp_cap; int n_kp;
    hvo_keyline *kl; uint8_t *ldesc; double *linefn; int kl_cap; int n_kl;
    int32_t *labels; hvo_plane *planes; int pl_cap; int n_planes;
    int status;                                  /* per-frame hvo_status */
    int8_t *labels8;                             /* optional: the label image as int8 (w*h bytes, -1 = none; plane ids < 64), i.e. as it
                                                    crosses PCIe, without the widening to CV_32S that `labels` gets (ABI version 2) */
} hvo_frame_out;

/* Results of the tail stages for one frame; any pointer may be NULL.  Capacities: lines3d / vp_idx kl_cap entries, plane_clouds 64,
 * cloud_xyz cloud_cap x 3 floats (hvo_tail_capacity), normals normals_cap, pt_cell_start / ln_cell_start 64*48+1, pt_cell_items kp_cap,
 * ln_cell_items kl_cap * 128.  The random draws of isLineGood and of the vanishing-point hypotheses use seed + frame index (batch) or
 * seed + ticket (stream): hvo_set_tail_params / hvo_stream_params.seed. */
typedef struct {
    hvo_line3d *lines3d;
    hvo_vp_result *vp; int32_t *vp_idx;
    hvo_plane_cloud *plane_clouds; float *cloud_xyz; int cloud_cap; int n_cloud;
    hvo_surface_normal *normals; int normals_cap; int n_normals;
    int32_t *pt_cell_start, *pt_cell_items; int pt_items_cap; int n_pt_items;
    int32_t *ln_cell_start, *ln_cell_items; int ln_items_cap; int n_ln_items;
    int status;
} hvo_frame_tail;
/* capacities of the tail results for a geometry: voxel-cloud points per frame, surface normals, line-grid items */
int hvo_tail_capacity(int kl_cap, int w, int h, int *cloud_cap, int *n_normals, int *ln_items_cap);
/* seed of the random draws, Plane.DistanceThreshold (default 0.05) and line2Vps' angle in radians (default 1 degree) for hvo_batch_run's tail stages */
int hvo_set_tail_params(hvo_ctx *ctx, uint32_t seed, double plane_dist_th, double vp_th_angle);
/* results of the tail stages of the first n frames of the resident batch (after hvo_batch_run with those stages) */
int hvo_batch_download_tail(hvo_ctx *ctx, int n, hvo_frame_tail *out);

/* host -> HBM copy of n (<= max_batch) frames of one geometry */
int hvo_batch_upload(hvo_ctx *ctx, int n, const hvo_frame_in *in, int w, int h);
/* enqueue every kernel of the selected stages for the resident batch and wait for completion */
int hvo_batch_run(hvo_ctx *ctx, unsigned stages);
/* HBM -> host copy of results (any pointer in hvo_frame_out may be NULL to skip it) */
int hvo_batch_download(hvo_ctx *ctx, int n, hvo_frame_out *out);
/* Result slabs in device memory (the only multi-GPU exchange is a gather of these).  One record of *slab_bytes per
 * frame: int32 {n_kp, n_kl, n_planes, status}, kp[kp_cap] (28 B), desc[kp_cap] (32 B), kl[kl_cap] (68 B), ldesc[kl_cap] (32 B),
 * linefn[kl_cap] (3 doubles), planes[pl_cap] (64 B); entries beyond the counts are zero.  hvo_batch_pack_results writes the first
 * n frames of the resident batch to d_slabs, a DEVICE pointer with room for n * slab_bytes (e.g. the tensor handed to
 * ncclAllGather); stages that did not run report zero counts. */
int hvo_batch_slab_layout(hvo_ctx *ctx, int *kp_cap, int *kl_cap, int *pl_cap, size_t *slab_bytes);
int hvo_batch_pack_results(hvo_ctx *ctx, int n, void *d_slabs);
/* The same with options: HVO_SLAB_LABELS appends the frame's label image (membershipImg as int8, -1 = no plane; w * h bytes rounded up
 * to 16) to every slab, so that the one collective of a multi-GPU caller also carries the plane labels -- 307 200 B per 640x480 frame on
 * top of the 93.7 KB of the records (a 256-frame gather over xGMI grows from 24 MB to 103 MB: ~0.7 ms per GPU at 153 GB/s per link). */
#define HVO_SLAB_LABELS 1u
int hvo_batch_slab_layout_ex(hvo_ctx *ctx, unsigned flags, int *kp_cap, int *kl_cap, int *pl_cap, size_t *labels_off, size_t *slab_bytes);
int hvo_batch_pack_results_ex(hvo_ctx *ctx, int n, void *d_slabs, unsigned flags);
/* Double-buffered batches: the end-to-end rate of consecutive batches at the resident batch's efficiency.  While the resident batch runs,
 * the NEXT batch's images go up into staging slabs (hvo_batch_stage_upload: enqueued on a copy stream of its own, returns at once) and the
 * LAST batch's results come down from one packed slab (hvo_batch_results_async: hvo_batch_pack_results_ex into a device slab, then ONE
 * contiguous copy into `host_slabs`, n * slab_bytes of page-locked memory; hvo_batch_results_wait waits for it).  hvo_batch_commit_staged
 * waits for the staged upload and makes it the resident batch (a device-to-device copy: ~6 ms per 8192 frames).  One host thread:
 *     stage_upload(0); commit
 *     loop k:  stage_upload(k + 1);  hvo_batch_run;  results_async(k);  commit            -- run(k) overlaps upload(k + 1) and download(k - 1)
 * Staging never rebuilds the plans under a resident batch (that would blank its slabs before it runs): while one is resident, a staged
 * batch must have its geometry, no more frames than the plans hold, and depth only if the plane plan exists (the resident batch had depth).
 * Otherwise the call returns HVO_ERR_INVALID_ARG and hvo_last_error says so; hvo_batch_upload of the new geometry or size comes first. */
int hvo_batch_stage_upload(hvo_ctx *ctx, int n, const hvo_frame_in *in, int w, int h);
int hvo_batch_commit_staged(hvo_ctx *ctx);
int hvo_batch_results_async(hvo_ctx *ctx, int n, unsigned flags, void *host_slabs);
int hvo_batch_results_wait(hvo_ctx *ctx);
/* upload + run + download */
int hvo_extract_batch(hvo_ctx *ctx, int n, const hvo_frame_in *in, hvo_frame_out *out, int w, int h,
                      unsigned stages);

/* ---- streamed sequence (BASELINE config 5) -----------------------------------------------------------------
 * The reference constructs one Frame per camera image (src/Tracking.cc:262 -> Frame ctor src/Frame.cc:205-233: ExtractORB ||
 * ExtractLSD || ComputePlanes on three threads, then UndistortKeyPoints / ComputeStereoFromRGBD) and matches it against the
 * previous frame (TrackWithMotionModel: SearchByProjection(Cur, Last) src/Tracking.cc:2396, LSDmatcher::match(Last.mLdesc,
 * Cur.mLdesc) src/Tracking.cc:2299 -> src/LSDmatcher.cpp:42).  A hvo_stream keeps `depth` frames in flight on the GPU (one
 * frame's serial chains -- AHC, region growing -- leave most of the chip idle, the next frames run beside them) and the
 * results of the last `depth` frames resident in HBM, so the frame-to-frame matching reads descriptors, undistorted key
 * points and mvuRight where they were produced: only the tracker's per-query projections cross PCIe.
 *   submit  : copies the images into pinned staging, enqueues uploads + every kernel + result downloads, returns at once
 *   collect : waits for that frame and copies its results out (tickets may be collected in any order; a slot is reused
 *             by ticket + depth, which is refused with HVO_ERR_BUSY until the slot's frame was collected)
 * A frame stays matchable until `depth` newer frames have been submitted.  Not thread-safe. */
typedef struct hvo_stream hvo_stream;
typedef struct {
    int32_t  width, height;
    int32_t  depth;             /* frames in flight / resident (ring slots), 2..16 */
    uint32_t stages;            /* HVO_STAGE_* mask */
    float    dist5[5];          /* k1 k2 p1 p2 k3 for UndistortKeyPoints (k1 == 0: key points are copied, Frame.cc:1703-1707) */
    float    bf;                /* ComputeStereoFromRGBD's mbf; <= 0: mvuRight / mvDepth are not computed */
    uint32_t seed;              /* tail stages: frame `ticket` draws with seed + ticket (ABI 3) */
    float    plane_dist_th;     /* Plane.DistanceThreshold of the settings file; <= 0: 0.05 */
    float    vp_th_angle;       /* line2Vps' thAngle in radians; <= 0: 1 degree (Frame.h:365) */
} hvo_stream_params;
#define HVO_LINE_MATCH_NNR 0    /* LSDmatcher::match -> matchNNR (src/LSDmatcher.cpp:803-863): d0 < nnr * d1 */
#define HVO_LINE_MATCH_BF 1     /* LSDmatcher::FrameBFMatch (942-966) */
#define HVO_LINE_MATCH_DOUBLE 2 /* LSDmatcher::SearchDouble (902-939): both directions + mutual check */

int  hvo_stream_create(const hvo_params *p, const hvo_stream_params *sp, hvo_stream **out);
void hvo_stream_destroy(hvo_stream *s);
const char *hvo_stream_last_error(const hvo_stream *s);
/* capacities of the per-frame result arrays (key points / key lines / planes) */
int  hvo_stream_capacity(const hvo_stream *s, int *kp_cap, int *kl_cap, int *pl_cap);
/* Frame::ComputeImageBounds with the stream's distortion: {mnMinX, mnMaxX, mnMinY, mnMaxY} */
int  hvo_stream_image_bounds(const hvo_stream *s, float bounds4[4]);
/* depth may be NULL when planes are not requested (then mvuRight / mvDepth are not computed either) */
int  hvo_stream_submit(hvo_stream *s, const uint8_t *gray, int gray_stride, const uint16_t *depth, int depth_stride, int64_t *ticket);
int  hvo_stream_poll(hvo_stream *s, int64_t ticket);                 /* 1: complete, 0: still running */
/* out as in hvo_batch_download (any pointer may be NULL); kp_un / uright / zdepth: kp_cap entries, may be NULL */
int  hvo_stream_collect(hvo_stream *s, int64_t ticket, hvo_frame_out *out, hvo_keypoint *kp_un, float *uright, float *zdepth);
/* results of the frame's tail stages (HVO_STAGE_LINES3D / _VP / _PLANE_TAIL / _GRIDS of hvo_stream_params.stages); call BEFORE hvo_stream_collect
 * releases the slot, or instead of it with out == NULL there: hvo_stream_collect_tail waits for the frame like hvo_stream_collect does */
int  hvo_stream_collect_tail(hvo_stream *s, int64_t ticket, hvo_frame_tail *tail);
/* device time from the start of the frame's upload to the end of its ORB / line / plane kernels (ms) */
int  hvo_stream_stage_ms(hvo_stream *s, int64_t ticket, float ms3[3]);
/* SearchByProjection(Cur, Last) core between two resident frames.  Query i = last-frame feature q_index[i] (its descriptor and
 * key-point angle are read from the last frame's slot; pass q_desc (nq x 32) when pMP->GetDescriptor() differs from the frame's
 * own descriptor); q_u .. q_blocks and t_occupied (n_kp(cur) entries, may be NULL) as in hvo_search_by_projection. */
int  hvo_stream_search_by_projection(hvo_stream *s, int64_t cur, int64_t last, int nq, const int32_t *q_index, const uint8_t *q_desc,
                                     const float *q_u, const float *q_v, const float *q_radius, const int32_t *q_min_level, const int32_t *q_max_level,
                                     const float *q_ur, const uint8_t *q_blocks, const uint8_t *t_occupied, int th_high, int check_orientation,
                                     int32_t *match_idx, int32_t *match_dist, int *n_matches);
/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) WHOLE, between two resident frames (src/ORBmatcher.cc:1353-1497):
 * the projection prologue (1364-1405) runs on the device too -- x3Dc = Rcw x3Dw + tcw, invzc, (u, v), the image-bounds tests,
 * bForward / bBackward from tlc = Rlw twc + tlw against mb, radius = th * mvScaleFactors[octave of the last frame's feature], the octave
 * band and ur = u - mbf invzc -- and feeds the search core where it stands: per query only the map point's world position crosses PCIe.
 * Tcw / Tlw: rows 0..2 of CurrentFrame.mTcw / LastFrame.mTcw, row-major 3 x 4.  Query i = last-frame feature q_index[i] whose map point
 * (not an outlier) has world position x3Dw[3 i ..]; q_blocks / q_desc / t_occupied as in hvo_stream_search_by_projection.  A point that
 * fails a projection test is never searched (match_idx -1).  q_uv (may be NULL, nq x 2): the projections, 1e30 where none was searched. */
typedef struct { float fx, fy, cx, cy, bf, b; } hvo_camera;      /* Frame::fx fy cx cy mbf mb */
int  hvo_stream_project_last(hvo_stream *s, int64_t cur, int64_t last, const hvo_camera *cam, const float Tcw[12], const float Tlw[12],
                             int nq, const int32_t *q_index, const float *x3Dw, const uint8_t *q_blocks, const uint8_t *q_desc,
                             const uint8_t *t_occupied, float th, int mono, int th_high, int check_orientation,
                             int32_t *match_idx, int32_t *match_dist, int *n_matches, float *q_uv);
/* line matching between two resident frames: query = lines of `from`, train = lines of `to`; matches12 needs kl_cap entries,
 * *n_from receives n_kl(from) */
int  hvo_stream_match_lines(hvo_stream *s, int64_t from, int64_t to, int mode, float th, float nnratio, int32_t *matches12, int *n_from, int *n_matches);

/* LSDmatcher::SearchByGeomNApearance(CurrentFrame, LastFrame, desc_th, matches_12) WHOLE between two resident frames (reference
 * src/Tracking.cc:2299 -> src/LSDmatcher.cpp:36-108; computeAngle2D 20-34): match(Last.mLdesc, Cur.mLdesc) and then, per pair, the 20-degree
 * angle gate on the in-octave end points and the position gate (start OR end point within a tenth of the image bounds in both axes).
 * last_has_mapline (n_kl(last) flags, NULL = every line has one): LastFrame.mvpMapLines[i] != NULL; a line without one is passed over and keeps
 * its descriptor match in matches12, as in the reference (57).  accepted[i] = 1 where the reference assigns CurrentFrame.mvpMapLines[matches12[i]]
 * = LastFrame.mvpMapLines[i]; *n_accepted = the reference's return value.  matches12 / accepted need kl_cap entries. */
int  hvo_stream_match_lines_geom(hvo_stream *s, int64_t cur, int64_t last, float desc_th, const uint8_t *last_has_mapline,
                                 int32_t *matches12, uint8_t *accepted, int *n_last, int *n_accepted);
/* LSDmatcher::SearchByProjection(CurrentFrame, LastFrame, th) core between two resident frames (reference src/LSDmatcher.cpp:561-662 over
 * Frame::GetFeaturesInAreaForLine src/Frame.cc:1557-1627), the tracker's retry when the descriptor match finds too few lines.  Query i =
 * last-frame line q_index[i] whose map line passed isInFrustum: q_xyxy[4 i ..] = (mTrackProjX1, mTrackProjY1, mTrackProjX2, mTrackProjY2);
 * q_desc (nq x 32, may be NULL: the last frame's own descriptors) = pML->GetDescriptor(); q_blocks[i] != 0 when the map line has observations;
 * t_occupied (n_kl(cur) flags, may be NULL): current lines already holding an observed map line.  The current frame's key lines, line functions,
 * descriptors and line grid are the resident ones: the stream must run HVO_STAGE_GRIDS.  match_idx[i] = current line or -1 (accepted at <= 95). */
int  hvo_stream_search_lines_by_projection(hvo_stream *s, int64_t cur, int64_t last, int nq, const int32_t *q_index, const float *q_xyxy, const uint8_t *q_desc,
                                           const uint8_t *q_blocks, const uint8_t *t_occupied, float th, int32_t *match_idx, int32_t *match_dist, int *n_matches);
/* LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) on the resident frame `cur` (reference src/LSDmatcher.cpp:709-801): its key lines, line
 * functions, descriptors, line grid and 3-D lines are read on the device; per query only the map line's fields go up (as in
 * hvo_search_lines_by_projection_map; t_occupied: n_kl(cur) flags, may be NULL).  The stream must run HVO_STAGE_GRIDS and HVO_STAGE_LINES3D and the
 * frame must have been submitted with depth (else HVO_ERR_INVALID_ARG).  Its scratch is allocated on the first call and grows on demand. */
int  hvo_stream_search_lines_by_projection_map(hvo_stream *s, int64_t cur, int nq, const float *q_xyxy, const float *q_view_cos,
                                               const double *q_wvec, const uint8_t *q_desc, const uint8_t *q_blocks, const uint8_t *t_occupied, float th, float nn_ratio,
                                               int32_t *match_idx, int32_t *match_dist, int *n_matches);

/* ---- Manhattan-frame tracking (csrc/manhattan.hip) ----
 * Tracking::TrackManhattanFrame(R_last, vSurfaceNormal, mVF3DLines) (reference src/Tracking.cc:1172-1348, called on every tracked frame at
 * :706 and at initialisation at :659), with ProjectSN2Conic (953-1026), ProjectSN2MF (1028-1150) and MeanShift (1152-1170).  Per axis a = 1..3
 * the normals within asin(sin 0.2018) and the 3-D line directions within asin(sin 0.1018) of column a-1 of R_last form the cone (numInCone
 * counts the normals); the threshold is size/20, or (b + a) / 2 of the sorted counts when the middle one is below it (1215-1226); each axis's
 * cone elements within sin 0.2518 of the CURRENT R_cm_update give m_j, and more than the threshold of them a mean shift and a new column a-1.
 * R_cm in the reference is a shallow cv::Mat copy of R_cm_update (1181), so axes 2 and 3 read the columns the earlier axes replaced.  Two
 * found axes: the third column is the code's cross product (negated when |det + 1| < 0.5); two or three: R = U V^T of the SVD.  Fewer than
 * two: no SVD, R is R_last with the one found column (if any) replaced.  DESIGN.md section 7 lists the readings of OpenCV's arithmetic. */
typedef struct {
    float   R[9];                 /* returned R_cm_update, row-major: the orthonormalised update when tracked, else R_last with a found column */
    float   axis_vec[3][3];       /* R_cm_Rec per axis, zeros when not found */
    float   density[3];           /* s_j_density per axis (0 when not found) */
    int32_t found[3], n_found;    /* directionFound1..3, numDirectionFound */
    int32_t n_in_cone[3], n_selected[3], min_num_sn;   /* numInCone, m_j_selected.size(), numOfSN */
    int32_t tracked;              /* 1: >= 2 axes, R is the orthonormalised update */
    int32_t status;               /* HVO_OK (written by the kernel for every frame it ran; a refused call returns its error instead) */
} hvo_mf_result;
/* On host arrays: normals = vSurfaceNormal (n_normals entries, NaN ones included: they count in size/20), l3d = hvo_lines_3d of every key
 * line (n_lines entries; the good ones, in order, are mVF3DLines), R_last row-major.  normal_axes (n_normals) / line_axes (n_lines) are
 * optional: bit a-1 is set where the element enters ProjectSN2MF's lists for axis a (vSurfaceNormal{x,y,z}, vVanishingLine{x,y,z}). */
int hvo_track_manhattan(hvo_ctx *ctx, const hvo_surface_normal *normals, int n_normals, const hvo_line3d *l3d, int n_lines,
                        const float R_last[9], hvo_mf_result *res, uint8_t *normal_axes, uint8_t *line_axes);
/* On the resident frame `cur`: its surface normals and 3-D lines stay on the device.  The stream must run HVO_STAGE_PLANE_TAIL and
 * HVO_STAGE_LINES3D and the frame must have been submitted with depth (else HVO_ERR_INVALID_ARG with hvo_stream_last_error set).  A tracker
 * threads mLastRcm through by passing the previous call's res->R as the next R_last.  line_axes has n_kl(cur) entries.  The result buffer is
 * allocated on the first call and grows on demand. */
int hvo_stream_track_manhattan(hvo_stream *s, int64_t cur, const float R_last[9], hvo_mf_result *res, uint8_t *normal_axes, uint8_t *line_axes);
/* The first n frames of the resident batch as a sequence, in one launch: frame k starts from frame k-1's R, frame 0 from R0.  Needs
 * HVO_STAGE_PLANE_TAIL and HVO_STAGE_LINES3D from the last hvo_batch_run. */
int hvo_batch_track_manhattan(hvo_ctx *ctx, int n, const float R0[9], hvo_mf_result *res);

/* ---- Map-plane association (csrc/plane_assoc.hip) ----
 * PlaneMatcher::SearchMapByCoefficients(Frame, GetAllMapPlanes()) (reference src/PlaneMatcher.cpp:10-68 with PointDistanceFromPlane :69-81 and
 * Frame::ComputePlaneWorldCoeff src/Frame.cc:2275-2280; called from src/Tracking.cc:2012 / :2407 and :2827).  For frame plane i and the map's
 * slots j in ascending order, bad slots skipped: pM = Tcw^T coef_i (sums in double, rounded to float), angle = the float
 * dot product of the two normals, left to right.  |angle| beyond aTh: dis = the smallest |pM . (x, y, z, 1)| over the slot's cloud in float
 * (100 for an empty cloud; a NaN distance never wins); dis below the running dTh makes j the match and lowers the threshold to dis.  Otherwise
 * (a gated slot whose dis is not below the running threshold included) |angle| below the running verTh makes j the vertical plane, else |angle|
 * beyond the running parTh makes j the parallel plane; each role lowers / raises its threshold to |angle|.  Every comparison is strict: the
 * first slot wins a tie.
 *
 * hvo_plane_map: the map's planes resident on one device -- per slot the world coefficients, a bad flag and the cloud (mvPlanePoints' xyz).
 * A slot's index is its position in the vector the tracker would have passed.  The map belongs to a device, not to a context: any hvo_ctx or
 * hvo_stream of that device may match against it.  Like a context it is NOT thread-safe: one call at a time on a map, the matching and update calls
 * included (they use the map's grow-only scratch).  Every call here returns after its device work has finished, so a set is visible to the
 * next match, and nothing is allocated by a call once the slot table, the point pool and the scratch have grown to the sizes in use. */
typedef struct hvo_plane_map hvo_plane_map;
#define HVO_PLANE_MAP_MAX_SLOTS (1 << 20)
/* slots / points: initial capacities (both grow on demand; 0 = a small default).  NULL when the device or the allocation fails. */
hvo_plane_map *hvo_plane_map_create(int device, int slots, int64_t points);
void hvo_plane_map_destroy(hvo_plane_map *m);
/* Set or replace slot `slot` (0 <= slot < HVO_PLANE_MAP_MAX_SLOTS): coef = GetWorldPos(), xyz = n_points x 3 floats (may be NULL when
 * n_points is 0).  A slot past the end extends the map; the slots skipped over start bad with no points.  A new slot starts good, a replaced
 * one keeps its flag.  A cloud that outgrows the slot's room moves that slot alone; the other slots' results do not change. */
int hvo_plane_map_set(hvo_plane_map *m, int slot, const float coef[4], const float *xyz, int n_points);
/* MapPlane::SetBadFlag / a slot taken back into use: bad != 0 makes the matcher skip the slot.  The slot must exist. */
int hvo_plane_map_set_bad(hvo_plane_map *m, int slot, int bad);
/* each pointer may be NULL: slots in the map, the good ones among them, the points of all slots */
int hvo_plane_map_counts(const hvo_plane_map *m, int *n_slots, int *n_good, int64_t *n_points);
/* one slot as the map holds it (each pointer may be NULL) */
int hvo_plane_map_slot(const hvo_plane_map *m, int slot, float coef[4], int *n_points, int *bad);
const char *hvo_plane_map_last_error(const hvo_plane_map *m);

typedef struct {
    int32_t n_planes;             /* mnPlaneNum: the frame planes matched (the valid ones, in order) */
    int32_t n_matches;            /* the return value: frame planes with a match */
    int32_t match[64];            /* mvpMapPlanes[i]: slot, or -1 (the reference leaves NULL) */
    int32_t vertical[64];         /* mvpVerticalPlanes[i] */
    int32_t parallel[64];         /* mvpParallelPlanes[i] */
    int32_t plane_idx[64];        /* the frame plane's index among the 64 plane_clouds records (resident forms; i itself on host arrays), -1 past n_planes */
    float   dist[64];             /* the matched slot's distance, 100 without a match */
    float   pM[64][4];            /* ComputePlaneWorldCoeff(i) */
} hvo_plane_match;
/* th = { dTh, aTh, verTh, parTh } (Plane.AssociationDisRef, AssociationAngRef, VerticalThreshold, ParallelThreshold), none NaN; NULL takes the
 * constructor's defaults { 0.1, 0.86, 0.08716, 0.9962 }.  Tcw: rows 0..2 of the pose, row-major 3 x 4, as in hvo_stream_project_last.
 * On host arrays: coef = n x 4 floats in the camera frame (mvPlaneCoefficients), n <= 64.  dist_mat / angle_mat (optional, n x slots
 * floats each, slots = the map's count): every pair's distance (100 where the gate did not pass or the slot is bad) and angle (computed for
 * bad slots too).  An empty map or n == 0 is not an error. */
int hvo_match_planes(hvo_ctx *ctx, hvo_plane_map *m, const float *coef, int n, const float Tcw[12], const float th[4], hvo_plane_match *res,
                     float *dist_mat, float *angle_mat);
/* On the resident frame `cur`: the valid hvo_plane_cloud records are read where HVO_STAGE_PLANE_TAIL left them; only Tcw and the thresholds
 * go up.  Without that stage, or for a frame submitted without depth: HVO_ERR_INVALID_ARG with hvo_stream_last_error set. */
int hvo_stream_match_planes(hvo_stream *s, hvo_plane_map *m, int64_t cur, const float Tcw[12], const float th[4], hvo_plane_match *res);
/* The first n frames of the resident batch (after hvo_batch_run with HVO_STAGE_PLANE_TAIL), frame k under Tcw + 12 k, in one launch
 * sequence: the map's clouds are read once for all n frames.  res: n entries. */
int hvo_batch_match_planes(hvo_ctx *ctx, hvo_plane_map *m, int n, const float *Tcw, const float th[4], hvo_plane_match *res);

/* ---- MapPlane::UpdateCoefficientsAndPoints on the resident plane map (csrc/plane_update.hip) ----
 * The call Tracking::Track() makes for every matched plane of every tracked frame (reference src/Tracking.cc:796-804, body
 * src/MapPlane.cc:337-368) and the no-argument overload CreateNewKeyFrame / StereoInitialization run on a new MapPlane (MapPlane.cc:300-335,
 * Tracking.cc:3208-3213, :1407), on clouds that stay on the device.
 *   MERGE   the frame's voxel cloud of plane i under inverse(toSE3Quat(Tcw)) (hvo_plane_update_transform), the slot's cloud appended,
 *           pcl::VoxelGrid(0.1) over both, the result is the slot's new cloud.  The slot's coefficients and flag stay; a bad slot is updated
 *           like a good one (Tracking.cc:800 does not look at isBad()).
 *   INSERT  the frame's voxel cloud of plane i under Twc (the caller's float GetPoseInverse(), each entry widened to double), the voxel grid,
 *           nothing appended; the slot's coefficients become ComputePlaneWorldCoeff(i) = the pM[i] of hvo_plane_match under Tcw.  The slot is
 *           set or replaced with hvo_plane_map_set's rules: a slot past the end extends the map, the skipped ones start bad and empty, a new
 *           slot starts good, a replaced one keeps its flag.
 * A transformed point is (float)(M00 x + M01 y + M02 z + M03) per row, in double, left to right.  The voxel grid is the one of
 * hvo_plane_clouds (oracle/planes_tail.c): float bounding box, inverse_leaf = 1.0f / 0.1f, min_b = floor(min * inverse_leaf), voxel
 * (int)(floorf(p * inverse_leaf) - (float)min_b) per axis, index i + j div0 + k div0 div1, one centroid per non-empty voxel in ascending
 * index order, the centroid the exact mean (2^-24 m fixed point in 64-bit integers, rounded to float once): no result depends on the order
 * of the points.  A point with a coordinate that is not finite is dropped before the bounding box.  The pcl::SACSegmentation block that
 * follows in the reference writes only locals and is not run; mWorldPos is not changed by a MERGE.
 * `plane`: frame plane i as hvo_plane_match numbers them (the i-th valid record).  Operations apply in list order: a later operation on the
 * same slot sees the earlier one's result; operations on different slots run at once.
 * A refused operation -- more than HVO_PLANE_UPDATE_MAX_POINTS frame + slot points, or a voxel index that overflows (a min_b / max_b outside
 * int32, or dx dy dz > INT32_MAX, where PCL returns the cloud unfiltered) -- gets status HVO_ERR_UNSUPPORTED and its slot stays bit for bit
 * as it was (an INSERT that would have extended the map does not); the others are done and the call returns HVO_OK.
 * A malformed list -- n outside 0..64, a plane index not below the frame's valid planes, a record whose cloud lies outside cloud_xyz, a
 * MERGE into a slot that does not exist (an INSERT earlier in the list makes it exist), an INSERT without Twc, a slot outside
 * 0..HVO_PLANE_MAP_MAX_SLOTS-1, an unknown op -- is HVO_ERR_INVALID_ARG before anything is touched, with the reason in the last-error text.
 * result: status / n_frame / n_before (the slot's points that entered: 0 for an INSERT) / n_after per operation, n_done = operations
 * with status HVO_OK.  The call returns with its device work done: the next match sees the update. */
#define HVO_PLANE_UPDATE_MERGE   0
#define HVO_PLANE_UPDATE_INSERT  1
#define HVO_PLANE_UPDATE_MAX_POINTS (1 << 20)
typedef struct { int32_t n; int32_t plane[64], slot[64], op[64]; } hvo_plane_update;
typedef struct { int32_t status[64], n_frame[64], n_before[64], n_after[64]; int32_t n_done; } hvo_plane_update_result;
/* on host arrays: records (n_records <= 64) and cloud_xyz (n_cloud x 3 floats) as hvo_plane_clouds / hvo_stream_collect_tail return them */
int hvo_update_map_planes(hvo_ctx *ctx, hvo_plane_map *m, const hvo_plane_cloud *records, int n_records, const float *cloud_xyz, int n_cloud,
                          const float Tcw[12], const float Twc[12], const hvo_plane_update *upd, hvo_plane_update_result *res);
/* on the resident frame `cur`: the clouds are read where HVO_STAGE_PLANE_TAIL left them; only the matrices and the list go up.  The stream
 * must run HVO_STAGE_PLANES | HVO_STAGE_PLANE_TAIL and the frame must have been submitted with depth, else HVO_ERR_INVALID_ARG with
 * hvo_stream_last_error set.  The frame's own results (hvo_stream_collect_tail, hvo_stream_collect) are not changed. */
int hvo_stream_update_map_planes(hvo_stream *s, hvo_plane_map *m, int64_t cur, const float Tcw[12], const float Twc[12], const hvo_plane_update *upd,
                                 hvo_plane_update_result *res);
/* the slot's cloud as the map holds it: n x 3 floats into xyz (cap points; HVO_ERR_CAPACITY with *n set when cap is too small; xyz may be
 * NULL when cap is 0) */
int hvo_plane_map_get_points(const hvo_plane_map *m, int slot, float *xyz, int cap, int *n);
/* the MERGE's matrix alone (host arithmetic in double, no device): rows 0..2 of inverse(toSE3Quat(Tcw)), row-major 3 x 4 */
int hvo_plane_update_transform(const float Tcw[12], double M[12]);

/* ---- Motion-only pose optimisation (csrc/pose_opt.hip) ----
 * Optimizer::PoseOptimization(Frame *) of the RGB-D tracker (reference src/Optimizer.cc:590-1478; called from src/Tracking.cc:2026, :2418, :2836
 * and :3859-3890): one SE3 vertex, and in the reference's insertion order the edges EdgeSE3ProjectXYZOnlyPose (mvuRight < 0) /
 * EdgeStereoSE3ProjectXYZOnlyPose per matched point, two DistPt2Line2DMultiFrameOnlyPose per matched line (start, end), DistVp2VpOnlyPose per
 * matched line whose 3-D direction and map direction have no zero component, EdgePlaneOnlyPose / EdgeParallelPlaneOnlyPose /
 * EdgeVerticalPlaneOnlyPose per frame plane and role; g2o's numeric Jacobians (central differences, 1e-9), Huber kernels, the dense 6 x 6 solve
 * and the Levenberg loop, four rounds from the initial pose with the outlier classification between them -- one kernel launch, one workgroup
 * per frame, all arithmetic in double.  Bit parity with g2o is not claimed (libm, a 1e-9 difference quotient); DESIGN.md section 7 lists the
 * readings.  Defined where the reference is not: an evaluation of DistVp2VpOnlyPose that takes its early return (a direction with z == 0)
 * contributes error 0 -- the reference keeps a stale or uninitialised _error -- and the edge is flagged in vp_outlier when a round's
 * classification reads that evaluation.  At most 8192 points, 4096 lines and 64 planes per frame (HVO_ERR_UNSUPPORTED).
 * The vanishing-direction measurement is B - A of the line's hvo_line3d record whatever its `good` flag: mvLines3D[i] holds the fitted pair
 * for every key line, and a record without a fit holds A = B = 0 (hvo_lines_3d), so Optimizer.cc:827 drops that edge here as there; a fitted
 * line shorter than 0.02 (good == 0) keeps its edge, as in the reference, which does not consult mVF3DLines.
 * A pose that is not finite in any of the n problems makes the call return HVO_ERR_INVALID_ARG before anything is launched or written. */
typedef struct { double angle_info, distance_info, parallel_info, vertical_info, chi, vp_chi; } hvo_pose_plane_params;   /* Plane.AngleInfo .. Plane.VPChi of the settings file */
typedef struct {
    float   Tcw[12];              /* pFrame->mTcw, rows 0..2, row-major 3 x 4 */
    int32_t n_points, n_lines, n_planes, reserved;   /* N, NL, mnPlaneNum: the lengths of the arrays below */
    /* frame side (host arrays; ignored by hvo_stream_pose_optimize, which reads the resident frame) */
    const hvo_keypoint *kp_un;    /* mvKeysUn: x, y, octave are read */
    const float  *uright;         /* mvuRight (NULL: every point monocular) */
    const float  *inv_sigma2;     /* mvInvLevelSigma2[octave] per point (NULL: the context's level table by octave) */
    const double *linefn;         /* mvKeyLineFunctions, n_lines x 3 */
    const hvo_line3d *lines3d;    /* mvLines3D: A = first, B = second are read */
    const float  *plane_coef;     /* mvPlaneCoefficients, n_planes x 4 */
    /* map side, indexed by feature */
    const uint8_t *pt_has;        /* mvpMapPoints[i] != NULL */
    const float  *pt_xyz;         /* GetWorldPos(), n_points x 3 */
    const uint8_t *ln_has;        /* mvpMapLines[i] != NULL */
    const double *ln_xyz;         /* mWorldPos (start, end), n_lines x 6 */
    const uint8_t *pl_has;        /* n_planes x 3: mvpMapPlanes[i], mvpParallelPlanes[i], mvpVerticalPlanes[i] != NULL */
    const float  *pl_coef_w;      /* their GetWorldPos(), n_planes x 3 x 4 */
    /* or the plane side as slots of a resident plane map, so that an hvo_plane_match passes on as it is (match, parallel, vertical of the
     * result; -1 = none; a NULL array = no plane of that role): when plane_map is set, pl_has / pl_coef_w are not read and the slots'
     * coefficients are taken from the map as it stands at the call */
    const hvo_plane_map *plane_map;
    const int32_t *slot_match, *slot_parallel, *slot_vertical;
} hvo_pose_problem;
typedef struct {                  /* each pointer may be NULL; an entry is written only where there is a correspondence, like the reference */
    uint8_t *pt_outlier;          /* mvbOutlier, n_points */
    uint8_t *ln_outlier;          /* mvbLineOutlier, n_lines */
    uint8_t *pl_outlier;          /* mvbPlaneOutlier / mvbParPlaneOutlier / mvbVerPlaneOutlier, n_planes x 3 */
    uint8_t *vp_outlier;          /* the function's local VpOutlier, n_lines (every entry written) */
} hvo_pose_flags;
typedef struct {
    double  Tcw_d[12];            /* the optimised pose in double */
    float   Tcw[12];              /* as SetPose receives it (Converter::toCvMat: float); the initial pose when ret == 0 by too few correspondences */
    int32_t ret;                  /* the return value nInitialCorrespondences - nBad - nLineBad; 0 with fewer than 3 correspondences */
    int32_t n_initial, n_bad, n_line_bad;
    int32_t n_edges;              /* optimizer.edges().size() */
    int32_t rounds;               /* rounds run (1 when the graph has fewer than 10 edges) */
    int32_t iterations[4], trials[4];   /* per round: solve() calls, Levenberg trials */
    int32_t status;               /* HVO_OK for every problem the kernel ran */
    int32_t reserved;
    double  lambda[4], chi2[4];   /* per round: the final lambda and the final active robust chi2 */
} hvo_pose_result;
/* On host arrays, n problems in one launch (one workgroup each); pp NULL = TUM3.yaml's { 0.5, 50, 0.1, 0.1, 100, 50 }.  res: n entries;
 * flags: n entries or NULL.  A problem equals the single call on it bit for bit. */
int hvo_pose_optimize(hvo_ctx *ctx, const hvo_camera *cam, const hvo_pose_plane_params *pp, int n, const hvo_pose_problem *prob,
                      hvo_pose_result *res, const hvo_pose_flags *flags);
/* On the resident frame `cur`: undistorted key points, mvuRight, octaves, key-line functions, 3-D lines and the valid plane records are read
 * where the stages left them; only the pose and the map side of `prob` go up (its frame-side pointers are ignored; n_points / n_lines are
 * capped by the frame's counts, frame plane i = the i-th valid hvo_plane_cloud record as in hvo_plane_match).  The stream must run
 * HVO_STAGE_LINES3D and HVO_STAGE_PLANE_TAIL with bf > 0 and the frame must have been submitted with depth, else HVO_ERR_INVALID_ARG with
 * hvo_stream_last_error set.  The same bytes on host arrays through hvo_pose_optimize give the same result bit for bit. */
int hvo_stream_pose_optimize(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_pose_plane_params *pp, const hvo_pose_problem *prob,
                             hvo_pose_result *res, const hvo_pose_flags *flags);

/* On the first n frames of the resident batch (after hvo_batch_run with HVO_STAGE_ORB, an LSD stage, HVO_STAGE_LINES3D and
 * HVO_STAGE_PLANE_TAIL on frames uploaded with depth), frame k under prob[k]'s pose and map side, in one launch.  A batch context carries no
 * distortion (k1 = 0: mvKeysUn = mvKeys, Frame.cc:1703-1707) and keeps no mvuRight: the kernel forms it per point from the resident depth
 * image exactly as Frame::ComputeStereoFromRGBD / hvo_stereo_from_rgbd do, with cam->bf (> 0) and the context's depth_map_factor.  Frame k
 * equals the stream form on the same image, pose and map side bit for bit.  n beyond the batch, a missing stage or no depth:
 * HVO_ERR_INVALID_ARG with hvo_last_error set. */
int hvo_batch_pose_optimize(hvo_ctx *ctx, const hvo_camera *cam, const hvo_pose_plane_params *pp, int n, const hvo_pose_problem *prob,
                            hvo_pose_result *res, const hvo_pose_flags *flags);
/* device time of the kernel launch of the last hvo_pose_optimize / hvo_batch_pose_optimize of this context, or of the last
 * hvo_stream_pose_optimize on frame `cur` of the stream (hipEvents around the launch; uploads and downloads not included), in ms */
int hvo_pose_last_kernel_ms(const hvo_ctx *ctx, float *ms);
int hvo_stream_pose_last_kernel_ms(hvo_stream *s, int64_t cur, float *ms);

/* ---- Line structural constraints and LineOptStruct (csrc/line_opt.hip) ----
 * The two per-frame steps between the Frame constructor and Track() in Tracking::GrabImageRGBD_wh (reference src/Tracking.cc:270-335):
 *   part 1  Manhattan::computeStructConstrains(frame, k, par, perp) for every key line k (src/Manhattan.cpp:107-161): per ordered pair
 *           (k, i), i != k, the 2-D cosine of (a/c, b/c) of both key-line functions and the 3-D cosine of both mvLineEq in double;
 *           perpendicular when both are < cos_perp, else parallel when both are > cos_par.  Line k is skipped by the row rule; a partner i
 *           with mvLineEq[i] == (-1,-1,-1) is not skipped (it may enter k's lists; part 2 gives it no edge).  c == 0 gives inf / NaN and
 *           neither list.  IEEE double without contraction: the result equals tests/line_opt_ref.py on every pair.
 *   part 2  Optimizer::LineOptStruct(frame) (src/Optimizer.cc:1480-1876): both 3-D end points of every line with at least
 *           min_constraints list entries are vertices; one ParEptsNVector3DSingleFrame / PerpEptsNVector3DSingleFrame edge
 *           (include/g2oMSC.h:123-190) per list entry whose partner has mvLineEq[2] != 0 and [0] != -1; g2o's numeric Jacobians (central
 *           differences, 1e-9), Huber kernels, one global Levenberg lambda over a block-diagonal Hessian (one 6 x 6 block per line), two
 *           rounds of optimize(iterations) without resetting the estimate, the classification on chi2 as float between them, and the final
 *           rejection on chi2 <= chi2_reject.  One workgroup per frame, all arithmetic in double, every sum over a fixed tree.
 * Relation matrix: int8 rel[n x n], row k: 0 none, 1 parallel, 2 perpendicular, -1 / -2 the same constraint rejected by part 2 (the
 * reference writes -1 into the list slot and keeps the slot).  Entry j of mvParLinesIdx[k] is the j-th entry of row k with |value| == 1
 * in ascending i, mvPerpLinesIdx[k] likewise with |value| == 2; a negative value is the reference's -1 in that slot.
 * Kept as written: the write-back test asks for vertex 0 in its second operand (Optimizer.cc:1861), so when line 0 did not enter the graph
 * NO line's end points are written back (the rejections still are) and when it did every line with vertices is; the function returns
 * nothing, hvo_line_opt_result is defined instead; only A and B of a record change.  Readings: DESIGN.md section 7.
 * At most 4096 lines per frame (HVO_ERR_UNSUPPORTED). */
#define HVO_LINE_STRUCT_CONSTRAINTS 1u   /* part 1: fill rel */
#define HVO_LINE_STRUCT_OPTIMIZE    2u   /* part 2 on rel: the one part 1 just filled, or, without HVO_LINE_STRUCT_CONSTRAINTS, the caller's */
#define HVO_LINE_STRUCT_ROW_UNSET   0    /* row k skipped when mvLineEq[k] == (-1,-1,-1): GrabImageRGBD_wh, src/Tracking.cc:280 */
#define HVO_LINE_STRUCT_ROW_Z0      1    /* row k skipped when mvLineEq[k][2] == 0.0: GrabImageRGBD, src/Tracking.cc:401 */
typedef struct {
    double  cos_par, cos_perp;    /* mCosThPar = cos(3 * 0.0174533), mCosThPerp = cos(87 * 0.0174533) (src/Manhattan.cpp:28-30) */
    double  huber_delta;          /* thHuberLine: sqrt(0.02) rounded to float */
    double  chi2_reject;          /* 0.02: the final rejection, in double */
    float   chi2_round[2];        /* chi2Manh = { 0.02f, 0.01f }: the classification after each round, in float */
    int32_t min_constraints;      /* 5 */
    int32_t iterations;           /* optimize(5) */
    int32_t row_rule;             /* HVO_LINE_STRUCT_ROW_* */
    uint32_t mode;                /* HVO_LINE_STRUCT_CONSTRAINTS | HVO_LINE_STRUCT_OPTIMIZE */
} hvo_line_struct_params;
/* the reference's values: both parts, the row rule of GrabImageRGBD_wh */
int hvo_line_struct_default_params(hvo_line_struct_params *p);
typedef struct {
    int32_t n_lines, reserved;    /* NL, the side of rel */
    const double *linefn;         /* mvKeyLineFunctions, n_lines x 3 (part 1 only) */
    const hvo_line3d *lines3d;    /* A, B (mvLines3D) and line_eq (mvLineEq) are read */
} hvo_line_struct_problem;
typedef struct {
    int32_t n_lines;              /* the lines the call worked on (a resident frame's count caps the caller's) */
    int32_t n_lines_to_opt;       /* lines that entered the graph */
    int32_t n_edges, n_par_edges, n_perp_edges;
    int32_t rounds;               /* 0: part 1 only; 1: the graph had fewer than 10 edges; else 2 */
    int32_t iterations[2], trials[2];   /* per round: solve() calls, Levenberg trials (0, 0 when no vertex was active) */
    int32_t n_flagged[2];         /* per round: edges whose chi2 exceeded chi2_round */
    int32_t written_back;         /* 1: the end points were written back (line 0 had vertices) */
    int32_t status;
    double  lambda[2], chi2[2];   /* per round: the final lambda and active robust chi2 */
} hvo_line_opt_result;
/* On host arrays, n_frames problems in one launch sequence; a problem equals the single call on it bit for bit.  rel[f]: n_lines^2 bytes,
 * written by part 1, or read (values 0, +-1, +-2) and rewritten by part 2 alone.  l3d_out (or l3d_out[f]) may be NULL; else n_lines x 6
 * doubles: A, B of every line after the call.  params NULL = hvo_line_struct_default_params.  The caller's records are not written. */
int hvo_line_struct_optimize(hvo_ctx *ctx, const hvo_line_struct_params *params, int n_frames, const hvo_line_struct_problem *problems,
                             int8_t *const *rel, double *const *l3d_out, hvo_line_opt_result *res);
/* On the resident frame `cur` of a stream that runs an LSD stage and HVO_STAGE_LINES3D: key-line functions and 3-D lines are read where the
 * stages left them and A, B of the resident hvo_line3d records are overwritten (when written_back), so a following hvo_stream_pose_optimize
 * or hvo_stream_search_lines_by_projection_map on that frame sees the optimised lines.  n_lines: the side of rel, the frame's key-line
 * count as hvo_stream_collect reported it.  Only rel, the result and (l3d_out != NULL) n_lines x 6 doubles come down.  A second call with
 * HVO_LINE_STRUCT_OPTIMIZE on the same frame would optimise optimised lines: HVO_ERR_INVALID_ARG, as for a missing stage or a frame
 * without depth, with hvo_stream_last_error set. */
int hvo_stream_line_struct_optimize(hvo_stream *s, int64_t cur, const hvo_line_struct_params *params, int n_lines, int8_t *rel,
                                    double *l3d_out, hvo_line_opt_result *res);
/* On the first n frames of the resident batch (after hvo_batch_run with an LSD stage and HVO_STAGE_LINES3D on frames uploaded with depth),
 * one launch sequence; n_lines[f] is the side of rel[f].  Frame k equals the stream form on the same image bit for bit.  A second
 * optimising call before the next hvo_batch_run, n beyond the batch, a missing stage or no depth: HVO_ERR_INVALID_ARG. */
int hvo_batch_line_struct_optimize(hvo_ctx *ctx, const hvo_line_struct_params *params, int n, const int32_t *n_lines, int8_t *const *rel,
                                   double *const *l3d_out, hvo_line_opt_result *res);
/* device time of the last call's two launches in ms: ms2[0] the pair pass, ms2[1] the optimisation (0 for a part that did not run) */
int hvo_line_opt_last_kernel_ms(const hvo_ctx *ctx, float ms2[2]);
int hvo_stream_line_opt_last_kernel_ms(hvo_stream *s, int64_t cur, float ms2[2]);

/* ---- The local map's lines resident on the device, SearchLocalLines and computeStructConstInMap (csrc/local_lines.hip) ----
 * The line side of Tracking::TrackLocalMapWithLines (reference src/Tracking.cc:2816-2921) in one call: Tracking::SearchLocalLines
 * (src/Tracking.cc:3279-3392) -- Frame::isInFrustum(MapLine *, 0.5) on every local map line (src/Frame.cc:1429-1499), the search core of
 * hvo_search_lines_by_projection_map on the lines in view, the CosSita > 0.09 post-gate (3357-3386) -- and
 * Manhattan::computeStructConstInMap (src/Manhattan.cpp:163-224) of every frame line against the lines in view.
 *
 * hvo_line_map: mvpLocalMapLines resident on one device.  A slot's index is the line's position in that vector.  Per slot: GetWorldPos()
 * (6 doubles: start, end), GetWorldVector(), GetNormal() (3 doubles each), mfMaxDistance / mfMinDistance (the raw members: the kernel
 * applies 1.2f and 0.8f), GetDescriptor() (32 bytes), isBad() and Observations() > 0.  Ownership and threading as for hvo_plane_map: the
 * map belongs to a device, not to a context; it is NOT thread-safe (one call at a time on a map, the searching calls included: they use the
 * map's grow-only scratch); every call returns after its device work has finished; storage grows only.
 *
 * Readings a caller can observe (DESIGN.md section 7 has all of them): Mat_<float> << double rounds each entry to float; Rcw X + tcw is the
 * reading of hvo_stream_project_last (the row's products summed in float, left to right, then the translation added through double with one
 * rounding); cv::norm is the square root of the double sum of squares stored to float; Mat::dot accumulates in double; PredictScale's log
 * is the float overload, so `level` is ceilf(logf(mfMaxDistance / dist) / log_scale_factor); K.inv() is taken in closed form in double with
 * each entry rounded to float; K.inv() x and Rcw v of the post-gate are products with double sums rounded to float once.  Both z tests are
 * `< 0.0f` as written: z == 0 passes and divides, and a NaN projection passes the bounds tests (it compares false).  The predicted level is
 * reported and never read by the search.  No arithmetic is contracted. */
typedef struct hvo_line_map hvo_line_map;
#define HVO_LINE_MAP_MAX_SLOTS (1 << 20)
/* slots: initial capacity (grows on demand; 0 = a small default).  NULL when the device or the allocation fails. */
hvo_line_map *hvo_line_map_create(int device, int slots);
void hvo_line_map_destroy(hvo_line_map *m);
/* Set or replace one slot (0 <= slot < HVO_LINE_MAP_MAX_SLOTS, else HVO_ERR_UNSUPPORTED).  A slot past the end extends the map; the slots
 * skipped over start bad.  The slot written is good (not bad) afterwards. */
int hvo_line_map_set(hvo_line_map *m, int slot, const double pos[6], const double wvec[3], const double normal[3], float max_dist, float min_dist,
                     const uint8_t desc[32], int observed);
/* Slots first .. first + n - 1 in one upload (a key frame replaces the local map): pos n x 6, wvec / normal n x 3, max_dist / min_dist n,
 * desc n x 32; observed (n bytes; NULL = every line has observations) and bad (n bytes; NULL = none is bad).  The map never shrinks: a
 * local map shorter than the one before leaves the slots past its end as they were, so the caller marks them bad (pass them in this call
 * with bad = 1, or hvo_line_map_set_bad). */
int hvo_line_map_set_many(hvo_line_map *m, int first, int n, const double *pos, const double *wvec, const double *normal, const float *max_dist,
                          const float *min_dist, const uint8_t *desc, const uint8_t *observed, const uint8_t *bad);
/* MapLine::SetBadFlag / Observations() crossing zero.  The slot must exist. */
int hvo_line_map_set_bad(hvo_line_map *m, int slot, int bad);
int hvo_line_map_set_observed(hvo_line_map *m, int slot, int observed);
/* each pointer may be NULL: slots in the map, the good ones, the ones with observations */
int hvo_line_map_counts(const hvo_line_map *m, int *n_slots, int *n_good, int *n_observed);
/* one slot as the map holds it (each pointer may be NULL) */
int hvo_line_map_slot(const hvo_line_map *m, int slot, double pos[6], double wvec[3], double normal[3], float *max_dist, float *min_dist,
                      uint8_t desc[32], int *bad, int *observed);
const char *hvo_line_map_last_error(const hvo_line_map *m);

typedef struct {
    float bounds[4];              /* mnMinX, mnMaxX, mnMinY, mnMaxY (host-array form; the resident forms take the bounds their line grid was built with) */
    float log_scale_factor;       /* mfLogScaleFactor */
    float th;                     /* SearchByProjection's th: 1, or 5 right after a relocalisation (Tracking.cc:3349-3352) */
    float nn_ratio;               /* LSDmatcher's mfNNratio */
} hvo_local_lines_params;
typedef struct {                  /* the frame side on host arrays, as for hvo_search_lines_by_projection_map */
    const hvo_keyline *kl; const double *linefn; const hvo_line3d *l3d; const uint8_t *desc; int32_t n_kl;
    const int32_t *cell_start, *cell_items;
} hvo_local_lines_frame;
typedef struct {                  /* one frame's inputs and outputs */
    int32_t n_kl;                 /* the length of held, n_par, n_perp: at least the frame's key-line count (on host arrays: frame->n_kl).  The
                                   * resident forms read the frame's own count; entries past it are not touched, a shorter array is refused. */
    int32_t *held;                /* in: the slot mvpMapLines[i] has at entry, or -1; out: after the call.  A held slot that is bad is set to -1
                                   * first (3296-3299).  t_occupied (held and the slot has observations) and the lines with mnLastFrameSeen ==
                                   * current (skipped at 3318) derive from it. */
    const int32_t *seen_extra; int32_t n_seen_extra;   /* further slots to skip: lines TrackWithMotionModel discarded as outliers (2455-2456); may be NULL / 0 */
    int32_t *in_view_slot;        /* out, room for min(slots, 16384) entries: mvpLocalMapLines_InFrustum as slots, ascending.  The caller does
                                   * IncreaseVisible() from this list and from the held lines; the library holds no such counters. */
    float *proj; float *view_cos; int32_t *level;      /* optional, per in-view entry: (u1, v1, u2, v2), mTrackViewCos, mnTrackScaleLevel */
    int32_t *match_idx, *match_dist;                   /* optional, per in-view entry: the frame line it was assigned to (-1 / 256 = none) */
    int32_t *n_par, *n_perp;      /* out, n_kl each: mvParallelLines[i]->size(), mvPerpLines[i]->size() */
    int8_t *rel_map;              /* optional, n_kl x n_in_view (room for n_kl x min(slots, 16384)), rows packed at n_in_view: 0 / 1 parallel /
                                   * 2 perpendicular against in-view entry j (the convention of hvo_line_struct_optimize's rel).  Not computed
                                   * into host memory unless given.  mvLineEq is the line_eq of the hvo_line3d records: on a resident frame
                                   * after hvo_stream_line_struct_optimize those are the optimised lines.  A (-1,-1,-1) or zero line_eq is not
                                   * skipped (the reference does not); NaN compares false both ways and gives 0. */
} hvo_local_lines_io;
typedef struct {
    int32_t n_slots_tested;       /* slots that reached isInFrustum (not bad, not seen) */
    int32_t n_in_view;            /* nToMatch */
    int32_t n_matches;            /* SearchByProjection's return value (0 when it did not run: nothing in view) */
    int32_t n_gated;              /* held lines the post-gate removed, lines held before the call included (it runs only when n_matches > 0) */
    int32_t status;
    float kernel_ms[3];           /* device time of the call: mark + frustum + compaction, the search, assignment + post-gate + constraints */
} hvo_local_lines_result;
/* On host arrays.  cam: fx, fy, cx, cy are read.  Tcw: rows 0..2 of the pose, row-major 3 x 4.  Limits: 2048 frame lines, 16384 lines in
 * view -- more gives HVO_ERR_UNSUPPORTED, never a truncated search: no output of io is written (held stays as passed in) and res
 * carries n_in_view and status.  The in-view counts come back to the host once in the middle of the call (the search's grid depends on them). */
int hvo_search_local_lines(hvo_ctx *ctx, hvo_line_map *m, const hvo_camera *cam, const float Tcw[12], const hvo_local_lines_params *params,
                           const hvo_local_lines_frame *frame, hvo_local_lines_io *io, hvo_local_lines_result *res);
/* On the resident frame `cur`: key lines, line functions, descriptors, line grid and 3-D lines are read where the stages left them; the pose,
 * held and seen_extra go up.  io->n_kl must be at least the frame's key-line count.  The stream must run an LSD stage, HVO_STAGE_GRIDS and
 * HVO_STAGE_LINES3D on a frame submitted with depth: otherwise HVO_ERR_INVALID_ARG with hvo_stream_last_error set. */
int hvo_stream_search_local_lines(hvo_stream *s, hvo_line_map *m, int64_t cur, const hvo_camera *cam, const float Tcw[12],
                                  const hvo_local_lines_params *params, hvo_local_lines_io *io, hvo_local_lines_result *res);
/* On the first n frames of the resident batch (after hvo_batch_run with an LSD stage, HVO_STAGE_GRIDS and HVO_STAGE_LINES3D on frames
 * uploaded with depth): frame k under Tcw + 12 k with io[k] / res[k]; the map is read once for all frames.  Frame k equals the stream form
 * on the same image bit for bit. */
int hvo_batch_search_local_lines(hvo_ctx *ctx, hvo_line_map *m, int n, const hvo_camera *cam, const float *Tcw, const hvo_local_lines_params *params,
                                 hvo_local_lines_io *io, hvo_local_lines_result *res);

/* ---- The local map's points resident on the device and SearchLocalPoints (csrc/local_points.hip) ----
 * The point side of Tracking::TrackLocalMapWithLines in one call: Tracking::SearchLocalPoints (reference src/Tracking.cc:3227-3277) --
 * Frame::isInFrustum(MapPoint *, 0.5) on every local map point (src/Frame.cc:1371-1427), MapPoint::PredictScale (src/MapPoint.cc:400-415)
 * and ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-132) on the points in view, through the search core of
 * hvo_search_by_projection_tracked.
 *
 * hvo_point_map: mvpLocalMapPoints resident on one device.  A slot's index is the point's position in that vector.  Per slot: GetWorldPos()
 * and GetNormal() (3 floats each: both are CV_32F), mfMaxDistance / mfMinDistance (the raw members: the kernel applies 1.2f and 0.8f),
 * GetDescriptor() (32 bytes), isBad() and Observations() > 0.  Ownership, threading and growth as for hvo_line_map: the map belongs to a
 * device, not to a context; it is NOT thread-safe (one call at a time on a map, the searching calls included: they use the map's grow-only
 * scratch); every call returns after its device work has finished; storage grows only.
 *
 * Readings a caller can observe (DESIGN.md section 7 has all of them): Rcw P + tcw and mOw as for the line map; `PcZ < 0.0f` as written
 * (z == 0 and -0.0 pass and divide; a NaN projection passes the bounds tests); invz is one float division; u = fx PcX invz + cx is float, left
 * to right; cv::norm is the square root of the double sum of squares stored to float; the dot product and its quotient by dist are double,
 * rounded to the float viewCos; PredictScale's log and ceil are the float overloads, and the clamp to [0, n_levels - 1] is part of it, so
 * `level` is clamp((int)ceilf(logf(mfMaxDistance / dist) / log_scale_factor)) (a NaN gives 0).  No arithmetic is contracted. */
typedef struct hvo_point_map hvo_point_map;
#define HVO_POINT_MAP_MAX_SLOTS (1 << 20)
/* values of hvo_local_points_io.held besides a slot (>= 0) and none (-1): a map point that is not in this map (the RGB-D tracker's temporal
 * points of UpdateLastFrame can still be held), with observations (it blocks its feature, ORBmatcher.cc:88-90) or without (it is overwritten) */
#define HVO_HELD_FOREIGN_OBSERVED (-2)
#define HVO_HELD_FOREIGN_UNOBSERVED (-3)
/* slots: initial capacity (grows on demand; 0 = a small default).  NULL when the device or the allocation fails. */
hvo_point_map *hvo_point_map_create(int device, int slots);
void hvo_point_map_destroy(hvo_point_map *m);
/* Set or replace one slot (0 <= slot < HVO_POINT_MAP_MAX_SLOTS, else HVO_ERR_UNSUPPORTED).  A slot past the end extends the map; the slots
 * skipped over start bad.  The slot written is good (not bad) afterwards. */
int hvo_point_map_set(hvo_point_map *m, int slot, const float pos[3], const float normal[3], float max_dist, float min_dist, const uint8_t desc[32],
                      int observed);
/* Slots first .. first + n - 1 in one upload (a key frame replaces the local map): pos / normal n x 3, max_dist / min_dist n, desc n x 32;
 * observed (n bytes; NULL = every point has observations) and bad (n bytes; NULL = none is bad).  The map never shrinks: a local map
 * shorter than the one before leaves the slots past its end as they were, so the caller marks them bad. */
int hvo_point_map_set_many(hvo_point_map *m, int first, int n, const float *pos, const float *normal, const float *max_dist, const float *min_dist,
                           const uint8_t *desc, const uint8_t *observed, const uint8_t *bad);
/* MapPoint::SetBadFlag / Observations() crossing zero.  The slot must exist. */
int hvo_point_map_set_bad(hvo_point_map *m, int slot, int bad);
int hvo_point_map_set_observed(hvo_point_map *m, int slot, int observed);
/* each pointer may be NULL: slots in the map, the good ones, the ones with observations */
int hvo_point_map_counts(const hvo_point_map *m, int *n_slots, int *n_good, int *n_observed);
/* one slot as the map holds it (each pointer may be NULL) */
int hvo_point_map_slot(const hvo_point_map *m, int slot, float pos[3], float normal[3], float *max_dist, float *min_dist, uint8_t desc[32], int *bad,
                       int *observed);
const char *hvo_point_map_last_error(const hvo_point_map *m);

typedef struct {
    float bounds[4];              /* mnMinX, mnMaxX, mnMinY, mnMaxY (host-array form; the resident forms take the bounds of their feature grid) */
    float log_scale_factor;       /* mfLogScaleFactor */
    int32_t n_levels;             /* mnScaleLevels, 1 .. 16: PredictScale clamps to [0, n_levels - 1]; the context's scale factors are read at the level */
    float bf;                     /* mbf: mTrackProjXR = u - bf * invz; the batch form also forms mvuRight from the depth image with it */
    float th;                     /* SearchByProjection's th: 1, 3 for RGB-D, 5 right after a relocalisation (Tracking.cc:3269-3274) */
    int32_t th_high;              /* TH_HIGH (100) */
    float nn_ratio;               /* ORBmatcher(0.8) */
    float view_cos_limit;         /* isInFrustum's viewingCosLimit (0.5) */
} hvo_local_points_params;
typedef struct {                  /* the frame side on host arrays: mvKeysUn, mvuRight (NULL: monocular, the stereo gate is off), mDescriptors */
    const hvo_keypoint *kp_un; const float *uright; const uint8_t *desc; int32_t n;
} hvo_local_points_frame;
typedef struct {                  /* one frame's inputs and outputs */
    int32_t n_kp;                 /* the length of held: at least the frame's key-point count (on host arrays: frame->n).  The resident forms read
                                   * the frame's own count; entries past it are not touched, a shorter array is refused. */
    int32_t *held;                /* in: mvpMapPoints[i] at entry as a slot, -1, HVO_HELD_FOREIGN_OBSERVED or HVO_HELD_FOREIGN_UNOBSERVED; out: after
                                   * the call.  A held slot that is bad is set to -1 first (3235-3238); every other held slot is "seen"
                                   * (mnLastFrameSeen, 3242) and is not tested.  A foreign value stays unless a match overwrites it. */
    const int32_t *seen_extra; int32_t n_seen_extra;   /* further slots to skip: points TrackWithMotionModel / TrackReferenceKeyFrame discarded
                                                        * as outliers with mnLastFrameSeen = current (2113-2114, 2434-2435); may be NULL / 0 */
    int32_t *in_view_slot;        /* out, room for min(slots, 16384) entries: the points with mbTrackInView as slots, ascending.  The caller does
                                   * IncreaseVisible() from this list and from the held points, IncreaseFound() from held after the pose
                                   * optimisation; the library holds no such counters. */
    float *proj; float *view_cos; int32_t *level;      /* optional, per in-view entry: (mTrackProjX, mTrackProjY, mTrackProjXR), mTrackViewCos, mnTrackScaleLevel */
    int32_t *match_idx, *match_dist;                   /* optional, per in-view entry: the feature it was assigned to (-1 / 256 = none) */
} hvo_local_points_io;
typedef struct {
    int32_t n_slots_tested;       /* slots that reached isInFrustum (not bad, not seen) */
    int32_t n_in_view;            /* nToMatch */
    int32_t n_matches;            /* SearchByProjection's return value (0 when it did not run: nothing in view) */
    int32_t status;
    float kernel_ms[3];           /* device time of the call: mark + frustum + compaction, the search, the assignment */
} hvo_local_points_result;
/* On host arrays.  cam: fx, fy, cx, cy are read.  Tcw: rows 0..2 of the pose, row-major 3 x 4.  Limits: 65535 frame features, 16384 points
 * in view -- more gives HVO_ERR_UNSUPPORTED, never a truncated search: no output of io is written (held stays as passed in) and res carries
 * n_in_view and status.  The in-view count comes back to the host once in the middle of the call (the search's grid depends on it). */
int hvo_search_local_points(hvo_ctx *ctx, hvo_point_map *m, const hvo_camera *cam, const float Tcw[12], const hvo_local_points_params *params,
                            const hvo_local_points_frame *frame, hvo_local_points_io *io, hvo_local_points_result *res);
/* On the resident frame `cur`: undistorted key points, mvuRight and descriptors are read where the stages left them; the pose, held and
 * seen_extra go up.  The stream must run HVO_STAGE_ORB: otherwise HVO_ERR_INVALID_ARG with hvo_stream_last_error set.  mvuRight takes part
 * when the frame was submitted with depth and the stream's bf is > 0. */
int hvo_stream_search_local_points(hvo_stream *s, hvo_point_map *m, int64_t cur, const hvo_camera *cam, const float Tcw[12],
                                   const hvo_local_points_params *params, hvo_local_points_io *io, hvo_local_points_result *res);
/* On the first n frames of the resident batch (after hvo_batch_run with HVO_STAGE_ORB): frame k under Tcw + 12 k with io[k] / res[k]; the
 * map is read once for all frames.  The batch holds no mvuRight: with depth uploaded and params->bf > 0 it is formed from the resident depth
 * image with hvo_stereo_from_rgbd's arithmetic (mvKeysUn = mvKeys, as in hvo_batch_pose_optimize).  Frame k equals the stream form on the
 * same image bit for bit. */
int hvo_batch_search_local_points(hvo_ctx *ctx, hvo_point_map *m, int n, const hvo_camera *cam, const float *Tcw, const hvo_local_points_params *params,
                                  hvo_local_points_io *io, hvo_local_points_result *res);

/* ---- The ORB vocabulary resident on the device, Frame::ComputeBoW and ORBmatcher::SearchByBoW(KeyFrame, Frame) (csrc/bow.hip) ----
 * The front of Tracking::TrackReferenceKeyFrame (reference src/Tracking.cc:1836, 1850) and Tracking::Relocalization (3763, 3796), and
 * KeyFrame::ComputeBoW (src/LocalMapping.cc:194): DBoW2's TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:
 * 1139-1271, BowVector.cpp:34-84, FORB.cpp:81-101) and ORBmatcher::SearchByBoW (src/ORBmatcher.cc:162-293).
 *
 * hvo_vocabulary: a k-ary tree of 32-byte descriptors, read-only after creation, owned by a device like hvo_plane_map / hvo_line_map (usable
 * from every context and stream of that device, from several threads at once).  The arrays of hvo_vocabulary_create are in the order of the
 * reference's text format (TemplatedVocabulary.h:1350-1436): row i is node i + 1, node 0 is the root and has no row, a parent's children
 * are in row order, the word id of a leaf is the running count of leaves.  2 <= k <= 20, 1 <= L <= 10, scoring 0..5, weighting 0..3.
 * HVO_ERR_INVALID_ARG for: a parent id that is negative or >= its child's id, a parent that is a leaf, a node that is not a leaf and has no
 * children, more than k children.  n_nodes = 0 (no words) is legal: every transform returns empty vectors (empty(), :1146) with all ids -1.
 * device < 0 makes a host-only vocabulary: it is validated and answers hvo_vocabulary_info, and every computing call refuses it.
 *
 * DEFINED BEHAVIOUR (unbalanced tree): when the descent meets a leaf above level L - levelsup, the reference leaves the node id
 * uninitialised; here node_id is that leaf's id, and hvo_bow.n_short counts such features (stopped words not included). */
typedef struct hvo_vocabulary hvo_vocabulary;
enum { HVO_VOC_TF_IDF = 0, HVO_VOC_TF = 1, HVO_VOC_IDF = 2, HVO_VOC_BINARY = 3 };                               /* DBoW2::WeightingType */
enum { HVO_VOC_L1_NORM = 0, HVO_VOC_L2_NORM = 1, HVO_VOC_CHI_SQUARE = 2, HVO_VOC_KL = 3, HVO_VOC_BHATTACHARYYA = 4, HVO_VOC_DOT_PRODUCT = 5 };   /* DBoW2::ScoringType */
typedef struct { int32_t k, L, n_nodes /* the root included */, n_words, scoring, weighting, device; } hvo_vocabulary_desc;
int hvo_vocabulary_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc,
                          const double *weight, hvo_vocabulary **voc);
/* the reference's text format (ORBvoc.txt): "k L scoring weighting", then one line per node "parent is_leaf b0 .. b31 weight".  Empty lines
 * are skipped.  The binary format is not read. */
int hvo_vocabulary_load_text(const char *path, int device, hvo_vocabulary **voc);
void hvo_vocabulary_destroy(hvo_vocabulary *voc);
int hvo_vocabulary_info(const hvo_vocabulary *voc, hvo_vocabulary_desc *info);

/* One frame's bag of words.  In: cap and the arrays (each may be NULL); out: the rest.  word_id / node_id: per feature, -1 / -1 for a
 * stopped word (weight > 0 fails); ids are the reference's.  BowVector: n_words ascending word ids with their values, bit-equal to the
 * reference's doubles (TF / TF_IDF: the weight added once per feature in feature order; IDF / BINARY: the first weight; then the norm the
 * scoring type asks for -- L1 for every type but L2_NORM and DOT_PRODUCT, summed in ascending word order -- or, for TF / TF_IDF under
 * DOT_PRODUCT, one division by the number of words).  FeatureVector as CSR: n_nodes ascending node ids, fv_start (n_nodes + 1 entries),
 * fv_index (n_valid feature indices, ascending inside a row). */
typedef struct {
    int32_t cap;                  /* room of every array in entries (fv_start: cap + 1); at least the frame's feature count */
    int32_t *word_id, *node_id;
    int32_t *bow_word; double *bow_value;
    int32_t *fv_node, *fv_start, *fv_index;
    int32_t n_features, n_words, n_nodes, n_valid /* features that are not stopped */, n_short;
    int32_t computed;             /* 1: the kernels ran; 0: the frame held this result already (same vocabulary, same levelsup) */
    int32_t status;
} hvo_bow;
/* On host descriptors: frame f has n_desc[f] descriptors of 32 bytes at desc[f]; all frames in one launch sequence.  At most 4096 features
 * per frame (HVO_ERR_UNSUPPORTED beyond). */
int hvo_compute_bow(hvo_ctx *ctx, const hvo_vocabulary *voc, int levelsup, int n_frames, const uint8_t *const *desc, const int32_t *n_desc, hvo_bow *out);
/* On the resident frame `ticket`: the descriptors where HVO_STAGE_ORB left them.  The result stays with the frame for
 * hvo_stream_search_by_bow.  A second call with the same vocabulary and levelsup launches nothing (`if (mBowVec.empty())`, src/Frame.cc:
 * 1692-1699) and returns the kept result with computed = 0; another vocabulary or levelsup recomputes. */
int hvo_stream_compute_bow(hvo_stream *s, int64_t ticket, const hvo_vocabulary *voc, int levelsup, hvo_bow *out);
/* On the first n frames of the resident batch (after hvo_batch_run with HVO_STAGE_ORB), out[k] for frame k; kept until the next
 * hvo_batch_run like the stream form.  Frame k equals the stream and the host-array forms on the same descriptors bit for bit. */
int hvo_batch_compute_bow(hvo_ctx *ctx, const hvo_vocabulary *voc, int n, int levelsup, hvo_bow *out);

/* SearchByBoW.  One side as host arrays: descriptors (n x 32), the per-feature node id hvo_*_compute_bow returned (-1: in no node), a byte
 * per feature "has a map point that is not bad" (key-frame side only), the key points' angles (mvKeysUn of the key frame, mvKeys of the
 * frame; read only with check_orientation). */
typedef struct { const uint8_t *desc; const int32_t *node_id; const uint8_t *has_map_point; const float *angle; int32_t n; } hvo_bow_keyframe;
typedef struct { float nnratio; int32_t check_orientation; int32_t th_low /* TH_LOW = 50 */; } hvo_bow_search_params;
typedef struct {
    int32_t *match_kf;            /* per frame feature: the key-frame feature whose map point it receives, or -1 (room for the frame's feature count) */
    int32_t n_matches;            /* after the rotation filter */
    int32_t status;
} hvo_bow_matches;
/* n_kf key frames against one frame in one launch, each with its own independent result (Relocalization's loop; TrackReferenceKeyFrame is
 * n_kf = 1).  Only nodes present on both sides take part; inside a node the key-frame features are visited in ascending index; best is the
 * first minimum among the node's frame features not yet claimed, second the second smallest of the multiset, both start at 256; accepted
 * when best <= th_low and (float)best < nnratio * (float)second.  At most 4096 features on a side. */
int hvo_search_by_bow(hvo_ctx *ctx, const hvo_bow_keyframe *frame, int n_kf, const hvo_bow_keyframe *kf, const hvo_bow_search_params *params, hvo_bow_matches *res);
/* The frame side is the resident frame `cur` with the bag of words hvo_stream_compute_bow left on it for `voc` (otherwise
 * HVO_ERR_INVALID_ARG): descriptors, key-point angles and FeatureVector never leave the device. */
int hvo_stream_search_by_bow(hvo_stream *s, int64_t cur, const hvo_vocabulary *voc, int n_kf, const hvo_bow_keyframe *kf, const hvo_bow_search_params *params,
                             hvo_bow_matches *res);

/* device time in ms of the last ComputeBoW (ms2[0]: descent + assembly; 0 when the kept result was returned) and the last SearchByBoW
 * (ms2[1]: the key frames' CSR + the search) of the context, or of the resident frame `cur` */
int hvo_bow_last_kernel_ms(const hvo_ctx *ctx, float ms2[2]);
int hvo_stream_bow_last_kernel_ms(hvo_stream *s, int64_t cur, float ms2[2]);

/* ---- The key-frame database resident on the device: KeyFrameDatabase and both candidate detections (csrc/kf_db.hip) ----
 * Restated: KeyFrameDatabase::add / erase / clear (src/KeyFrameDatabase.cc:40-73), DetectLoopCandidates (:76-197),
 * DetectRelocalizationCandidates (:199-309) and the vocabulary's score() (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-310).
 *
 * A key frame is a SLOT (0 <= slot < HVO_KFDB_MAX_SLOTS) the caller numbers: it holds the key frame's bag of words (ascending word ids,
 * double values, at most 4096 words), the order number of its add, up to 10 neighbour slots (the key frame's
 * GetBestCovisibilityKeyFrames(10), in that order; the host owns the covisibility graph and sets them) and the two scores the last
 * queries left on it (mRelocScore, mLoopScore), which persist from query to query as they do on a KeyFrame.  DEFINED BEHAVIOUR: a slot
 * that has never been scored holds 0.0f where the reference reads an uninitialised float; add resets both.
 *
 * The database belongs to the vocabulary's device like hvo_plane_map (a host-only vocabulary is refused), has its own HIP stream and is
 * not thread-safe: guard it by the mutex that guards the reference's database.  Every call returns with its device work done.  Every
 * refusal is whole -- nothing of the database changes -- and leaves its reason in hvo_keyframe_db_last_error:
 *   slot outside [0, 16384); add on a live slot (erase first); more than 4096 words (HVO_ERR_UNSUPPORTED); word ids that are not strictly
 *   ascending or not below the vocabulary's word count; a value that is negative or not finite (no DBoW2 weighting produces one, and it
 *   keeps NaN out of the scores); set_covisible / get on a slot that is not live; more than 10 neighbours; a query on a vocabulary with KL
 *   scoring (HVO_ERR_UNSUPPORTED: it needs log); result.cap below the candidate count (HVO_ERR_CAPACITY with n_candidates = the count
 *   needed and the kept scores left as they were); slot_cap below the slot count when a view is asked for.
 * erase of a slot that is not live does nothing.  A neighbour id or a connected id that is out of range or erased is skipped. */
#define HVO_KFDB_MAX_SLOTS 16384
#define HVO_KFDB_MAX_COVISIBLE 10
enum { HVO_KFDB_RELOC = 0, HVO_KFDB_LOOP = 1 };
typedef struct hvo_keyframe_db hvo_keyframe_db;
typedef struct {
    int32_t n_slots;              /* highest slot ever added + 1 (0 after clear): the length of the per-slot views */
    int32_t n_live;
    int32_t scoring, device;
    int64_t pooled_words;         /* words of pool in use (rooms are multiples of 64; an erased slot keeps its room) */
    int64_t pool_capacity;
    int64_t next_sequence;        /* the order number the next add gets */
} hvo_keyframe_db_desc;
int hvo_keyframe_db_create(const hvo_vocabulary *voc, hvo_keyframe_db **db);
void hvo_keyframe_db_destroy(hvo_keyframe_db *db);
const char *hvo_keyframe_db_last_error(const hvo_keyframe_db *db);
int hvo_keyframe_db_add(hvo_keyframe_db *db, int slot, int n_words, const int32_t *word, const double *value);
/* add with the bag hvo_stream_compute_bow left on the resident frame `ticket` for `voc`: device to device, only the word count comes down */
int hvo_stream_keyframe_db_add(hvo_stream *s, int64_t ticket, const hvo_vocabulary *voc, hvo_keyframe_db *db, int slot);
int hvo_keyframe_db_erase(hvo_keyframe_db *db, int slot);
int hvo_keyframe_db_clear(hvo_keyframe_db *db);
int hvo_keyframe_db_set_covisible(hvo_keyframe_db *db, int slot, int n, const int32_t *slots);
/* read-back (tests, a viewer): a live slot's bag (cap entries; HVO_ERR_CAPACITY with *n_words set when too small; word / value may be
 * NULL) and score2 = { kept reloc score, kept loop score } as the device holds them */
int hvo_keyframe_db_get(const hvo_keyframe_db *db, int slot, int cap, int32_t *word, double *value, int32_t *n_words, float score2[2]);
int hvo_keyframe_db_info(const hvo_keyframe_db *db, hvo_keyframe_db_desc *info);

typedef struct {
    int32_t mode;                 /* HVO_KFDB_RELOC: DetectRelocalizationCandidates; HVO_KFDB_LOOP: DetectLoopCandidates */
    float min_score;              /* loop form: minScore */
    const int32_t *connected;     /* loop form: the slots of pKF->GetConnectedKeyFrames(); they are never "in the query" */
    int32_t n_connected;
} hvo_kfdb_params;
typedef struct {
    int32_t cap; int32_t *candidate; int32_t n_candidates;      /* the returned vector: slots (pBestKF), in the reference's order */
    /* optional views (NULL: not wanted) of slot_cap >= n_slots entries, entry = slot: the common words (0: not in the query), the score
     * THIS query wrote (NaN: none), accScore (NaN: the slot did not enter lScoreAndMatch) and pBestKF (-1 likewise) */
    int32_t slot_cap; int32_t *words; float *score; float *acc; int32_t *best;
    int32_t n_sharing, max_common, min_common, n_scored;        /* lKFsSharingWords.size(), maxCommonWords, minCommonWords, nscores */
    float best_acc_score;         /* bestAccScore (its start value, 0 or min_score, when nothing entered) */
    int32_t status;
} hvo_kfdb_result;
/* An empty database, a query without words and a query that shares no word with any slot are HVO_OK with n_candidates = 0.  Candidates
 * are ordered as the reference's list walk orders them: by (smallest word in common with the query, order of add).  The host form takes
 * the bag as hvo_bow returns it; the stream form reads the bag hvo_stream_compute_bow left on the frame `ticket` for `voc` and the batch
 * form the bags hvo_batch_compute_bow left on frames 0 .. n-1, queried one after the other in that order (the kept scores make the order
 * matter): frame k's answer is bit for bit that of the k-th of n stream calls.  A frame without a bag of words for `voc` (or a database
 * created for another vocabulary) is HVO_ERR_INVALID_ARG.  Each query synchronises once, at its end. */
int hvo_keyframe_db_query(hvo_keyframe_db *db, int n_words, const int32_t *word, const double *value, const hvo_kfdb_params *p, hvo_kfdb_result *res);
int hvo_stream_keyframe_db_query(hvo_stream *s, int64_t ticket, const hvo_vocabulary *voc, hvo_keyframe_db *db, const hvo_kfdb_params *p, hvo_kfdb_result *res);
int hvo_batch_keyframe_db_query(hvo_ctx *ctx, const hvo_vocabulary *voc, hvo_keyframe_db *db, int n, const hvo_kfdb_params *p, hvo_kfdb_result *res);
/* device time in ms of the last query's four kernels (0 when it launched nothing) */
int hvo_keyframe_db_last_kernel_ms(const hvo_keyframe_db *db, float *ms);

/* ---- The relocalisation PnP solver: PnPsolver's EPnP RANSAC for all candidates of a relocalisation in one call (csrc/pnp.hip) ----
 * Restated: the PnPsolver constructor (src/PnPsolver.cc:67-110), SetRansacParameters (:121-157), iterate (:165-258), Refine (:260-305),
 * CheckInliers (:308-339) and EPnP (:342-950), as Tracking::Relocalization drives them (src/Tracking.cc:3789-3909).  There is no batch
 * form: a relocalisation is ONE frame against many key frames, and the many are the launch's width.
 *
 * iterate() is sequential only through mnIterations, mnBestInliers and mvbBestInliers, and Refine() depends on nothing but the current
 * best set.  So one call evaluates all T hypotheses of every candidate and returns what a host replay of the loop needs (hvo::PnPsolver
 * in hvo.hpp, hvo_amd.pnp_iterate in Python).  With it = 1..T: hypothesis it has a count hyp_inliers[it-1]; it PASSES when that count is
 * >= min_inliers; a passing iteration is a RECORD when its count exceeds the running best (only passing iterations update the best);
 * Refine runs EPnP on the record's inliers in ascending correspondence index and then CheckInliers, and succeeds when the refined count
 * is STRICTLY greater than min_inliers (:292, against >= at :209); a passing iteration that is no record repeats the last record's Refine
 * with the same outcome.  Every record is an event, in order; hyp_event[it-1] is the event iterate() returns in iteration it, or -1.
 * T = the effective maxIts + extra_iterations (the loop's `mnIterations < maxIts || nCurrentIterations < nIterations` may overrun the cap
 * by a chunk; a replay that needs hypothesis T + 1 reports bNoMore).  N < min_inliers: T = 0 and no_more is set (:173-177).
 * Limits: T <= 1024, N <= 4096, 4 <= min_set <= 64, n_kf <= 256, max_events <= 64, and 1 GiB of device scratch per call
 * (HVO_ERR_UNSUPPORTED beyond; min_set < 4 is HVO_ERR_INVALID_ARG).  More records than max_events: that candidate's status and the
 * call's return value are HVO_ERR_CAPACITY, its first max_events events are complete, nothing past them is written, and hyp_event is -1
 * where it would name a record that was not kept.
 *
 * Determinism and readings.  Random draws: the reference draws from the process-global rand(), shared by all solvers; here `seed` is a
 * parameter, hypothesis (candidate j, iteration it) has its own xorshift32 stream seeded seed ^ (0x9E3779B9 * (1024 j + it)) (0 ->
 * 0x6D2B79F5), a draw from a set of size s is x % s, removal is the reference's swap-with-last (:199-200).  Linear algebra (OpenCV is not
 * in the tree): cvSVD of the symmetric 3 x 3 and 12 x 12 matrices is a cyclic two-sided Jacobi eigen-iteration, pairs in row-major order,
 * exactly 12 sweeps, an exactly zero off-diagonal element giving the identity rotation, eigenpairs in descending eigenvalue with ties by
 * index; cvSVD of ABt, cvInvert(CV_SVD) and the three cvSolve(CV_SVD) are one-sided (Hestenes) Jacobi, 12 sweeps, singular values at
 * or below 2 DBL_EPSILON (sum of singular values) cut, so coplanar points take the pseudo-inverse; sums over correspondences
 * (cvMulTransposed and the loops) are plain ascending sums for up to 64 rows and one fixed tree above (256 strided partials, each run
 * of 64 halved, the four runs in order).  Only + - * / sqrt, in a fixed order, without contraction.  NOT claimed: with min_set = 4 the
 * null space of MtM has dimension >= 4 and the four vectors EPnP takes are a basis of it fixed by the Jacobi order, OpenCV's another, so
 * hypothesis-level parity with the reference binary cannot be claimed; claimed are bit equality with the restatement tests/pnp_ref.py
 * and recovery of planted poses.  Kept as written: CheckInliers' mix of float and double, a[0] = 1.0f - ..., the 2.0f factors, qr_solve's
 * pivot scan over rows k..nr-2, > in Refine against >= in iterate, N == min_inliers -> one iteration, the host libm log / pow / ceil of
 * SetRansacParameters.  Defined: qr_solve's early return on a zero column is a zero step; a hypothesis with a non-finite pose counts 0. */
typedef struct {
    double probability; int32_t min_inliers, max_iterations, min_set; float epsilon, th2;      /* SetRansacParameters' arguments */
    uint32_t seed; int32_t extra_iterations /* 8 */, max_events /* 8 */;
} hvo_pnp_params;
void hvo_pnp_default_params(hvo_pnp_params *p);               /* (0.99, 10, 300, 4, 0.5, 5.991), src/Tracking.cc:3805; seed 1 */
/* One candidate's correspondences, already compacted as the constructor does: mvP3Dw (n x 3), mvP2D (n x 2), mvSigma2 (n), mvKeyPointIndices
 * (n, each in [0, n_features)); n_features = F.N, the length of vbInliers. */
typedef struct { const float *p3d, *p2d, *sigma2; const int32_t *feature_index; int32_t n, n_features; } hvo_pnp_problem;
/* A record: its iteration (1-based), Refine's count, whether Refine succeeded, mRefinedTcw's upper 3 x 4 after convertTo(CV_32F)
 * (row-major) and Refine's vbInliers (n_features bytes, caller-owned); and the record's own hypothesis -- mnBestInliers, mBestTcw and
 * mvbBestInliers (by frame feature) for as long as it is the best, which is what iterate() returns with bNoMore when the loop ends
 * between this record and the next (:241-255). */
typedef struct { int32_t iteration, n_inliers, success, hyp_n_inliers; float Tcw[12], hyp_Tcw[12]; uint8_t *inliers, *hyp_inliers; } hvo_pnp_event;
typedef struct {
    int32_t cap_hyp, cap_events;                                /* in: room of the hyp_* arrays (>= T) and of events (>= max_events) */
    int32_t *hyp_inliers, *hyp_event;                           /* caller-owned, cap_hyp entries */
    int32_t *hyp_sample;                                        /* optional (may be null), cap_hyp x min_set: the drawn correspondence indices */
    hvo_pnp_event *events;
    uint8_t *best_inliers;                                      /* n_features bytes: mvbBestInliers through mvKeyPointIndices (:247-252), after all T */
    float best_Tcw[12];                                         /* mBestTcw after all T hypotheses (= the last record's hyp_Tcw) */
    int32_t best_n_inliers, best_valid /* best >= min_inliers */, best_iteration;
    int32_t n, n_features, min_inliers, max_its; float epsilon; /* the effective N, F.N, mRansacMinInliers, mRansacMaxIts, mRansacEpsilon */
    int32_t n_hyp /* T */, n_events, no_more, status;
} hvo_pnp_result;
/* n_kf candidates on host arrays, in one launch sequence */
int hvo_pnp_ransac(hvo_ctx *ctx, const hvo_camera *cam, const hvo_pnp_params *params, int n_kf, const hvo_pnp_problem *problems, hvo_pnp_result *results);
/* The frame side is the resident frame `cur`: mvKeysUn positions and octaves are read where the stages left them, mvSigma2 is the float
 * scale[octave]^2 the pose optimisation forms.  Per candidate only the map side goes up: match_kf as hvo_stream_search_by_bow returned it
 * (one entry per frame feature, -1: none), the key frame's per-feature world positions (n x 3) and a bad-point byte per key-frame feature.
 * The constructor's compaction runs on the device in ascending frame-feature index.  The result is the host-array form's on the same data. */
typedef struct { const int32_t *match_kf; const float *pos; const uint8_t *bad; int32_t n; } hvo_pnp_keyframe_side;
int hvo_stream_pnp_ransac(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_pnp_params *params, int n_kf, const hvo_pnp_keyframe_side *kf_sides,
                          hvo_pnp_result *results);
/* device time in ms of the last call's hypothesis kernels (ms2[0]: hypotheses + scan) and refine kernels (ms2[1]: refine + events) */
int hvo_pnp_last_kernel_ms(const hvo_ctx *ctx, float ms2[2]);
int hvo_stream_pnp_last_kernel_ms(hvo_stream *s, int64_t cur, float ms2[2]);

/* ---- ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1499-1628; csrc/kf_search.hip) ----
 * The refinement Tracking::Relocalization runs between its pose optimisations (Tracking.cc:3871 with (10, 100), :3885 with (3, 64)): every
 * map point of a candidate key frame that is not bad and not already found is projected under the frame's pose, gated by the image bounds
 * and its distance range, given a predicted level, and searched in the frame's grid within [level - 1, level + 1].  n_kf candidates go in
 * one call, each with its own pose and its own occupancy.  Unlike the other guided searches there is NO depth-sign test (a point behind
 * the camera whose projection lands inside the bounds is searched; z == 0 gives inf or NaN, and a NaN passes the bounds tests and finds
 * nothing), EVERY non-NULL feature blocks (occupied at entry, or taken by an earlier entry of the same candidate), and a match is accepted
 * when bestDist <= orb_dist (no ratio test, no mvuRight gate).  Entries are walked in order; a later entry takes its next best free feature. */
typedef struct {
    int32_t n;                 /* pKF->GetMapPointMatches().size() */
    const float   *pos;        /* n x 3, GetWorldPos() (CV_32F); not read where skip[i] */
    const uint8_t *skip;       /* n: !pMP || pMP->isBad() || sAlreadyFound.count(pMP) */
    const float   *max_dist, *min_dist;   /* RAW mfMaxDistance / mfMinDistance; the 1.2f / 0.8f factors are applied by the call, as in hvo_point_map */
    const uint8_t *desc;       /* n x 32, pMP->GetDescriptor() */
    const float   *angle;      /* n, pKF->mvKeysUn[i].angle; may be NULL when check_orientation == 0 */
    float Tcw[12];             /* CurrentFrame.mTcw rows 0..2 for THIS candidate */
    const uint8_t *occupied;   /* frame's N: CurrentFrame.mvpMapPoints[i2] != NULL at entry (NULL: none) */
} hvo_kf_search_candidate;
typedef struct {
    float th; int32_t orb_dist; int32_t check_orientation; float log_scale_factor; int32_t n_levels;
    float bounds[4];           /* mnMinX, mnMaxX, mnMinY, mnMaxY (host-array form; the stream form takes the bounds of its feature grid) */
} hvo_kf_search_params;
/* gate codes, in the reference's order */
#define HVO_KF_GATE_SEARCHED 0
#define HVO_KF_GATE_SKIP     1      /* skip[i] */
#define HVO_KF_GATE_U_MIN    2      /* u < mnMinX */
#define HVO_KF_GATE_U_MAX    3      /* u > mnMaxX */
#define HVO_KF_GATE_V_MIN    4      /* v < mnMinY */
#define HVO_KF_GATE_V_MAX    5      /* v > mnMaxY */
#define HVO_KF_GATE_DIST_MIN 6      /* dist3D < 0.8f * mfMinDistance */
#define HVO_KF_GATE_DIST_MAX 7      /* dist3D > 1.2f * mfMaxDistance */
typedef struct {               /* per candidate; every pointer but match_idx may be NULL */
    int32_t *match_idx, *match_dist;   /* n: the frame feature entry i was assigned to, after the rotation cull (-1 / 256 = none) */
    int32_t *feature_kf;               /* frame's N: the key-frame entry now holding feature i2, -1 = none (the inverse; occupied features stay -1) */
    float *proj; int32_t *level; int8_t *gate;   /* n x 2 (u, v), n, n: what the prologue decided.  proj is (0, 0) for a skipped entry;
                                                  * level is -1 for every entry that was not searched */
    int32_t n_matches, n_searched, status; float kernel_ms[2];   /* return value; entries with gate 0; prologue and search device time (of the whole call) */
} hvo_kf_search_result;
/* On host arrays.  cam: fx, fy, cx, cy are read; frame: kp_un, desc, n (uright is not read); the scale factors are the context's.
 * Limits: 16384 entries per candidate, 65535 frame features (HVO_ERR_UNSUPPORTED beyond); n_levels outside 1 .. 16, empty bounds, a
 * missing array or orb_dist > 255 (the reference would then write mvpMapPoints[-1]) are HVO_ERR_INVALID_ARG.  Every refusal is whole:
 * nothing is written and hvo_last_error says why.  A candidate with n == 0 and a frame without features are HVO_OK with no match.
 * All candidates are enqueued before the call's single synchronisation. */
int hvo_search_by_projection_keyframe(hvo_ctx *ctx, const hvo_camera *cam, const hvo_kf_search_params *params, const hvo_local_points_frame *frame,
                                      int n_kf, const hvo_kf_search_candidate *candidates, hvo_kf_search_result *results);
/* On the resident frame `cur`: undistorted key points and descriptors are read where the stages left them, the bounds are the frame grid's
 * (params->bounds is ignored); only the candidates go up.  The stream must run HVO_STAGE_ORB: otherwise HVO_ERR_INVALID_ARG with
 * hvo_stream_last_error set.  The result is the host-array form's on the downloaded frame, bit for bit. */
int hvo_stream_search_by_projection_keyframe(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_kf_search_params *params,
                                             int n_kf, const hvo_kf_search_candidate *candidates, hvo_kf_search_result *results);

/* ---- ORBmatcher::Fuse(KeyFrame *, const vector<MapPoint *> &, float th) (src/ORBmatcher.cc:838-994; csrc/fuse.hip) ----
 * The matcher of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1567-1696): every map point of a list that is not bad and not already
 * in the key frame is projected into the key frame, gated (depth sign, image, distance range, viewing angle), given a predicted level and
 * compared with the key frame's features in a window of th * mvScaleFactors[level] within the levels [level - 1, level] under a chi-square
 * test on the reprojection error (7.8 with mvuRight, 5.99 without, scaled by mvInvLevelSigma2).  Fuse has NO occupancy: an entry's best
 * feature does not depend on what other entries took, so all (key frame, entry) pairs of n_kf key frames are searched in one launch.
 * The pointer part stays with the caller, who walks fused_entry / fused_idx in order and re-tests `isBad() || IsInKeyFrame(pKF)` per entry
 * (it only ever turns from "not skipped" to "skipped" during the walk): Replace against AddObservation + AddMapPoint.
 *
 * Readings a caller can observe (DESIGN.md section 7 has all of them): Rcw P + tcw and mOw as for the point map; `z < 0.0f` as written
 * (z == 0 and -0.0 pass and divide); invz = 1 / z is ONE FLOAT division (the text has the int literal 1); u = fx * (X * invz) + cx, two
 * float products; IsInImage is u >= minX && u < maxX && v >= minY && v < maxY, so a NaN projection FAILS; ur = u - bf * invz; cv::norm is
 * the square root of the double sum of squares stored to float; PO.dot(Pn) accumulates in double and is compared with the double
 * 0.5 * dist3D; PredictScale as in the key-frame search; the radius is a float product; GetFeaturesInArea's cell range is applied as
 * written IN ADDITION to the two fabs tests; e2 is float, left to right, e2 * mvInvLevelSigma2[octave] a float product compared with the
 * double literals 7.8 / 5.99 (mvuRight >= 0 chooses; a NaN there takes the mono gate).  A feature whose octave is negative is in no band.
 * The strict `dist < bestDist` keeps the first of equal distances in GetFeaturesInArea's visiting order: cell column, then cell row, then
 * feature index.  No arithmetic is contracted. */
typedef struct {               /* the key-frame side on host arrays */
    int32_t n;                 /* pKF->N */
    const hvo_keypoint *kp_un; /* mvKeysUn: x, y, octave are read */
    const float   *uright;     /* mvuRight; NULL: every feature takes the mono gate */
    const uint8_t *desc;       /* n x 32, mDescriptors */
    float Tcw[12];             /* rows 0..2 of the key frame's pose, row-major 3 x 4 */
    const uint8_t *skip;       /* one byte per map entry FOR THIS key frame: !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF); NULL: none */
} hvo_fuse_keyframe;
typedef struct {               /* a map side on host arrays: vpMapPoints */
    int32_t n;
    const float   *pos, *normal;          /* n x 3 each: GetWorldPos(), GetNormal() (CV_32F) */
    const float   *max_dist, *min_dist;   /* RAW mfMaxDistance / mfMinDistance; the call applies 1.2f / 0.8f, as in hvo_point_map */
    const uint8_t *desc;                  /* n x 32, GetDescriptor() */
} hvo_fuse_map;
/* n = 0 is served on either side, alone or inside a longer list, and its arrays may then be NULL: a key frame without features searches its
 * entries and finds nothing (best_idx -1, n_fused 0), a map side without entries gives n_searched = n_fused = 0 and writes no array. */
typedef struct {
    float th;                  /* 3 */
    int32_t th_low;            /* TH_LOW (50); above 255 is refused (bestDist starts at 256: the reference would accept bestIdx = -1) */
    float log_scale_factor;    /* pKF->mfLogScaleFactor */
    int32_t n_levels;          /* pKF->mnScaleLevels, 1 .. 16; mvScaleFactors and mvInvLevelSigma2 are the context's */
    float bf;                  /* pKF->mbf */
    float bounds[4];           /* mnMinX, mnMaxX, mnMinY, mnMaxY (host-array form; the stream form takes the bounds of its feature grid) */
    int32_t map_per_keyframe;  /* hvo_fuse_points: 0 = map_side[0] is shared by all key frames (uploaded once: the first loop of
                                * SearchInNeighbors); 1 = key frame j is searched with map_side[j] */
} hvo_fuse_params;
/* gate codes, in the reference's order */
#define HVO_FUSE_GATE_SEARCHED     0   /* also an entry whose area holds no feature: best_idx stays -1 */
#define HVO_FUSE_GATE_SKIP         1   /* skip[i], or a bad slot */
#define HVO_FUSE_GATE_BEHIND       2   /* z < 0.0f */
#define HVO_FUSE_GATE_OUT_OF_IMAGE 3   /* !IsInImage(u, v) */
#define HVO_FUSE_GATE_DIST_MIN     4   /* dist3D < 0.8f * mfMinDistance */
#define HVO_FUSE_GATE_DIST_MAX     5   /* dist3D > 1.2f * mfMaxDistance */
#define HVO_FUSE_GATE_VIEW_ANGLE   6   /* PO.dot(Pn) < 0.5 * dist3D */
typedef struct {               /* per key frame; every pointer but best_idx may be NULL.  n = the entries of this key frame's map side */
    int32_t *best_idx, *best_dist;   /* n: bestIdx / bestDist after the loop (-1 / 256 where no candidate survived or the entry was not searched) */
    int8_t  *gate;                   /* n */
    int32_t *level;                  /* n: nPredictedLevel; -1 where the entry was not searched */
    float   *proj;                   /* n x 3: u, v, ur as far as the reference computed them (skip, behind: 0, 0, 0; out of image: u, v, 0) */
    int32_t *fused_entry, *fused_idx;   /* room for n each: the entries with best_dist <= th_low in ascending order and their features:
                                         * the list the caller walks */
    int32_t n_fused, n_searched, status; float kernel_ms[3];   /* entries in the list; entries with gate 0; device time of the whole call's
                                                                * grid, projection and search (with the compaction) kernels */
} hvo_fuse_result;
/* On host arrays: n_kf key frames against map_side[0] (shared) or map_side[j].  cam: fx, fy, cx, cy are read.  Limits: 65535 features per
 * key frame (the search key holds the candidate's rank in 16 bits), 1048576 entries per key frame (HVO_ERR_UNSUPPORTED beyond); th_low > 255,
 * n_levels outside 1 .. 16, empty bounds or a missing array are HVO_ERR_INVALID_ARG.  Every refusal is whole: nothing is written and
 * hvo_last_error says why.  n == 0 on either side is HVO_OK with no match.  One synchronisation per call. */
int hvo_fuse_points(hvo_ctx *ctx, const hvo_camera *cam, const hvo_fuse_params *params, const hvo_fuse_map *map_side,
                    int n_kf, const hvo_fuse_keyframe *keyframes, hvo_fuse_result *results);
/* The map side as n slots of a resident point map, shared by all key frames: the map's device arrays are read in place, only the slot list
 * and the skip bytes go up.  A bad slot counts as skipped; a slot outside the map is HVO_ERR_INVALID_ARG (whole).  The map must live on the
 * context's device.  The refusal's text is in hvo_last_error and in hvo_point_map_last_error. */
int hvo_fuse_points_slots(hvo_ctx *ctx, hvo_point_map *m, int n, const int32_t *slots, const hvo_camera *cam, const hvo_fuse_params *params,
                          int n_kf, const hvo_fuse_keyframe *keyframes, hvo_fuse_result *results);
/* The resident frame `cur` is the one key frame, under Tcw: Fuse(mpCurrentKeyFrame, vpFuseCandidates), valid while the frame is in the
 * ring.  Its undistorted key points, mvuRight (when it was submitted with depth and the stream's bf is > 0) and descriptors are read where
 * the stages left them; the bounds are its grid's (params->bounds is ignored).  The map side is map_side (host arrays) or, when map_side is
 * NULL, n slots of m.  skip: one byte per entry or NULL.  The stream must run HVO_STAGE_ORB: otherwise HVO_ERR_INVALID_ARG with
 * hvo_stream_last_error set.  The result is the host-array form's on the downloaded frame, bit for bit. */
int hvo_stream_fuse_points(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_fuse_params *params, const float Tcw[12], const uint8_t *skip,
                           const hvo_fuse_map *map_side, hvo_point_map *m, int n, const int32_t *slots, hvo_fuse_result *result);

/* ---- LSDmatcher::Fuse(KeyFrame *, const vector<MapLine *> &, float th) (src/LSDmatcher.cpp:1297-1434; csrc/line_fuse.inc) ----
 * The line matcher of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:1651, :1677): every map line of a list that is not skipped is
 * projected into the key frame by both end points, gated (depth sign of both ends, image bounds of both ends, distance range, viewing
 * angle), given a predicted level and compared with the key lines KeyFrame::GetLinesInArea (src/KeyFrame.cc:668-702) returns: it uses no
 * grid and tests EVERY key line of the key frame (squared mid-point distance <= r * r, |cos| of the two directions >= 0.998f), so the work
 * is key frames x entries x lines.  Among those in the levels [level - 1, level] the lowest Hamming distance wins, the lowest line index
 * among equals; it is accepted at best_dist <= th_low.  There is no occupancy, so all (key frame, entry) pairs are searched in one launch.
 * The pointer part stays with the caller (hvo::LSDmatcher::walkFused in hvo.hpp): Replace against AddObservation + AddMapLine.
 *
 * Three readings are decided here (tests/line_fuse_ref.py):
 *  1. Which descriptors.  The text compares the map line's LBD descriptor with pKF->mDescriptors.row(idx): ORB rows under a line index
 *     (mLineDescriptors is fetched and never used).  desc_rows / n_desc_rows are "the rows the candidates are compared with":
 *     mLineDescriptors (the intended reading) or mDescriptors (as written).  A candidate idx >= n_desc_rows is not compared.  No flag.
 *  2. The predicted level.  MapLine::PredictScale does not clamp and indexes mvScaleFactorsLine.  HVO_LF_LEVEL_CLAMPED (the default) clamps to
 *     [0, n_levels - 1] before the radius and the band; HVO_LF_LEVEL_AS_WRITTEN keeps the level, and an entry whose level is outside
 *     [0, n_levels) gets HVO_LF_GATE_LEVEL and is not searched.  log_scale_factor is the key frame's mfLogScaleFactorLine (the reference
 *     sets it to the log of the ORB factor); the table is sf[0] = 1, sf[l] = sf[l - 1] * scale_factor in float (the line extractor's).
 *  3. `return false` on a negative depth (:1340-1341) stops the reference's call at the first entry that lies behind and is still not
 *     skipped when the walk reaches it.  The device applies no stop: every entry is evaluated, such an entry reports HVO_LF_GATE_BEHIND,
 *     and behind_entry / n_behind list them in ascending order, for the walk to apply the stop or not.
 * Arithmetic a caller can observe: Mat_<float> << double rounds to float; Rcw P + tcw as for the line map; invz = 1.0f / z is one float
 * division and u = fx * X * invz + cx goes left to right; IsInImage(u1, v1) is tested before u2, v2 exist and a NaN fails it;
 * 0.5 * (SP + EP) is the float of SP * 0.5 + EP * 0.5 formed in double; cv::norm and Mat::dot as in hvo_fuse_points; the angle gate
 * compares with the double 0.5 * dist; inside GetLinesInArea the mid-point distance is formed in double and rounded to float, compared
 * with the float r * r by `>`; both directions are normalised in float; `CosSita < 0.998f` lets a NaN (a line of zero length on either
 * side) PASS.  An octave of -1 lies in the band at level 0.  No arithmetic is contracted. */
typedef struct {               /* the key-frame side on host arrays */
    int32_t n;                 /* mvKeyLines.size() */
    const hvo_keyline *kl;     /* pt_x, pt_y, sx, sy, ex, ey, octave are read */
    const uint8_t *desc_rows;  /* n_desc_rows x 32: the rows the candidates are compared with (reading 1) */
    int32_t n_desc_rows;
    float Tcw[12];             /* rows 0..2 of the key frame's pose, row-major 3 x 4 */
    float bounds[4];           /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float fx, fy, cx, cy;      /* the key frame's own */
    const uint8_t *skip;       /* one byte per map entry FOR THIS key frame: !pML || pML->isBad() || pML->IsInKeyFrame(pKF); NULL: none */
} hvo_lf_keyframe;
typedef struct {               /* a map side on host arrays: vpMapLines */
    int32_t n;
    const double  *pos;                         /* n x 6: GetWorldPos(), start then end */
    const double  *normal;                      /* n x 3: GetNormal() */
    const float   *max_distance, *min_distance; /* RAW mfMaxDistance / mfMinDistance; the call applies 1.2f / 0.8f, as in hvo_line_map */
    const uint8_t *desc;                        /* n x 32, mLDescriptor */
} hvo_lf_map;
#define HVO_LF_LEVEL_CLAMPED    0
#define HVO_LF_LEVEL_AS_WRITTEN 1
typedef struct {
    float th;                  /* 3 */
    int32_t th_low;            /* TH_LOW (50); above 255 is refused */
    float log_scale_factor;    /* pKF->mfLogScaleFactorLine */
    int32_t n_levels;          /* levels of mvScaleFactorsLine, 1 .. 16 */
    float scale_factor;        /* the line extractor's: the table is built from it */
    int32_t level_rule;        /* HVO_LF_LEVEL_* (reading 2) */
    int32_t map_per_keyframe;  /* hvo_fuse_lines: 0 = map_side[0] is shared by all key frames; 1 = key frame j is searched with map_side[j] */
} hvo_lf_params;
/* gate codes, in the reference's order */
#define HVO_LF_GATE_SEARCHED     0   /* also an entry for which GetLinesInArea returns nothing: best_idx stays -1 */
#define HVO_LF_GATE_SKIP         1   /* skip[i], or a bad slot */
#define HVO_LF_GATE_BEHIND       2   /* SPcZ < 0.0f || EPcZ < 0.0f: where the reference returns */
#define HVO_LF_GATE_OUT_OF_IMAGE 3   /* !IsInImage(u1, v1), or !IsInImage(u2, v2) */
#define HVO_LF_GATE_DIST_MIN     4   /* dist < 0.8f * mfMinDistance */
#define HVO_LF_GATE_DIST_MAX     5   /* dist > 1.2f * mfMaxDistance */
#define HVO_LF_GATE_VIEW_ANGLE   6   /* OM.dot(pn) < 0.5 * dist */
#define HVO_LF_GATE_LEVEL        7   /* HVO_LF_LEVEL_AS_WRITTEN only: the predicted level is outside [0, n_levels) */
typedef struct {               /* per key frame; every pointer but best_idx may be NULL.  n = the entries of this key frame's map side */
    int32_t *best_idx, *best_dist;   /* n: bestIdx / bestDist after the loop (-1 / 256 where no candidate survived or the entry was not searched) */
    int8_t  *gate;                   /* n */
    int32_t *level;                  /* n: nPredictedLevel (unclamped under HVO_LF_GATE_LEVEL); -1 where the reference did not compute it */
    float   *proj;                   /* n x 4: u1 v1 u2 v2 as far as the reference computed them (skip, behind: zeros; u1, v1 out of image: u1 v1 0 0) */
    int32_t *fused_entry, *fused_idx;   /* room for n each: the entries with best_dist <= th_low in ascending order and their key lines */
    int32_t *behind_entry;              /* room for n: the entries with HVO_LF_GATE_BEHIND in ascending order */
    int32_t n_fused, n_behind, n_searched, status; float kernel_ms[3];   /* device time of the whole call's records + projection, search, and
                                                                          * count + compaction kernels */
} hvo_lf_result;
/* On host arrays: n_kf key frames against map_side[0] (shared) or map_side[j].  Limits: 2048 lines per key frame, 65536 entries per key
 * frame, 2^24 padded (key frame, entry) pairs per call (HVO_ERR_UNSUPPORTED beyond); th_low > 255, n_levels outside 1 .. 16, an unknown
 * level_rule, empty bounds or a missing array are HVO_ERR_INVALID_ARG.  Every refusal is whole: nothing is written and hvo_last_error says
 * why.  n == 0 on either side is HVO_OK with no match.  One synchronisation per call. */
int hvo_fuse_lines(hvo_ctx *ctx, const hvo_lf_params *params, const hvo_lf_map *map_side, int n_kf, const hvo_lf_keyframe *keyframes, hvo_lf_result *results);
/* The map side as n slots of a resident line map, shared by all key frames: the map's device arrays are read in place (end points and
 * normal rounded to float as Mat_<float> << does), only the slot list and the skip bytes go up.  A bad slot counts as skipped; a slot
 * outside the map is HVO_ERR_INVALID_ARG (whole).  The map must live on the context's device.  The refusal's text is in hvo_last_error and
 * in hvo_line_map_last_error. */
int hvo_fuse_lines_slots(hvo_ctx *ctx, hvo_line_map *m, int n, const int32_t *slots, const hvo_lf_params *params, int n_kf, const hvo_lf_keyframe *keyframes,
                         hvo_lf_result *results);
/* The resident frame `cur` is the one key frame, under Tcw and cam (fx, fy, cx, cy), valid while the frame is in the ring.  Its key lines
 * and LBD descriptors are read where the stages left them (n_desc_rows = its line count); the bounds are its grid's.  The map side is
 * map_side (host arrays) or, when map_side is NULL, n slots of m.  skip: one byte per entry or NULL.  The stream must run an LSD stage:
 * otherwise HVO_ERR_INVALID_ARG with hvo_stream_last_error set.  The result is the host-array form's on the downloaded frame, bit for bit. */
int hvo_stream_fuse_lines(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_lf_params *params, const float Tcw[12], const uint8_t *skip,
                          const hvo_lf_map *map_side, hvo_line_map *m, int n, const int32_t *slots, hvo_lf_result *result);

/* ---- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:335-580; csrc/new_points.hip) ----
 * The epipolar search (ComputeF12 :1779-1796, ORBmatcher::SearchForTriangulation src/ORBmatcher.cc:668-836 with CheckDistEpipolarLine
 * :143-160) and the triangulation of every match (parallax test, 4 x 4 linear triangulation or KeyFrame::UnprojectStereo, two depth signs,
 * two chi-square tests, scale consistency) of the current key frame against n_kf neighbours in one call with one synchronisation.
 * SearchForTriangulation never sets vbMatched2 and runs without the rotation histogram here, so every (neighbour, idx1) pair is
 * independent; the only coupling between neighbours is AddMapPoint(pMP, idx1), which makes later neighbours skip idx1.  The call evaluates
 * every pair under the INITIAL occupancy and resolves the chain: the point at idx1 is created by the first neighbour, in list order, whose
 * match passes every gate.  A caller that leaves after neighbour i (`if(i>0 && CheckNewKeyFrames()) return;`) uses the lists of neighbours
 * 0 .. i: a prefix's results do not depend on what follows.  new MapPoint, AddObservation, AddMapPoint, ComputeDistinctiveDescriptors,
 * UpdateNormalAndDepth and mlpRecentAddedMapPoints stay with the caller (examples/create_map_points.cpp).  Two idx1 may be given the same
 * idx2 (the reference never marks vbMatched2): both are listed.
 *
 * Readings a caller can observe (csrc/new_points.hip and DESIGN.md section 7 have all of them; tests/new_points_ref.py is the definition):
 * only + - * / sqrt in a written order, nothing contracted.  Among equal descriptor distances the LAST candidate in index order wins (the
 * reference refuses `dist > bestDist`, not `>=`).  A feature whose octave is outside [0, n_levels) is refused for the pair.  The stereo
 * parallax cos(2 atan2(mb / 2, d)) is evaluated as (d d - h h) / (d d + h h), h = mb / 2, in double.  cv::SVD::compute of the 4 x 4 A is a
 * one-sided Jacobi iteration of exactly 12 sweeps in double on the float entries of A, its vector rounded to float once; bit parity with an OpenCV binary is NOT claimed.
 * u2_r uses the current key frame's bf; UnprojectStereo reads the distorted mvKeys; z <= 0 fails, so a NaN passes on; den == 0 fails. */
typedef struct {               /* the current key frame, and each neighbour */
    int32_t n;                 /* N */
    const hvo_keypoint *kp_un; /* mvKeysUn: x, y, octave are read */
    const hvo_keypoint *kp;    /* mvKeys, which UnprojectStereo reads; NULL: kp_un */
    const float   *uright, *depth;   /* mvuRight, mvDepth; NULL for both: every feature is monocular (one without the other is refused) */
    const uint8_t *desc;       /* n x 32 */
    const int32_t *node_id;    /* per feature, as hvo_*_compute_bow returns it; negative: the feature is in no node */
    const uint8_t *has_map_point;    /* one byte per feature: GetMapPoint(idx) != NULL (bad points included, as in the text) */
    float Tcw[12];             /* rows 0..2 of the pose, row-major 3 x 4 */
    float mb;                  /* the key frame's mb: the stereo parallax, and `baseline < pKF2->mb` for a neighbour (0: never too short) */
    uint8_t skip;              /* neighbours only: the caller's own pre-gate (the monocular median-depth ratio needs the map and stays on the host) */
} hvo_np_keyframe;
typedef struct {
    int32_t th_low;            /* TH_LOW (50); above 255 is refused */
    int32_t n_levels;          /* mnScaleLevels, 1 .. 16; mvScaleFactors and mvLevelSigma2 are the context's */
    float scale_factor;        /* mfScaleFactor: ratioFactor = 1.5f * mfScaleFactor */
    float bf;                  /* mpCurrentKeyFrame->mbf (both sides' u_r use it) */
} hvo_np_params;
/* outcome codes: the first `continue` the pair runs into, in the reference's order */
#define HVO_NP_CREATED      0
#define HVO_NP_OCCUPIED     1   /* idx1 holds a map point */
#define HVO_NP_NO_MATCH     2   /* also: every pair of a neighbour that was not searched (gate != 0) */
#define HVO_NP_LOW_PARALLAX 3   /* no stereo and very low parallax */
#define HVO_NP_W_ZERO       4   /* x3D.at<float>(3) == 0 */
#define HVO_NP_NO_DEPTH     5   /* UnprojectStereo returns an empty Mat for z <= 0: DEFINED here as a refusal of the pair */
#define HVO_NP_BEHIND_1     6
#define HVO_NP_BEHIND_2     7
#define HVO_NP_REPROJ_1     8
#define HVO_NP_REPROJ_2     9
#define HVO_NP_ZERO_DIST    10
#define HVO_NP_SCALE        11
#define HVO_NP_GATE_SEARCHED 0
#define HVO_NP_GATE_SKIP     1   /* the neighbour's skip byte */
#define HVO_NP_GATE_BASELINE 2   /* baseline < mb */
typedef struct {               /* per neighbour; n1 = the current key frame's feature count.  Every pointer but match_idx2 may be NULL */
    int32_t *match_idx2, *match_dist;   /* n1: vMatches12 of SearchForTriangulation under the initial occupancy and its distance; -1 / 256 where none */
    int8_t  *outcome, *branch;          /* n1: HVO_NP_*; 0 none, 1 linear triangulation, 2 UnprojectStereo of the current key frame, 3 of the neighbour */
    float   *x3d;                       /* n1 x 3: the point as far as the reference computed it, zeros otherwise */
    int32_t *created_idx1, *created_idx2;   /* room for n1 each: the points this neighbour creates after the chain is resolved, ascending idx1
                                             * (the order of vMatchedPairs) */
    int32_t n_created, gate, status;    /* gate: HVO_NP_GATE_* */
} hvo_np_result;
typedef struct {
    int32_t *owner;            /* n1 (may be NULL): the neighbour that creates the point at idx1, or -1; neighbour j's list is {idx1 : owner == j} */
    int32_t n_new;
    float kernel_ms[3];        /* device time of the neighbours' rows + the search, of the triangulation, of resolve + compaction */
} hvo_np_summary;
/* On host arrays.  cam: fx, fy, cx, cy are read (one camera for both sides, as in the reference's data sets).  Limits: 4096 features per side
 * (the rows are built by the bag-of-words kernel), 64 neighbours per call (HVO_ERR_UNSUPPORTED beyond); th_low > 255, n_levels outside
 * 1 .. 16 or a missing array are HVO_ERR_INVALID_ARG.  Every refusal is whole: nothing is written and hvo_last_error says why.  n == 0 on
 * either side or n_kf == 0 is HVO_OK with nothing created.  One synchronisation per call. */
int hvo_create_new_map_points(hvo_ctx *ctx, const hvo_camera *cam, const hvo_np_params *params, const hvo_np_keyframe *current,
                              int n_kf, const hvo_np_keyframe *neighbours, hvo_np_result *results, hvo_np_summary *summary);
/* The resident frame `cur` is the current key frame under Tcw.  It must hold the bag of words hvo_stream_compute_bow left on it for voc:
 * otherwise HVO_ERR_INVALID_ARG with hvo_stream_last_error set.  Key points, mvuRight, mvDepth, descriptors and node ids are read where the
 * stages left them; only the occupancy bytes, the pose and the neighbours go up.  The current key frame's mb is cam->b.  The result is the
 * host-array form's on the downloaded frame, bit for bit. */
int hvo_stream_create_new_map_points(hvo_stream *s, int64_t cur, const hvo_vocabulary *voc, const hvo_camera *cam, const hvo_np_params *params, const float Tcw[12],
                                     const uint8_t *has_map_point, int n_kf, const hvo_np_keyframe *neighbours, hvo_np_result *results, hvo_np_summary *summary);

/* ---- LocalMapping::CreateNewMapLinesConstraint (reference src/LocalMapping.cc:1064-1565; csrc/line_triang.inc) ----
 * LSDmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, true) (src/LSDmatcher.cpp:1195-1231: FrameBFMatch both ways with
 * lineDescriptorMAD, the mutual check, the two occupancy bytes) of the current key frame against every neighbour that passes the baseline
 * gate, and for every pair a < b of the searched neighbours and every current line the three-view triangulation with all of its gates, in
 * one call with one synchronisation.  The matches are mutual, so a match vector maps current lines to neighbour lines injectively and a key
 * frame at list position p is only indexed through match vector p: a created line can block nothing but later triples of the same current
 * line.  The call evaluates every (pair, line) under the occupancy at entry; the line at ikl is created by the first pair, in (a, b) order,
 * that passes.  `if(i>1 && CheckNewKeyFrames()) return;` leaves before anything is created: a caller that sees a new key frame discards
 * the call's result.  new MapLine, AddObservation, AddMapLine, ComputeDistinctiveDescriptors and UpdateAverageDir stay with the caller
 * (examples/create_map_lines.cpp).  A context is not thread-safe: the thread that runs this call beside CreateNewMapPoints owns a context.
 *
 * The reference skips a gated neighbour BEFORE it pushes the match vector, so its list of match vectors is compacted, and then reads
 * pKF2 = vpNeighKFs[a] by LIST POSITION.  After a gated neighbour match vectors are applied to the wrong key frames, and only `idx >= NL`
 * guards that.  HVO_NL_PAIR_AS_WRITTEN does exactly this; HVO_NL_PAIR_ALIGNED takes the searched neighbour itself.  Every pair reports
 * both positions.  Readings: csrc/line_triang.inc and DESIGN.md section 7; tests/new_lines_ref.py is the definition. */
typedef struct {               /* the current key frame, and each neighbour */
    int32_t n;                 /* NL */
    const hvo_keyline *kl;     /* mvKeyLines: sx, sy, ex, ey, angle and octave are read */
    const double  *linefn;     /* mvKeyLineFunctions, n x 3 */
    const uint8_t *desc;       /* mLineDescriptors, n x 32 */
    const uint8_t *has_map_line;     /* one byte per line: GetMapLine(idx) != NULL */
    float Tcw[12];             /* rows 0..2 of the pose, row-major 3 x 4 */
    hvo_camera cam;            /* the key frame's own mK: fx, fy, cx, cy are read */
    float mb;                  /* neighbours: `baseline < pKF2->mb` (0: never too short) */
    float median_depth;        /* neighbours: pKF2->ComputeSceneMedianDepth(2) as the caller read it (the map's points change beside this call) */
    uint8_t skip;              /* neighbours: the caller's own pre-gate (the monocular baseline / depth ratio) */
} hvo_nl_keyframe;
#define HVO_NL_PAIR_AS_WRITTEN 0
#define HVO_NL_PAIR_ALIGNED    1
typedef struct {
    int32_t th_high;           /* TH_HIGH (80); above 255 is refused */
    float nn_ratio;            /* lmatcher(0.85) */
    int32_t n_levels;          /* of the LINE pyramid, 1 .. 16 */
    float scale_factor;        /* of the LINE pyramid: mvLevelSigma2Line[l] = sf[l] * sf[l], sf[0] = 1, sf[l] = sf[l - 1] * scale_factor, all in float
                                * (LINEextractor's constructor; its level 0 is 1) */
    int32_t pairing;           /* HVO_NL_PAIR_* */
} hvo_nl_params;
/* outcome codes: the first `continue` the triple runs into, in the reference's order; one code per `continue` (the six depth signs, the six
 * line distances and the three overlap tests each have their own: view 1 is the current key frame, S / E the start / end point) */
#define HVO_NL_CREATED       0
#define HVO_NL_NO_MATCH      1   /* idx1 == -1 || idx2 == -1 */
#define HVO_NL_IDX_RANGE     2   /* idx1 >= pKF2->NL || idx2 >= pKF3->NL (a shifted pair under HVO_NL_PAIR_AS_WRITTEN) */
#define HVO_NL_OCCUPIED_1    3   /* never reached by a call: the search drops a match of an occupied current line, so the index test fires first */
#define HVO_NL_OCCUPIED_2    4   /* _2 and _3: reached by a shifted pair only (the search drops a match whose own line is occupied) */
#define HVO_NL_OCCUPIED_3    5
#define HVO_NL_BAD_OCTAVE    6   /* an octave of the three outside [0, n_levels): the reference would read mvLevelSigma2Line out of range */
#define HVO_NL_EPI_PARALLEL  7   /* abs(Result1) > 0.996 || abs(Result2) > 0.996 */
#define HVO_NL_NORM_ZERO_23  8
#define HVO_NL_NORM_ZERO_1   9
#define HVO_NL_NOT_COPLANAR  10  /* CosSita > 0.0087 */
#define HVO_NL_W_ZERO_S      11
#define HVO_NL_W_ZERO_E      12
#define HVO_NL_PARALLAX_S    13
#define HVO_NL_PARALLAX_E    14
#define HVO_NL_RATIO_1       15
#define HVO_NL_RATIO_2       16
#define HVO_NL_RATIO_3       17
#define HVO_NL_BEHIND_1S     18  /* .. _1E 19, _2S 20, _2E 21, _3S 22, _3E 23 */
#define HVO_NL_REPROJ_1S     24  /* .. _1E 25, _2S 26, _2E 27, _3S 28, _3E 29 */
#define HVO_NL_DISJOINT_1    30  /* the projected and the observed segment do not overlap on the chosen axis */
#define HVO_NL_OVERLAP_1     31  /* an overlap ratio below 0.85 */
#define HVO_NL_DISJOINT_2    32
#define HVO_NL_OVERLAP_2     33
#define HVO_NL_DISJOINT_3    34
#define HVO_NL_OVERLAP_3     35
#define HVO_NL_GATE_SEARCHED 0   /* as HVO_NP_GATE_* */
#define HVO_NL_GATE_SKIP     1
#define HVO_NL_GATE_BASELINE 2
#define HVO_NL_MAX_LINES      2048
#define HVO_NL_MAX_NEIGHBOURS 16
typedef struct {               /* per neighbour; n1 = the current key frame's line count */
    int32_t *match_idx;        /* n1: vMatchedIndices, -1 for no match (all -1 for a neighbour that was not searched) */
    int32_t n_matched, gate;   /* nlmatch; HVO_NL_GATE_* */
} hvo_nl_match;
typedef struct {               /* per pair.  outcome must be given; every other pointer may be NULL */
    int32_t kf2, kf3, mv2, mv3;         /* neighbour positions: which served as pKF2 / pKF3, and whose match vectors were applied */
    int8_t  *outcome;                   /* n1: HVO_NL_* */
    float   *line3d;                    /* n1 x 6: start and end point as far as they were computed, zeros otherwise */
    int32_t *created_idx0, *created_idx1, *created_idx2;   /* room for n1 each: ikl ascending, with its idx1 and idx2, after the chain is resolved */
    int32_t n_created, status;
} hvo_nl_result;
typedef struct {
    int32_t *owner_pair;       /* n1 (may be NULL): the pair that creates the line at ikl, or -1 */
    int32_t n_new, n_pairs;    /* n_pairs: results written, ns (ns - 1) / 2 for ns searched neighbours */
    float kernel_ms[3];        /* device time of the search, of the triangulation, of resolve + compaction */
} hvo_nl_summary;
/* On host arrays.  Limits: 2048 lines per side, 16 neighbours (120 pairs) per call, HVO_ERR_UNSUPPORTED beyond.  A missing array,
 * th_high > 255, n_levels outside 1 .. 16, an unknown pairing or n_pairs_cap below the number of pairs are HVO_ERR_INVALID_ARG.  Every
 * refusal is whole: nothing is written and hvo_last_error says why.  Fewer than 2 neighbours, fewer than 2 searched, or n == 0 on the current
 * side is HVO_OK with nothing created (the matches' gates are still reported).  A neighbour with fewer than 2 lines matches nothing, and so
 * does a current key frame with fewer than 2 (knnMatch(k = 2) needs two train descriptors).  One synchronisation per call. */
int hvo_create_new_map_lines(hvo_ctx *ctx, const hvo_nl_params *params, const hvo_nl_keyframe *current, int n_kf, const hvo_nl_keyframe *neighbours,
                             hvo_nl_match *matches, int n_pairs_cap, hvo_nl_result *results, hvo_nl_summary *summary);
/* The resident frame `cur` (either LSD stage) is the current key frame under Tcw with camera cam: key lines, line functions and descriptors
 * are read where the stage left them; only the occupancy bytes, the pose and the neighbours go up.  The result is the host-array form's on
 * the downloaded frame, bit for bit. */
int hvo_stream_create_new_map_lines(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_nl_params *params, const float Tcw[12],
                                    const uint8_t *has_map_line, int n_kf, const hvo_nl_keyframe *neighbours, hvo_nl_match *matches, int n_pairs_cap,
                                    hvo_nl_result *results, hvo_nl_summary *summary);

/* ---- MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (reference src/MapPoint.cc:240-305, 328-369) and
 * MapLine::ComputeDistinctiveDescriptors + UpdateAverageDir (src/MapLine.cpp:331-396, 404-455); csrc/map_refresh.inc ----
 * One call refreshes n map points (or lines) from their observations: the descriptor with the least median Hamming distance to the other
 * observers' descriptors, the mean viewing direction, the distance range and, for a line, the world vector.  No feature reads another's
 * result.  The observations are a ragged list in the order mObservations iterates (std::map<KeyFrame *, size_t>: the caller's pointer
 * order): the order decides which of equal medians wins (the first) and the rounding of the sums.  The caller resolves
 * `observations[pRefKF]` itself; see INTEGRATION.md for operator[] on the copied map when pRefKF is not an observer.
 * Readings: csrc/map_refresh.inc and DESIGN.md section 7; tests/map_refresh_ref.py is the definition. */
#define HVO_MR_DESCRIPTOR 1    /* hvo_mr_params.what: ComputeDistinctiveDescriptors */
#define HVO_MR_GEOMETRY   2    /* UpdateNormalAndDepth / UpdateAverageDir (the optimiser calls only this half) */
#define HVO_MR_MAX_OBS        256        /* observations per feature */
#define HVO_MR_MAX_FEATURES   65536      /* features per call */
#define HVO_MR_MAX_OBS_TOTAL  1048576    /* observations per call */
/* status, one per feature: the first that applies */
#define HVO_MR_REFRESHED  0
#define HVO_MR_SKIPPED    1    /* skip (mbBad), or a bad slot in the slot form: nothing is written */
#define HVO_MR_NO_OBS     2    /* observations.empty(): nothing is written */
#define HVO_MR_DESC_KEPT  3    /* DESCRIPTOR asked for and every observer is bad: the descriptor is kept, the geometry is written */
#define HVO_MR_BAD_LEVEL  4    /* GEOMETRY asked for and ref_level outside [0, n_levels): the reference would read its table out of bounds.
                                * max_dist and min_dist are left as they were (also under status 3); descriptor, normal and wvec are written */
typedef struct {
    int32_t n_levels;          /* 1 .. 16: mnScaleLevels (points) / mnScaleLevelsLine (lines) */
    float scale_factor;        /* lines: sf[0] = 1, sf[l] = sf[l - 1] * scale_factor in float (as hvo_nl_params).  Points read the context's
                                * ORB pyramid table (n_levels may not exceed the context's levels) and ignore this field */
    int32_t what;              /* HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY, not 0 */
} hvo_mr_params;
typedef struct {               /* what goes up.  n_obs = obs_start[n] */
    int32_t n;
    const int32_t *obs_start;  /* n + 1: CSR over the observations, obs_start[0] = 0, non-decreasing */
    const uint8_t *obs_desc;   /* n_obs x 32: the observing key frame's descriptor row (ORB / LBD) */
    const float   *obs_Ow;     /* n_obs x 3: its GetCameraCenter() */
    const uint8_t *kf_bad;     /* n_obs, or NULL for none: pKF->isBad().  A bad observer stays out of the descriptor list and still counts in the normal */
    const float   *ref_Ow;     /* n x 3: pRefKF->GetCameraCenter() */
    const int32_t *ref_level;  /* n: pRefKF->mvKeysUn[observations[pRefKF]].octave (mvKeyLines for a line) */
    const uint8_t *skip;       /* n, or NULL for none: mbBad */
} hvo_mr_input;
typedef struct {               /* every pointer may be NULL.  An entry that the status says was not written is left as the caller had it */
    int32_t *best_obs;         /* n: the winner's index within the feature's own observation list (bad observers counted), -1 when no descriptor was written */
    int32_t *best_median;      /* n: its median, -1 likewise */
    uint8_t *desc;             /* n x 32 */
    float   *normal;           /* n x 3: mNormalVector */
    float   *max_dist, *min_dist;      /* n: RAW mfMaxDistance / mfMinDistance */
    uint8_t *status;           /* n: HVO_MR_* */
    float   kernel_ms;         /* device time of the kernel */
} hvo_mr_point_out;
typedef struct {
    int32_t *best_obs, *best_median;
    uint8_t *desc;
    double  *normal;           /* n x 3 */
    double  *wvec;             /* n x 3: mWorldVector */
    float   *max_dist, *min_dist;
    uint8_t *status;
    float   kernel_ms;
} hvo_mr_line_out;
/* On host arrays: pos is n x 3 floats (mWorldPos) / n x 6 doubles (start, end).  Limits: HVO_MR_MAX_*; beyond them the call is refused
 * whole with HVO_ERR_UNSUPPORTED.  A missing array, obs_start[0] != 0, a decreasing obs_start, what == 0 or with unknown bits, or n_levels
 * outside 1 .. 16 is HVO_ERR_INVALID_ARG.  On a refusal nothing is written and hvo_last_error says why.  n == 0 is HVO_OK.  One
 * synchronisation per call. */
int hvo_refresh_map_points(hvo_ctx *ctx, const hvo_mr_params *params, const hvo_mr_input *in, const float *pos, hvo_mr_point_out *out);
int hvo_refresh_map_lines(hvo_ctx *ctx, const hvo_mr_params *params, const hvo_mr_input *in, const double *pos, hvo_mr_line_out *out);
/* On n slots of a resident map: the position is the slot's, and descriptor, normal, distance range (and world vector) are rewritten in
 * place, in the map's device arrays and in its host mirror (hvo_*_map_slot reads back exactly what `out` reports); observed and bad are
 * never touched.  Only the observation arrays and the per-feature side go up.  A bad slot counts as skipped.  A slot outside the map or
 * listed twice is HVO_ERR_INVALID_ARG (whole); the map must live on the context's device.  A refusal's text is in hvo_last_error and in
 * the map's last error.  Bit for bit the host-array form on the slots' positions. */
int hvo_point_map_refresh(hvo_ctx *ctx, hvo_point_map *m, const int32_t *slots, const hvo_mr_params *params, const hvo_mr_input *in, hvo_mr_point_out *out);
int hvo_line_map_refresh(hvo_ctx *ctx, hvo_line_map *m, const int32_t *slots, const hvo_mr_params *params, const hvo_mr_input *in, hvo_mr_line_out *out);

/* ---- Optimizer::LocalMapOptimization (reference src/Optimizer.cc:3014-3940, called at src/LocalMapping.cc:122; csrc/local_ba.hip) ----
 * Local bundle adjustment over the covisibility window: one SE3 vertex per key frame (free unless `fixed`), one XYZ vertex per map point,
 * a start and an end XYZ vertex per map line; EdgeSE3ProjectXYZ per point observation, two DistPt2Line2DMultiFrame per line observation,
 * ParEptsNVector3DSingleFrame against the Manhattan axis, ParEptsNVector2DMultiFrame / PerpEptsNVector2DMultiFrame per parallel /
 * perpendicular entry, all under Huber kernels; Levenberg with optimize(5), the classification of :3656-3743, optimize(10), and the
 * erase tests of :3753-3847 as flags.  A line is ONE 6-dimensional landmark here: every landmark (3 x 3 or 6 x 6 block, plus lambda) is
 * eliminated and the dense reduced system over the free key frames (at most 384 unknowns) is factored by LDL^T without pivoting -- the
 * step g2o solves, with another rounding.  The Levenberg loop runs on the host over the launches; two calls on the same bytes return the
 * same bytes (no floating-point atomic, every sum in a fixed order).
 *
 * The object owns a grow-only workspace (graph, per-edge blocks, reduced system, one pinned block) on its device; create it once beside
 * the map and reuse it for every key frame.  Not thread-safe.
 *
 * Conventions.  Key frame 0 of the list is the CURRENT key frame (pKF); the local key frames come first, the outside observers after
 * them with fixed = 1; a local key frame is fixed iff its mnId == 0.  Observations are CSR lists per point / per line (obs_start has
 * n + 1 entries), each naming its observer by its index in the key-frame list; the caller leaves out bad key frames, bad points and bad
 * lines.  par / perp entries are the (key frame, k) entries of GetParObservations() / GetPerpObservations() in map order with idx =
 * observation.second[k] and linefn = that key frame's mvKeyLineFunctions[idx]; entries of key frames with mnId > maxKFid or isBad() are
 * left out by the caller; par_map_size / perp_map_size are the maps' numbers of KEYS.  manh_axis is 3 x 3 row-major, column a - 1 =
 * axis a.
 *
 * The readings taken (the restatement tests/local_ba_ref.py makes the same ones):
 *  1. the END-point edge and the par / perp edges take fx fy cx cy of key frame 0, the start-point edge its observer's (:3459, :3518, :3579);
 *  2. chi2() is read from the error an edge HOLDS: an edge put on level 1 after round 1 is never evaluated again and its erase test
 *     reads round 1's last evaluation (the last trial, accepted or not); isDepthPositive() is evaluated at the final estimate;
 *  3. the erase test of a line observation reads its START-point edge twice (:3772-3774); the classification between the rounds reads
 *     start or end;
 *  4. flags come back per observation; pairing an erased line observation with a key frame (vpLineEdgeKF holds two entries per
 *     observation and is indexed by observation, :3782) is host logic (hvo::walkErased);
 *  5. vpLineManhKF is never filled (:3800 reads past its end): manh_erase is a flag per line and the caller decides;
 *  6. zero points or zero lines are ordinary inputs (the reference reads MapPointID[-1]);
 *  7. a par / perp entry's key frame must be in the list: an index outside it is refused (the reference passes a null vertex);
 *  8. isBad() is read as false throughout: the graph holds only non-bad elements.
 * Also: SE3Quat::map is the quaternion's rotation matrix applied to the point; landmark blocks and the reduced system are inverted /
 * factored by LDL^T without pivoting, "not positive" = a pivot <= 0 of the reduced system; every key frame's returned pose is its
 * quaternion estimate written out (Converter::toCvMat), fixed ones included.
 *
 * Limits, refused whole with HVO_ERR_UNSUPPORTED, the reason in hvo_local_ba_last_error and NO output written: more than 64 free or
 * 1024 key frames, 65536 points, 16384 lines, 2^20 point observations, 2^18 line observations, 2^18 par plus perp entries, a key-frame
 * index out of range, a key frame observing one point or one line twice.  No free key frame or no edge at all: status
 * HVO_LBA_NOTHING, outputs = inputs, no launch.  A landmark or key frame without active edges keeps its estimate. */
typedef struct hvo_local_ba hvo_local_ba;
#define HVO_LBA_MAX_FREE_KF   64
#define HVO_LBA_MAX_KF        1024
#define HVO_LBA_MAX_POINTS    65536
#define HVO_LBA_MAX_LINES     16384
#define HVO_LBA_MAX_PT_OBS    (1 << 20)
#define HVO_LBA_MAX_LN_OBS    (1 << 18)
#define HVO_LBA_MAX_STRUCT    (1 << 18)
#define HVO_LBA_OPTIMISED 0       /* status: both rounds ran (or the stop flag ended them) */
#define HVO_LBA_NOTHING   1       /*         no free key frame or no edge: outputs = inputs */
#define HVO_LBA_STOPPED   2       /*         the stop flag was set at the test before the first round (:3641): outputs = inputs */
typedef struct {
    int32_t iterations[2];         /* optimize(5), optimize(10) */
    int32_t max_trials;            /* 10: g2o's maxTrialsAfterFailure */
    int32_t stop_at_poll;          /* -1: off; k: the k-th read of the stop flag (0-based) and every later one reads "stop" (tests) */
    double huber_delta[3];         /* point, line end point, parallel / perpendicular / Manhattan: (float)sqrt(5.991), sqrt(3.84), sqrt(0.08) */
    double chi2_gate[3];           /* 5.991, 3.84, 0.13 */
    double inv_sigma[3];           /* line end points 0.3, Manhattan 0.3, structural 0.5 (+ map_size / 10) */
} hvo_local_ba_params;
typedef struct {
    int32_t n_kf, n_points, n_lines, manh_available;
    const float *Tcw;              /* n_kf x 12: rows 0..2 of GetPose() */
    const uint8_t *fixed;          /* n_kf */
    const float *cam;              /* n_kf x 4: fx fy cx cy */
    const float *pt_pos;           /* n_points x 3 */
    const int32_t *pt_obs_start;   /* n_points + 1 */
    const int32_t *pt_obs_kf;
    const float *pt_obs_uv;        /* x 2: mvKeysUn[idx].pt */
    const float *pt_obs_inv_sigma2;
    const double *ln_pos;          /* n_lines x 6 */
    const int32_t *ln_manh_idx;    /* n_lines: GetManhIdx() */
    const int32_t *ln_obs_start;   /* n_lines + 1 */
    const int32_t *ln_obs_kf;
    const double *ln_obs_fn;       /* x 3: mvKeyLineFunctions[idx] */
    const int32_t *par_start, *par_kf, *par_idx; const double *par_fn; const int32_t *par_map_size;
    const int32_t *perp_start, *perp_kf, *perp_idx; const double *perp_fn; const int32_t *perp_map_size;
    const double *manh_axis;       /* 9, may be NULL when manh_available == 0 */
} hvo_local_ba_graph;
typedef struct {
    float *Tcw_f; double *Tcw_d;   /* n_kf x 12 */
    float *pt_f; double *pt_d;     /* n_points x 3 */
    float *ln_f; double *ln_d;     /* n_lines x 6; SetWorldPos receives the float values (Converter::toCvMat) */
    uint8_t *pt_erase, *ln_erase;  /* per point / line observation */
    uint8_t *manh_erase;           /* per line */
    uint8_t *par_erase, *perp_erase;   /* per entry */
    uint8_t *par_made, *perp_made; /* per entry: 0 = no edge (idx < 0, linefn[0] == 0 or -1, a NaN, or the line was skipped) */
    uint8_t *line_made;            /* per line: 0 = skipped whole (:3358-3366) */
    int32_t iterations[2], trials[2];
    double lambda[2], chi2[2];
    int32_t n_free_kf, n_pt_edges, n_line_obs, n_manh_edges, n_par_edges, n_perp_edges, n_lines_made, rounds;
    int32_t stopped_at;            /* index of the first poll that read "stop", or -1 */
    int32_t status;                /* HVO_LBA_* */
} hvo_local_ba_result;
int hvo_local_ba_create(int device, hvo_local_ba **ba);
void hvo_local_ba_destroy(hvo_local_ba *ba);
const char *hvo_local_ba_last_error(const hvo_local_ba *ba);
/* device time of the last call's launches (hipEvents around every linearisation's and every trial's group of kernels, summed) */
int hvo_local_ba_last_ms(const hvo_local_ba *ba, float *ms);
/* its parts: ms[0] the linearisations, ms[1] the trials, ms[2] of the trials the one-workgroup factorisation, ms[3] the whole call on the
 * stream from the upload to the last download (the host's Levenberg bookkeeping between the launches included); n = their counts */
int hvo_local_ba_last_profile(const hvo_local_ba *ba, float ms[4], int32_t n[2]);
void hvo_local_ba_default_params(hvo_local_ba_params *p);
/* stop: the caller's abort flag (mbAbortBA), polled where g2o calls terminate() and at :3641 / :3650; may be NULL */
int hvo_local_ba_optimize(hvo_local_ba *ba, const hvo_local_ba_params *params, const hvo_local_ba_graph *graph, const volatile int *stop,
                          hvo_local_ba_result *res);

/* ---- Tracking::CreateNewKeyFrame (reference src/Tracking.cc:3032-3187, points and lines), Tracking::StereoInitialization (1364-1400) and
 * Tracking::UpdateLastFrame (2194-2246); csrc/new_keyframe.hip ----
 * One call makes the new map points and map lines of a key frame from the frame's own arrays and writes them into the resident maps: the
 * selection (the depth order, the counters and their breaks), Frame::UnprojectStereo / PtToWorldCoord, the descriptor, the normal and
 * the distance range of the sole observer, and the structural relation of every new line to the frame's lines.  tests/new_keyframe_ref.py
 * is the definition; the readings are in csrc/new_keyframe.hip and DESIGN.md section 7.
 *   HVO_KFI_KEYFRAME   points: the features with depth > 0 in (depth, index) order; the first min(M, max(c, 100) + 1) are processed (c: those
 *                      with depth <= th_depth) and a processed one is created when held is -1, an unobserved slot or
 *                      HVO_HELD_FOREIGN_UNOBSERVED.  Lines: the lines whose end points both have z != 0, in ((float)max(sz, ez), index)
 *                      order; the counter runs over the creatable ones only: the first max(c', 100) + 1 of them are created
 *   HVO_KFI_INIT       index order, no limit: points with depth > 0; lines with keyline sx > 0 and A[0] != 0.  held is ignored on input
 *   HVO_KFI_TEMPORAL   the point rule of HVO_KFI_KEYFRAME; nothing is written to a map, lines are not read, the normal is the Frame
 *                      constructor's (src/MapPoint.cc:45-69: a -0.0 component stays -0.0, where UpdateNormalAndDepth's sum gives +0.0)
 * A created entry k (creation order) goes to slot first + k, good and observed, and held[i] becomes its slot; with first = -1 (and always in
 * HVO_KFI_TEMPORAL) the values are returned only and held[i] becomes HVO_HELD_FOREIGN_OBSERVED (HVO_HELD_FOREIGN_UNOBSERVED in
 * HVO_KFI_TEMPORAL).  In HVO_KFI_KEYFRAME a processed unobserved entry is cleared (-1) before it is created, in HVO_KFI_INIT every entry that is
 * not created becomes -1.  n_slots moves to first + n_created; slots outside [first, first + n_created) keep their bytes. */
#define HVO_KFI_KEYFRAME 0
#define HVO_KFI_INIT     1
#define HVO_KFI_TEMPORAL 2
#define HVO_KFI_MAX_FEATURES 16384       /* key points of the frame; more is HVO_ERR_UNSUPPORTED, nothing is written */
#define HVO_KFI_MAX_LINES    2048        /* key lines of the frame */
#define HVO_KFI_CREATED   0
#define HVO_KFI_BAD_LEVEL 1              /* the octave is outside [0, n_levels): the reference would read its table out of bounds.  The entry is counted
                                          * by the selection, takes no slot and is not created */
typedef struct hvo_kf_insert hvo_kf_insert;
typedef struct {
    int32_t mode;                 /* HVO_KFI_* */
    float   th_depth;             /* mThDepth */
    int32_t n_levels;             /* points: mnScaleLevels, 1 .. the context's ORB levels (mvScaleFactors is the context's table) */
    int32_t line_n_levels;        /* lines: 1 .. 16, with the table sf[0] = 1, sf[l] = sf[l - 1] * line_scale_factor in float (as hvo_mr_params) */
    float   line_scale_factor;
    int32_t line_geometry;        /* 1 (default): normal and distance range of a new line as MapLine::UpdateAverageDir gives them for the sole
                                   * observer (Tracking.cc:3171 uncommented); 0: normal zero and both distances 0, the constructor's members */
    double  cos_par, cos_perp;    /* mCosThPar, mCosThPerp (src/Manhattan.cpp:28-30) */
    int32_t first_point_slot, first_line_slot;     /* -1: return the values only */
} hvo_kfi_params;
/* HVO_KFI_KEYFRAME, th_depth 3, 8 point levels, 1 line level with scale 1.2, line_geometry 1, cos(3 * 0.0174533) and cos(87 * 0.0174533), both
 * first slots -1.  th_depth is the caller's mThDepth (mbf * ThDepth / fx of the settings file) */
void hvo_kfi_default_params(hvo_kfi_params *p);
typedef struct {                  /* the frame side on host arrays.  Lines are skipped when n_kl == 0 */
    const hvo_keypoint *kp_un; const float *depth; const uint8_t *desc; int32_t n_kp;      /* mvKeysUn, mvDepth, mDescriptors */
    const hvo_keyline *keylines; const uint8_t *ldesc; const hvo_line3d *lines3d; int32_t n_kl;    /* mvKeylinesUn, mLdesc, mvLines3D */
} hvo_kfi_frame;
typedef struct {                  /* held_*: in and out; every other pointer is an output, may be NULL, and has room for n_kp (points) / n_kl (lines) entries */
    int32_t n_kp, n_kl;           /* the lengths of held_points / held_lines: at least the frame's counts (the resident form reads the frame's own) */
    int32_t *held_points;         /* mvpMapPoints[i]: a slot, -1, HVO_HELD_FOREIGN_OBSERVED or HVO_HELD_FOREIGN_UNOBSERVED */
    int32_t *held_lines;          /* mvpMapLines[i] likewise, against the line map */
    /* per selected point, in creation order (n_point_entries of them) */
    int32_t *pt_index, *pt_slot;  /* the feature; its slot (-1: returned only, or not created) */
    uint8_t *pt_status;           /* HVO_KFI_CREATED / HVO_KFI_BAD_LEVEL */
    float *pt_pos, *pt_normal;    /* x 3 */
    float *pt_max_dist, *pt_min_dist;
    /* per selected line (n_line_entries of them) */
    int32_t *ln_index, *ln_slot; uint8_t *ln_status;
    double *ln_pos, *ln_wvec, *ln_normal;          /* x 6 (start, end), x 3, x 3 */
    float *ln_max_dist, *ln_min_dist;
    uint8_t *ln_rel;              /* HVO_KFI_KEYFRAME only: n_line_entries x (the frame's key-line count), rows packed: 0 / 1 parallel / 2 perpendicular
                                   * of the new line against frame line i; frame lines with A[0] == 0.0 and rows of entries that were not created are 0.
                                   * Room for n_kl x n_kl.  The mvParallelLines[i]->size() > 0 gate stays with the caller */
} hvo_kfi_io;
typedef struct {
    int32_t n_kp, n_kl;                            /* the frame's counts as the call read them */
    int32_t n_point_entries, n_points_created;     /* entries = created + those refused for their level */
    int32_t n_line_entries, n_lines_created;
    int32_t n_point_candidates, n_line_candidates;
    float   kernel_ms;                             /* device time of the call's launches */
    int32_t status;
} hvo_kfi_result;
/* The handle owns a grow-only workspace on its device (a device block, a pinned block, events): create it once beside the maps. */
hvo_kf_insert *hvo_kf_insert_create(int device);
void hvo_kf_insert_destroy(hvo_kf_insert *k);
const char *hvo_kf_insert_last_error(const hvo_kf_insert *k);
/* On host arrays.  pmap / lmap may be NULL where the matching first_*_slot is -1 and held names no slot.  Refusals are whole and write
 * nothing (held, the maps' bytes and n_slots stay): more than HVO_KFI_MAX_* features (HVO_ERR_UNSUPPORTED); a NaN among the line depths, which
 * leaves the reference's sort undefined, a held value outside the map, a missing array (HVO_ERR_INVALID_ARG).  One launch sequence, one
 * download, one synchronisation. */
int hvo_create_keyframe_features(hvo_kf_insert *k, hvo_ctx *ctx, hvo_point_map *pmap, hvo_line_map *lmap, const hvo_camera *cam, const float Tcw[12],
                                 const hvo_kfi_params *params, const hvo_kfi_frame *frame, hvo_kfi_io *io, hvo_kfi_result *res);
/* On the resident frame `cur` of a stream: mvKeysUn, mvDepth, the descriptors, the key lines and the 3-D lines are read where they lie (after
 * hvo_stream_line_struct_optimize: the optimised lines); only held goes up.  The stream must run HVO_STAGE_ORB, an LSD stage and
 * HVO_STAGE_LINES3D, with bf > 0, and the frame must have been submitted with depth. */
int hvo_stream_create_keyframe_features(hvo_kf_insert *k, hvo_stream *s, hvo_point_map *pmap, hvo_line_map *lmap, int64_t cur, const hvo_camera *cam,
                                        const float Tcw[12], const hvo_kfi_params *params, hvo_kfi_io *io, hvo_kfi_result *res);

/* Page-lock (hipHostRegister) / unlock a caller's host buffer. Images handed to hvo_batch_upload / hvo_stream_submit and result
 * slabs handed to hvo_batch_download move by DMA at the link rate when they are pinned (no staging copy on either side); equally
 * sized, equally spaced pinned destinations (e.g. labels8 of consecutive frames in one slab) take a single strided DMA. */
int hvo_pin_host(void *p, size_t bytes);
int hvo_unpin_host(void *p);

/* What the line growing of the last small batch / streamed frame fell back on (lsd_async.inc: several waves per frame, used for up to 16 frames):
 * frames that were grown again by the one-wave kernel because the workers gave up (never an error: the result is the same lines), workers that
 * found themselves on another XCD than their frame's and counted themselves out (exact, slower; > 0 means the dispatcher does not deal
 * workgroups b, b + 8, ... to one XCD on this system: set HVO_LSD_ASYNC=0), and the workers per frame of that launch (0: it was not async). */
int hvo_lsd_async_report(hvo_ctx *ctx, int *frames_regrown, int *foreign_workers, int *workers_per_frame);

/* ---- alternative readings of two un-vendored OpenCV calls (SURVEY.md Appendix A "(?)"; csrc/readings.hip) ----
 * The defaults (mask 0) are what the golden vectors pin.  A maintainer with the author's OpenCV 3.2 decides by running one
 * cv::GaussianBlur(ramp image, 7 x 7, sigma 2) and comparing it with both readings; the oracle has the same
 * switches (oracle.h orc_set_reading), and the parity tests run with both sides flipped. */
#define HVO_READING_BLUR_FLOAT 1u   /* cv::GaussianBlur on CV_8U served by IPP: float kernel, one rounding (ORB's 7x7 blur, LBD's 5x5 blur; with LSD_8U the detector's too) */
#define HVO_READING_LSD_8U     2u   /* cv::LineSegmentDetector working on CV_8U: u8 blur and u8 0.8x resize, gradients of the rounded bytes */
int hvo_set_readings(hvo_ctx *ctx, unsigned mask);            /* takes effect with the next extraction; HVO_ERR_INVALID_ARG for unknown bits */
int hvo_stream_set_readings(hvo_stream *s, unsigned mask);     /* every frame submitted afterwards */

/* ---- measurement hooks (bench.py) ---- */
/* Per-kernel-group device time of the last hvo_batch_run, measured with hipEvents on the ctx
 * stream.  names[i] points at static strings.  Returns the number of groups written (<= cap). */
int hvo_profile_last(const hvo_ctx *ctx, const char **names, float *ms, int cap);
/* 0: off (default); 1: hipEvent bracketing of each kernel group inside hvo_batch_run; 2: as 1 and the
 * three subsystems run back to back on one stream, so that group times are free of cross-stream contention */
int hvo_profile_enable(hvo_ctx *ctx, int on);

#ifdef __cplusplus
}
#endif
#endif /* HVO_H */
