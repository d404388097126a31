// hvo.hpp -- header-only C++ mirror of the reference's front-end interfaces on top of the C ABI
// (include/hvo.h).  Same class names, constructor arguments, call operators and error behaviour as
//
//   ORB_SLAM2::ORBextractor      reference include/ORBextractor.h:47-116, src/ORBextractor.cc:408,1041
//   ORB_SLAM2::LINEextractor     reference include/LineExtractor.h:186-283, src/LineExtractor.cpp:329
//   PlaneDetection               reference include/PlaneExtractor.h:36-56,  src/PlaneExtractor.cpp:26-66
//   ORB_SLAM2::ORBmatcher        reference include/ORBmatcher.h:44,         src/ORBmatcher.cc:1676
//   ORB_SLAM2::LSDmatcher        reference include/LSDmatcher.h:43,         src/LSDmatcher.cpp:803-863
//
// but without OpenCV/Eigen types: images are (pointer, width, height, stride) and results are
// std::vectors of PODs whose layout equals cv::KeyPoint / cv::line_descriptor::KeyLine, so a
// Frame.cc adaptor is a reinterpret of vector storage.  No CPU fallback: every call
// throws hvo::Error when libhvo.so / a gfx950 device is unavailable.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "hvo.h"

namespace hvo {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &what) : std::runtime_error(what + ": " + hvo_strerror(s)), status(s) {}
};
inline void check(int rc, const char *what) { if (rc != HVO_OK) throw Error(rc, what); }

using KeyPoint = hvo_keypoint;   // == cv::KeyPoint (28 B)
using KeyLine = hvo_keyline;     // == cv::line_descriptor::KeyLine (68 B)
using Plane = hvo_plane;
static_assert(sizeof(KeyPoint) == 28 && sizeof(KeyLine) == 68, "layouts must match OpenCV's");

struct Image8 { const uint8_t *data; int width, height, stride; bool empty() const { return !data || width <= 0 || height <= 0; } };
struct Image16 { const uint16_t *data; int width, height, stride; bool empty() const { return !data || width <= 0 || height <= 0; } };

// shared ownership of one hvo_ctx (one HIP stream set; NOT thread-safe, like ORBextractor)
class Context {
public:
    explicit Context(const hvo_params &p) { check(hvo_create(&p, &ctx_), "hvo_create"); }
    ~Context() { hvo_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    hvo_ctx *get() const { return ctx_; }
private:
    hvo_ctx *ctx_ = nullptr;
};

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
        : nfeatures_(nfeatures), nlevels_(nlevels), scaleFactor_(scaleFactor)
    {
        hvo_params p; hvo_default_params(&p);
        p.orb_nfeatures = nfeatures; p.orb_scale_factor = scaleFactor; p.orb_nlevels = nlevels;
        p.orb_ini_th_fast = iniThFAST; p.orb_min_th_fast = minThFAST; p.device = device;
        ctx_.reset(new Context(p));
        // scale tables exactly as ORBextractor.cc:413-428
        mvScaleFactor.resize(nlevels); mvLevelSigma2.resize(nlevels); mvInvScaleFactor.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
        mvScaleFactor[0] = 1.0f; mvLevelSigma2[0] = 1.0f;
        for (int i = 1; i < nlevels; i++) { mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor; mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i]; }
        for (int i = 0; i < nlevels; i++) { mvInvScaleFactor[i] = 1.0f / mvScaleFactor[i]; mvInvLevelSigma2[i] = 1.0f / mvLevelSigma2[i]; }
    }
    // operator()(image, mask, keypoints, descriptors): the mask is ignored (ORBextractor.h:58)
    void operator()(const Image8 &image, std::vector<KeyPoint> &keypoints, std::vector<uint8_t> &descriptors)
    {
        keypoints.clear(); descriptors.clear();
        if (image.empty()) return;                                   // ORBextractor.cc:1044
        const int cap = nfeatures_ + 8 * nlevels_ + 64;
        keypoints.resize(cap); descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(hvo_extract_orb(ctx_->get(), image.data, image.width, image.height, image.stride, keypoints.data(), descriptors.data(), cap, &n), "hvo_extract_orb");
        keypoints.resize(n); descriptors.resize((size_t)n * 32);
    }
    int GetLevels() const { return nlevels_; }
    float GetScaleFactor() const { return scaleFactor_; }
    const std::vector<float> &GetScaleFactors() const { return mvScaleFactor; }
    const std::vector<float> &GetInverseScaleFactors() const { return mvInvScaleFactor; }
    const std::vector<float> &GetScaleSigmaSquares() const { return mvLevelSigma2; }
    const std::vector<float> &GetInverseScaleSigmaSquares() const { return mvInvLevelSigma2; }
    hvo_ctx *ctx() const { return ctx_->get(); }
private:
    int nfeatures_, nlevels_; float scaleFactor_;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
    std::unique_ptr<Context> ctx_;
};

class LINEextractor {
public:
    // LINEextractor(numOctaves, scale, nLSDFeature, min_line_length) (LineExtractor.h:190)
    LINEextractor(int numOctaves, float scale, unsigned nLSDFeature, double /*min_line_length*/ = 0, int device = 0)
        : nfeat_((int)nLSDFeature), numOctaves_(numOctaves), scale_(scale)
    {
        hvo_params p; hvo_default_params(&p);
        p.lsd_num_octaves = numOctaves; p.lsd_scale = scale; p.lsd_nfeatures = (int)nLSDFeature; p.device = device;
        ctx_.reset(new Context(p));
    }
    // operator()(image, mask, keylines, descriptors, lineVec2d); lineVec2d is n x 3 doubles
    void operator()(const Image8 &image, std::vector<KeyLine> &keylines, std::vector<uint8_t> &descriptors, std::vector<double> &lineVec2d)
    {
        keylines.clear(); descriptors.clear(); lineVec2d.clear();
        if (image.empty()) return;                                   // LineExtractor.cpp:331-332
        const int cap = nfeat_ > 0 ? nfeat_ : 1;
        keylines.resize(cap); descriptors.resize((size_t)cap * 32); lineVec2d.resize((size_t)cap * 3);
        int n = 0;
        check(hvo_extract_lsd(ctx_->get(), image.data, image.width, image.height, image.stride, keylines.data(), descriptors.data(), lineVec2d.data(), cap, &n), "hvo_extract_lsd");
        keylines.resize(n); descriptors.resize((size_t)n * 32); lineVec2d.resize((size_t)n * 3);
    }
    // Frame::ExtractLSD up to and including cullingLine(im, dis, angle, endpoint_dis, .) (Frame.cc:895-934, 952-1116):
    // the extractor's lines with near-collinear segments merged, re-sorted, re-described
    void ExtractLSDCulled(const Image8 &image, std::vector<KeyLine> &keylines, std::vector<uint8_t> &descriptors, std::vector<double> &lineVec2d,
                          double dis = 5, double angle = 2.5, double endpoint_dis = 15)
    {
        keylines.clear(); descriptors.clear(); lineVec2d.clear();
        if (image.empty()) return;
        const int cap = nfeat_ > 0 ? nfeat_ : 1;
        keylines.resize(cap); descriptors.resize((size_t)cap * 32); lineVec2d.resize((size_t)cap * 3);
        int n = 0;
        check(hvo_set_line_culling(ctx_->get(), dis, angle, endpoint_dis), "hvo_set_line_culling");
        check(hvo_extract_lsd_culled(ctx_->get(), image.data, image.width, image.height, image.stride, keylines.data(), descriptors.data(), lineVec2d.data(), cap, &n), "hvo_extract_lsd_culled");
        keylines.resize(n); descriptors.resize((size_t)n * 32); lineVec2d.resize((size_t)n * 3);
    }
    // Frame::isLineGood (Frame.cc:1205-1322): the 3-D line of every key line from the raw depth image; intrinsics and depth factor
    // are the constructor's (setCamera); the reference's time-seeded rand() is an explicit seed here
    void setCamera(float fx, float fy, float cx, float cy, float depthMapFactor)
    {
        hvo_params p; hvo_default_params(&p);
        p.lsd_num_octaves = numOctaves_; p.lsd_scale = scale_; p.lsd_nfeatures = nfeat_; p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.depth_map_factor = depthMapFactor;
        ctx_.reset(new Context(p));
    }
    void isLineGood(const std::vector<KeyLine> &keylines, const Image16 &depth, uint32_t seed, std::vector<hvo_line3d> &lines3d)
    {
        lines3d.assign(keylines.size(), hvo_line3d());
        if (keylines.empty() || depth.empty()) return;
        check(hvo_lines_3d(ctx_->get(), keylines.data(), (int)keylines.size(), depth.data, depth.width, depth.height, depth.stride, seed, lines3d.data()), "hvo_lines_3d");
    }
    // the vanishing-point block of the Frame constructor (Frame.cc:328-337): tmp_vps and local_vp_ids (3 = no structure line)
    hvo_vp_result line2Vps(const std::vector<KeyLine> &keylines, uint32_t seed, std::vector<int32_t> &vp_idx, double thAngle = 1.0 / 180.0 * 3.14159265358979323846)
    {
        hvo_vp_result r; vp_idx.assign(keylines.size(), 3);
        check(hvo_vanishing_points(ctx_->get(), keylines.data(), (int)keylines.size(), seed, thAngle, &r, vp_idx.data(), nullptr), "hvo_vanishing_points");
        return r;
    }
    int GetLevels() const { return numOctaves_; }
    float GetScaleFactor() const { return scale_; }
private:
    int nfeat_, numOctaves_; float scale_;
    std::unique_ptr<Context> ctx_;
};

class PlaneDetection {
public:
    std::vector<std::vector<int>> plane_vertices_;   // vertex indices each plane contains (PlaneExtractor.h:43)
    std::vector<Plane> planes;                        // plane_filter.extractedPlanes (normal, center, mse, N)
    std::vector<int32_t> membership;                  // plane_filter.membershipImg, -1 = none
    int plane_num_ = 0;

    explicit PlaneDetection(int device = 0) : device_(device) {}
    // readDepthImage(depthImg, K, kScaleFactor): CV_16U only (PlaneExtractor.cpp:34-38) -> false otherwise
    bool readDepthImage(const Image16 &depth, float fx, float fy, float cx, float cy, float kScaleFactor)
    {
        if (depth.empty()) return false;
        depth_ = depth;
        if (!ctx_ || fx != fx_ || fy != fy_ || cx != cx_ || cy != cy_ || kScaleFactor != sf_) {
            hvo_params p; hvo_default_params(&p);
            p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy; p.depth_map_factor = kScaleFactor; p.device = device_;
            ctx_.reset(new Context(p));
            fx_ = fx; fy_ = fy; cx_ = cx; cy_ = cy; sf_ = kScaleFactor;
        }
        return true;
    }
    void runPlaneDetection()
    {
        const int w = depth_.width, h = depth_.height;
        membership.assign((size_t)w * h, -1);
        planes.resize(64);
        int n = 0;
        check(hvo_compute_planes(ctx_->get(), depth_.data, w, h, depth_.stride, membership.data(), planes.data(), 64, &n), "hvo_compute_planes");
        planes.resize(n); plane_num_ = n;
        plane_vertices_.assign(n, std::vector<int>());
        for (int i = 0; i < w * h; i++) if (membership[i] >= 0) plane_vertices_[membership[i]].push_back(i);   // raster order, like refineDetails
    }
    // the tail of Frame::ComputePlanes (Frame.cc:2110-2212): per plane the 0.1 m voxel cloud, the distance gate and the RANSAC refit
    // (mvPlanePoints / mvPlaneCoefficients = the entries with valid == 1), and the integral-image surface normals (vSurfaceNormal)
    void planeClouds(double distanceThreshold, std::vector<hvo_plane_cloud> &clouds, std::vector<float> &xyz, int cap = 200000)
    {
        clouds.assign(planes.size(), hvo_plane_cloud()); xyz.assign((size_t)cap * 3, 0.f);
        int total = 0;
        if (!planes.empty())
            check(hvo_plane_clouds(ctx_->get(), depth_.data, depth_.width, depth_.height, depth_.stride, membership.data(), planes.data(), (int)planes.size(),
                                   distanceThreshold, xyz.data(), cap, clouds.data(), &total), "hvo_plane_clouds");
        xyz.resize((size_t)total * 3);
    }
    void surfaceNormals(std::vector<hvo_surface_normal> &normals)
    {
        const int cap = (depth_.height / 3 / 2 + 1) * (depth_.width / 3 / 2 + 1);
        normals.assign(cap, hvo_surface_normal());
        int n = 0;
        check(hvo_surface_normals(ctx_->get(), depth_.data, depth_.width, depth_.height, depth_.stride, normals.data(), cap, &n), "hvo_surface_normals");
        normals.resize(n);
    }
private:
    int device_; Image16 depth_{ nullptr, 0, 0, 0 };
    float fx_ = 0, fy_ = 0, cx_ = 0, cy_ = 0, sf_ = 0;
    std::unique_ptr<Context> ctx_;
};

// Frame post-processing of the extractor outputs: what the Frame constructor does right after
// ExtractORB / ExtractLSD (Frame.cc:231-262): UndistortKeyPoints, ComputeImageBounds, AssignFeaturesToGrid,
// AssignFeaturesToGridForLine.  Grids are CSR (cell = col * 48 + row), see hvo.h.
class FrameGrid {
public:
    static const int COLS = HVO_GRID_COLS, ROWS = HVO_GRID_ROWS;
    explicit FrameGrid(hvo_ctx *ctx) : ctx_(ctx) {}
    void UndistortKeyPoints(const std::vector<KeyPoint> &keys, const float distCoef[5], std::vector<KeyPoint> &keysUn) const
    {
        keysUn.resize(keys.size());
        check(hvo_undistort_keypoints(ctx_, keys.data(), (int)keys.size(), distCoef, keysUn.data()), "hvo_undistort_keypoints");
    }
    void ComputeImageBounds(int cols, int rows, const float distCoef[5], float &mnMinX, float &mnMaxX, float &mnMinY, float &mnMaxY) const
    {
        float b[4]; check(hvo_image_bounds(ctx_, cols, rows, distCoef, b), "hvo_image_bounds");
        mnMinX = b[0]; mnMaxX = b[1]; mnMinY = b[2]; mnMaxY = b[3];
    }
    // mGrid[col][row] == items[start[col*48+row] .. start[col*48+row+1])
    void AssignFeaturesToGrid(const std::vector<KeyPoint> &keysUn, const float bounds[4], std::vector<int> &start, std::vector<int> &items) const
    {
        start.assign(COLS * ROWS + 1, 0); items.assign(keysUn.size() ? keysUn.size() : 1, 0);
        int n = 0;
        check(hvo_assign_features_to_grid(ctx_, keysUn.data(), (int)keysUn.size(), bounds, start.data(), items.data(), &n), "hvo_assign_features_to_grid");
        items.resize(n);
    }
    void AssignFeaturesToGridForLine(const std::vector<KeyLine> &keylines, const float bounds[4], std::vector<int> &start, std::vector<int> &items) const
    {
        start.assign(COLS * ROWS + 1, 0); items.assign(keylines.size() * 128 + 1, 0);
        int n = 0;
        check(hvo_assign_lines_to_grid(ctx_, keylines.data(), (int)keylines.size(), bounds, start.data(), items.data(), (int)items.size(), &n), "hvo_assign_lines_to_grid");
        items.resize(n);
    }
private:
    hvo_ctx *ctx_;
};

class FrameStream;
class ORBVocabulary;
// A candidate key frame as SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) reads it: one entry per feature of
// pKF->GetMapPointMatches() -- GetWorldPos(), the RAW mfMaxDistance / mfMinDistance, GetDescriptor(), mvKeysUn[i].angle.  What the call skips
// (!pMP, isBad(), sAlreadyFound.count(pMP)) is the `skip` argument, a byte per entry; positions of skipped entries are not read.
struct KeyFrameSide {
    int n = 0;
    const float *pos = nullptr, *max_dist = nullptr, *min_dist = nullptr; const uint8_t *desc = nullptr; const float *angle = nullptr;
};
// what the search leaves: per key-frame entry the frame feature it was assigned to (-1: none) and the distance; per frame feature the entry
// that now holds it (-1: none) -- CurrentFrame.mvpMapPoints[i2] = vpMPs[feature_kf[i2]] where feature_kf[i2] >= 0
struct KeyFrameMatches { std::vector<int> match_idx, match_dist, feature_kf; int n_searched = 0; float kernel_ms[2] = { 0.f, 0.f }; };

// What Fuse(pKF, vpMapPoints, th) leaves per key frame: bestIdx / bestDist per entry and the entries with bestDist <= TH_LOW in ascending
// order with their features.  The caller walks fused_entry / fused_idx in order, re-tests `pMP->isBad() || pMP->IsInKeyFrame(pKF)` per entry
// and does Replace (by observation count) or AddObservation + AddMapPoint: the pointer part of ORBmatcher.cc:967-990.
struct FuseMatches {
    std::vector<int> best_idx, best_dist, fused_entry, fused_idx; std::vector<int8_t> gate;
    int n_fused = 0, n_searched = 0; float kernel_ms[3] = { 0.f, 0.f, 0.f };
};

class ORBmatcher {
public:
    static const int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;       // ORBmatcher.cc:37-39
    // Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:838-994) for n_kf key frames on host arrays against ONE map side (the first loop of
    // LocalMapping::SearchInNeighbors, LocalMapping.cc:1596-1603) in one device call.  kf[j].skip: a byte per entry, !pMP || isBad() ||
    // IsInKeyFrame(pKF_j).  Returns the sum of nFused's upper bound (the fused lists' lengths); res gets one FuseMatches per key frame.
    int Fuse(const hvo_camera &cam, const float bounds[4], float bf, const hvo_fuse_map &vpMapPoints, int n_kf, const hvo_fuse_keyframe *kf,
             std::vector<FuseMatches> &res, float th = 3.0f, float logScaleFactor = 0.18232161f, int nLevels = 8) const
    {
        hvo_fuse_params p = fuse_params(bf, th, logScaleFactor, nLevels);
        for (int k = 0; k < 4; k++) p.bounds[k] = bounds[k];
        std::vector<hvo_fuse_result> r((size_t)std::max(n_kf, 1));
        res.assign((size_t)std::max(n_kf, 0), FuseMatches());
        for (int j = 0; j < n_kf; j++) r[j] = fuse_result(res[j], vpMapPoints.n);
        check(hvo_fuse_points(ctx_, &cam, &p, &vpMapPoints, n_kf, kf, r.data()), "hvo_fuse_points");
        int total = 0;
        for (int j = 0; j < n_kf; j++) total += fuse_take(res[j], r[j]);
        return total;
    }
    // Fuse(mpCurrentKeyFrame, vpFuseCandidates) (LocalMapping.cc:1627) with the resident frame `cur` as the key frame under Tcw: its key
    // points, mvuRight and descriptors stay on the device.  The map side is host arrays, or (vpMapPoints == nullptr) n slots of a resident
    // point map.  Valid while the frame is in the ring.
    int Fuse(FrameStream &fs, int64_t cur, const hvo_camera &cam, float bf, const float Tcw[12], const uint8_t *skip, const hvo_fuse_map *vpMapPoints,
             hvo_point_map *map, int n_slots, const int32_t *slots, FuseMatches &res, float th = 3.0f, float logScaleFactor = 0.18232161f, int nLevels = 8) const;
    // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1499-1628), Relocalization's refinement, on the resident
    // frame `cur` under the pose Tcw (rows 0..2 of mTcw): nothing of the frame comes down.  occupied: a byte per frame feature,
    // mvpMapPoints[i2] != NULL at entry (n_features of them).  Returns nmatches; see hvo.h for the three things that set this search apart.
    int SearchByProjection(FrameStream &fs, int64_t cur, const hvo_camera &cam, const float Tcw[12], const KeyFrameSide &kf, const uint8_t *skip,
                           const uint8_t *occupied, int n_features, float th, int ORBdist, KeyFrameMatches &res, bool checkOrientation = true,
                           float logScaleFactor = 0.18232161f, int nLevels = 8) const;
    // the same on host arrays: mvKeysUn, mDescriptors and the image bounds (mnMinX, mnMaxX, mnMinY, mnMaxY) go up with the call
    int SearchByProjection(const hvo_camera &cam, const float bounds[4], const KeyPoint *kp_un, const uint8_t *desc, int n_features, const float Tcw[12],
                           const KeyFrameSide &kf, const uint8_t *skip, const uint8_t *occupied, float th, int ORBdist, KeyFrameMatches &res,
                           bool checkOrientation = true, float logScaleFactor = 0.18232161f, int nLevels = 8) const
    {
        hvo_kf_search_candidate c; hvo_kf_search_params p; hvo_kf_search_result r;
        kf_search_fill(Tcw, kf, skip, occupied, n_features, th, ORBdist, checkOrientation, logScaleFactor, nLevels, res, c, p, r);
        for (int k = 0; k < 4; k++) p.bounds[k] = bounds[k];
        hvo_local_points_frame f = { kp_un, nullptr, desc, n_features };
        check(hvo_search_by_projection_keyframe(ctx_, &cam, &p, &f, 1, &c, &r), "hvo_search_by_projection_keyframe");
        res.n_searched = r.n_searched; res.kernel_ms[0] = r.kernel_ms[0]; res.kernel_ms[1] = r.kernel_ms[1];
        return r.n_matches;
    }
    explicit ORBmatcher(hvo_ctx *ctx) : ctx_(ctx) {}
    // DescriptorDistance(a, b): 32-byte descriptors
    int DescriptorDistance(const uint8_t *a, const uint8_t *b) const
    {
        uint16_t d = 0; check(hvo_hamming_matrix(ctx_, a, 1, b, 1, &d), "hvo_hamming_matrix"); return d;
    }
    // all-pairs distances for the guided searches (nq x nt, row-major)
    void DistanceMatrix(const uint8_t *q, int nq, const uint8_t *t, int nt, std::vector<uint16_t> &d) const
    {
        d.resize((size_t)nq * nt); check(hvo_hamming_matrix(ctx_, q, nq, t, nt, d.data()), "hvo_hamming_matrix");
    }
    // SearchByProjection(CurrentFrame, LastFrame, th, mono) core (ORBmatcher.cc:1353-1497): see hvo.h.
    // Returns the number of matches; match_idx[i] is the current-frame feature of query i or -1.
    int SearchByProjection(const uint8_t *q_desc, int nq, const float *q_u, const float *q_v, const float *q_radius,
                           const int32_t *q_min_level, const int32_t *q_max_level, const float *q_ur, const float *q_angle,
                           const uint8_t *q_blocks, const KeyPoint *t_kp, const float *t_uright, const uint8_t *t_occupied,
                           const uint8_t *t_desc, int nt, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY,
                           bool checkOrientation, std::vector<int> &match_idx) const
    {
        match_idx.assign(nq, -1);
        std::vector<int> dist(nq);
        int n = 0;
        check(hvo_search_by_projection(ctx_, q_desc, nq, q_u, q_v, q_radius, q_min_level, q_max_level, q_ur, q_angle, q_blocks, t_kp, t_uright,
                                       t_occupied, t_desc, nt, mnMinX, mnMinY, mnMaxX, mnMaxY, TH_HIGH, checkOrientation ? 1 : 0,
                                       match_idx.data(), dist.data(), &n), "hvo_search_by_projection");
        return n;
    }
    // SearchByProjection(F, vpMapPoints, th) core (ORBmatcher.cc:45-132): best / second best with the same-octave
    // ratio test (mfNNratio); see hvo.h.  Returns the number of matches.
    int SearchByProjectionMap(const uint8_t *q_desc, int nq, const float *q_u, const float *q_v, const float *q_radius,
                              const int32_t *q_min_level, const int32_t *q_max_level, const float *q_ur, const uint8_t *q_blocks,
                              const KeyPoint *t_kp, const float *t_uright, const uint8_t *t_occupied, const uint8_t *t_desc, int nt,
                              float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, float nnratio, std::vector<int> &match_idx) const
    {
        match_idx.assign(nq, -1);
        std::vector<int> dist(nq);
        int n = 0;
        check(hvo_search_by_projection_map(ctx_, q_desc, nq, q_u, q_v, q_radius, q_min_level, q_max_level, q_ur, q_blocks, t_kp, t_uright,
                                           t_occupied, t_desc, nt, mnMinX, mnMinY, mnMaxX, mnMaxY, TH_HIGH, nnratio,
                                           match_idx.data(), dist.data(), &n), "hvo_search_by_projection_map");
        return n;
    }
    // SearchByProjection(F, vpMapPoints, th) from the tracker's own per-point fields: the window prologue (ORBmatcher.cc:55-70,
    // RadiusByViewingCos 134-140) runs on the device.  One entry per map point with mbTrackInView && !isBad().
    int SearchByProjection(const uint8_t *mp_desc, int nq, const float *mTrackProjX, const float *mTrackProjY, const float *mTrackProjXR,
                           const int32_t *mnTrackScaleLevel, const float *mTrackViewCos, const uint8_t *q_blocks, float th,
                           const KeyPoint *t_kp, const float *t_uright, const uint8_t *t_occupied, const uint8_t *t_desc, int nt,
                           float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, float nnratio, std::vector<int> &match_idx) const
    {
        match_idx.assign(nq, -1);
        std::vector<int> dist(nq);
        int n = 0;
        check(hvo_search_by_projection_tracked(ctx_, mp_desc, nq, mTrackProjX, mTrackProjY, mTrackProjXR, mnTrackScaleLevel, mTrackViewCos, q_blocks, th,
                                               t_kp, t_uright, t_occupied, t_desc, nt, mnMinX, mnMinY, mnMaxX, mnMaxY, TH_HIGH, nnratio,
                                               match_idx.data(), dist.data(), &n), "hvo_search_by_projection_tracked");
        return n;
    }
    // SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:162-293) on host arrays: match_kf[i] is the key-frame feature whose map point frame
    // feature i receives, or -1 (the caller turns it into vpMapPointMatches); the return value is nmatches.  Both sides carry the node ids
    // ComputeBoW returned; the frame's has_map_point is not read.
    int SearchByBoW(const hvo_bow_keyframe &kf, const hvo_bow_keyframe &frame, std::vector<int> &match_kf, float nnratio = 0.7f, bool checkOrientation = true) const
    {
        match_kf.assign((size_t)frame.n, -1);
        hvo_bow_search_params p = { nnratio, checkOrientation ? 1 : 0, TH_LOW };
        hvo_bow_matches r = { match_kf.data(), 0, 0 };
        check(hvo_search_by_bow(ctx_, &frame, 1, &kf, &p, &r), "hvo_search_by_bow");
        return r.n_matches;
    }
private:
    static hvo_fuse_params fuse_params(float bf, float th, float logScaleFactor, int nLevels)
    {
        hvo_fuse_params p = hvo_fuse_params();
        p.th = th; p.th_low = TH_LOW; p.log_scale_factor = logScaleFactor; p.n_levels = nLevels; p.bf = bf;
        return p;
    }
    static hvo_fuse_result fuse_result(FuseMatches &m, int n)
    {
        const size_t k = (size_t)std::max(n, 1);
        m.best_idx.assign(k, -1); m.best_dist.assign(k, 256); m.fused_entry.assign(k, -1); m.fused_idx.assign(k, -1); m.gate.assign(k, 0);
        hvo_fuse_result r = hvo_fuse_result();
        r.best_idx = m.best_idx.data(); r.best_dist = m.best_dist.data(); r.fused_entry = m.fused_entry.data(); r.fused_idx = m.fused_idx.data(); r.gate = m.gate.data();
        return r;
    }
    static int fuse_take(FuseMatches &m, const hvo_fuse_result &r)
    {
        m.n_fused = r.n_fused; m.n_searched = r.n_searched;
        for (int k = 0; k < 3; k++) m.kernel_ms[k] = r.kernel_ms[k];
        m.fused_entry.resize((size_t)r.n_fused); m.fused_idx.resize((size_t)r.n_fused);
        return r.n_fused;
    }
    static void kf_search_fill(const float Tcw[12], const KeyFrameSide &kf, const uint8_t *skip, const uint8_t *occupied, int n_features, float th, int ORBdist,
                               bool checkOrientation, float logScaleFactor, int nLevels, KeyFrameMatches &res, hvo_kf_search_candidate &c,
                               hvo_kf_search_params &p, hvo_kf_search_result &r)
    {
        c = hvo_kf_search_candidate(); p = hvo_kf_search_params(); r = hvo_kf_search_result();
        c.n = kf.n; c.pos = kf.pos; c.skip = skip; c.max_dist = kf.max_dist; c.min_dist = kf.min_dist; c.desc = kf.desc; c.angle = kf.angle; c.occupied = occupied;
        for (int k = 0; k < 12; k++) c.Tcw[k] = Tcw[k];
        p.th = th; p.orb_dist = ORBdist; p.check_orientation = checkOrientation ? 1 : 0; p.log_scale_factor = logScaleFactor; p.n_levels = nLevels;
        res.match_idx.assign((size_t)std::max(kf.n, 1), -1); res.match_dist.assign((size_t)std::max(kf.n, 1), 256); res.feature_kf.assign((size_t)std::max(n_features, 1), -1);
        r.match_idx = res.match_idx.data(); r.match_dist = res.match_dist.data(); r.feature_kf = res.feature_kf.data();
    }
    hvo_ctx *ctx_;
};

// What LocalMapping::CreateNewMapPoints leaves per neighbour: vMatches12 of SearchForTriangulation under the initial occupancy, the outcome of
// every pair (HVO_NP_*), the branch, the point, and -- after the chain over the neighbours is resolved -- the points this neighbour creates in
// ascending idx1.  The caller walks created_idx1 / created_idx2 in order: new MapPoint(x3d[idx1]), AddObservation on both sides, AddMapPoint,
// ComputeDistinctiveDescriptors, UpdateNormalAndDepth, mlpRecentAddedMapPoints (LocalMapping.cc:562-577).
struct NewMapPoints {
    std::vector<int> match_idx2, match_dist, created_idx1, created_idx2; std::vector<int8_t> outcome, branch; std::vector<float> x3d;
    int n_created = 0, gate = 0;
};

// What LocalMapping::CreateNewMapLinesConstraint leaves: per neighbour vMatchedIndices of SearchForTriangulation (-1: none), nlmatch and the gate;
// per pair of searched neighbours the positions that served as key frames (kf2, kf3) and as match vectors (mv2, mv3), the outcome of every
// current line (HVO_NL_*), both end points as far as they were computed and -- after the chain is resolved -- the lines this pair creates in
// ascending ikl.  The caller walks the pairs in order (LocalMapping.cc:1541-1559): new MapLine(line3d[ikl], vManhAxisIdx[ikl]), three
// AddObservation, three AddMapLine, ComputeDistinctiveDescriptors, UpdateAverageDir, mpMap->AddMapLine, mlpRecentAddedMapLines.  A caller
// that saw CheckNewKeyFrames() during the call discards the result.  A context is not thread-safe: the thread that runs this beside
// CreateNewMapPoints has a context of its own.
struct NewMapLineMatches { std::vector<int> match_idx; int n_matched = 0, gate = 0; };
struct NewMapLines {
    int kf2 = -1, kf3 = -1, mv2 = -1, mv3 = -1, n_created = 0;
    std::vector<int8_t> outcome; std::vector<float> line3d; std::vector<int> created_idx0, created_idx1, created_idx2;
};

class LocalMapping {
public:
    explicit LocalMapping(hvo_ctx *ctx) : ctx_(ctx) {}
    // CreateNewMapLinesConstraint (LocalMapping.cc:1064-1565) on host arrays: one device call.  Returns nnew; res has one entry per pair of searched
    // neighbours; owner_pair (may be null) gets the pair that creates the line at ikl, or -1.  nLevels / scale: the LINE pyramid
    int CreateNewMapLinesConstraint(const hvo_nl_keyframe &current, int n_kf, const hvo_nl_keyframe *vpNeighKFs, std::vector<NewMapLineMatches> &matches,
                                    std::vector<NewMapLines> &res, std::vector<int> *owner_pair = nullptr, int pairing = HVO_NL_PAIR_AS_WRITTEN, int nLevels = 8,
                                    float scale = 1.2f, float kernel_ms[3] = nullptr) const
    {
        hvo_nl_params p = { 80, 0.85f, nLevels, scale, pairing };
        std::vector<hvo_nl_match> m; std::vector<hvo_nl_result> r; hvo_nl_summary s = nl_begin(current.n, n_kf, matches, res, m, r, owner_pair);
        check(hvo_create_new_map_lines(ctx_, &p, &current, n_kf, vpNeighKFs, m.data(), (int)r.size(), r.data(), &s), "hvo_create_new_map_lines");
        return nl_end(matches, res, m, r, s, kernel_ms);
    }
    // the resident frame `cur` (either LSD stage) is the current key frame under Tcw: its key lines, line functions and descriptors stay on the
    // device.  n_lines: the number of occupancy bytes given, the frame's line count; the result arrays have the stream's key-line capacity
    // (entries past the frame's count keep their initial values), so a wrong n_lines reads zeros and overruns nothing
    int CreateNewMapLinesConstraint(FrameStream &fs, int64_t cur, const hvo_camera &cam, const float Tcw[12], const uint8_t *has_map_line, int n_lines, int n_kf,
                                    const hvo_nl_keyframe *vpNeighKFs, std::vector<NewMapLineMatches> &matches, std::vector<NewMapLines> &res,
                                    std::vector<int> *owner_pair = nullptr, int pairing = HVO_NL_PAIR_AS_WRITTEN, int nLevels = 8, float scale = 1.2f,
                                    float kernel_ms[3] = nullptr) const;
    // CreateNewMapPoints (LocalMapping.cc:335-580) on host arrays: the current key frame against vpNeighKFs in list order, one device call.
    // A caller that leaves after neighbour i (`if(i>0 && CheckNewKeyFrames()) return;`) walks res[0 .. i] only.  Returns nnew; owner (may be
    // null) gets the neighbour that creates the point at idx1, or -1.
    int CreateNewMapPoints(const hvo_camera &cam, const hvo_np_keyframe &current, int n_kf, const hvo_np_keyframe *vpNeighKFs, std::vector<NewMapPoints> &res,
                           std::vector<int> *owner = nullptr, float mfScaleFactor = 1.2f, int nLevels = 8, float kernel_ms[3] = nullptr) const
    {
        hvo_np_params p = { ORBmatcher::TH_LOW, nLevels, mfScaleFactor, cam.bf };
        std::vector<hvo_np_result> r; hvo_np_summary s = np_begin(current.n, n_kf, res, r, owner);
        check(hvo_create_new_map_points(ctx_, &cam, &p, &current, n_kf, vpNeighKFs, r.data(), &s), "hvo_create_new_map_points");
        return np_end(res, r, s, kernel_ms);
    }
    // the resident frame `cur` is the current key frame under Tcw and carries the bag of words ComputeBoW left on it for voc: its key points,
    // mvuRight, mvDepth, descriptors and node ids stay on the device.  n_features: the frame's feature count (has_map_point has as many bytes)
    int CreateNewMapPoints(FrameStream &fs, int64_t cur, const ORBVocabulary &voc, const hvo_camera &cam, const float Tcw[12], const uint8_t *has_map_point, int n_features,
                           int n_kf, const hvo_np_keyframe *vpNeighKFs, std::vector<NewMapPoints> &res, std::vector<int> *owner = nullptr, float mfScaleFactor = 1.2f,
                           int nLevels = 8, float kernel_ms[3] = nullptr) const;
private:
    static hvo_nl_summary nl_begin(int n1, int n_kf, std::vector<NewMapLineMatches> &matches, std::vector<NewMapLines> &res, std::vector<hvo_nl_match> &m,
                                   std::vector<hvo_nl_result> &r, std::vector<int> *owner_pair)
    {
        const size_t k = (size_t)std::max(n1, 1), nk = (size_t)std::max(n_kf, 0), np = nk * (nk > 0 ? nk - 1 : 0) / 2;
        matches.assign(nk, NewMapLineMatches()); res.assign(np, NewMapLines()); m.assign(std::max<size_t>(nk, 1), hvo_nl_match()); r.assign(std::max<size_t>(np, 1), hvo_nl_result());
        for (size_t j = 0; j < nk; j++) { matches[j].match_idx.assign(k, -1); m[j].match_idx = matches[j].match_idx.data(); }
        for (size_t q = 0; q < np; q++) {
            NewMapLines &x = res[q];
            x.outcome.assign(k, HVO_NL_NO_MATCH); x.line3d.assign(6 * k, 0.f); x.created_idx0.assign(k, -1); x.created_idx1.assign(k, -1); x.created_idx2.assign(k, -1);
            r[q].outcome = x.outcome.data(); r[q].line3d = x.line3d.data();
            r[q].created_idx0 = x.created_idx0.data(); r[q].created_idx1 = x.created_idx1.data(); r[q].created_idx2 = x.created_idx2.data();
        }
        if (np == 0) r.clear();
        hvo_nl_summary s; memset(&s, 0, sizeof(s));
        if (owner_pair) { owner_pair->assign(k, -1); s.owner_pair = owner_pair->data(); }
        return s;
    }
    static int nl_end(std::vector<NewMapLineMatches> &matches, std::vector<NewMapLines> &res, const std::vector<hvo_nl_match> &m, const std::vector<hvo_nl_result> &r,
                      const hvo_nl_summary &s, float kernel_ms[3])
    {
        for (size_t j = 0; j < matches.size(); j++) { matches[j].n_matched = m[j].n_matched; matches[j].gate = m[j].gate; }
        res.resize((size_t)std::max(s.n_pairs, 0));
        for (size_t q = 0; q < res.size(); q++) {
            NewMapLines &x = res[q];
            x.kf2 = r[q].kf2; x.kf3 = r[q].kf3; x.mv2 = r[q].mv2; x.mv3 = r[q].mv3; x.n_created = r[q].n_created;
            x.created_idx0.resize((size_t)x.n_created); x.created_idx1.resize((size_t)x.n_created); x.created_idx2.resize((size_t)x.n_created);
        }
        if (kernel_ms) for (int q = 0; q < 3; q++) kernel_ms[q] = s.kernel_ms[q];
        return s.n_new;
    }
    static hvo_np_summary np_begin(int n1, int n_kf, std::vector<NewMapPoints> &res, std::vector<hvo_np_result> &r, std::vector<int> *owner)
    {
        const size_t k = (size_t)std::max(n1, 1);
        res.assign((size_t)std::max(n_kf, 0), NewMapPoints()); r.assign((size_t)std::max(n_kf, 1), hvo_np_result());
        for (int j = 0; j < n_kf; j++) {
            NewMapPoints &m = res[j];
            m.match_idx2.assign(k, -1); m.match_dist.assign(k, 256); m.created_idx1.assign(k, -1); m.created_idx2.assign(k, -1);
            m.outcome.assign(k, HVO_NP_NO_MATCH); m.branch.assign(k, 0); m.x3d.assign(3 * k, 0.f);
            r[j].match_idx2 = m.match_idx2.data(); r[j].match_dist = m.match_dist.data(); r[j].outcome = m.outcome.data(); r[j].branch = m.branch.data();
            r[j].x3d = m.x3d.data(); r[j].created_idx1 = m.created_idx1.data(); r[j].created_idx2 = m.created_idx2.data();
        }
        hvo_np_summary s = hvo_np_summary();
        if (owner) { owner->assign(k, -1); s.owner = owner->data(); }
        return s;
    }
    static int np_end(std::vector<NewMapPoints> &res, const std::vector<hvo_np_result> &r, const hvo_np_summary &s, float kernel_ms[3])
    {
        for (size_t j = 0; j < res.size(); j++) {
            res[j].n_created = r[j].n_created; res[j].gate = r[j].gate;
            res[j].created_idx1.resize((size_t)r[j].n_created); res[j].created_idx2.resize((size_t)r[j].n_created);
        }
        if (kernel_ms) for (int k = 0; k < 3; k++) kernel_ms[k] = s.kernel_ms[k];
        return s.n_new;
    }
    hvo_ctx *ctx_;
};

// What LSDmatcher::Fuse(pKF, vpMapLines, th) leaves per key frame: bestIdx / bestDist per entry, the entries with bestDist <= TH_LOW in ascending
// order with their key lines, and the entries at which the reference's `return false` (a negative depth) would fire, in ascending order.
struct LineFuseMatches {
    std::vector<int> best_idx, best_dist, fused_entry, fused_idx, behind_entry; std::vector<int8_t> gate;
    int n_fused = 0, n_behind = 0, n_searched = 0; float kernel_ms[3] = { 0.f, 0.f, 0.f };
};
// what a walk did: the fusions made, the behind entry that ended it (-1: none), and whether on_fused reported a Replace.  Within one (key
// frame, list) pair the walk is exact.  Across the key frames of one shared-map call a Replace can change the descriptor of an entry that
// later key frames were already searched with (MapLine::Replace -> ComputeDistinctiveDescriptors on the survivor): a caller that wants the
// sequential result calls Fuse again for the remaining key frames when `replaced` is set.
struct LineFuseWalk { int n_fused = 0, stopped_at = -1; bool replaced = false; };

class LSDmatcher {
public:
    static const int TH_HIGH = 80, TH_LOW = 50;                            // LSDmatcher.cpp:12-14
    // hvo_lf_params for Fuse: th, the key frame's mfLogScaleFactorLine, the levels and factor of mvScaleFactorsLine, HVO_LF_LEVEL_*
    static hvo_lf_params fuseParams(float th = 3.0f, float logScaleFactor = 0.18232161f, int nLevels = 1, float scaleFactor = 1.2f, int levelRule = HVO_LF_LEVEL_CLAMPED)
    {
        hvo_lf_params p = hvo_lf_params();
        p.th = th; p.th_low = TH_LOW; p.log_scale_factor = logScaleFactor; p.n_levels = nLevels; p.scale_factor = scaleFactor; p.level_rule = levelRule;
        return p;
    }
    // Fuse(pKF, vpMapLines, th) (LSDmatcher.cpp:1297-1434) for n_kf key frames on host arrays against ONE map side (LocalMapping.cc:1651) in one
    // device call.  kf[j].desc_rows: the rows the candidates are compared with (mLineDescriptors, or mDescriptors for the text as written);
    // kf[j].skip: a byte per entry, !pML || isBad() || IsInKeyFrame(pKF_j).  Returns the fused lists' total length.
    int Fuse(const hvo_lf_map &vpMapLines, int n_kf, const hvo_lf_keyframe *kf, std::vector<LineFuseMatches> &res, const hvo_lf_params &p = fuseParams()) const
    {
        std::vector<hvo_lf_result> r((size_t)std::max(n_kf, 1));
        res.assign((size_t)std::max(n_kf, 0), LineFuseMatches());
        for (int j = 0; j < n_kf; j++) r[j] = lf_result(res[j], vpMapLines.n);
        hvo_lf_params q = p; q.map_per_keyframe = 0;
        check(hvo_fuse_lines(ctx_, &q, &vpMapLines, n_kf, kf, r.data()), "hvo_fuse_lines");
        int total = 0;
        for (int j = 0; j < n_kf; j++) total += lf_take(res[j], r[j]);
        return total;
    }
    // the map side as n_slots slots of a resident line map (the tracker's, LocalMapping.cc:1677): its arrays are read in place
    int Fuse(hvo_line_map *map, int n_slots, const int32_t *slots, int n_kf, const hvo_lf_keyframe *kf, std::vector<LineFuseMatches> &res, const hvo_lf_params &p = fuseParams()) const
    {
        std::vector<hvo_lf_result> r((size_t)std::max(n_kf, 1));
        res.assign((size_t)std::max(n_kf, 0), LineFuseMatches());
        for (int j = 0; j < n_kf; j++) r[j] = lf_result(res[j], n_slots);
        check(hvo_fuse_lines_slots(ctx_, map, n_slots, slots, &p, n_kf, kf, r.data()), "hvo_fuse_lines_slots");
        int total = 0;
        for (int j = 0; j < n_kf; j++) total += lf_take(res[j], r[j]);
        return total;
    }
    // the resident frame `cur` as the one key frame under Tcw and cam; the map side is host arrays or (vpMapLines == nullptr) slots of a line map
    int Fuse(FrameStream &fs, int64_t cur, const hvo_camera &cam, const float Tcw[12], const uint8_t *skip, const hvo_lf_map *vpMapLines, hvo_line_map *map,
             int n_slots, const int32_t *slots, LineFuseMatches &res, const hvo_lf_params &p = fuseParams()) const;
    // The pointer part of LSDmatcher.cpp:1340-1341 and :1411-1431 for one key frame: the fused and the behind entries merged in entry order.
    // still_skipped(entry): `pML->isBad() || pML->IsInKeyFrame(pKF)` NOW (it only ever turns from "not skipped" to "skipped" during the walk);
    // on_fused(entry, idx) does Replace or AddObservation + AddMapLine and returns true when it called Replace.  stop_on_behind (as written):
    // the walk ends at the first behind entry that is still not skipped when it is reached; false: it continues, as `continue` would have.
    template <class StillSkipped, class OnFused>
    static LineFuseWalk walkFused(const LineFuseMatches &r, bool stop_on_behind, StillSkipped still_skipped, OnFused on_fused)
    {
        LineFuseWalk w;
        size_t f = 0, b = 0;
        const size_t nf = (size_t)std::max(r.n_fused, 0), nb = (size_t)std::max(r.n_behind, 0);
        while (f < nf || b < nb) {
            const bool behind = f >= nf || (b < nb && r.behind_entry[b] < r.fused_entry[f]);      // an entry is in one list at most
            const int e = behind ? r.behind_entry[b] : r.fused_entry[f];
            const int idx = behind ? -1 : r.fused_idx[f];
            if (behind) b++; else f++;
            if (still_skipped(e)) continue;
            if (behind) { if (stop_on_behind) { w.stopped_at = e; break; } continue; }
            if (on_fused(e, idx)) w.replaced = true;
            w.n_fused++;
        }
        return w;
    }
    // FrameBFMatch(ldesc1, ldesc2, LineMatches, TH) (LSDmatcher.cpp:942-966)
    void FrameBFMatch(const uint8_t *ldesc1, int n1, const uint8_t *ldesc2, int n2, std::vector<int> &LineMatches, float TH, float nnratio) const
    {
        LineMatches.assign(n1 > 0 ? n1 : 1, -1); int n = 0;
        check(hvo_frame_bf_match(ctx_, ldesc1, n1, ldesc2, n2, TH, nnratio, LineMatches.data(), &n), "hvo_frame_bf_match");
        LineMatches.resize(n1);
    }
    // SearchDouble(InitialFrame, CurrentFrame, LineMatches) core (LSDmatcher.cpp:902-939): two-way FrameBFMatch at TH_LOW
    int SearchDouble(const uint8_t *ldesc1, int n1, const uint8_t *ldesc2, int n2, std::vector<int> &LineMatches, float nnratio) const
    {
        LineMatches.assign(n1 > 0 ? n1 : 1, -1); int n = 0;
        check(hvo_search_double(ctx_, ldesc1, n1, ldesc2, n2, (float)TH_LOW, nnratio, LineMatches.data(), &n), "hvo_search_double");
        LineMatches.resize(n1);
        return n;
    }
    // LSDmatcher(nnratio = 0.95, checkOri) (include/LSDmatcher.h:23): mfNNratio is read by the local-map SearchByProjection only
    explicit LSDmatcher(hvo_ctx *ctx, float nnratio = 0.95f) : ctx_(ctx), mfNNratio(nnratio) {}
    // int match(desc1, desc2, nnr, matches_12) -> matchNNR (LSDmatcher.cpp:828-863, 803-826)
    int match(const uint8_t *desc1, int n1, const uint8_t *desc2, int n2, float nnr, std::vector<int> &matches_12) const
    {
        matches_12.assign(n1, -1);
        int m = 0;
        check(hvo_match_nnr(ctx_, desc1, n1, desc2, n2, nnr, matches_12.data(), &m), "hvo_match_nnr");
        return m;
    }
    // int SearchByGeomNApearance(CurrentFrame, LastFrame, desc_th, matches_12) (LSDmatcher.cpp:36-108) on host arrays: the descriptor match and the
    // angle / end-point gates; accepted[i1] != 0 where the reference assigns CurrentFrame.mvpMapLines[matches_12[i1]] = LastFrame.mvpMapLines[i1]
    int SearchByGeomNApearance(const uint8_t *ldescLast, const hvo_keyline *klLast, const uint8_t *lastHasMapLine, int nLast,
                               const uint8_t *ldescCur, const hvo_keyline *klCur, int nCur, float desc_th, const float bounds4[4],
                               std::vector<int> &matches_12, std::vector<uint8_t> &accepted) const
    {
        matches_12.assign(nLast > 0 ? nLast : 1, -1); accepted.assign(nLast > 0 ? nLast : 1, 0);
        int n = 0;
        check(hvo_match_lines_geom(ctx_, ldescLast, klLast, lastHasMapLine, nLast, ldescCur, klCur, nCur, desc_th, bounds4, matches_12.data(), accepted.data(), &n), "hvo_match_lines_geom");
        matches_12.resize(nLast); accepted.resize(nLast);
        return n;
    }
    // int SearchByProjection(CurrentFrame, LastFrame, th) core (LSDmatcher.cpp:561-662 over Frame::GetFeaturesInAreaForLine, Frame.cc:1557-1627): one query per
    // last-frame map line in view (its projected end points, its key line, its descriptor, whether it has observations); the current frame's key lines, line
    // functions, descriptors, occupied flags and line grid (hvo::FrameGrid / hvo_assign_lines_to_grid)
    int SearchByProjection(int nq, const float *q_xyxy, const hvo_keyline *q_kl, const uint8_t *q_desc, const uint8_t *q_blocks,
                           const hvo_keyline *t_kl, const double *t_linefn, const uint8_t *t_desc, const uint8_t *t_occupied, int nt,
                           const int32_t *cell_start, const int32_t *cell_items, const float bounds4[4], float th, std::vector<int32_t> &match_idx) const
    {
        match_idx.assign(nq > 0 ? nq : 1, -1); std::vector<int32_t> dist(nq > 0 ? nq : 1, 256);
        int n = 0;
        check(hvo_search_lines_by_projection(ctx_, nq, q_xyxy, q_kl, q_desc, q_blocks, t_kl, t_linefn, t_desc, t_occupied, nt, cell_start, cell_items, bounds4, th,
                                             match_idx.data(), dist.data(), &n), "hvo_search_lines_by_projection");
        match_idx.resize(nq);
        return n;
    }
    // int SearchByProjection(F, vpMapLines, eval_orient, th) (LSDmatcher.cpp:709-801), the local-map line search of Tracking::SearchLocalLines: one
    // query per map line with mbTrackInView && !isBad() (mTrackProjX1/Y1/X2/Y2, mTrackViewCos, GetWorldVector(), GetDescriptor(), Observations() > 0);
    // the current frame's key lines, line functions, 3-D lines (mvLines3D), descriptors, occupied flags and line grid.  eval_orient is not read by
    // the reference and is not taken.  The caller assigns F.mvpMapLines[match_idx[i]] = pML in query order.
    int SearchByProjection(int nq, const float *q_xyxy, const float *q_view_cos, const double *q_wvec, const uint8_t *q_desc, const uint8_t *q_blocks,
                           const hvo_keyline *t_kl, const double *t_linefn, const hvo_line3d *t_l3d, const uint8_t *t_desc, const uint8_t *t_occupied, int nt,
                           const int32_t *cell_start, const int32_t *cell_items, const float bounds4[4], float th, std::vector<int32_t> &match_idx) const
    {
        match_idx.assign(nq > 0 ? nq : 1, -1); std::vector<int32_t> dist(nq > 0 ? nq : 1, 256);
        int n = 0;
        check(hvo_search_lines_by_projection_map(ctx_, nq, q_xyxy, q_view_cos, q_wvec, q_desc, q_blocks, t_kl, t_linefn, t_l3d, t_desc, t_occupied, nt,
                                                 cell_start, cell_items, bounds4, th, mfNNratio, match_idx.data(), dist.data(), &n), "hvo_search_lines_by_projection_map");
        match_idx.resize(nq);
        return n;
    }
private:
    static hvo_lf_result lf_result(LineFuseMatches &m, int n)
    {
        const size_t k = (size_t)std::max(n, 1);
        m.best_idx.assign(k, -1); m.best_dist.assign(k, 256); m.fused_entry.assign(k, -1); m.fused_idx.assign(k, -1); m.behind_entry.assign(k, -1); m.gate.assign(k, 0);
        hvo_lf_result r = hvo_lf_result();
        r.best_idx = m.best_idx.data(); r.best_dist = m.best_dist.data(); r.fused_entry = m.fused_entry.data(); r.fused_idx = m.fused_idx.data();
        r.behind_entry = m.behind_entry.data(); r.gate = m.gate.data();
        return r;
    }
    static int lf_take(LineFuseMatches &m, const hvo_lf_result &r)
    {
        m.n_fused = r.n_fused; m.n_behind = r.n_behind; m.n_searched = r.n_searched;
        for (int k = 0; k < 3; k++) m.kernel_ms[k] = r.kernel_ms[k];
        m.fused_entry.resize((size_t)r.n_fused); m.fused_idx.resize((size_t)r.n_fused); m.behind_entry.resize((size_t)r.n_behind);
        return r.n_fused;
    }
    hvo_ctx *ctx_;
    float mfNNratio;
};


// One camera, one frame at a time (Tracking.cc:262 -> Frame.cc:205-233, then the matching of Tracking.cc:2299 / 2396): a ring of
// frames in flight whose results stay on the device for matching against the previous frame (hvo_stream_*, see hvo.h).
class FrameStream {
public:
    FrameStream(const hvo_params &p, const hvo_stream_params &sp)
    {
        check(hvo_stream_create(&p, &sp, &s_), "hvo_stream_create");
        check(hvo_stream_capacity(s_, &kp_cap_, &kl_cap_, &pl_cap_), "hvo_stream_capacity");
    }
    ~FrameStream() { if (s_) hvo_stream_destroy(s_); }
    FrameStream(const FrameStream &) = delete;
    FrameStream &operator=(const FrameStream &) = delete;
    int64_t submit(const Image8 &gray, const Image16 &depth)
    {
        int64_t t = -1;
        check(hvo_stream_submit(s_, gray.data, gray.stride, depth.data, depth.stride, &t), "hvo_stream_submit");
        return t;
    }
    bool done(int64_t ticket) { const int r = hvo_stream_poll(s_, ticket); if (r < 0) throw Error(r, "hvo_stream_poll"); return r == 1; }
    // waits for the frame; any pointer of out may be null (hvo_batch_download's conventions)
    void collect(int64_t ticket, hvo_frame_out &out, hvo_keypoint *kp_un = nullptr, float *uright = nullptr, float *zdepth = nullptr)
    {
        check(hvo_stream_collect(s_, ticket, &out, kp_un, uright, zdepth), "hvo_stream_collect");
    }
    // The rest of the Frame constructor (HVO_STAGE_LINES3D / _VP / _PLANE_TAIL / _GRIDS in hvo_stream_params.stages): isLineGood's 3-D
    // lines, the vanishing points and line2Vps clusters, mvPlanePoints / mvPlaneCoefficients / vSurfaceNormal, the two 64 x 48 grids.
    // Call before collect() releases the slot.  FrameTail owns its arrays, sized from the stream's capacities.
    struct FrameTail {
        std::vector<hvo_line3d> lines3d; hvo_vp_result vp{}; std::vector<int32_t> vp_idx;
        std::vector<hvo_plane_cloud> plane_clouds; std::vector<float> cloud_xyz; std::vector<hvo_surface_normal> normals;
        std::vector<int32_t> pt_cell_start, pt_cell_items, ln_cell_start, ln_cell_items;
        hvo_frame_tail c{};
    };
    void collectTail(int64_t ticket, int w, int h, FrameTail &t)
    {
        int cc = 0, nn = 0, lc = 0;
        check(hvo_tail_capacity(kl_cap_, w, h, &cc, &nn, &lc), "hvo_tail_capacity");
        t.lines3d.resize(kl_cap_); t.vp_idx.assign(kl_cap_, 3); t.plane_clouds.resize(64); t.cloud_xyz.resize(3 * (size_t)cc); t.normals.resize(nn > 0 ? nn : 1);
        t.pt_cell_start.resize(HVO_GRID_COLS * HVO_GRID_ROWS + 1); t.pt_cell_items.resize(kp_cap_ > 0 ? kp_cap_ : 1);
        t.ln_cell_start.resize(HVO_GRID_COLS * HVO_GRID_ROWS + 1); t.ln_cell_items.resize(lc > 0 ? lc : 1);
        hvo_frame_tail &c = t.c;
        c.lines3d = t.lines3d.data(); c.vp = &t.vp; c.vp_idx = t.vp_idx.data(); c.plane_clouds = t.plane_clouds.data(); c.cloud_xyz = t.cloud_xyz.data(); c.cloud_cap = cc;
        c.normals = t.normals.data(); c.normals_cap = nn; c.pt_cell_start = t.pt_cell_start.data(); c.pt_cell_items = t.pt_cell_items.data(); c.pt_items_cap = kp_cap_;
        c.ln_cell_start = t.ln_cell_start.data(); c.ln_cell_items = t.ln_cell_items.data(); c.ln_items_cap = lc;
        check(hvo_stream_collect_tail(s_, ticket, &c), "hvo_stream_collect_tail");
    }
    // ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) whole (ORBmatcher.cc:1353-1497) between two resident frames: the
    // projection prologue (1364-1405) and the search core on the device.  Tcw / Tlw: rows 0..2 of the frames' mTcw (row-major 3 x 4);
    // q_index[i] = last-frame feature whose map point (no outlier) has world position x3Dw[3 i ..].  Returns the number of matches.
    int SearchByProjection(int64_t cur, int64_t last, const hvo_camera &cam, const float *Tcw, const float *Tlw, int nq, const int32_t *q_index,
                           const float *x3Dw, const uint8_t *q_blocks, const uint8_t *t_occupied, float th, bool bMono, bool checkOrientation,
                           std::vector<int32_t> &match_idx)
    {
        match_idx.assign(nq, -1);
        std::vector<int32_t> dist(nq > 0 ? nq : 1);
        int n = 0;
        check(hvo_stream_project_last(s_, cur, last, &cam, Tcw, Tlw, nq, q_index, x3Dw, q_blocks, nullptr, t_occupied, th, bMono ? 1 : 0, 100,
                                      checkOrientation ? 1 : 0, match_idx.data(), dist.data(), &n, nullptr), "hvo_stream_project_last");
        return n;
    }
    // LSDmatcher::match / FrameBFMatch / SearchDouble between two resident frames (mode = HVO_LINE_MATCH_*)
    int matchLines(int64_t from, int64_t to, int mode, float th, float nnratio, std::vector<int32_t> &matches12)
    {
        matches12.assign(kl_cap_, -1);
        int nfrom = 0, nm = 0;
        check(hvo_stream_match_lines(s_, from, to, mode, th, nnratio, matches12.data(), &nfrom, &nm), "hvo_stream_match_lines");
        matches12.resize(nfrom);
        return nm;
    }
    // LSDmatcher::SearchByGeomNApearance(Cur, Last, desc_th, matches_12) whole between two resident frames (LSDmatcher.cpp:36-108)
    int searchByGeomNApearance(int64_t cur, int64_t last, float desc_th, const uint8_t *lastHasMapLine, std::vector<int32_t> &matches12, std::vector<uint8_t> &accepted)
    {
        matches12.assign(kl_cap_, -1); accepted.assign(kl_cap_, 0);
        int nlast = 0, nm = 0;
        check(hvo_stream_match_lines_geom(s_, cur, last, desc_th, lastHasMapLine, matches12.data(), accepted.data(), &nlast, &nm), "hvo_stream_match_lines_geom");
        matches12.resize(nlast); accepted.resize(nlast);
        return nm;
    }
    // LSDmatcher::SearchByProjection(Cur, Last, th) core between two resident frames (LSDmatcher.cpp:561-662); the stream must run HVO_STAGE_GRIDS
    int searchLinesByProjection(int64_t cur, int64_t last, const std::vector<int32_t> &q_index, const std::vector<float> &q_xyxy, const uint8_t *q_desc,
                                const uint8_t *q_blocks, const uint8_t *t_occupied, float th, std::vector<int32_t> &match_idx)
    {
        const int nq = (int)q_index.size();
        match_idx.assign(nq > 0 ? nq : 1, -1); std::vector<int32_t> dist(nq > 0 ? nq : 1, 256);
        int n = 0;
        check(hvo_stream_search_lines_by_projection(s_, cur, last, nq, q_index.data(), q_xyxy.data(), q_desc, q_blocks, t_occupied, th, match_idx.data(), dist.data(), &n),
              "hvo_stream_search_lines_by_projection");
        match_idx.resize(nq);
        return n;
    }
    // Tracking::SearchLocalLines' matcher.SearchByProjection(mCurrentFrame, mvpLocalMapLines, eval_orient, th) (Tracking.cc:3279-3355 ->
    // LSDmatcher.cpp:709-801) on the resident frame `cur`: per query the map line's fields as in LSDmatcher::SearchByProjection above; the frame's lines,
    // line grid and 3-D lines stay on the device.  The stream must run HVO_STAGE_GRIDS | HVO_STAGE_LINES3D and the frame must come with depth.
    int searchLocalLines(int64_t cur, int nq, const float *q_xyxy, const float *q_view_cos, const double *q_wvec, const uint8_t *q_desc, const uint8_t *q_blocks,
                         const uint8_t *t_occupied, float th, std::vector<int32_t> &match_idx, float nnratio = 0.95f)
    {
        match_idx.assign(nq > 0 ? nq : 1, -1); std::vector<int32_t> dist(nq > 0 ? nq : 1, 256);
        int n = 0;
        check(hvo_stream_search_lines_by_projection_map(s_, cur, nq, q_xyxy, q_view_cos, q_wvec, q_desc, q_blocks, t_occupied, th, nnratio,
                                                        match_idx.data(), dist.data(), &n), "hvo_stream_search_lines_by_projection_map");
        match_idx.resize(nq);
        return n;
    }
    // Tracking::TrackManhattanFrame(mLastRcm, mCurrentFrame.vSurfaceNormal, mCurrentFrame.mVF3DLines) (Tracking.cc:1172-1348) on the resident
    // frame `cur`: its normals and 3-D lines stay on the device.  The stream must run HVO_STAGE_PLANE_TAIL | HVO_STAGE_LINES3D.  Call before
    // collect() releases the slot.  normal_axes / line_axes (optional): n_normals / klCap() entries.
    hvo_mf_result trackManhattanFrame(int64_t cur, const float R_last[9], uint8_t *normal_axes = nullptr, uint8_t *line_axes = nullptr)
    {
        hvo_mf_result r;
        check(hvo_stream_track_manhattan(s_, cur, R_last, &r, normal_axes, line_axes), "hvo_stream_track_manhattan");
        return r;
    }
    void setReadings(unsigned mask) { check(hvo_stream_set_readings(s_, mask), "hvo_stream_set_readings"); }
    hvo_stream *get() const { return s_; }
    int kpCap() const { return kp_cap_; } int klCap() const { return kl_cap_; } int plCap() const { return pl_cap_; }
private:
    hvo_stream *s_ = nullptr; int kp_cap_ = 0, kl_cap_ = 0, pl_cap_ = 0;
};

// The Manhattan-frame part of Tracking (src/Tracking.cc:706-718 and 1172-1348): it keeps mLastRcm and threads it through the per-frame calls,
// MF_can = TrackManhattanFrame(mLastRcm, vSurfaceNormal, mVF3DLines); MF_can.copyTo(mLastRcm).  The caller seeds mLastRcm with the
// initialisation's Rotation_cm (Map::FindManhattan, which stays on the host) and forms mRotation_wc = (Rotation_cm * MF_can^T)^T itself.
class ManhattanTracking {
public:
    ManhattanTracking(hvo_ctx *ctx, const float R_init[9]) : ctx_(ctx) { for (int i = 0; i < 9; i++) mLastRcm[i] = R_init[i]; }
    // on host arrays: vSurfaceNormal (NaN ones included) and hvo_lines_3d of every key line (the good ones are mVF3DLines)
    hvo_mf_result TrackManhattanFrame(const hvo_surface_normal *normals, int n_normals, const hvo_line3d *l3d, int n_lines)
    {
        hvo_mf_result r;
        check(hvo_track_manhattan(ctx_, normals, n_normals, l3d, n_lines, mLastRcm, &r, nullptr, nullptr), "hvo_track_manhattan");
        for (int i = 0; i < 9; i++) mLastRcm[i] = r.R[i];
        return r;
    }
    // on the resident frame `cur` of a stream
    hvo_mf_result TrackManhattanFrame(FrameStream &fs, int64_t cur)
    {
        const hvo_mf_result r = fs.trackManhattanFrame(cur, mLastRcm);
        for (int i = 0; i < 9; i++) mLastRcm[i] = r.R[i];
        return r;
    }
    float mLastRcm[9];          // R_cm of the last frame, row-major
private:
    hvo_ctx *ctx_;
};

// The map's planes resident on one device (hvo_plane_map): per slot GetWorldPos(), isBad() and mvPlanePoints' xyz.  The slot index is the
// position in the vector PlaneMatcher::SearchMapByCoefficients would have received (mpMap->GetAllMapPlanes()).  The local mapper calls set()
// where a cloud is made on the host (MapPlane::Replace, the local mapper's multi-observation update) and setBad() where SetBadFlag runs.
// MapPlane::UpdateCoefficientsAndPoints, both overloads as Tracking calls them, runs on the device: UpdateCoefficientsAndPoints() / insert().
// Not thread-safe.
class PlaneMap {
public:
    explicit PlaneMap(int device = 0, int slots = 0, int64_t points = 0) : m_(hvo_plane_map_create(device, slots, points))
    {
        if (!m_) throw Error(HVO_ERR_HIP, "hvo_plane_map_create");
    }
    ~PlaneMap() { hvo_plane_map_destroy(m_); }
    PlaneMap(const PlaneMap &) = delete;
    PlaneMap &operator=(const PlaneMap &) = delete;
    void set(int slot, const float coef[4], const float *xyz, int n_points) { check(hvo_plane_map_set(m_, slot, coef, xyz, n_points), "hvo_plane_map_set"); }
    void setBad(int slot, bool bad = true) { check(hvo_plane_map_set_bad(m_, slot, bad ? 1 : 0), "hvo_plane_map_set_bad"); }
    int size() const { int n = 0; check(hvo_plane_map_counts(m_, &n, nullptr, nullptr), "hvo_plane_map_counts"); return n; }
    int64_t points() const { int64_t n = 0; check(hvo_plane_map_counts(m_, nullptr, nullptr, &n), "hvo_plane_map_counts"); return n; }
    // mvPlanePoints of one slot as n x 3 floats (a viewer's read-back: nothing else needs the cloud on the host)
    std::vector<float> points(int slot) const
    {
        int n = 0;
        check(hvo_plane_map_slot(m_, slot, nullptr, &n, nullptr), "hvo_plane_map_slot");
        std::vector<float> xyz(3 * (size_t)n);
        check(hvo_plane_map_get_points(m_, slot, n ? xyz.data() : nullptr, n, &n), "hvo_plane_map_get_points");
        return xyz;
    }
    // The loop of Tracking::Track() after the pose is known (src/Tracking.cc:796-804):
    //   for i < mnPlaneNum: if mvpMapPlanes[i]: UpdateCoefficientsAndPoints(mCurrentFrame, i)   else if !mvbPlaneOutlier[i]: newPlane = true
    // match: the association's result for that frame.  outlier: mvbPlaneOutlier, the flag of frame plane i at outlier[i * outlier_stride]
    // (null = no plane is an outlier).  A tracker's own mvbPlaneOutlier is one byte per plane: stride 1.  The pose optimiser writes
    // hvo_pose_flags.pl_outlier as n_planes x 3 bytes, per plane [mvbPlaneOutlier, mvbParPlaneOutlier, mvbVerPlaneOutlier]: pass that
    // buffer with outlier_stride = kPoseFlagsPlaneStride, and only the first byte of each triple is read.
    // Matched planes are updated whether or not they are outliers, as in the reference.
    static const int kPoseFlagsPlaneStride = 3;
    // the list of that loop alone (host only): the MERGE operations in `u`, the reference's flag in newPlane
    static void trackUpdateList(const hvo_plane_match &match, const uint8_t *outlier, int outlier_stride, hvo_plane_update &u, bool &newPlane)
    {
        u = hvo_plane_update();
        newPlane = false;
        for (int i = 0; i < match.n_planes && i < 64; i++) {
            if (match.match[i] >= 0) { u.plane[u.n] = i; u.slot[u.n] = match.match[i]; u.op[u.n] = HVO_PLANE_UPDATE_MERGE; u.n++; }
            else if (!outlier || !outlier[(size_t)i * outlier_stride]) newPlane = true;
        }
    }
    // the loop on the resident frame `cur`; returns the operations done
    int UpdateCoefficientsAndPoints(FrameStream &fs, int64_t cur, const float Tcw[12], const hvo_plane_match &match, const uint8_t *outlier, bool &newPlane,
                                    int outlier_stride = 1, hvo_plane_update_result *result = nullptr)
    {
        if (outlier_stride < 1) throw Error(HVO_ERR_INVALID_ARG, "PlaneMap::UpdateCoefficientsAndPoints: outlier_stride < 1");
        hvo_plane_update u;
        trackUpdateList(match, outlier, outlier_stride, u, newPlane);
        hvo_plane_update_result r;
        check(hvo_stream_update_map_planes(fs.get(), m_, cur, Tcw, nullptr, &u, &r), "hvo_stream_update_map_planes");
        if (result) *result = r;
        return r.n_done;
    }
    // CreateNewKeyFrame / StereoInitialization (src/Tracking.cc:3208-3213, :1407): new MapPlane(ComputePlaneWorldCoeff(i), pKF, i) and its
    // UpdateCoefficientsAndPoints() for frame plane i of the resident frame `cur`, into `slot` (size() appends).  Twc: GetPoseInverse().
    // Returns the points of the new cloud, or -1 when the operation was refused.
    int insert(FrameStream &fs, int64_t cur, const float Tcw[12], const float Twc[12], int plane, int slot)
    {
        hvo_plane_update u = hvo_plane_update();
        u.n = 1; u.plane[0] = plane; u.slot[0] = slot; u.op[0] = HVO_PLANE_UPDATE_INSERT;
        hvo_plane_update_result r;
        check(hvo_stream_update_map_planes(fs.get(), m_, cur, Tcw, Twc, &u, &r), "hvo_stream_update_map_planes");
        return r.status[0] == HVO_OK ? r.n_after[0] : -1;
    }
    hvo_plane_map *get() const { return m_; }
private:
    hvo_plane_map *m_;
};

// PlaneMatcher (include/PlaneMatcher.h, src/PlaneMatcher.cpp): the constructor's four thresholds and SearchMapByCoefficients over a resident
// PlaneMap.  The result's match / vertical / parallel hold slot indices where the reference fills mvpMapPlanes / mvpVerticalPlanes /
// mvpParallelPlanes (-1: left NULL); the return value of the reference is res.n_matches.
class PlaneMatcher {
public:
    PlaneMatcher(float dTh = 0.1f, float aTh = 0.86f, float verTh = 0.08716f, float parTh = 0.9962f) { th_[0] = dTh; th_[1] = aTh; th_[2] = verTh; th_[3] = parTh; }
    // on host arrays: mvPlaneCoefficients (n x 4 floats, n <= 64) and rows 0..2 of mTcw
    int SearchMapByCoefficients(hvo_ctx *ctx, const float *coef, int n, const float Tcw[12], const PlaneMap &map, hvo_plane_match &res) const
    {
        check(hvo_match_planes(ctx, map.get(), coef, n, Tcw, th_, &res, nullptr, nullptr), "hvo_match_planes");
        return res.n_matches;
    }
    // on the resident frame `cur` of a stream (HVO_STAGE_PLANE_TAIL); call before collect() releases the slot
    int SearchMapByCoefficients(FrameStream &fs, int64_t cur, const float Tcw[12], const PlaneMap &map, hvo_plane_match &res) const
    {
        check(hvo_stream_match_planes(fs.get(), map.get(), cur, Tcw, th_, &res), "hvo_stream_match_planes");
        return res.n_matches;
    }
private:
    float th_[4];
};

namespace detail {
// What LineMap and PointMap share: the ownership of the handle, get() and lastError().
template <class M, void (*Destroy)(M *), const char *(*LastError)(const M *)>
class SlotMapHandle {
public:
    ~SlotMapHandle() { Destroy(m_); }
    SlotMapHandle(const SlotMapHandle &) = delete;
    SlotMapHandle &operator=(const SlotMapHandle &) = delete;
    const char *lastError() const { return LastError(m_); }
    M *get() const { return m_; }
protected:
    SlotMapHandle(M *m, const char *what) : m_(m) { if (!m_) throw Error(HVO_ERR_HIP, what); }
    M *m_;
};
}  // namespace detail

// The local map's lines resident on one device (hvo_line_map): per slot GetWorldPos(), GetWorldVector(), GetNormal(), mfMaxDistance,
// mfMinDistance, GetDescriptor(), isBad() and Observations() > 0.  The slot index is the position in mvpLocalMapLines: the tracker calls
// setMany() after UpdateLocalLines has rebuilt that vector.  Not thread-safe.
class LineMap : public detail::SlotMapHandle<hvo_line_map, hvo_line_map_destroy, hvo_line_map_last_error> {
public:
    explicit LineMap(int device = 0, int slots = 0) : SlotMapHandle(hvo_line_map_create(device, slots), "hvo_line_map_create") {}
    void set(int slot, const double pos[6], const double wvec[3], const double normal[3], float maxDistance, float minDistance, const uint8_t desc[32], bool observed = true)
    {
        check(hvo_line_map_set(m_, slot, pos, wvec, normal, maxDistance, minDistance, desc, observed ? 1 : 0), "hvo_line_map_set");
    }
    void setMany(int first, int n, const double *pos, const double *wvec, const double *normal, const float *maxDistance, const float *minDistance,
                 const uint8_t *desc, const uint8_t *observed = nullptr, const uint8_t *bad = nullptr)
    {
        check(hvo_line_map_set_many(m_, first, n, pos, wvec, normal, maxDistance, minDistance, desc, observed, bad), "hvo_line_map_set_many");
    }
    void setBad(int slot, bool bad = true) { check(hvo_line_map_set_bad(m_, slot, bad ? 1 : 0), "hvo_line_map_set_bad"); }
    void setObserved(int slot, bool observed = true) { check(hvo_line_map_set_observed(m_, slot, observed ? 1 : 0), "hvo_line_map_set_observed"); }
    int size() const { int n = 0; check(hvo_line_map_counts(m_, &n, nullptr, nullptr), "hvo_line_map_counts"); return n; }
    // MapLine::ComputeDistinctiveDescriptors + UpdateAverageDir (src/MapLine.cpp:331-396, 404-455) on in.n slots: descriptor, normal, world
    // vector and distance range are rewritten in place from the observations; `what`: HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY (the optimiser
    // passes HVO_MR_GEOMETRY alone).  nLevels / scale: the LINE pyramid.  out's pointers may be null; returns the kernel's device ms
    float refresh(hvo_ctx *ctx, const int32_t *slots, const hvo_mr_input &in, hvo_mr_line_out &out, int what = HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY, int nLevels = 8,
                  float scale = 1.2f)
    {
        const hvo_mr_params p = { nLevels, scale, what };
        check(hvo_line_map_refresh(ctx, m_, slots, &p, &in, &out), "hvo_line_map_refresh");
        return out.kernel_ms;
    }
};

// Tracking::SearchLocalLines (src/Tracking.cc:3279-3392) together with Manhattan::computeStructConstInMap (src/Manhattan.cpp:163-224) over a
// resident LineMap: io.held carries mvpMapLines as slots in and out, io.in_view_slot returns mvpLocalMapLines_InFrustum; the return value
// is SearchByProjection's nmatches.  th: 1, or 5 right after a relocalisation.
class LocalLines {
public:
    LocalLines(const hvo_camera &cam, float logScaleFactor, float nnratio = 0.95f) : cam_(cam) { p_ = hvo_local_lines_params(); p_.log_scale_factor = logScaleFactor; p_.nn_ratio = nnratio; }
    // on host arrays; bounds4 = mnMinX, mnMaxX, mnMinY, mnMaxY
    int SearchLocalLines(hvo_ctx *ctx, const LineMap &map, const float Tcw[12], const float bounds4[4], const hvo_local_lines_frame &frame, hvo_local_lines_io &io,
                         hvo_local_lines_result &res, float th = 1.0f) const
    {
        hvo_local_lines_params p = p_; p.th = th;
        for (int k = 0; k < 4; k++) p.bounds[k] = bounds4[k];
        check(hvo_search_local_lines(ctx, map.get(), &cam_, Tcw, &p, &frame, &io, &res), "hvo_search_local_lines");
        return res.n_matches;
    }
    // on the resident frame `cur` of a stream (an LSD stage, HVO_STAGE_GRIDS, HVO_STAGE_LINES3D, depth); call before collect() releases the slot
    int SearchLocalLines(FrameStream &fs, int64_t cur, const LineMap &map, const float Tcw[12], hvo_local_lines_io &io, hvo_local_lines_result &res, float th = 1.0f) const
    {
        hvo_local_lines_params p = p_; p.th = th;
        check(hvo_stream_search_local_lines(fs.get(), map.get(), cur, &cam_, Tcw, &p, &io, &res), "hvo_stream_search_local_lines");
        return res.n_matches;
    }
    // on the first n frames of the context's resident batch, frame k under Tcw + 12 k with io[k] / res[k]
    void SearchLocalLinesBatch(hvo_ctx *ctx, const LineMap &map, int n, const float *Tcw, hvo_local_lines_io *io, hvo_local_lines_result *res, float th = 1.0f) const
    {
        hvo_local_lines_params p = p_; p.th = th;
        check(hvo_batch_search_local_lines(ctx, map.get(), n, &cam_, Tcw, &p, io, res), "hvo_batch_search_local_lines");
    }
private:
    hvo_camera cam_; hvo_local_lines_params p_;
};

// The local map's points resident on one device (hvo_point_map): per slot GetWorldPos(), GetNormal(), mfMaxDistance, mfMinDistance,
// GetDescriptor(), isBad() and Observations() > 0.  The slot index is the position in mvpLocalMapPoints: the tracker calls setMany() after
// UpdateLocalPoints has rebuilt that vector.  Not thread-safe.
class PointMap : public detail::SlotMapHandle<hvo_point_map, hvo_point_map_destroy, hvo_point_map_last_error> {
public:
    explicit PointMap(int device = 0, int slots = 0) : SlotMapHandle(hvo_point_map_create(device, slots), "hvo_point_map_create") {}
    void set(int slot, const float pos[3], const float normal[3], float maxDistance, float minDistance, const uint8_t desc[32], bool observed = true)
    {
        check(hvo_point_map_set(m_, slot, pos, normal, maxDistance, minDistance, desc, observed ? 1 : 0), "hvo_point_map_set");
    }
    void setMany(int first, int n, const float *pos, const float *normal, const float *maxDistance, const float *minDistance, const uint8_t *desc,
                 const uint8_t *observed = nullptr, const uint8_t *bad = nullptr)
    {
        check(hvo_point_map_set_many(m_, first, n, pos, normal, maxDistance, minDistance, desc, observed, bad), "hvo_point_map_set_many");
    }
    void setBad(int slot, bool bad = true) { check(hvo_point_map_set_bad(m_, slot, bad ? 1 : 0), "hvo_point_map_set_bad"); }
    void setObserved(int slot, bool observed = true) { check(hvo_point_map_set_observed(m_, slot, observed ? 1 : 0), "hvo_point_map_set_observed"); }
    int size() const { int n = 0; check(hvo_point_map_counts(m_, &n, nullptr, nullptr), "hvo_point_map_counts"); return n; }
    // MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (src/MapPoint.cc:240-305, 328-369) on in.n slots: descriptor, normal and
    // distance range are rewritten in place from the observations; the scale table is the context's.  Returns the kernel's device ms
    float refresh(hvo_ctx *ctx, const int32_t *slots, const hvo_mr_input &in, hvo_mr_point_out &out, int what = HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY, int nLevels = 8)
    {
        const hvo_mr_params p = { nLevels, 1.2f, what };
        check(hvo_point_map_refresh(ctx, m_, slots, &p, &in, &out), "hvo_point_map_refresh");
        return out.kernel_ms;
    }
};

// the same two sweeps on host arrays: pos is in.n x 3 floats (mWorldPos) / in.n x 6 doubles (start and end point).  An entry of `out` that a
// feature's status (HVO_MR_*) says was not written keeps what the caller put there
inline float refreshMapPoints(hvo_ctx *ctx, const hvo_mr_input &in, const float *pos, hvo_mr_point_out &out, int what = HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY, int nLevels = 8)
{
    const hvo_mr_params p = { nLevels, 1.2f, what };
    check(hvo_refresh_map_points(ctx, &p, &in, pos, &out), "hvo_refresh_map_points");
    return out.kernel_ms;
}
inline float refreshMapLines(hvo_ctx *ctx, const hvo_mr_input &in, const double *pos, hvo_mr_line_out &out, int what = HVO_MR_DESCRIPTOR | HVO_MR_GEOMETRY, int nLevels = 8,
                             float scale = 1.2f)
{
    const hvo_mr_params p = { nLevels, scale, what };
    check(hvo_refresh_map_lines(ctx, &p, &in, pos, &out), "hvo_refresh_map_lines");
    return out.kernel_ms;
}

// Tracking::SearchLocalPoints (src/Tracking.cc:3227-3277) over a resident PointMap: io.held carries mvpMapPoints as slots (or -1,
// HVO_HELD_FOREIGN_OBSERVED, HVO_HELD_FOREIGN_UNOBSERVED) in and out, io.in_view_slot returns the points with mbTrackInView; the return value
// is SearchByProjection's nmatches.  th: 1, 3 for RGB-D, 5 right after a relocalisation.
class LocalPoints {
public:
    LocalPoints(const hvo_camera &cam, float logScaleFactor, int nLevels, float nnratio = 0.8f) : cam_(cam)
    {
        p_ = hvo_local_points_params(); p_.log_scale_factor = logScaleFactor; p_.n_levels = nLevels; p_.bf = cam.bf; p_.th_high = 100; p_.nn_ratio = nnratio;
        p_.view_cos_limit = 0.5f;
    }
    // on host arrays; bounds4 = mnMinX, mnMaxX, mnMinY, mnMaxY
    int SearchLocalPoints(hvo_ctx *ctx, const PointMap &map, const float Tcw[12], const float bounds4[4], const hvo_local_points_frame &frame, hvo_local_points_io &io,
                          hvo_local_points_result &res, float th = 1.0f) const
    {
        hvo_local_points_params p = p_; p.th = th;
        for (int k = 0; k < 4; k++) p.bounds[k] = bounds4[k];
        check(hvo_search_local_points(ctx, map.get(), &cam_, Tcw, &p, &frame, &io, &res), "hvo_search_local_points");
        return res.n_matches;
    }
    // on the resident frame `cur` of a stream (HVO_STAGE_ORB); the slot stays resident until `depth` newer frames were submitted
    int SearchLocalPoints(FrameStream &fs, int64_t cur, const PointMap &map, const float Tcw[12], hvo_local_points_io &io, hvo_local_points_result &res, float th = 1.0f) const
    {
        hvo_local_points_params p = p_; p.th = th;
        check(hvo_stream_search_local_points(fs.get(), map.get(), cur, &cam_, Tcw, &p, &io, &res), "hvo_stream_search_local_points");
        return res.n_matches;
    }
    // on the first n frames of the context's resident batch, frame k under Tcw + 12 k with io[k] / res[k]
    void SearchLocalPointsBatch(hvo_ctx *ctx, const PointMap &map, int n, const float *Tcw, hvo_local_points_io *io, hvo_local_points_result *res, float th = 1.0f) const
    {
        hvo_local_points_params p = p_; p.th = th;
        check(hvo_batch_search_local_points(ctx, map.get(), n, &cam_, Tcw, &p, io, res), "hvo_batch_search_local_points");
    }
private:
    hvo_camera cam_; hvo_local_points_params p_;
};

// The map-making steps of Tracking over the resident maps (hvo_kf_insert, csrc/new_keyframe.hip): the new map points and map lines of
// CreateNewKeyFrame (src/Tracking.cc:3032-3187), of StereoInitialization (1364-1400) and the temporal points of UpdateLastFrame (2194-2246).
// io.held_points / io.held_lines carry mvpMapPoints / mvpMapLines as slots in and out; per created entry io returns the feature index, the
// slot, position, normal and distance range for `new MapPoint` / `new MapLine`.  AddObservation, AddMapPoint, UpdateManhAxis, ids and the
// KeyFrame object stay with the caller, and so does the mvParallelLines[i]->size() > 0 gate on io.ln_rel.  The object owns the call's
// workspace: make one beside the maps.  Not thread-safe.
class Tracking {
public:
    explicit Tracking(const hvo_camera &cam, float thDepth, int nLevels = 8, int lineLevels = 1, float lineScale = 1.2f, int device = 0)
        : k_(hvo_kf_insert_create(device)), cam_(cam)
    {
        if (!k_) throw Error(HVO_ERR_HIP, "hvo_kf_insert_create");
        hvo_kfi_default_params(&p_);
        p_.th_depth = thDepth; p_.n_levels = nLevels; p_.line_n_levels = lineLevels; p_.line_scale_factor = lineScale;
    }
    ~Tracking() { hvo_kf_insert_destroy(k_); }
    Tracking(const Tracking &) = delete;
    Tracking &operator=(const Tracking &) = delete;
    hvo_kfi_params &params() { return p_; }                      // line_geometry, cos_par, cos_perp
    const char *lastError() const { return hvo_kf_insert_last_error(k_); }
    // on host arrays; the new entries go to firstPointSlot / firstLineSlot onwards (-1: returned only)
    hvo_kfi_result CreateNewKeyFrame(hvo_ctx *ctx, PointMap &points, LineMap &lines, const float Tcw[12], const hvo_kfi_frame &frame, hvo_kfi_io &io,
                                     int firstPointSlot, int firstLineSlot)
    {
        return run(ctx, nullptr, 0, &points, &lines, HVO_KFI_KEYFRAME, Tcw, &frame, io, firstPointSlot, firstLineSlot);
    }
    hvo_kfi_result StereoInitialization(hvo_ctx *ctx, PointMap &points, LineMap &lines, const float Tcw[12], const hvo_kfi_frame &frame, hvo_kfi_io &io,
                                        int firstPointSlot = 0, int firstLineSlot = 0)
    {
        return run(ctx, nullptr, 0, &points, &lines, HVO_KFI_INIT, Tcw, &frame, io, firstPointSlot, firstLineSlot);
    }
    // the temporal points of the last frame: returned only, io.held_points[i] becomes HVO_HELD_FOREIGN_UNOBSERVED
    hvo_kfi_result UpdateLastFrame(hvo_ctx *ctx, const PointMap &points, const float Tcw[12], const hvo_kfi_frame &frame, hvo_kfi_io &io)
    {
        return run(ctx, nullptr, 0, &points, nullptr, HVO_KFI_TEMPORAL, Tcw, &frame, io, -1, -1);
    }
    // on the resident frame `cur` of a stream (HVO_STAGE_ORB, an LSD stage, HVO_STAGE_LINES3D, bf > 0, depth); call before collect() releases the slot
    hvo_kfi_result CreateNewKeyFrame(FrameStream &fs, int64_t cur, PointMap &points, LineMap &lines, const float Tcw[12], hvo_kfi_io &io, int firstPointSlot, int firstLineSlot)
    {
        return run(nullptr, fs.get(), cur, &points, &lines, HVO_KFI_KEYFRAME, Tcw, nullptr, io, firstPointSlot, firstLineSlot);
    }
    hvo_kfi_result StereoInitialization(FrameStream &fs, int64_t cur, PointMap &points, LineMap &lines, const float Tcw[12], hvo_kfi_io &io, int firstPointSlot = 0,
                                        int firstLineSlot = 0)
    {
        return run(nullptr, fs.get(), cur, &points, &lines, HVO_KFI_INIT, Tcw, nullptr, io, firstPointSlot, firstLineSlot);
    }
    hvo_kfi_result UpdateLastFrame(FrameStream &fs, int64_t last, const PointMap &points, const float Tcw[12], hvo_kfi_io &io)
    {
        return run(nullptr, fs.get(), last, &points, nullptr, HVO_KFI_TEMPORAL, Tcw, nullptr, io, -1, -1);
    }
private:
    hvo_kfi_result run(hvo_ctx *ctx, hvo_stream *s, int64_t cur, const PointMap *pm, const LineMap *lm, int mode, const float Tcw[12], const hvo_kfi_frame *frame,
                       hvo_kfi_io &io, int fp, int fl)
    {
        hvo_kfi_params p = p_; p.mode = mode; p.first_point_slot = fp; p.first_line_slot = fl;
        hvo_kfi_result res;
        hvo_point_map *hp = pm ? pm->get() : nullptr; hvo_line_map *hl = lm ? lm->get() : nullptr;
        if (s) check(hvo_stream_create_keyframe_features(k_, s, hp, hl, cur, &cam_, Tcw, &p, &io, &res), "hvo_stream_create_keyframe_features");
        else check(hvo_create_keyframe_features(k_, ctx, hp, hl, &cam_, Tcw, &p, frame, &io, &res), "hvo_create_keyframe_features");
        return res;
    }
    hvo_kf_insert *k_; hvo_camera cam_; hvo_kfi_params p_;
};

// ORBVocabulary (include/ORBVocabulary.h = DBoW2's TemplatedVocabulary<FORB::TDescriptor, FORB>) resident on one device, read-only.  BowVectors is
// what Frame holds afterwards: mBowVec as (word, value) pairs in ascending word order, mFeatVec as CSR (node ids ascending, rows of ascending
// feature indices), and the per-feature node ids SearchByBoW takes for a key frame.
struct BowVectors {
    std::vector<int32_t> word_id, node_id, bow_word, fv_node, fv_start, fv_index; std::vector<double> bow_value;
    int n_short = 0; bool computed = false;
    hvo_bow prepare(int cap)
    {
        const size_t c = (size_t)(cap < 1 ? 1 : cap);
        word_id.assign(c, -1); node_id.assign(c, -1); bow_word.assign(c, 0); bow_value.assign(c, 0.0); fv_node.assign(c, 0); fv_start.assign(c + 1, 0); fv_index.assign(c, 0);
        hvo_bow b = hvo_bow(); b.cap = (int32_t)c;
        b.word_id = word_id.data(); b.node_id = node_id.data(); b.bow_word = bow_word.data(); b.bow_value = bow_value.data();
        b.fv_node = fv_node.data(); b.fv_start = fv_start.data(); b.fv_index = fv_index.data();
        return b;
    }
    void finish(const hvo_bow &b)
    {
        word_id.resize(b.n_features); node_id.resize(b.n_features); bow_word.resize(b.n_words); bow_value.resize(b.n_words);
        fv_node.resize(b.n_nodes); fv_start.resize(b.n_nodes + 1); fv_index.resize(b.n_valid); n_short = b.n_short; computed = b.computed != 0;
    }
};
class ORBVocabulary {
public:
    ORBVocabulary() : v_(nullptr) {}
    ORBVocabulary(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc, const double *weight)
        : v_(nullptr) { check(hvo_vocabulary_create(device, k, L, scoring, weighting, n_nodes, parent, is_leaf, desc, weight, &v_), "hvo_vocabulary_create"); }
    ~ORBVocabulary() { hvo_vocabulary_destroy(v_); }
    ORBVocabulary(const ORBVocabulary &) = delete;
    ORBVocabulary &operator=(const ORBVocabulary &) = delete;
    // the text format (ORBvoc.txt); false when the file is missing or malformed, like the reference
    bool loadFromTextFile(const std::string &filename, int device = 0)
    {
        hvo_vocabulary *v = nullptr;
        if (hvo_vocabulary_load_text(filename.c_str(), device, &v) != HVO_OK) return false;
        hvo_vocabulary_destroy(v_); v_ = v;
        return true;
    }
    bool empty() const { hvo_vocabulary_desc d; return !v_ || hvo_vocabulary_info(v_, &d) != HVO_OK || d.n_words == 0; }
    // transform(features, BowVector, FeatureVector, levelsup) on host descriptors (n x 32 bytes)
    void transform(hvo_ctx *ctx, const uint8_t *desc, int n, BowVectors &out, int levelsup = 4) const
    {
        hvo_bow b = out.prepare(n); const int32_t nd = n;
        check(hvo_compute_bow(ctx, v_, levelsup, 1, &desc, &nd, &b), "hvo_compute_bow");
        out.finish(b);
    }
    hvo_vocabulary *get() const { return v_; }
private:
    hvo_vocabulary *v_;
};
// Frame::ComputeBoW (src/Frame.cc:1692-1699) and ORBmatcher::SearchByBoW(pKF, F, ...) on a resident frame of a stream: the bag of words stays
// with the frame; a second ComputeBoW with the same vocabulary and levelsup launches nothing.
struct Frame {
    static void ComputeBoW(FrameStream &fs, int64_t ticket, const ORBVocabulary &voc, BowVectors &out, int levelsup = 4)
    {
        int kp = 0; check(hvo_stream_capacity(fs.get(), &kp, nullptr, nullptr), "hvo_stream_capacity");
        hvo_bow b = out.prepare(kp);
        check(hvo_stream_compute_bow(fs.get(), ticket, voc.get(), levelsup, &b), "hvo_stream_compute_bow");
        out.finish(b);
    }
    // n_kf key frames in one launch (Relocalization's loop); match_kf[j] gets the stream's key-point capacity, entries past the frame's count stay -1
    static void SearchByBoW(FrameStream &fs, int64_t cur, const ORBVocabulary &voc, int n_kf, const hvo_bow_keyframe *kf, std::vector<std::vector<int>> &match_kf,
                            std::vector<int> &nmatches, float nnratio = 0.7f, bool checkOrientation = true, int th_low = 50)
    {
        int kp = 0; check(hvo_stream_capacity(fs.get(), &kp, nullptr, nullptr), "hvo_stream_capacity");
        match_kf.assign((size_t)n_kf, std::vector<int>((size_t)kp, -1)); nmatches.assign((size_t)n_kf, 0);
        std::vector<hvo_bow_matches> r((size_t)n_kf);
        for (int j = 0; j < n_kf; j++) { r[j].match_kf = match_kf[j].data(); r[j].n_matches = 0; r[j].status = 0; }
        hvo_bow_search_params p = { nnratio, checkOrientation ? 1 : 0, th_low };
        check(hvo_stream_search_by_bow(fs.get(), cur, voc.get(), n_kf, kf, &p, r.data()), "hvo_stream_search_by_bow");
        for (int j = 0; j < n_kf; j++) nmatches[j] = r[j].n_matches;
    }
};

// KeyFrameDatabase (src/KeyFrameDatabase.cc) resident on the vocabulary's device.  A key frame is a slot (0 <= slot < 16384) the caller
// numbers -- the index of the KeyFrame in whatever table the tracker keeps; both detections return slots, in the reference's order.  The
// host owns the covisibility graph: after UpdateConnections it hands each touched key frame's GetBestCovisibilityKeyFrames(10) to
// setCovisible.  Not thread-safe: guard it by the mutex the reference's database has.
class KeyFrameDatabase {
public:
    explicit KeyFrameDatabase(const ORBVocabulary &voc) : db_(nullptr), voc_(voc.get()) { check(hvo_keyframe_db_create(voc_, &db_), "hvo_keyframe_db_create"); }
    ~KeyFrameDatabase() { hvo_keyframe_db_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete;
    KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;
    // add(pKF) with pKF->mBowVec on the host, or with the bag Frame::ComputeBoW left on the resident frame (device to device)
    void add(int slot, const BowVectors &bow) { chk(hvo_keyframe_db_add(db_, slot, (int)bow.bow_word.size(), bow.bow_word.data(), bow.bow_value.data()), "hvo_keyframe_db_add"); }
    void add(FrameStream &fs, int64_t ticket, int slot) { chk(hvo_stream_keyframe_db_add(fs.get(), ticket, voc_, db_, slot), "hvo_stream_keyframe_db_add"); }
    void erase(int slot) { chk(hvo_keyframe_db_erase(db_, slot), "hvo_keyframe_db_erase"); }
    void clear() { chk(hvo_keyframe_db_clear(db_), "hvo_keyframe_db_clear"); }
    void setCovisible(int slot, const std::vector<int> &slots) { chk(hvo_keyframe_db_set_covisible(db_, slot, (int)slots.size(), slots.data()), "hvo_keyframe_db_set_covisible"); }
    int size() const { hvo_keyframe_db_desc d; check(hvo_keyframe_db_info(db_, &d), "hvo_keyframe_db_info"); return d.n_live; }
    // Tracking.cc:3767: the frame's bag of words is the one Frame::ComputeBoW left on it
    std::vector<int> DetectRelocalizationCandidates(FrameStream &fs, int64_t ticket)
    {
        hvo_kfdb_params p = { HVO_KFDB_RELOC, 0.f, nullptr, 0 };
        hvo_kfdb_result r = result();
        chk(hvo_stream_keyframe_db_query(fs.get(), ticket, voc_, db_, &p, &r), "hvo_stream_keyframe_db_query");
        return std::vector<int>(cand_.begin(), cand_.begin() + r.n_candidates);
    }
    // LoopClosing::DetectLoop: the query key frame's bag, the slots of its GetConnectedKeyFrames(), minScore
    std::vector<int> DetectLoopCandidates(const BowVectors &bow, const std::vector<int> &connected, float minScore)
    {
        hvo_kfdb_params p = { HVO_KFDB_LOOP, minScore, connected.data(), (int32_t)connected.size() };
        hvo_kfdb_result r = result();
        chk(hvo_keyframe_db_query(db_, (int)bow.bow_word.size(), bow.bow_word.data(), bow.bow_value.data(), &p, &r), "hvo_keyframe_db_query");
        return std::vector<int>(cand_.begin(), cand_.begin() + r.n_candidates);
    }
    float lastKernelMs() const { float ms = 0.f; check(hvo_keyframe_db_last_kernel_ms(db_, &ms), "hvo_keyframe_db_last_kernel_ms"); return ms; }
    hvo_keyframe_db *get() const { return db_; }
private:
    void chk(int rc, const char *what) const { if (rc != HVO_OK) throw Error(rc, std::string(what) + ": " + hvo_keyframe_db_last_error(db_)); }
    hvo_kfdb_result result()
    {
        hvo_keyframe_db_desc d; check(hvo_keyframe_db_info(db_, &d), "hvo_keyframe_db_info");
        cand_.assign((size_t)(d.n_slots < 1 ? 1 : d.n_slots), -1);
        hvo_kfdb_result r = hvo_kfdb_result(); r.cap = (int32_t)cand_.size(); r.candidate = cand_.data();
        return r;
    }
    hvo_keyframe_db *db_; const hvo_vocabulary *voc_; std::vector<int32_t> cand_;
};

inline int ORBmatcher::SearchByProjection(FrameStream &fs, int64_t cur, const hvo_camera &cam, const float Tcw[12], const KeyFrameSide &kf, const uint8_t *skip,
                                          const uint8_t *occupied, int n_features, float th, int ORBdist, KeyFrameMatches &res, bool checkOrientation,
                                          float logScaleFactor, int nLevels) const
{
    hvo_kf_search_candidate c; hvo_kf_search_params p; hvo_kf_search_result r;
    kf_search_fill(Tcw, kf, skip, occupied, n_features, th, ORBdist, checkOrientation, logScaleFactor, nLevels, res, c, p, r);
    check(hvo_stream_search_by_projection_keyframe(fs.get(), cur, &cam, &p, 1, &c, &r), "hvo_stream_search_by_projection_keyframe");
    res.n_searched = r.n_searched; res.kernel_ms[0] = r.kernel_ms[0]; res.kernel_ms[1] = r.kernel_ms[1];
    return r.n_matches;
}

inline int ORBmatcher::Fuse(FrameStream &fs, int64_t cur, const hvo_camera &cam, float bf, const float Tcw[12], const uint8_t *skip, const hvo_fuse_map *vpMapPoints,
                            hvo_point_map *map, int n_slots, const int32_t *slots, FuseMatches &res, float th, float logScaleFactor, int nLevels) const
{
    hvo_fuse_params p = fuse_params(bf, th, logScaleFactor, nLevels);
    hvo_fuse_result r = fuse_result(res, vpMapPoints ? vpMapPoints->n : n_slots);
    check(hvo_stream_fuse_points(fs.get(), cur, &cam, &p, Tcw, skip, vpMapPoints, map, n_slots, slots, &r), "hvo_stream_fuse_points");
    return fuse_take(res, r);
}

inline int LSDmatcher::Fuse(FrameStream &fs, int64_t cur, const hvo_camera &cam, const float Tcw[12], const uint8_t *skip, const hvo_lf_map *vpMapLines, hvo_line_map *map,
                            int n_slots, const int32_t *slots, LineFuseMatches &res, const hvo_lf_params &p) const
{
    hvo_lf_result r = lf_result(res, vpMapLines ? vpMapLines->n : n_slots);
    check(hvo_stream_fuse_lines(fs.get(), cur, &cam, &p, Tcw, skip, vpMapLines, map, n_slots, slots, &r), "hvo_stream_fuse_lines");
    return lf_take(res, r);
}

inline int LocalMapping::CreateNewMapLinesConstraint(FrameStream &fs, int64_t cur, const hvo_camera &cam, const float Tcw[12], const uint8_t *has_map_line, int n_lines,
                                                     int n_kf, const hvo_nl_keyframe *vpNeighKFs, std::vector<NewMapLineMatches> &matches, std::vector<NewMapLines> &res,
                                                     std::vector<int> *owner_pair, int pairing, int nLevels, float scale, float kernel_ms[3]) const
{
    hvo_nl_params p = { 80, 0.85f, nLevels, scale, pairing };
    // The library reads one occupancy byte and writes one entry per line the frame HOLDS, and the C ABI takes no count: every array is sized by
    // the stream's key-line capacity, which bounds that count, and the occupancy bytes are copied into a zero-padded buffer of that size.
    const int cap = std::max(std::max(n_lines, 0), fs.klCap());
    std::vector<uint8_t> has((size_t)std::max(cap, 1), 0);
    if (has_map_line && n_lines > 0) memcpy(has.data(), has_map_line, (size_t)n_lines);
    std::vector<hvo_nl_match> m; std::vector<hvo_nl_result> r; hvo_nl_summary s = nl_begin(cap, n_kf, matches, res, m, r, owner_pair);
    check(hvo_stream_create_new_map_lines(fs.get(), cur, &cam, &p, Tcw, has.data(), n_kf, vpNeighKFs, m.data(), (int)r.size(), r.data(), &s), "hvo_stream_create_new_map_lines");
    return nl_end(matches, res, m, r, s, kernel_ms);
}

inline int LocalMapping::CreateNewMapPoints(FrameStream &fs, int64_t cur, const ORBVocabulary &voc, const hvo_camera &cam, const float Tcw[12], const uint8_t *has_map_point,
                                            int n_features, int n_kf, const hvo_np_keyframe *vpNeighKFs, std::vector<NewMapPoints> &res, std::vector<int> *owner,
                                            float mfScaleFactor, int nLevels, float kernel_ms[3]) const
{
    hvo_np_params p = { ORBmatcher::TH_LOW, nLevels, mfScaleFactor, cam.bf };
    std::vector<hvo_np_result> r; hvo_np_summary s = np_begin(n_features, n_kf, res, r, owner);
    check(hvo_stream_create_new_map_points(fs.get(), cur, voc.get(), &cam, &p, Tcw, has_map_point, n_kf, vpNeighKFs, r.data(), &s), "hvo_stream_create_new_map_points");
    return np_end(res, r, s, kernel_ms);
}

// Optimizer (include/Optimizer.h, src/Optimizer.cc:590-1478): PoseOptimization on the mirror's frame handle.  The map side (one row per feature:
// the matched map point's / map line's world position, the planes of the three roles as world coefficients or as slots of a PlaneMap) is what
// the tracker fills from mvpMapPoints / mvpMapLines / mvpMapPlanes...; the frame side is read from the resident frame.  The optimised pose comes
// back in res.Tcw (what SetPose receives), the flags in `flags`; the return value is the reference's.
struct PoseMapSide {
    int n_points = 0, n_lines = 0, n_planes = 0;
    const uint8_t *pt_has = nullptr; const float *pt_xyz = nullptr;
    const uint8_t *ln_has = nullptr; const double *ln_xyz = nullptr;
    const uint8_t *pl_has = nullptr; const float *pl_coef_w = nullptr;
    const PlaneMap *plane_map = nullptr; const hvo_plane_match *plane_match = nullptr;    // instead of pl_has / pl_coef_w
    hvo_pose_flags flags = { nullptr, nullptr, nullptr, nullptr };
};
// Optimizer::LocalMapOptimization (src/Optimizer.cc:3014-3940) on the device: hvo_local_ba.  The object owns its grow-only workspace;
// create it once beside the map.  LocalMapGraph is what the adaptor gathers: key frame 0 is the CURRENT key
// frame, the local key frames first, the outside observers after them with fixed = 1; observations name their key frame by its index.
class LocalBA {
public:
    explicit LocalBA(int device = 0) : ba_(nullptr) { check(hvo_local_ba_create(device, &ba_), "hvo_local_ba_create"); }
    ~LocalBA() { hvo_local_ba_destroy(ba_); }
    LocalBA(const LocalBA &) = delete;
    LocalBA &operator=(const LocalBA &) = delete;
    hvo_local_ba *get() const { return ba_; }
    std::string lastError() const { return hvo_local_ba_last_error(ba_); }
    float lastMs() const { float ms = 0.f; hvo_local_ba_last_ms(ba_, &ms); return ms; }
private:
    hvo_local_ba *ba_;
};
struct LocalMapGraph {
    std::vector<float> Tcw, cam; std::vector<uint8_t> fixed;                              // n_kf x 12, x 4, x 1
    std::vector<float> pt_pos, pt_obs_uv, pt_obs_inv_sigma2; std::vector<int32_t> pt_obs_start = { 0 }, pt_obs_kf;
    std::vector<double> ln_pos, ln_obs_fn, par_fn, perp_fn;
    std::vector<int32_t> ln_manh_idx, ln_obs_start = { 0 }, ln_obs_kf, par_start = { 0 }, par_kf, par_idx, par_map_size, perp_start = { 0 }, perp_kf, perp_idx, perp_map_size;
    double manh_axis[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }; bool manh_available = false;       // row-major, column a - 1 = axis a
    hvo_local_ba_params params;
    LocalMapGraph() { hvo_local_ba_default_params(&params); }
    int nKF() const { return (int)fixed.size(); }
    int nPoints() const { return (int)pt_obs_start.size() - 1; }
    int nLines() const { return (int)ln_obs_start.size() - 1; }
    // the builders follow the reference's loops: one call per key frame, per map point with its observations, per map line
    int addKeyFrame(const float Tcw12[12], bool isFixed, float fx, float fy, float cx, float cy)
    {
        Tcw.insert(Tcw.end(), Tcw12, Tcw12 + 12); fixed.push_back(isFixed ? 1 : 0);
        cam.push_back(fx); cam.push_back(fy); cam.push_back(cx); cam.push_back(cy);
        return nKF() - 1;
    }
    int addPoint(const float pos[3]) { pt_pos.insert(pt_pos.end(), pos, pos + 3); pt_obs_start.push_back(pt_obs_start.back()); return nPoints() - 1; }
    void addPointObservation(int kf, float u, float v, float invSigma2)                  // of the point added last
    {
        pt_obs_kf.push_back(kf); pt_obs_uv.push_back(u); pt_obs_uv.push_back(v); pt_obs_inv_sigma2.push_back(invSigma2); pt_obs_start.back()++;
    }
    int addLine(const double pos[6], int manhIdx, int parMapSize, int perpMapSize)
    {
        ln_pos.insert(ln_pos.end(), pos, pos + 6); ln_manh_idx.push_back(manhIdx); par_map_size.push_back(parMapSize); perp_map_size.push_back(perpMapSize);
        ln_obs_start.push_back(ln_obs_start.back()); par_start.push_back(par_start.back()); perp_start.push_back(perp_start.back());
        return nLines() - 1;
    }
    void addLineObservation(int kf, const double fn[3]) { ln_obs_kf.push_back(kf); ln_obs_fn.insert(ln_obs_fn.end(), fn, fn + 3); ln_obs_start.back()++; }
    void addParEntry(int kf, int idx, const double fn[3]) { par_kf.push_back(kf); par_idx.push_back(idx); par_fn.insert(par_fn.end(), fn, fn + 3); par_start.back()++; }
    void addPerpEntry(int kf, int idx, const double fn[3]) { perp_kf.push_back(kf); perp_idx.push_back(idx); perp_fn.insert(perp_fn.end(), fn, fn + 3); perp_start.back()++; }
    hvo_local_ba_graph view() const
    {
        hvo_local_ba_graph g = {};
        g.n_kf = nKF(); g.n_points = nPoints(); g.n_lines = nLines(); g.manh_available = manh_available ? 1 : 0;
        g.Tcw = Tcw.data(); g.fixed = fixed.data(); g.cam = cam.data();
        g.pt_pos = pt_pos.data(); g.pt_obs_start = pt_obs_start.data(); g.pt_obs_kf = pt_obs_kf.data(); g.pt_obs_uv = pt_obs_uv.data(); g.pt_obs_inv_sigma2 = pt_obs_inv_sigma2.data();
        g.ln_pos = ln_pos.data(); g.ln_manh_idx = ln_manh_idx.data(); g.ln_obs_start = ln_obs_start.data(); g.ln_obs_kf = ln_obs_kf.data(); g.ln_obs_fn = ln_obs_fn.data();
        g.par_start = par_start.data(); g.par_kf = par_kf.data(); g.par_idx = par_idx.data(); g.par_fn = par_fn.data(); g.par_map_size = par_map_size.data();
        g.perp_start = perp_start.data(); g.perp_kf = perp_kf.data(); g.perp_idx = perp_idx.data(); g.perp_fn = perp_fn.data(); g.perp_map_size = perp_map_size.data();
        g.manh_axis = manh_axis;
        return g;
    }
};
struct LocalMapResult {
    std::vector<float> Tcw, points, lines;                                                 // what SetPose / SetWorldPos receive (Converter::toCvMat)
    std::vector<double> Tcw_d, points_d, lines_d;
    std::vector<uint8_t> pt_erase, ln_erase, manh_erase, par_erase, perp_erase, par_made, perp_made, line_made;
    hvo_local_ba_result res = hvo_local_ba_result();
    void bind(const LocalMapGraph &g)
    {
        const size_t one = 1;                                                              // never hand over a null pointer for an empty list
        Tcw.assign(std::max(one, g.Tcw.size()), 0.f); Tcw_d.assign(Tcw.size(), 0.0); points.assign(std::max(one, g.pt_pos.size()), 0.f); points_d.assign(points.size(), 0.0);
        lines.assign(std::max(one, g.ln_pos.size()), 0.f); lines_d.assign(lines.size(), 0.0);
        pt_erase.assign(std::max(one, g.pt_obs_kf.size()), 0); ln_erase.assign(std::max(one, g.ln_obs_kf.size()), 0); manh_erase.assign(std::max(one, (size_t)g.nLines()), 0);
        par_erase.assign(std::max(one, g.par_kf.size()), 0); perp_erase.assign(std::max(one, g.perp_kf.size()), 0); par_made = par_erase; perp_made = perp_erase; line_made = manh_erase;
        res = hvo_local_ba_result();
        res.Tcw_f = Tcw.data(); res.Tcw_d = Tcw_d.data(); res.pt_f = points.data(); res.pt_d = points_d.data(); res.ln_f = lines.data(); res.ln_d = lines_d.data();
        res.pt_erase = pt_erase.data(); res.ln_erase = ln_erase.data(); res.manh_erase = manh_erase.data(); res.par_erase = par_erase.data(); res.perp_erase = perp_erase.data();
        res.par_made = par_made.data(); res.perp_made = perp_made.data(); res.line_made = line_made.data();
    }
};
// The host walk of :3849-3901 over the flags, under the caller's mMutexMapUpdate.  Each callback receives indices of the graph; the walk
// re-tests isBad() through them (reading 8: return without erasing when the element turned bad meanwhile).
//   erasePoint(kf, point)        pKFi->EraseMapPointMatch(pMP); pMP->EraseObservation(pKFi)
//   eraseLine(kf, line)          pKFi->EraseMapLineMatch(pML); pML->EraseObservation(pKFi)
//   erasePar / erasePerp(line, kf, k)   pML->EraseParObs(pKFi, k): k is the entry's position in its key frame's vector
// Reading 4: vpLineEdgeKF holds TWO entries per observation and is indexed by observation, so the reference pairs the erased line
// observation i (in push order over the made lines) with the key frame of observation i / 2.  asWritten = true reproduces that;
// false pairs an observation with its own key frame.  Reading 5: no Manhattan observation is erased (vpLineManhKF is never filled);
// LocalMapResult::manh_erase is the caller's to use.
template <class EP, class EL, class EPar, class EPerp>
inline void walkErased(const LocalMapGraph &g, const LocalMapResult &r, EP erasePoint, EL eraseLine, EPar erasePar, EPerp erasePerp, bool asWritten = true)
{
    for (int p = 0; p < g.nPoints(); p++)
        for (int o = g.pt_obs_start[p]; o < g.pt_obs_start[p + 1]; o++) if (r.pt_erase[o]) erasePoint(g.pt_obs_kf[o], p);
    std::vector<int> push;                                                                 // vpLineEdgesSP's order: the observations of the made lines
    for (int l = 0; l < g.nLines(); l++) if (r.line_made[l]) for (int o = g.ln_obs_start[l]; o < g.ln_obs_start[l + 1]; o++) push.push_back(o);
    std::vector<int> owner(g.ln_obs_kf.size(), 0);
    for (int l = 0; l < g.nLines(); l++) for (int o = g.ln_obs_start[l]; o < g.ln_obs_start[l + 1]; o++) owner[o] = l;
    for (size_t i = 0; i < push.size(); i++)
        if (r.ln_erase[push[i]]) eraseLine(g.ln_obs_kf[asWritten ? push[i / 2] : push[i]], owner[push[i]]);
    for (int s = 0; s < 2; s++) {
        const std::vector<int32_t> &start = s ? g.perp_start : g.par_start, &kf = s ? g.perp_kf : g.par_kf;
        const std::vector<uint8_t> &flag = s ? r.perp_erase : r.par_erase;
        for (int l = 0; l < g.nLines(); l++)
            for (int o = start[l]; o < start[l + 1]; o++) {
                if (!flag[o]) continue;
                int first = o;
                while (first > start[l] && kf[first - 1] == kf[o]) first--;
                if (s) erasePerp(l, kf[o], o - first); else erasePar(l, kf[o], o - first);
            }
    }
}

class Optimizer {
public:
    // Optimizer::LocalMapOptimization(mManhAxis, mpCurrentKeyFrame, &mbAbortBA, mpMap, mAvailableOptManh) becomes
    // Optimizer::LocalMapOptimization(ba, graph, &abort, result); stop may be null.  Returns the status (HVO_LBA_*).
    static int LocalMapOptimization(LocalBA &ba, const LocalMapGraph &g, const int *stop, LocalMapResult &r)
    {
        r.bind(g);
        const hvo_local_ba_graph v = g.view();
        const int rc = hvo_local_ba_optimize(ba.get(), &g.params, &v, stop, &r.res);
        if (rc != HVO_OK) throw Error(rc, "hvo_local_ba_optimize: " + ba.lastError());
        return r.res.status;
    }
    explicit Optimizer(const hvo_camera &cam, const hvo_pose_plane_params *pp = nullptr) : cam_(cam), has_pp_(pp != nullptr) { if (pp) pp_ = *pp; }
    // int nInliers = Optimizer::PoseOptimization(&mCurrentFrame)  becomes  optimizer.PoseOptimization(fs, ticket, Tcw, side, res)
    int PoseOptimization(FrameStream &fs, int64_t cur, const float Tcw[12], const PoseMapSide &m, hvo_pose_result &res) const
    {
        hvo_pose_problem p = fill(Tcw, m);
        check(hvo_stream_pose_optimize(fs.get(), cur, &cam_, has_pp_ ? &pp_ : nullptr, &p, &res, &m.flags), "hvo_stream_pose_optimize");
        return res.ret;
    }
    // on host arrays: p carries the frame side too
    int PoseOptimization(hvo_ctx *ctx, const hvo_pose_problem &p, hvo_pose_result &res, const hvo_pose_flags *flags = nullptr) const
    {
        check(hvo_pose_optimize(ctx, &cam_, has_pp_ ? &pp_ : nullptr, 1, &p, &res, flags), "hvo_pose_optimize");
        return res.ret;
    }
private:
    static hvo_pose_problem fill(const float Tcw[12], const PoseMapSide &m)
    {
        hvo_pose_problem p = {};
        for (int i = 0; i < 12; i++) p.Tcw[i] = Tcw[i];
        p.n_points = m.n_points; p.n_lines = m.n_lines; p.n_planes = m.n_planes;
        p.pt_has = m.pt_has; p.pt_xyz = m.pt_xyz; p.ln_has = m.ln_has; p.ln_xyz = m.ln_xyz; p.pl_has = m.pl_has; p.pl_coef_w = m.pl_coef_w;
        if (m.plane_map && m.plane_match) {
            p.plane_map = m.plane_map->get(); p.slot_match = m.plane_match->match; p.slot_parallel = m.plane_match->parallel; p.slot_vertical = m.plane_match->vertical;
        }
        return p;
    }
    hvo_camera cam_; hvo_pose_plane_params pp_ = { 0.5, 50.0, 0.1, 0.1, 100.0, 50.0 }; bool has_pp_;
};

// The per-frame step between the Frame constructor and Track() (src/Tracking.cc:270-335): Manhattan::computeStructConstrains for every key line
// and Optimizer::LineOptStruct, on the mirror's frame handle.  FrameLines holds what the reference keeps on the Frame: mvParLinesIdx /
// mvPerpLinesIdx (partner indices in ascending order, -1 in a slot LineOptStruct rejected) and mvLines3D (start, end) after the call.
struct FrameLines {
    int NL = 0;
    std::vector<int8_t> rel;                                   // NL x NL: 0 none, 1 parallel, 2 perpendicular, negative = rejected
    std::vector<std::vector<int>> mvParLinesIdx, mvPerpLinesIdx;
    std::vector<double> mvLines3D;                             // NL x 6
    hvo_line_opt_result res = hvo_line_opt_result();
    void rebuild()                                             // the vectors from rel
    {
        mvParLinesIdx.assign(NL, std::vector<int>()); mvPerpLinesIdx.assign(NL, std::vector<int>());
        for (int k = 0; k < NL; k++) for (int i = 0; i < NL; i++) {
            const int v = rel[(size_t)k * NL + i];
            if (v == 1 || v == -1) mvParLinesIdx[k].push_back(v > 0 ? i : -1);
            else if (v == 2 || v == -2) mvPerpLinesIdx[k].push_back(v > 0 ? i : -1);
        }
    }
};
class Manhattan {
public:
    // mpManh->computeStructConstrains(mCurrentFrame, k, par, perp) for every k at once (the loop at Tracking.cc:270-293); NL = the frame's key-line count
    static void computeStructConstrains(FrameStream &fs, int64_t cur, int NL, FrameLines &f, int row_rule = HVO_LINE_STRUCT_ROW_UNSET)
    {
        run(fs, cur, NL, f, HVO_LINE_STRUCT_CONSTRAINTS, row_rule);
    }
    // the reference's per-line form, read from the lists computed above
    static void computeStructConstrains(const FrameLines &f, int idx, std::vector<int> &idxPar, std::vector<int> &idxPerp)
    {
        idxPar = f.mvParLinesIdx[idx]; idxPerp = f.mvPerpLinesIdx[idx];
    }
    static void run(FrameStream &fs, int64_t cur, int NL, FrameLines &f, unsigned mode, int row_rule)
    {
        hvo_line_struct_params p; check(hvo_line_struct_default_params(&p), "hvo_line_struct_default_params");
        p.mode = mode; p.row_rule = row_rule;
        if (!(mode & HVO_LINE_STRUCT_CONSTRAINTS) && (f.NL != NL || f.rel.size() != (size_t)NL * NL)) throw Error(HVO_ERR_INVALID_ARG, "LineOptStruct without lists");
        f.NL = NL; f.rel.resize((size_t)NL * NL); f.mvLines3D.resize((size_t)NL * 6);
        check(hvo_stream_line_struct_optimize(fs.get(), cur, &p, NL, f.rel.data(), f.mvLines3D.data(), &f.res), "hvo_stream_line_struct_optimize");
        f.rebuild();
    }
};
// Optimizer::LineOptStruct(&mCurrentFrame) on the lists of f (computeStructConstrains first), or both steps in one call with both = true
inline void LineOptStruct(FrameStream &fs, int64_t cur, int NL, FrameLines &f, bool both = false, int row_rule = HVO_LINE_STRUCT_ROW_UNSET)
{
    Manhattan::run(fs, cur, NL, f, both ? (HVO_LINE_STRUCT_CONSTRAINTS | HVO_LINE_STRUCT_OPTIMIZE) : HVO_LINE_STRUCT_OPTIMIZE, row_rule);
}

// PnPsolver (src/PnPsolver.h) with the reference's surface and ONE device call underneath for all candidates of a relocalisation:
// solve_candidates evaluates every hypothesis of every candidate (hvo_stream_pnp_ransac), iterate() is a host replay over hyp_event /
// the events that keeps mnIterations between calls, so Tracking::Relocalization's round-robin loop (src/Tracking.cc:3834-3909) reads as it
// does today.  A replay that would need a hypothesis past the T evaluated ones reports bNoMore.
class PnPsolver {
public:
    PnPsolver() { hvo_pnp_default_params(&params_); }
    // the result's pointers lead into this object's own vectors: a move carries the buffers along, a copy would leave them behind
    PnPsolver(const PnPsolver &) = delete;
    PnPsolver &operator=(const PnPsolver &) = delete;
    PnPsolver(PnPsolver &&) = default;
    PnPsolver &operator=(PnPsolver &&) = default;
    // the reference sets the parameters per solver before iterating; here they apply to the next solve_candidates
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f, float th2 = 5.991f)
    {
        params_.probability = probability; params_.min_inliers = minInliers; params_.max_iterations = maxIterations; params_.min_set = minSet;
        params_.epsilon = epsilon; params_.th2 = th2;
    }
    hvo_pnp_params &params() { return params_; }
    // one call for all candidates: solvers[j] takes candidate j's result (its parameters are solvers[0]'s: Relocalization gives every solver the same)
    static void solve_candidates(FrameStream &fs, int64_t cur, const hvo_camera &cam, const std::vector<hvo_pnp_keyframe_side> &kf_sides, std::vector<PnPsolver> &solvers)
    {
        const int n = (int)kf_sides.size();
        if (n < 1 || (int)solvers.size() != n) throw Error(HVO_ERR_INVALID_ARG, "PnPsolver::solve_candidates");
        const hvo_pnp_params P = solvers[0].params_;
        std::vector<hvo_pnp_result> res((size_t)n);
        for (int j = 0; j < n; j++) { solvers[j].params_ = P; solvers[j].alloc(fs.kpCap()); res[j] = solvers[j].res_; }
        const int rc = hvo_stream_pnp_ransac(fs.get(), cur, &cam, &P, n, kf_sides.data(), res.data());
        for (int j = 0; j < n; j++) { solvers[j].res_ = res[j]; solvers[j].mnIterations = 0; }
        if (rc != HVO_ERR_CAPACITY) check(rc, "hvo_stream_pnp_ransac");      // a candidate past max_events keeps its status; iterate() throws for that one
    }
    // cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers): true and Tcw (upper 3 x 4, row-major) when the reference returns a pose
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float Tcw[12])
    {
        bNoMore = false; vbInliers.clear(); nInliers = 0;
        if (res_.status != HVO_OK) throw Error(res_.status, "PnPsolver::iterate: more records than max_events");
        if (res_.n < res_.min_inliers) { bNoMore = true; return false; }
        int nCurrentIterations = 0;
        while (mnIterations < res_.max_its || nCurrentIterations < nIterations) {
            nCurrentIterations++; mnIterations++;
            if (mnIterations > res_.n_hyp) { bNoMore = true; return false; }
            const int e = hyp_event_[mnIterations - 1];
            if (e >= 0) {
                const hvo_pnp_event &V = events_[e];
                nInliers = V.n_inliers; vbInliers.assign(V.inliers, V.inliers + res_.n_features);
                for (int i = 0; i < 12; i++) Tcw[i] = V.Tcw[i];
                return true;
            }
        }
        if (mnIterations >= res_.max_its) {
            bNoMore = true;
            const hvo_pnp_event *last = nullptr;                 // mnBestInliers / mBestTcw now: the latest record at or before mnIterations
            for (int e = 0; e < res_.n_events; e++) if (events_[e].iteration <= mnIterations) last = &events_[e];
            if (last) {
                nInliers = last->hyp_n_inliers; vbInliers.assign(last->hyp_inliers, last->hyp_inliers + res_.n_features);
                for (int i = 0; i < 12; i++) Tcw[i] = last->hyp_Tcw[i];
                return true;
            }
        }
        return false;
    }
    bool find(std::vector<bool> &vbInliers, int &nInliers, float Tcw[12]) { bool f; return iterate(res_.max_its, f, vbInliers, nInliers, Tcw); }
    const hvo_pnp_result &result() const { return res_; }
    int mnIterations = 0;
private:
    void alloc(int n_features)
    {
        const int cap = std::min(1024, params_.max_iterations + params_.extra_iterations), E = params_.max_events;
        hyp_inl_.assign(cap, 0); hyp_event_.assign(cap, -1); events_.assign(E, hvo_pnp_event()); inl_.assign((size_t)(2 * E + 1) * n_features, 0);
        for (int e = 0; e < E; e++) { events_[e].inliers = inl_.data() + (size_t)(2 * e) * n_features; events_[e].hyp_inliers = inl_.data() + (size_t)(2 * e + 1) * n_features; }
        res_ = hvo_pnp_result();
        res_.cap_hyp = cap; res_.cap_events = E; res_.hyp_inliers = hyp_inl_.data(); res_.hyp_event = hyp_event_.data(); res_.hyp_sample = nullptr;
        res_.events = events_.data(); res_.best_inliers = inl_.data() + (size_t)(2 * E) * n_features;
    }
    hvo_pnp_params params_; hvo_pnp_result res_ = hvo_pnp_result();
    std::vector<int32_t> hyp_inl_, hyp_event_; std::vector<hvo_pnp_event> events_; std::vector<uint8_t> inl_;
};

}  // namespace hvo
