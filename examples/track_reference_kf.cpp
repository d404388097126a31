// track_reference_kf.cpp -- the whole of Tracking::TrackReferenceKeyFrame (reference src/Tracking.cc:1831-1960) on a resident frame through
// the C++ mirror (include/hvo.hpp): mCurrentFrame.ComputeBoW(), ORBmatcher::SearchByBoW(mpReferenceKF, mCurrentFrame, ...),
// LSDmatcher::match(Last, Cur), PlaneMatcher::SearchMapByCoefficients and Optimizer::PoseOptimization with those matches.  The first
// frame plays the reference key frame (camera = world): its features with depth are the map points, its good 3-D lines the map lines, its
// planes the plane map, and its own bag of words (KeyFrame::ComputeBoW) gives the node ids the search needs.  Every later frame is tracked
// against it from the identity pose; before the key frame's slot would leave the stream's ring of resident frames (the line matcher reads
// its descriptors there), the frame just tracked becomes the new reference key frame, as a tracker inserts key frames.  Between the frames' upload and the optimised pose only the key frame's arrays, the matches and the
// matched positions cross PCIe.  No vocabulary file is needed: the example generates a small random k = 8, L = 3 tree (a trained
// ORBvoc.txt loads with ORBVocabulary::loadFromTextFile).  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/track_reference_kf.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o track_reference_kf
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "hvo.hpp"

static bool read_raw(const char *path, void *dst, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

// a full k-ary tree of depth L with random descriptors and weights, rows level by level (parents before children)
static void make_vocabulary(int k, int L, std::vector<int32_t> &parent, std::vector<uint8_t> &leaf, std::vector<uint8_t> &desc, std::vector<double> &weight)
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    int first = 0, count = 1;                                                // the nodes of the level above: ids first .. first + count - 1
    for (int level = 1; level <= L; level++) {
        const int base = (int)parent.size() + 1;
        for (int p = first; p < first + count; p++)
            for (int c = 0; c < k; c++) {
                parent.push_back(p); leaf.push_back(level == L);
                for (int b = 0; b < 32; b++) desc.push_back((uint8_t)(rnd() >> 24));
                weight.push_back(level == L ? 0.5 + (double)(rnd() % 1000) / 200.0 : 0.0);
            }
        first = base; count *= k;
    }
}

int main(int argc, char **argv)
{
    if (argc < 5 || argc % 2 != 1) { fprintf(stderr, "usage: %s gray0.u8 depth0.u16 gray1.u8 depth1.u16 [...]\n", argv[0]); return 2; }
    const int W = 640, H = 480, n = (argc - 1) / 2;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 4; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_FRAME;
        hvo::FrameStream fs(p, sp);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::Optimizer optimizer(cam);
        hvo::PlaneMatcher pmatcher(0.05f, 0.985f, 0.08716f, 0.9962f);
        std::vector<int32_t> vp; std::vector<uint8_t> vl, vd; std::vector<double> vw;
        make_vocabulary(8, 3, vp, vl, vd, vw);
        hvo::ORBVocabulary voc(p.device, 8, 3, HVO_VOC_L1_NORM, HVO_VOC_TF_IDF, (int)vp.size(), vp.data(), vl.data(), vd.data(), vw.data());
        const int levelsup = 1;                                              // (ORBvoc: 4 of 6 levels)
        int kp_cap = 0, kl_cap = 0, pl_cap = 0;
        hvo::check(hvo_stream_capacity(fs.get(), &kp_cap, &kl_cap, &pl_cap), "hvo_stream_capacity");
        const float I[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        // the reference key frame, as the host keeps it
        int64_t t_kf = -1; int N_kf = 0, NL_kf = 0, k_kf = 0;
        std::vector<uint8_t> kf_desc((size_t)kp_cap * 32), kf_has(kp_cap); std::vector<float> kf_angle(kp_cap), kf_xyz(3 * (size_t)kp_cap);
        std::vector<double> kf_lxyz(6 * (size_t)kl_cap); std::vector<uint8_t> kf_lgood(kl_cap);
        hvo::BowVectors kf_bow;
        std::unique_ptr<hvo::PlaneMap> pmap;
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo::FrameStream::FrameTail tail;
            fs.collectTail(t, W, H, tail);
            std::vector<hvo_keypoint> kp(kp_cap), kpu(kp_cap); std::vector<float> ur(kp_cap), zd(kp_cap); std::vector<uint8_t> desc((size_t)kp_cap * 32);
            std::vector<hvo_keyline> kl(kl_cap);
            hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.desc = desc.data(); fo.kp_cap = kp_cap; fo.kl = kl.data(); fo.kl_cap = kl_cap;
            fs.collect(t, fo, kpu.data(), ur.data(), zd.data());               // the slot stays resident until `depth` newer frames were submitted
            const int N = fo.n_kp, NL = fo.n_kl;
            hvo::BowVectors bow;
            hvo::Frame::ComputeBoW(fs, t, voc, bow, levelsup);                 // mCurrentFrame.ComputeBoW()
            auto make_key_frame = [&]() {                                     // this frame becomes the reference key frame (camera = world)
                t_kf = t; k_kf = k; N_kf = N; NL_kf = NL; kf_bow = bow; kf_desc = desc;
                for (int i = 0; i < N; i++) {
                    kf_has[i] = zd[i] > 0; kf_angle[i] = kpu[i].angle;
                    const float z = zd[i] > 0 ? zd[i] : 1.f;
                    kf_xyz[3 * i] = (kpu[i].x - p.cx) / p.fx * z; kf_xyz[3 * i + 1] = (kpu[i].y - p.cy) / p.fy * z; kf_xyz[3 * i + 2] = z;
                }
                for (int i = 0; i < NL; i++) {
                    kf_lgood[i] = tail.lines3d[i].good != 0;
                    for (int j = 0; j < 3; j++) { kf_lxyz[6 * i + j] = tail.lines3d[i].A[j]; kf_lxyz[6 * i + 3 + j] = tail.lines3d[i].B[j]; }
                }
                pmap.reset(new hvo::PlaneMap(p.device));
                for (int i = 0; i < 64; i++) {
                    const hvo_plane_cloud &pc = tail.plane_clouds[i];
                    if (pc.valid) pmap->set(pmap->size(), pc.coef, tail.cloud_xyz.data() + 3 * (size_t)pc.first, pc.n_points);
                }
                printf("key frame %d: %d points (%d words, %d nodes), %d lines, %d map planes\n", k, N, (int)bow.bow_word.size(), (int)bow.fv_node.size(), NL, pmap->size());
            };
            if (k == 0) { make_key_frame(); continue; }
            // ORBmatcher matcher(0.7, true); matcher.SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches)
            const hvo_bow_keyframe kf = { kf_desc.data(), kf_bow.node_id.data(), kf_has.data(), kf_angle.data(), N_kf };
            std::vector<std::vector<int>> match_kf; std::vector<int> nmatches;
            hvo::Frame::SearchByBoW(fs, t, voc, 1, &kf, match_kf, nmatches, 0.7f, true);
            // LSDmatcher::match(Last.mLdesc, Cur.mLdesc, 0.9) between the two resident frames
            std::vector<int32_t> m12(kl_cap, -1); int n_from = 0, n_lm = 0;
            hvo::check(hvo_stream_match_lines(fs.get(), t_kf, t, 0, 50.f, 0.9f, m12.data(), &n_from, &n_lm), "hvo_stream_match_lines");
            hvo_plane_match pm; memset(&pm, 0, sizeof(pm));
            pmatcher.SearchMapByCoefficients(fs, t, I, *pmap, pm);
            // mCurrentFrame.mvpMapPoints = vpMapPointMatches; PoseOptimization(&mCurrentFrame)
            std::vector<uint8_t> pt_has(N), ln_has(NL), out_pt(N), out_ln(NL), out_pl(3 * 64);
            std::vector<float> xyz(3 * (size_t)(N > 0 ? N : 1), 0.f); std::vector<double> lxyz(6 * (size_t)(NL > 0 ? NL : 1), 0.0);
            for (int i = 0; i < N; i++) {
                const int j = match_kf[0][i];
                pt_has[i] = j >= 0;
                if (j >= 0) for (int c = 0; c < 3; c++) xyz[3 * i + c] = kf_xyz[3 * j + c];
            }
            int nl = 0;
            for (int i = 0; i < n_from && i < NL_kf; i++) {
                const int j = m12[i];
                if (j < 0 || j >= NL || !kf_lgood[i]) continue;
                ln_has[j] = 1; nl++;
                for (int c = 0; c < 6; c++) lxyz[6 * j + c] = kf_lxyz[6 * i + c];
            }
            hvo::PoseMapSide side;
            side.n_points = N; side.n_lines = NL; side.n_planes = pm.n_planes;
            side.pt_has = pt_has.data(); side.pt_xyz = xyz.data(); side.ln_has = ln_has.data(); side.ln_xyz = lxyz.data();
            side.plane_map = pmap.get(); side.plane_match = &pm;
            side.flags.pt_outlier = out_pt.data(); side.flags.ln_outlier = out_ln.data(); side.flags.pl_outlier = out_pl.data();
            hvo_pose_result r;
            const int inliers = optimizer.PoseOptimization(fs, t, I, side, r);
            printf("frame %d: %d points (%d words), SearchByBoW %d matches, %d line matches, %d planes -> inliers %d (nBad %d nLineBad %d), t = (%.5f %.5f %.5f)\n",
                   k, N, (int)bow.bow_word.size(), nmatches[0], nl, pm.n_planes, inliers, r.n_bad, r.n_line_bad, r.Tcw[3], r.Tcw[7], r.Tcw[11]);
            if (k - k_kf >= sp.depth - 2) make_key_frame();                  // the key frame's slot is about to be reused
        }
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
