// relocalization_pnp.cpp -- the loop of Tracking::Relocalization (reference src/Tracking.cc:3789-3909) on a resident frame through the C++
// mirror (include/hvo.hpp): mCurrentFrame.ComputeBoW(), ORBmatcher::SearchByBoW against EVERY candidate key frame in one call, one
// hvo::PnPsolver per candidate filled by ONE device call (PnPsolver::solve_candidates -> hvo_stream_pnp_ransac), the round-robin
// `iterate(5, bNoMore, vbInliers, nInliers)` loop as a host replay, and Optimizer::PoseOptimization with the accepted candidate's inliers.
// The frames but the last play the candidate key frames (camera = world for each: its features with depth are its map points); the last
// frame is the one to relocalise.  Between its upload and the optimised pose only the key frames' arrays, the match vectors and the matched
// positions cross PCIe.  The candidate query (DetectRelocalizationCandidates) is examples/keyframe_db.cpp; SearchByProjection(Frame, KeyFrame, ...) and
// the optimisations around it are examples/relocalization_refine.cpp.  Neither is part of this example.  No vocabulary file is needed: a small random k = 8, L = 3 tree is generated.
// Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/relocalization_pnp.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o relocalization_pnp
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
    if (argc < 5 || argc % 2 != 1) { fprintf(stderr, "usage: %s kf0.u8 kf0.u16 [kf1.u8 kf1.u16 ...] frame.u8 frame.u16\n", argv[0]); return 2; }
    const int W = 640, H = 480, n = (argc - 1) / 2, nKFs = n - 1;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_FRAME;
        hvo::FrameStream fs(p, sp);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::Optimizer optimizer(cam);
        std::vector<int32_t> vp; std::vector<uint8_t> vl, vd; std::vector<double> vw;
        make_vocabulary(8, 3, vp, vl, vd, vw);
        hvo::ORBVocabulary voc(p.device, 8, 3, HVO_VOC_L1_NORM, HVO_VOC_TF_IDF, (int)vp.size(), vp.data(), vl.data(), vd.data(), vw.data());
        const int levelsup = 1, kp_cap = fs.kpCap();
        // the candidate key frames, as the host keeps them: descriptors, node ids, angles, world positions (camera = world), a bad-point byte
        struct KF { int N; std::vector<uint8_t> desc, has, bad; std::vector<float> angle, xyz; hvo::BowVectors bow; };
        std::vector<KF> kfs(nKFs);
        int64_t t = -1; int N = 0, NL = 0;
        std::vector<hvo_keypoint> kp(kp_cap), kpu(kp_cap); std::vector<float> ur(kp_cap), zd(kp_cap); std::vector<uint8_t> desc((size_t)kp_cap * 32);
        std::vector<hvo_keyline> kl(fs.klCap());
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.desc = desc.data(); fo.kp_cap = kp_cap; fo.kl = kl.data(); fo.kl_cap = fs.klCap();
            fs.collect(t, fo, kpu.data(), ur.data(), zd.data());
            N = fo.n_kp; NL = fo.n_kl;
            if (k == nKFs) break;                                             // the frame to relocalise stays resident
            KF &K = kfs[k];
            hvo::Frame::ComputeBoW(fs, t, voc, K.bow, levelsup);               // KeyFrame::ComputeBoW
            K.N = N; K.desc = desc; K.has.assign(N, 0); K.bad.assign(N, 0); K.angle.assign(N, 0.f); K.xyz.assign(3 * (size_t)(N > 0 ? N : 1), 0.f);
            for (int i = 0; i < N; i++) {
                K.has[i] = zd[i] > 0; K.bad[i] = !(zd[i] > 0); K.angle[i] = kpu[i].angle;
                const float z = zd[i] > 0 ? zd[i] : 1.f;
                K.xyz[3 * i] = (kpu[i].x - p.cx) / p.fx * z; K.xyz[3 * i + 1] = (kpu[i].y - p.cy) / p.fy * z; K.xyz[3 * i + 2] = z;
            }
            printf("candidate %d: %d points (%d words)\n", k, N, (int)K.bow.bow_word.size());
        }
        // mCurrentFrame.ComputeBoW(); matcher(0.75, true).SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]) for every candidate (:3789-3803)
        hvo::BowVectors bow;
        hvo::Frame::ComputeBoW(fs, t, voc, bow, levelsup);
        std::vector<hvo_bow_keyframe> bk(nKFs);
        for (int i = 0; i < nKFs; i++) bk[i] = hvo_bow_keyframe{ kfs[i].desc.data(), kfs[i].bow.node_id.data(), kfs[i].has.data(), kfs[i].angle.data(), kfs[i].N };
        std::vector<std::vector<int>> match_kf; std::vector<int> nmatches;
        hvo::Frame::SearchByBoW(fs, t, voc, nKFs, bk.data(), match_kf, nmatches, 0.75f, true);
        // PnPsolver *pSolver = new PnPsolver(mCurrentFrame, vvpMapPointMatches[i]); pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) (:3804-3808):
        // candidates with fewer than 15 matches are discarded, the others are solved in ONE call
        std::vector<bool> vbDiscarded(nKFs, false);
        std::vector<int> live; std::vector<hvo_pnp_keyframe_side> sides; std::vector<std::vector<int32_t>> mk(nKFs);
        for (int i = 0; i < nKFs; i++) {
            if (nmatches[i] < 15) { vbDiscarded[i] = true; continue; }
            mk[i].assign(match_kf[i].begin(), match_kf[i].end()); mk[i].resize(kp_cap, -1);
            live.push_back(i); sides.push_back(hvo_pnp_keyframe_side{ mk[i].data(), kfs[i].xyz.data(), kfs[i].bad.data(), kfs[i].N });
        }
        int nCandidates = (int)live.size();
        printf("frame: %d points, %d of %d candidates with >= 15 matches\n", N, nCandidates, nKFs);
        if (!nCandidates) { printf("relocalisation failed: no candidate\n"); return 0; }
        std::vector<hvo::PnPsolver> solvers(live.size());
        solvers[0].SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
        hvo::PnPsolver::solve_candidates(fs, t, cam, sides, solvers);
        float ms2[2] = { 0.f, 0.f };
        hvo::check(hvo_stream_pnp_last_kernel_ms(fs.get(), t, ms2), "hvo_stream_pnp_last_kernel_ms");
        // the round-robin loop (:3834-3909): five RANSAC iterations per candidate per round until one is accepted
        bool bMatch = false; int accepted = -1;
        std::vector<bool> done(live.size(), false);
        while (nCandidates > 0 && !bMatch) {
            for (size_t c = 0; c < live.size() && !bMatch; c++) {
                if (done[c]) continue;
                std::vector<bool> vbInliers; int nInliers; bool bNoMore; float Tcw[12];
                const bool have = solvers[c].iterate(5, bNoMore, vbInliers, nInliers, Tcw);
                if (bNoMore) { done[c] = true; nCandidates--; }
                if (!have) continue;
                // mCurrentFrame.mvpMapPoints[j] = vvpMapPointMatches[i][j] for the inliers; nGood = Optimizer::PoseOptimization(&mCurrentFrame)
                const int i = live[c];
                std::vector<uint8_t> pt_has(N), ln_has(NL > 0 ? NL : 1), out_pt(N), out_ln(NL > 0 ? NL : 1), out_pl(3 * 64);
                std::vector<float> xyz(3 * (size_t)(N > 0 ? N : 1), 0.f); std::vector<double> lxyz(6 * (size_t)(NL > 0 ? NL : 1), 0.0);
                for (int j = 0; j < N; j++) {
                    const int m = match_kf[i][j];
                    pt_has[j] = vbInliers[j] && m >= 0;
                    if (pt_has[j]) for (int q = 0; q < 3; q++) xyz[3 * j + q] = kfs[i].xyz[3 * m + q];
                }
                hvo::PoseMapSide side;
                side.n_points = N; side.n_lines = NL; side.n_planes = 0;
                side.pt_has = pt_has.data(); side.pt_xyz = xyz.data(); side.ln_has = ln_has.data(); side.ln_xyz = lxyz.data();
                side.flags.pt_outlier = out_pt.data(); side.flags.ln_outlier = out_ln.data(); side.flags.pl_outlier = out_pl.data();
                hvo_pose_result r;
                const int nGood = optimizer.PoseOptimization(fs, t, Tcw, side, r);
                printf("candidate %d at iteration %d: PnP %d inliers, PoseOptimization %d good, t = (%.5f %.5f %.5f)\n", i, solvers[c].mnIterations, nInliers, nGood,
                       r.Tcw[3], r.Tcw[7], r.Tcw[11]);
                if (nGood < 10) continue;
                // (nGood < 50: SearchByProjection(mCurrentFrame, vpCandidateKFs[i], ...) would widen the match set here: examples/relocalization_refine.cpp)
                bMatch = true; accepted = i;
            }
        }
        if (bMatch) printf("relocalised against candidate %d (hypothesis kernels %.3f ms, refine kernels %.3f ms)\n", accepted, ms2[0], ms2[1]);
        else printf("relocalisation failed: no candidate accepted\n");
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
