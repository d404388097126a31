// relocalization_refine.cpp -- the refinement block of Tracking::Relocalization (reference src/Tracking.cc:3840-3907) end to end on a resident
// frame through the C++ mirror (include/hvo.hpp), with the reference's thresholds (10, 50, 30):
//   PoseOptimization -> clear the outliers -> SearchByProjection(mCurrentFrame, pKF, sFound, 10, 100) -> PoseOptimization
//   -> rebuild sFound -> SearchByProjection(mCurrentFrame, pKF, sFound, 3, 64) -> PoseOptimization -> clear the outliers
// Between the frame's upload and the final pose nothing of the frame comes down for the loop: key points, descriptors and the feature grid
// stay on the device; per call the key frame's arrays, the skip and occupancy bytes go up and the match vectors come back.
// The frame plays its own candidate key frame (camera = world: 70 of its features with depth are the key frame's map points).  The loop starts
// where PnP would leave it: a planted pose a few centimetres off and a thinned inlier set (24 right and 12 wrong matches).
// Reads one raw 640x480 gray (u8) + depth (u16) pair.
//
// build:  g++ -std=c++14 -Iinclude examples/relocalization_refine.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o relocalization_refine
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s frame.u8 frame.u16\n", argv[0]); return 2; }
    const int W = 640, H = 480;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    if (!read_raw(argv[1], gray.data(), gray.size()) || !read_raw(argv[2], depth.data(), depth.size() * 2)) return 3;
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_FRAME;
        hvo::FrameStream fs(p, sp);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::Optimizer optimizer(cam);
        hvo::ORBmatcher matcher2(nullptr);                         // ORBmatcher matcher2(0.9, true): the stream form needs no context
        const int kp_cap = fs.kpCap();
        std::vector<hvo_keypoint> kp(kp_cap), kpu(kp_cap); std::vector<float> ur(kp_cap), zd(kp_cap); std::vector<uint8_t> desc((size_t)kp_cap * 32);
        std::vector<hvo_keyline> kl(fs.klCap());
        const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
        hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.desc = desc.data(); fo.kp_cap = kp_cap; fo.kl = kl.data(); fo.kl_cap = fs.klCap();
        fs.collect(t, fo, kpu.data(), ur.data(), zd.data());
        const int N = fo.n_kp, NL = fo.n_kl;
        // The candidate key frame as the host keeps it: GetWorldPos(), mfMaxDistance / mfMinDistance as MapPoint::UpdateNormalAndDepth forms
        // them (dist * mvScaleFactors[level], / mvScaleFactors[nLevels - 1]), GetDescriptor(), mvKeysUn[i].angle.  It holds 70 map points, spread
        // over the frame's features with depth, in four roles chosen so that every branch of the block runs with the reference's thresholds:
        //   24 that PnP matched correctly                     -> the start inliers
        //   12 that PnP matched to a WRONG feature            -> outliers of the first optimisation, cleared, but still in sFound: the (10, 100)
        //                                                        search skips them; the rebuilt sFound no longer holds them, (3, 64) finds them
        //   22 PnP did not match                              -> found by the (10, 100) search
        //   12 PnP did not match, their position 6 px (times the level's scale) off -> found by (10, 100), outliers of the second optimisation
        float sf[16]; sf[0] = 1.f;
        for (int l = 1; l < 16; l++) sf[l] = sf[l - 1] * p.orb_scale_factor;
        const int Ne = N > 0 ? N : 1;
        std::vector<float> xyz(3 * (size_t)Ne, 0.f), maxd(Ne, 0.f), mind(Ne, 0.f), angle(Ne, 0.f);
        std::vector<uint8_t> none(Ne, 1);                          // !pMP: a key-frame feature without a map point
        std::vector<int> mvpMapPoints(Ne, -1);                     // per frame feature: the key-frame entry it holds, -1 = NULL
        std::vector<int> withDepth;
        for (int i = 0; i < N; i++) if (zd[i] > 0) withDepth.push_back(i);
        const int nChosen = 70, stride = (int)withDepth.size() / nChosen;
        if (stride < 2) { printf("too few points with depth (%d)\n", (int)withDepth.size()); printf("final: 0 inliers\n"); return 0; }
        static const char roles[35 + 1] = "ssWhsBhsWhsBhBsWhshsBhWshsBhWshsBhW";      // s start, W wrong start, h hidden, B hidden and off; 12 + 6 + 11 + 6
        std::vector<uint8_t> chosen(Ne, 0);
        for (int k = 0; k < nChosen; k++) chosen[withDepth[(size_t)k * stride]] = 1;
        int nStart = 0, nWrong = 0, nHidden = 0, nOff = 0;
        for (int k = 0; k < nChosen; k++) {
            const int i = withDepth[(size_t)k * stride];
            const char role = roles[k % 35];
            const float z = zd[i];
            float *X = &xyz[3 * (size_t)i];
            X[0] = (kpu[i].x - p.cx) / p.fx * z; X[1] = (kpu[i].y - p.cy) / p.fy * z; X[2] = z;
            if (role == 'B') { X[0] += 6.f * sf[kpu[i].octave] * z / p.fx; nOff++; }
            const float dist = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
            maxd[i] = dist * sf[kpu[i].octave]; mind[i] = maxd[i] / sf[p.orb_nlevels - 1];
            angle[i] = kpu[i].angle; none[i] = 0;
            if (role == 's') { mvpMapPoints[i] = i; nStart++; }
            else if (role == 'h') nHidden++;
            else if (role == 'W') {                                // a feature of the frame that is no map point's and lies far from the right one
                int w = (i + N / 2) % N;
                while (chosen[w] || mvpMapPoints[w] >= 0 || std::fabs(kpu[w].x - kpu[i].x) + std::fabs(kpu[w].y - kpu[i].y) < 100.f) w = (w + 1) % N;
                mvpMapPoints[w] = i; nWrong++;
            }
        }
        hvo::KeyFrameSide kf; kf.n = N; kf.pos = xyz.data(); kf.max_dist = maxd.data(); kf.min_dist = mind.data(); kf.desc = desc.data(); kf.angle = angle.data();
        // where PnP would leave the loop: Tcw a few centimetres off the truth (the identity: camera = world)
        float Tcw[12] = { 1, 0, 0, 0.02f, 0, 1, 0, -0.01f, 0, 0, 1, 0.015f };
        printf("frame: %d points, %d with depth; key frame: %d map points; start: %d inliers and %d wrong matches, %d unmatched, %d unmatched and off\n", N,
               (int)withDepth.size(), nChosen, nStart, nWrong, nHidden, nOff);

        std::vector<uint8_t> pt_has(Ne), out_pt(Ne), ln_has(NL > 0 ? NL : 1, 0), out_ln(NL > 0 ? NL : 1), out_pl(3 * 64), skip(Ne), occupied(Ne);
        std::vector<float> pt_xyz(3 * (size_t)Ne, 0.f); std::vector<double> ln_xyz(6 * (size_t)(NL > 0 ? NL : 1), 0.0);
        auto optimise = [&]() {                                    // nGood = Optimizer::PoseOptimization(&mCurrentFrame); SetPose
            for (int j = 0; j < N; j++) {
                const int m = mvpMapPoints[j];
                pt_has[j] = m >= 0; out_pt[j] = 0;
                for (int q = 0; q < 3; q++) pt_xyz[3 * (size_t)j + q] = m >= 0 ? xyz[3 * (size_t)m + q] : 0.f;
            }
            hvo::PoseMapSide side;
            side.n_points = N; side.n_lines = NL; side.n_planes = 0;
            side.pt_has = pt_has.data(); side.pt_xyz = pt_xyz.data(); side.ln_has = ln_has.data(); side.ln_xyz = ln_xyz.data();
            side.flags.pt_outlier = out_pt.data(); side.flags.ln_outlier = out_ln.data(); side.flags.pl_outlier = out_pl.data();
            hvo_pose_result r;
            const int nGood = optimizer.PoseOptimization(fs, t, Tcw, side, r);
            memcpy(Tcw, r.Tcw, sizeof(Tcw));
            return nGood;
        };
        auto clear_outliers = [&]() { for (int io = 0; io < N; io++) if (mvpMapPoints[io] >= 0 && out_pt[io]) mvpMapPoints[io] = -1; };
        auto search = [&](float th, int ORBdist) {                 // matcher2.SearchByProjection(mCurrentFrame, pKF, sFound, th, ORBdist)
            hvo::KeyFrameMatches res;
            for (int j = 0; j < N; j++) occupied[j] = mvpMapPoints[j] >= 0;
            const int nadditional = matcher2.SearchByProjection(fs, t, cam, Tcw, kf, skip.data(), occupied.data(), N, th, ORBdist, res);
            for (int j = 0; j < N; j++) if (res.feature_kf[j] >= 0) mvpMapPoints[j] = res.feature_kf[j];
            printf("search (%g, %d): %d additional of %d searched (prologue %.3f ms, search %.3f ms)\n", th, ORBdist, nadditional, res.n_searched,
                   res.kernel_ms[0], res.kernel_ms[1]);
            return nadditional;
        };
        // set<MapPoint*> sFound: the inliers PnP handed over (3844-3857), as a skip byte per key-frame entry
        for (int i = 0; i < N; i++) skip[i] = none[i];
        for (int j = 0; j < N; j++) if (mvpMapPoints[j] >= 0) skip[mvpMapPoints[j]] = 1;
        int nGood = optimise();
        printf("PoseOptimization: %d good, t = (%.5f %.5f %.5f)\n", nGood, Tcw[3], Tcw[7], Tcw[11]);
        if (nGood < 10) { printf("final: %d inliers\n", nGood); return 0; }
        clear_outliers();
        if (nGood < 50) {
            int nadditional = search(10.f, 100);
            if (nadditional + nGood >= 50) {
                nGood = optimise();
                printf("PoseOptimization: %d good, t = (%.5f %.5f %.5f)\n", nGood, Tcw[3], Tcw[7], Tcw[11]);
                if (nGood > 30 && nGood < 50) {
                    for (int i = 0; i < N; i++) skip[i] = none[i];                                  // sFound.clear(); insert what the frame holds
                    for (int ip = 0; ip < N; ip++) if (mvpMapPoints[ip] >= 0) skip[mvpMapPoints[ip]] = 1;
                    nadditional = search(3.f, 64);
                    if (nGood + nadditional >= 50) {
                        nGood = optimise();
                        printf("PoseOptimization: %d good, t = (%.5f %.5f %.5f)\n", nGood, Tcw[3], Tcw[7], Tcw[11]);
                        clear_outliers();
                    }
                }
            }
        }
        printf("final: %d inliers%s\n", nGood, nGood >= 50 ? ": relocalised" : "");
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
