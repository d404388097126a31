// line_opt.cpp -- the per-frame step between the Frame constructor and Track() the way Tracking::GrabImageRGBD_wh runs it (reference
// src/Tracking.cc:270-335), through the C++ mirror (include/hvo.hpp), chained on ONE resident frame: structural constraints of every key
// line -> LineOptStruct (the resident 3-D lines are rewritten) -> Optimizer::PoseOptimization, whose vanishing-direction edges then measure
// the optimised lines.  The frame is synthetic: bright rectangles on a dark wall 2 m away, seen head-on, so its lines fall into two
// orthogonal families.  Only the relation matrix, the end points and the pose cross PCIe.
//
// build:  g++ -std=c++14 -Iinclude examples/line_opt.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o line_opt
#include <cstdio>
#include <cstring>
#include <vector>
#include "hvo.hpp"

int main()
{
    const int W = 640, H = 480;
    std::vector<uint8_t> gray((size_t)W * H, 40); std::vector<uint16_t> depth((size_t)W * H);
    for (int v = 0; v < H; v++) for (int u = 0; u < W; u++) {
        const int cu = u / 80, cv = v / 80, lu = u % 80, lv = v % 80;
        if (lu > 12 && lu < 68 && lv > 12 && lv < 68) gray[(size_t)v * W + u] = (uint8_t)(120 + 15 * ((cu + 2 * cv) % 8));
        depth[(size_t)v * W + u] = (uint16_t)(10000 + ((u * 7 + v * 13) % 41) - 20);      // 2 m at 5000 per metre, a few millimetres of noise
    }
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_FRAME;
        hvo::FrameStream fs(p, sp);
        int kp_cap = 0, kl_cap = 0, pl_cap = 0;
        hvo::check(hvo_stream_capacity(fs.get(), &kp_cap, &kl_cap, &pl_cap), "hvo_stream_capacity");
        const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
        hvo::FrameStream::FrameTail tail;
        fs.collectTail(t, W, H, tail);
        std::vector<hvo_keypoint> kp(kp_cap), kpu(kp_cap); std::vector<float> ur(kp_cap), zd(kp_cap); std::vector<hvo_keyline> kl(kl_cap);
        hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.kp_cap = kp_cap; fo.kl = kl.data(); fo.kl_cap = kl_cap;
        fs.collect(t, fo, kpu.data(), ur.data(), zd.data());
        const int N = fo.n_kp, NL = fo.n_kl;

        hvo::FrameLines lines;
        hvo::Manhattan::computeStructConstrains(fs, t, NL, lines);                      // the loop at Tracking.cc:270-293
        size_t npar = 0, nperp = 0;
        for (int k = 0; k < NL; k++) { npar += lines.mvParLinesIdx[k].size(); nperp += lines.mvPerpLinesIdx[k].size(); }
        hvo::LineOptStruct(fs, t, NL, lines);                                           // Tracking.cc:331
        const hvo_line_opt_result &r = lines.res;
        double moved = 0;
        for (int i = 0; i < NL; i++) for (int j = 0; j < 3; j++) {
            const double a = lines.mvLines3D[6 * (size_t)i + j] - tail.lines3d[i].A[j], b = lines.mvLines3D[6 * (size_t)i + 3 + j] - tail.lines3d[i].B[j];
            moved = a > moved ? a : (-a > moved ? -a : moved); moved = b > moved ? b : (-b > moved ? -b : moved);
        }
        printf("%d key lines: %zu parallel and %zu perpendicular list entries; %d lines optimised over %d edges, rounds %d, iterations %d %d, flagged %d %d, "
               "written back %d, largest end-point move %.4f m\n", NL, npar, nperp, r.n_lines_to_opt, r.n_edges, r.rounds, r.iterations[0], r.iterations[1],
               r.n_flagged[0], r.n_flagged[1], r.written_back, moved);

        // the frame is its own map under the identity pose; the optimisation starts a degree and a few centimetres off
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::Optimizer optimizer(cam);
        std::vector<uint8_t> pt_has(N), ln_has(NL); std::vector<float> xyz(3 * (size_t)N); std::vector<double> lxyz(6 * (size_t)NL);
        for (int i = 0; i < N; i++) {
            pt_has[i] = zd[i] > 0; const float z = zd[i] > 0 ? zd[i] : 1.f;
            xyz[3 * i] = (kpu[i].x - p.cx) / p.fx * z; xyz[3 * i + 1] = (kpu[i].y - p.cy) / p.fy * z; xyz[3 * i + 2] = z;
        }
        for (int i = 0; i < NL; i++) { ln_has[i] = tail.lines3d[i].good != 0; for (int j = 0; j < 6; j++) lxyz[6 * (size_t)i + j] = lines.mvLines3D[6 * (size_t)i + j]; }
        hvo::PoseMapSide side;
        side.n_points = N; side.n_lines = NL; side.n_planes = 0;
        side.pt_has = pt_has.data(); side.pt_xyz = xyz.data(); side.ln_has = ln_has.data(); side.ln_xyz = lxyz.data();
        const float c = 0.99984770f, s = 0.01745241f;
        const float T0[12] = { c, 0, s, 0.03f, 0, 1, 0, -0.02f, -s, 0, c, 0.04f };
        hvo_pose_result pr;
        const int inliers = optimizer.PoseOptimization(fs, t, T0, side, pr);
        printf("pose optimisation on the optimised lines: %d points, %d lines -> inliers %d, t = (%.5f %.5f %.5f)\n", N, NL, inliers, pr.Tcw[3], pr.Tcw[7], pr.Tcw[11]);
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
