// local_map_search.cpp -- the line side of Tracking::TrackLocalMapWithLines (reference src/Tracking.cc:2816-2921) through the C++ mirror
// (include/hvo.hpp): the local map's lines stay on the device in an hvo::LineMap, and Tracking::SearchLocalLines plus
// Manhattan::computeStructConstInMap are one call on the resident frame.  RGB-D frames go through a stream with the line grid and the 3-D
// lines resident.  The first frame's good 3-D lines become the map (camera = world for that frame), the way the first key frame seeds
// mpMap; every later frame is searched against it under the identity pose.  `held` after the call is mvpMapLines as slots, and it goes
// straight on to Optimizer::PoseOptimization as the frame's line matches (ln_has[i] = held[i] >= 0, ln_xyz[i] = the slot's end points),
// the way TrackLocalMapWithLines chains the two (src/Tracking.cc:2823-2836): between "pose predicted" and "pose optimised against the
// local map" only the pose, `held` and the matched end points cross PCIe.  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/local_map_search.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o local_map_search
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
    if (argc < 5 || argc % 2 != 1) { fprintf(stderr, "usage: %s gray0.u8 depth0.u16 gray1.u8 depth1.u16 [...]\n", argv[0]); return 2; }
    const int W = 640, H = 480, n = (argc - 1) / 2;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_FRAME;                                         // the pose optimisation reads the whole Frame tail
        hvo::FrameStream fs(p, sp);
        hvo::LineMap map(p.device);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::LocalLines local(cam, logf(1.2f));
        hvo::Optimizer optimizer(cam);
        const float Tcw[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        const int cap = fs.klCap();
        std::vector<hvo_keyline> kl(cap); std::vector<uint8_t> ld((size_t)cap * 32); std::vector<double> fn((size_t)cap * 3);
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo::FrameStream::FrameTail tail;
            fs.collectTail(t, W, H, tail);
            hvo_frame_out fo = hvo_frame_out();
            fo.kl = kl.data(); fo.ldesc = ld.data(); fo.linefn = fn.data(); fo.kl_cap = cap;
            fs.collect(t, fo);                                               // the slot stays resident until `depth` newer frames were submitted
            if (k > 0) {
                const int ns = map.size(), capq = ns < 16384 ? (ns > 0 ? ns : 1) : 16384, NL = fo.n_kl;
                std::vector<int32_t> held(NL > 0 ? NL : 1, -1), in_view(capq), n_par(held.size()), n_perp(held.size());
                hvo_local_lines_io io = hvo_local_lines_io();
                io.n_kl = NL; io.held = held.data(); io.in_view_slot = in_view.data(); io.n_par = n_par.data(); io.n_perp = n_perp.data();
                hvo_local_lines_result r;
                local.SearchLocalLines(fs, t, map, Tcw, io, r);
                int nheld = 0, npar = 0, nperp = 0;
                for (int i = 0; i < NL; i++) { nheld += held[i] >= 0; npar += n_par[i]; nperp += n_perp[i]; }
                printf("frame %d: %d slots tested, %d in view, %d matched, %d gated, %d lines hold a map line; constraints: %d parallel, %d perpendicular; "
                       "kernels %.3f + %.3f + %.3f ms\n", k, r.n_slots_tested, r.n_in_view, r.n_matches, r.n_gated, nheld, npar, nperp,
                       r.kernel_ms[0], r.kernel_ms[1], r.kernel_ms[2]);
                // PoseOptimization on the same resident frame: `held` is mvpMapLines
                std::vector<uint8_t> ln_has(held.size()), out_ln(held.size()); std::vector<double> ln_xyz(6 * held.size(), 0.0);
                for (int i = 0; i < NL; i++) {
                    ln_has[i] = held[i] >= 0;
                    if (held[i] >= 0) hvo::check(hvo_line_map_slot(map.get(), held[i], &ln_xyz[6 * (size_t)i], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "hvo_line_map_slot");
                }
                hvo::PoseMapSide side;
                side.n_lines = NL; side.ln_has = ln_has.data(); side.ln_xyz = ln_xyz.data(); side.flags.ln_outlier = out_ln.data();
                hvo_pose_result pr;
                const int inliers = optimizer.PoseOptimization(fs, t, Tcw, side, pr);
                printf("frame %d: pose optimised against %d map lines -> inliers %d (nLineBad %d), iterations %d %d %d %d, t = (%.5f %.5f %.5f)\n",
                       k, nheld, inliers, pr.n_line_bad, pr.iterations[0], pr.iterations[1], pr.iterations[2], pr.iterations[3], pr.Tcw[3], pr.Tcw[7], pr.Tcw[11]);
            }
            if (k > 0) continue;
            for (int i = 0; i < fo.n_kl; i++) {                              // MapLine(pos, pKF, ...): a new slot per good 3-D line
                const hvo_line3d &L = tail.lines3d[i];
                if (!L.good) continue;
                const double pos[6] = { L.A[0], L.A[1], L.A[2], L.B[0], L.B[1], L.B[2] }, wv[3] = { L.A[0] - L.B[0], L.A[1] - L.B[1], L.A[2] - L.B[2] };
                const double mid[3] = { 0.5 * (L.A[0] + L.B[0]), 0.5 * (L.A[1] + L.B[1]), 0.5 * (L.A[2] + L.B[2]) };
                const double d = sqrt(mid[0] * mid[0] + mid[1] * mid[1] + mid[2] * mid[2]);
                const double nrm[3] = { mid[0] / d, mid[1] / d, mid[2] / d };
                map.set(map.size(), pos, wv, nrm, (float)(2.0 * d), (float)(0.5 * d), ld.data() + 32 * (size_t)i);
            }
            printf("map: %d lines\n", map.size());
        }
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
