// pose_opt.cpp -- the motion-only pose optimisation the way Tracking uses it after every association step (reference src/Tracking.cc:2026 /
// 2418 / 2836 -> Optimizer::PoseOptimization, src/Optimizer.cc:590-1478), through the C++ mirror (include/hvo.hpp).  RGB-D frames go through
// a stream with the whole Frame tail resident.  Every frame is its own map here: its key points with a depth, back-projected under the identity
// pose, are the map points; its good 3-D lines the map lines; its valid planes, set into a PlaneMap and associated by PlaneMatcher, the map
// planes (passed on as slots).  The optimisation starts from a pose a few centimetres and a degree off and must come back to the identity:
// only the pose and these map-side arrays cross PCIe.  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/pose_opt.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o pose_opt
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
    if (argc < 3 || argc % 2 != 1) { fprintf(stderr, "usage: %s gray0.u8 depth0.u16 [gray1.u8 depth1.u16 ...]\n", argv[0]); return 2; }
    const int W = 640, H = 480, n = (argc - 1) / 2;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_FRAME;
        hvo::FrameStream fs(p, sp);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::Optimizer optimizer(cam);
        hvo::PlaneMatcher matcher(0.05f, 0.985f, 0.08716f, 0.9962f);
        int kp_cap = 0, kl_cap = 0, pl_cap = 0;
        hvo::check(hvo_stream_capacity(fs.get(), &kp_cap, &kl_cap, &pl_cap), "hvo_stream_capacity");
        const float I[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        const float c = 0.99984770f, s = 0.01745241f;                          // one degree about y, 3 / 2 / 4 cm
        const float T0[12] = { c, 0, s, 0.03f, 0, 1, 0, -0.02f, -s, 0, c, 0.04f };
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo::FrameStream::FrameTail tail;
            fs.collectTail(t, W, H, tail);
            std::vector<hvo_keypoint> kp(kp_cap), kpu(kp_cap); std::vector<float> ur(kp_cap), zd(kp_cap);
            std::vector<hvo_keyline> kl(kl_cap);
            hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.kp_cap = kp_cap; fo.kl = kl.data(); fo.kl_cap = kl_cap;
            fs.collect(t, fo, kpu.data(), ur.data(), zd.data());               // the slot stays resident until `depth` newer frames were submitted
            hvo::PlaneMap map(p.device);
            int m = 0;
            for (int i = 0; i < 64; i++) {
                const hvo_plane_cloud &pc = tail.plane_clouds[i];
                if (pc.valid) { map.set(map.size(), pc.coef, tail.cloud_xyz.data() + 3 * (size_t)pc.first, pc.n_points); m++; }
            }
            hvo_plane_match pm; memset(&pm, 0, sizeof(pm));
            matcher.SearchMapByCoefficients(fs, t, I, map, pm);
            hvo::PoseMapSide side;
            const int N = fo.n_kp, NL = fo.n_kl;
            std::vector<uint8_t> pt_has(N), ln_has(NL), out_pt(N), out_ln(NL), out_pl(3 * 64);
            std::vector<float> xyz(3 * (size_t)N); std::vector<double> lxyz(6 * (size_t)NL);
            for (int i = 0; i < N; i++) {
                pt_has[i] = zd[i] > 0;
                const float z = zd[i] > 0 ? zd[i] : 1.f;
                xyz[3 * i] = (kpu[i].x - p.cx) / p.fx * z; xyz[3 * i + 1] = (kpu[i].y - p.cy) / p.fy * z; xyz[3 * i + 2] = z;
            }
            for (int i = 0; i < NL; i++) {
                ln_has[i] = tail.lines3d[i].good != 0;
                for (int j = 0; j < 3; j++) { lxyz[6 * i + j] = tail.lines3d[i].A[j]; lxyz[6 * i + 3 + j] = tail.lines3d[i].B[j]; }
            }
            side.n_points = N; side.n_lines = NL; side.n_planes = pm.n_planes;
            side.pt_has = pt_has.data(); side.pt_xyz = xyz.data(); side.ln_has = ln_has.data(); side.ln_xyz = lxyz.data();
            side.plane_map = &map; side.plane_match = &pm;
            side.flags.pt_outlier = out_pt.data(); side.flags.ln_outlier = out_ln.data(); side.flags.pl_outlier = out_pl.data();
            hvo_pose_result r;
            const int inliers = optimizer.PoseOptimization(fs, t, T0, side, r);
            printf("frame %d: %d points %d lines %d planes -> inliers %d (nBad %d nLineBad %d), iterations %d %d %d %d, t = (%.5f %.5f %.5f), R00 %.6f R02 %.6f\n",
                   k, N, NL, pm.n_planes, inliers, r.n_bad, r.n_line_bad, r.iterations[0], r.iterations[1], r.iterations[2], r.iterations[3],
                   r.Tcw[3], r.Tcw[7], r.Tcw[11], r.Tcw[0], r.Tcw[2]);
        }
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
