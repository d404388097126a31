// local_map_points.cpp -- the point side of Tracking::TrackLocalMapWithLines (reference src/Tracking.cc:2816-2921) through the C++ mirror
// (include/hvo.hpp): the local map's points stay on the device in an hvo::PointMap, and Tracking::SearchLocalPoints is one call on the
// resident frame.  An RGB-D frame goes through a stream; its own key points with depth, unprojected through the depth (camera = world),
// become the map, the way the first key frame seeds mpMap; the same resident frame is then searched against it under the identity pose
// and the matches are printed.  `held` after the call is mvpMapPoints as slots.  Reads one raw 640x480 gray (u8) + depth (u16) pair.
//
// build:  g++ -std=c++14 -Iinclude examples/local_map_points.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o local_map_points
#include <cmath>
#include <cstdio>
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
    if (argc != 3) { fprintf(stderr, "usage: %s gray.u8 depth.u16\n", argv[0]); return 2; }
    const int W = 640, H = 480;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    if (!read_raw(argv[1], gray.data(), gray.size()) || !read_raw(argv[2], depth.data(), depth.size() * 2)) return 3;
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_ORB;
        hvo::FrameStream fs(p, sp);
        hvo::PointMap map(p.device);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::LocalPoints local(cam, logf(p.orb_scale_factor), p.orb_nlevels);
        const float Tcw[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        const int cap = fs.kpCap();
        std::vector<hvo_keypoint> kp(cap), kpu(cap); std::vector<uint8_t> desc((size_t)cap * 32); std::vector<float> ur(cap), z(cap);
        const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
        hvo_frame_out fo = hvo_frame_out();
        fo.kp = kp.data(); fo.desc = desc.data(); fo.kp_cap = cap;
        fs.collect(t, fo, kpu.data(), ur.data(), z.data());              // the slot stays resident until `depth` newer frames were submitted
        const int N = fo.n_kp;
        // MapPoint(x3D, pKF, ...): a slot per key point with depth; mfMaxDistance = dist * scale(octave), a little inside the level boundary
        std::vector<int> slot_of(N, -1);
        for (int i = 0; i < N; i++) {
            if (!(z[i] > 0)) continue;
            const float X[3] = { (kpu[i].x - p.cx) / p.fx * z[i], (kpu[i].y - p.cy) / p.fy * z[i], z[i] };
            const float d = sqrtf(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
            const float nrm[3] = { X[0] / d, X[1] / d, X[2] / d };
            const float maxd = d * powf(p.orb_scale_factor, (float)kpu[i].octave - 0.5f), mind = maxd / powf(p.orb_scale_factor, (float)(p.orb_nlevels - 1));
            slot_of[i] = map.size();
            map.set(map.size(), X, nrm, maxd, mind, desc.data() + 32 * (size_t)i);
        }
        const int ns = map.size(), capq = ns < 16384 ? (ns > 0 ? ns : 1) : 16384;
        std::vector<int32_t> held(N > 0 ? N : 1, -1), in_view(capq), match_idx(capq), match_dist(capq);
        hvo_local_points_io io = hvo_local_points_io();
        io.n_kp = N; io.held = held.data(); io.in_view_slot = in_view.data(); io.match_idx = match_idx.data(); io.match_dist = match_dist.data();
        hvo_local_points_result r;
        local.SearchLocalPoints(fs, t, map, Tcw, io, r, 3.0f);           // th = 3: RGB-D
        int own = 0;
        for (int i = 0; i < N; i++) own += held[i] >= 0 && held[i] == slot_of[i];
        printf("map: %d points of %d key points; %d slots tested, %d in view, %d matched (%d features hold their own point); kernels %.3f + %.3f + %.3f ms\n",
               ns, N, r.n_slots_tested, r.n_in_view, r.n_matches, own, r.kernel_ms[0], r.kernel_ms[1], r.kernel_ms[2]);
        for (int q = 0; q < r.n_in_view && q < 10; q++)
            printf("  slot %d -> feature %d (distance %d)\n", in_view[q], match_idx[q], match_dist[q]);
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
