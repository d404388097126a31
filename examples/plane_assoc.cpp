// plane_assoc.cpp -- map-plane association the way Tracking uses it on every frame (reference src/Tracking.cc:2012 / 2407 / 2827 ->
// PlaneMatcher::SearchMapByCoefficients, src/PlaneMatcher.cpp:10-68), through the C++ mirror (include/hvo.hpp).  RGB-D frames go through a
// stream with the plane tail resident.  The first frame's valid planes become the map (camera = world for that frame: their coefficients and
// voxel clouds as they are), the way the first key frame seeds mpMap; every frame is then associated against the resident map, once on the
// resident frame and once on the collected host arrays, under the identity pose.  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/plane_assoc.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o plane_assoc
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
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u;
        sp.stages = HVO_STAGE_PLANES | HVO_STAGE_PLANE_TAIL;
        hvo::FrameStream fs(p, sp);
        hvo::Context ctx(p);
        hvo::PlaneMap map(p.device);
        hvo::PlaneMatcher matcher(0.05f, 0.985f, 0.08716f, 0.9962f);          // the TUM3 settings' Plane.Association* values
        const float Tcw[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo_plane_match rd; memset(&rd, 0, sizeof(rd));
            if (k > 0) matcher.SearchMapByCoefficients(fs, t, Tcw, map, rd);   // before collect() releases the slot
            hvo::FrameStream::FrameTail tail;
            fs.collectTail(t, W, H, tail);
            hvo_frame_out fo = hvo_frame_out();
            fs.collect(t, fo);
            std::vector<float> coef;
            for (int i = 0; i < 64; i++) {
                const hvo_plane_cloud &pc = tail.plane_clouds[i];
                if (!pc.valid) continue;
                coef.insert(coef.end(), pc.coef, pc.coef + 4);
                if (k == 0) map.set(map.size(), pc.coef, tail.cloud_xyz.data() + 3 * (size_t)pc.first, pc.n_points);   // MapPlane(pKF, idx): a new slot
            }
            if (k == 0) { printf("map: %d planes, %lld points\n", map.size(), (long long)map.points()); continue; }
            hvo_plane_match rh;
            matcher.SearchMapByCoefficients(ctx.get(), coef.data(), (int)coef.size() / 4, Tcw, map, rh);
            printf("frame %d planes %d matched %d same %d:", k, rd.n_planes, rd.n_matches,
                   (int)(rd.n_planes == rh.n_planes && !memcmp(rd.match, rh.match, sizeof(rd.match)) && !memcmp(rd.dist, rh.dist, sizeof(rd.dist))));
            for (int i = 0; i < rd.n_planes; i++) printf(" [%d: map %d ver %d par %d d %.4f]", rd.plane_idx[i], rd.match[i], rd.vertical[i], rd.parallel[i], rd.dist[i]);
            printf("\n");
        }
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
