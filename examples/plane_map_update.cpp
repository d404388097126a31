// plane_map_update.cpp -- the per-frame plane chain of Tracking::Track() with the map's clouds resident (reference src/Tracking.cc:2012-2026
// and :796-804): associate the frame's planes with the map (PlaneMatcher::SearchMapByCoefficients), optimise the pose on the plane edges
// (Optimizer::PoseOptimization), take every matched plane's cloud into its map plane (MapPlane::UpdateCoefficientsAndPoints), and associate
// again against the updated map -- the host handles no cloud in between.  The first frame seeds the map the way CreateNewKeyFrame does:
// every valid plane is inserted under Twc.  Reads raw 640x480 gray (u8) + depth (u16) pairs, two frames or more.
//
// build:  g++ -std=c++14 -Iinclude examples/plane_map_update.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o plane_map_update
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
        sp.stages = HVO_STAGE_FRAME;
        hvo::FrameStream fs(p, sp);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        hvo::Optimizer optimizer(cam);
        hvo::PlaneMatcher matcher(0.05f, 0.985f, 0.08716f, 0.9962f);          // the TUM3 settings' Plane.Association* values
        hvo::PlaneMap map(p.device);
        float Tcw[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };               // the first frame is the world
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo_plane_match pm; memset(&pm, 0, sizeof(pm));
            matcher.SearchMapByCoefficients(fs, t, Tcw, map, pm);
            if (k == 0) {                                                      // CreateNewKeyFrame: a new MapPlane per valid plane
                for (int i = 0; i < pm.n_planes; i++) map.insert(fs, t, Tcw, Tcw, i, map.size());   // (Twc = Tcw = identity here)
                printf("map: %d planes, %lld points\n", map.size(), (long long)map.points());
            } else {
                // the plane edges alone: no map points or lines are held in this example
                hvo::PoseMapSide side;
                std::vector<uint8_t> out_pl(3 * 64);
                side.n_planes = pm.n_planes; side.plane_map = &map; side.plane_match = &pm; side.flags.pl_outlier = out_pl.data();
                hvo_pose_result r;
                const int inliers = optimizer.PoseOptimization(fs, t, Tcw, side, r);
                for (int i = 0; i < 12; i++) Tcw[i] = r.Tcw[i];
                const long long before = (long long)map.points();
                bool newPlane = false;
                hvo_plane_update_result ur;
                // (the optimiser's pl_outlier holds three bytes per plane: mvbPlaneOutlier is the first of each triple)
                const int done = map.UpdateCoefficientsAndPoints(fs, t, Tcw, pm, out_pl.data(), newPlane, hvo::PlaneMap::kPoseFlagsPlaneStride, &ur);
                hvo_plane_match again; memset(&again, 0, sizeof(again));
                matcher.SearchMapByCoefficients(fs, t, Tcw, map, again);
                printf("frame %d planes %d matched %d inliers %d updated %d points %lld -> %lld newPlane %d rematched %d t = (%.5f %.5f %.5f)\n",
                       k, pm.n_planes, pm.n_matches, inliers, done, before, (long long)map.points(), (int)newPlane, again.n_matches, Tcw[3], Tcw[7], Tcw[11]);
            }
            hvo_frame_out fo = hvo_frame_out();
            fs.collect(t, fo);
        }
        const std::vector<float> xyz = map.size() ? map.points(0) : std::vector<float>();
        printf("slot 0: %d points\n", (int)xyz.size() / 3);
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
