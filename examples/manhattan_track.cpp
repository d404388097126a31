// manhattan_track.cpp -- Manhattan-frame tracking the way Tracking::Track uses it on every frame (reference src/Tracking.cc:706-718 ->
// TrackManhattanFrame, 1172-1348), through the C++ mirror (include/hvo.hpp).  RGB-D frames go through a stream with the surface normals and
// the 3-D lines resident; hvo::ManhattanTracking threads mLastRcm from frame to frame on the resident frames, a second one does the same on
// the collected host arrays, and the two rotations are printed.  mLastRcm starts at the identity (the reference seeds it with
// Map::FindManhattan's Rotation_cm, which stays on the host).  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/manhattan_track.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o manhattan_track
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
        sp.stages = HVO_STAGE_LSD | HVO_STAGE_PLANES | HVO_STAGE_LINES3D | HVO_STAGE_PLANE_TAIL;
        hvo::FrameStream fs(p, sp);
        hvo::Context ctx(p);
        const float I[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        hvo::ManhattanTracking on_device(ctx.get(), I), on_host(ctx.get(), I);
        std::vector<hvo_keyline> kl(fs.klCap());
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            const hvo_mf_result rd = on_device.TrackManhattanFrame(fs, t);       // before collect() releases the slot
            hvo::FrameStream::FrameTail tail;
            fs.collectTail(t, W, H, tail);
            hvo_frame_out fo = hvo_frame_out(); fo.kl = kl.data(); fo.kl_cap = fs.klCap();
            fs.collect(t, fo);
            const hvo_mf_result rh = on_host.TrackManhattanFrame(tail.normals.data(), tail.c.n_normals, tail.lines3d.data(), fo.n_kl);
            printf("frame %d axes %d%d%d tracked %d  R = [%.5f %.5f %.5f; %.5f %.5f %.5f; %.5f %.5f %.5f]  same %d\n", k, rd.found[0], rd.found[1], rd.found[2],
                   rd.tracked, rd.R[0], rd.R[1], rd.R[2], rd.R[3], rd.R[4], rd.R[5], rd.R[6], rd.R[7], rd.R[8], (int)(memcmp(&rd, &rh, sizeof(rd)) == 0));
        }
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
