// local_map_lines.cpp -- the local-map line search the way Tracking::SearchLocalLines uses it (reference src/Tracking.cc:3279-3355 ->
// LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th), src/LSDmatcher.cpp:709-801), through the C++ mirror (include/hvo.hpp).
// Two RGB-D frames go through a stream with the line grid and the 3-D lines resident; the lines of the first frame stand in for the local
// map's lines (camera = world, so a line's world vector is its own A - B; every line "in view"; its projection = its own end points).  The
// search runs on the resident second frame (FrameStream::searchLocalLines) and on host arrays (LSDmatcher::SearchByProjection), and the two
// results are printed.  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/local_map_lines.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o local_map_lines
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
    if (argc < 5) { fprintf(stderr, "usage: %s gray0.u8 depth0.u16 gray1.u8 depth1.u16\n", argv[0]); return 2; }
    const int W = 640, H = 480;
    std::vector<uint8_t> gray[2] = { std::vector<uint8_t>(W * H), std::vector<uint8_t>(W * H) };
    std::vector<uint16_t> depth[2] = { std::vector<uint16_t>(W * H), std::vector<uint16_t>(W * H) };
    for (int k = 0; k < 2; k++)
        if (!read_raw(argv[1 + 2 * k], gray[k].data(), gray[k].size()) || !read_raw(argv[2 + 2 * k], depth[k].data(), depth[k].size() * 2)) return 3;
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u;
        sp.stages = HVO_STAGE_ORB | HVO_STAGE_LSD | HVO_STAGE_LSD_CULL | HVO_STAGE_LINES3D | HVO_STAGE_GRIDS;
        hvo::FrameStream fs(p, sp);
        int64_t t[2];
        std::vector<hvo_keyline> kl[2]; std::vector<uint8_t> ld[2]; std::vector<double> fn[2];
        hvo::FrameStream::FrameTail tail[2];
        for (int k = 0; k < 2; k++) t[k] = fs.submit(hvo::Image8{ gray[k].data(), W, H, W }, hvo::Image16{ depth[k].data(), W, H, W * 2 });
        // the current frame (1) stays resident for the search: its tail is collected, the slot itself is not released
        for (int k = 0; k < 2; k++) {
            kl[k].resize(fs.klCap()); ld[k].resize((size_t)fs.klCap() * 32); fn[k].resize((size_t)fs.klCap() * 3);
            fs.collectTail(t[k], W, H, tail[k]);
        }
        hvo_frame_out fo[2] = { hvo_frame_out(), hvo_frame_out() };
        for (int k = 0; k < 2; k++) { fo[k].kl = kl[k].data(); fo[k].ldesc = ld[k].data(); fo[k].linefn = fn[k].data(); fo[k].kl_cap = fs.klCap(); }
        fs.collect(t[0], fo[0]);
        // the "local map": frame 0's lines with a fitted 3-D line (MapLine::mbTrackInView && !isBad(), in vpMapLines order)
        std::vector<float> q_xyxy, q_vc; std::vector<double> q_wv; std::vector<uint8_t> q_desc, q_blocks;
        for (int i = 0; i < fo[0].n_kl; i++) {
            const hvo_line3d &l = tail[0].lines3d[i];
            if (!l.good) continue;
            const hvo_keyline &k = kl[0][i];
            q_xyxy.insert(q_xyxy.end(), { k.sx, k.sy, k.ex, k.ey });
            q_vc.push_back(1.0f);
            q_wv.insert(q_wv.end(), { l.A[0] - l.B[0], l.A[1] - l.B[1], l.A[2] - l.B[2] });
            q_desc.insert(q_desc.end(), ld[0].begin() + 32 * (size_t)i, ld[0].begin() + 32 * (size_t)i + 32);
            q_blocks.push_back((uint8_t)(i % 2));                                     // Observations() > 0 for every other map line
        }
        const int nq = (int)q_vc.size();
        std::vector<int32_t> mi_stream, mi_host;
        const int ns = fs.searchLocalLines(t[1], nq, q_xyxy.data(), q_vc.data(), q_wv.data(), q_desc.data(), q_blocks.data(), nullptr, 3.0f, mi_stream);
        fs.collect(t[1], fo[1]);
        hvo::Context ctx(p);
        hvo::LSDmatcher lm(ctx.get());
        const float b[4] = { 0.f, (float)W, 0.f, (float)H };                          // TUM3: no distortion
        const int nh = lm.SearchByProjection(nq, q_xyxy.data(), q_vc.data(), q_wv.data(), q_desc.data(), q_blocks.data(), kl[1].data(), fn[1].data(),
                                             tail[1].lines3d.data(), ld[1].data(), nullptr, fo[1].n_kl, tail[1].ln_cell_start.data(), tail[1].ln_cell_items.data(),
                                             b, 3.0f, mi_host);
        // Tracking::SearchLocalLines then assigns mCurrentFrame.mvpMapLines[mi[q]] = pML in query order
        printf("map lines %d lines %d stream %d host %d same %d\n", nq, fo[1].n_kl, ns, nh, (int)(ns == nh && mi_stream == mi_host));
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
