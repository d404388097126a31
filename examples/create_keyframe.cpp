// create_keyframe.cpp -- the new map points and map lines of Tracking::CreateNewKeyFrame (reference src/Tracking.cc:3032-3187) in one device
// call, through the C++ mirror (include/hvo.hpp), into a resident point map and line map.
//
// At a key frame the tracker sorts the features by depth, walks them with its counters and makes a MapPoint for every one that holds none (or
// one without observations), then does the same for the key lines.  hvo::Tracking::CreateNewKeyFrame does the selection, the unprojection, the
// normal and the distance range of the sole observer and the structural relation of every new line on the device and writes the slots of
// hvo::PointMap / hvo::LineMap in place: the tracker's next SearchLocalPoints / SearchLocalLines read them where they are.  What comes
// back is what `new MapPoint` / `new MapLine` need: per created entry the feature index, its slot, position, normal and distance range, and
// held[i] is the feature's slot afterwards.  AddObservation, AddMapPoint, UpdateManhAxis, the ids and the KeyFrame object stay here on the host.
//
// The toy frame (tests/test_new_keyframe_gpu.py builds the same): six key points at depths 2, 1, 0, 3, 1, 2.5 -- feature 2 has no depth,
// feature 3 holds the observed slot 0 and is kept, feature 4 holds the unobserved slot 1 and is made again -- and three lines: along x, along
// y, and one without depth.  The maps hold two slots each before the call; the new entries go behind them.
//
// build:  g++ -std=c++14 -Iinclude examples/create_keyframe.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o create_keyframe
#include <cstdio>
#include <cstring>
#include <vector>
#include "hvo.hpp"

int main()
{
    try {
        hvo_params hp; hvo_default_params(&hp); hp.max_batch = 1;
        hvo::Context ctx(hp);
        const hvo_camera cam = { 535.4f, 539.2f, 320.1f, 247.6f, 40.0f, 0.08f };
        const float Tcw[12] = { 1.f, 0.f, 0.f, 0.25f, 0.f, 1.f, 0.f, -0.125f, 0.f, 0.f, 1.f, 0.5f };
        // the maps as the tracker left them: two slots each, the first observed, the second not
        const int n0 = 2;
        hvo::PointMap points(0, 0); hvo::LineMap lines(0, 0);
        {
            const float pos[6] = { 0.f, 0.f, 2.f, 1.f, 0.f, 2.f }, nrm[6] = { 0.f, 0.f, 1.f, 0.f, 0.f, 1.f }, mx[2] = { 4.f, 4.f }, mi[2] = { 1.f, 1.f };
            const double lpos[12] = { 0, 0, 2, 1, 0, 2, 0, 1, 2, 1, 1, 2 }, lw[6] = { -1, 0, 0, -1, 0, 0 }, ln[6] = { 0, 0, 1, 0, 0, 1 };
            const uint8_t observed[2] = { 1, 0 };
            std::vector<uint8_t> desc(2 * 32, 0xAA);
            points.setMany(0, n0, pos, nrm, mx, mi, desc.data(), observed);
            lines.setMany(0, n0, lpos, lw, ln, mx, mi, desc.data(), observed);
        }
        // the frame
        const int n_kp = 6, n_kl = 3;
        hvo_keypoint kp[n_kp]; memset(kp, 0, sizeof(kp));
        const float uv[n_kp][2] = { { 100.f, 120.f }, { 500.f, 90.f }, { 320.f, 240.f }, { 250.f, 400.f }, { 420.f, 300.f }, { 60.f, 200.f } };
        const float depth[n_kp] = { 2.f, 1.f, 0.f, 3.f, 1.f, 2.5f };
        const int octave[n_kp] = { 0, 2, 1, 0, 3, 1 };
        std::vector<uint8_t> desc(n_kp * 32), ldesc(n_kl * 32);
        for (int i = 0; i < n_kp; i++) { kp[i].x = uv[i][0]; kp[i].y = uv[i][1]; kp[i].octave = octave[i]; kp[i].class_id = -1; memset(&desc[32 * i], 16 * i + 1, 32); }
        hvo_keyline kl[n_kl]; memset(kl, 0, sizeof(kl));
        hvo_line3d l3[n_kl]; memset(l3, 0, sizeof(l3));
        const double A[n_kl][3] = { { -0.5, 0.25, 2.0 }, { 0.5, -0.5, 3.0 }, { 0, 0, 0 } }, B[n_kl][3] = { { 0.5, 0.25, 2.0 }, { 0.5, 0.5, 3.0 }, { 0, 0, 0 } };
        for (int i = 0; i < n_kl; i++) {
            kl[i].sx = 100.f + 50.f * i; kl[i].sy = 200.f; kl[i].ex = 300.f; kl[i].ey = 210.f + 5.f * i;
            for (int c = 0; c < 3; c++) { l3[i].A[c] = A[i][c]; l3[i].B[c] = B[i][c]; }
            memset(&ldesc[32 * i], 0x30 + i, 32);
        }
        hvo_kfi_frame frame; memset(&frame, 0, sizeof(frame));
        frame.kp_un = kp; frame.depth = depth; frame.desc = desc.data(); frame.n_kp = n_kp;
        frame.keylines = kl; frame.ldesc = ldesc.data(); frame.lines3d = l3; frame.n_kl = n_kl;
        // mvpMapPoints / mvpMapLines as slots
        int32_t held_points[n_kp] = { -1, -1, -1, 0, 1, HVO_HELD_FOREIGN_UNOBSERVED }, held_lines[n_kl] = { -1, -1, -1 };
        int32_t pt_index[n_kp], pt_slot[n_kp], ln_index[n_kl], ln_slot[n_kl]; uint8_t pt_status[n_kp], ln_status[n_kl], rel[n_kl * n_kl];
        float pt_pos[n_kp * 3], pt_normal[n_kp * 3], pt_max[n_kp], pt_min[n_kp], ln_max[n_kl], ln_min[n_kl];
        double ln_pos[n_kl * 6], ln_wvec[n_kl * 3], ln_normal[n_kl * 3];
        hvo_kfi_io io; memset(&io, 0, sizeof(io));
        io.n_kp = n_kp; io.n_kl = n_kl; io.held_points = held_points; io.held_lines = held_lines;
        io.pt_index = pt_index; io.pt_slot = pt_slot; io.pt_status = pt_status; io.pt_pos = pt_pos; io.pt_normal = pt_normal; io.pt_max_dist = pt_max; io.pt_min_dist = pt_min;
        io.ln_index = ln_index; io.ln_slot = ln_slot; io.ln_status = ln_status; io.ln_pos = ln_pos; io.ln_wvec = ln_wvec; io.ln_normal = ln_normal;
        io.ln_max_dist = ln_max; io.ln_min_dist = ln_min; io.ln_rel = rel;
        hvo::Tracking tracking(cam, 2.25f);
        const hvo_kfi_result r = tracking.CreateNewKeyFrame(ctx.get(), points, lines, Tcw, frame, io, n0, n0);
        printf("created %d of %d point candidates and %d of %d line candidates, kernel %.3f ms; the maps hold %d and %d slots\n", r.n_points_created,
               r.n_point_candidates, r.n_lines_created, r.n_line_candidates, r.kernel_ms, points.size(), lines.size());
        for (int e = 0; e < r.n_point_entries; e++) {
            float X[3], N[3], mx, mi; uint8_t d[32]; int bad, observed;
            hvo::check(hvo_point_map_slot(points.get(), pt_slot[e], X, N, &mx, &mi, d, &bad, &observed), "hvo_point_map_slot");
            printf("point %d: feature %d slot %d status %d desc %d pos %.9g %.9g %.9g normal %.9g %.9g %.9g range %.9g %.9g\n", e, pt_index[e], pt_slot[e], (int)pt_status[e],
                   (int)d[0], X[0], X[1], X[2], N[0], N[1], N[2], mx, mi);
        }
        for (int e = 0; e < r.n_line_entries; e++)
            printf("line %d: feature %d slot %d status %d start %.17g %.17g %.17g end %.17g %.17g %.17g range %.9g %.9g rel %d %d %d\n", e, ln_index[e], ln_slot[e],
                   (int)ln_status[e], ln_pos[6 * e], ln_pos[6 * e + 1], ln_pos[6 * e + 2], ln_pos[6 * e + 3], ln_pos[6 * e + 4], ln_pos[6 * e + 5], ln_max[e], ln_min[e],
                   (int)rel[n_kl * e], (int)rel[n_kl * e + 1], (int)rel[n_kl * e + 2]);
        printf("held points %d %d %d %d %d %d lines %d %d %d\n", held_points[0], held_points[1], held_points[2], held_points[3], held_points[4], held_points[5],
               held_lines[0], held_lines[1], held_lines[2]);
    } catch (const hvo::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
