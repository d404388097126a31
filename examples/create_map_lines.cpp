// create_map_lines.cpp -- LocalMapping::CreateNewMapLinesConstraint (reference src/LocalMapping.cc:1064-1565) on a toy map through the C++
// mirror (include/hvo.hpp): SearchForTriangulation of the current key frame against ALL its neighbours and the three-view triangulation of
// every pair of searched neighbours in one device call, and the caller's walk over what it returns.
//
// The call replaces lines 1105-1539 of the reference: the baseline gate, the searches, and per (pair, line) every test up to the overlap
// ratios.  What stays on the host is what the reference does with pointers (:1541-1559): new MapLine(line3D, vManhAxisIdx[ikl], ..), three
// AddObservation, three AddMapLine, ComputeDistinctiveDescriptors, UpdateAverageDir, mpMap->AddMapLine, mlpRecentAddedMapLines -- per entry
// of created_idx0 / idx1 / idx2, pair by pair in order.  The chain over the pairs is already resolved: a current line appears in exactly one
// pair's list, the first one whose triple passed every gate.  The reference runs this function in a thread of its own beside
// CreateNewMapPoints: that thread has its own context.  A caller that sees CheckNewKeyFrames() while the call runs discards its result
// (the reference returns from the search loop, before anything is created).
//
// The toy map (tests/new_lines_ref.py toy_map() is the same): six vertical segments 2 m away, the current key frame at the origin, three
// neighbours 25 cm right, 25 cm left and 50 cm right of it, each with its lines in reversed order.  Neighbour 0 lacks lines 2 and 3 (other
// descriptors), so those two are created by the pair (1, 2); the current line 5 already holds a map line.
//
// build:  g++ -std=c++14 -Iinclude examples/create_map_lines.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o create_map_lines
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "hvo.hpp"

struct MapLine { float line3d[6]; int manh_axis; std::vector<std::pair<int, int> > obs; };      // (key frame, line)
struct KeyFrame {
    std::vector<hvo_keyline> kl; std::vector<double> fn; std::vector<uint8_t> desc, has; std::vector<int> ml, manh; float Tcw[12];
};

static void toy_desc(int k, uint8_t *d)
{
    uint32_t v = (uint32_t)(((uint64_t)(k + 1) * 2654435761ull) & 0xFFFFFFFFull);
    for (int b = 0; b < 32; b++) { v = v * 1664525u + 1013904223u; d[b] = (uint8_t)(v >> 24); }
}

// the vertical segment at world x seen from a camera at (cx, 0, 0) looking along z: fx = fy = 512, principal point (320, 240)
static void add_line(KeyFrame &K, double x, double cx, int desc_id, int has)
{
    hvo_keyline l; memset(&l, 0, sizeof(l));
    const double u = 512.0 * (x - cx) / 2.0 + 320.0, v0 = 512.0 * -0.25 / 2.0 + 240.0, v1 = 512.0 * 0.25 / 2.0 + 240.0;
    l.sx = l.sox = (float)u; l.sy = l.soy = (float)v0; l.ex = l.eox = (float)u; l.ey = l.eoy = (float)v1;
    l.angle = (float)atan2((double)l.ey - l.sy, (double)l.ex - l.sx); l.class_id = -1; l.octave = 0;
    l.pt_x = (l.sx + l.ex) / 2; l.pt_y = (l.sy + l.ey) / 2; l.length = (float)hypot((double)l.ex - l.sx, (double)l.ey - l.sy);
    const double a = (double)l.sy - l.ey, b = (double)l.ex - l.sx, c = (double)l.sx * l.ey - (double)l.ex * l.sy, n = hypot(a, b);
    K.kl.push_back(l); K.fn.push_back(a / n); K.fn.push_back(b / n); K.fn.push_back(c / n);
    K.desc.resize(K.desc.size() + 32); toy_desc(desc_id, K.desc.data() + K.desc.size() - 32);
    K.has.push_back((uint8_t)has); K.ml.push_back(has ? 0 : -1); K.manh.push_back(0);
}

static hvo_nl_keyframe describe(const KeyFrame &K)
{
    hvo_nl_keyframe d; memset(&d, 0, sizeof(d));
    d.n = (int32_t)K.kl.size(); d.kl = K.kl.data(); d.linefn = K.fn.data(); d.desc = K.desc.data(); d.has_map_line = K.has.data();
    memcpy(d.Tcw, K.Tcw, sizeof(d.Tcw));
    d.cam.fx = d.cam.fy = 512.f; d.cam.cx = 320.f; d.cam.cy = 240.f;
    d.mb = 0.f; d.median_depth = 2.f;                                  // pKF2->ComputeSceneMedianDepth(2), read by the caller before the call
    return d;
}

int main()
{
    const double X[6] = { -0.5, -0.25, 0.25, 0.5, 0.75, 1.0 }, CX[3] = { 0.25, -0.25, 0.5 };
    std::vector<KeyFrame> kfs(4);                                      // 0: the current key frame; 1 .. 3: vpNeighKFs
    for (int j = 0; j < 4; j++) {
        const double cx = j ? CX[j - 1] : 0.0;
        const float T[12] = { 1, 0, 0, (float)-cx, 0, 1, 0, 0, 0, 0, 1, 0 };
        memcpy(kfs[j].Tcw, T, sizeof(T));
        if (j == 0) for (int i = 0; i < 6; i++) add_line(kfs[0], X[i], 0.0, i, i == 5);
        else for (int i = 5; i >= 0; i--) add_line(kfs[j], X[i], cx, (j == 1 && (i == 2 || i == 3)) ? 100 + i : i, 0);
    }
    std::vector<MapLine> map(1);                                       // map line 0: the one the current line 5 holds
    try {
        hvo_params hp; hvo_default_params(&hp); hp.max_batch = 1;
        hvo::Context ctx(hp);
        hvo::LocalMapping lm(ctx.get());
        const hvo_nl_keyframe cur = describe(kfs[0]);
        std::vector<hvo_nl_keyframe> nb;
        for (int j = 1; j < 4; j++) nb.push_back(describe(kfs[j]));
        std::vector<hvo::NewMapLineMatches> matches; std::vector<hvo::NewMapLines> res; std::vector<int> owner;
        const int nnew = lm.CreateNewMapLinesConstraint(cur, 3, nb.data(), matches, res, &owner);
        for (size_t j = 0; j < matches.size(); j++) printf("neighbour %d: gate %d, %d matches\n", (int)j, matches[j].gate, matches[j].n_matched);
        // LocalMapping.cc:1541-1559, pair by pair
        int walked = 0;
        std::vector<int> recent;
        for (size_t p = 0; p < res.size(); p++) {
            const hvo::NewMapLines &r = res[p];
            for (int k = 0; k < r.n_created; k++) {
                const int ikl = r.created_idx0[k], idx1 = r.created_idx1[k], idx2 = r.created_idx2[k];
                MapLine m;                                               // new MapLine(line3D, vManhAxisIdx[ikl], mpCurrentKeyFrame, mpMap)
                for (int q = 0; q < 6; q++) m.line3d[q] = r.line3d[6 * (size_t)ikl + q];
                m.manh_axis = kfs[0].manh[ikl];
                m.obs.push_back(std::make_pair(0, ikl)); m.obs.push_back(std::make_pair(r.kf2 + 1, idx1)); m.obs.push_back(std::make_pair(r.kf3 + 1, idx2));     // AddObservation x 3
                const int id = (int)map.size();
                kfs[0].ml[ikl] = id; kfs[r.kf2 + 1].ml[idx1] = id; kfs[r.kf3 + 1].ml[idx2] = id;      // AddMapLine x 3
                map.push_back(m); recent.push_back(id); walked++;       // ComputeDistinctiveDescriptors, UpdateAverageDir: not shown
                printf("pair %d (key frames %d, %d): line %d with %d and %d -> (%.3f %.3f %.3f) - (%.3f %.3f %.3f)\n", (int)p, r.kf2, r.kf3, ikl, idx1, idx2,
                       m.line3d[0], m.line3d[1], m.line3d[2], m.line3d[3], m.line3d[4], m.line3d[5]);
            }
        }
        printf("created %d new map lines (the call says %d); the map now holds %d\n", walked, nnew, (int)map.size());
        return walked == nnew ? 0 : 1;
    } catch (const hvo::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
}
