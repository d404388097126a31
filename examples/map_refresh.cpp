// map_refresh.cpp -- MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:240-305, 328-369) for
// the map points of a key frame in one device call, through the C++ mirror (include/hvo.hpp), on a resident point map.
//
// The local mapper runs the two functions for every map point of the current key frame after ProcessNewKeyFrame, after every creation, after
// SearchInNeighbors and after every bundle adjustment.  With the points resident (hvo::PointMap) the sweep is hvo::PointMap::refresh: the
// caller flattens each point's mObservations IN THE MAP'S ITERATION ORDER into one ragged list -- the observing key frame's descriptor row,
// its camera centre and its isBad() -- adds the reference key frame's camera centre and the octave of the point's key point there, and the
// slots' descriptor, normal and distance range are rewritten in place; the tracker's next SearchLocalPoints reads them where they are.
// What comes back is small: per point the status, the winning observation and its median.  hvo::refreshMapPoints is the same on host arrays.
//
// The toy map (tests/test_map_refresh_gpu.py builds the same): four points 2 m in front of key frames standing 25 cm apart along x.
// Descriptor k has its first k bits set, so two descriptors differ by the difference of their numbers.
//   point 0   seen with descriptors 0, 10, 20: every row's median is 10, the first is kept
//   point 1   seen with 0, 50, 60: the rows' medians are 50, 10, 10, observation 1 wins
//   point 2   every observer is bad: the descriptor is kept, the normal and the range are written
//   point 3   no observations: nothing is written
//
// build:  g++ -std=c++14 -Iinclude examples/map_refresh.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o map_refresh
#include <cstdio>
#include <cstring>
#include <vector>
#include "hvo.hpp"

static void toy_desc(int k, uint8_t *d)
{
    memset(d, 0, 32);
    for (int i = 0; i < k; i++) d[i >> 3] |= (uint8_t)(1u << (i & 7));
}

int main()
{
    try {
        hvo_params hp; hvo_default_params(&hp); hp.max_batch = 1;
        hvo::Context ctx(hp);
        const int n = 4;
        const float pos[n * 3] = { 0.f, 0.f, 2.f, 0.5f, 0.f, 2.f, -0.5f, 0.25f, 2.f, 0.f, 0.5f, 2.f };
        // the map as the tracker left it: any normal, range and descriptor
        std::vector<float> nrm(n * 3, 0.f), maxd(n, 9.f), mind(n, 1.f);
        std::vector<uint8_t> desc(n * 32, 0xAA);
        hvo::PointMap map(0, n);
        map.setMany(0, n, pos, nrm.data(), maxd.data(), mind.data(), desc.data());
        // mObservations of the four points, flattened
        const int numbers[3][3] = { { 0, 10, 20 }, { 0, 50, 60 }, { 5, 6, 7 } };
        const int32_t obs_start[n + 1] = { 0, 3, 6, 9, 9 };
        std::vector<uint8_t> obs_desc(9 * 32), kf_bad(9, 0);
        std::vector<float> obs_Ow(9 * 3, 0.f);
        for (int p = 0; p < 3; p++) for (int j = 0; j < 3; j++) {
            toy_desc(numbers[p][j], &obs_desc[32 * (3 * p + j)]);
            obs_Ow[3 * (3 * p + j)] = 0.25f * (float)j;                // key frame j stands at (0.25 j, 0, 0)
            if (p == 2) kf_bad[3 * p + j] = 1;
        }
        const float ref_Ow[n * 3] = { 0.f, 0.f, 0.f, 0.25f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
        const int32_t ref_level[n] = { 0, 2, 1, 0 }, slots[n] = { 0, 1, 2, 3 };
        hvo_mr_input in; memset(&in, 0, sizeof(in));
        in.n = n; in.obs_start = obs_start; in.obs_desc = obs_desc.data(); in.obs_Ow = obs_Ow.data(); in.kf_bad = kf_bad.data();
        in.ref_Ow = ref_Ow; in.ref_level = ref_level;
        std::vector<int32_t> best(n), median(n); std::vector<uint8_t> status(n);
        hvo_mr_point_out out; memset(&out, 0, sizeof(out));
        out.best_obs = best.data(); out.best_median = median.data(); out.status = status.data();
        const float ms = map.refresh(ctx.get(), slots, in, out);
        printf("refreshed %d map points, kernel %.3f ms\n", n, ms);
        for (int p = 0; p < n; p++) {
            float X[3], N[3], mx, mi; uint8_t d[32]; int bad, observed;
            hvo::check(hvo_point_map_slot(map.get(), p, X, N, &mx, &mi, d, &bad, &observed), "hvo_point_map_slot");
            int bits = 0;
            for (int b = 0; b < 32; b++) bits += __builtin_popcount(d[b]);
            printf("point %d: status %d best %d median %d descriptor bits %d normal %.9g %.9g %.9g range %.9g %.9g\n", p, (int)status[p], best[p], median[p], bits,
                   N[0], N[1], N[2], mx, mi);
        }
    } catch (const hvo::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
