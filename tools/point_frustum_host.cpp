// point_frustum_host.cpp -- the host side of the path that hvo_search_local_points replaces, as a plain single-thread loop: for every local
// map point the bad / seen skip and the in-frustum test (the point transformed and projected, the image-bounds tests, the distance range,
// the viewing angle, the predicted scale level with its clamp), and for every point that passes the query record the search call takes --
// the projection with its right coordinate, the level, the viewing cosine, the descriptor, the observation flag -- appended to the upload
// arrays.  It is the figure that stands beside the device call in profiles/r13_point_map.txt (tools/point_map_timing.py builds it with
// g++ -O2 and feeds it the same map).  Written for this tool from the rule as include/hvo.h states it, on plain floats: a tracker that
// builds a matrix object per operand and takes two mutexes per point pays more than this loop does, so the figure is a lower bound for
// such a host.
//
// input file: int32 n, n_levels; float cam[5] (fx fy cx cy bf), bounds[4], logsf, Tcw[12]; float pos[n][3], normal[n][3], maxd[n], mind[n];
//             uint8 desc[n][32], flags[n] (bit 0 bad, bit 1 observed, bit 2 seen)
// output: "<median ms per call> <in view> <checksum>"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct PointMapHost {
    int n, n_levels; float cam[5], b[4], logsf, T[12];
    std::vector<float> pos, nrm, maxd, mind; std::vector<uint8_t> desc, flags;
};
struct PointQueries { std::vector<float> u, v, ur, vc; std::vector<int32_t> level, slot; std::vector<uint8_t> desc, blocks; };

static int points_in_view(const PointMapHost &M, PointQueries &Q)
{
    const float *T = M.T;
    float Ow[3];
    for (int r = 0; r < 3; r++) Ow[r] = -(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);
    Q.u.clear(); Q.v.clear(); Q.ur.clear(); Q.vc.clear(); Q.level.clear(); Q.slot.clear(); Q.desc.clear(); Q.blocks.clear();
    for (int j = 0; j < M.n; j++) {
        if (M.flags[j] & 5) continue;                                            // seen in this frame, or bad
        const float *P = &M.pos[3 * (size_t)j], *N = &M.nrm[3 * (size_t)j];
        float C[3];
        for (int r = 0; r < 3; r++) C[r] = T[4 * r] * P[0] + T[4 * r + 1] * P[1] + T[4 * r + 2] * P[2] + T[4 * r + 3];
        if (C[2] < 0.0f) continue;
        const float iz = 1.0f / C[2], u = M.cam[0] * C[0] * iz + M.cam[2], v = M.cam[1] * C[1] * iz + M.cam[3];
        if (u < M.b[0] || u > M.b[1] || v < M.b[2] || v > M.b[3]) continue;
        const float po[3] = { P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2] };
        const float dist = (float)std::sqrt((double)po[0] * po[0] + (double)po[1] * po[1] + (double)po[2] * po[2]);
        if (dist < 0.8f * M.mind[j] || dist > 1.2f * M.maxd[j]) continue;
        const float vc = (float)(((double)po[0] * N[0] + (double)po[1] * N[1] + (double)po[2] * N[2]) / dist);
        if (vc < 0.5f) continue;
        int level = (int)std::ceil(std::log(M.maxd[j] / dist) / M.logsf);
        level = level < 0 ? 0 : level >= M.n_levels ? M.n_levels - 1 : level;
        Q.u.push_back(u); Q.v.push_back(v); Q.ur.push_back(u - M.cam[4] * iz); Q.vc.push_back(vc); Q.level.push_back(level); Q.slot.push_back(j);
        Q.desc.insert(Q.desc.end(), &M.desc[32 * (size_t)j], &M.desc[32 * (size_t)j] + 32);
        Q.blocks.push_back((M.flags[j] & 2) ? 1 : 0);
    }
    return (int)Q.slot.size();
}

template <class T> static bool rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s map.bin [calls]\n", argv[0]); return 2; }
    const int calls = argc > 2 ? std::max(1, atoi(argv[2])) : 30;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    PointMapHost M; int32_t hd_i[2] = { 0, 0 }; float hd[22];
    if (fread(hd_i, 4, 2, f) != 2 || hd_i[0] < 0 || fread(hd, 4, 22, f) != 22) return 3;
    M.n = hd_i[0]; M.n_levels = hd_i[1]; memcpy(M.cam, hd, 20); memcpy(M.b, hd + 5, 16); M.logsf = hd[9]; memcpy(M.T, hd + 10, 48);
    const size_t N = (size_t)M.n;
    if (!rd(f, M.pos, 3 * N) || !rd(f, M.nrm, 3 * N) || !rd(f, M.maxd, N) || !rd(f, M.mind, N) || !rd(f, M.desc, 32 * N) || !rd(f, M.flags, N)) return 3;
    fclose(f);
    PointQueries Q; int nv = 0;
    std::vector<double> ms;
    for (int c = 0; c < calls + 3; c++) {
        const auto t0 = std::chrono::steady_clock::now();
        nv = points_in_view(M, Q);
        const auto t1 = std::chrono::steady_clock::now();
        if (c >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    double sum = 0;
    for (size_t i = 0; i < Q.vc.size(); i++) sum += Q.vc[i] + Q.u[i] + Q.level[i];
    printf("%.6f %d %.6f\n", ms[ms.size() / 2], nv, sum);
    return 0;
}
