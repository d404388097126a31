// line_frustum_host.cpp -- the host side of the path that hvo_search_local_lines replaces, as a plain single-thread loop: for every local
// map line the bad / seen skip and the in-frustum test (both end points transformed and projected, the image-bounds tests, the distance
// range, the viewing angle, the predicted scale level), and for every line that passes the query record the search call takes -- the
// projection, the viewing cosine, the world vector, the descriptor, the observation flag -- appended to the upload arrays.  It is the
// figure that stands beside the device call in profiles/r11_line_map.txt (tools/line_map_timing.py builds it with g++ -O2 and feeds it
// the same map).  Written for this tool from the rule as include/hvo.h states it, on plain floats: a tracker that builds a matrix object
// per operand for every line pays more than this loop does, so the figure is a lower bound for such a host.
//
// input file: int32 n; float cam[4] (fx fy cx cy), bounds[4], logsf, Tcw[12]; double pos[n][6], wvec[n][3], normal[n][3];
//             float maxd[n], mind[n]; uint8 desc[n][32], flags[n] (bit 0 bad, bit 1 observed, bit 2 seen)
// output: "<median ms per call> <in view> <checksum>"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Map {
    int n; float cam[4], b[4], logsf, T[12];
    std::vector<double> pos, wvec, nrm; std::vector<float> maxd, mind; std::vector<uint8_t> desc, flags;
};
struct Queries { std::vector<float> xyxy, vc; std::vector<int32_t> level, slot; std::vector<double> wvec; std::vector<uint8_t> desc, blocks; };

static int frustum(const Map &M, Queries &Q)
{
    const float *T = M.T;
    float Ow[3];
    for (int r = 0; r < 3; r++) Ow[r] = -(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);
    Q.xyxy.clear(); Q.vc.clear(); Q.level.clear(); Q.slot.clear(); Q.wvec.clear(); Q.desc.clear(); Q.blocks.clear();
    for (int j = 0; j < M.n; j++) {
        if (M.flags[j] & 5) continue;                                            // seen in this frame, or bad
        const double *P = &M.pos[6 * (size_t)j];
        const float S[3] = { (float)P[0], (float)P[1], (float)P[2] }, E[3] = { (float)P[3], (float)P[4], (float)P[5] };
        float Sc[3], Ec[3];
        for (int r = 0; r < 3; r++) {
            Sc[r] = T[4 * r] * S[0] + T[4 * r + 1] * S[1] + T[4 * r + 2] * S[2] + T[4 * r + 3];
            Ec[r] = T[4 * r] * E[0] + T[4 * r + 1] * E[1] + T[4 * r + 2] * E[2] + T[4 * r + 3];
        }
        if (Sc[2] < 0.0f || Ec[2] < 0.0f) continue;
        const float iz1 = 1.0f / Sc[2], u1 = M.cam[0] * Sc[0] * iz1 + M.cam[2], v1 = M.cam[1] * Sc[1] * iz1 + M.cam[3];
        if (u1 < M.b[0] || u1 > M.b[1] || v1 < M.b[2] || v1 > M.b[3]) continue;
        const float iz2 = 1.0f / Ec[2], u2 = M.cam[0] * Ec[0] * iz2 + M.cam[2], v2 = M.cam[1] * Ec[1] * iz2 + M.cam[3];
        if (u2 < M.b[0] || u2 > M.b[1] || v2 < M.b[2] || v2 > M.b[3]) continue;
        float om[3];
        for (int r = 0; r < 3; r++) om[r] = 0.5f * (S[r] + E[r]) - Ow[r];
        const float dist = (float)std::sqrt((double)om[0] * om[0] + (double)om[1] * om[1] + (double)om[2] * om[2]);
        if (dist < 0.8f * M.mind[j] || dist > 1.2f * M.maxd[j]) continue;
        const double *N = &M.nrm[3 * (size_t)j];
        const float vc = (float)(((double)om[0] * (float)N[0] + (double)om[1] * (float)N[1] + (double)om[2] * (float)N[2]) / dist);
        if (vc < 0.5f) continue;
        const int level = (int)std::ceil(std::log(M.maxd[j] / dist) / M.logsf);
        const float q[4] = { u1, v1, u2, v2 };
        Q.xyxy.insert(Q.xyxy.end(), q, q + 4); Q.vc.push_back(vc); Q.level.push_back(level); Q.slot.push_back(j);
        Q.wvec.insert(Q.wvec.end(), &M.wvec[3 * (size_t)j], &M.wvec[3 * (size_t)j] + 3);
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
    Map M; int32_t n = 0; float hd[21];
    if (fread(&n, 4, 1, f) != 1 || n < 0 || fread(hd, 4, 21, f) != 21) return 3;
    M.n = n; memcpy(M.cam, hd, 16); memcpy(M.b, hd + 4, 16); M.logsf = hd[8]; memcpy(M.T, hd + 9, 48);
    const size_t N = (size_t)n;
    if (!rd(f, M.pos, 6 * N) || !rd(f, M.wvec, 3 * N) || !rd(f, M.nrm, 3 * N) || !rd(f, M.maxd, N) || !rd(f, M.mind, N) || !rd(f, M.desc, 32 * N) || !rd(f, M.flags, N)) return 3;
    fclose(f);
    Queries Q; int nv = 0;
    std::vector<double> ms;
    for (int c = 0; c < calls + 3; c++) {
        const auto t0 = std::chrono::steady_clock::now();
        nv = frustum(M, Q);
        const auto t1 = std::chrono::steady_clock::now();
        if (c >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    double sum = 0;
    for (size_t i = 0; i < Q.vc.size(); i++) sum += Q.vc[i] + Q.xyxy[4 * i] + Q.level[i];
    printf("%.6f %d %.6f\n", ms[ms.size() / 2], nv, sum);
    return 0;
}
