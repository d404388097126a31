// plane_assoc_host.cpp -- the map-plane association as a plain single-thread loop on the host, the figure that stands beside the device
// forms in profiles/r08_plane_assoc.txt (tools/plane_assoc_timing.py builds it with g++ -O2 and feeds it the same inputs).  Written for
// this tool from the rule as include/hvo.h states it: per frame plane the world coefficients, then the slots in order -- angle gate,
// smallest point distance, running thresholds for the match, the vertical and the parallel plane.
//
// input file: int32 n, ns; float th[4], Tcw[12], coef[n][4]; per slot: float w[4]; int32 bad, npts; float xyz[npts][3]
// output: "<median ms per call> <matches> <checksum>"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

struct Slot { float w[4]; int32_t bad, npts; std::vector<float> xyz; };

static int search(const std::vector<float> &coef, int n, const float *T, const float *th, const std::vector<Slot> &slots, std::vector<int> &out)
{
    int nmatches = 0;
    for (int i = 0; i < n; i++) {
        const float *c = &coef[4 * i];
        float pM[4];
        for (int k = 0; k < 4; k++)
            pM[k] = (float)((double)T[k] * c[0] + (double)T[4 + k] * c[1] + (double)T[8 + k] * c[2] + (k == 3 ? 1.0 : 0.0) * c[3]);
        float ld = th[0], lv = th[2], lp = th[3];
        int mi = -1, vi = -1, pi = -1;
        for (size_t j = 0; j < slots.size(); j++) {
            const Slot &s = slots[j];
            if (s.bad) continue;
            const float angle = pM[0] * s.w[0] + pM[1] * s.w[1] + pM[2] * s.w[2];
            if (angle > th[1] || angle < -th[1]) {
                float res = 100.f;
                const float *p = s.xyz.data();
                for (int q = 0; q < s.npts; q++, p += 3) {
                    const float d = std::fabs(pM[0] * p[0] + pM[1] * p[1] + pM[2] * p[2] + pM[3]);
                    if (d < res) res = d;
                }
                if (res < ld) { ld = res; mi = (int)j; continue; }
            }
            if (angle < lv && angle > -lv) { lv = std::fabs(angle); vi = (int)j; continue; }
            if (angle > lp || angle < -lp) { lp = std::fabs(angle); pi = (int)j; }
        }
        out[3 * i] = mi; out[3 * i + 1] = vi; out[3 * i + 2] = pi;
        nmatches += mi >= 0;
    }
    return nmatches;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s scene.bin [calls]\n", argv[0]); return 2; }
    const int calls = argc > 2 ? atoi(argv[2]) : 11;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t n = 0, ns = 0; float th[4], T[12];
    if (fread(&n, 4, 1, f) != 1 || fread(&ns, 4, 1, f) != 1 || fread(th, 4, 4, f) != 4 || fread(T, 4, 12, f) != 12) return 3;
    std::vector<float> coef((size_t)n * 4);
    if (n && fread(coef.data(), 16, n, f) != (size_t)n) return 3;
    std::vector<Slot> slots(ns);
    for (auto &s : slots) {
        if (fread(s.w, 4, 4, f) != 4 || fread(&s.bad, 4, 1, f) != 1 || fread(&s.npts, 4, 1, f) != 1) return 3;
        s.xyz.resize((size_t)s.npts * 3);
        if (s.npts && fread(s.xyz.data(), 12, s.npts, f) != (size_t)s.npts) return 3;
    }
    fclose(f);
    std::vector<int> out((size_t)n * 3 + 1);
    std::vector<double> ms;
    int nm = 0;
    for (int k = 0; k < calls + 2; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        nm = search(coef, n, T, th, slots, out);
        const auto t1 = std::chrono::steady_clock::now();
        if (k >= 2) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    long long sum = 0;
    for (int v : out) sum = sum * 31 + v;
    printf("%.4f %d %lld\n", ms[ms.size() / 2], nm, sum);
    return 0;
}
