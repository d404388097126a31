// map_refresh_host.cpp -- MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (reference src/MapPoint.cc:240-305, 328-369) and
// MapLine::ComputeDistinctiveDescriptors + UpdateAverageDir (src/MapLine.cpp:331-396, 404-455) as a plain single-thread host program: the loops
// AS WRITTEN (the N x N matrix, every row copied and sorted, the sums in list order) with the readings of csrc/map_refresh.hip.
// tools/map_refresh_timing.py times it beside the device call; tests/test_map_refresh.py compares its answers with the restatement.
//
//   map_refresh_host <case file> <result file> <reps>        prints the median wall ms of the sweep over <reps> runs
//
// case file: int32 line, n, n_obs, n_levels, what; float32 sf[n_levels]; int32 obs_start[n + 1]; n_obs x 32 bytes; n_obs x 3 float32 Ow;
//   n_obs kf_bad bytes; n x 3 float32 ref_Ow; n int32 ref_level; n skip bytes; the positions (n x 3 float32, or n x 6 double for lines)
// result file: n int32 best_obs, n int32 best_median, n x 32 bytes, the normals (n x 3 float32 / double), for lines n x 3 double wvec, n float32
//   max_dist, n float32 min_dist, n status bytes.  What a feature's status says is not written holds 119.
//
// build:  g++ -std=c++17 -O2 -ffp-contract=off tools/map_refresh_host.cpp -o map_refresh_host
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>

enum { DESCRIPTOR = 1, GEOMETRY = 2, REFRESHED = 0, SKIPPED, NO_OBS, DESC_KEPT, BAD_LEVEL, UNTOUCHED = 119 };

struct Case {
    int line, n, n_obs, n_levels, what;
    std::vector<float> sf, Ow, ref_Ow, posf; std::vector<int32_t> start, level; std::vector<uint8_t> desc, bad, skip; std::vector<double> posd;
};
struct Result {
    std::vector<int32_t> best_obs, best_median; std::vector<uint8_t> desc, status; std::vector<float> nf, maxd, mind; std::vector<double> nd, wvec;
};

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static int ham(const uint8_t *a, const uint8_t *b)
{
    int h = 0;
    for (int w = 0; w < 8; w++) { uint32_t x, y; memcpy(&x, a + 4 * w, 4); memcpy(&y, b + 4 * w, 4); h += __builtin_popcount(x ^ y); }
    return h;
}

static void sweep(const Case &c, Result &r)
{
    const size_t n = (size_t)c.n;
    r.best_obs.assign(n, UNTOUCHED); r.best_median.assign(n, UNTOUCHED); r.desc.assign(n * 32, UNTOUCHED); r.status.assign(n, 0);
    r.nf.assign(c.line ? 0 : n * 3, (float)UNTOUCHED); r.nd.assign(c.line ? n * 3 : 0, (double)UNTOUCHED); r.wvec.assign(c.line ? n * 3 : 0, (double)UNTOUCHED);
    r.maxd.assign(n, (float)UNTOUCHED); r.mind.assign(n, (float)UNTOUCHED);
    std::vector<const uint8_t *> vd; std::vector<int> which; std::vector<float> D; std::vector<int> v;
    for (size_t f = 0; f < n; f++) {
        const int a = c.start[f], b = c.start[f + 1];
        r.best_obs[f] = r.best_median[f] = -1;
        if (c.skip[f]) { r.status[f] = SKIPPED; continue; }
        if (a == b) { r.status[f] = NO_OBS; continue; }
        int status = REFRESHED;
        if (c.what & DESCRIPTOR) {
            vd.clear(); which.clear();
            for (int i = a; i < b; i++) if (!c.bad[i]) { vd.push_back(&c.desc[32 * (size_t)i]); which.push_back(i - a); }
            if (vd.empty()) status = DESC_KEPT;
            else {
                const size_t N = vd.size();
                D.assign(N * N, 0.f);
                for (size_t i = 0; i < N; i++) {
                    D[i * N + i] = 0;
                    // (MapLine.cpp:367 starts at 0: every pair twice, and the diagonal)
                    for (size_t j = c.line ? 0 : i + 1; j < N; j++) { const int d = ham(vd[i], vd[j]); D[i * N + j] = (float)d; D[j * N + i] = (float)d; }
                }
                int BestMedian = INT_MAX, BestIdx = 0;
                for (size_t i = 0; i < N; i++) {
                    v.assign(D.begin() + i * N, D.begin() + (i + 1) * N);
                    std::sort(v.begin(), v.end());
                    const int median = v[(size_t)(0.5 * (N - 1))];
                    if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
                }
                r.best_obs[f] = which[BestIdx]; r.best_median[f] = BestMedian; memcpy(&r.desc[32 * f], vd[BestIdx], 32);
            }
        }
        if (c.what & GEOMETRY) {
            const int nobs = b - a;
            const float *Or = &c.ref_Ow[3 * f];
            float cm[3];
            if (c.line) {
                const double *P = &c.posd[6 * f];
                const double mid[3] = { 0.5 * (P[0] + P[3]), 0.5 * (P[1] + P[4]), 0.5 * (P[2] + P[5]) };
                double s[3] = { 0, 0, 0 };
                for (int i = a; i < b; i++) {
                    const float *O = &c.Ow[3 * (size_t)i];
                    const double x = mid[0] - (double)O[0], y = mid[1] - (double)O[1], z = mid[2] - (double)O[2];
                    const double nn = sqrt((x * x + y * y) + z * z);
                    s[0] = s[0] + x / nn; s[1] = s[1] + y / nn; s[2] = s[2] + z / nn;
                }
                for (int k = 0; k < 3; k++) r.nd[3 * f + k] = s[k] / (double)nobs;
                for (int k = 0; k < 3; k++) { const float sp = (float)P[k], ep = (float)P[3 + k]; cm[k] = (float)((double)sp * 0.5 + (double)ep * 0.5) - Or[k]; }
                double w[3] = { P[0] - P[3], P[1] - P[4], P[2] - P[5] };
                const double z = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
                if (z > 0.0) { const double q = sqrt(z); for (int k = 0; k < 3; k++) w[k] = w[k] / q; }
                for (int k = 0; k < 3; k++) r.wvec[3 * f + k] = w[k];
            } else {
                const float *P = &c.posf[3 * f];
                float s[3] = { 0, 0, 0 };
                for (int i = a; i < b; i++) {
                    const float *O = &c.Ow[3 * (size_t)i];
                    const float x = P[0] - O[0], y = P[1] - O[1], z = P[2] - O[2];
                    double q = (double)x * (double)x; q = q + (double)y * (double)y; q = q + (double)z * (double)z;
                    const double inv = 1.0 / sqrt(q);
                    s[0] = s[0] + (float)((double)x * inv); s[1] = s[1] + (float)((double)y * inv); s[2] = s[2] + (float)((double)z * inv);
                }
                const double in = 1.0 / (double)nobs;
                for (int k = 0; k < 3; k++) { r.nf[3 * f + k] = (float)((double)s[k] * in); cm[k] = P[k] - Or[k]; }
            }
            const int level = c.level[f];
            if (level >= 0 && level < c.n_levels) {
                double q = (double)cm[0] * (double)cm[0]; q = q + (double)cm[1] * (double)cm[1]; q = q + (double)cm[2] * (double)cm[2];
                const float dist = (float)sqrt(q);
                r.maxd[f] = dist * c.sf[level]; r.mind[f] = r.maxd[f] / c.sf[c.n_levels - 1];
            } else if (status == REFRESHED) status = BAD_LEVEL;
        }
        r.status[f] = (uint8_t)status;
    }
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: map_refresh_host <case file> <result file> <reps>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Case c; int h[5];
    if (!rd(f, h, sizeof(h))) return 2;
    c.line = h[0]; c.n = h[1]; c.n_obs = h[2]; c.n_levels = h[3]; c.what = h[4];
    if (c.n < 0 || c.n_obs < 0 || c.n_levels < 1 || c.n_levels > 16) return 2;
    const size_t n = (size_t)c.n, no = (size_t)c.n_obs;
    c.sf.resize(c.n_levels); c.start.resize(n + 1); c.desc.resize(no * 32); c.Ow.resize(no * 3); c.bad.resize(no); c.ref_Ow.resize(n * 3); c.level.resize(n); c.skip.resize(n);
    if (c.line) c.posd.resize(n * 6); else c.posf.resize(n * 3);
    bool ok = rd(f, c.sf.data(), c.n_levels * 4) && rd(f, c.start.data(), (n + 1) * 4) && rd(f, c.desc.data(), no * 32) && rd(f, c.Ow.data(), no * 12) && rd(f, c.bad.data(), no) &&
              rd(f, c.ref_Ow.data(), n * 12) && rd(f, c.level.data(), n * 4) && rd(f, c.skip.data(), n) &&
              (c.line ? rd(f, c.posd.data(), n * 48) : rd(f, c.posf.data(), n * 12));
    fclose(f);
    if (!ok || c.start[0] != 0 || c.start[n] != c.n_obs) { fprintf(stderr, "short or inconsistent case file\n"); return 2; }
    for (size_t i = 0; i < n; i++) if (c.start[i + 1] < c.start[i]) return 2;
    const int reps = std::max(1, atoi(argv[3]));
    Result r; std::vector<double> ms;
    for (int k = 0; k < reps; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        sweep(c, r);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%.4f\n", ms[ms.size() / 2]);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(r.best_obs.data(), 4, n, o); fwrite(r.best_median.data(), 4, n, o); fwrite(r.desc.data(), 1, n * 32, o);
    if (c.line) { fwrite(r.nd.data(), 8, n * 3, o); fwrite(r.wvec.data(), 8, n * 3, o); } else fwrite(r.nf.data(), 4, n * 3, o);
    fwrite(r.maxd.data(), 4, n, o); fwrite(r.mind.data(), 4, n, o); fwrite(r.status.data(), 1, n, o);
    fclose(o);
    return 0;
}
