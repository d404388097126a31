// line_fuse_host.cpp -- LSDmatcher::Fuse (reference src/LSDmatcher.cpp:1297-1434) with KeyFrame::GetLinesInArea (src/KeyFrame.cc:668-702) as a
// plain single-thread host loop: one call per key frame, per entry a sweep over every key line with a real vIndices vector, each key line's
// direction normalised again for every entry, as the reference does it.  The arithmetic and the three readings are those of
// csrc/line_fuse.hip and tests/line_fuse_ref.py (no stop at an entry behind the camera: every entry is evaluated).  It is what
// tools/line_fuse_timing.py puts beside the device call; it does not pay for cv::Mat temporaries, mutexes or the pointer walk.
//
//   line_fuse_host <case> <result> [reps]      prints the median wall ms of `reps` runs of all key frames
// case:   int32 n_kf, n, n_levels, th_low, level_rule; float32 th, log_scale_factor, scale_factor;
//         map side: pos n x 6 f64, normal n x 3 f64, max_distance n f32, min_distance n f32, desc n x 32 u8;
//         per key frame: int32 n_lines, n_desc_rows; Tcw 12 f32; fx fy cx cy f32; bounds 4 f32; pt_x, pt_y, sx, sy, ex, ey n_lines f32 each;
//         octave n_lines i32; desc_rows n_desc_rows x 32 u8; skip n u8
// result: per key frame best_idx n i32, best_dist n i32, gate n i8
//
// build:  g++ -std=c++14 -O2 -ffp-contract=off tools/line_fuse_host.cpp -o line_fuse_host
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct KF { int nl, nr; float T[12], cam[4], b[4]; std::vector<float> ptx, pty, sx, sy, ex, ey; std::vector<int32_t> oct; std::vector<uint8_t> rows, skip; };
struct Case {
    int n_kf, n, n_levels, th_low, rule; float th, logsf, scale;
    std::vector<double> pos, nrm; std::vector<float> maxd, mind; std::vector<uint8_t> desc; std::vector<KF> kf;
};
template <class T> static void rd(FILE *f, std::vector<T> &v, size_t n) { v.resize(n); if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }
template <class T> static void rd(FILE *f, T *v, size_t n) { if (fread(v, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

static float row(const float *a, const float *X, float t)          // one row of Rcw * X + tcw
{
    float s = a[0] * X[0]; s = s + a[1] * X[1]; s = s + a[2] * X[2];
    return (float)((double)s * 1.0 + (double)t * 1.0);
}
static int to_level(float v) { return v != v ? 0 : v >= 2147483648.0f ? 2147483647 : v <= -2147483648.0f ? (-2147483647 - 1) : (int)v; }
static int ham(const uint8_t *a, const uint8_t *b)
{
    const uint64_t *x = (const uint64_t *)a, *y = (const uint64_t *)b;
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

static void lines_in_area(const KF &k, float x1, float y1, float x2, float y2, float r, std::vector<size_t> &out)
{
    out.clear();
    float d1x = x1 - x2, d1y = y1 - y2;
    const float n1 = std::sqrt(d1x * d1x + d1y * d1y);
    d1x /= n1; d1y /= n1;
    for (int i = 0; i < k.nl; i++) {
        const float distance = (float)((0.5 * (x1 + x2) - k.ptx[i]) * (0.5 * (x1 + x2) - k.ptx[i]) + (0.5 * (y1 + y2) - k.pty[i]) * (0.5 * (y1 + y2) - k.pty[i]));
        if (distance > r * r) continue;
        float d2x = k.sx[i] - k.ex[i], d2y = k.sy[i] - k.ey[i];
        const float n2 = std::sqrt(d2x * d2x + d2y * d2y);
        d2x /= n2; d2y /= n2;
        const float c = std::fabs(d1x * d2x + d1y * d2y);
        if (c < 0.998f) continue;
        out.push_back((size_t)i);
    }
}

static void fuse(const Case &c, const KF &k, const float *sf, int32_t *bi, int32_t *bd, int8_t *gate)
{
    float R[9], t[3], Ow[3];
    for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) R[3 * r + q] = k.T[4 * r + q]; t[r] = k.T[4 * r + 3]; }
    for (int r = 0; r < 3; r++) { double s = 0; for (int q = 0; q < 3; q++) s += (double)R[3 * q + r] * (double)t[q]; Ow[r] = (float)(s * -1.0); }
    const float fx = k.cam[0], fy = k.cam[1], cx = k.cam[2], cy = k.cam[3];
    std::vector<size_t> vIndices;
    for (int i = 0; i < c.n; i++) {
        bi[i] = -1; bd[i] = 256; gate[i] = 1;
        if (k.skip[i]) continue;
        float S[3], E[3];
        for (int q = 0; q < 3; q++) { S[q] = (float)c.pos[6 * (size_t)i + q]; E[q] = (float)c.pos[6 * (size_t)i + 3 + q]; }
        const float sx = row(R, S, t[0]), sy = row(R + 3, S, t[1]), sz = row(R + 6, S, t[2]);
        const float ex = row(R, E, t[0]), ey = row(R + 3, E, t[1]), ez = row(R + 6, E, t[2]);
        gate[i] = 2;
        if (sz < 0.0f || ez < 0.0f) continue;
        const float invz1 = 1.0f / sz, u1 = fx * sx * invz1 + cx, v1 = fy * sy * invz1 + cy;
        gate[i] = 3;
        if (!(u1 >= k.b[0] && u1 < k.b[1] && v1 >= k.b[2] && v1 < k.b[3])) continue;
        const float invz2 = 1.0f / ez, u2 = fx * ex * invz2 + cx, v2 = fy * ey * invz2 + cy;
        if (!(u2 >= k.b[0] && u2 < k.b[1] && v2 >= k.b[2] && v2 < k.b[3])) continue;
        const float maxD = 1.2f * c.maxd[i], minD = 0.8f * c.mind[i];
        double d[3];
        for (int q = 0; q < 3; q++) { const float mid = (float)((double)S[q] * 0.5 + (double)E[q] * 0.5); d[q] = (double)(mid - Ow[q]); }
        const float dist = (float)std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (dist < minD) { gate[i] = 4; continue; }
        if (dist > maxD) { gate[i] = 5; continue; }
        const double dot = d[0] * (double)(float)c.nrm[3 * (size_t)i] + d[1] * (double)(float)c.nrm[3 * (size_t)i + 1] + d[2] * (double)(float)c.nrm[3 * (size_t)i + 2];
        if (dot < 0.5 * dist) { gate[i] = 6; continue; }
        const float ratio = c.maxd[i] / dist;
        int lvl = to_level(std::ceil(std::log(ratio) / c.logsf));
        if (c.rule) { if (lvl < 0 || lvl >= c.n_levels) { gate[i] = 7; continue; } }
        else lvl = lvl < 0 ? 0 : lvl >= c.n_levels ? c.n_levels - 1 : lvl;
        gate[i] = 0;
        const float radius = c.th * sf[lvl];
        lines_in_area(k, u1, v1, u2, v2, radius, vIndices);
        int bestDist = 256, bestIdx = -1;
        for (size_t idx : vIndices) {
            const int o = k.oct[idx];
            if (o < lvl - 1 || o > lvl) continue;
            if ((int)idx >= k.nr) continue;
            const int dd = ham(&c.desc[32 * (size_t)i], &k.rows[32 * idx]);
            if (dd < bestDist) { bestDist = dd; bestIdx = (int)idx; }
        }
        bi[i] = bestIdx; bd[i] = bestDist;
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: line_fuse_host <case> <result> [reps]\n"); return 2; }
    const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    Case c; int32_t h[5]; float p[3];
    rd(f, h, 5); rd(f, p, 3);
    c.n_kf = h[0]; c.n = h[1]; c.n_levels = h[2]; c.th_low = h[3]; c.rule = h[4]; c.th = p[0]; c.logsf = p[1]; c.scale = p[2];
    const size_t n = (size_t)c.n;
    rd(f, c.pos, n * 6); rd(f, c.nrm, n * 3); rd(f, c.maxd, n); rd(f, c.mind, n); rd(f, c.desc, n * 32);
    c.kf.resize((size_t)c.n_kf);
    for (KF &k : c.kf) {
        int32_t m[2]; rd(f, m, 2); k.nl = m[0]; k.nr = m[1];
        rd(f, k.T, 12); rd(f, k.cam, 4); rd(f, k.b, 4);
        const size_t nl = (size_t)k.nl;
        rd(f, k.ptx, nl); rd(f, k.pty, nl); rd(f, k.sx, nl); rd(f, k.sy, nl); rd(f, k.ex, nl); rd(f, k.ey, nl); rd(f, k.oct, nl);
        rd(f, k.rows, (size_t)k.nr * 32); rd(f, k.skip, n);
    }
    fclose(f);
    float sf[16]; sf[0] = 1.0f;
    for (int l = 1; l < 16; l++) sf[l] = l < c.n_levels ? sf[l - 1] * c.scale : 1.0f;
    std::vector<int32_t> bi((size_t)c.n_kf * n), bd((size_t)c.n_kf * n); std::vector<int8_t> gate((size_t)c.n_kf * n);
    std::vector<double> ms;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int j = 0; j < c.n_kf; j++) fuse(c, c.kf[j], sf, &bi[j * n], &bd[j * n], &gate[j * n]);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%.4f\n", ms[ms.size() / 2]);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    for (int j = 0; j < c.n_kf; j++) { fwrite(&bi[j * n], 4, n, f); fwrite(&bd[j * n], 4, n, f); fwrite(&gate[j * n], 1, n, f); }
    fclose(f);
    return 0;
}
