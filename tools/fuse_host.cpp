// fuse_host.cpp -- a plain single-thread host restatement of ORBmatcher::Fuse(pKF, vpMapPoints, th) (reference src/ORBmatcher.cc:838-994)
// with real per-cell lists and one call per key frame: what tools/fuse_timing.py measures beside the device call, and what
// tests/test_fuse.py ties to tests/fuse_ref.py.  Build: g++ -O2 -ffp-contract=off tools/fuse_host.cpp -o fuse_host
//
//   fuse_host case.bin result.bin [reps]
//
// case.bin (little endian; written by tools/fuse_host_io.py): int32 n_kf, n_map, n_levels, th_low; float fx, fy, cx, cy, bf, bounds[4], th,
// log_scale_factor, mvScaleFactors[16], mvInvLevelSigma2[16]; the map side: pos n x 3, normal n x 3, max_dist n, min_dist n (floats),
// desc n x 32; then per key frame: int32 n_feat, float Tcw[12], x[n_feat], y[n_feat], int32 octave[n_feat], float uright[n_feat] (-1: none),
// desc n_feat x 32, skip n_map bytes.  result.bin: per key frame int32 best_idx[n_map], best_dist[n_map], int8 gate[n_map].
// stdout: the median wall time in ms of `reps` runs over all key frames (the grid of each key frame is built inside the timed part, as
// KeyFrame's constructor has built it once; reported separately).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

enum { COLS = 64, ROWS = 48 };
struct Cam { float fx, fy, cx, cy, bf, minX, maxX, minY, maxY, th, logsf, sf[16], isig[16]; int n_levels, th_low; };
struct Map { int n; std::vector<float> pos, nrm, maxd, mind; std::vector<uint8_t> desc; };
struct Kf {
    int n; float T[12]; std::vector<float> x, y, ur; std::vector<int32_t> oct; std::vector<uint8_t> desc, skip;
    std::vector<int> grid[COLS][ROWS];
};

static float row(const float *a, float b0, float b1, float b2, float c)
{
    float t = a[0] * b0; t = t + a[1] * b1; t = t + a[2] * b2;
    return (float)((double)t * 1.0 + (double)c * 1.0);
}

static int to_int(float v) { return v != v ? 0 : v >= 2147483648.0f ? 2147483647 : v <= -2147483648.0f ? (-2147483647 - 1) : (int)v; }

static void build_grid(const Cam &c, Kf &k)
{
    const float invW = (float)COLS / (c.maxX - c.minX), invH = (float)ROWS / (c.maxY - c.minY);
    for (int ix = 0; ix < COLS; ix++) for (int iy = 0; iy < ROWS; iy++) k.grid[ix][iy].clear();
    for (int i = 0; i < k.n; i++) {
        const float px = std::round((k.x[i] - c.minX) * invW), py = std::round((k.y[i] - c.minY) * invH);
        if (!(px >= 0.f && px < (float)COLS && py >= 0.f && py < (float)ROWS)) continue;
        k.grid[(int)px][(int)py].push_back(i);
    }
}

static int popcount256(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int w = 0; w < 4; w++) { uint64_t x, y; memcpy(&x, a + 8 * w, 8); memcpy(&y, b + 8 * w, 8); d += __builtin_popcountll(x ^ y); }
    return d;
}

static void fuse(const Cam &c, const Map &m, const Kf &k, int32_t *bi, int32_t *bd, int8_t *gate)
{
    const float invW = (float)COLS / (c.maxX - c.minX), invH = (float)ROWS / (c.maxY - c.minY);
    float Ow[3];
    for (int r = 0; r < 3; r++) { double s = 0; for (int q = 0; q < 3; q++) s += (double)k.T[4 * q + r] * (double)k.T[4 * q + 3]; Ow[r] = (float)(s * -1.0); }
    const float R[9] = { k.T[0], k.T[1], k.T[2], k.T[4], k.T[5], k.T[6], k.T[8], k.T[9], k.T[10] };
    std::vector<int> idx;
    for (int i = 0; i < m.n; i++) {
        bi[i] = -1; bd[i] = 256; gate[i] = 1;
        if (k.skip[i]) continue;
        const float X = m.pos[3 * i], Y = m.pos[3 * i + 1], Z = m.pos[3 * i + 2];
        const float xc = row(R, X, Y, Z, k.T[3]), yc = row(R + 3, X, Y, Z, k.T[7]), zc = row(R + 6, X, Y, Z, k.T[11]);
        gate[i] = 2; if (zc < 0.0f) continue;
        const float invz = 1 / zc, x = xc * invz, y = yc * invz;
        const float u = c.fx * x + c.cx, v = c.fy * y + c.cy;
        gate[i] = 3; if (!(u >= c.minX && u < c.maxX && v >= c.minY && v < c.maxY)) continue;
        const float ur = u - c.bf * invz;
        const float maxD = 1.2f * m.maxd[i], minD = 0.8f * m.mind[i];
        const double d0 = X - Ow[0], d1 = Y - Ow[1], d2 = Z - Ow[2];
        const float dist = (float)std::sqrt((d0 * d0 + d1 * d1) + d2 * d2);
        gate[i] = 4; if (dist < minD) continue;
        gate[i] = 5; if (dist > maxD) continue;
        const double dot = (d0 * (double)m.nrm[3 * i] + d1 * (double)m.nrm[3 * i + 1]) + d2 * (double)m.nrm[3 * i + 2];
        gate[i] = 6; if (dot < 0.5 * (double)dist) continue;
        gate[i] = 0;
        const float ratio = m.maxd[i] / dist;
        int lvl = to_int(std::ceil(std::log(ratio) / c.logsf));
        if (lvl < 0) lvl = 0; else if (lvl >= c.n_levels) lvl = c.n_levels - 1;
        const float r = c.th * c.sf[lvl];
        // KeyFrame::GetFeaturesInArea
        idx.clear();
        do {
            const int x0 = std::max(0, to_int(std::floor((u - c.minX - r) * invW))); if (x0 >= COLS) break;
            const int x1 = std::min((int)COLS - 1, to_int(std::ceil((u - c.minX + r) * invW))); if (x1 < 0) break;
            const int y0 = std::max(0, to_int(std::floor((v - c.minY - r) * invH))); if (y0 >= ROWS) break;
            const int y1 = std::min((int)ROWS - 1, to_int(std::ceil((v - c.minY + r) * invH))); if (y1 < 0) break;
            for (int ix = x0; ix <= x1; ix++) for (int iy = y0; iy <= y1; iy++) for (int j : k.grid[ix][iy]) {
                const float dx = k.x[j] - u, dy = k.y[j] - v;
                if (std::fabs(dx) < r && std::fabs(dy) < r) idx.push_back(j);
            }
        } while (0);
        int best = 256, bidx = -1;
        for (int j : idx) {
            const int o = k.oct[j];
            if (o < lvl - 1 || o > lvl || o < 0) continue;
            const float ex = u - k.x[j], ey = v - k.y[j];
            if (k.ur[j] >= 0) { const float er = ur - k.ur[j]; const float e2 = ex * ex + ey * ey + er * er; if (e2 * c.isig[o] > 7.8) continue; }
            else { const float e2 = ex * ex + ey * ey; if (e2 * c.isig[o] > 5.99) continue; }
            const int d = popcount256(&m.desc[32 * (size_t)i], &k.desc[32 * (size_t)j]);
            if (d < best) { best = d; bidx = j; }
        }
        bi[i] = bidx; bd[i] = best;
    }
}

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: fuse_host case.bin result.bin [reps]\n"); return 2; }
    const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int32_t hd[4]; Cam c; float fl[11];
    bool ok = rd(f, hd, 4) && rd(f, fl, 11) && rd(f, c.sf, 16) && rd(f, c.isig, 16);
    if (!ok || hd[0] < 0 || hd[1] < 0) { fprintf(stderr, "bad header\n"); return 1; }
    c.fx = fl[0]; c.fy = fl[1]; c.cx = fl[2]; c.cy = fl[3]; c.bf = fl[4]; c.minX = fl[5]; c.maxX = fl[6]; c.minY = fl[7]; c.maxY = fl[8]; c.th = fl[9]; c.logsf = fl[10];
    c.n_levels = hd[2]; c.th_low = hd[3];
    Map m; m.n = hd[1];
    const size_t n = (size_t)m.n;
    m.pos.resize(3 * n); m.nrm.resize(3 * n); m.maxd.resize(n); m.mind.resize(n); m.desc.resize(32 * n);
    ok = rd(f, m.pos.data(), 3 * n) && rd(f, m.nrm.data(), 3 * n) && rd(f, m.maxd.data(), n) && rd(f, m.mind.data(), n) && rd(f, m.desc.data(), 32 * n);
    std::vector<Kf> kfs((size_t)hd[0]);
    for (Kf &k : kfs) {
        int32_t nf = 0;
        ok = ok && rd(f, &nf, 1) && nf >= 0 && rd(f, k.T, 12);
        if (!ok) break;
        k.n = nf; k.x.resize(nf); k.y.resize(nf); k.oct.resize(nf); k.ur.resize(nf); k.desc.resize(32 * (size_t)nf); k.skip.resize(n);
        ok = rd(f, k.x.data(), nf) && rd(f, k.y.data(), nf) && rd(f, k.oct.data(), nf) && rd(f, k.ur.data(), nf) && rd(f, k.desc.data(), 32 * (size_t)nf) && rd(f, k.skip.data(), n);
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "short case file\n"); return 1; }
    std::vector<int32_t> bi(kfs.size() * n), bd(kfs.size() * n); std::vector<int8_t> gate(kfs.size() * n);
    std::vector<double> t_grid, t_fuse;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (Kf &k : kfs) build_grid(c, k);
        const auto t1 = std::chrono::steady_clock::now();
        for (size_t j = 0; j < kfs.size(); j++) fuse(c, m, kfs[j], &bi[j * n], &bd[j * n], &gate[j * n]);
        const auto t2 = std::chrono::steady_clock::now();
        t_grid.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); t_fuse.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::sort(t_grid.begin(), t_grid.end()); std::sort(t_fuse.begin(), t_fuse.end());
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    for (size_t j = 0; j < kfs.size(); j++) { fwrite(&bi[j * n], 4, n, o); fwrite(&bd[j * n], 4, n, o); fwrite(&gate[j * n], 1, n, o); }
    fclose(o);
    printf("%.4f %.4f\n", t_grid[t_grid.size() / 2], t_fuse[t_fuse.size() / 2]);
    return 0;
}
