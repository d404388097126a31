// new_points_host.cpp -- a plain single-thread host restatement of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:335-580)
// as the reference runs it: neighbour by neighbour, SearchForTriangulation over real per-node lists, every match triangulated in order, the
// occupancy byte set as points are created.  It is what tools/new_points_timing.py measures beside the device call, with the readings of
// csrc/new_points.hip (tests/new_points_ref.py is their definition), so its answers equal the device's.
// Build: g++ -O2 -ffp-contract=off tools/new_points_host.cpp -o new_points_host
//
//   new_points_host case.bin result.bin [reps]
//
// case.bin (little endian; written by tools/new_points_timing.py): int32 n_kf, n_levels, th_low; float fx, fy, cx, cy, bf, scale_factor,
// mvScaleFactors[16], mvLevelSigma2[16]; then the current key frame and the n_kf neighbours, each: int32 n, stereo, skip; float Tcw[12], mb;
// float x[n], y[n] (mvKeysUn), rx[n], ry[n] (mvKeys); int32 octave[n]; float uright[n], depth[n]; desc n x 32; int32 node[n]; has n bytes.
// result.bin: per neighbour int32 n_created, idx1[n_created], idx2[n_created], float x3d[3 n_created]; then int32 owner[n1].
// stdout: the median wall time in ms of `reps` runs of the whole function (the per-node lists of every key frame are built outside the timed
// part: a KeyFrame carries its FeatureVector).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

struct Cam { float fx, fy, cx, cy, bf, scale_factor, sf[16], sig[16]; int n_levels, th_low; };
struct Kf {
    int n, stereo, skip; float T[12], mb; std::vector<float> x, y, rx, ry, ur, depth; std::vector<int32_t> oct, node; std::vector<uint8_t> desc, has;
    std::map<int, std::vector<int> > fv;                             // DBoW2::FeatureVector
    float R[9], t[3], Ow[3];
};
struct Created { std::vector<int32_t> i1, i2; std::vector<float> x; };

static float dot3f(float a0, float a1, float a2, float b0, float b1, float b2) { float s = a0 * b0; s = s + a1 * b1; s = s + a2 * b2; return s; }
static float row(float a0, float a1, float a2, float b0, float b1, float b2, float c) { return (float)((double)dot3f(a0, a1, a2, b0, b1, b2) * 1.0 + (double)c * 1.0); }
static double dotd(float a0, float a1, float a2, float b0, float b1, float b2) { double s = (double)a0 * (double)b0; s = s + (double)a1 * (double)b1; s = s + (double)a2 * (double)b2; return s; }
static double normd(float a0, float a1, float a2) { return std::sqrt(dotd(a0, a1, a2, a0, a1, a2)); }

static void pose(Kf &k)
{
    for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) k.R[3 * r + q] = k.T[4 * r + q]; k.t[r] = k.T[4 * r + 3]; }
    for (int r = 0; r < 3; r++) { double s = 0; for (int q = 0; q < 3; q++) s += (double)k.R[3 * q + r] * (double)k.t[q]; k.Ow[r] = (float)(s * -1.0); }
}
static void inv3(const float *m, float *o)
{
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5], a20 = m[6], a21 = m[7], a22 = m[8];
    double d = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    d = 1.0 / d;
    o[0] = (float)((a11 * a22 - a12 * a21) * d); o[1] = (float)((a02 * a21 - a01 * a22) * d); o[2] = (float)((a01 * a12 - a02 * a11) * d);
    o[3] = (float)((a12 * a20 - a10 * a22) * d); o[4] = (float)((a00 * a22 - a02 * a20) * d); o[5] = (float)((a02 * a10 - a00 * a12) * d);
    o[6] = (float)((a10 * a21 - a11 * a20) * d); o[7] = (float)((a01 * a20 - a00 * a21) * d); o[8] = (float)((a00 * a11 - a01 * a10) * d);
}
static void mul3(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) C[3 * r + c] = dot3f(A[3 * r], A[3 * r + 1], A[3 * r + 2], B[c], B[3 + c], B[6 + c]);
}
static void compute_f12(const Cam &c, const Kf &k1, const Kf &k2, float *F)
{
    float R12[9], t12[3];
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) R12[3 * r + q] = dot3f(k1.R[3 * r], k1.R[3 * r + 1], k1.R[3 * r + 2], k2.R[3 * q], k2.R[3 * q + 1], k2.R[3 * q + 2]);
    for (int r = 0; r < 3; r++) t12[r] = row(-R12[3 * r], -R12[3 * r + 1], -R12[3 * r + 2], k2.t[0], k2.t[1], k2.t[2], k1.t[r]);
    const float tx[9] = { 0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f };
    const float Kt[9] = { c.fx, 0.f, 0.f, 0.f, c.fy, 0.f, c.cx, c.cy, 1.f }, Km[9] = { c.fx, 0.f, c.cx, 0.f, c.fy, c.cy, 0.f, 0.f, 1.f };
    float Kti[9], Ki[9], M1[9], M2[9];
    inv3(Kt, Kti); inv3(Km, Ki); mul3(Kti, tx, M1); mul3(M1, R12, M2); mul3(M2, Ki, F);
}

static int hamming(const uint8_t *a, const uint8_t *b)
{
    uint64_t x[4], y[4]; memcpy(x, a, 32); memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

// ORBmatcher::SearchForTriangulation with mbCheckOrientation = false, bOnlyStereo = false
static void search(const Cam &c, const Kf &k1, const Kf &k2, const float *F, const std::vector<uint8_t> &has1, std::vector<int> &m12)
{
    const float C0 = row(k2.R[0], k2.R[1], k2.R[2], k1.Ow[0], k1.Ow[1], k1.Ow[2], k2.t[0]), C1 = row(k2.R[3], k2.R[4], k2.R[5], k1.Ow[0], k1.Ow[1], k1.Ow[2], k2.t[1]),
                C2 = row(k2.R[6], k2.R[7], k2.R[8], k1.Ow[0], k1.Ow[1], k1.Ow[2], k2.t[2]);
    const float invz = 1.0f / C2;
    const float ex = c.fx * C0 * invz + c.cx, ey = c.fy * C1 * invz + c.cy;
    m12.assign((size_t)k1.n, -1);
    auto f1 = k1.fv.begin(); auto f2 = k2.fv.begin();
    while (f1 != k1.fv.end() && f2 != k2.fv.end()) {
        if (f1->first == f2->first) {
            for (int i1 : f1->second) {
                if (has1[i1]) continue;
                const int o1 = k1.oct[i1];
                if (o1 < 0 || o1 >= c.n_levels) continue;
                const bool st1 = k1.ur[i1] >= 0;
                const float x1 = k1.x[i1], y1 = k1.y[i1];
                const float a = x1 * F[0] + y1 * F[3] + F[6], b = x1 * F[1] + y1 * F[4] + F[7], cc = x1 * F[2] + y1 * F[5] + F[8];
                const float den = a * a + b * b;
                int bestDist = c.th_low, best = -1;
                for (int i2 : f2->second) {
                    if (k2.has[i2]) continue;
                    const int dist = hamming(&k1.desc[32 * (size_t)i1], &k2.desc[32 * (size_t)i2]);
                    if (dist > c.th_low || dist > bestDist) continue;
                    const int o2 = k2.oct[i2];
                    if (o2 < 0 || o2 >= c.n_levels) continue;
                    const float x2 = k2.x[i2], y2 = k2.y[i2];
                    if (!st1 && !(k2.ur[i2] >= 0)) {
                        const float dx = ex - x2, dy = ey - y2;
                        if (dx * dx + dy * dy < 100.0f * c.sf[o2]) continue;
                    }
                    if (den == 0) continue;
                    const float num = a * x2 + b * y2 + cc;
                    const float dsqr = num * num / den;
                    if ((double)dsqr < 3.84 * (double)c.sig[o2]) { best = i2; bestDist = dist; }
                }
                m12[i1] = best;
            }
            ++f1; ++f2;
        } else if (f1->first < f2->first) f1 = k1.fv.lower_bound(f2->first);
        else f2 = k2.fv.lower_bound(f1->first);
    }
}

static void rot(double num, double den2, double *c, double *s)
{
    if (den2 * 0.5 == 0.0) { *c = 1.0; *s = 0.0; return; }
    const double th = num / den2, at = th < 0.0 ? -th : th;
    double tt = 1.0 / (at + std::sqrt(th * th + 1.0));
    if (th < 0.0) tt = -tt;
    const double cc = 1.0 / std::sqrt(tt * tt + 1.0);
    *c = cc; *s = tt * cc;
}
static void svd4(const float A[4][4], float x[4])
{
    double W[4][4], V[4][4];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { W[r][c] = A[r][c]; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sw = 0; sw < 12; sw++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 4; r++) { const double wp = W[r][p], wq = W[r][q]; al = al + wp * wp; be = be + wq * wq; ga = ga + wp * wq; }
                double c, s; rot(be - al, 2.0 * ga, &c, &s);
                for (int r = 0; r < 4; r++) {
                    const double wp = W[r][p], wq = W[r][q], vp = V[r][p], vq = V[r][q];
                    W[r][p] = c * wp - s * wq; W[r][q] = s * wp + c * wq; V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
                }
            }
    double best = 0;
    for (int c = 0; c < 4; c++) {
        double s2 = 0;
        for (int r = 0; r < 4; r++) s2 = s2 + W[r][c] * W[r][c];
        if (c == 0 || s2 <= best) { best = s2; for (int r = 0; r < 4; r++) x[r] = (float)V[r][c]; }
    }
}
static float stereo_cos(float mb, float depth)
{
    const double h = (double)(mb / 2), d = (double)depth, dd = d * d, hh = h * h;
    return (float)((dd - hh) / (dd + hh));
}
static bool reproj_fails(const Cam &c, const Kf &k, const float *X, float z, float kx, float ky, float kur, bool stereo, float sigma2)
{
    const float x = (float)(dotd(k.R[0], k.R[1], k.R[2], X[0], X[1], X[2]) + (double)k.t[0]), y = (float)(dotd(k.R[3], k.R[4], k.R[5], X[0], X[1], X[2]) + (double)k.t[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = c.fx * x * invz + c.cx, v = c.fy * y * invz + c.cy;
    const float ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float ur = u - c.bf * invz, er = ur - kur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// LocalMapping.cc:416-559 for one match: true when the point is created
static bool triangulate(const Cam &c, const Kf &k1, const Kf &k2, int i1, int i2, float *X)
{
    const float invfx = 1.0f / c.fx, invfy = 1.0f / c.fy;
    const float ur1 = k1.ur[i1], ur2 = k2.ur[i2];
    const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
    const float x1n = (k1.x[i1] - c.cx) * invfx, y1n = (k1.y[i1] - c.cy) * invfy, x2n = (k2.x[i2] - c.cx) * invfx, y2n = (k2.y[i2] - c.cy) * invfy;
    const float *A = k1.R, *B = k2.R;
    const float r10 = dot3f(A[0], A[3], A[6], x1n, y1n, 1.f), r11 = dot3f(A[1], A[4], A[7], x1n, y1n, 1.f), r12 = dot3f(A[2], A[5], A[8], x1n, y1n, 1.f);
    const float r20 = dot3f(B[0], B[3], B[6], x2n, y2n, 1.f), r21 = dot3f(B[1], B[4], B[7], x2n, y2n, 1.f), r22 = dot3f(B[2], B[5], B[8], x2n, y2n, 1.f);
    const float cosr = (float)(dotd(r10, r11, r12, r20, r21, r22) / (normd(r10, r11, r12) * normd(r20, r21, r22)));
    const float cs = cosr + 1.0f;
    float s1 = cs, s2 = cs;
    if (st1) s1 = stereo_cos(k1.mb, k1.depth[i1]);
    else if (st2) s2 = stereo_cos(k2.mb, k2.depth[i2]);
    const float cst = s2 < s1 ? s2 : s1;
    if (cosr < cst && cosr > 0.f && (st1 || st2 || (double)cosr < 0.9998)) {
        float W[4][4], x[4];
        const float T1[3][4] = { { A[0], A[1], A[2], k1.t[0] }, { A[3], A[4], A[5], k1.t[1] }, { A[6], A[7], A[8], k1.t[2] } };
        const float T2[3][4] = { { B[0], B[1], B[2], k2.t[0] }, { B[3], B[4], B[5], k2.t[1] }, { B[6], B[7], B[8], k2.t[2] } };
        for (int q = 0; q < 4; q++) {
            W[0][q] = x1n * T1[2][q] - T1[0][q]; W[1][q] = y1n * T1[2][q] - T1[1][q]; W[2][q] = x2n * T2[2][q] - T2[0][q]; W[3][q] = y2n * T2[2][q] - T2[1][q];
        }
        svd4(W, x);
        if (x[3] == 0.f) return false;
        const double iw = 1.0 / (double)x[3];
        for (int q = 0; q < 3; q++) X[q] = (float)((double)x[q] * iw);
    } else if ((st1 && s1 < s2) || (st2 && s2 < s1)) {
        const bool first = st1 && s1 < s2;
        const Kf &k = first ? k1 : k2; const int i = first ? i1 : i2;
        const float z = k.depth[i];
        if (!(z > 0.f)) return false;
        const float xc = (k.rx[i] - c.cx) * z * invfx, yc = (k.ry[i] - c.cy) * z * invfy;
        for (int q = 0; q < 3; q++) X[q] = row(k.R[q], k.R[3 + q], k.R[6 + q], xc, yc, z, k.Ow[q]);
    } else return false;
    const float z1 = (float)(dotd(A[6], A[7], A[8], X[0], X[1], X[2]) + (double)k1.t[2]);
    if (z1 <= 0.f) return false;
    const float z2 = (float)(dotd(B[6], B[7], B[8], X[0], X[1], X[2]) + (double)k2.t[2]);
    if (z2 <= 0.f) return false;
    const int o1 = k1.oct[i1], o2 = k2.oct[i2];
    if (reproj_fails(c, k1, X, z1, k1.x[i1], k1.y[i1], ur1, st1, c.sig[o1])) return false;
    if (reproj_fails(c, k2, X, z2, k2.x[i2], k2.y[i2], ur2, st2, c.sig[o2])) return false;
    const float d1 = (float)normd(X[0] - k1.Ow[0], X[1] - k1.Ow[1], X[2] - k1.Ow[2]), d2 = (float)normd(X[0] - k2.Ow[0], X[1] - k2.Ow[1], X[2] - k2.Ow[2]);
    if (d1 == 0.f || d2 == 0.f) return false;
    const float rd = d2 / d1, ro = c.sf[o1] / c.sf[o2], rf = 1.5f * c.scale_factor;
    return !(rd * rf < ro || rd > ro * rf);
}

static void create_new_map_points(const Cam &c, const Kf &cur, const std::vector<Kf> &nb, std::vector<Created> &out, std::vector<int32_t> &owner)
{
    std::vector<uint8_t> has1 = cur.has;
    owner.assign((size_t)cur.n, -1); out.assign(nb.size(), Created());
    std::vector<int> m12;
    for (size_t j = 0; j < nb.size(); j++) {
        const Kf &k2 = nb[j];
        const float baseline = (float)normd(k2.Ow[0] - cur.Ow[0], k2.Ow[1] - cur.Ow[1], k2.Ow[2] - cur.Ow[2]);
        if (k2.skip || baseline < k2.mb) continue;
        float F[9]; compute_f12(c, cur, k2, F);
        search(c, cur, k2, F, has1, m12);
        for (int i1 = 0; i1 < cur.n; i1++) {
            if (m12[i1] < 0) continue;
            float X[3];
            if (!triangulate(c, cur, k2, i1, m12[i1], X)) continue;
            has1[i1] = 1; owner[i1] = (int32_t)j;
            out[j].i1.push_back(i1); out[j].i2.push_back(m12[i1]); out[j].x.insert(out[j].x.end(), X, X + 3);
        }
    }
}

template <class T> static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
static bool read_kf(FILE *f, Kf &k)
{
    int32_t h[3];
    if (!rd(f, h, 3) || !rd(f, k.T, 12) || !rd(f, &k.mb, 1)) return false;
    k.n = h[0]; k.stereo = h[1]; k.skip = h[2];
    const size_t n = (size_t)k.n;
    k.x.resize(n); k.y.resize(n); k.rx.resize(n); k.ry.resize(n); k.oct.resize(n); k.ur.resize(n); k.depth.resize(n); k.desc.resize(n * 32); k.node.resize(n); k.has.resize(n);
    if (!rd(f, k.x.data(), n) || !rd(f, k.y.data(), n) || !rd(f, k.rx.data(), n) || !rd(f, k.ry.data(), n) || !rd(f, k.oct.data(), n) || !rd(f, k.ur.data(), n) ||
        !rd(f, k.depth.data(), n) || !rd(f, k.desc.data(), n * 32) || !rd(f, k.node.data(), n) || !rd(f, k.has.data(), n)) return false;
    if (!k.stereo) for (size_t i = 0; i < n; i++) { k.ur[i] = -1.f; k.depth[i] = -1.f; }
    for (int i = 0; i < k.n; i++) if (k.node[i] >= 0) k.fv[k.node[i]].push_back(i);
    pose(k);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s case.bin result.bin [reps]\n", argv[0]); return 2; }
    const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t h[3]; Cam c;
    if (!rd(f, h, 3) || !rd(f, &c.fx, 6) || !rd(f, c.sf, 16) || !rd(f, c.sig, 16)) return 3;
    c.n_levels = h[1]; c.th_low = h[2];
    Kf cur; std::vector<Kf> nb((size_t)h[0]);
    if (!read_kf(f, cur)) return 3;
    for (Kf &k : nb) if (!read_kf(f, k)) return 3;
    fclose(f);
    std::vector<Created> out; std::vector<int32_t> owner; std::vector<double> ms;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        create_new_map_points(c, cur, nb, out, owner);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    for (const Created &o : out) {
        const int32_t n = (int32_t)o.i1.size();
        fwrite(&n, 4, 1, f); fwrite(o.i1.data(), 4, o.i1.size(), f); fwrite(o.i2.data(), 4, o.i2.size(), f); fwrite(o.x.data(), 4, o.x.size(), f);
    }
    fwrite(owner.data(), 4, owner.size(), f);
    fclose(f);
    printf("%.4f\n", ms[ms.size() / 2]);
    return 0;
}
