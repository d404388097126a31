// new_lines_host.cpp -- LocalMapping::CreateNewMapLinesConstraint (reference src/LocalMapping.cc:1064-1565) as a plain single-thread host
// program: the SEQUENTIAL loops as written (the searches neighbour by neighbour, the compacted list of match vectors, key frames by list
// position or aligned, every triple in (a, b, ikl) order under the occupancy as it stands) with the readings of csrc/line_triang.hip, whose
// shared arithmetic (csrc/triangulate4.inc) it includes.  tools/new_lines_timing.py times it beside the device call and compares the answers.
//
//   new_lines_host <case file> <result file> <reps>        prints the median wall ms of the loop over <reps> runs
//
// case file: int32 n_kf, n_levels, th_high, pairing; float32 nn_ratio, scale_factor; then the current key frame and the n_kf neighbours, each
//   int32 n, skip; float32 Tcw[12], fx, fy, cx, cy, mb, median_depth; n key lines (68 bytes each); n x 3 double; n x 32 bytes; n occupancy bytes
// result file: int32 n_pairs; per pair int32 kf2, kf3, mv2, mv3, n, then n x int32 ikl, idx1, idx2 and n x 6 float32; then n1 x int32 owner_pair
//
// build:  g++ -std=c++14 -O2 -ffp-contract=off -Iinclude tools/new_lines_host.cpp -o new_lines_host
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <vector>
#include "hvo.h"
#define __host__
#define __device__
#define __forceinline__ inline
#include "../a-low-texture-robust-hybrid-feature-based-visual-odometry_amd/csrc/triangulate4.inc"
#include "../a-low-texture-robust-hybrid-feature-based-visual-odometry_amd/csrc/call_stage.hpp"

struct Kf {
    int n, skip; float Tcw[12], fx, fy, cx, cy, mb, med;
    std::vector<hvo_keyline> kl; std::vector<double> fn; std::vector<uint8_t> desc, has;
    float R[9], t[3], Ow[3], Ki[9], M[12], F21[9], R1k[9]; int gate;
};
struct Pair { int kf2, kf3, mv2, mv3; std::vector<int> c0, c1, c2; std::vector<float> x; };

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool read_kf(FILE *f, Kf &k)
{
    int h[2]; float g[18];
    if (!rd(f, h, 8) || !rd(f, g, 72)) return false;
    k.n = h[0]; k.skip = h[1]; memcpy(k.Tcw, g, 48); k.fx = g[12]; k.fy = g[13]; k.cx = g[14]; k.cy = g[15]; k.mb = g[16]; k.med = g[17];
    k.kl.resize(k.n); k.fn.resize(3 * (size_t)k.n); k.desc.resize(32 * (size_t)k.n); k.has.resize(k.n);
    return rd(f, k.kl.data(), sizeof(hvo_keyline) * k.n) && rd(f, k.fn.data(), 24 * (size_t)k.n) && rd(f, k.desc.data(), 32 * (size_t)k.n) && rd(f, k.has.data(), k.n);
}

static void constants(Kf &c, const Kf *c1)
{
    pose_split(c.Tcw, c.R, c.t, c.Ow);
    const float Km[9] = { c.fx, 0.f, c.cx, 0.f, c.fy, c.cy, 0.f, 0.f, 1.f }, Kt[9] = { c.fx, 0.f, 0.f, 0.f, c.fy, 0.f, c.cx, c.cy, 1.f };
    np_inv3(Km, c.Ki);
    for (int r = 0; r < 3; r++) for (int q = 0; q < 4; q++)
        c.M[4 * r + q] = q < 3 ? np_dot3f(Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], c.R[q], c.R[3 + q], c.R[6 + q]) : np_dot3f(Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], c.t[0], c.t[1], c.t[2]);
    c.gate = 0;
    if (!c1) return;
    float R21[9], d[3], t21[3], Kti[9], M1[9], M2[9];
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) {
        R21[3 * r + q] = np_dot3f(c.R[3 * r], c.R[3 * r + 1], c.R[3 * r + 2], c1->R[3 * q], c1->R[3 * q + 1], c1->R[3 * q + 2]);
        c.R1k[3 * r + q] = np_dot3f(c1->R[3 * r], c1->R[3 * r + 1], c1->R[3 * r + 2], c.R[3 * q], c.R[3 * q + 1], c.R[3 * q + 2]);
    }
    for (int r = 0; r < 3; r++) d[r] = np_dot3f(c.R[r], c.R[3 + r], c.R[6 + r], c.t[0], c.t[1], c.t[2]) - np_dot3f(c1->R[r], c1->R[3 + r], c1->R[6 + r], c1->t[0], c1->t[1], c1->t[2]);
    for (int r = 0; r < 3; r++) t21[r] = np_dot3f(c.R[3 * r], c.R[3 * r + 1], c.R[3 * r + 2], d[0], d[1], d[2]);
    const float tx[9] = { 0.f, -t21[2], t21[1], t21[2], 0.f, -t21[0], -t21[1], t21[0], 0.f };
    np_inv3(Kt, Kti);
    np_mul3(Kti, tx, M1); np_mul3(M1, R21, M2); np_mul3(M2, c1->Ki, c.F21);
    const float baseline = (float)np_normd(c.Ow[0] - c1->Ow[0], c.Ow[1] - c1->Ow[1], c.Ow[2] - c1->Ow[2]);
    c.gate = c.skip ? 1 : (baseline < c.mb ? 2 : 0);
}

// LSDmatcher::FrameBFMatch with lineDescriptorMAD (src/LSDmatcher.cpp:942-966, 1110-1135)
static void frame_bf(const std::vector<uint8_t> &d1, int n1, const std::vector<uint8_t> &d2, int n2, float TH, float nnr, std::vector<int> &m)
{
    m.assign(n1, -1);
    if (n1 == 0 || n2 < 2) return;
    std::vector<int> bi(n1), b0(n1), b1(n1);
    for (int i = 0; i < n1; i++) {
        unsigned k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;
        const uint64_t *a = (const uint64_t *)(d1.data() + 32 * (size_t)i);
        for (int j = 0; j < n2; j++) {
            const uint64_t *b = (const uint64_t *)(d2.data() + 32 * (size_t)j);
            const unsigned d = __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) + __builtin_popcountll(a[3] ^ b[3]);
            const unsigned k = (d << 16) | (unsigned)j;
            if (k < k0) { k1 = k0; k0 = k; } else if (k < k1) k1 = k;
        }
        bi[i] = (int)(k0 & 0xFFFF); b0[i] = (int)(k0 >> 16); b1[i] = (int)(k1 >> 16);
    }
    std::vector<float> v(n1), w(n1);
    for (int i = 0; i < n1; i++) v[i] = (float)b1[i] - (float)b0[i];
    w = v; std::sort(w.begin(), w.end(), [](float x, float y) { return x > y; });
    const double med = (double)w[n1 / 2];
    for (int i = 0; i < n1; i++) w[i] = fabsf((float)((double)v[i] - med));
    std::sort(w.begin(), w.end());
    double th = 1.4826 * (double)w[n1 / 2];
    th = th * 0.5;
    for (int i = 0; i < n1; i++) if ((double)v[i] > th && (float)b0[i] < TH && (float)b0[i] < nnr * (float)b1[i]) m[i] = bi[i];
}

static void cross(const float *a, const float *b, float *c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; }
static void plane_normal(const float *Ki, const hvo_keyline &k, float *L)
{
    float s[3], e[3];
    for (int r = 0; r < 3; r++) { s[r] = np_dot3f(Ki[3 * r], Ki[3 * r + 1], Ki[3 * r + 2], k.sx, k.sy, 1.0f); e[r] = np_dot3f(Ki[3 * r], Ki[3 * r + 1], Ki[3 * r + 2], k.ex, k.ey, 1.0f); }
    cross(s, e, L);
}
static float epi_cos(const float *F, float x, float y, float lv0, float lv1)
{
    const float th0 = np_dot3f(F[0], F[1], F[2], x, y, 1.0f), th1 = np_dot3f(F[3], F[4], F[5], x, y, 1.0f);
    const float a0 = -th1, a1 = th0;
    const double dot = (double)a0 * (double)lv0 + (double)a1 * (double)lv1;
    return fabsf((float)(dot / (sqrt((double)a0 * (double)a0 + (double)a1 * (double)a1) * sqrt((double)lv0 * (double)lv0 + (double)lv1 * (double)lv1))));
}
static float camrow(const Kf &k, int r, const float *p) { return (float)(np_dotd(k.R[3 * r], k.R[3 * r + 1], k.R[3 * r + 2], p[0], p[1], p[2]) + (double)k.t[r]); }
static bool reproj_fails(const Kf &k, const float *p, float z, const double *fn, float sigma2, float *u, float *v)
{
    const float x = camrow(k, 0, p), y = camrow(k, 1, p), invz = (float)(1.0 / (double)z);
    *u = k.fx * x * invz + k.cx; *v = k.fy * y * invz + k.cy;
    const double err = (fn[0] * (double)*u + fn[1] * (double)*v) + fn[2];
    return err * err > 3.84 * (double)sigma2;
}
static int overlap(const hvo_keyline &k, float us, float vs, float ue, float ve)
{
    const double PI = 3.1415926, fa = fabs((double)k.angle);
    const bool vert = fa < 3.0 * PI / 4.0 && fa > 1.0 * PI / 4.0;
    const float pe = vert ? ve : ue, ps = vert ? vs : us, ks = vert ? k.sy : k.sx, ke = vert ? k.ey : k.ex;
    const float minp = ps < pe ? ps : pe, maxp = pe < ps ? ps : pe, maxk = ks < ke ? ke : ks, mink = ke < ks ? ke : ks;
    if (minp > maxk || mink > maxp) return 1;
    const float hi = maxk < maxp ? maxk : maxp, lo = minp < mink ? mink : minp;
    const float r1 = (hi - lo) / (maxp - minp), r2 = (hi - lo) / (maxk - mink);
    return ((double)r1 < 0.85 || (double)r2 < 0.85) ? 2 : 0;
}

// LocalMapping.cc:1205-1539 for one triple: true = a map line is created, its end points in S, E
static bool triple(const Kf &k1, const Kf &k2, const Kf &k3, int i, int i1, int i2, const float *sig, int n_levels, float *S, float *E)
{
    const hvo_keyline &l1 = k1.kl[i], &l2 = k2.kl[i1], &l3 = k3.kl[i2];
    const double *f1 = &k1.fn[3 * (size_t)i], *f2 = &k2.fn[3 * (size_t)i1], *f3 = &k3.fn[3 * (size_t)i2];
    if (l1.octave < 0 || l1.octave >= n_levels || l2.octave < 0 || l2.octave >= n_levels || l3.octave < 0 || l3.octave >= n_levels) return false;
    const float lv0 = -(float)f2[1], lv1 = (float)f2[0];
    if ((double)epi_cos(k2.F21, l1.sx, l1.sy, lv0, lv1) > 0.996 || (double)epi_cos(k2.F21, l1.ex, l1.ey, lv0, lv1) > 0.996) return false;
    float L1[3], L2[3], L3[3], w2[3], w3[3], tw[3];
    plane_normal(k1.Ki, l1, L1); plane_normal(k2.Ki, l2, L2); plane_normal(k3.Ki, l3, L3);
    for (int r = 0; r < 3; r++) {
        w2[r] = np_dot3f(k2.R1k[3 * r], k2.R1k[3 * r + 1], k2.R1k[3 * r + 2], L2[0], L2[1], L2[2]);
        w3[r] = np_dot3f(k3.R1k[3 * r], k3.R1k[3 * r + 1], k3.R1k[3 * r + 2], L3[0], L3[1], L3[2]);
    }
    cross(w2, w3, tw);
    float norm_ = (float)np_normd(tw[0], tw[1], tw[2]);
    if (norm_ == 0.f) return false;
    double inv = 1.0 / (double)norm_;
    for (int r = 0; r < 3; r++) tw[r] = (float)((double)tw[r] * inv);
    norm_ = (float)np_normd(L1[0], L1[1], L1[2]);
    if (norm_ == 0.f) return false;
    inv = 1.0 / (double)norm_;
    for (int r = 0; r < 3; r++) L1[r] = (float)((double)L1[r] * inv);
    if ((double)(float)fabs(np_dotd(L1[0], L1[1], L1[2], tw[0], tw[1], tw[2])) > 0.0087) return false;
    const float g3[3] = { (float)f3[0], (float)f3[1], (float)f3[2] }, g2[3] = { (float)f2[0], (float)f2[1], (float)f2[2] };
    for (int e = 0; e < 2; e++) {
        const float px = e ? l1.ex : l1.sx, py = e ? l1.ey : l1.sy;
        float W[4][4], x[4];
        for (int c = 0; c < 4; c++) {
            W[0][c] = np_dot3f(g3[0], g3[1], g3[2], k3.M[c], k3.M[4 + c], k3.M[8 + c]); W[1][c] = np_dot3f(g2[0], g2[1], g2[2], k2.M[c], k2.M[4 + c], k2.M[8 + c]);
            W[2][c] = px * k1.M[8 + c] - k1.M[c]; W[3][c] = py * k1.M[8 + c] - k1.M[4 + c];
        }
        np_svd4(W, x);
        if (x[3] == 0.f) return false;
        const double iw = 1.0 / (double)x[3];
        float *q = e ? E : S;
        for (int r = 0; r < 3; r++) q[r] = (float)((double)x[r] * iw);
    }
    float dS1 = 0.f, dS2 = 0.f;
    for (int e = 0; e < 2; e++) {
        const float *q = e ? E : S;
        const float n1[3] = { q[0] - k1.Ow[0], q[1] - k1.Ow[1], q[2] - k1.Ow[2] }, n2[3] = { q[0] - k2.Ow[0], q[1] - k2.Ow[1], q[2] - k2.Ow[2] }, n3[3] = { q[0] - k3.Ow[0], q[1] - k3.Ow[1], q[2] - k3.Ow[2] };
        const float d1 = (float)np_normd(n1[0], n1[1], n1[2]), d2 = (float)np_normd(n2[0], n2[1], n2[2]), d3 = (float)np_normd(n3[0], n3[1], n3[2]);
        const float c12 = (float)(np_dotd(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]) / (double)(d1 * d2)), c13 = (float)(np_dotd(n1[0], n1[1], n1[2], n3[0], n3[1], n3[2]) / (double)(d1 * d3));
        if ((double)c12 >= 0.99998 || (double)c13 >= 0.99998) return false;
        if (e == 0) { dS1 = d1; dS2 = d2; }
    }
    if ((double)(dS1 / k2.med) < 0.3 || (double)(dS2 / k2.med) < 0.3) return false;
    if ((float)np_normd(E[0] - S[0], E[1] - S[1], E[2] - S[2]) / k2.med > 1.0f) return false;
    const Kf *ks[3] = { &k1, &k2, &k3 }; const hvo_keyline *ls[3] = { &l1, &l2, &l3 }; const double *fs[3] = { f1, f2, f3 };
    float z[6], u[6], v[6];
    for (int q = 0; q < 6; q++) { z[q] = camrow(*ks[q / 2], 2, q & 1 ? E : S); if (z[q] <= 0.f) return false; }
    for (int q = 0; q < 6; q++) if (reproj_fails(*ks[q / 2], q & 1 ? E : S, z[q], fs[q / 2], sig[ls[q / 2]->octave], &u[q], &v[q])) return false;
    for (int q = 0; q < 3; q++) if (overlap(*ls[q], u[2 * q], v[2 * q], u[2 * q + 1], v[2 * q + 1])) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: new_lines_host <case> <result> <reps>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int h[4]; float g[2];
    if (!f || !rd(f, h, 16) || !rd(f, g, 8)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int n_kf = h[0], n_levels = h[1], th_high = h[2], pairing = h[3], reps = std::max(1, atoi(argv[3]));
    std::vector<Kf> in(n_kf + 1);
    for (int j = 0; j <= n_kf; j++) if (!read_kf(f, in[j])) { fprintf(stderr, "short case file\n"); return 2; }
    fclose(f);
    float sig[16], sf = 1.0f;
    for (int l = 0; l < 16; l++) { if (l > 0 && l < n_levels) sf = sf * g[1]; sig[l] = l < n_levels ? sf * sf : 1.0f; }
    std::vector<Pair> pairs; std::vector<int> owner;
    std::vector<double> ms;
    for (int rep = 0; rep < reps; rep++) {
        std::vector<Kf> K = in;                                        // (the occupancy is written: every run starts from the case)
        const auto t0 = std::chrono::steady_clock::now();
        Kf &c = K[0];
        constants(c, nullptr);
        std::vector<std::vector<int> > M; std::vector<int> nm, S;
        if (n_kf >= 2)
            for (int j = 1; j <= n_kf; j++) {
                constants(K[j], &c);
                if (K[j].gate) continue;
                std::vector<int> m12, m21, out(c.n, -1);
                int n = 0;
                if (c.n && K[j].n) {
                    frame_bf(c.desc, c.n, K[j].desc, K[j].n, (float)th_high, g[0], m12); frame_bf(K[j].desc, K[j].n, c.desc, c.n, (float)th_high, g[0], m21);
                    for (int i = 0; i < c.n; i++) { const int q = m12[i]; if (q >= 0 && m21[q] == i && !c.has[i] && !K[j].has[q]) { out[i] = q; n++; } }
                }
                M.push_back(out); nm.push_back(n); S.push_back(j - 1);
            }
        pairs.clear(); owner.assign(c.n, -1);
        if (M.size() >= 2 && c.n)
            for (size_t a = 0; a + 1 < M.size(); a++) for (size_t b = a + 1; b < M.size(); b++) {
                Pair P; P.mv2 = S[a]; P.mv3 = S[b]; P.kf2 = pairing == 0 ? (int)a : S[a]; P.kf3 = pairing == 0 ? (int)b : S[b];
                Kf &k2 = K[P.kf2 + 1], &k3 = K[P.kf3 + 1];
                if (nm[a] && nm[b])
                    for (int i = 0; i < c.n; i++) {
                        const int i1 = M[a][i], i2 = M[b][i];
                        if (i1 == -1 || i2 == -1 || i1 >= k2.n || i2 >= k3.n) continue;
                        if (c.has[i] || k2.has[i1] || k3.has[i2]) continue;
                        float s[3], e[3];
                        if (!triple(c, k2, k3, i, i1, i2, sig, n_levels, s, e)) continue;
                        c.has[i] = k2.has[i1] = k3.has[i2] = 1; owner[i] = (int)pairs.size();
                        P.c0.push_back(i); P.c1.push_back(i1); P.c2.push_back(i2);
                        for (int q = 0; q < 3; q++) P.x.push_back(s[q]);
                        for (int q = 0; q < 3; q++) P.x.push_back(e[q]);
                    }
                pairs.push_back(P);
            }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%.4f\n", ms[ms.size() / 2]);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int np = (int)pairs.size();
    fwrite(&np, 4, 1, f);
    for (const Pair &P : pairs) {
        const int hd[5] = { P.kf2, P.kf3, P.mv2, P.mv3, (int)P.c0.size() };
        fwrite(hd, 4, 5, f); fwrite(P.c0.data(), 4, P.c0.size(), f); fwrite(P.c1.data(), 4, P.c1.size(), f); fwrite(P.c2.data(), 4, P.c2.size(), f); fwrite(P.x.data(), 4, P.x.size(), f);
    }
    fwrite(owner.data(), 4, owner.size(), f);
    fclose(f);
    return 0;
}
