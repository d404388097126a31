// pnp_host.cpp -- the host path that hvo_stream_pnp_ransac replaces, as a plain single-thread C++ restatement: one PnPsolver per candidate
// (reference src/PnPsolver.cc), every hypothesis, the records and their Refine, under the readings of include/hvo.h.  It includes the text
// the kernels are compiled from (csrc/pnp_core.inc with a group of one lane), so tests/test_pnp.py can tie it to tests/pnp_ref.py bit for
// bit, and tools/pnp_timing.py times it as the comparator.
// build:  g++ -O2 -std=c++14 -ffp-contract=off tools/pnp_host.cpp -o tools/pnp_host
// usage:  pnp_host problem.bin result.bin [repeats]     (prints the median wall time of the solve in ms)
//
// problem.bin: int32 n_kf, min_set, min_inliers, max_iterations, extra_iterations, max_events; uint32 seed; float epsilon, th2, fx, fy, cx, cy;
//              double probability; then per candidate int32 N, n_features; float p3d[3N], p2d[2N], sigma2[N]; int32 feature_index[N].
// result.bin:  per candidate int32 N, min_inliers, max_its, T, no_more; float epsilon; int32 hyp_inliers[T], hyp_sample[T * min_set];
//              float hyp_Tcw[12 T]; uint8 hyp_mask[T * N]; int32 n_records; per record int32 iteration0, refined count; float Tcw[12]; uint8 mask[N].
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <algorithm>
#include <chrono>
#include "../a-low-texture-robust-hybrid-feature-based-visual-odometry_amd/csrc/pnp_core.inc"

struct Params { int n_kf, min_set, min_inliers, max_iterations, extra_iterations, max_events; uint32_t seed; float epsilon, th2, fx, fy, cx, cy; double probability; };
struct Cand { int N, nfeat; std::vector<float> p3d, p2d, sigma2, max_err; std::vector<int> fidx; int min_inl, max_its, T, no_more; float eps; };
struct Rec { int it0, count; float Tcw[12]; std::vector<uint8_t> mask; };
struct Out { std::vector<int> inl, samp; std::vector<float> pose; std::vector<uint8_t> mask; std::vector<Rec> recs; };

static unsigned xs32(unsigned &s) { unsigned x = s; x ^= x << 13; x ^= x >> 17; x ^= x << 5; s = x; return x; }

static void set_ransac(const Params &P, Cand &c)                 // SetRansacParameters (:121-157)
{
    const int N = c.N;
    float eps = P.epsilon;
    int nMin = (int)(N * eps);
    if (nMin < P.min_inliers) nMin = P.min_inliers;
    if (nMin < P.min_set) nMin = P.min_set;
    if (N > 0 && eps < (float)nMin / N) eps = (float)nMin / N;
    int nIt;
    if (nMin == N) nIt = 1;
    else {
        const double v = ceil(log(1 - P.probability) / log(1 - pow((double)eps, 3)));
        nIt = !(v < (double)P.max_iterations) ? P.max_iterations : (v < 1.0 ? 1 : (int)v);
    }
    c.min_inl = nMin; c.eps = eps; c.max_its = std::max(1, std::min(nIt, P.max_iterations));
    c.no_more = N < nMin ? 1 : 0;
    c.T = c.no_more ? 0 : c.max_its + P.extra_iterations;
}

static int check_all(const PnpWs *w, const Cand &c, const Params &P, uint8_t *mask)
{
    const int finite = pnp_pose_finite(w);
    int cnt = 0;
    for (int i = 0; i < c.N; i++) {
        const int in = finite ? pnp_check_one(w, c.p3d.data(), c.p2d.data(), c.max_err.data(), P.fx, P.fy, P.cx, P.cy, i) : 0;
        mask[i] = (uint8_t)in; cnt += in;
    }
    return cnt;
}
static void pose32(const PnpWs *w, float *T) { for (int q = 0; q < 3; q++) { for (int r = 0; r < 3; r++) T[4 * q + r] = (float)w->R[3 * q + r]; T[4 * q + 3] = (float)w->t[q]; } }

static void solve(const Params &P, int j, const Cand &c, Out &o, PnpWs *w, double *tbuf)
{
    const int ms = P.min_set, N = c.N, T = c.T;
    o.inl.assign(T, 0); o.samp.assign((size_t)T * ms, 0); o.pose.assign((size_t)T * 12, 0.f); o.mask.assign((size_t)T * N, 0); o.recs.clear();
    std::vector<int> avail, sel(ms);
    PnpCorr cr; cr.p3d = c.p3d.data(); cr.p2d = c.p2d.data(); cr.fu = P.fx; cr.fv = P.fy; cr.uc = P.cx; cr.vc = P.cy;
    int best = 0;
    for (int it = 0; it < T; it++) {
        unsigned rs = P.seed ^ (0x9E3779B9u * (unsigned)(j * 1024 + it + 1)); if (rs == 0) rs = 0x6D2B79F5u;
        avail.resize(N); for (int i = 0; i < N; i++) avail[i] = i;
        for (int s = 0; s < ms; s++) { const int r = (int)(xs32(rs) % (unsigned)avail.size()); sel[s] = avail[r]; avail[r] = avail.back(); avail.pop_back(); }
        cr.sel = sel.data(); cr.n = ms;
        pnp_epnp<1>(cr, w, tbuf, 0);
        o.inl[it] = check_all(w, c, P, &o.mask[(size_t)it * N]);
        pose32(w, &o.pose[(size_t)it * 12]);
        for (int s = 0; s < ms; s++) o.samp[(size_t)it * ms + s] = sel[s];
        if (o.inl[it] >= c.min_inl && o.inl[it] > best) {          // a record: Refine (:260-305)
            best = o.inl[it];
            std::vector<int> idx;
            for (int i = 0; i < N; i++) if (o.mask[(size_t)it * N + i]) idx.push_back(i);
            cr.sel = idx.data(); cr.n = (int)idx.size();
            pnp_epnp<1>(cr, w, tbuf, 0);
            Rec r; r.it0 = it; r.mask.resize(N);
            r.count = check_all(w, c, P, r.mask.data());
            pose32(w, r.Tcw);
            o.recs.push_back(r);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: pnp_host problem.bin result.bin [repeats]\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    Params P;
    int32_t hi[6]; uint32_t seed; float hf[6]; double pr;
    if (fread(hi, 4, 6, f) != 6 || fread(&seed, 4, 1, f) != 1 || fread(hf, 4, 6, f) != 6 || fread(&pr, 8, 1, f) != 1) return 1;
    P.n_kf = hi[0]; P.min_set = hi[1]; P.min_inliers = hi[2]; P.max_iterations = hi[3]; P.extra_iterations = hi[4]; P.max_events = hi[5]; P.seed = seed;
    P.epsilon = hf[0]; P.th2 = hf[1]; P.fx = hf[2]; P.fy = hf[3]; P.cx = hf[4]; P.cy = hf[5]; P.probability = pr;
    if (P.n_kf < 1 || P.n_kf > 256 || P.min_set < 4 || P.min_set > 64) return 1;
    std::vector<Cand> cand(P.n_kf);
    for (auto &c : cand) {
        int32_t nn[2];
        if (fread(nn, 4, 2, f) != 2 || nn[0] < 0 || nn[0] > 4096) return 1;
        c.N = nn[0]; c.nfeat = nn[1];
        c.p3d.resize(3 * c.N); c.p2d.resize(2 * c.N); c.sigma2.resize(c.N); c.fidx.resize(c.N); c.max_err.resize(c.N);
        if (c.N && (fread(c.p3d.data(), 4, 3 * c.N, f) != (size_t)3 * c.N || fread(c.p2d.data(), 4, 2 * c.N, f) != (size_t)2 * c.N ||
                    fread(c.sigma2.data(), 4, c.N, f) != (size_t)c.N || fread(c.fidx.data(), 4, c.N, f) != (size_t)c.N)) return 1;
        for (int i = 0; i < c.N; i++) { volatile float m = c.sigma2[i] * P.th2; c.max_err[i] = m; }
        set_ransac(P, c);
        if (c.T > 1024) return 1;
    }
    fclose(f);
    const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
    std::vector<Out> out(P.n_kf);
    std::vector<double> ms;
    PnpWs *w = new PnpWs; std::vector<double> tbuf(PNP_TREE_BATCH * 256);
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int j = 0; j < P.n_kf; j++) solve(P, j, cand[j], out[j], w, tbuf.data());
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("%.4f\n", ms[ms.size() / 2]);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    for (int j = 0; j < P.n_kf; j++) {
        const Cand &c = cand[j]; const Out &o = out[j];
        const int32_t h[5] = { c.N, c.min_inl, c.max_its, c.T, c.no_more };
        fwrite(h, 4, 5, f); fwrite(&c.eps, 4, 1, f);
        fwrite(o.inl.data(), 4, o.inl.size(), f); fwrite(o.samp.data(), 4, o.samp.size(), f); fwrite(o.pose.data(), 4, o.pose.size(), f);
        fwrite(o.mask.data(), 1, o.mask.size(), f);
        const int32_t nr = (int32_t)o.recs.size(); fwrite(&nr, 4, 1, f);
        for (const Rec &r : o.recs) { const int32_t q[2] = { r.it0, r.count }; fwrite(q, 4, 2, f); fwrite(r.Tcw, 4, 12, f); fwrite(r.mask.data(), 1, r.mask.size(), f); }
    }
    fclose(f);
    delete w;
    return 0;
}
