// bow_host.cpp -- the host path that hvo_stream_compute_bow + hvo_stream_search_by_bow replace, as a plain single-thread C++ restatement
// written for this project (tools/bow_timing.py times it): the vocabulary as nodes with child vectors, transform() into a std::map
// BowVector and a std::map FeatureVector, and SearchByBoW over the two FeatureVectors with the sequential claims.  It reads one binary
// file (the layout bow_timing.py writes) and prints: transform ms, search ms (medians of `reps` runs), words, matches, and a hash of the
// match vector and of the BowVector.
//
// build:  g++ -O2 -std=c++14 tools/bow_host.cpp -o tools/bow_host
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

struct Node { std::vector<int> children; uint64_t d[4]; double weight = 0; int word = -1; bool leaf = false; };
static inline int ham(const uint64_t *a, const uint64_t *b)
{
    return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) + __builtin_popcountll(a[3] ^ b[3]);
}
typedef std::map<int, double> BowVector;
typedef std::map<int, std::vector<unsigned>> FeatureVector;

static void transform(const std::vector<Node> &nodes, int L, bool tf, int norm, const uint64_t *desc, int n, int levelsup, BowVector &v, FeatureVector &fv)
{
    v.clear(); fv.clear();
    const int nid_level = L - levelsup;
    for (int i = 0; i < n; i++) {
        int fin = 0, level = 0, nid = 0;
        do {
            level++;
            const std::vector<int> &ch = nodes[fin].children;
            fin = ch[0]; int best = ham(desc + 4 * i, nodes[fin].d);
            for (size_t c = 1; c < ch.size(); c++) { const int d = ham(desc + 4 * i, nodes[ch[c]].d); if (d < best) { best = d; fin = ch[c]; } }
            if (level == nid_level) nid = fin;
        } while (!nodes[fin].leaf);
        if (nid_level > 0 && level < nid_level) nid = fin;
        const double w = nodes[fin].weight;
        if (w > 0) {
            BowVector::iterator it = v.lower_bound(nodes[fin].word);
            if (it != v.end() && it->first == nodes[fin].word) { if (tf) it->second += w; } else v.insert(it, std::make_pair(nodes[fin].word, w));
            fv[nid].push_back((unsigned)i);
        }
    }
    if (tf && !v.empty() && !norm) { const double nd = (double)v.size(); for (auto &e : v) e.second /= nd; }
    if (norm) {
        double s = 0;
        if (norm == 1) for (auto &e : v) s += std::fabs(e.second); else { for (auto &e : v) s += e.second * e.second; s = std::sqrt(s); }
        if (s > 0) for (auto &e : v) e.second /= s;
    }
}

static int search(const FeatureVector &fk, const FeatureVector &ff, const uint64_t *dk, const uint64_t *df, const uint8_t *has, const float *ak, const float *af,
                  int nF, float nnratio, int th_low, std::vector<int> &match)
{
    match.assign(nF, -1);
    std::vector<int> hist[30]; int nm = 0;
    FeatureVector::const_iterator K = fk.begin(), F = ff.begin();
    while (K != fk.end() && F != ff.end()) {
        if (K->first == F->first) {
            for (unsigned ik : K->second) {
                if (!has[ik]) continue;
                int b1 = 256, b2 = 256, bi = -1;
                for (unsigned i : F->second) {
                    if (match[i] >= 0) continue;
                    const int d = ham(dk + 4 * ik, df + 4 * i);
                    if (d < b1) { b2 = b1; b1 = d; bi = (int)i; } else if (d < b2) b2 = d;
                }
                if (b1 <= th_low && bi >= 0 && (float)b1 < nnratio * (float)b2) {
                    match[bi] = (int)ik; nm++;
                    float rot = ak[ik] - af[bi]; if (rot < 0.0f) rot += 360.0f;
                    int bin = (int)std::round(rot * (1.0f / 30)); if (bin == 30) bin = 0;
                    if (bin >= 0 && bin < 30) hist[bin].push_back(bi);
                }
            }
            ++K; ++F;
        } else if (K->first < F->first) K = fk.lower_bound(F->first); else F = ff.lower_bound(K->first);
    }
    int m1 = 0, m2 = 0, m3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int b = 0; b < 30; b++) {
        const int s = (int)hist[b].size();
        if (s > m1) { m3 = m2; m2 = m1; m1 = s; i3 = i2; i2 = i1; i1 = b; } else if (s > m2) { m3 = m2; m2 = s; i3 = i2; i2 = b; } else if (s > m3) { m3 = s; i3 = b; }
    }
    if ((float)m2 < 0.1f * (float)m1) { i2 = -1; i3 = -1; } else if ((float)m3 < 0.1f * (float)m1) i3 = -1;
    for (int b = 0; b < 30; b++) if (b != i1 && b != i2 && b != i3) for (int i : hist[b]) { match[i] = -1; nm--; }
    return nm;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t h[9];
    if (fread(h, 4, 9, f) != 9) return 3;
    const int k = h[0], L = h[1], scoring = h[2], weighting = h[3], rows = h[4], levelsup = h[5], nF = h[6], nK = h[7], reps = h[8];
    (void)k;
    std::vector<int32_t> parent(rows); std::vector<uint8_t> leaf(rows), desc((size_t)rows * 32); std::vector<double> weight(rows);
    std::vector<uint64_t> df((size_t)nF * 4), dk((size_t)nK * 4); std::vector<uint8_t> has(nK); std::vector<float> ak(nK), af(nF);
    bool ok = fread(parent.data(), 4, rows, f) == (size_t)rows && fread(leaf.data(), 1, rows, f) == (size_t)rows && fread(desc.data(), 32, rows, f) == (size_t)rows &&
              fread(weight.data(), 8, rows, f) == (size_t)rows && fread(df.data(), 32, nF, f) == (size_t)nF && fread(dk.data(), 32, nK, f) == (size_t)nK &&
              fread(has.data(), 1, nK, f) == (size_t)nK && fread(ak.data(), 4, nK, f) == (size_t)nK && fread(af.data(), 4, nF, f) == (size_t)nF;
    fclose(f);
    if (!ok) return 3;
    std::vector<Node> nodes(rows + 1); int nw = 0;
    for (int i = 0; i < rows; i++) {
        Node &n = nodes[i + 1];
        nodes[parent[i]].children.push_back(i + 1);
        for (int q = 0; q < 4; q++) { uint64_t v = 0; for (int b = 0; b < 8; b++) v |= (uint64_t)desc[(size_t)i * 32 + q * 8 + b] << (8 * b); n.d[q] = v; }
        n.weight = weight[i]; n.leaf = leaf[i] != 0; if (n.leaf) n.word = nw++;
    }
    const bool tf = weighting == 0 || weighting == 1; const int norm = scoring == 5 ? 0 : (scoring == 1 ? 2 : 1);
    BowVector vF, vK; FeatureVector fF, fK; std::vector<int> match; int nm = 0;
    transform(nodes, L, tf, norm, dk.data(), nK, levelsup, vK, fK);
    std::vector<double> tt, ts;
    for (int r = 0; r < reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        transform(nodes, L, tf, norm, df.data(), nF, levelsup, vF, fF);
        auto t1 = std::chrono::steady_clock::now();
        nm = search(fK, fF, dk.data(), df.data(), has.data(), ak.data(), af.data(), nF, 0.7f, 50, match);
        auto t2 = std::chrono::steady_clock::now();
        tt.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); ts.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    std::sort(tt.begin(), tt.end()); std::sort(ts.begin(), ts.end());
    // FNV-1a of the match vector and of the BowVector (words, then the values' bits): tests/test_bow.py compares them with tests/bow_ref.py
    uint64_t hm = 0xcbf29ce484222325ull, hv = hm;
    auto eat = [](uint64_t &h, const void *p, size_t n) { for (size_t i = 0; i < n; i++) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull; };
    for (int i = 0; i < nF; i++) { const int32_t v = match[i]; eat(hm, &v, 4); }
    for (auto &e : vF) { const int32_t w = e.first; eat(hv, &w, 4); }
    for (auto &e : vF) eat(hv, &e.second, 8);
    printf("%.4f %.4f %d %d %016llx %016llx\n", tt[tt.size() / 2], ts[ts.size() / 2], (int)vF.size(), nm, (unsigned long long)hm, (unsigned long long)hv);
    return 0;
}
