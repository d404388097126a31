// kf_db_host.cpp -- the host path that hvo_stream_keyframe_db_query replaces, as a plain single-thread C++ restatement written for this
// project (tools/kf_db_timing.py times it): the reference's shape -- an inverted file of std::list<KeyFrame *> per word, key frames that
// carry their bag of words as a std::map and the query / words / score fields, the score as a merge of two maps with lower_bound -- for
// add, erase, clear, DetectRelocalizationCandidates and DetectLoopCandidates.  It reads one binary script (the layout
// kf_db_timing.write_case writes), plays it, prints every query's candidate list ("candidates <n> <slot> ...") and, with reps > 1, the
// median time of `reps` repetitions of the LAST query ("query_ms <ms>").
//
// build:  g++ -O2 -std=c++14 tools/kf_db_host.cpp -o tools/kf_db_host
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <set>
#include <vector>

typedef std::map<int, double> BowVector;
struct KeyFrame {
    int slot = 0; BowVector bow; std::vector<int> neigh;
    long relocQuery = 0, loopQuery = 0; int relocWords = 0, loopWords = 0; float relocScore = 0.f, loopScore = 0.f;
};

static double score(int scoring, const BowVector &v1, const BowVector &v2)
{
    BowVector::const_iterator a = v1.begin(), b = v2.begin();
    double s = 0;
    while (a != v1.end() && b != v2.end()) {
        const double vi = a->second, wi = b->second;
        if (a->first == b->first) {
            switch (scoring) {
            case 0: s += fabs(vi - wi) - fabs(vi) - fabs(wi); break;
            case 2: if (vi + wi != 0.0) s += vi * wi / (vi + wi); break;
            case 4: s += sqrt(vi * wi); break;
            default: s += vi * wi; break;
            }
            ++a; ++b;
        } else if (a->first < b->first) a = v1.lower_bound(b->first);
        else b = v2.lower_bound(a->first);
    }
    if (scoring == 0) s = -s / 2.0;
    else if (scoring == 1) s = s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s);
    else if (scoring == 2) s = 2. * s;
    return s;
}

struct Database {
    int scoring = 0; long nextId = 0;
    std::vector<std::list<KeyFrame *>> inverted; std::map<int, KeyFrame *> kf;
    void add(int slot, const BowVector &bow) { KeyFrame *k = new KeyFrame(); k->slot = slot; k->bow = bow; kf[slot] = k; for (const auto &e : bow) inverted[e.first].push_back(k); }
    void erase(int slot)
    {
        auto it = kf.find(slot);
        if (it == kf.end()) return;
        KeyFrame *k = it->second;
        for (const auto &e : k->bow) { std::list<KeyFrame *> &l = inverted[e.first]; for (auto li = l.begin(); li != l.end(); ++li) if (*li == k) { l.erase(li); break; } }
        kf.erase(it); delete k;
    }
    void clear() { for (auto &l : inverted) l.clear(); for (auto &e : kf) delete e.second; kf.clear(); }
    std::vector<int> detect(const BowVector &q, int mode, float minScore, const std::set<int> &connected)
    {
        const long id = ++nextId;
        std::list<KeyFrame *> sharing;
        for (const auto &e : q)
            for (KeyFrame *k : inverted[e.first]) {
                if (mode == 0) { if (k->relocQuery != id) { k->relocWords = 0; k->relocQuery = id; sharing.push_back(k); } k->relocWords++; }
                else { if (k->loopQuery != id) { k->loopWords = 0; if (!connected.count(k->slot)) { k->loopQuery = id; sharing.push_back(k); } } k->loopWords++; }
            }
        if (sharing.empty()) return std::vector<int>();
        int maxCommonWords = 0;
        for (KeyFrame *k : sharing) maxCommonWords = std::max(maxCommonWords, mode == 0 ? k->relocWords : k->loopWords);
        const int minCommonWords = maxCommonWords * 0.8f;
        std::list<std::pair<float, KeyFrame *>> scoreAndMatch;
        for (KeyFrame *k : sharing) {
            if ((mode == 0 ? k->relocWords : k->loopWords) <= minCommonWords) continue;
            const float si = score(scoring, q, k->bow);
            if (mode == 0) { k->relocScore = si; scoreAndMatch.push_back(std::make_pair(si, k)); }
            else { k->loopScore = si; if (si >= minScore) scoreAndMatch.push_back(std::make_pair(si, k)); }
        }
        if (scoreAndMatch.empty()) return std::vector<int>();
        std::list<std::pair<float, KeyFrame *>> accAndMatch;
        float bestAccScore = mode == 0 ? 0.f : minScore;
        for (const auto &e : scoreAndMatch) {
            float bestScore = e.first, accScore = e.first; KeyFrame *best = e.second;
            for (int nb : e.second->neigh) {
                auto it = kf.find(nb);
                if (it == kf.end()) continue;
                KeyFrame *k2 = it->second;
                if (mode == 0 ? k2->relocQuery != id : !(k2->loopQuery == id && k2->loopWords > minCommonWords)) continue;
                const float s2 = mode == 0 ? k2->relocScore : k2->loopScore;
                accScore += s2;
                if (s2 > bestScore) { best = k2; bestScore = s2; }
            }
            accAndMatch.push_back(std::make_pair(accScore, best));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        const float minScoreToRetain = 0.75f * bestAccScore;
        std::set<KeyFrame *> already; std::vector<int> out;
        for (const auto &e : accAndMatch)
            if (e.first > minScoreToRetain && !already.count(e.second)) { out.push_back(e.second->slot); already.insert(e.second); }
        return out;
    }
};

template <class T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s script.bin [reps]\n", argv[0]); return 2; }
    const int reps = argc > 2 ? atoi(argv[2]) : 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    if (!rd(f, head, 3)) return 3;
    Database db; db.scoring = head[1]; db.inverted.resize((size_t)head[0]);
    BowVector lastq; int lastmode = 0; float lastmin = 0.f; std::set<int> lastconn; bool any = false;
    for (int op = 0; op < head[2]; op++) {
        int32_t h[2];
        if (!rd(f, h, 2)) return 3;
        const int type = h[0];
        if (type == 0 || type == 4) {                            // add: slot; query: mode, then min_score, the connected slots; both: the bag
            float ms = 0.f; std::set<int> conn;
            if (type == 4) {
                int32_t nc; if (!rd(f, &ms, 1) || !rd(f, &nc, 1)) return 3;
                std::vector<int32_t> c((size_t)nc); if (!rd(f, c.data(), c.size())) return 3;
                conn.insert(c.begin(), c.end());
            }
            int32_t n; if (!rd(f, &n, 1)) return 3;
            std::vector<int32_t> w((size_t)n); std::vector<double> v((size_t)n);
            if (!rd(f, w.data(), w.size()) || !rd(f, v.data(), v.size())) return 3;
            BowVector bow; for (int i = 0; i < n; i++) bow[w[i]] = v[i];
            if (type == 0) db.add(h[1], bow);
            else {
                const std::vector<int> c = db.detect(bow, h[1], ms, conn);
                printf("candidates %d", (int)c.size()); for (int s : c) printf(" %d", s); printf("\n");
                lastq = bow; lastmode = h[1]; lastmin = ms; lastconn = conn; any = true;
            }
        } else if (type == 1) db.erase(h[1]);
        else if (type == 2) db.clear();
        else if (type == 3) {
            int32_t n; if (!rd(f, &n, 1)) return 3;
            std::vector<int32_t> c((size_t)n); if (!rd(f, c.data(), c.size())) return 3;
            auto it = db.kf.find(h[1]); if (it != db.kf.end()) it->second->neigh.assign(c.begin(), c.end());
        } else return 4;
    }
    fclose(f);
    if (reps > 1 && any) {
        std::vector<double> t;
        size_t sink = 0;
        for (int r = 0; r < reps; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            sink += db.detect(lastq, lastmode, lastmin, lastconn).size();
            t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(t.begin(), t.end());
        printf("query_ms %.6f %zu\n", t[t.size() / 2], sink);
    }
    return 0;
}
