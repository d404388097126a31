// fuse_line_neighbors.cpp -- the line half of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:1644-1677) on a toy map
// through the C++ mirror (include/hvo.hpp):
//   1. lineMatcher.Fuse(pKFi, vpMapLineMatches) for every target key frame (:1644-1651): ONE device call for all targets, the current key
//      frame's map lines uploaded once;
//   2. lineMatcher.Fuse(mpCurrentKeyFrame, vpLineFuseCandidates) (:1655-1677): the candidates are slots of a resident line map.
// What stays on the host is what the reference does with pointers: hvo::LSDmatcher::walkFused merges the fused entries and the entries at
// which the reference's `return false` (a negative depth) would fire, repeats the skip test `isBad() || IsInKeyFrame(pKF)` per entry (an
// earlier Replace of the same walk can have made it true) and calls back for Replace against AddObservation + AddMapLine.  The whole
// run is made twice, with stop_on_behind true (the text as written: a key frame's walk ends at the first entry behind the camera) and false.
// The toy map needs no image: 12 world segments at 2 m in front of three key frames that stand 2 px apart; the current key frame (0) holds a
// map line on each of them and one map line that lies behind all cameras; the targets (1, 2) hold map lines of their own on some.
//
// build:  g++ -std=c++14 -Iinclude examples/fuse_line_neighbors.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o fuse_line_neighbors
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "hvo.hpp"

struct MapLine {
    double pos[6], nrm[3]; float maxd, mind; uint8_t desc[32];
    bool bad = false; std::vector<std::pair<int, int> > obs;       // (key frame, key line); key frame -1: one outside this toy map
    int Observations() const { return (int)obs.size(); }
    bool IsInKeyFrame(int kf) const { for (const auto &o : obs) if (o.first == kf) return true; return false; }
};
struct KeyFrame { std::vector<hvo_keyline> kl; std::vector<uint8_t> desc; float Tcw[12]; std::vector<int> ml; };      // ml: map line per key line, -1 = NULL
static std::vector<MapLine> lines; static std::vector<KeyFrame> kfs;
static const int W = 12, BEHIND = 12;                              // world segments; the map line behind the cameras

static void world(int k, double P[6])                              // segment k: pixels (80 + 40 k, 100 + 20 k) .. (+48, +8 (k % 3)) of key frame 0 at z = 2
{
    const double ua = 80 + 40 * k, va = 100 + 20 * k, ub = ua + 48, vb = va + 8 * (k % 3);
    P[0] = 0; P[1] = (ua - 320) / 256 - 0.5; P[2] = (va - 240) / 256 + 0.25; P[3] = 0; P[4] = (ub - 320) / 256 - 0.5; P[5] = (vb - 240) / 256 + 0.25;
}
static void descriptor(int k, int flipped, uint8_t d[32])         // segment k's pattern with its first `flipped` (< 8) bits flipped
{
    for (int b = 0; b < 32; b++) d[b] = (uint8_t)(7 * b + 3 + 13 * k);
    d[0] ^= (uint8_t)(0xFF << (8 - flipped));
}
static int add_line(int k, int flipped, int kf, int idx, int outside)
{
    MapLine m; memset(m.pos, 0, sizeof(m.pos));
    if (k == BEHIND) { const double P[6] = { -4, -0.5, 0.25, -4, -0.25, 0.25 }; memcpy(m.pos, P, sizeof(P)); memset(m.desc, 0, 32); }
    else { world(k, m.pos); descriptor(k, flipped, m.desc); }
    m.nrm[0] = 1; m.nrm[1] = m.nrm[2] = 0; m.maxd = 3.0f; m.mind = 1.0f;
    m.obs.push_back(std::make_pair(kf, idx));
    for (int q = 0; q < outside; q++) m.obs.push_back(std::make_pair(-1, q));
    lines.push_back(m); kfs[kf].ml[idx] = (int)lines.size() - 1;
    return (int)lines.size() - 1;
}
static void build_map()
{
    lines.clear(); kfs.assign(3, KeyFrame());
    for (int j = 0; j < 3; j++) {
        KeyFrame &K = kfs[j];
        const float T[12] = { 0, 1, 0, 0.5f + j / 128.0f, 0, 0, 1, -0.25f, 1, 0, 0, 2 };      // Xc = (Yw + 0.5 + 2 px, Zw - 0.25, Xw + 2)
        memcpy(K.Tcw, T, sizeof(T));
        const int n = j == 0 ? W + 1 : W;
        K.kl.assign(n, hvo_keyline()); K.desc.assign((size_t)n * 32, 0); K.ml.assign(n, -1);
        for (int i = 0; i < n; i++) {
            // key frame 0 shows the segments in order with the line behind at index 5; key frame j shows segment k at (k + 3 j) % 12
            const int k = j == 0 ? (i < 5 ? i : i == 5 ? BEHIND : i - 1) : (i + W - 3 * j) % W;
            hvo_keyline &l = K.kl[i]; l.class_id = i;
            if (k == BEHIND) { l.sx = 10; l.sy = 10; l.ex = 30; l.ey = 10; }
            else { l.sx = 80 + 40 * k + 2 * j; l.sy = 100 + 20 * k; l.ex = l.sx + 48; l.ey = l.sy + 8 * (k % 3); descriptor(k, (k + j) % 4, &K.desc[(size_t)i * 32]); }
            l.pt_x = (l.sx + l.ex) / 2; l.pt_y = (l.sy + l.ey) / 2; l.sox = l.sx; l.soy = l.sy; l.eox = l.ex; l.eoy = l.ey;
        }
    }
    for (int i = 0; i < W + 1; i++) { const int k = i < 5 ? i : i == 5 ? BEHIND : i - 1; add_line(k, 0, 0, i, (k != BEHIND && k % 4 == 0) ? 1 : 0); }      // map lines 0 .. 12
    for (int k = 0; k < W; k += 3) add_line(k, 1, 1, (k + 3) % W, (k % 6 == 0) ? 2 : 0);                                                           // 13 .. 16: key frame 1's own
    for (int k = 1; k < W; k += 4) add_line(k, 2, 2, (k + 6) % W, k == 5 ? 1 : 0);                                                                 // 17 .. 19: key frame 2's own
}

static void Replace(int from, int to)                              // MapLine::Replace (src/MapLine.cpp:274-312)
{
    if (from == to) return;
    std::vector<std::pair<int, int> > obs; obs.swap(lines[from].obs);
    lines[from].bad = true;
    for (const auto &o : obs) {
        if (o.first < 0) { lines[to].obs.push_back(o); continue; }
        if (!lines[to].IsInKeyFrame(o.first)) { kfs[o.first].ml[o.second] = to; lines[to].obs.push_back(o); }
        else kfs[o.first].ml[o.second] = -1;
    }
}

// LSDmatcher.cpp:1340-1341 and :1411-1431 for key frame kf over the list the device returned
static void walk(const char *what, int kf, const std::vector<int> &entries, const hvo::LineFuseMatches &r, bool stop)
{
    std::vector<std::pair<int, int> > seen;
    const hvo::LineFuseWalk w = hvo::LSDmatcher::walkFused(r, stop,
        [&](int e) { const int pML = entries[e]; return pML < 0 || lines[pML].bad || lines[pML].IsInKeyFrame(kf); },
        [&](int e, int bestIdx) {
            const int pML = entries[e], pMLinKF = kfs[kf].ml[bestIdx];
            seen.push_back(std::make_pair(e, bestIdx));
            if (pMLinKF >= 0) {
                if (lines[pMLinKF].bad) return false;
                if (lines[pMLinKF].Observations() > lines[pML].Observations()) Replace(pML, pMLinKF); else Replace(pMLinKF, pML);
                return true;
            }
            lines[pML].obs.push_back(std::make_pair(kf, bestIdx)); kfs[kf].ml[bestIdx] = pML;
            return false;
        });
    printf("%s kf %d: fused %d stopped_at %d replaced %d |", what, kf, w.n_fused, w.stopped_at, w.replaced ? 1 : 0);
    for (const auto &s : seen) printf(" %d>%d", s.first, s.second);
    printf("\n");
}

static hvo_lf_keyframe describe(const KeyFrame &K, const std::vector<uint8_t> &skip)
{
    hvo_lf_keyframe k = hvo_lf_keyframe();
    k.n = (int)K.kl.size(); k.kl = K.kl.data(); k.desc_rows = K.desc.data(); k.n_desc_rows = k.n;      // the intended reading: mLineDescriptors
    memcpy(k.Tcw, K.Tcw, sizeof(k.Tcw));
    k.bounds[0] = 0; k.bounds[1] = 640; k.bounds[2] = 0; k.bounds[3] = 480; k.fx = k.fy = 512; k.cx = 320; k.cy = 240;
    k.skip = skip.data();
    return k;
}

static void run(hvo::LSDmatcher &matcher, hvo::LineMap &lmap, bool stop)
{
    build_map();
    printf("stop_on_behind %d\n", stop ? 1 : 0);
    // ---- 1. the current key frame's map lines into the targets (:1644-1651) ----
    const std::vector<int> cur = kfs[0].ml;                          // vpMapLineMatches
    const int n = (int)cur.size();
    std::vector<double> pos((size_t)n * 6), nrm((size_t)n * 3); std::vector<float> maxd(n), mind(n); std::vector<uint8_t> desc((size_t)n * 32);
    for (int i = 0; i < n; i++) {
        const MapLine &m = lines[cur[i]];
        memcpy(&pos[6 * (size_t)i], m.pos, sizeof(m.pos)); memcpy(&nrm[3 * (size_t)i], m.nrm, sizeof(m.nrm)); maxd[i] = m.maxd; mind[i] = m.mind; memcpy(&desc[32 * (size_t)i], m.desc, 32);
    }
    hvo_lf_map side = hvo_lf_map();
    side.n = n; side.pos = pos.data(); side.normal = nrm.data(); side.max_distance = maxd.data(); side.min_distance = mind.data(); side.desc = desc.data();
    std::vector<std::vector<uint8_t> > skip(2, std::vector<uint8_t>(n, 0));
    std::vector<hvo_lf_keyframe> targets;
    for (int j = 1; j <= 2; j++) {
        for (int i = 0; i < n; i++) skip[j - 1][i] = cur[i] < 0 || lines[cur[i]].bad || lines[cur[i]].IsInKeyFrame(j);
        targets.push_back(describe(kfs[j], skip[j - 1]));
    }
    std::vector<hvo::LineFuseMatches> res;
    matcher.Fuse(side, 2, targets.data(), res);
    for (int j = 1; j <= 2; j++) walk("call 1", j, cur, res[j - 1], stop);
    // ---- 2. the targets' map lines into the current key frame (:1655-1677), as slots of the resident line map ----
    std::vector<int> cand; std::vector<uint8_t> marked(lines.size(), 0);
    for (int j = 1; j <= 2; j++) for (int pML : kfs[j].ml) {
        if (pML < 0 || lines[pML].bad || marked[pML]) continue;      // mnFuseCandidateForKF
        marked[pML] = 1; cand.push_back(pML);
    }
    const int N = (int)lines.size();
    std::vector<double> mp((size_t)N * 6), mw((size_t)N * 3), mn((size_t)N * 3); std::vector<float> mx(N), mi(N); std::vector<uint8_t> md((size_t)N * 32), bad(N);
    for (int i = 0; i < N; i++) {
        const MapLine &m = lines[i];
        memcpy(&mp[6 * (size_t)i], m.pos, sizeof(m.pos)); memcpy(&mn[3 * (size_t)i], m.nrm, sizeof(m.nrm));
        for (int q = 0; q < 3; q++) mw[3 * (size_t)i + q] = m.pos[3 + q] - m.pos[q];
        mx[i] = m.maxd; mi[i] = m.mind; memcpy(&md[32 * (size_t)i], m.desc, 32); bad[i] = m.bad ? 1 : 0;
    }
    lmap.setMany(0, N, mp.data(), mw.data(), mn.data(), mx.data(), mi.data(), md.data(), nullptr, bad.data());
    std::vector<uint8_t> skip0(cand.size() ? cand.size() : 1, 0);
    for (size_t i = 0; i < cand.size(); i++) skip0[i] = lines[cand[i]].IsInKeyFrame(0);
    const hvo_lf_keyframe current = describe(kfs[0], skip0);
    matcher.Fuse(lmap.get(), (int)cand.size(), cand.data(), 1, &current, res);
    walk("call 2", 0, cand, res[0], stop);
    printf("bad:"); for (int i = 0; i < N; i++) if (lines[i].bad) printf(" %d", i);
    printf(" | observations:"); for (int i = 0; i < N; i++) printf(" %d", lines[i].Observations());
    printf("\n");
}

int main()
{
    try {
        hvo_params hp; hvo_default_params(&hp); hp.max_batch = 1;
        hvo::Context ctx(hp);
        hvo::LSDmatcher matcher(ctx.get());
        hvo::LineMap lmap(hp.device, 32);
        run(matcher, lmap, true);
        run(matcher, lmap, false);
        return 0;
    } catch (const hvo::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
}
