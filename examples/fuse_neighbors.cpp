// fuse_neighbors.cpp -- both halves of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:1567-1696) on a toy map through the
// C++ mirror (include/hvo.hpp):
//   1. matcher.Fuse(pKFi, vpMapPointMatches) for every target key frame (LocalMapping.cc:1596-1603): ONE device call for all targets, the
//      current key frame's map points uploaded once;
//   2. matcher.Fuse(mpCurrentKeyFrame, vpFuseCandidates) (:1605-1627): the current key frame is the frame the stream just tracked, still
//      resident; the candidates are slots of a resident point map.
// What stays on the host is what the reference does with pointers: choosing the targets, the walk over the fused entries with the skip test
// `isBad() || IsInKeyFrame(pKF)` repeated per entry (an earlier Replace of the same walk can have made it true), Replace against
// AddObservation + AddMapPoint by observation count, and after both halves ComputeDistinctiveDescriptors, UpdateNormalAndDepth and
// UpdateConnections (not shown: they read nothing the searches write).
// The toy map: the current key frame is one extracted frame (camera = world); its map points are every second feature with depth.  Two
// neighbours see the same points from 3 and 6 cm aside; every third of their features holds a map point of its own.
// Reads one raw 640x480 gray (u8) + depth (u16) pair.
//
// build:  g++ -std=c++14 -Iinclude examples/fuse_neighbors.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o fuse_neighbors
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "hvo.hpp"

struct MapPoint {
    float pos[3], nrm[3], maxd, mind; uint8_t desc[32];
    bool bad = false; std::vector<std::pair<int, int> > obs;       // (key frame, feature)
    int Observations() const { return (int)obs.size(); }
    bool IsInKeyFrame(int kf) const { for (const auto &o : obs) if (o.first == kf) return true; return false; }
};
struct KeyFrame {
    std::vector<hvo_keypoint> kpu; std::vector<float> ur; std::vector<uint8_t> desc; float Tcw[12]; std::vector<int> mp;      // mp: map point per feature, -1 = NULL
};
static std::vector<MapPoint> points; static std::vector<KeyFrame> kfs;

static void Replace(int from, int to)                              // MapPoint::Replace (src/MapPoint.cc:183-226)
{
    if (from == to) return;
    std::vector<std::pair<int, int> > obs; obs.swap(points[from].obs);
    points[from].bad = true;
    for (const auto &o : obs) {
        if (o.first < 0) { points[to].obs.push_back(o); continue; }      // an older key frame outside this toy map
        if (!points[to].IsInKeyFrame(o.first)) { kfs[o.first].mp[o.second] = to; points[to].obs.push_back(o); }
        else kfs[o.first].mp[o.second] = -1;
    }
}

// ORBmatcher.cc:967-990 over the list the device returned, in entry order
static void walk(int kf, const std::vector<int> &entries, const hvo::FuseMatches &r, int &nReplaced, int &nAdded, int &nSkipped)
{
    nReplaced = nAdded = nSkipped = 0;
    for (int k = 0; k < r.n_fused; k++) {
        const int pMP = entries[r.fused_entry[k]], bestIdx = r.fused_idx[k];
        if (pMP < 0 || points[pMP].bad || points[pMP].IsInKeyFrame(kf)) { nSkipped++; continue; }    // the skip test again: it may have turned true during this walk
        const int pMPinKF = kfs[kf].mp[bestIdx];
        if (pMPinKF >= 0) {
            if (!points[pMPinKF].bad) {
                if (points[pMPinKF].Observations() > points[pMP].Observations()) Replace(pMP, pMPinKF); else Replace(pMPinKF, pMP);
                nReplaced++;
            }
        } else { points[pMP].obs.push_back(std::make_pair(kf, bestIdx)); kfs[kf].mp[bestIdx] = pMP; nAdded++; }
    }
}

static bool read_raw(const char *path, void *dst, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s frame.u8 frame.u16\n", argv[0]); return 2; }
    const int W = 640, H = 480;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    if (!read_raw(argv[1], gray.data(), gray.size()) || !read_raw(argv[2], depth.data(), depth.size() * 2)) return 3;
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f; sp.stages = HVO_STAGE_ORB;
        hvo::FrameStream fs(p, sp);
        hvo::Context ctx(p);
        const hvo_camera cam = { p.fx, p.fy, p.cx, p.cy, sp.bf, sp.bf / p.fx };
        const float bounds[4] = { 0.f, (float)W, 0.f, (float)H };
        hvo::ORBmatcher matcher(ctx.get());
        const int kp_cap = fs.kpCap();
        kfs.resize(3);
        KeyFrame &cur = kfs[0];
        std::vector<hvo_keypoint> kp(kp_cap); std::vector<float> zd(kp_cap);
        cur.kpu.resize(kp_cap); cur.ur.resize(kp_cap); cur.desc.resize((size_t)kp_cap * 32);
        const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
        hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.desc = cur.desc.data(); fo.kp_cap = kp_cap;
        fs.collect(t, fo, cur.kpu.data(), cur.ur.data(), zd.data());
        const int N = fo.n_kp;
        cur.kpu.resize(N); cur.ur.resize(N); cur.desc.resize((size_t)N * 32); cur.mp.assign(N, -1);
        const float I[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        memcpy(cur.Tcw, I, sizeof(I));
        float sf[16]; sf[0] = 1.f;
        for (int l = 1; l < 16; l++) sf[l] = sf[l - 1] * p.orb_scale_factor;
        // the current key frame's map points, and the two neighbours with theirs
        std::vector<float> X(3 * (size_t)(N > 0 ? N : 1), 0.f);
        for (int i = 0, k = 0; i < N; i++) {
            if (!(zd[i] > 0)) continue;
            const float z = zd[i];
            float *x = &X[3 * (size_t)i];
            x[0] = (cur.kpu[i].x - p.cx) / p.fx * z; x[1] = (cur.kpu[i].y - p.cy) / p.fy * z; x[2] = z;
            if (k++ % 2) continue;
            MapPoint m; const float d = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            for (int q = 0; q < 3; q++) { m.pos[q] = x[q]; m.nrm[q] = x[q] / d; }
            m.maxd = d * sf[cur.kpu[i].octave]; m.mind = m.maxd / sf[p.orb_nlevels - 1]; memcpy(m.desc, &cur.desc[32 * (size_t)i], 32);
            m.obs.push_back(std::make_pair(0, i)); m.obs.push_back(std::make_pair(-1, 0)); m.obs.push_back(std::make_pair(-2, 0));       // seen by two older key frames too
            cur.mp[i] = (int)points.size(); points.push_back(m);
        }
        const int nCurPoints = (int)points.size();
        for (int j = 1; j <= 2; j++) {
            KeyFrame &K = kfs[j];
            memcpy(K.Tcw, I, sizeof(I)); K.Tcw[3] = 0.03f * j; K.Tcw[7] = -0.02f; K.Tcw[11] = 0.01f;
            for (int i = 0, k = 0; i < N; i++) {
                if (!(zd[i] > 0)) continue;
                const float *x = &X[3 * (size_t)i];
                const float xc = x[0] + K.Tcw[3], yc = x[1] + K.Tcw[7], zc = x[2] + K.Tcw[11];
                const float u = p.fx * xc / zc + p.cx, v = p.fy * yc / zc + p.cy;
                if (!(u > 8 && u < W - 8 && v > 8 && v < H - 8)) continue;
                hvo_keypoint f = cur.kpu[i]; f.x = u + 0.25f * (float)((i % 3) - 1); f.y = v - 0.25f * (float)((i % 5) - 2);
                K.kpu.push_back(f); K.ur.push_back(f.x - sp.bf / zc);
                uint8_t d[32]; memcpy(d, &cur.desc[32 * (size_t)i], 32);
                for (int b = 0; b < 6; b++) d[(i + 5 * b) % 32] ^= (uint8_t)(1u << ((i + b) % 8));     // six bits of noise
                K.desc.insert(K.desc.end(), d, d + 32);
                int held = -1;
                if (k++ % 3 == 0) {                                // a map point of the neighbour's own on this feature, seen by 1 .. 5 key frames
                    MapPoint m; const float dist = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
                    for (int q = 0; q < 3; q++) { m.pos[q] = x[q]; m.nrm[q] = x[q] / dist; }
                    m.maxd = dist * sf[f.octave]; m.mind = m.maxd / sf[p.orb_nlevels - 1]; memcpy(m.desc, d, 32);
                    m.obs.push_back(std::make_pair(j, (int)K.mp.size()));
                    for (int o = 0; o < k % 5; o++) m.obs.push_back(std::make_pair(-3 - o, 0));
                    held = (int)points.size(); points.push_back(m);
                }
                K.mp.push_back(held);
            }
        }
        printf("current key frame: %d features, %d map points; neighbours: %d and %d features\n", N, nCurPoints, (int)kfs[1].kpu.size(), (int)kfs[2].kpu.size());

        // ---- 1. Fuse(pKFi, vpMapPointMatches) for all targets in one call ----
        const std::vector<int> vpMapPointMatches = cur.mp;          // one entry per feature of the current key frame, NULLs included
        const size_t Ne = (size_t)(N > 0 ? N : 1);
        std::vector<float> pos(3 * Ne, 0.f), nrm(3 * Ne, 0.f), maxd(Ne, 0.f), mind(Ne, 0.f); std::vector<uint8_t> desc(32 * Ne, 0);
        for (int i = 0; i < N; i++) {
            const int m = vpMapPointMatches[i];
            if (m < 0) continue;
            memcpy(&pos[3 * (size_t)i], points[m].pos, 12); memcpy(&nrm[3 * (size_t)i], points[m].nrm, 12); maxd[i] = points[m].maxd; mind[i] = points[m].mind;
            memcpy(&desc[32 * (size_t)i], points[m].desc, 32);
        }
        hvo_fuse_map side = { N, pos.data(), nrm.data(), maxd.data(), mind.data(), desc.data() };
        std::vector<std::vector<uint8_t> > skip(2, std::vector<uint8_t>(Ne, 1));
        hvo_fuse_keyframe target[2];
        for (int j = 0; j < 2; j++) {
            const KeyFrame &K = kfs[j + 1];
            for (int i = 0; i < N; i++) { const int m = vpMapPointMatches[i]; skip[j][i] = m < 0 || points[m].bad || points[m].IsInKeyFrame(j + 1); }
            target[j] = hvo_fuse_keyframe();
            target[j].n = (int)K.kpu.size(); target[j].kp_un = K.kpu.data(); target[j].uright = K.ur.data(); target[j].desc = K.desc.data();
            memcpy(target[j].Tcw, K.Tcw, sizeof(K.Tcw)); target[j].skip = skip[j].data();
        }
        std::vector<hvo::FuseMatches> res;
        matcher.Fuse(cam, bounds, sp.bf, side, 2, target, res);
        int fusedFirst = 0;
        for (int j = 0; j < 2; j++) {
            int nR, nA, nS; walk(j + 1, vpMapPointMatches, res[j], nR, nA, nS);
            printf("first loop, neighbour %d: %d searched, %d fused: %d replaced, %d added, %d skipped in the walk (grid %.3f, projection %.3f, search %.3f ms)\n", j + 1,
                   res[j].n_searched, res[j].n_fused, nR, nA, nS, res[j].kernel_ms[0], res[j].kernel_ms[1], res[j].kernel_ms[2]);
            fusedFirst += res[j].n_fused;
        }

        // ---- 2. Fuse(mpCurrentKeyFrame, vpFuseCandidates): the candidates as slots of a resident point map, the key frame resident ----
        std::vector<int> vpFuseCandidates; std::vector<uint8_t> isCandidate(points.size(), 0);      // mnFuseCandidateForKF
        for (int j = 1; j <= 2; j++) for (int m : kfs[j].mp) {
            if (m < 0 || points[m].bad || isCandidate[m]) continue;
            isCandidate[m] = 1; vpFuseCandidates.push_back(m);
        }
        const int nc = (int)vpFuseCandidates.size(); const size_t Nc = (size_t)(nc > 0 ? nc : 1);
        std::vector<float> cpos(3 * Nc), cnrm(3 * Nc), cmax(Nc), cmin(Nc); std::vector<uint8_t> cdesc(32 * Nc), cskip(Nc, 0); std::vector<int32_t> slots(Nc, 0);
        for (int k = 0; k < nc; k++) {
            const MapPoint &m = points[vpFuseCandidates[k]];
            memcpy(&cpos[3 * (size_t)k], m.pos, 12); memcpy(&cnrm[3 * (size_t)k], m.nrm, 12); cmax[k] = m.maxd; cmin[k] = m.mind; memcpy(&cdesc[32 * (size_t)k], m.desc, 32);
            cskip[k] = m.bad || m.IsInKeyFrame(0); slots[k] = k;
        }
        hvo::PointMap map(0, nc);
        if (nc) map.setMany(0, nc, cpos.data(), cnrm.data(), cmax.data(), cmin.data(), cdesc.data(), nullptr, nullptr);
        hvo::FuseMatches r2;
        matcher.Fuse(fs, t, cam, sp.bf, cur.Tcw, cskip.data(), nullptr, map.get(), nc, slots.data(), r2);
        int nR, nA, nS; walk(0, vpFuseCandidates, r2, nR, nA, nS);
        printf("second call: %d candidates, %d searched, %d fused: %d replaced, %d added, %d skipped in the walk (grid %.3f, projection %.3f, search %.3f ms)\n", nc,
               r2.n_searched, r2.n_fused, nR, nA, nS, r2.kernel_ms[0], r2.kernel_ms[1], r2.kernel_ms[2]);
        int alive = 0;
        for (const MapPoint &m : points) alive += m.bad ? 0 : 1;
        printf("map: %d points before, %d after; fused %d + %d\n", (int)points.size(), alive, fusedFirst, r2.n_fused);
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
