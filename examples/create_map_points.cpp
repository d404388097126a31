// create_map_points.cpp -- LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:335-580) on a toy map through the C++ mirror
// (include/hvo.hpp): the epipolar search and the triangulation of the current key frame against ALL its neighbours in one device call,
// and the caller's walk over what it returns.
//
// The call replaces lines 367-559 of the reference for every neighbour at once: the baseline test, ComputeF12, SearchForTriangulation and,
// per match, the parallax test, the triangulation and the gates.  What stays on the host is what the reference does with pointers
// (:562-577): new MapPoint(x3D), AddObservation on both sides, AddMapPoint on both key frames, ComputeDistinctiveDescriptors,
// UpdateNormalAndDepth, mpMap->AddMapPoint, mlpRecentAddedMapPoints -- per entry of created_idx1 / created_idx2, neighbour by neighbour in
// list order.  The chain over the neighbours is already resolved: a feature appears in exactly one neighbour's list, the first one whose
// match passed every gate.  A caller that leaves early (`if(i>0 && CheckNewKeyFrames()) return;`) simply stops walking: the lists of the
// neighbours walked so far do not depend on the ones after them.
//
// The toy map: the current key frame is one extracted frame, resident on its stream with its bag of words (camera = world); every third
// feature with depth already holds a map point.  Three neighbours see the same scene from 12 cm to the right, from 2 cm aside (below mb:
// not searched) and from 20 cm ahead.  The vocabulary is a small random tree built here.
// Reads one raw 640x480 gray (u8) + depth (u16) pair.
//
// build:  g++ -std=c++14 -Iinclude examples/create_map_points.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o create_map_points
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include "hvo.hpp"

struct MapPoint { float pos[3]; std::vector<std::pair<int, int> > obs; };      // (key frame, feature)
struct KeyFrame {
    std::vector<hvo_keypoint> kpu; std::vector<float> ur, zd; std::vector<uint8_t> desc, has; std::vector<int32_t> node; float Tcw[12]; std::vector<int> mp;
};

static bool read_raw(const char *path, void *dst, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

// LocalMapping.cc:562-577 for the points of neighbours 0 .. last, in list order
static int walk(std::vector<MapPoint> &points, std::vector<KeyFrame> &kfs, const std::vector<hvo::NewMapPoints> &res, int last, std::vector<int> &recent)
{
    int nnew = 0;
    for (int j = 0; j <= last && j < (int)res.size(); j++) {           // `if(i>0 && CheckNewKeyFrames()) return;` is this loop's bound
        const hvo::NewMapPoints &r = res[j];
        for (int k = 0; k < r.n_created; k++) {
            const int idx1 = r.created_idx1[k], idx2 = r.created_idx2[k];
            MapPoint m;                                                  // new MapPoint(x3D, mpCurrentKeyFrame, mpMap)
            for (int q = 0; q < 3; q++) m.pos[q] = r.x3d[3 * (size_t)idx1 + q];
            m.obs.push_back(std::make_pair(0, idx1)); m.obs.push_back(std::make_pair(j + 1, idx2));        // AddObservation x 2
            const int id = (int)points.size();
            kfs[0].mp[idx1] = id; kfs[j + 1].mp[idx2] = id;             // AddMapPoint x 2 (two idx1 may name one idx2: the later one stays, as in the reference)
            points.push_back(m); recent.push_back(id); nnew++;        // ComputeDistinctiveDescriptors, UpdateNormalAndDepth: not shown
        }
    }
    return nnew;
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
        // a small vocabulary: k = 4, L = 3, random descriptors, every leaf a word of weight 1
        const int k = 4, L = 3;
        std::vector<int32_t> parent; std::vector<uint8_t> leaf, vdesc; std::vector<double> weight;
        unsigned lcg = 12345u;
        std::vector<int> level_nodes(1, 0);
        for (int l = 1; l <= L; l++) {
            std::vector<int> next;
            for (int pn : level_nodes) for (int c = 0; c < k; c++) {
                parent.push_back(pn); leaf.push_back(l == L ? 1 : 0); weight.push_back(1.0);
                for (int b = 0; b < 32; b++) { lcg = lcg * 1664525u + 1013904223u; vdesc.push_back((uint8_t)(lcg >> 24)); }
                next.push_back((int)parent.size());
            }
            level_nodes.swap(next);
        }
        hvo::ORBVocabulary voc(0, k, L, HVO_VOC_L1_NORM, HVO_VOC_TF_IDF, (int)parent.size(), parent.data(), leaf.data(), vdesc.data(), weight.data());
        // the current key frame: extracted, collected for the toy map's own use, still resident
        const int kp_cap = fs.kpCap();
        std::vector<KeyFrame> kfs(4);
        KeyFrame &cur = kfs[0];
        std::vector<hvo_keypoint> kp(kp_cap);
        cur.kpu.resize(kp_cap); cur.ur.resize(kp_cap); cur.zd.resize(kp_cap); cur.desc.resize((size_t)kp_cap * 32);
        const int64_t t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
        hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.desc = cur.desc.data(); fo.kp_cap = kp_cap;
        fs.collect(t, fo, cur.kpu.data(), cur.ur.data(), cur.zd.data());
        const int N = fo.n_kp;
        cur.kpu.resize(N); cur.ur.resize(N); cur.zd.resize(N); cur.desc.resize((size_t)N * 32); cur.mp.assign(N, -1); cur.has.assign(N > 0 ? N : 1, 0);
        const float I[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
        memcpy(cur.Tcw, I, sizeof(I));
        hvo::BowVectors bow;
        hvo::Frame::ComputeBoW(fs, t, voc, bow, 1);                  // the node ids stay on the frame; the copy here serves the neighbours
        std::vector<MapPoint> points;
        for (int i = 0, q = 0; i < N; i++) {
            if (!(cur.zd[i] > 0) || q++ % 3) continue;
            MapPoint m; const float z = cur.zd[i];
            m.pos[0] = (cur.kpu[i].x - p.cx) / p.fx * z; m.pos[1] = (cur.kpu[i].y - p.cy) / p.fy * z; m.pos[2] = z;
            m.obs.push_back(std::make_pair(0, i));
            cur.mp[i] = (int)points.size(); cur.has[i] = 1; points.push_back(m);
        }
        const int nOld = (int)points.size();
        // the neighbours: the same scene from three poses (camera centres 12 cm right, 2 cm aside, 20 cm ahead), six descriptor bits of noise
        const float centre[3][3] = { { 0.12f, 0.f, 0.f }, { 0.02f, 0.f, 0.f }, { 0.f, 0.01f, 0.2f } };
        for (int j = 1; j <= 3; j++) {
            KeyFrame &K = kfs[j];
            memcpy(K.Tcw, I, sizeof(I)); for (int q = 0; q < 3; q++) K.Tcw[4 * q + 3] = -centre[j - 1][q];
            for (int i = 0; i < N; i++) {
                const float z = cur.zd[i] > 0 ? cur.zd[i] : 2.5f;      // a feature without depth: somewhere along its ray
                const float xc = (cur.kpu[i].x - p.cx) / p.fx * z + K.Tcw[3], yc = (cur.kpu[i].y - p.cy) / p.fy * z + K.Tcw[7], zc = z + K.Tcw[11];
                if (!(zc > 0.3f) || (j == 1 && i % 4 == 0)) continue;   // the first neighbour misses a quarter of the scene: the third creates those
                hvo_keypoint f = cur.kpu[i]; f.x = p.fx * xc / zc + p.cx + 0.25f * (float)((i % 3) - 1); f.y = p.fy * yc / zc + p.cy - 0.25f * (float)((i % 5) - 2);
                const bool has_depth = cur.zd[i] > 0 && i % 7 != 0;
                K.kpu.push_back(f); K.ur.push_back(has_depth ? f.x - sp.bf / zc : -1.f); K.zd.push_back(has_depth ? zc : -1.f);
                uint8_t d[32]; memcpy(d, &cur.desc[32 * (size_t)i], 32);
                for (int b = 0; b < 6; b++) d[(i + 5 * b) % 32] ^= (uint8_t)(1u << ((i + b) % 8));
                K.desc.insert(K.desc.end(), d, d + 32);
                K.node.push_back(bow.node_id[i]);                      // (a real neighbour carries the node ids of its own ComputeBoW)
                K.has.push_back(i % 11 == 0 ? 1 : 0); K.mp.push_back(-1);
            }
        }
        std::vector<hvo_np_keyframe> nb(3);
        for (int j = 0; j < 3; j++) {
            KeyFrame &K = kfs[j + 1];
            nb[j] = hvo_np_keyframe();
            nb[j].n = (int)K.kpu.size(); nb[j].kp_un = K.kpu.data(); nb[j].uright = K.ur.data(); nb[j].depth = K.zd.data(); nb[j].desc = K.desc.data();
            nb[j].node_id = K.node.data(); nb[j].has_map_point = K.has.data(); memcpy(nb[j].Tcw, K.Tcw, sizeof(K.Tcw)); nb[j].mb = cam.b;
        }
        hvo::LocalMapping mapper(ctx.get());
        std::vector<hvo::NewMapPoints> res; std::vector<int> owner; float ms[3];
        const int nnew = mapper.CreateNewMapPoints(fs, t, voc, cam, cur.Tcw, cur.has.data(), N, 3, nb.data(), res, &owner, p.orb_scale_factor, p.orb_nlevels, ms);
        printf("current key frame: %d features, %d map points\n", N, nOld);
        for (int j = 0; j < 3; j++) {
            int nm = 0; for (int i = 0; i < N; i++) nm += res[j].match_idx2[i] >= 0 ? 1 : 0;
            printf("neighbour %d: gate %d, %d matches, %d created\n", j, res[j].gate, nm, res[j].n_created);
        }
        // a caller that sees a new key frame after neighbour 0 walks one list; the lists are the same ones
        std::vector<MapPoint> early_points = points; std::vector<KeyFrame> early_kfs = kfs; std::vector<int> early_recent;
        const int nearly = walk(early_points, early_kfs, res, 0, early_recent);
        std::vector<int> recent;
        const int nwalk = walk(points, kfs, res, 2, recent);
        int held = 0; for (int i = 0; i < N; i++) held += cur.mp[i] >= 0 ? 1 : 0;
        printf("created %d new map points (the call says %d); the current key frame now holds %d; leaving after neighbour 0: %d\n", nwalk, nnew, held, nearly);
        printf("kernels: search %.3f ms, triangulation %.3f ms, resolve %.3f ms\n", ms[0], ms[1], ms[2]);
    } catch (const hvo::Error &e) {
        fprintf(stderr, "hvo error %d: %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
