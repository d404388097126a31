// keyframe_db.cpp -- the head of Tracking::Relocalization (reference src/Tracking.cc:3763-3796) on a resident frame through the C++ mirror
// (include/hvo.hpp): mCurrentFrame.ComputeBoW(), mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame) on the database that lives on
// the device, and ORBmatcher::SearchByBoW against the candidates it returned, all of them in one call.  The frames but the last play the
// key frames: each is added to the database with the bag of words ComputeBoW left on it (device to device, as
// LocalMapping::ProcessNewKeyFrame would), and consecutive key frames are each other's covisible neighbours.  The last frame is the one to
// relocalise.  Between its upload and the match vectors only slot numbers and the candidates' host arrays cross PCIe; the bag of words of
// the frame never comes down for the query.  The PnP loop that follows is examples/relocalization_pnp.cpp.  No vocabulary file is needed:
// a small random k = 8, L = 3 tree is generated.  Reads raw 640x480 gray (u8) + depth (u16) pairs.
//
// build:  g++ -std=c++14 -Iinclude examples/keyframe_db.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o keyframe_db
#include <cstdio>
#include <cstring>
#include <vector>
#include "hvo.hpp"

static bool read_raw(const char *path, void *dst, size_t bytes)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(dst, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

// a full k-ary tree of depth L with random descriptors and weights, rows level by level (parents before children)
static void make_vocabulary(int k, int L, std::vector<int32_t> &parent, std::vector<uint8_t> &leaf, std::vector<uint8_t> &desc, std::vector<double> &weight)
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    int first = 0, count = 1;
    for (int level = 1; level <= L; level++) {
        const int base = (int)parent.size() + 1;
        for (int p = first; p < first + count; p++)
            for (int c = 0; c < k; c++) {
                parent.push_back(p); leaf.push_back(level == L);
                for (int b = 0; b < 32; b++) desc.push_back((uint8_t)(rnd() >> 24));
                weight.push_back(level == L ? 0.5 + (double)(rnd() % 1000) / 200.0 : 0.0);
            }
        first = base; count *= k;
    }
}

int main(int argc, char **argv)
{
    if (argc < 5 || argc % 2 != 1) { fprintf(stderr, "usage: %s kf0.u8 kf0.u16 [kf1.u8 kf1.u16 ...] frame.u8 frame.u16\n", argv[0]); return 2; }
    const int W = 640, H = 480, n = (argc - 1) / 2, nKFs = n - 1;
    std::vector<uint8_t> gray(W * H); std::vector<uint16_t> depth(W * H);
    try {
        hvo_params p; hvo_default_params(&p);
        hvo_stream_params sp = hvo_stream_params(); sp.width = W; sp.height = H; sp.depth = 2; sp.seed = 7u; sp.bf = 40.f;
        sp.stages = HVO_STAGE_ORB;
        hvo::FrameStream fs(p, sp);
        std::vector<int32_t> vp; std::vector<uint8_t> vl, vd; std::vector<double> vw;
        make_vocabulary(8, 3, vp, vl, vd, vw);
        hvo::ORBVocabulary voc(p.device, 8, 3, HVO_VOC_L1_NORM, HVO_VOC_TF_IDF, (int)vp.size(), vp.data(), vl.data(), vd.data(), vw.data());
        hvo::KeyFrameDatabase db(voc);                                        // mpKeyFrameDB: slot = the key frame's index in `kfs`
        const int levelsup = 1, kp_cap = fs.kpCap();
        struct KF { int N; std::vector<uint8_t> desc, has; std::vector<float> angle; hvo::BowVectors bow; };
        std::vector<KF> kfs(nKFs);
        int64_t t = -1; int N = 0;
        std::vector<hvo_keypoint> kp(kp_cap); std::vector<uint8_t> desc((size_t)kp_cap * 32);
        for (int k = 0; k < n; k++) {
            if (!read_raw(argv[1 + 2 * k], gray.data(), gray.size()) || !read_raw(argv[2 + 2 * k], depth.data(), depth.size() * 2)) return 3;
            t = fs.submit(hvo::Image8{ gray.data(), W, H, W }, hvo::Image16{ depth.data(), W, H, W * 2 });
            hvo_frame_out fo = hvo_frame_out(); fo.kp = kp.data(); fo.desc = desc.data(); fo.kp_cap = kp_cap;
            fs.collect(t, fo);
            N = fo.n_kp;
            if (k == nKFs) break;                                             // the frame to relocalise stays resident
            KF &K = kfs[k];
            hvo::Frame::ComputeBoW(fs, t, voc, K.bow, levelsup);               // KeyFrame::ComputeBoW
            db.add(fs, t, k);                                                 // mpKeyFrameDB->add(pKF): the bag goes from the frame to the database on the device
            K.N = N; K.desc = desc; K.has.assign(N, 1); K.angle.assign(N, 0.f);
            for (int i = 0; i < N; i++) K.angle[i] = kp[i].angle;
            printf("key frame %d: %d points (%d words)\n", k, N, (int)K.bow.bow_word.size());
        }
        for (int k = 0; k < nKFs; k++) {                                      // after UpdateConnections: GetBestCovisibilityKeyFrames(10) per key frame
            std::vector<int> nb;
            if (k > 0) nb.push_back(k - 1);
            if (k + 1 < nKFs) nb.push_back(k + 1);
            db.setCovisible(k, nb);
        }
        // Relocalization: mCurrentFrame.ComputeBoW(); vpCandidateKFs = mpKeyFrameDB->DetectRelocalizationCandidates(&mCurrentFrame) (:3763-3767)
        hvo::BowVectors bow;
        hvo::Frame::ComputeBoW(fs, t, voc, bow, levelsup);
        const std::vector<int> cand = db.DetectRelocalizationCandidates(fs, t);
        printf("frame: %d points (%d words), %d of %d key frames are candidates (query kernels %.3f ms):", N, (int)bow.bow_word.size(), (int)cand.size(), db.size(),
               db.lastKernelMs());
        for (int c : cand) printf(" %d", c);
        printf("\n");
        if (cand.empty()) { printf("relocalisation failed: no candidate\n"); return 0; }
        // matcher(0.75, true).SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i]) for every candidate (:3789-3796), in one call
        std::vector<hvo_bow_keyframe> bk(cand.size());
        for (size_t i = 0; i < cand.size(); i++) {
            const KF &K = kfs[cand[i]];
            bk[i] = hvo_bow_keyframe{ K.desc.data(), K.bow.node_id.data(), K.has.data(), K.angle.data(), K.N };
        }
        std::vector<std::vector<int>> match_kf; std::vector<int> nmatches;
        hvo::Frame::SearchByBoW(fs, t, voc, (int)cand.size(), bk.data(), match_kf, nmatches, 0.75f, true);
        for (size_t i = 0; i < cand.size(); i++) printf("candidate %d: SearchByBoW %d matches%s\n", cand[i], nmatches[i], nmatches[i] < 15 ? " (discarded)" : "");
    } catch (const hvo::Error &e) { fprintf(stderr, "hvo error: %s\n", e.what()); return 1; }
    return 0;
}
