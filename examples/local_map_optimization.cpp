// local_map_optimization.cpp -- Optimizer::LocalMapOptimization (reference src/Optimizer.cc:3014-3940, called at src/LocalMapping.cc:122)
// through the C++ mirror (include/hvo.hpp) on a toy window: the list building of :3021-3148 on toy key frames, points and lines, ONE
// device call for the graph, both rounds and the erase tests, then the host walk of :3849-3901, SetPose / SetWorldPos and the refresh of
// the moved points on a resident point map (hvo::PointMap::refresh with HVO_MR_GEOMETRY).
//
// The toy window: five key frames standing 25 cm apart along x and looking down +z.  Key frame 4 is the current one; 3, 2, 1 are its
// covisible key frames, key frame 0 (mnId == 0) is among them and stays fixed; key frame 5 sees some of their points and is an outside
// observer.  24 points and 3 lines (two along world axes, one of them with a parallel entry; the second shares x between its end points and
// is skipped whole, :3365) are seen exactly; the free poses and the
// landmarks start off the truth, one observation is a gross outlier and must come back flagged.
//
// build:  g++ -std=c++14 -Iinclude examples/local_map_optimization.cpp -L<csrc> -lhvo -Wl,-rpath,<csrc> -o local_map_optimization
#include <cmath>
#include <cstdio>
#include <cstring>
#include <list>
#include <map>
#include <vector>
#include "hvo.hpp"

namespace {

const float FX = 535.4f, FY = 539.2f, CX = 320.1f, CY = 247.6f;

struct KeyFrame {
    unsigned long mnId; float Tcw[12]; bool bad;
    unsigned long mnBALocalForKF, mnBAFixedForKF;
    std::vector<int> points, lines;                      // GetMapPointMatches() / GetMapLineMatches() as indices
    std::vector<KeyFrame *> covisible;
};
struct MapPoint { float pos[3]; bool bad; unsigned long mnBALocalForKF; std::map<KeyFrame *, std::pair<float, float>> observations; };
struct MapLine {
    double pos[6]; bool bad; int manhIdx; unsigned long mnBALocalForKF;
    std::map<KeyFrame *, std::vector<double>> observations;                       // key frame -> its key line's function
    std::map<KeyFrame *, std::vector<std::vector<double>>> parObservations;       // key frame -> the functions of its parallel key lines
};

void project(const float *T, const double *X, double *uv)
{
    const double x = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3], y = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7], z = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    uv[0] = x / z * FX + CX; uv[1] = y / z * FY + CY;
}

}  // namespace

int main()
{
    try {
        // ---- the toy map
        const int NKF = 6;
        std::vector<KeyFrame> kfs(NKF);
        float truth[NKF][12];
        for (int k = 0; k < NKF; k++) {
            const float T[12] = { 1, 0, 0, -0.25f * (float)k, 0, 1, 0, 0, 0, 0, 1, 0 };
            memcpy(truth[k], T, sizeof T); memcpy(kfs[k].Tcw, T, sizeof T);
            kfs[k].mnId = (unsigned long)k; kfs[k].bad = false; kfs[k].mnBALocalForKF = kfs[k].mnBAFixedForKF = 999;
        }
        KeyFrame *pKF = &kfs[4];
        pKF->covisible = { &kfs[3], &kfs[2], &kfs[1], &kfs[0] };
        const int NP = 24, NL = 3;
        std::vector<MapPoint> pts(NP); std::vector<MapLine> lns(NL);
        std::vector<double> Xtrue(3 * NP);
        for (int i = 0; i < NP; i++) {
            double X[3] = { -0.6 + 0.35 * (i % 6) + 0.03 * (i / 6), -0.5 + 0.33 * (i / 6), 2.5 + 0.4 * ((i * 7) % 5) };
            for (int c = 0; c < 3; c++) { X[c] = (double)(float)X[c]; Xtrue[3 * i + c] = X[c]; pts[i].pos[c] = (float)(X[c] + 0.004 * ((i + c) % 3 - 1)); }
            pts[i].bad = false; pts[i].mnBALocalForKF = 999;
            for (int k = 0; k < NKF; k++) {
                if (k == 5 && i % 3) continue;                               // the outside observer sees every third point
                double uv[2]; project(truth[k], X, uv);
                pts[i].observations[&kfs[k]] = std::make_pair((float)uv[0], (float)uv[1]);
                if (k < 5) kfs[k].points.push_back(i);
            }
        }
        pts[7].observations[&kfs[2]].first += 40.f;                          // a wrong match
        const double ends[NL][6] = { { -0.4, -0.3, 3.0, 0.5, -0.3, 3.0 }, { 0.2, -0.4, 3.5, 0.2, 0.5, 3.5004 }, { 0.3, 0.1, 2.8, 0.9, 0.5, 3.4 } };
        for (int l = 0; l < NL; l++) {
            for (int c = 0; c < 6; c++) lns[l].pos[c] = ends[l][c] + 0.003 * ((l + c) % 3 - 1);
            lns[l].bad = false; lns[l].mnBALocalForKF = 999; lns[l].manhIdx = l == 0 ? 1 : (l == 1 ? 2 : 0);
            for (int k = 0; k < 5; k++) {
                double a[2], b[2]; project(truth[k], ends[l], a); project(truth[k], ends[l] + 3, b);
                double fn[3] = { a[1] - b[1], b[0] - a[0], a[0] * b[1] - b[0] * a[1] };                     // the line through both projections
                const double n = std::sqrt(fn[0] * fn[0] + fn[1] * fn[1]);
                lns[l].observations[&kfs[k]] = { fn[0] / n, fn[1] / n, fn[2] / n };
                kfs[k].lines.push_back(l);
                if (l == 0 && k == 4) lns[l].parObservations[&kfs[k]].push_back({ (b[0] - a[0]) * 2.0, (b[1] - a[1]) * 2.0, 2.0 });
            }
        }
        // the free key frames start off the truth
        for (int k = 1; k <= 4; k++) { kfs[k].Tcw[3] += 0.004f * (float)(k - 2); kfs[k].Tcw[7] -= 0.003f; kfs[k].Tcw[11] += 0.002f * (float)k; }

        // ---- Optimizer.cc:3021-3148: the local key frames, their points and lines, the fixed cameras
        std::list<KeyFrame *> lLocalKeyFrames;
        lLocalKeyFrames.push_back(pKF); pKF->mnBALocalForKF = pKF->mnId;
        for (KeyFrame *pKFi : pKF->covisible) { pKFi->mnBALocalForKF = pKF->mnId; if (!pKFi->bad) lLocalKeyFrames.push_back(pKFi); }
        std::list<MapPoint *> lLocalMapPoints; std::list<MapLine *> lLocalMapLines;
        for (KeyFrame *k : lLocalKeyFrames) {
            for (int i : k->points) if (!pts[i].bad && pts[i].mnBALocalForKF != pKF->mnId) { lLocalMapPoints.push_back(&pts[i]); pts[i].mnBALocalForKF = pKF->mnId; }
            for (int i : k->lines) if (!lns[i].bad && lns[i].mnBALocalForKF != pKF->mnId) { lLocalMapLines.push_back(&lns[i]); lns[i].mnBALocalForKF = pKF->mnId; }
        }
        std::list<KeyFrame *> lFixedCameras;
        auto fix = [&](KeyFrame *pKFi) {
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) { pKFi->mnBAFixedForKF = pKF->mnId; if (!pKFi->bad) lFixedCameras.push_back(pKFi); }
        };
        for (MapPoint *p : lLocalMapPoints) for (auto &o : p->observations) fix(o.first);
        for (MapLine *l : lLocalMapLines) for (auto &o : l->observations) fix(o.first);

        // ---- the adaptor: the graph in the call's index convention (key frame 0 = pKF, then the other local ones, then the fixed cameras)
        hvo::LocalMapGraph g;
        std::map<KeyFrame *, int> slot; std::vector<KeyFrame *> kfOf;
        for (KeyFrame *k : lLocalKeyFrames) { slot[k] = g.addKeyFrame(k->Tcw, k->mnId == 0, FX, FY, CX, CY); kfOf.push_back(k); }
        for (KeyFrame *k : lFixedCameras) { slot[k] = g.addKeyFrame(k->Tcw, true, FX, FY, CX, CY); kfOf.push_back(k); }
        std::vector<MapPoint *> ptOf; std::vector<MapLine *> lnOf;
        for (MapPoint *p : lLocalMapPoints) {
            g.addPoint(p->pos); ptOf.push_back(p);
            for (auto &o : p->observations) if (!o.first->bad) g.addPointObservation(slot[o.first], o.second.first, o.second.second, 1.0f);     // mvInvLevelSigma2[octave 0]
        }
        for (MapLine *l : lLocalMapLines) {
            g.addLine(l->pos, l->manhIdx, (int)l->parObservations.size(), 0); lnOf.push_back(l);
            for (auto &o : l->observations) if (!o.first->bad) g.addLineObservation(slot[o.first], o.second.data());
            for (auto &o : l->parObservations) {
                if (o.first->bad || !slot.count(o.first)) continue;                    // isBad() || mnId > maxKFid: not a vertex of this graph (reading 7)
                for (size_t k = 0; k < o.second.size(); k++) g.addParEntry(slot[o.first], (int)k, o.second[k].data());
            }
        }
        g.manh_available = true;                                                       // mManhAxis = identity, mAvailableOptManh

        // ---- the call
        hvo::LocalBA ba(0);
        hvo::LocalMapResult r;
        int abortBA = 0;                                                               // mbAbortBA
        const int status = hvo::Optimizer::LocalMapOptimization(ba, g, &abortBA, r);
        printf("status %d rounds %d iterations %d + %d trials %d + %d chi2 %.6g -> %.6g, %d point / %d line observations, %.3f ms\n", status, r.res.rounds,
               r.res.iterations[0], r.res.iterations[1], r.res.trials[0], r.res.trials[1], r.res.chi2[0], r.res.chi2[1], r.res.n_pt_edges, r.res.n_line_obs, ba.lastMs());

        // ---- the walk (under mMutexMapUpdate), as written
        int erasedPoints = 0, erasedLines = 0, erasedPar = 0;
        hvo::walkErased(g, r,
            [&](int kf, int p) { if (ptOf[p]->bad) return; ptOf[p]->observations.erase(kfOf[kf]); erasedPoints++; printf("erase point %d from key frame %lu\n", p, kfOf[kf]->mnId); },
            [&](int kf, int l) { if (lnOf[l]->bad) return; lnOf[l]->observations.erase(kfOf[kf]); erasedLines++; },
            [&](int l, int kf, int k) { (void)l; (void)kf; (void)k; erasedPar++; },
            [&](int, int, int) {});
        // ---- :3903-3939
        for (size_t k = 0; k < lLocalKeyFrames.size(); k++) memcpy(kfOf[k]->Tcw, &r.Tcw[12 * k], sizeof(float) * 12);            // SetPose
        for (size_t p = 0; p < ptOf.size(); p++) memcpy(ptOf[p]->pos, &r.points[3 * p], sizeof(float) * 3);                       // SetWorldPos
        for (size_t l = 0; l < lnOf.size(); l++) if (r.line_made[l]) for (int c = 0; c < 6; c++) lnOf[l]->pos[c] = (double)r.lines[6 * l + c];

        // ---- UpdateNormalAndDepth of the moved points on the resident map (HVO_MR_GEOMETRY)
        hvo_params hp; hvo_default_params(&hp); hp.max_batch = 1;
        hvo::Context ctx(hp);
        const int n = (int)ptOf.size();
        hvo::PointMap map(0, n);
        std::vector<float> pos(3 * n), nrm(3 * n, 0.f), maxd(n, 9.f), mind(n, 1.f); std::vector<uint8_t> desc(32 * n, 0);
        for (int p = 0; p < n; p++) memcpy(&pos[3 * p], ptOf[p]->pos, sizeof(float) * 3);
        map.setMany(0, n, pos.data(), nrm.data(), maxd.data(), mind.data(), desc.data());
        std::vector<int32_t> obs_start(1, 0), ref_level(n, 0), slots(n); std::vector<float> obs_Ow, ref_Ow;
        for (int p = 0; p < n; p++) {
            slots[p] = p;
            for (auto &o : ptOf[p]->observations) { obs_Ow.push_back(-o.first->Tcw[3]); obs_Ow.push_back(-o.first->Tcw[7]); obs_Ow.push_back(-o.first->Tcw[11]); }
            obs_start.push_back((int32_t)(obs_Ow.size() / 3));
            KeyFrame *ref = ptOf[p]->observations.begin()->first;
            ref_Ow.push_back(-ref->Tcw[3]); ref_Ow.push_back(-ref->Tcw[7]); ref_Ow.push_back(-ref->Tcw[11]);
        }
        std::vector<uint8_t> obs_desc(32 * (obs_Ow.size() / 3), 0), st(n);
        hvo_mr_input in; memset(&in, 0, sizeof in);
        in.n = n; in.obs_start = obs_start.data(); in.obs_desc = obs_desc.data(); in.obs_Ow = obs_Ow.data(); in.ref_Ow = ref_Ow.data(); in.ref_level = ref_level.data();
        hvo_mr_point_out out; memset(&out, 0, sizeof out); out.status = st.data();
        map.refresh(ctx.get(), slots.data(), in, out, HVO_MR_GEOMETRY);

        // ---- what came back
        double ePose = 0, ePt = 0;
        for (int k = 1; k <= 4; k++) for (int c = 0; c < 12; c++) ePose = std::max(ePose, (double)std::fabs(kfs[k].Tcw[c] - truth[k][c]));
        for (int p = 0; p < n; p++) { const long i = ptOf[p] - &pts[0]; for (int c = 0; c < 3; c++) ePt = std::max(ePt, std::fabs((double)ptOf[p]->pos[c] - Xtrue[3 * i + c])); }
        printf("largest pose error %.3g, largest point error %.3g, erased %d point / %d line observations, %d par entries, %d Manhattan flags\n", ePose, ePt, erasedPoints,
               erasedLines, erasedPar, (int)r.manh_erase[0] + r.manh_erase[1] + r.manh_erase[2]);
        const bool ok = status == HVO_LBA_OPTIMISED && r.res.rounds == 2 && erasedPoints == 1 && ePose < 2e-3 && ePt < 2e-2 && st[0] == HVO_MR_REFRESHED;
        printf(ok ? "local map optimization ok\n" : "local map optimization FAILED\n");
        return ok ? 0 : 1;
    } catch (const hvo::Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
