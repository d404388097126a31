// new_keyframe_host.cpp -- the host side of the path hvo_stream_create_keyframe_features replaces, for tools/new_keyframe_timing.py: the loops of
// Tracking::CreateNewKeyFrame (reference src/Tracking.cc:3049-3187) over a frame's downloaded arrays in plain single-thread C++ -- sort by depth,
// the counters, UnprojectStereo, the sole observer's normal and distance range, PtToWorldCoord and computeStructConstrains for the new lines --
// filling the arrays set_many takes.  Plain float / double arithmetic, not the library's readings: it is timed, not compared bit for bit.
//
//   new_keyframe_host <file> <calls>   ->   "<median ms> <points created> <lines created>"
// file: int32 n_kp, n_kl; float fx, fy, cx, cy, th; float Tcw[12]; then n_kp x (float u, v, z; int32 octave, held) and n_kl x (double A[3], B[3]; int32 held)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

struct Pt { float u, v, z; int32_t octave, held; };
struct Ln { double A[3], B[3]; int32_t held, pad; };

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n[2]; float c[5], T[12];
    if (fread(n, 4, 2, f) != 2 || fread(c, 4, 5, f) != 5 || fread(T, 4, 12, f) != 12) return 2;
    std::vector<Pt> P(n[0]); std::vector<Ln> L(n[1]);
    if (fread(P.data(), sizeof(Pt), P.size(), f) != P.size() || fread(L.data(), sizeof(Ln), L.size(), f) != L.size()) return 2;
    fclose(f);
    const int calls = atoi(argv[2]);
    float sf[8]; sf[0] = 1.f; for (int l = 1; l < 8; l++) sf[l] = sf[l - 1] * 1.2f;
    float R[9], Ow[3];
    for (int r = 0; r < 3; r++) { Ow[r] = 0; for (int k = 0; k < 3; k++) { R[3 * r + k] = T[4 * k + r]; Ow[r] -= T[4 * k + r] * T[4 * k + 3]; } }
    const double cpar = cos(3.0 * 0.0174533), cperp = cos(87.0 * 0.0174533);
    std::vector<double> ms; int np = 0, nl = 0;
    std::vector<float> pos, nrm, mx, mi; std::vector<double> lpos, lw, ln; std::vector<float> lmx, lmi; std::vector<uint8_t> rel;
    for (int it = 0; it < calls + 5; it++) {
        const auto t0 = std::chrono::steady_clock::now();
        pos.clear(); nrm.clear(); mx.clear(); mi.clear(); lpos.clear(); lw.clear(); ln.clear(); lmx.clear(); lmi.clear(); rel.clear();
        std::vector<std::pair<float, int>> v; v.reserve(P.size());
        for (int i = 0; i < n[0]; i++) if (P[i].z > 0) v.push_back(std::make_pair(P[i].z, i));
        std::sort(v.begin(), v.end());
        int cnt = 0;
        for (size_t j = 0; j < v.size(); j++) {
            const Pt &p = P[v[j].second];
            if (p.held < 0) {
                const float x = (p.u - c[2]) * p.z / c[0], y = (p.v - c[3]) * p.z / c[1];
                float X[3], d[3];
                for (int r = 0; r < 3; r++) { X[r] = R[3 * r] * x + R[3 * r + 1] * y + R[3 * r + 2] * p.z + Ow[r]; d[r] = X[r] - Ow[r]; }
                const float dist = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                for (int r = 0; r < 3; r++) { pos.push_back(X[r]); nrm.push_back(d[r] / dist); }
                mx.push_back(dist * sf[p.octave & 7]); mi.push_back(mx.back() / sf[7]);
            }
            cnt++;
            if (v[j].first > c[4] && cnt > 100) break;
        }
        std::vector<std::pair<float, int>> w; w.reserve(L.size());
        for (int i = 0; i < n[1]; i++) if (L[i].A[2] != 0 && L[i].B[2] != 0) w.push_back(std::make_pair((float)std::max(L[i].A[2], L[i].B[2]), i));
        std::sort(w.begin(), w.end());
        std::vector<double> dir(3 * L.size());
        for (int i = 0; i < n[1]; i++) for (int r = 0; r < 3; r++)
            dir[3 * i + r] = R[3 * r] * (L[i].B[0] - L[i].A[0]) + R[3 * r + 1] * (L[i].B[1] - L[i].A[1]) + R[3 * r + 2] * (L[i].B[2] - L[i].A[2]);
        cnt = 0;
        for (size_t j = 0; j < w.size(); j++) {
            const Ln &l = L[w[j].second];
            if (l.held >= 0) continue;
            double S[3], E[3], m[3], wv[3];
            for (int r = 0; r < 3; r++) {
                S[r] = R[3 * r] * l.A[0] + R[3 * r + 1] * l.A[1] + R[3 * r + 2] * l.A[2] + Ow[r]; E[r] = R[3 * r] * l.B[0] + R[3 * r + 1] * l.B[1] + R[3 * r + 2] * l.B[2] + Ow[r];
                m[r] = 0.5 * (S[r] + E[r]) - Ow[r]; wv[r] = S[r] - E[r];
            }
            const double dm = std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]), dw = std::sqrt(wv[0] * wv[0] + wv[1] * wv[1] + wv[2] * wv[2]);
            for (int r = 0; r < 3; r++) { lpos.push_back(S[r]); ln.push_back(m[r] / dm); lw.push_back(wv[r] / dw); }
            for (int r = 0; r < 3; r++) lpos.push_back(E[r]);
            lmx.push_back((float)dm); lmi.push_back((float)dm);
            for (int i = 0; i < n[1]; i++) {
                uint8_t q = 0;
                if (L[i].A[0] != 0.0) {
                    const double *e = &dir[3 * i];
                    const double a = std::fabs((e[0] * wv[0] + e[1] * wv[1] + e[2] * wv[2]) / (std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) * dw));
                    q = a < cperp ? 2 : (a > cpar ? 1 : 0);
                }
                rel.push_back(q);
            }
            cnt++;
            if (w[j].first > c[4] && cnt > 100) break;
        }
        const auto t1 = std::chrono::steady_clock::now();
        if (it >= 5) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        np = (int)mx.size(); nl = (int)lmx.size();
    }
    std::sort(ms.begin(), ms.end());
    printf("%.4f %d %d\n", ms.empty() ? 0.0 : ms[ms.size() / 2], np, nl);
    return 0;
}
