// plane_update_host.cpp -- the host side of MapPlane::UpdateCoefficientsAndPoints as a stand-alone program (no device, no library):
//   plane_update_host transform IN OUT      IN: n x 12 floats (Tcw rows 0..2); OUT: n x 12 doubles = hvo_plane_update_transform of each,
//                                           through csrc/plane_update_xform.inc, the text the library compiles
//   plane_update_host merge TCW FRAME SLOT OUT [REPEAT]
//                                           the whole merge on the host, the route the device call replaces: FRAME (n x 3 floats, camera
//                                           frame) under the transform of TCW (12 floats), SLOT (m x 3 floats) appended, the voxel grid of
//                                           leaf 0.1 with exact-mean centroids; OUT: k x 3 floats.  Exit status 3 when the grid's index
//                                           overflows.  With REPEAT the merge runs that often and the median time is printed in microseconds.
// Build: g++ -O2 -std=c++14 -ffp-contract=off tools/plane_update_host.cpp -o plane_update_host
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../a-low-texture-robust-hybrid-feature-based-visual-odometry_amd/csrc/plane_update_xform.inc"

template <class T> static bool read_all(const char *path, std::vector<T> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
    v.resize(bytes > 0 ? (size_t)bytes / sizeof(T) : 0);
    const size_t got = v.empty() ? 0 : fread(v.data(), sizeof(T), v.size(), f);
    fclose(f);
    return got == v.size();
}

template <class T> static bool write_all(const char *path, const std::vector<T> &v)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), f);
    return fclose(f) == 0 && put == v.size();
}

// pcl::VoxelGrid(0.1) as oracle/planes_tail.c states it; false when the index overflows
static bool voxel_grid(const std::vector<float> &p, std::vector<float> &out)
{
    out.clear();
    const float inv = 1.0f / 0.1f;
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    std::vector<uint32_t> keep;
    for (size_t i = 0; i < p.size() / 3; i++) {
        if (!std::isfinite(p[3 * i]) || !std::isfinite(p[3 * i + 1]) || !std::isfinite(p[3 * i + 2])) continue;
        keep.push_back((uint32_t)i);
        for (int k = 0; k < 3; k++) { mn[k] = std::min(mn[k], p[3 * i + k]); mx[k] = std::max(mx[k], p[3 * i + k]); }
    }
    if (keep.empty()) return true;
    float fmin_b[3]; long long div[3];
    for (int k = 0; k < 3; k++) {
        const float lo = floorf(mn[k] * inv), hi = floorf(mx[k] * inv);
        if (!(lo >= -2147483648.f && lo < 2147483648.f && hi >= -2147483648.f && hi < 2147483648.f)) return false;
        fmin_b[k] = (float)(int)lo; div[k] = (long long)(int)hi - (long long)(int)lo + 1;
    }
    if (div[0] * div[1] > 2147483647ll || div[0] * div[1] * div[2] > 2147483647ll) return false;
    std::vector<std::pair<long long, uint32_t>> key(keep.size());
    for (size_t n = 0; n < keep.size(); n++) {
        const float *q = &p[3 * (size_t)keep[n]];
        const int i0 = (int)(floorf(q[0] * inv) - fmin_b[0]), i1 = (int)(floorf(q[1] * inv) - fmin_b[1]), i2 = (int)(floorf(q[2] * inv) - fmin_b[2]);
        key[n] = std::make_pair((long long)i0 + (long long)i1 * div[0] + (long long)i2 * div[0] * div[1], keep[n]);
    }
    std::sort(key.begin(), key.end());
    for (size_t a = 0; a < key.size();) {
        size_t b = a; long long s[3] = { 0, 0, 0 };
        for (; b < key.size() && key[b].first == key[a].first; b++)
            for (int k = 0; k < 3; k++) s[k] += llrint((double)p[3 * (size_t)key[b].second + k] * 16777216.0);
        const double den = (double)(b - a) * 16777216.0;
        for (int k = 0; k < 3; k++) out.push_back((float)((double)s[k] / den));
        a = b;
    }
    return true;
}

static bool merge(const float Tcw[12], const std::vector<float> &frame, const std::vector<float> &slot, std::vector<float> &out)
{
    double M[12];
    hvo_pu_transform(Tcw, M);
    std::vector<float> all(frame.size() + slot.size());
    for (size_t i = 0; i < frame.size() / 3; i++) {
        const double x = frame[3 * i], y = frame[3 * i + 1], z = frame[3 * i + 2];
        for (int r = 0; r < 3; r++) all[3 * i + r] = (float)(((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3]);
    }
    if (!slot.empty()) memcpy(all.data() + frame.size(), slot.data(), slot.size() * sizeof(float));
    return voxel_grid(all, out);
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "transform")) {
        std::vector<float> in;
        if (!read_all(argv[2], in) || in.size() % 12) { fprintf(stderr, "cannot read poses from %s\n", argv[2]); return 2; }
        std::vector<double> out(in.size());
        for (size_t k = 0; k < in.size() / 12; k++) hvo_pu_transform(&in[12 * k], &out[12 * k]);
        return write_all(argv[3], out) ? 0 : 2;
    }
    if ((argc == 6 || argc == 7) && !strcmp(argv[1], "merge")) {
        std::vector<float> T, frame, slot, out;
        if (!read_all(argv[2], T) || T.size() != 12 || !read_all(argv[3], frame) || frame.size() % 3 || !read_all(argv[4], slot) || slot.size() % 3) {
            fprintf(stderr, "cannot read the merge's inputs\n"); return 2;
        }
        const int repeat = argc == 7 ? atoi(argv[6]) : 1;
        std::vector<double> us;
        for (int r = 0; r < std::max(repeat, 1); r++) {
            const auto t0 = std::chrono::steady_clock::now();
            if (!merge(T.data(), frame, slot, out)) return 3;
            us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(us.begin(), us.end());
        if (argc == 7) printf("%.1f\n", us[us.size() / 2]);
        return write_all(argv[5], out) ? 0 : 2;
    }
    fprintf(stderr, "usage: %s transform IN OUT | merge TCW FRAME SLOT OUT [REPEAT]\n", argv[0]);
    return 1;
}
