// line_triang.hip -- LocalMapping::CreateNewMapLinesConstraint (reference src/LocalMapping.cc:1064-1565) for all neighbour key frames in one
// call with one synchronisation (a staged call: staged_call.hpp; the searches are match.hip's match_lines_enqueue).
//
// Why one launch sequence serves the loops.  LSDmatcher::SearchForTriangulation(.., true) (src/LSDmatcher.cpp:1195-1231) keeps i -> j only
// if j -> i, so a match vector maps current lines to a neighbour's lines injectively, and the key frame at list position p is only ever
// indexed through match vector p.  The only state the pair loops write and later read is the occupancy (AddMapLine on the three key
// frames): a creation at (pair, ikl) occupies ikl, M_a[ikl] in pKF2 and M_b[ikl] in pKF3, and those two are reached again only through the
// same ikl.  So every (pair, ikl) is evaluated under the occupancy at entry and the line at ikl goes to the first pair in (a, b) order that
// passes.  `if(i>1 && CheckNewKeyFrames()) return;` leaves before anything is created: the caller discards the result.
//
//   match_lines_enqueue (mode 2)   per searched neighbour, back to back: k_hamming_knn2 + k_frame_bf_epilogue both ways, k_mutual_check
//   k_nl_occupancy    per searched neighbour: `GetMapLine(i) || GetMapLine(j)` on the mutual matches; writes M and nlmatch
//   k_nl_triangulate  one lane per (pair, ikl): every gate in the reference's order, outcome = the first `continue` met; both end points as
//                     far as they were computed.  The two 4 x 4 solves run in ONE loop over the end point (one copy of the Jacobi code),
//                     the matrices in registers with constant indices after unrolling
//   k_nl_resolve      per ikl the first pair with outcome CREATED is the owner
//   k_nl_compact      per pair the list {ikl : owner == pair} in ascending ikl with idx1 and idx2 (sm_compact_pos)
//
// The compacted list and the positional key frames.  A gated neighbour is skipped before its match vector is pushed, and the pair loops
// read vpNeighKFs[a] by list position: HVO_NL_PAIR_AS_WRITTEN pairs match vector S[a] (the a-th searched neighbour) with key frame a,
// HVO_NL_PAIR_ALIGNED with key frame S[a].  Everything a key frame contributes is per key frame (F21 and R12 need the current pose only),
// so a pair is four positions.
//
// Readings (tests/new_lines_ref.py is the definition).  Only + - * / sqrt and fabs in the written order, nothing
// contracted.  The readings of new_points.hip hold: dot3f for every element of a float matrix product (also 3 x 3 times 3 x 1 and
// 1 x 3 times 3 x 4), cv::norm and Mat::dot as double sums, inv() as OpenCV's closed 3 x 3 form, Mat / scalar as a double reciprocal,
// cv::SVD::compute as np_svd4.  New here:
//   per key frame (host)  M = K Tcw by dot3f; R21 = Rcw2 Rwc1, R12 = Rcw1 Rwc2 by dot3f; t21 = Rcw2 (Rwc2 tcw2 - Rwc1 tcw1): two dot3f
//                         products, a float subtraction, a dot3f product; F21 = ((K2^T.inv() t21x) R21) K1.inv() left to right
//   sigma2                sf[0] = 1, sf[l] = sf[l - 1] * scale_factor, sigma2[l] = sf[l] * sf[l] in float (LINEextractor's constructor)
//   klF, lineVector2      the double line function narrowed to float per element
//   Result1 / 2           Th = F21 (x, y, 1) by dot3f; (float)(dot / (norm * norm)) in double; fabsf, then compared as a double with 0.996
//   L = lS_.cross(lE_)    lS_ = K.inv() (x, y, 1) by dot3f; each cross element two float products and a float subtraction
//   norm_, CosSita        (float)norm; tWorldVector /= norm_ and L1 /= norm_ element * (1.0 / (double)norm_) rounded to float;
//                         CosSita = (float)fabs(double dot), compared as a double with 0.0087 (a NaN passes on)
//   A                     rows 0 and 1 by dot3f over the columns of M3 / M2; rows 2 and 3 one float product then one float subtraction
//   s3D, e3D              x_k * (1.0 / x_3) in double, rounded to float
//   cosParallax           (float)(double dot / (double)(dist1 * dist2)), the product of the two float distances in float; >= 0.99998 as doubles
//   ratios                float distance / float median depth, compared as doubles with 0.3; ratio3 > 1 in float
//   SZC, x, y             (float)(Mat::dot(row, p) + (double)t); z <= 0 fails, a NaN passes on; invz = (float)(1.0 / (double)z)
//   u, v                  fx * x * invz + cx left to right in float
//   err                   (fn0 * (double)u + fn1 * (double)v) + fn2 in double; err * err > 3.84 * (double)sigma2[octave]
//   overlap               fabs((double)angle) against 3.0 * PI / 4.0 and 1.0 * PI / 4.0 with PI = 3.1415926; std::min(a, b) = b < a ? b : a and
//                         std::max(a, b) = a < b ? b : a on floats in the argument order of the text; the ratios in float, compared as
//                         doubles with 0.85.  A zero-length segment makes a ratio inf or NaN: the comparison is false and the triple passes on
//   octaves               an octave of the three lines outside [0, n_levels) refuses the triple (HVO_NL_BAD_OCTAVE) after the occupancy tests
#include "hvo_internal.hpp"
#include "slot_map.hpp"
#include "frame_view.hpp"
#include "staged_call.hpp"
#include "triangulate4.inc"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#define NL_BLOCK SM_BLOCK
#define NL_MAXN HVO_NL_MAX_LINES
#define NL_MAXKF HVO_NL_MAX_NEIGHBOURS
#define NL_PI 3.1415926

struct NlKf { float R[9], t[3], Ow[3], fx, fy, cx, cy, Ki[9], M[12], F21[9], R1k[9], med; int n; };
struct NlPair { int kf2, kf3, mv2, mv3; };
struct NlDev {
    const hvo_keyline *c_kl; const double *c_fn; const uint8_t *c_has; int n1;
    const NlKf *kf;                                              // the neighbours, then the current key frame at index n_kf
    int n_kf;
    const hvo_keyline *k_kl; const double *k_fn; const uint8_t *k_has;      // neighbour j's arrays at base + j * ct
    const NlPair *pairs; const int32_t *M; const float *sig;
    int cq, ct, n_pairs, nb, n_levels;
    int8_t *outcome; float *line3d; int32_t *owner; uint8_t *pass; int *blockcnt, *ncreated; int32_t *c0, *c1, *c2;
};

// SearchForTriangulation's last test (LSDmatcher.cpp:1222) on the mutual matches of one neighbour; one workgroup, like k_mutual_check
__global__ __launch_bounds__(256) void k_nl_occupancy(int32_t *__restrict__ m12, int n1, int n2, const uint8_t *__restrict__ has1, const uint8_t *__restrict__ has2,
                                                      int *__restrict__ nmatch)
{
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n1; i += 256) {
        const int j = m12[i];
        const bool ok = j >= 0 && j < n2 && !has1[i] && !has2[j];
        m12[i] = ok ? j : -1;
        mine += ok;
    }
    if (mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) *nmatch = s_cnt;
}

static __host__ __device__ __forceinline__ void nl_cross(const float *a, const float *b, float *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// L = (K.inv() lS).cross(K.inv() lE)
static __host__ __device__ __forceinline__ void nl_plane_normal(const float *Ki, const hvo_keyline &k, float *L)
{
    float s[3], e[3];
#pragma unroll
    for (int r = 0; r < 3; r++) { s[r] = np_dot3f(Ki[3 * r], Ki[3 * r + 1], Ki[3 * r + 2], k.sx, k.sy, 1.0f); e[r] = np_dot3f(Ki[3 * r], Ki[3 * r + 1], Ki[3 * r + 2], k.ex, k.ey, 1.0f); }
    nl_cross(s, e, L);
}
// abs(Result) of LocalMapping.cc:1227-1232 for one end point
static __host__ __device__ __forceinline__ float nl_epi_cos(const float *F, float x, float y, float lv0, float lv1)
{
    const float th0 = np_dot3f(F[0], F[1], F[2], x, y, 1.0f), th1 = np_dot3f(F[3], F[4], F[5], x, y, 1.0f);
    const float a0 = -th1, a1 = th0;
    const double dot = (double)a0 * (double)lv0 + (double)a1 * (double)lv1;
    const double na = sqrt((double)a0 * (double)a0 + (double)a1 * (double)a1), nb = sqrt((double)lv0 * (double)lv0 + (double)lv1 * (double)lv1);
    return fabsf((float)(dot / (na * nb)));
}
// (float)(row . p + t)
static __host__ __device__ __forceinline__ float nl_cam(const float *R, float t, int r, const float *p)
{
    return (float)(np_dotd(R[3 * r], R[3 * r + 1], R[3 * r + 2], p[0], p[1], p[2]) + (double)t);
}
// the projection of p at depth z and the line-distance test: true = refused
static __host__ __device__ __forceinline__ bool nl_reproj_fails(const NlKf &k, const float *p, float z, const double *fn, float sigma2, float *u, float *v)
{
    const float x = nl_cam(k.R, k.t[0], 0, p), y = nl_cam(k.R, k.t[1], 1, p);
    const float invz = (float)(1.0 / (double)z);
    *u = k.fx * x * invz + k.cx; *v = k.fy * y * invz + k.cy;
    const double err = (fn[0] * (double)*u + fn[1] * (double)*v) + fn[2];
    return err * err > 3.84 * (double)sigma2;
}
// LocalMapping.cc:1460-1485 for one view: 0 passes, 1 the segments are disjoint, 2 a ratio is below 0.85
static __host__ __device__ __forceinline__ int nl_overlap(const hvo_keyline &k, float us, float vs, float ue, float ve)
{
    const double fa = fabs((double)k.angle);
    const bool vert = fa < 3.0 * NL_PI / 4.0 && fa > 1.0 * NL_PI / 4.0;
    const float pe = vert ? ve : ue, ps = vert ? vs : us, ks = vert ? k.sy : k.sx, ke = vert ? k.ey : k.ex;
    const float minp = ps < pe ? ps : pe, maxp = pe < ps ? ps : pe;          // min(pe, ps), max(pe, ps)
    const float maxk = ks < ke ? ke : ks, mink = ke < ks ? ke : ks;          // max(ks, ke), min(ks, ke)
    if (minp > maxk || mink > maxp) return 1;
    const float hi = maxk < maxp ? maxk : maxp, lo = minp < mink ? mink : minp;      // min(maxp, maxk), max(minp, mink)
    const float r1 = (hi - lo) / (maxp - minp), r2 = (hi - lo) / (maxk - mink);
    return ((double)r1 < 0.85 || (double)r2 < 0.85) ? 2 : 0;
}

// The three key-frame records are uniform over a workgroup, so their fields are scalar loads; a phase mark makes the record pointers opaque
// so that the loads of a later phase are not issued (and their registers held) across the two Jacobi solves.  It changes no value: it is
// an empty statement that names the three pointers as scalar registers, which holds as long as the compiler sees them as uniform (they
// derive from blockIdx and kernel arguments).  Should a compiler stop doing so the file no longer builds; replacing the macro's body by
// nothing is then correct and costs registers only, which tests/test_new_lines_budget.py reports.
#define NL_PHASE(p1, p2, p3) asm volatile("" : "+s"(p1), "+s"(p2), "+s"(p3))
// Every gate is evaluated for every lane and the first one that fires is kept: apart from the two solves the arithmetic is a few dozen
// operations, and forty nested early exits would each hold a saved exec mask.  A value behind a fired gate may be inf or NaN and an index
// behind one is replaced by 0 (every row has at least 64 staged entries); nothing reads what they give.  The cost was weighed: a lane
// without a triple (most lanes: NO_MATCH) still runs the double sqrt and divide arithmetic outside the solves on such values, and only the
// two solves are skipped; the whole kernel measures 0.06 .. 0.08 ms for 10 as for 45 pairs of 200 lines (profiles/new_lines.txt).
#define NL_GATE(cond, c) do { const bool f_ = (cond); code = (open && f_) ? (c) : code; open = open && !f_; } while (0)

__global__ __launch_bounds__(NL_BLOCK) void k_nl_triangulate(NlDev a)
{
    const int p = blockIdx.y, i = blockIdx.x * NL_BLOCK + threadIdx.x;
    if (i >= a.n1) return;
    const NlPair pr = a.pairs[p];
    const NlKf *p1 = a.kf + a.n_kf, *p2 = a.kf + pr.kf2, *p3 = a.kf + pr.kf3;
    const size_t o = (size_t)p * a.cq + (size_t)i;
    const int idx1 = a.M[(size_t)pr.mv2 * a.cq + i], idx2 = a.M[(size_t)pr.mv3 * a.cq + i];
    int code = HVO_NL_CREATED; bool open = true;
    NL_GATE(idx1 < 0 || idx2 < 0, HVO_NL_NO_MATCH);                  // (an index is -1 or a line of the searched neighbour)
    NL_GATE(idx1 >= p2->n || idx2 >= p3->n, HVO_NL_IDX_RANGE);
    const size_t o2 = (size_t)pr.kf2 * a.ct + (size_t)(open ? idx1 : 0), o3 = (size_t)pr.kf3 * a.ct + (size_t)(open ? idx2 : 0);
    NL_GATE(a.c_has[i] != 0, HVO_NL_OCCUPIED_1); NL_GATE(a.k_has[o2] != 0, HVO_NL_OCCUPIED_2); NL_GATE(a.k_has[o3] != 0, HVO_NL_OCCUPIED_3);
    const hvo_keyline l1 = a.c_kl[i], l2 = a.k_kl[o2], l3 = a.k_kl[o3];
    const double f1[3] = { a.c_fn[3 * (size_t)i], a.c_fn[3 * (size_t)i + 1], a.c_fn[3 * (size_t)i + 2] };
    const double f2[3] = { a.k_fn[3 * o2], a.k_fn[3 * o2 + 1], a.k_fn[3 * o2 + 2] }, f3[3] = { a.k_fn[3 * o3], a.k_fn[3 * o3 + 1], a.k_fn[3 * o3 + 2] };
    NL_GATE(l1.octave < 0 || l1.octave >= a.n_levels || l2.octave < 0 || l2.octave >= a.n_levels || l3.octave < 0 || l3.octave >= a.n_levels, HVO_NL_BAD_OCTAVE);
    const float sg1 = a.sig[open ? l1.octave : 0], sg2 = a.sig[open ? l2.octave : 0], sg3 = a.sig[open ? l3.octave : 0];
    // the epipolar-parallel gate (:1221-1235)
    const float lv0 = -(float)f2[1], lv1 = (float)f2[0];
    const float r1 = nl_epi_cos(p2->F21, l1.sx, l1.sy, lv0, lv1), r2 = nl_epi_cos(p2->F21, l1.ex, l1.ey, lv0, lv1);
    NL_GATE((double)r1 > 0.996 || (double)r2 > 0.996, HVO_NL_EPI_PARALLEL);
    // the three back-projected planes (:1237-1268)
    float L1[3], L2[3], L3[3], w2[3], w3[3], tw[3];
    nl_plane_normal(p1->Ki, l1, L1); nl_plane_normal(p2->Ki, l2, L2); nl_plane_normal(p3->Ki, l3, L3);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        w2[r] = np_dot3f(p2->R1k[3 * r], p2->R1k[3 * r + 1], p2->R1k[3 * r + 2], L2[0], L2[1], L2[2]);
        w3[r] = np_dot3f(p3->R1k[3 * r], p3->R1k[3 * r + 1], p3->R1k[3 * r + 2], L3[0], L3[1], L3[2]);
    }
    nl_cross(w2, w3, tw);
    float norm_ = (float)np_normd(tw[0], tw[1], tw[2]);
    NL_GATE(norm_ == 0.f, HVO_NL_NORM_ZERO_23);
    double inv = 1.0 / (double)norm_;
#pragma unroll
    for (int r = 0; r < 3; r++) tw[r] = (float)((double)tw[r] * inv);
    norm_ = (float)np_normd(L1[0], L1[1], L1[2]);
    NL_GATE(norm_ == 0.f, HVO_NL_NORM_ZERO_1);
    inv = 1.0 / (double)norm_;
#pragma unroll
    for (int r = 0; r < 3; r++) L1[r] = (float)((double)L1[r] * inv);
    const float cos_sita = (float)fabs(np_dotd(L1[0], L1[1], L1[2], tw[0], tw[1], tw[2]));
    NL_GATE((double)cos_sita > 0.0087, HVO_NL_NOT_COPLANAR);
    // the two 4 x 4 systems (:1274-1312): rows 0 and 1 are shared
    const float g3[3] = { (float)f3[0], (float)f3[1], (float)f3[2] }, g2[3] = { (float)f2[0], (float)f2[1], (float)f2[2] };
    float A0[4], A1[4];
    NL_PHASE(p1, p2, p3);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A0[c] = np_dot3f(g3[0], g3[1], g3[2], p3->M[c], p3->M[4 + c], p3->M[8 + c]);
        A1[c] = np_dot3f(g2[0], g2[1], g2[2], p2->M[c], p2->M[4 + c], p2->M[8 + c]);
    }
    float S[3] = { 0.f, 0.f, 0.f }, E[3] = { 0.f, 0.f, 0.f };
    bool haveS = false, haveE = false;
    if (open) {
#pragma unroll 1
        for (int e = 0; e < 2; e++) {
            const float px = e ? l1.ex : l1.sx, py = e ? l1.ey : l1.sy;
            float W[4][4], x[4];
#pragma unroll
            for (int c = 0; c < 4; c++) { W[0][c] = A0[c]; W[1][c] = A1[c]; W[2][c] = px * p1->M[8 + c] - p1->M[c]; W[3][c] = py * p1->M[8 + c] - p1->M[4 + c]; }
            np_svd4(W, x);
            NL_GATE(x[3] == 0.f, e ? HVO_NL_W_ZERO_E : HVO_NL_W_ZERO_S);
            const double iw = 1.0 / (double)x[3];
            const float q0 = (float)((double)x[0] * iw), q1 = (float)((double)x[1] * iw), q2 = (float)((double)x[2] * iw);
            if (e == 0) { S[0] = q0; S[1] = q1; S[2] = q2; haveS = open; }
            else { E[0] = q0; E[1] = q1; E[2] = q2; haveE = open; }
        }
    }
    NL_PHASE(p1, p2, p3);
    // the parallax of either end point against both neighbours (:1317-1345)
    float dS1 = 0.f, dS2 = 0.f;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const float *q = e ? E : S;
        const float n1[3] = { q[0] - p1->Ow[0], q[1] - p1->Ow[1], q[2] - p1->Ow[2] }, n2[3] = { q[0] - p2->Ow[0], q[1] - p2->Ow[1], q[2] - p2->Ow[2] },
                    n3[3] = { q[0] - p3->Ow[0], q[1] - p3->Ow[1], q[2] - p3->Ow[2] };
        const float d1 = (float)np_normd(n1[0], n1[1], n1[2]), d2 = (float)np_normd(n2[0], n2[1], n2[2]), d3 = (float)np_normd(n3[0], n3[1], n3[2]);
        const float c12 = (float)(np_dotd(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]) / (double)(d1 * d2));
        const float c13 = (float)(np_dotd(n1[0], n1[1], n1[2], n3[0], n3[1], n3[2]) / (double)(d1 * d3));
        NL_GATE((double)c12 >= 0.99998 || (double)c13 >= 0.99998, e ? HVO_NL_PARALLAX_E : HVO_NL_PARALLAX_S);
        if (e == 0) { dS1 = d1; dS2 = d2; }
    }
    // the three ratios against pKF2's median depth (:1347-1364)
    NL_GATE((double)(dS1 / p2->med) < 0.3, HVO_NL_RATIO_1);
    NL_GATE((double)(dS2 / p2->med) < 0.3, HVO_NL_RATIO_2);
    const float dse = (float)np_normd(E[0] - S[0], E[1] - S[1], E[2] - S[2]);
    NL_GATE(dse / p2->med > 1.0f, HVO_NL_RATIO_3);
    // six depth signs (:1366-1388)
    NL_PHASE(p1, p2, p3);
    const float zs1 = nl_cam(p1->R, p1->t[2], 2, S), ze1 = nl_cam(p1->R, p1->t[2], 2, E);
    const float zs2 = nl_cam(p2->R, p2->t[2], 2, S), ze2 = nl_cam(p2->R, p2->t[2], 2, E);
    const float zs3 = nl_cam(p3->R, p3->t[2], 2, S), ze3 = nl_cam(p3->R, p3->t[2], 2, E);
    NL_GATE(zs1 <= 0.f, HVO_NL_BEHIND_1S); NL_GATE(ze1 <= 0.f, HVO_NL_BEHIND_1S + 1);
    NL_GATE(zs2 <= 0.f, HVO_NL_BEHIND_1S + 2); NL_GATE(ze2 <= 0.f, HVO_NL_BEHIND_1S + 3);
    NL_GATE(zs3 <= 0.f, HVO_NL_BEHIND_1S + 4); NL_GATE(ze3 <= 0.f, HVO_NL_BEHIND_1S + 5);
    // six line distances (:1391-1458)
    float u1s, v1s, u1e, v1e, u2s, v2s, u2e, v2e, u3s, v3s, u3e, v3e;
    NL_GATE(nl_reproj_fails(*p1, S, zs1, f1, sg1, &u1s, &v1s), HVO_NL_REPROJ_1S);
    NL_GATE(nl_reproj_fails(*p1, E, ze1, f1, sg1, &u1e, &v1e), HVO_NL_REPROJ_1S + 1);
    NL_PHASE(p1, p2, p3);
    NL_GATE(nl_reproj_fails(*p2, S, zs2, f2, sg2, &u2s, &v2s), HVO_NL_REPROJ_1S + 2);
    NL_GATE(nl_reproj_fails(*p2, E, ze2, f2, sg2, &u2e, &v2e), HVO_NL_REPROJ_1S + 3);
    NL_PHASE(p1, p2, p3);
    NL_GATE(nl_reproj_fails(*p3, S, zs3, f3, sg3, &u3s, &v3s), HVO_NL_REPROJ_1S + 4);
    NL_GATE(nl_reproj_fails(*p3, E, ze3, f3, sg3, &u3e, &v3e), HVO_NL_REPROJ_1S + 5);
    // three overlaps (:1460-1539)
    const int o1 = nl_overlap(l1, u1s, v1s, u1e, v1e), ov2 = nl_overlap(l2, u2s, v2s, u2e, v2e), ov3 = nl_overlap(l3, u3s, v3s, u3e, v3e);
    NL_GATE(o1 != 0, HVO_NL_DISJOINT_1 + o1 - 1); NL_GATE(ov2 != 0, HVO_NL_DISJOINT_2 + ov2 - 1); NL_GATE(ov3 != 0, HVO_NL_DISJOINT_3 + ov3 - 1);
    a.outcome[o] = (int8_t)code;
    float *x = a.line3d + 6 * o;                                     // both end points as far as the reference computed them
    x[0] = haveS ? S[0] : 0.f; x[1] = haveS ? S[1] : 0.f; x[2] = haveS ? S[2] : 0.f;
    x[3] = haveE ? E[0] : 0.f; x[4] = haveE ? E[1] : 0.f; x[5] = haveE ? E[2] : 0.f;
}
#undef NL_GATE

__global__ __launch_bounds__(NL_BLOCK) void k_nl_resolve(NlDev a)
{
    const int i = blockIdx.x * NL_BLOCK + threadIdx.x;
    if (i >= a.n1) return;
    int own = -1;
    for (int p = a.n_pairs - 1; p >= 0; p--) if (a.outcome[(size_t)p * a.cq + i] == HVO_NL_CREATED) own = p;       // the first in (a, b) order
    a.owner[i] = own;
    if (own >= 0) { a.pass[(size_t)own * a.cq + i] = 1; atomicAdd(&a.blockcnt[(size_t)own * a.nb + blockIdx.x], 1); }
}

__global__ __launch_bounds__(NL_BLOCK) void k_nl_compact(NlDev a)
{
    const int p = blockIdx.y, i = blockIdx.x * NL_BLOCK + threadIdx.x;
    bool ok;
    const int at = sm_compact_pos(a.blockcnt, a.nb, a.cq, p, a.pass, a.ncreated, &ok);
    if (ok) {
        const NlPair pr = a.pairs[p];
        const size_t q0 = (size_t)p * a.cq;
        a.c0[q0 + at] = i; a.c1[q0 + at] = a.M[(size_t)pr.mv2 * a.cq + i]; a.c2[q0 + at] = a.M[(size_t)pr.mv3 * a.cq + i];
    }
}

// everything one key frame contributes (about 150 float operations; the restatement fixes the bits).  c1: the current key frame's, or null for itself
static void nl_keyframe(const hvo_nl_keyframe &K, const NlKf *c1, NlKf &c)
{
    memset(&c, 0, sizeof(c));
    pose_split(K.Tcw, c.R, c.t, c.Ow);
    c.fx = K.cam.fx; c.fy = K.cam.fy; c.cx = K.cam.cx; c.cy = K.cam.cy; c.med = K.median_depth; c.n = K.n;
    const float Km[9] = { c.fx, 0.f, c.cx, 0.f, c.fy, c.cy, 0.f, 0.f, 1.f }, Kt[9] = { c.fx, 0.f, 0.f, 0.f, c.fy, 0.f, c.cx, c.cy, 1.f };
    np_inv3(Km, c.Ki);
    for (int r = 0; r < 3; r++) for (int q = 0; q < 4; q++)
        c.M[4 * r + q] = q < 3 ? np_dot3f(Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], c.R[q], c.R[3 + q], c.R[6 + q]) : np_dot3f(Km[3 * r], Km[3 * r + 1], Km[3 * r + 2], c.t[0], c.t[1], c.t[2]);
    if (!c1) return;
    float R21[9], wa[3], wb[3], d[3], t21[3], Kti[9], M1[9], M2[9];
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) {
        R21[3 * r + q] = np_dot3f(c.R[3 * r], c.R[3 * r + 1], c.R[3 * r + 2], c1->R[3 * q], c1->R[3 * q + 1], c1->R[3 * q + 2]);
        c.R1k[3 * r + q] = np_dot3f(c1->R[3 * r], c1->R[3 * r + 1], c1->R[3 * r + 2], c.R[3 * q], c.R[3 * q + 1], c.R[3 * q + 2]);
    }
    for (int r = 0; r < 3; r++) {
        wa[r] = np_dot3f(c.R[r], c.R[3 + r], c.R[6 + r], c.t[0], c.t[1], c.t[2]);
        wb[r] = np_dot3f(c1->R[r], c1->R[3 + r], c1->R[6 + r], c1->t[0], c1->t[1], c1->t[2]);
        d[r] = wa[r] - wb[r];
    }
    for (int r = 0; r < 3; r++) t21[r] = np_dot3f(c.R[3 * r], c.R[3 * r + 1], c.R[3 * r + 2], d[0], d[1], d[2]);
    const float tx[9] = { 0.f, -t21[2], t21[1], t21[2], 0.f, -t21[0], -t21[1], t21[0], 0.f };
    np_inv3(Kt, Kti);
    np_mul3(Kti, tx, M1); np_mul3(M1, R21, M2); np_mul3(M2, c1->Ki, c.F21);
}

static bool nl_side_ok(const hvo_nl_keyframe &K)
{
    if (K.n < 0) return false;
    return K.n == 0 || (K.kl && K.linefn && K.desc && K.has_map_line);
}

// fr null: cur's host arrays go up; else the current key frame is the resident frame and cur carries Tcw, cam and has_map_line only
static int nl_run(hvo_ctx *ctx, hipStream_t st, const hvo_nl_params *P, const hvo_nl_keyframe *cur, const FrameView *fr, int n_kf, const hvo_nl_keyframe *kf,
                  hvo_nl_match *mt, int n_pairs_cap, hvo_nl_result *res, hvo_nl_summary *sum, std::string *err)
{
    const int n1 = fr ? fr->n_kl : cur->n;
    // ---- refusals: whole, before anything is written ----
    if (P->th_high > 255) { *err = "create new map lines: th_high above 255 (a distance is at most 256)"; return HVO_ERR_INVALID_ARG; }
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { *err = "create new map lines: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (P->pairing != HVO_NL_PAIR_AS_WRITTEN && P->pairing != HVO_NL_PAIR_ALIGNED) { *err = "create new map lines: unknown pairing"; return HVO_ERR_INVALID_ARG; }
    if (n_kf < 0 || n_pairs_cap < 0 || (n_kf > 0 && (!kf || !mt)) || (n_pairs_cap > 0 && !res)) { *err = "create new map lines: n_kf < 0, n_pairs_cap < 0 or no neighbours / matches / results"; return HVO_ERR_INVALID_ARG; }
    if (fr ? (n1 > 0 && !cur->has_map_line) : !nl_side_ok(*cur)) { *err = "create new map lines: the current key frame has n < 0 or lacks an array"; return HVO_ERR_INVALID_ARG; }
    if (n_kf > NL_MAXKF) { *err = "create new map lines: " + std::to_string(n_kf) + " neighbours (limit " + std::to_string(NL_MAXKF) + "); nothing was written"; return HVO_ERR_UNSUPPORTED; }
    int tmax = 0;
    for (int j = 0; j < n_kf; j++) {
        if (!nl_side_ok(kf[j])) { *err = "create new map lines: neighbour " + std::to_string(j) + " has n < 0 or lacks an array"; return HVO_ERR_INVALID_ARG; }
        if (n1 > 0 && !mt[j].match_idx) { *err = "create new map lines: a match record without match_idx"; return HVO_ERR_INVALID_ARG; }
        tmax = std::max(tmax, (int)kf[j].n);
    }
    if (n1 > NL_MAXN || tmax > NL_MAXN) {
        *err = "create new map lines: " + std::to_string(std::max(n1, tmax)) + " lines on one side (limit " + std::to_string(NL_MAXN) + "); nothing was written";
        return HVO_ERR_UNSUPPORTED;
    }
    // the gates, the compacted list of searched neighbours and the pairs
    const size_t F = (size_t)n_kf;
    NlKf c1; nl_keyframe(*cur, nullptr, c1);
    std::vector<NlKf> hk(F + 1);
    std::vector<int> gate(F), S;
    for (int j = 0; j < n_kf; j++) {
        nl_keyframe(kf[j], &c1, hk[j]);
        const float baseline = (float)np_normd(hk[j].Ow[0] - c1.Ow[0], hk[j].Ow[1] - c1.Ow[1], hk[j].Ow[2] - c1.Ow[2]);
        gate[j] = kf[j].skip ? HVO_NL_GATE_SKIP : (baseline < kf[j].mb ? HVO_NL_GATE_BASELINE : HVO_NL_GATE_SEARCHED);
        if (n_kf >= 2 && gate[j] == HVO_NL_GATE_SEARCHED) S.push_back(j);
    }
    hk[F] = c1;
    std::vector<NlPair> hp;
    if (S.size() >= 2 && n1 > 0)
        for (size_t x = 0; x + 1 < S.size(); x++) for (size_t y = x + 1; y < S.size(); y++) {
            const bool w = P->pairing == HVO_NL_PAIR_AS_WRITTEN;
            hp.push_back(NlPair{ w ? (int)x : S[x], w ? (int)y : S[y], S[x], S[y] });
        }
    const size_t NP = hp.size();
    if ((int)NP > n_pairs_cap) { *err = "create new map lines: " + std::to_string(NP) + " pairs, n_pairs_cap " + std::to_string(n_pairs_cap); return HVO_ERR_INVALID_ARG; }
    for (size_t p = 0; p < NP; p++) if (!res[p].outcome) { *err = "create new map lines: a result without outcome"; return HVO_ERR_INVALID_ARG; }
    sum->n_new = 0; sum->n_pairs = (int32_t)NP; for (int q = 0; q < 3; q++) sum->kernel_ms[q] = 0.f;
    if (n1 == 0 || S.size() < 2) {                                   // the reference returns before the pair loops (a lone search creates nothing)
        for (int j = 0; j < n_kf; j++) { mt[j].n_matched = 0; mt[j].gate = gate[j]; for (int i = 0; i < n1; i++) mt[j].match_idx[i] = -1; }
        if (sum->owner_pair) for (int i = 0; i < n1; i++) sum->owner_pair[i] = -1;
        return HVO_OK;
    }
    // ---- one carve of the context's arena: what goes up, the search's scratch, what is cleared, what comes down ----
    const size_t cq = (size_t)((n1 + NL_BLOCK - 1) / NL_BLOCK * NL_BLOCK), ct = (size_t)std::max(64, (tmax + 63) & ~63), nb = cq / NL_BLOCK;
    StageCarver C(256);
    const auto u_kf = C.take<NlKf>(F + 1); const auto u_pr = C.take<NlPair>(NP); const auto u_sig = C.take<float>(HVO_MAX_LEVELS); const auto u_chas = C.take<uint8_t>(cq);
    const auto u_ckl = C.take<hvo_keyline>(fr ? 0 : cq); const auto u_cfn = C.take<double>(fr ? 0 : cq * 3); const auto u_cds = C.take<uint8_t>(fr ? 0 : cq * 32);
    const auto u_kl = C.take<hvo_keyline>(F, ct); const auto u_fn = C.take<double>(F, ct * 3); const auto u_ds = C.take<uint8_t>(F, ct * 32); const auto u_has = C.take<uint8_t>(F, ct);
    const size_t up_end = C.mark();
    const auto s_ml = C.take<char>(match_lines_scratch_bytes((int)cq, (int)ct));
    const size_t z0 = C.mark();                                      // [z0, z1) is zeroed
    const auto s_pass = C.take<uint8_t>(NP, cq); const auto s_bc = C.take<int>(NP, nb);
    const size_t r0 = C.mark();                                      // [r0, r1) comes down; its head belongs to the zeroed range
    const auto r_cnt = C.take<int>(NP); const auto r_nm = C.take<int>(F);
    const size_t z1 = C.mark();
    const auto r_M = C.take<int32_t>(F, cq);                         // set to -1: a neighbour that is not searched has no kernel that writes its row
    const size_t m1 = C.mark();
    const auto r_out = C.take<int8_t>(NP, cq); const auto r_x = C.take<float>(NP, cq * 6);
    const auto r_c0 = C.take<int32_t>(NP, cq), r_c1 = C.take<int32_t>(NP, cq), r_c2 = C.take<int32_t>(NP, cq), r_own = C.take<int32_t>(cq);
    const size_t r1 = C.mark();
    StagedCall sc(ctx, st, "create new map lines: ", err); int rc;
    if ((rc = sc.begin(r1, up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    memcpy(u_kf.host(h), hk.data(), (F + 1) * sizeof(NlKf)); memcpy(u_pr.host(h), hp.data(), NP * sizeof(NlPair));
    float *sig = u_sig.host(h), sf = 1.0f;
    for (int l = 0; l < HVO_MAX_LEVELS; l++) { if (l > 0 && l < P->n_levels) sf = sf * P->scale_factor; sig[l] = l < P->n_levels ? sf * sf : 1.0f; }
    memcpy(u_chas.host(h), cur->has_map_line, (size_t)n1);
    if (!fr) { memcpy(u_ckl.host(h), cur->kl, (size_t)n1 * sizeof(hvo_keyline)); memcpy(u_cfn.host(h), cur->linefn, (size_t)n1 * 24); memcpy(u_cds.host(h), cur->desc, (size_t)n1 * 32); }
    for (int j = 0; j < n_kf; j++) {
        const hvo_nl_keyframe &K = kf[j];
        const size_t n = (size_t)K.n;
        if (!n) continue;
        memcpy(u_kl.host(h, j), K.kl, n * sizeof(hvo_keyline)); memcpy(u_fn.host(h, j), K.linefn, n * 24);
        memcpy(u_ds.host(h, j), K.desc, n * 32); memcpy(u_has.host(h, j), K.has_map_line, n);
    }
    if ((rc = sc.up(0, up_end)) || (rc = sc.clear(z0, z1)) || (rc = sc.clear(z1, m1, 0xFF))) return rc;
    sc.tick();
    NlDev a; memset(&a, 0, sizeof(a));
    const uint8_t *c_desc;
    if (fr) { a.c_kl = fr->kl; a.c_fn = fr->fn; c_desc = fr->ldesc; }
    else { a.c_kl = u_ckl.dev(d); a.c_fn = u_cfn.dev(d); c_desc = u_cds.dev(d); }
    a.c_has = u_chas.dev(d); a.n1 = n1;
    a.kf = u_kf.dev(d); a.n_kf = n_kf; a.k_kl = u_kl.dev(d); a.k_fn = u_fn.dev(d); a.k_has = u_has.dev(d);
    a.pairs = u_pr.dev(d); a.M = r_M.dev(d); a.sig = u_sig.dev(d);
    a.cq = (int)cq; a.ct = (int)ct; a.n_pairs = (int)NP; a.nb = (int)nb; a.n_levels = P->n_levels;
    a.outcome = r_out.dev(d); a.line3d = r_x.dev(d); a.owner = r_own.dev(d); a.pass = s_pass.dev(d); a.blockcnt = s_bc.dev(d); a.ncreated = r_cnt.dev(d);
    a.c0 = r_c0.dev(d); a.c1 = r_c1.dev(d); a.c2 = r_c2.dev(d);
    // the searches, back to back (one scratch: the stream keeps them in order)
    for (int j : S) {
        if (match_lines_enqueue(st, c_desc, n1, u_ds.dev(d, j), kf[j].n, (float)P->th_high, P->nn_ratio, 2, s_ml.dev(d), r_M.dev(d, j), r_nm.dev(d) + j)) { *err = "create new map lines: search launch"; return HVO_ERR_HIP; }
        hipLaunchKernelGGL(k_nl_occupancy, dim3(1), dim3(256), 0, st, r_M.dev(d, j), n1, (int)kf[j].n, u_chas.dev(d), u_has.dev(d, j), r_nm.dev(d) + j);
    }
    sc.tick();
    hipLaunchKernelGGL(k_nl_triangulate, dim3((unsigned)nb, (unsigned)NP), dim3(NL_BLOCK), 0, st, a);
    sc.tick();
    hipLaunchKernelGGL(k_nl_resolve, dim3((unsigned)nb), dim3(NL_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_nl_compact, dim3((unsigned)nb, (unsigned)NP), dim3(NL_BLOCK), 0, st, a);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    for (int i = 0; i < 3; i++) sum->kernel_ms[i] = sc.ms[i];
    const size_t n = (size_t)n1;
    for (int j = 0; j < n_kf; j++) { mt[j].n_matched = r_nm.down(b)[j]; mt[j].gate = gate[j]; memcpy(mt[j].match_idx, r_M.down(b, j), n * 4); }
    int n_new = 0;
    for (size_t p = 0; p < NP; p++) {
        hvo_nl_result &R = res[p];
        R.kf2 = hp[p].kf2; R.kf3 = hp[p].kf3; R.mv2 = hp[p].mv2; R.mv3 = hp[p].mv3;
        R.n_created = r_cnt.down(b)[p]; R.status = HVO_OK;
        n_new += R.n_created;
        memcpy(R.outcome, r_out.down(b, p), n);
        if (R.line3d) memcpy(R.line3d, r_x.down(b, p), n * 24);
        const size_t nc = (size_t)std::max(0, std::min(R.n_created, (int32_t)n));
        if (R.created_idx0) memcpy(R.created_idx0, r_c0.down(b, p), nc * 4);
        if (R.created_idx1) memcpy(R.created_idx1, r_c1.down(b, p), nc * 4);
        if (R.created_idx2) memcpy(R.created_idx2, r_c2.down(b, p), nc * 4);
    }
    if (sum->owner_pair) memcpy(sum->owner_pair, r_own.down(b), n * 4);
    sum->n_new = n_new;
    return HVO_OK;
}

extern "C" {

int hvo_create_new_map_lines(hvo_ctx *ctx, const hvo_nl_params *params, const hvo_nl_keyframe *current, int n_kf, const hvo_nl_keyframe *neighbours,
                             hvo_nl_match *matches, int n_pairs_cap, hvo_nl_result *results, hvo_nl_summary *summary)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!params || !current || !summary) { ctx->last_error = "create new map lines: a null argument"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return nl_run(ctx, ctx->stream, params, current, nullptr, n_kf, neighbours, matches, n_pairs_cap, results, summary, &ctx->last_error);
}

int hvo_stream_create_new_map_lines(hvo_stream *s, int64_t cur, const hvo_camera *cam, const hvo_nl_params *params, const float Tcw[12],
                                    const uint8_t *has_map_line, int n_kf, const hvo_nl_keyframe *neighbours, hvo_nl_match *matches, int n_pairs_cap,
                                    hvo_nl_result *results, hvo_nl_summary *summary)
{
    if (!s) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !Tcw || !summary) { s->last_error = "create new map lines: a null argument"; return HVO_ERR_INVALID_ARG; }
    FrameView V; int rc;
    if ((rc = stream_view(s, cur, need_new_lines, s->s_match, V))) return rc;
    hvo_nl_keyframe K; memset(&K, 0, sizeof(K));
    memcpy(K.Tcw, Tcw, sizeof(K.Tcw)); K.has_map_line = has_map_line; K.cam = *cam; K.n = V.n_kl;
    return nl_run(V.ctx, s->s_match, params, &K, &V, n_kf, neighbours, matches, n_pairs_cap, results, summary, &s->last_error);
}

}   // extern "C"
