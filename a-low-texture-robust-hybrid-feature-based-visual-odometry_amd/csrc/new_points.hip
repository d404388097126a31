// new_points.hip -- LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:335-580) for all neighbour key frames in one call with
// one synchronisation.  With it: LocalMapping::ComputeF12 (:1779-1796), ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:668-836),
// ORBmatcher::CheckDistEpipolarLine (:143-160) and KeyFrame::UnprojectStereo (src/KeyFrame.cc:785-801).
//
// Why one launch sequence serves the whole loop.  (1) SearchForTriangulation allocates vbMatched2 and tests it but never sets it: the match
// of feature idx1 does not depend on any other feature's match.  (2) CreateNewMapPoints builds ORBmatcher(0.6, false) and passes
// bOnlyStereo = false: no rotation histogram, no stereo filter.  (3) The only thing a neighbour's pass writes that a later pass reads is
// mpCurrentKeyFrame->AddMapPoint(pMP, idx1): later neighbours skip idx1.  So the point at idx1 is created by the FIRST neighbour in list
// order whose match for idx1 passes every gate under the INITIAL occupancy; every (neighbour, idx1) pair is evaluated independently and one
// small pass resolves the chain.  A caller that leaves after neighbour i uses a prefix of the list; a prefix does not depend on what follows.
//
//   k_bow_csr        (bow.hip) the CSR of (node, feature index) per neighbour, rows ascending in node, a row ascending in index: the
//                    order of DBoW2's FeatureVector
//   k_np_search      16 lanes (a quarter wave) per (neighbour, idx1), four pairs per wave: the neighbour's row of node_id[idx1] by
//                    bisection, the row walked in ascending position with idx1's descriptor in registers (4 x u64).  A candidate takes
//                    part when it has no map point, dist <= th_low, the epipole test does not exclude it (both features monocular only)
//                    and CheckDistEpipolarLine holds.  The reference moves bestDist only on acceptance and refuses `dist > bestDist`, so
//                    its result is the smallest distance among these candidates with the LAST of equal distances in visiting order: the
//                    group minimum of  dist << 16 | (0xFFFF - CSR position).
//   k_np_triangulate one lane per (neighbour, idx1): the parallax test, the branch (linear triangulation / UnprojectStereo of either
//                    side), the two depth signs, the two chi-square tests, the scale consistency; outcome = the first `continue` met.
//                    The 4 x 4 solve keeps A and V in registers: every loop over them unrolls, no private array takes a run-time index.
//   k_np_resolve     per idx1 the first neighbour with outcome CREATED is the owner
//   k_np_compact     per neighbour the list {idx1 : owner == neighbour} in ascending idx1 (sm_compact_pos).  Integer atomics only count.
//
// Readings (OpenCV is not in the reference tree; tests/new_points_ref.py restates the same and is the definition).
// Only + - * / sqrt in the written order, no contraction (-ffp-contract=off for device AND host code of this file).
//   dot3f(a, b)           ((a0 b0 + a1 b1) + a2 b2) in float: the element of a 3 x 3 product without addend
//   R p + t               sm_row: dot3f, then (float)((double)sum * 1.0 + (double)t * 1.0)
//   Ow                    -Rcw^T tcw: double sums times -1.0 rounded to float (as fuse.hip)
//   cv::norm              sqrt of the double sum of squares ((d0^2 + d1^2) + d2^2); stored to float where the text stores it to a float
//   Mat::dot              the double sum in order
//   per neighbour (host)  baseline = (float)norm(Ow2 - Ow1), the difference in float; gate: skip, then baseline < mb.  R12 = R1w R2w^T by
//                         dot3f; t12 = sm_row(-R12 row, t2w, t1w); K^T.inv() and K.inv() by OpenCV's closed 3 x 3 form (cofactors and
//                         determinant in double from the float entries, each entry (float)(cofactor * (1 / det))); the product
//                         ((K1^T.inv() t12x) R12) K2.inv() left to right by dot3f.  Epipole: C2 = sm_row(R2w, Ow1, t2w), invz = 1.0f / C2z,
//                         ex = fx * C2x * invz + cx left to right in float
//   epipolar line         a = (x1 F00 + y1 F10) + F20 in float, b, c alike; num = (a x2 + b y2) + c; den = a a + b b; den == 0 fails;
//                         dsqr = num * num / den in float, compared as a double with the double product 3.84 * sigma2[octave2]
//   epipole test          dx = ex - x2, dy = ey - y2; dx dx + dy dy < 100.0f * mvScaleFactors[octave2] (a float) excludes the candidate
//   octaves               a feature whose octave is outside [0, n_levels) is refused for the pair: as idx1 it has no match, as idx2 it is
//                         no candidate (the reference would read mvLevelSigma2[-1])
//   xn                    ((x - cx) * invfx, (y - cy) * invfy, 1), invfx = 1.0f / fx; ray = Rwc xn by dot3f over the columns of Rcw
//   cosParallaxRays       (float)(dot / (norm1 * norm2)), all three in double as the expression is written
//   stereo parallax       cos(2 atan2(mb / 2, d)) = (d d - h h) / (d d + h h) with h = mb / 2, in double, rounded to float: no libm call.
//                         bStereo1 decides first (if / else if); cosParallaxStereo = min(s1, s2) as std::min: s2 < s1 ? s2 : s1
//   rows of A             each element one float product then one float subtraction: xn.x * T[2][k] - T[0][k]
//   cv::SVD::compute      one-sided (Hestenes) Jacobi on the columns of the 4 x 4 A: the float entries of A are taken to double once, the
//                         working columns and V stay in DOUBLE, the three column sums of a pair and the rotation (pnp_core.inc's pnp_rot) are
//                         double; pairs in row-major order, exactly 12 sweeps, no data-dependent exit; the column of V whose column of A has
//                         the smallest squared norm, the highest index among equals, rounded to float ONCE (vt is CV_32F).  Working columns
//                         stored in float between rotations were measured first: 52 times the error of numpy.linalg.svd on the float32 A for the planted
//                         pairs of tests/test_new_points.py, against the 4 times the accuracy check allows (DESIGN.md section 7 has the
//                         figures); every rotation then rounds A again.  x3D = V_k * (1.0 / V_3) in double rounded to float (Mat / scalar
//                         scales by the reciprocal).  NOT CLAIMED: bit parity with an OpenCV binary.
//   UnprojectStereo       z = mvDepth (z > 0, else NO_DEPTH), x = (u - cx) * z * invfx left to right on the DISTORTED mvKeys,
//                         sm_row(column of Rcw, (x, y, z), Ow)
//   z1, x1, y1            (float)(Mat::dot(row, x3D) + (double)t); z <= 0 fails, a NaN passes on; invz = (float)(1.0 / (double)z)
//   reprojection          u = fx * x * invz + cx left to right; u_r = u - bf * invz with the CURRENT key frame's bf for both sides; the float
//                         sum of squares against the double products 5.991 * sigma2 / 7.8 * sigma2
//   scale                 dist = (float)norm(x3D - Ow); ratioDist = dist2 / dist1; ratioOctave = sf[o1] / sf[o2]; ratioFactor = 1.5f * scale_factor
#include "slot_map.hpp"
#include "frame_view.hpp"
#include "staged_call.hpp"
#include <math.h>
#include <string.h>
#include <string>
#include <vector>

#define NP_BLOCK SM_BLOCK
#define NP_GROUP 16
#define NP_MAXN HVO_BOW_MAXN      // features per side (k_bow_csr's sort keys live in LDS)
#define NP_MAXKF 64               // neighbours per call
#define NP_NOKEY 0xFFFFFFFFu

#include "triangulate4.inc"                 // np_dot3f .. np_normd, np_rot, np_svd4 (NP_SWEEPS), np_inv3, np_mul3

struct NpKf { float R[9], t[3], Ow[3], F[9], ex, ey, mb; int n, gate, stereo; };
struct NpDev {
    // the current key frame
    const hvo_keypoint *c_kpun, *c_kp; const float *c_ur, *c_depth; const uint8_t *c_desc, *c_has; const int *c_node;
    int n1; float R[9], t[3], Ow[3], mb1;
    // the neighbours: neighbour j's arrays at base + j * ct (its CSR starts at fv_start + j * (ct + 1))
    const NpKf *kf; const hvo_keypoint *k_kpun, *k_kp; const float *k_ur, *k_depth; const uint8_t *k_desc, *k_has;
    const int *fv_node, *fv_start, *fv_idx, *n_rows;
    int cq, ct, n_kf, nb, n_levels, th_low;
    float fx, fy, cx, cy, invfx, invfy, bf, ratio_factor; const float *tab;     // tab: mvScaleFactors[16] then mvLevelSigma2[16]
    int32_t *midx, *mdist; int8_t *outcome, *branch; float *x3d; int32_t *owner; uint8_t *pass; int *blockcnt, *ncreated; int32_t *c1, *c2;
};

__global__ __launch_bounds__(NP_BLOCK) void k_np_search(NpDev a)
{
    const int j = blockIdx.y, sub = threadIdx.x & (NP_GROUP - 1);
    const int i = blockIdx.x * (NP_BLOCK / NP_GROUP) + (threadIdx.x / NP_GROUP);
    if (i >= a.n1) return;                                           // (a whole group leaves together: the shuffles below stay inside a group)
    const NpKf &k = a.kf[j];
    const size_t o = (size_t)j * a.cq + (size_t)i;
    const hvo_keypoint p1 = a.c_kpun[i];
    const int node = a.c_node[i];
    unsigned best = NP_NOKEY;
    const int *kidx = a.fv_idx + (size_t)j * a.ct;
    if (k.gate == 0 && k.n > 0 && !a.c_has[i] && node >= 0 && p1.octave >= 0 && p1.octave < a.n_levels) {
        // CheckDistEpipolarLine's line of idx1 (ORBmatcher.cc:146-152)
        const float la = __fadd_rn(__fadd_rn(__fmul_rn(p1.x, k.F[0]), __fmul_rn(p1.y, k.F[3])), k.F[6]);
        const float lb = __fadd_rn(__fadd_rn(__fmul_rn(p1.x, k.F[1]), __fmul_rn(p1.y, k.F[4])), k.F[7]);
        const float lc = __fadd_rn(__fadd_rn(__fmul_rn(p1.x, k.F[2]), __fmul_rn(p1.y, k.F[5])), k.F[8]);
        const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
        const int *rnode = a.fv_node + (size_t)j * a.ct, *rstart = a.fv_start + (size_t)j * (a.ct + 1);
        const int nr = a.n_rows[j];
        int lo = 0, hi = nr;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (rnode[m] < node) lo = m + 1; else hi = m; }
        if (!(den == 0.f) && lo < nr && rnode[lo] == node) {
            const bool mono1 = !(a.c_ur && a.c_ur[i] >= 0.f);
            const ulonglong4 qd = ld256(a.c_desc + (size_t)i * 32);
            const hvo_keypoint *kp2 = a.k_kpun + (size_t)j * a.ct; const float *ur2 = a.k_ur + (size_t)j * a.ct;
            const uint8_t *has2 = a.k_has + (size_t)j * a.ct, *desc2 = a.k_desc + (size_t)j * a.ct * 32;
            const float *sf = a.tab, *sig = a.tab + HVO_MAX_LEVELS;
            const int p0 = rstart[lo], pe = rstart[lo + 1];
            for (int p = p0 + sub; p < pe; p += NP_GROUP) {
                const int i2 = kidx[p];
                if (has2[i2]) continue;                                  // ORBmatcher.cc:736 (vbMatched2 is never set)
                const int dist = ham256(qd, ld256(desc2 + (size_t)i2 * 32));
                if (dist > a.th_low) continue;                           // :751
                const float x2 = kp2[i2].x, y2 = kp2[i2].y; const int o2 = kp2[i2].octave;
                if (o2 < 0 || o2 >= a.n_levels) continue;
                if (mono1 && !(k.stereo && ur2[i2] >= 0.f)) {            // :756-762
                    const float dx = __fsub_rn(k.ex, x2), dy = __fsub_rn(k.ey, y2);
                    if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.0f, sf[o2])) continue;
                }
                const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, x2), __fmul_rn(lb, y2)), lc);
                const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
                if (!((double)dsqr < __dmul_rn(3.84, (double)sig[o2]))) continue;      // :159
                const unsigned key = ((unsigned)dist << 16) | (0xFFFFu - (unsigned)p);
                best = key < best ? key : best;
            }
        }
    }
    for (int w = NP_GROUP / 2; w > 0; w >>= 1) { const unsigned other = (unsigned)__shfl_xor((int)best, w); best = other < best ? other : best; }
    if (sub == 0) {
        const bool hit = best != NP_NOKEY;
        a.midx[o] = hit ? kidx[0xFFFFu - (best & 0xFFFFu)] : -1;
        a.mdist[o] = hit ? (int)(best >> 16) : 256;
    }
}

// cos(2 atan2(mb / 2, d)) without libm
static __host__ __device__ __forceinline__ float np_stereo_cos(float mb, float depth)
{
    const double h = (double)(mb / 2), d = (double)depth;
    const double dd = d * d, hh = h * h;
    return (float)((dd - hh) / (dd + hh));
}

// one side's chi-square test (LocalMapping.cc:492-543): true = the pair is refused
static __host__ __device__ __forceinline__ bool np_reproj_fails(const float *R, const float *t, float X, float Y, float Z, float z, float fx, float fy, float cx, float cy,
                                                                float bf, float kx, float ky, float kur, bool stereo, float sigma2)
{
    const float x = (float)(np_dotd(R[0], R[1], R[2], X, Y, Z) + (double)t[0]), y = (float)(np_dotd(R[3], R[4], R[5], X, Y, Z) + (double)t[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = fx * x * invz + cx, v = fy * y * invz + cy;
    const float ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float ur = u - bf * invz;
    const float er = ur - kur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

__global__ __launch_bounds__(NP_BLOCK) void k_np_triangulate(NpDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * NP_BLOCK + threadIdx.x;
    if (i >= a.n1) return;
    const NpKf &k = a.kf[j];
    const size_t o = (size_t)j * a.cq + (size_t)i;
    int out = HVO_NP_NO_MATCH, br = 0;
    float X = 0.f, Y = 0.f, Z = 0.f;
    const int i2 = a.midx[o];
    if (a.c_has[i]) out = HVO_NP_OCCUPIED;
    else if (i2 >= 0) {
        const size_t o2 = (size_t)j * a.ct + (size_t)i2;
        const hvo_keypoint p1 = a.c_kpun[i], p2 = a.k_kpun[o2];
        const float ur1 = a.c_ur ? a.c_ur[i] : -1.0f, ur2 = k.stereo ? a.k_ur[o2] : -1.0f;
        const bool st1 = ur1 >= 0.f, st2 = ur2 >= 0.f;
        const float *sf = a.tab, *sig = a.tab + HVO_MAX_LEVELS;
        // the rays and their parallax (:430-446)
        const float x1n = (p1.x - a.cx) * a.invfx, y1n = (p1.y - a.cy) * a.invfy, x2n = (p2.x - a.cx) * a.invfx, y2n = (p2.y - a.cy) * a.invfy;
        const float r10 = np_dot3f(a.R[0], a.R[3], a.R[6], x1n, y1n, 1.0f), r11 = np_dot3f(a.R[1], a.R[4], a.R[7], x1n, y1n, 1.0f), r12 = np_dot3f(a.R[2], a.R[5], a.R[8], x1n, y1n, 1.0f);
        const float r20 = np_dot3f(k.R[0], k.R[3], k.R[6], x2n, y2n, 1.0f), r21 = np_dot3f(k.R[1], k.R[4], k.R[7], x2n, y2n, 1.0f), r22 = np_dot3f(k.R[2], k.R[5], k.R[8], x2n, y2n, 1.0f);
        const float cosr = (float)(np_dotd(r10, r11, r12, r20, r21, r22) / (np_normd(r10, r11, r12) * np_normd(r20, r21, r22)));
        const float cs = cosr + 1.0f;
        float s1 = cs, s2 = cs;
        if (st1) s1 = np_stereo_cos(a.mb1, a.c_depth[i]);
        else if (st2) s2 = np_stereo_cos(k.mb, a.k_depth[o2]);
        const float cst = s2 < s1 ? s2 : s1;
        bool have = false;
        if (cosr < cst && cosr > 0.f && (st1 || st2 || (double)cosr < 0.9998)) {
            br = 1;
            float W[4][4], x[4];
            const float T1[3][4] = { { a.R[0], a.R[1], a.R[2], a.t[0] }, { a.R[3], a.R[4], a.R[5], a.t[1] }, { a.R[6], a.R[7], a.R[8], a.t[2] } };
            const float T2[3][4] = { { k.R[0], k.R[1], k.R[2], k.t[0] }, { k.R[3], k.R[4], k.R[5], k.t[1] }, { k.R[6], k.R[7], k.R[8], k.t[2] } };
#pragma unroll
            for (int c = 0; c < 4; c++) {
                W[0][c] = x1n * T1[2][c] - T1[0][c]; W[1][c] = y1n * T1[2][c] - T1[1][c];
                W[2][c] = x2n * T2[2][c] - T2[0][c]; W[3][c] = y2n * T2[2][c] - T2[1][c];
            }
            np_svd4(W, x);
            if (x[3] == 0.f) out = HVO_NP_W_ZERO;
            else {
                const double iw = 1.0 / (double)x[3];
                X = (float)((double)x[0] * iw); Y = (float)((double)x[1] * iw); Z = (float)((double)x[2] * iw);
                have = true;
            }
        } else if ((st1 && s1 < s2) || (st2 && s2 < s1)) {
            const bool first = st1 && s1 < s2;
            br = first ? 2 : 3;
            const float z = first ? a.c_depth[i] : a.k_depth[o2];
            if (!(z > 0.f)) out = HVO_NP_NO_DEPTH;
            else {
                const hvo_keypoint pr = first ? a.c_kp[i] : a.k_kp[o2];
                const float *R = first ? a.R : k.R, *Ow = first ? a.Ow : k.Ow;
                const float xc = (pr.x - a.cx) * z * a.invfx, yc = (pr.y - a.cy) * z * a.invfy;
                X = np_row(R[0], R[3], R[6], xc, yc, z, Ow[0]); Y = np_row(R[1], R[4], R[7], xc, yc, z, Ow[1]); Z = np_row(R[2], R[5], R[8], xc, yc, z, Ow[2]);
                have = true;
            }
        } else out = HVO_NP_LOW_PARALLAX;
        if (have) {
            const float z1 = (float)(np_dotd(a.R[6], a.R[7], a.R[8], X, Y, Z) + (double)a.t[2]);
            const float z2 = (float)(np_dotd(k.R[6], k.R[7], k.R[8], X, Y, Z) + (double)k.t[2]);
            if (z1 <= 0.f) out = HVO_NP_BEHIND_1;
            else if (z2 <= 0.f) out = HVO_NP_BEHIND_2;
            else if (np_reproj_fails(a.R, a.t, X, Y, Z, z1, a.fx, a.fy, a.cx, a.cy, a.bf, p1.x, p1.y, ur1, st1, sig[p1.octave])) out = HVO_NP_REPROJ_1;
            else if (np_reproj_fails(k.R, k.t, X, Y, Z, z2, a.fx, a.fy, a.cx, a.cy, a.bf, p2.x, p2.y, ur2, st2, sig[p2.octave])) out = HVO_NP_REPROJ_2;
            else {
                const float d1 = (float)np_normd(X - a.Ow[0], Y - a.Ow[1], Z - a.Ow[2]), d2 = (float)np_normd(X - k.Ow[0], Y - k.Ow[1], Z - k.Ow[2]);
                if (d1 == 0.f || d2 == 0.f) out = HVO_NP_ZERO_DIST;
                else {
                    const float rd = d2 / d1, ro = sf[p1.octave] / sf[p2.octave];
                    out = (rd * a.ratio_factor < ro || rd > ro * a.ratio_factor) ? HVO_NP_SCALE : HVO_NP_CREATED;
                }
            }
        }
    }
    a.outcome[o] = (int8_t)out; a.branch[o] = (int8_t)br;
    a.x3d[3 * o] = X; a.x3d[3 * o + 1] = Y; a.x3d[3 * o + 2] = Z;
}

__global__ __launch_bounds__(NP_BLOCK) void k_np_resolve(NpDev a)
{
    const int i = blockIdx.x * NP_BLOCK + threadIdx.x;
    if (i >= a.n1) return;
    int own = -1;
    for (int j = a.n_kf - 1; j >= 0; j--) if (a.outcome[(size_t)j * a.cq + i] == HVO_NP_CREATED) own = j;       // the first in list order
    a.owner[i] = own;
    if (own >= 0) { a.pass[(size_t)own * a.cq + i] = 1; atomicAdd(&a.blockcnt[(size_t)own * a.nb + blockIdx.x], 1); }
}

__global__ __launch_bounds__(NP_BLOCK) void k_np_compact(NpDev a)
{
    const int j = blockIdx.y, i = blockIdx.x * NP_BLOCK + threadIdx.x;
    bool p;
    const int at = sm_compact_pos(a.blockcnt, a.nb, a.cq, j, a.pass, a.ncreated, &p);
    if (p) { const size_t q0 = (size_t)j * a.cq; a.c1[q0 + at] = i; a.c2[q0 + at] = a.midx[q0 + i]; }
}

// Ow2, the baseline gate, ComputeF12 and the epipole of one neighbour (about 60 float operations; the restatement fixes the bits)
static void np_neighbour(const hvo_camera *cam, const float *R1, const float *t1, const float *Ow1, const hvo_np_keyframe &K, NpKf &c)
{
    pose_split(K.Tcw, c.R, c.t, c.Ow);
    c.mb = K.mb; c.n = K.n; c.stereo = (K.uright && K.depth) ? 1 : 0;
    const float baseline = (float)np_normd(c.Ow[0] - Ow1[0], c.Ow[1] - Ow1[1], c.Ow[2] - Ow1[2]);
    c.gate = K.skip ? HVO_NP_GATE_SKIP : (baseline < K.mb ? HVO_NP_GATE_BASELINE : HVO_NP_GATE_SEARCHED);
    float R12[9], t12[3];
    for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) R12[3 * r + q] = np_dot3f(R1[3 * r], R1[3 * r + 1], R1[3 * r + 2], c.R[3 * q], c.R[3 * q + 1], c.R[3 * q + 2]);
    for (int r = 0; r < 3; r++) t12[r] = np_row(-R12[3 * r], -R12[3 * r + 1], -R12[3 * r + 2], c.t[0], c.t[1], c.t[2], t1[r]);
    const float tx[9] = { 0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f };
    const float Kt[9] = { cam->fx, 0.f, 0.f, 0.f, cam->fy, 0.f, cam->cx, cam->cy, 1.f }, Km[9] = { cam->fx, 0.f, cam->cx, 0.f, cam->fy, cam->cy, 0.f, 0.f, 1.f };
    float Kti[9], Ki[9], M1[9], M2[9];
    np_inv3(Kt, Kti); np_inv3(Km, Ki);
    np_mul3(Kti, tx, M1); np_mul3(M1, R12, M2); np_mul3(M2, Ki, c.F);
    const float C0 = np_row(c.R[0], c.R[1], c.R[2], Ow1[0], Ow1[1], Ow1[2], c.t[0]), C1 = np_row(c.R[3], c.R[4], c.R[5], Ow1[0], Ow1[1], Ow1[2], c.t[1]),
                C2 = np_row(c.R[6], c.R[7], c.R[8], Ow1[0], Ow1[1], Ow1[2], c.t[2]);
    const float invz = 1.0f / C2;
    c.ex = cam->fx * C0 * invz + cam->cx; c.ey = cam->fy * C1 * invz + cam->cy;
}

static bool np_side_ok(const hvo_np_keyframe &K)
{
    if (K.n < 0) return false;
    if (K.n > 0 && (!K.kp_un || !K.desc || !K.node_id || !K.has_map_point)) return false;
    return (K.uright == nullptr) == (K.depth == nullptr);
}

// fr null: cur's host arrays go up; else the current key frame is the resident frame (its node ids at d_node) and cur carries Tcw, mb and
// has_map_point only
static int np_run(hvo_ctx *ctx, hipStream_t st, const hvo_camera *cam, const hvo_np_params *P, const hvo_np_keyframe *cur, const FrameView *fr, const int *d_node,
                  int n_kf, const hvo_np_keyframe *kf, hvo_np_result *res, hvo_np_summary *sum, std::string *err)
{
    const int n1 = fr ? fr->n_kp : cur->n;
    // ---- refusals: whole, before anything is written ----
    if (P->th_low > 255) { *err = "create new map points: th_low above 255 (a distance is at most 256)"; return HVO_ERR_INVALID_ARG; }
    if (P->n_levels < 1 || P->n_levels > HVO_MAX_LEVELS) { *err = "create new map points: n_levels outside 1 .. 16"; return HVO_ERR_INVALID_ARG; }
    if (n_kf < 0 || (n_kf > 0 && (!kf || !res))) { *err = "create new map points: n_kf < 0 or no neighbours / results"; return HVO_ERR_INVALID_ARG; }
    if (fr ? (n1 > 0 && !cur->has_map_point) : !np_side_ok(*cur)) { *err = "create new map points: the current key frame has n < 0 or lacks an array (uright and depth come together)"; return HVO_ERR_INVALID_ARG; }
    if (n_kf > NP_MAXKF) { *err = "create new map points: " + std::to_string(n_kf) + " neighbours (limit " + std::to_string(NP_MAXKF) + "); nothing was written"; return HVO_ERR_UNSUPPORTED; }
    int tmax = 0;
    for (int j = 0; j < n_kf; j++) {
        if (!np_side_ok(kf[j])) { *err = "create new map points: neighbour " + std::to_string(j) + " has n < 0 or lacks an array (uright and depth come together)"; return HVO_ERR_INVALID_ARG; }
        if (n1 > 0 && !res[j].match_idx2) { *err = "create new map points: a result without match_idx2"; return HVO_ERR_INVALID_ARG; }
        tmax = std::max(tmax, (int)kf[j].n);
    }
    if (n1 > NP_MAXN || tmax > NP_MAXN) {
        *err = "create new map points: " + std::to_string(std::max(n1, tmax)) + " features on one side (limit " + std::to_string(NP_MAXN) + "); nothing was written";
        return HVO_ERR_UNSUPPORTED;
    }
    const size_t F = (size_t)n_kf;
    std::vector<NpKf> hk(F);
    float R1[9], t1[3], Ow1[3];
    pose_split(cur->Tcw, R1, t1, Ow1);
    for (int j = 0; j < n_kf; j++) np_neighbour(cam, R1, t1, Ow1, kf[j], hk[j]);
    sum->n_new = 0; for (int q = 0; q < 3; q++) sum->kernel_ms[q] = 0.f;
    if (n1 == 0 || n_kf == 0) {
        for (int j = 0; j < n_kf; j++) { res[j].n_created = 0; res[j].gate = hk[j].gate; res[j].status = HVO_OK; }
        if (n_kf == 0 && sum->owner) for (int i = 0; i < n1; i++) sum->owner[i] = -1;
        return HVO_OK;
    }
    // ---- one carve of the context's arena: what goes up, the rows, the scratch, what comes down ----
    const size_t cq = (size_t)((n1 + NP_BLOCK - 1) / NP_BLOCK * NP_BLOCK), ct = (size_t)std::max(64, (tmax + 63) & ~63), nb = cq / NP_BLOCK;
    const bool c_raw = !fr && cur->kp, c_st = !fr && cur->uright;
    bool k_raw = false;
    for (int j = 0; j < n_kf; j++) k_raw = k_raw || kf[j].kp;
    StageCarver C(256);
    const auto u_kf = C.take<NpKf>(F); const auto u_tab = C.take<float>(2 * HVO_MAX_LEVELS); const auto u_n = C.take<int>(F); const auto u_chas = C.take<uint8_t>(cq);
    const auto u_ckp = C.take<hvo_keypoint>(fr ? 0 : cq), u_ckr = C.take<hvo_keypoint>(c_raw ? cq : 0);
    const auto u_cur = C.take<float>(c_st ? cq : 0), u_cdp = C.take<float>(c_st ? cq : 0);
    const auto u_cds = C.take<uint8_t>(fr ? 0 : cq * 32); const auto u_cnd = C.take<int>(fr ? 0 : cq);
    const auto u_kp = C.take<hvo_keypoint>(F, ct), u_kr = C.take<hvo_keypoint>(k_raw ? F : 0, ct);
    const auto u_ur = C.take<float>(F, ct), u_dp = C.take<float>(F, ct);
    const auto u_ds = C.take<uint8_t>(F, ct * 32); const auto u_nd = C.take<int>(F, ct); const auto u_has = C.take<uint8_t>(F, ct);
    const size_t up_end = C.mark();
    const auto g_node = C.take<int>(F, ct), g_start = C.take<int>(F, ct + 1), g_idx = C.take<int>(F, ct), g_rows = C.take<int>(F);
    const size_t z0 = C.mark();                                      // [z0, z1) is zeroed
    const auto s_pass = C.take<uint8_t>(F, cq); const auto s_bc = C.take<int>(F, nb);
    const size_t r0 = C.mark();                                      // [r0, r1) comes down; its head belongs to the zeroed range
    const auto r_cnt = C.take<int>(F);
    const size_t z1 = C.mark();
    const auto r_mi = C.take<int32_t>(F, cq), r_md = C.take<int32_t>(F, cq);
    const auto r_out = C.take<int8_t>(F, cq), r_br = C.take<int8_t>(F, cq); const auto r_x = C.take<float>(F, cq * 3);
    const auto r_c1 = C.take<int32_t>(F, cq), r_c2 = C.take<int32_t>(F, cq), r_own = C.take<int32_t>(cq);
    const size_t r1 = C.mark();
    StagedCall sc(ctx, st, "create new map points: ", err); int rc;
    if ((rc = sc.begin(C.mark(), up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    memcpy(u_kf.host(h), hk.data(), F * sizeof(NpKf));
    float *tab = u_tab.host(h);
    const hvo_ctx *tc = fr ? fr->ctx : ctx;
    for (int l = 0; l < HVO_MAX_LEVELS; l++) tab[l] = fr ? fr->sf[l] : ctx->scale[l];
    frame_level_sigma2(tc, tab + HVO_MAX_LEVELS, nullptr);
    memcpy(u_chas.host(h), cur->has_map_point, (size_t)n1);
    if (!fr) {
        memcpy(u_ckp.host(h), cur->kp_un, (size_t)n1 * sizeof(hvo_keypoint)); memcpy(u_cds.host(h), cur->desc, (size_t)n1 * 32); memcpy(u_cnd.host(h), cur->node_id, (size_t)n1 * 4);
        if (c_raw) memcpy(u_ckr.host(h), cur->kp, (size_t)n1 * sizeof(hvo_keypoint));
        if (c_st) { memcpy(u_cur.host(h), cur->uright, (size_t)n1 * 4); memcpy(u_cdp.host(h), cur->depth, (size_t)n1 * 4); }
    }
    for (int j = 0; j < n_kf; j++) {
        const hvo_np_keyframe &K = kf[j];
        const size_t n = (size_t)K.n;
        u_n.host(h)[j] = K.n;
        if (!n) continue;
        memcpy(u_kp.host(h, j), K.kp_un, n * sizeof(hvo_keypoint));
        if (k_raw) memcpy(u_kr.host(h, j), K.kp ? K.kp : K.kp_un, n * sizeof(hvo_keypoint));
        if (K.uright) { memcpy(u_ur.host(h, j), K.uright, n * 4); memcpy(u_dp.host(h, j), K.depth, n * 4); }
        memcpy(u_ds.host(h, j), K.desc, n * 32); memcpy(u_nd.host(h, j), K.node_id, n * 4); memcpy(u_has.host(h, j), K.has_map_point, n);
    }
    if ((rc = sc.up(0, up_end)) || (rc = sc.clear(z0, z1))) return rc;
    sc.tick();
    NpDev a; memset(&a, 0, sizeof(a));
    if (fr) { a.c_kpun = fr->kp_un; a.c_kp = fr->kp; a.c_ur = fr->uright; a.c_depth = fr->zdepth; a.c_desc = fr->desc; a.c_node = d_node; }
    else {
        a.c_kpun = u_ckp.dev(d); a.c_kp = c_raw ? u_ckr.dev(d) : a.c_kpun;
        a.c_ur = c_st ? u_cur.dev(d) : nullptr; a.c_depth = c_st ? u_cdp.dev(d) : nullptr;
        a.c_desc = u_cds.dev(d); a.c_node = u_cnd.dev(d);
    }
    a.c_has = u_chas.dev(d); a.n1 = n1; a.mb1 = cur->mb;
    memcpy(a.R, R1, sizeof(R1)); memcpy(a.t, t1, sizeof(t1)); memcpy(a.Ow, Ow1, sizeof(Ow1));
    a.kf = u_kf.dev(d); a.k_kpun = u_kp.dev(d); a.k_kp = k_raw ? u_kr.dev(d) : a.k_kpun;
    a.k_ur = u_ur.dev(d); a.k_depth = u_dp.dev(d); a.k_desc = u_ds.dev(d); a.k_has = u_has.dev(d);
    a.fv_node = g_node.dev(d); a.fv_start = g_start.dev(d); a.fv_idx = g_idx.dev(d); a.n_rows = g_rows.dev(d);
    a.cq = (int)cq; a.ct = (int)ct; a.n_kf = n_kf; a.nb = (int)nb; a.n_levels = P->n_levels; a.th_low = P->th_low;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.invfx = 1.0f / cam->fx; a.invfy = 1.0f / cam->fy; a.bf = P->bf;
    a.ratio_factor = 1.5f * P->scale_factor; a.tab = u_tab.dev(d);
    a.midx = r_mi.dev(d); a.mdist = r_md.dev(d); a.outcome = r_out.dev(d); a.branch = r_br.dev(d); a.x3d = r_x.dev(d);
    a.owner = r_own.dev(d); a.pass = s_pass.dev(d); a.blockcnt = s_bc.dev(d); a.ncreated = r_cnt.dev(d);
    a.c1 = r_c1.dev(d); a.c2 = r_c2.dev(d);
    bow_csr_enqueue(st, n_kf, (int)ct, u_nd.dev(d), u_n.dev(d), g_node.dev(d), g_start.dev(d), g_idx.dev(d), g_rows.dev(d));
    hipLaunchKernelGGL(k_np_search, dim3((unsigned)(cq / (NP_BLOCK / NP_GROUP)), n_kf), dim3(NP_BLOCK), 0, st, a);
    sc.tick();
    hipLaunchKernelGGL(k_np_triangulate, dim3((unsigned)nb, n_kf), dim3(NP_BLOCK), 0, st, a);
    sc.tick();
    hipLaunchKernelGGL(k_np_resolve, dim3((unsigned)nb), dim3(NP_BLOCK), 0, st, a);
    hipLaunchKernelGGL(k_np_compact, dim3((unsigned)nb, n_kf), dim3(NP_BLOCK), 0, st, a);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    for (int i = 0; i < 3; i++) sum->kernel_ms[i] = sc.ms[i];
    const size_t n = (size_t)n1;
    int n_new = 0;
    for (int j = 0; j < n_kf; j++) {
        hvo_np_result &R = res[j];
        R.n_created = r_cnt.down(b)[j]; R.gate = hk[j].gate; R.status = HVO_OK;
        n_new += R.n_created;
        memcpy(R.match_idx2, r_mi.down(b, j), n * 4);
        if (R.match_dist) memcpy(R.match_dist, r_md.down(b, j), n * 4);
        if (R.outcome) memcpy(R.outcome, r_out.down(b, j), n);
        if (R.branch) memcpy(R.branch, r_br.down(b, j), n);
        if (R.x3d) memcpy(R.x3d, r_x.down(b, j), n * 12);
        const size_t nc = (size_t)std::max(0, std::min(R.n_created, (int32_t)n));
        if (R.created_idx1) memcpy(R.created_idx1, r_c1.down(b, j), nc * 4);
        if (R.created_idx2) memcpy(R.created_idx2, r_c2.down(b, j), nc * 4);
    }
    if (sum->owner) memcpy(sum->owner, r_own.down(b), n * 4);
    sum->n_new = n_new;
    return HVO_OK;
}

extern "C" {

int hvo_create_new_map_points(hvo_ctx *ctx, const hvo_camera *cam, const hvo_np_params *params, const hvo_np_keyframe *current,
                              int n_kf, const hvo_np_keyframe *neighbours, hvo_np_result *results, hvo_np_summary *summary)
{
    if (!ctx) return HVO_ERR_INVALID_ARG;
    if (!cam || !params || !current || !summary) { ctx->last_error = "create new map points: a null argument"; return HVO_ERR_INVALID_ARG; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return np_run(ctx, ctx->stream, cam, params, current, nullptr, nullptr, n_kf, neighbours, results, summary, &ctx->last_error);
}

int hvo_stream_create_new_map_points(hvo_stream *s, int64_t cur, const hvo_vocabulary *voc, const hvo_camera *cam, const hvo_np_params *params, const float Tcw[12],
                                     const uint8_t *has_map_point, int n_kf, const hvo_np_keyframe *neighbours, hvo_np_result *results, hvo_np_summary *summary)
{
    if (!s) return HVO_ERR_INVALID_ARG;
    if (!voc || !cam || !params || !Tcw || !summary) { s->last_error = "create new map points: a null argument"; return HVO_ERR_INVALID_ARG; }
    const StreamSlot *B = slot_of(s, cur);
    if (B && (!B->bow.valid || B->bow.voc_uid != bow_voc_uid(voc))) {
        s->last_error = "create new map points: the frame holds no bag of words of this vocabulary (hvo_stream_compute_bow first)"; return HVO_ERR_INVALID_ARG;
    }
    FrameView V; int rc;
    if ((rc = stream_view(s, cur, need_new_points, s->s_match, V))) return rc;
    hvo_np_keyframe K; memset(&K, 0, sizeof(K));
    memcpy(K.Tcw, Tcw, sizeof(K.Tcw)); K.has_map_point = has_map_point; K.mb = cam->b; K.n = V.n_kp;
    BowLayout L; bow_layout(B->bow.cap, L);
    return np_run(V.ctx, s->s_match, cam, params, &K, &V, (const int *)(B->bow.d_blk + L.node_id), n_kf, neighbours, results, summary, &s->last_error);
}

}   // extern "C"
