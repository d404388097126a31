// bow.hip -- the ORB vocabulary resident on the device, Frame::ComputeBoW and ORBmatcher::SearchByBoW(KeyFrame, Frame).
//
// Reference: DBoW2 TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1271), BowVector::addWeight /
// addIfNotExist / normalize (BowVector.cpp:34-84), FORB::distance (FORB.cpp:81-101), the text format (TemplatedVocabulary.h:1350-1436),
// Frame::ComputeBoW (src/Frame.cc:1692-1699) and ORBmatcher::SearchByBoW (src/ORBmatcher.cc:162-293).  Nothing of DBoW2 is copied: this
// is a restatement of what those functions compute.
//
// Vocabulary layout.  The reference numbers the nodes in file order (row i is node i + 1, node 0 the root) and keeps a vector of child
// ids per node.  Here the nodes are renumbered breadth first at creation, so that the children of one node are consecutive: one round of
// one descriptor's descent is one contiguous load of up to k x 32 bytes, spread over the lanes of a 16-lane group.  Per node (device
// number): the descriptor (32 bytes), (first child, child count) with count 0 for a leaf, the reference's node id, the word id (-1 for
// an inner node) and the weight.  Results are reported in the reference's ids through the id table.
//
// Kernels.
//   k_bow_descend   16 lanes per descriptor, four descriptors per wave.  The descriptor sits in registers as 4 x u64; lane c (and
//                   c + 16 when k > 16) takes child c: four __popcll, and the group minimum is taken over distance << 8 | child
//                   position, so the first of equal children wins (the reference's strict `<`) without a branch.  It stops at the first
//                   leaf.  node_id is the node reached at level L - levelsup (the root when that is <= 0).
//                   DEFINED BEHAVIOUR (unbalanced tree): when the descent meets a leaf above level L - levelsup the reference leaves
//                   nid uninitialised; here node_id is that leaf's id and the feature is counted in n_short.
//   k_bow_assemble  one workgroup per frame: the features' (word, index) keys are sorted in LDS (bitonic), a thread at the head of each
//                   run forms the word's value -- for TF / TF_IDF the repeated `+=` of the leaf weight, once per feature in feature
//                   order (weight * count is a different double), for IDF / BINARY the first weight -- then ONE lane sums the norm in
//                   ascending word order, left to right (L1: fabs; L2: squares and one sqrt; TF / TF_IDF without a norm: the number of
//                   words), and every thread divides its words once.  The (node, index) keys are sorted the same way into the
//                   FeatureVector as CSR.  No atomic decides an order: the same bytes give the same result on every run and in all forms.
//   k_bow_csr       the same CSR from per-feature node ids (the key-frame side of the search, and the frame side on host arrays).
//   k_bow_search    one workgroup per (key frame, frame) pair, one wave per node present on both sides.  The node's key-frame features
//                   are visited in ascending index (those without a good map point skipped); the lanes hold the node's frame features,
//                   position p on lane p % 64, and the wave loops when a node holds more than 64.  Best = the smallest
//                   distance << 16 | position (the first minimum in list order), second = the second smallest key (the second smallest
//                   of the multiset); both start at 256.  The claimed flags are a 64-bit mask per lane (bit c: position 64 c + lane),
//                   private to the node because a frame feature lies in exactly one node.  Then the 30-bin rotation histogram and
//                   ComputeThreeMaxima (hvo_three_maxima, shared with the guided search).
#include "frame_view.hpp"
#include "staged_call.hpp"
#include "map_gates.hpp"      // ham256
#include <string.h>
#include <stdio.h>
#include <math.h>
#include <algorithm>
#include <atomic>
#include <fstream>
#include <new>
#include <sstream>

#define BOW_GROUP 16
#define BOW_MAXN HVO_BOW_MAXN

struct VocDev {
    const ulonglong4 *desc; const int2 *child; const int *ref_id; const int *word; const double *weight;
};

struct hvo_vocabulary {
    int device = -1, k = 0, L = 0, scoring = 0, weighting = 0, n_nodes = 1, n_words = 0;
    unsigned long long uid = 0;
    void *d_base = nullptr;
    VocDev d = {};
};

static std::atomic<unsigned long long> g_voc_uid{ 1 };

int bow_voc_device(const hvo_vocabulary *v) { return v->device; }
unsigned long long bow_voc_uid(const hvo_vocabulary *v) { return v->uid; }
void bow_layout(int cap, BowLayout &L)
{
    size_t o = 0; const size_t c = (size_t)(cap < 1 ? 1 : cap);
    L.cap = cap;
    L.counts = o; o += 256;
    L.word_id = o; o += stage_align(c * 4);
    L.node_id = o; o += stage_align(c * 4);
    L.flag = o; o += stage_align(c * 4);
    L.weight = o; o += stage_align(c * 8);
    L.bow_word = o; o += stage_align(c * 4);
    L.bow_val = o; o += stage_align(c * 8);
    L.fv_node = o; o += stage_align(c * 4);
    L.fv_start = o; o += stage_align((c + 1) * 4);
    L.fv_idx = o; o += stage_align(c * 4);
    L.total = o;
}

void bow_state_free(BowState *b)
{
    if (b->d_blk) (void)hipFree(b->d_blk);
    b->d_blk = nullptr; b->bytes = 0; b->valid = false;
}

// ------------------------------------------------------------------------------------------------ kernels
// grid (ceil(cap / 16), frames); frame f: descriptors at desc + f * desc_stride, count d_n[f * n_stride] (clamped to cap), block at blk + f * L.total
__global__ __launch_bounds__(256) void k_bow_descend(VocDev V, int nid_level, const uint8_t *__restrict__ desc, size_t desc_stride, const int *__restrict__ d_n,
                                                     int n_stride, char *__restrict__ blk, BowLayout L)
{
    const int f = blockIdx.y, gl = threadIdx.x & (BOW_GROUP - 1), i = blockIdx.x * (256 / BOW_GROUP) + (threadIdx.x / BOW_GROUP);
    const int n = max(0, min(d_n[(size_t)f * n_stride], L.cap));
    if (i >= n) return;                                        // a whole group leaves together
    char *b = blk + (size_t)f * L.total;
    const ulonglong4 q = *reinterpret_cast<const ulonglong4 *>(desc + (size_t)f * desc_stride + (size_t)i * 32);
    int node = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
    int2 ch = V.child[0];                                      // (first child, child count) of the node reached: loaded once per round
    do {
        level++;
        unsigned best = 0xFFFFFFFFu;
        for (int c = gl; c < ch.y; c += BOW_GROUP) {
            const unsigned key = ((unsigned)ham256(q, V.desc[ch.x + c]) << 8) | (unsigned)c;
            best = min(best, key);
        }
#pragma unroll
        for (int o = BOW_GROUP / 2; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, BOW_GROUP));
        node = ch.x + (int)(best & 255u);
        if (level == nid_level) nid = V.ref_id[node];
        ch = V.child[node];
    } while (ch.y != 0);
    int shortf = 0;
    if (nid < 0) { nid = V.ref_id[node]; shortf = 1; }         // a leaf above level L - levelsup: the defined behaviour
    int word = V.word[node];
    const double w = V.weight[node];
    if (!(w > 0)) { word = -1; nid = -1; shortf = 0; }         // a stopped word
    if (gl == 0) {
        ((int *)(b + L.word_id))[i] = word; ((int *)(b + L.node_id))[i] = nid; ((int *)(b + L.flag))[i] = shortf; ((double *)(b + L.weight))[i] = w;
    }
}

// ascending bitonic sort of keys[0 .. P), P a power of two >= 256, by the 256 threads of the workgroup
static __device__ void bow_sort(unsigned long long *keys, int P)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += 256) {
                const int x = t ^ j;
                if (x > t) {
                    const unsigned long long a = keys[t], b = keys[x];
                    if ((a > b) == ((t & k) == 0)) { keys[t] = b; keys[x] = a; }
                }
            }
            __syncthreads();
        }
}

static __device__ __forceinline__ int bow_pow2(int n) { int P = 256; while (P < n) P <<= 1; return P; }

// keys sorted, nv of them valid: the runs of equal high words.  Thread t owns positions [t * S, (t + 1) * S), S = P / 256; the return value is
// the rank (among all runs) of the first run that starts in the caller's segment, *n_runs the number of runs.  sc: 257 ints of LDS.
static __device__ int bow_run_ranks(const unsigned long long *keys, int P, int nv, int *sc, int *n_runs)
{
    const int S = P / 256, p0 = threadIdx.x * S;
    int c = 0;
    for (int p = p0; p < p0 + S && p < nv; p++) c += (p == 0 || (keys[p] >> 32) != (keys[p - 1] >> 32)) ? 1 : 0;
    sc[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int a = 0; for (int t = 0; t < 256; t++) { const int v = sc[t]; sc[t] = a; a += v; } sc[256] = a; }
    __syncthreads();
    const int r = sc[threadIdx.x];
    *n_runs = sc[256];
    __syncthreads();
    return r;
}

// the CSR of (node, index) keys that lie sorted in keys[0 .. nv)
static __device__ void bow_write_csr(const unsigned long long *keys, int P, int nv, int *sc, int *fv_node, int *fv_start, int *fv_idx, int *n_rows)
{
    int nr; int r = bow_run_ranks(keys, P, nv, sc, &nr);
    const int S = P / 256, p0 = threadIdx.x * S;
    for (int p = p0; p < p0 + S && p < nv; p++) {
        const unsigned long long key = keys[p];
        if (p == 0 || (key >> 32) != (keys[p - 1] >> 32)) { fv_node[r] = (int)(key >> 32); fv_start[r] = p; r++; }
        fv_idx[p] = (int)(key & 0xFFFFFFFFull);
    }
    if (threadIdx.x == 0) fv_start[nr] = nv;
    *n_rows = nr;
}

__global__ __launch_bounds__(256) void k_bow_assemble(int tf, int norm /* 0 none, 1 L1, 2 L2 */, const int *__restrict__ d_n, int n_stride, char *__restrict__ blk, BowLayout L)
{
    __shared__ unsigned long long keys[BOW_MAXN];
    __shared__ int sc[257];
    __shared__ int s_cnt[2];
    __shared__ double s_norm;
    const int f = blockIdx.x, tid = threadIdx.x;
    char *b = blk + (size_t)f * L.total;
    const int n = max(0, min(d_n[(size_t)f * n_stride], L.cap));
    const int *word_id = (const int *)(b + L.word_id), *node_id = (const int *)(b + L.node_id), *flag = (const int *)(b + L.flag);
    const double *weight = (const double *)(b + L.weight);
    int *bow_word = (int *)(b + L.bow_word); double *bow_val = (double *)(b + L.bow_val);
    int *counts = (int *)(b + L.counts);
    const int P = bow_pow2(n), S = P / 256;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    // ---- BowVector: (word, index) ----
    int nv_l = 0, ns_l = 0;
    for (int i = tid; i < P; i += 256) {
        unsigned long long key = ~0ull;
        if (i < n && word_id[i] >= 0) { key = ((unsigned long long)(unsigned)word_id[i] << 32) | (unsigned)i; nv_l++; ns_l += flag[i]; }
        keys[i] = key;
    }
    if (nv_l) atomicAdd(&s_cnt[0], nv_l);                      // integer counts only: no order depends on them
    if (ns_l) atomicAdd(&s_cnt[1], ns_l);
    __syncthreads();
    const int nv = s_cnt[0];
    bow_sort(keys, P);
    int nw; int r = bow_run_ranks(keys, P, nv, sc, &nw);
    for (int p = tid * S; p < tid * S + S && p < nv; p++) {
        const unsigned long long key = keys[p];
        if (p != 0 && (key >> 32) == (keys[p - 1] >> 32)) continue;
        const double w = weight[(int)(key & 0xFFFFFFFFull)];   // every feature of a word carries the leaf's weight
        double v = w;
        if (tf) for (int e = p + 1; e < nv && (keys[e] >> 32) == (key >> 32); e++) v += w;
        bow_word[r] = (int)(key >> 32); bow_val[r] = v; r++;
    }
    __syncthreads();                                            // the values are visible to the workgroup; the keys are free
    if (norm || tf) {
        double *vals = reinterpret_cast<double *>(keys);
        for (int i = tid; i < nw; i += 256) vals[i] = bow_val[i];
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            if (norm == 1) for (int i = 0; i < nw; i++) s += fabs(vals[i]);
            else if (norm == 2) { for (int i = 0; i < nw; i++) s += vals[i] * vals[i]; s = sqrt(s); }
            else s = (double)nw;                                // TF / TF_IDF without a norm: v.size()
            s_norm = s;
        }
        __syncthreads();
        const double s = s_norm;
        if (s > 0.0) for (int i = tid; i < nw; i += 256) bow_val[i] = vals[i] / s;
        __syncthreads();
    }
    // ---- FeatureVector: (node, index) ----
    for (int i = tid; i < P; i += 256)
        keys[i] = (i < n && word_id[i] >= 0) ? (((unsigned long long)(unsigned)node_id[i] << 32) | (unsigned)i) : ~0ull;
    __syncthreads();
    bow_sort(keys, P);
    int nr;
    bow_write_csr(keys, P, nv, sc, (int *)(b + L.fv_node), (int *)(b + L.fv_start), (int *)(b + L.fv_idx), &nr);
    if (tid == 0) { counts[0] = n; counts[1] = nw; counts[2] = nr; counts[3] = nv; counts[4] = s_cnt[1]; }
}

// one side of the search as device arrays; side j's arrays lie at base + j * stride (elements), its feature count at n[j]
struct BowSideDev {
    const uint8_t *desc; const int *node; const uint8_t *has_mp; const float *angle; int angle_step;   // angle of feature i at angle[i * angle_step]
    int *fv_node, *fv_start, *fv_idx, *n_rows;
    const int *n; int cap;
};

__global__ __launch_bounds__(256) void k_bow_csr(BowSideDev K)
{
    __shared__ unsigned long long keys[BOW_MAXN];
    __shared__ int sc[257];
    __shared__ int s_nv;
    const int j = blockIdx.x, tid = threadIdx.x;
    const int n = max(0, min(K.n[j], K.cap));
    const int *node = K.node + (size_t)j * K.cap;
    const int P = bow_pow2(n);
    if (tid == 0) s_nv = 0;
    __syncthreads();
    int nv_l = 0;
    for (int i = tid; i < P; i += 256) {
        unsigned long long key = ~0ull;
        if (i < n && node[i] >= 0) { key = ((unsigned long long)(unsigned)node[i] << 32) | (unsigned)i; nv_l++; }
        keys[i] = key;
    }
    if (nv_l) atomicAdd(&s_nv, nv_l);
    __syncthreads();
    const int nv = s_nv;
    bow_sort(keys, P);
    int nr;
    bow_write_csr(keys, P, nv, sc, K.fv_node + (size_t)j * K.cap, K.fv_start + (size_t)j * (K.cap + 1), K.fv_idx + (size_t)j * K.cap, &nr);
    if (tid == 0) K.n_rows[j] = nr;
}

void bow_csr_enqueue(hipStream_t st, int count, int cap, const int *node, const int *n, int *fv_node, int *fv_start, int *fv_idx, int *n_rows)
{
    BowSideDev K; memset(&K, 0, sizeof(K));
    K.node = node; K.n = n; K.cap = cap; K.fv_node = fv_node; K.fv_start = fv_start; K.fv_idx = fv_idx; K.n_rows = n_rows;
    hipLaunchKernelGGL(k_bow_csr, dim3(count), dim3(256), 0, st, K);
}

struct BowSearchDev {
    BowSideDev kf;                                             // key frame j
    const uint8_t *f_desc; const float *f_angle; int f_angle_step; const int *f_n; int f_cap;
    const int *f_fv_node, *f_fv_start, *f_fv_idx, *f_n_rows;
    float nnratio; int check_orientation, th_low;
    int *match_kf; int *n_matches;                             // key frame j: match_kf + j * f_cap
};

#define BOW_WAVES 4
__global__ __launch_bounds__(64 * BOW_WAVES) void k_bow_search(BowSearchDev a)
{
    __shared__ signed char rot[BOW_MAXN];
    __shared__ int hist[30], keep[3], s_nm;
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nf = max(0, min(*a.f_n, a.f_cap)), nk = max(0, min(a.kf.n[j], a.kf.cap));
    int *match = a.match_kf + (size_t)j * a.f_cap;
    for (int i = tid; i < nf; i += 64 * BOW_WAVES) { match[i] = -1; rot[i] = -1; }
    if (tid < 30) hist[tid] = 0;
    if (tid == 0) s_nm = 0;
    __syncthreads();
    const uint8_t *kdesc = a.kf.desc + (size_t)j * a.kf.cap * 32, *khas = a.kf.has_mp + (size_t)j * a.kf.cap;
    const float *kang = a.kf.angle + (size_t)j * a.kf.cap * a.kf.angle_step;
    const int *krow_node = a.kf.fv_node + (size_t)j * a.kf.cap, *krow_start = a.kf.fv_start + (size_t)j * (a.kf.cap + 1), *kidx = a.kf.fv_idx + (size_t)j * a.kf.cap;
    const int nkr = nk ? a.kf.n_rows[j] : 0, nfr = nf ? *a.f_n_rows : 0;
    const float factor = 1.0f / 30;
    for (int r = wave; r < nkr; r += BOW_WAVES) {              // wave-uniform from here on
        const int node = krow_node[r];
        int lo = 0, hi = nfr;                                   // the node's row on the frame side
        while (lo < hi) { const int m = (lo + hi) >> 1; if (a.f_fv_node[m] < node) lo = m + 1; else hi = m; }
        if (lo >= nfr || a.f_fv_node[lo] != node) continue;
        const int fb = a.f_fv_start[lo], nb = a.f_fv_start[lo + 1] - fb, kb = krow_start[r], na = krow_start[r + 1] - kb;
        const int nchunk = (nb + 63) >> 6;
        unsigned long long claimed = 0;                         // bit c: position 64 c + lane of this node's frame features has a match
        ulonglong4 fd0 = make_ulonglong4(0, 0, 0, 0);
        if (lane < nb) fd0 = reinterpret_cast<const ulonglong4 *>(a.f_desc)[a.f_fv_idx[fb + lane]];
        for (int ia = 0; ia < na; ia++) {
            const int ik = kidx[kb + ia];
            if (!khas[ik]) continue;
            const ulonglong4 kd = reinterpret_cast<const ulonglong4 *>(kdesc)[ik];
            unsigned k1 = (256u << 16) | 0xFFFFu, k2 = k1;      // distance << 16 | position; 256 = nothing yet
            for (int c = 0; c < nchunk; c++) {
                const int p = c * 64 + lane;
                if (p < nb && !((claimed >> c) & 1ull)) {
                    const int d = c == 0 ? ham256(kd, fd0) : ham256(kd, reinterpret_cast<const ulonglong4 *>(a.f_desc)[a.f_fv_idx[fb + p]]);
                    const unsigned key = ((unsigned)d << 16) | (unsigned)p;
                    if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned o1 = (unsigned)__shfl_xor((int)k1, o), o2 = (unsigned)__shfl_xor((int)k2, o);
                const unsigned mn = min(k1, o1), mx = max(k1, o1);
                k2 = min(mx, min(k2, o2)); k1 = mn;
            }
            const int d1 = (int)(k1 >> 16), d2 = min(256, (int)(k2 >> 16)), p1 = (int)(k1 & 0xFFFFu);
            if (d1 < 256 && d1 <= a.th_low && (float)d1 < __fmul_rn(a.nnratio, (float)d2)) {
                const int fi = a.f_fv_idx[fb + p1];
                if (lane == (p1 & 63)) claimed |= 1ull << (p1 >> 6);
                if (lane == 0) {
                    match[fi] = ik;
                    if (a.check_orientation) {
                        const int bin = hvo_rot_bin(kang[(size_t)ik * a.kf.angle_step], a.f_angle[(size_t)fi * a.f_angle_step], factor);
                        rot[fi] = (signed char)((bin >= 0 && bin < 30) ? bin : -1);   // (the reference asserts the range; angles outside [0, 360) are never culled here)
                    }
                }
            }
        }
    }
    __syncthreads();
    if (a.check_orientation) {
        for (int i = tid; i < nf; i += 64 * BOW_WAVES) if (rot[i] >= 0) atomicAdd(&hist[rot[i]], 1);
        __syncthreads();
        if (tid == 0) hvo_three_maxima(hist, keep);
        __syncthreads();
        for (int i = tid; i < nf; i += 64 * BOW_WAVES) { const int bn = rot[i]; if (bn >= 0 && bn != keep[0] && bn != keep[1] && bn != keep[2]) match[i] = -1; }
        __syncthreads();
    }
    int c = 0;
    for (int i = tid; i < nf; i += 64 * BOW_WAVES) c += match[i] >= 0 ? 1 : 0;
    if (c) atomicAdd(&s_nm, c);
    __syncthreads();
    if (tid == 0) a.n_matches[j] = s_nm;
}

// ------------------------------------------------------------------------------------------------ host: the vocabulary
static int voc_build(int device, int k, int L, int scoring, int weighting, int n_rows, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc,
                     const double *weight, hvo_vocabulary **out)
{
    if (!out) return HVO_ERR_INVALID_ARG;
    *out = nullptr;
    if (k < 2 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3 || n_rows < 0) return HVO_ERR_INVALID_ARG;
    if (n_rows > 0 && (!parent || !is_leaf || !desc || !weight)) return HVO_ERR_INVALID_ARG;
    const int nn = n_rows + 1;
    std::vector<int> nchild((size_t)nn, 0), first((size_t)nn, 0), fill((size_t)nn, 0), leaf((size_t)nn, 0), word((size_t)nn, -1);
    int n_words = 0;
    for (int i = 0; i < n_rows; i++) {
        const int id = i + 1, p = parent[i];
        if (p < 0 || p >= id) return HVO_ERR_INVALID_ARG;                    // a parent comes before its children
        if (leaf[p]) return HVO_ERR_INVALID_ARG;                             // a word has no children
        if (++nchild[p] > k) return HVO_ERR_INVALID_ARG;
        leaf[id] = is_leaf[i] ? 1 : 0;
        if (leaf[id]) word[id] = n_words++;                                  // the word id is the running count of leaves
    }
    for (int id = 1; id < nn; id++) if (!leaf[id] && nchild[id] == 0) return HVO_ERR_INVALID_ARG;
    // breadth-first renumbering: `order` lists the reference ids in device order, children of a node consecutive and in row order
    std::vector<int> child_start((size_t)nn + 1, 0), child_list((size_t)(n_rows > 0 ? n_rows : 1), 0), order((size_t)nn, 0), newid((size_t)nn, 0);
    for (int id = 0; id < nn; id++) child_start[id + 1] = child_start[id] + nchild[id];
    for (int i = 0; i < n_rows; i++) { const int p = parent[i]; child_list[child_start[p] + fill[p]++] = i + 1; }
    int head = 0, tail = 0;
    order[tail++] = 0;
    while (head < tail) {
        const int id = order[head]; newid[id] = head; first[id] = tail; head++;
        for (int c = 0; c < nchild[id]; c++) order[tail++] = child_list[child_start[id] + c];
    }
    if (tail != nn) return HVO_ERR_INVALID_ARG;                              // (cannot happen: every parent precedes its child)
    hvo_vocabulary *v = new (std::nothrow) hvo_vocabulary();
    if (!v) return HVO_ERR_HIP;                                              // out of memory: an allocation status, not a bad argument
    v->device = device; v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting; v->n_nodes = nn; v->n_words = n_words;
    v->uid = g_voc_uid.fetch_add(1);
    if (device >= 0) {
        const size_t o_desc = 0, o_child = stage_align((size_t)nn * 32), o_ref = o_child + stage_align((size_t)nn * 8), o_word = o_ref + stage_align((size_t)nn * 4),
                     o_w = o_word + stage_align((size_t)nn * 4), total = o_w + stage_align((size_t)nn * 8);
        std::vector<char> h;
        try { h.assign(total, 0); } catch (const std::bad_alloc &) { delete v; throw; }
        for (int q = 0; q < nn; q++) {
            const int id = order[q];
            if (id > 0) memcpy(&h[o_desc + (size_t)q * 32], desc + (size_t)(id - 1) * 32, 32);
            ((int2 *)&h[o_child])[q] = make_int2(first[id], nchild[id]);
            ((int *)&h[o_ref])[q] = id; ((int *)&h[o_word])[q] = word[id];
            ((double *)&h[o_w])[q] = id > 0 ? weight[id - 1] : 0.0;
        }
        if (hipSetDevice(device) != hipSuccess) { delete v; return HVO_ERR_NO_DEVICE; }
        if (hipMalloc(&v->d_base, total) != hipSuccess) { delete v; return HVO_ERR_HIP; }
        if (hipMemcpy(v->d_base, h.data(), total, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(v->d_base); delete v; return HVO_ERR_HIP; }
        char *d = (char *)v->d_base;
        v->d.desc = (const ulonglong4 *)(d + o_desc); v->d.child = (const int2 *)(d + o_child); v->d.ref_id = (const int *)(d + o_ref);
        v->d.word = (const int *)(d + o_word); v->d.weight = (const double *)(d + o_w);
    }
    *out = v;
    return HVO_OK;
}

// ------------------------------------------------------------------------------------------------ host: ComputeBoW
int bow_transform(hvo_ctx *ctx, hipStream_t st, const hvo_vocabulary *v, int levelsup, int nframes, const FrameView *fr, BowState *keep, bool may_keep,
                  hvo_bow *out, std::string *err)
{
    // one launch walks the frames: frame f's descriptors at d_desc + f * desc_stride, its count at d_n[f * n_stride]
    const uint8_t *d_desc = fr[0].desc; const int *d_n = fr[0].d_nkp; const int cap = fr[0].kp_cap;
    const size_t desc_stride = nframes > 1 ? (size_t)(fr[1].desc - fr[0].desc) : 0; const int n_stride = nframes > 1 ? (int)(fr[1].d_nkp - fr[0].d_nkp) : 0;
    for (int f = 0; f < nframes; f++) {
        const int n = fr[f].n_kp;
        if (n > BOW_MAXN) { *err = "bag of words: more than 4096 features in a frame"; return HVO_ERR_UNSUPPORTED; }
        if (out[f].cap < n) { *err = "bag of words: out.cap below the frame's feature count"; return HVO_ERR_INVALID_ARG; }
    }
    BowLayout L; bow_layout(cap, L);
    const bool kept = may_keep && keep->valid && keep->voc_uid == v->uid && keep->levelsup == levelsup && keep->n >= nframes && keep->cap == cap;
    const bool empty = v->n_words == 0;
    ctx->bow_ms[0] = 0.f;                                       // stays 0 when the kept result is returned or nothing is launched
    CallTimer timer(ctx, st);
    if (!kept) {
        keep->valid = false;
        const size_t need = (size_t)nframes * L.total;
        if (keep->bytes < need) {
            if (keep->d_blk) { (void)hipStreamSynchronize(st); (void)hipFree(keep->d_blk); keep->d_blk = nullptr; keep->bytes = 0; }
            if (hipMalloc((void **)&keep->d_blk, need) != hipSuccess) { *err = "bag of words: hipMalloc"; return HVO_ERR_HIP; }
            keep->bytes = need;
        }
        if (empty) {                                            // empty(): both vectors stay empty, every feature is reported as stopped
            if (hipMemsetAsync(keep->d_blk, 0xFF, need, st) != hipSuccess) return HVO_ERR_HIP;
            for (int f = 0; f < nframes; f++) if (hipMemsetAsync(keep->d_blk + (size_t)f * L.total + L.counts, 0, 256, st) != hipSuccess) return HVO_ERR_HIP;
        } else if (cap > 0) {
            const int tf = v->weighting == HVO_VOC_TF_IDF || v->weighting == HVO_VOC_TF;
            const int norm = v->scoring == HVO_VOC_DOT_PRODUCT ? 0 : (v->scoring == HVO_VOC_L2_NORM ? 2 : 1);
            timer.tick();
            hipLaunchKernelGGL(k_bow_descend, dim3((cap + 256 / BOW_GROUP - 1) / (256 / BOW_GROUP), nframes), dim3(256), 0, st, v->d, v->L - levelsup, d_desc, desc_stride,
                               d_n, n_stride, keep->d_blk, L);
            hipLaunchKernelGGL(k_bow_assemble, dim3(nframes), dim3(256), 0, st, tf, norm, d_n, n_stride, keep->d_blk, L);
            timer.tick();
            if (hipGetLastError() != hipSuccess) { *err = "bag of words: launch"; return HVO_ERR_HIP; }
        } else if (hipMemsetAsync(keep->d_blk, 0, need, st) != hipSuccess) return HVO_ERR_HIP;
        keep->voc_uid = v->uid; keep->levelsup = levelsup; keep->n = nframes; keep->cap = cap;
    }
    std::vector<char> h((size_t)nframes * L.total);
    if (hipMemcpyAsync(h.data(), keep->d_blk, h.size(), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        *err = std::string("bag of words: ") + hipGetErrorString(hipGetLastError()); return HVO_ERR_HIP;
    }
    keep->valid = true;
    float ms[3];
    timer.read(ms); ctx->bow_ms[0] = ms[0];
    for (int f = 0; f < nframes; f++) {
        const char *b = h.data() + (size_t)f * L.total; const int *c = (const int *)(b + L.counts);
        hvo_bow &o = out[f];
        const int n = fr[f].n_kp;
        o.n_features = n; o.n_words = empty ? 0 : c[1]; o.n_nodes = empty ? 0 : c[2]; o.n_valid = empty ? 0 : c[3]; o.n_short = empty ? 0 : c[4];
        o.computed = kept ? 0 : 1; o.status = HVO_OK;
        if (o.word_id) memcpy(o.word_id, b + L.word_id, (size_t)n * 4);
        if (o.node_id) memcpy(o.node_id, b + L.node_id, (size_t)n * 4);
        if (o.bow_word) memcpy(o.bow_word, b + L.bow_word, (size_t)o.n_words * 4);
        if (o.bow_value) memcpy(o.bow_value, b + L.bow_val, (size_t)o.n_words * 8);
        if (o.fv_node) memcpy(o.fv_node, b + L.fv_node, (size_t)o.n_nodes * 4);
        if (o.fv_start) { memcpy(o.fv_start, b + L.fv_start, (size_t)(o.n_nodes + 1) * 4); if (empty) o.fv_start[0] = 0; }
        if (o.fv_index) memcpy(o.fv_index, b + L.fv_idx, (size_t)o.n_valid * 4);
    }
    return HVO_OK;
}

// ------------------------------------------------------------------------------------------------ host: SearchByBoW
int bow_search(hvo_ctx *ctx, hipStream_t st, const hvo_bow_keyframe *F, const FrameView *fr, const BowState *bow, int n_kf, const hvo_bow_keyframe *kf,
               const hvo_bow_search_params *P, hvo_bow_matches *res, std::string *err)
{
    const int nf = F ? F->n : fr->n_kp;
    int capk = 0;
    for (int j = 0; j < n_kf; j++) {
        if (kf[j].n < 0 || (kf[j].n > 0 && (!kf[j].desc || !kf[j].node_id || !kf[j].has_map_point || (P->check_orientation && !kf[j].angle)))) return HVO_ERR_INVALID_ARG;
        capk = std::max(capk, kf[j].n);
    }
    if (nf > BOW_MAXN || capk > BOW_MAXN) { *err = "search by bag of words: more than 4096 features on one side"; return HVO_ERR_UNSUPPORTED; }
    for (int j = 0; j < n_kf; j++) { res[j].n_matches = 0; res[j].status = HVO_OK; if (nf > 0 && !res[j].match_kf) return HVO_ERR_INVALID_ARG; }
    if (nf == 0) return HVO_OK;
    if (capk == 0) { for (int j = 0; j < n_kf; j++) for (int i = 0; i < nf; i++) res[j].match_kf[i] = -1; return HVO_OK; }
    const bool fhost = F != nullptr;
    // one carve of the context's arena: the key-frame side (n_kf slots of capk), the frame side when it comes from the host, the results
    const size_t Kf = (size_t)n_kf, ck = (size_t)capk, cf = (size_t)nf;
    StageCarver C(256);
    const auto k_desc = C.take<uint8_t>(Kf, ck * 32); const auto k_node = C.take<int>(Kf, ck); const auto k_has = C.take<uint8_t>(Kf, ck);
    const auto k_ang = C.take<float>(Kf, ck); const auto k_n = C.take<int>(Kf);
    const auto f_desc = C.take<uint8_t>(cf * 32); const auto f_node = C.take<int>(cf); const auto f_ang = C.take<float>(cf); const auto f_n = C.take<int>(1);
    const size_t up_end = C.mark();
    const auto c_node = C.take<int>(Kf, ck), c_start = C.take<int>(Kf, ck + 1), c_idx = C.take<int>(Kf, ck), c_rows = C.take<int>(Kf);
    const auto g_node = C.take<int>(cf), g_start = C.take<int>(cf + 1), g_idx = C.take<int>(cf), g_rows = C.take<int>(1);
    const auto r_match = C.take<int>(Kf, cf), r_n = C.take<int>(Kf);
    const size_t r0 = r_match.off, r1 = C.mark();               // the two results come down
    StagedCall sc(ctx, st, "search by bag of words: ", err); int rc;
    ctx->bow_ms[1] = 0.f;
    if ((rc = sc.begin(r1, up_end, r1 - r0))) return rc;
    char *const d = sc.d, *const h = sc.h;
    for (int j = 0; j < n_kf; j++) {
        const int n = kf[j].n;
        k_n.host(h)[j] = n;
        if (!n) continue;
        for (int i = 0; i < n; i++) if (kf[j].node_id[i] < -1) return HVO_ERR_INVALID_ARG;
        memcpy(k_desc.host(h, j), kf[j].desc, (size_t)n * 32);
        memcpy(k_node.host(h, j), kf[j].node_id, (size_t)n * 4);
        memcpy(k_has.host(h, j), kf[j].has_map_point, (size_t)n);
        if (kf[j].angle) memcpy(k_ang.host(h, j), kf[j].angle, (size_t)n * 4);
    }
    f_n.host(h)[0] = nf;
    if (fhost) {
        for (int i = 0; i < nf; i++) if (F->node_id[i] < -1) return HVO_ERR_INVALID_ARG;
        memcpy(f_desc.host(h), F->desc, (size_t)nf * 32); memcpy(f_node.host(h), F->node_id, (size_t)nf * 4);
        if (F->angle) memcpy(f_ang.host(h), F->angle, (size_t)nf * 4);
    }
    if ((rc = sc.up(0, up_end))) return rc;
    BowSideDev K; memset(&K, 0, sizeof(K));
    K.desc = k_desc.dev(d); K.node = k_node.dev(d); K.has_mp = k_has.dev(d); K.angle = k_ang.dev(d); K.angle_step = 1;
    K.fv_node = c_node.dev(d); K.fv_start = c_start.dev(d); K.fv_idx = c_idx.dev(d); K.n_rows = c_rows.dev(d); K.n = k_n.dev(d); K.cap = capk;
    sc.tick();
    hipLaunchKernelGGL(k_bow_csr, dim3(n_kf), dim3(256), 0, st, K);
    BowSearchDev A; memset(&A, 0, sizeof(A));
    A.kf = K; A.f_n = f_n.dev(d); A.f_cap = nf;
    if (fhost) {
        BowSideDev G; memset(&G, 0, sizeof(G));
        G.node = f_node.dev(d); G.fv_node = g_node.dev(d); G.fv_start = g_start.dev(d); G.fv_idx = g_idx.dev(d); G.n_rows = g_rows.dev(d);
        G.n = A.f_n; G.cap = nf;
        hipLaunchKernelGGL(k_bow_csr, dim3(1), dim3(256), 0, st, G);
        A.f_desc = f_desc.dev(d); A.f_angle = f_ang.dev(d); A.f_angle_step = 1;
        A.f_fv_node = G.fv_node; A.f_fv_start = G.fv_start; A.f_fv_idx = G.fv_idx; A.f_n_rows = G.n_rows;
    } else {
        BowLayout L; bow_layout(bow->cap, L);
        A.f_desc = fr->desc; A.f_angle = &fr->kp->angle; A.f_angle_step = (int)(sizeof(hvo_keypoint) / sizeof(float));      // F.mvKeys[i].angle
        A.f_fv_node = (const int *)(bow->d_blk + L.fv_node); A.f_fv_start = (const int *)(bow->d_blk + L.fv_start); A.f_fv_idx = (const int *)(bow->d_blk + L.fv_idx);
        A.f_n_rows = (const int *)(bow->d_blk + L.counts) + 2;
    }
    A.nnratio = P->nnratio; A.check_orientation = P->check_orientation ? 1 : 0; A.th_low = P->th_low;
    A.match_kf = r_match.dev(d); A.n_matches = r_n.dev(d);
    hipLaunchKernelGGL(k_bow_search, dim3(n_kf), dim3(64 * BOW_WAVES), 0, st, A);
    sc.tick();
    StageDown b;
    if ((rc = sc.down(r0, r1, &b))) return rc;
    ctx->bow_ms[1] = sc.ms[0];
    for (int j = 0; j < n_kf; j++) { memcpy(res[j].match_kf, r_match.down(b, j), (size_t)nf * 4); res[j].n_matches = r_n.down(b)[j]; }
    return HVO_OK;
}

// ------------------------------------------------------------------------------------------------ the C ABI (context forms; the stream forms are in stream.hip)
extern "C" {

int hvo_vocabulary_create(int device, int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent, const uint8_t *is_leaf, const uint8_t *desc,
                          const double *weight, hvo_vocabulary **voc)
{
    // the host staging of a large tree (62 MB for ORBvoc) may fail to allocate: no exception crosses the C boundary
    try { return voc_build(device, k, L, scoring, weighting, n_nodes, parent, is_leaf, desc, weight, voc); }
    catch (const std::bad_alloc &) { if (voc) *voc = nullptr; return HVO_ERR_HIP; }
}

int hvo_vocabulary_load_text(const char *path, int device, hvo_vocabulary **voc)
{
    if (!path || !voc) return HVO_ERR_INVALID_ARG;
    *voc = nullptr;
    try {
    std::ifstream f(path);
    if (!f.good()) return HVO_ERR_INVALID_ARG;
    std::string line;
    if (!std::getline(f, line)) return HVO_ERR_INVALID_ARG;
    int k = -1, L = -1, sc = -1, wt = -1;
    { std::istringstream ss(line); ss >> k >> L >> sc >> wt; if (ss.fail()) return HVO_ERR_INVALID_ARG; }
    std::vector<int32_t> parent; std::vector<uint8_t> leaf, desc; std::vector<double> weight;
    while (std::getline(f, line)) {
        const char *p = line.c_str(); char *e = nullptr;
        while (*p == ' ' || *p == '\t' || *p == '\r') p++;
        if (!*p) continue;                                      // (the reference turns a trailing empty line into a node; it is skipped here)
        const long pid = strtol(p, &e, 10); if (e == p) return HVO_ERR_INVALID_ARG; p = e;
        const long lf = strtol(p, &e, 10); if (e == p) return HVO_ERR_INVALID_ARG; p = e;
        for (int b = 0; b < 32; b++) { const long v = strtol(p, &e, 10); if (e == p || v < 0 || v > 255) return HVO_ERR_INVALID_ARG; p = e; desc.push_back((uint8_t)v); }
        const double w = strtod(p, &e); if (e == p) return HVO_ERR_INVALID_ARG;
        if (pid < 0 || pid > 0x7FFFFFFF) return HVO_ERR_INVALID_ARG;
        parent.push_back((int32_t)pid); leaf.push_back(lf > 0 ? 1 : 0); weight.push_back(w);
    }
    return voc_build(device, k, L, sc, wt, (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data(), voc);
    } catch (const std::bad_alloc &) { *voc = nullptr; return HVO_ERR_HIP; }
}

void hvo_vocabulary_destroy(hvo_vocabulary *v)
{
    if (!v) return;
    if (v->d_base) { (void)hipSetDevice(v->device); (void)hipDeviceSynchronize(); (void)hipFree(v->d_base); }
    delete v;
}

int hvo_vocabulary_info(const hvo_vocabulary *v, hvo_vocabulary_desc *info)
{
    if (!v || !info) return HVO_ERR_INVALID_ARG;
    info->k = v->k; info->L = v->L; info->n_nodes = v->n_nodes; info->n_words = v->n_words; info->scoring = v->scoring; info->weighting = v->weighting;
    info->device = v->device;
    return HVO_OK;
}

// on host descriptors, n_frames frames in one launch sequence
int hvo_compute_bow(hvo_ctx *ctx, const hvo_vocabulary *voc, int levelsup, int n_frames, const uint8_t *const *desc, const int32_t *n_desc, hvo_bow *out)
{
    if (!ctx || !voc || !out || n_frames < 1 || !n_desc || !desc) return HVO_ERR_INVALID_ARG;
    if (voc->device != ctx->device) { ctx->last_error = "bag of words: the vocabulary lives on another device (or on none)"; return HVO_ERR_INVALID_ARG; }
    int cap = 0;
    for (int f = 0; f < n_frames; f++) { if (n_desc[f] < 0 || (n_desc[f] > 0 && !desc[f])) return HVO_ERR_INVALID_ARG; cap = std::max(cap, (int)n_desc[f]); }
    if (cap > BOW_MAXN) { ctx->last_error = "bag of words: more than 4096 features in a frame"; return HVO_ERR_UNSUPPORTED; }
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    const size_t b_desc = stage_align((size_t)n_frames * std::max(cap, 1) * 32), b_n = stage_align((size_t)n_frames * 4);
    char *a = (char *)hvo_call_arena(ctx, b_desc + b_n);
    if (!a) return HVO_ERR_HIP;
    std::vector<char> h(b_desc + b_n, 0);
    for (int f = 0; f < n_frames; f++) { if (n_desc[f]) memcpy(&h[(size_t)f * cap * 32], desc[f], (size_t)n_desc[f] * 32); ((int *)&h[b_desc])[f] = n_desc[f]; }
    HVO_HIP(hipMemcpyAsync(a, h.data(), h.size(), hipMemcpyHostToDevice, ctx->stream));
    FrameView zero; memset(&zero, 0, sizeof(zero));
    std::vector<FrameView> F((size_t)n_frames, zero);
    for (int f = 0; f < n_frames; f++) { F[f].desc = (const uint8_t *)a + (size_t)f * cap * 32; F[f].d_nkp = (const int *)(a + b_desc) + f; F[f].kp_cap = cap; F[f].n_kp = n_desc[f]; }
    return bow_transform(ctx, ctx->stream, voc, levelsup, n_frames, F.data(), &ctx->bow_call, false, out, &ctx->last_error);
}

// on the first n frames of the resident batch: the descriptors where HVO_STAGE_ORB left them; the result stays with the batch
int hvo_batch_compute_bow(hvo_ctx *ctx, const hvo_vocabulary *voc, int n, int levelsup, hvo_bow *out)
{
    if (!ctx || !voc || !out || n < 1) return HVO_ERR_INVALID_ARG;
    std::vector<FrameView> F; int rc;
    if ((rc = batch_views(ctx, n, need_bow, F))) return rc;
    if (voc->device != ctx->device) { ctx->last_error = "bag of words: the vocabulary lives on another device (or on none)"; return HVO_ERR_INVALID_ARG; }
    return bow_transform(ctx, ctx->stream, voc, levelsup, n, F.data(), &ctx->bow_batch, true, out, &ctx->last_error);
}

// ORBmatcher::SearchByBoW on host arrays for both sides: n_kf key frames against one frame in one launch
int hvo_search_by_bow(hvo_ctx *ctx, const hvo_bow_keyframe *frame, int n_kf, const hvo_bow_keyframe *kf, const hvo_bow_search_params *params, hvo_bow_matches *res)
{
    if (!ctx || !frame || !kf || !params || !res || n_kf < 1 || frame->n < 0) return HVO_ERR_INVALID_ARG;
    if (frame->n > 0 && (!frame->desc || !frame->node_id || (params->check_orientation && !frame->angle))) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    if (frame->n == 0) { for (int j = 0; j < n_kf; j++) { res[j].n_matches = 0; res[j].status = HVO_OK; } return HVO_OK; }
    return bow_search(ctx, ctx->stream, frame, nullptr, nullptr, n_kf, kf, params, res, &ctx->last_error);
}

// device time of the context's last ComputeBoW (ms2[0]: descent + assembly; 0 when the kept result was returned) and last SearchByBoW
// (ms2[1]: the key frames' CSR + the search kernel)
int hvo_bow_last_kernel_ms(const hvo_ctx *ctx, float ms2[2])
{
    if (!ctx || !ms2) return HVO_ERR_INVALID_ARG;
    ms2[0] = ctx->bow_ms[0]; ms2[1] = ctx->bow_ms[1];
    return HVO_OK;
}

}   // extern "C"
