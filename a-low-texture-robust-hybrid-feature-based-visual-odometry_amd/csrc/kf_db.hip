// kf_db.hip -- the key-frame database resident on the device: KeyFrameDatabase::add / erase / clear, DetectRelocalizationCandidates and
// DetectLoopCandidates with the vocabulary's score().
//
// Reference: src/KeyFrameDatabase.cc:40-73 (add, erase, clear), :76-197 (DetectLoopCandidates), :199-309 (DetectRelocalizationCandidates),
// Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-310 (the score functions) and src/KeyFrame.cc:36 (the query fields start at 0, the two scores
// are not initialised).  Nothing of them is copied: this is a restatement of what they compute.
//
// The reference keeps an inverted file (word -> list of key frames) and walks the query's words.  Here a key frame is a slot that keeps
// its own bag of words (ascending word ids, double values) in a pool, and a query visits every live slot with one wave.  What the walk
// of the inverted file decides besides the counts is an ORDER: a key frame enters lKFsSharingWords when the walk first meets it, i.e.
// ordered by (its smallest word in common with the query, its position in that word's list = the order of add).  That pair is the
// 64-bit discovery key below; everything the reference keeps in list order is ordered by it.  DESIGN.md ("Key-frame database") lists
// the readings.
//
// Storage.  Slot table (device, KFDB_MAX_SLOTS records, allocated once: 1.2 MB): first / cap / count of the slot's room in the pool, add
// sequence, live flag, up to 10 neighbour slots; beside it the two kept scores per slot (reloc, loop), which only the kernels write.
// The pool (word ids, values) is grow-only: it doubles with one device copy, an erased slot keeps its room for the next add, and a bag
// that outgrows its room gets a new room at the pool's end (the slot alone moves).  The query's scratch and the pinned staging are sized
// once for the limits (about 1 MB and 0.4 MB).
//
// A query: one upload (the connected bytes and the header's start values; in the host form the bag's two arrays too), four kernels, one
// download, ONE synchronisation at the end.  Nothing is read back in between: every kernel derives what it needs (min_common from
// max_common, the 0.75 threshold from best_acc) from the header on the device.
//   k_kfdb_common      one wave per slot: common-word count, discovery key, max_common
//   k_kfdb_score       one wave per slot that passes words > min_common: the score, summed left to right
//   k_kfdb_accumulate  one lane per entered slot: the neighbours' scores (this query's, else the kept one), accScore, pBestKF, bestAccScore
//   k_kfdb_select      one workgroup: the entries above 0.75f * bestAccScore in discovery order, later duplicates of a pBestKF removed;
//                      then, unless the candidates outgrow the caller's cap (the call is refused whole), this query's scores become the kept ones
#include "frame_view.hpp"
#include <string.h>
#include <math.h>
#include <algorithm>
#include <new>

#define KFDB_MAX_SLOTS HVO_KFDB_MAX_SLOTS
#define KFDB_MAX_WORDS HVO_BOW_MAXN
#define KFDB_NB HVO_KFDB_MAX_COVISIBLE
#define KFDB_SPB 4                          // slots per workgroup in the per-slot kernels: one per wave
#define KFDB_U 4                            // words per lane and round in the per-slot kernels: four independent look-ups in flight
#define KFDB_LDS_SORT 2048                  // entries the select kernel sorts in LDS; more are sorted in global scratch

struct KfSlot { long long first; int cap, count, seq, live, n_nb, pad; int nb[KFDB_NB]; };
struct KfHdr { int max_common, n_sharing, n_scored, pad0, n_cand, min_common; unsigned best_key; float best_acc; int q_n; int pad[7]; };
static_assert(sizeof(KfSlot) == 72 && sizeof(KfHdr) == 64, "device records");

struct KfArgs {
    const KfSlot *slot; float2 *kept; const int *pw; const double *pv;
    const int *q_n; const int *q_word; const double *q_val;
    int n_slots, mode, scoring, cap; float min_score;
    KfHdr *hdr; int *cand, *words, *best; float *score, *acc;
    unsigned long long *key; uint8_t *entered; const uint8_t *conn; int *first_pos;
    unsigned long long *skey; int *sval;
};

struct hvo_keyframe_db {
    int device = 0, scoring = 0, voc_words = 0; unsigned long long voc_uid = 0;
    hipStream_t st = nullptr; hipEvent_t ev[2] = { nullptr, nullptr }; float last_ms = 0.f;
    std::vector<KfSlot> slot; int n_slots = 0, n_live = 0; long long next_seq = 0;
    KfSlot *d_slot = nullptr; float2 *d_kept = nullptr;
    int *d_pw = nullptr; double *d_pv = nullptr; size_t pool_cap = 0, pool_used = 0;
    char *d_scr = nullptr, *h_up = nullptr, *h_res = nullptr;
    std::string last_error;
};

// the query's device scratch, sized once for KFDB_MAX_SLOTS and KFDB_MAX_WORDS.  The connected bytes end where the result block (header,
// candidates, the four views) begins, so the bytes and the header's start values go up in one copy and the block comes down in one; the host
// form's bag lies in front.
enum : size_t {
    KS_QWORD = 0, KS_QVAL = KS_QWORD + KFDB_MAX_WORDS * 4, KS_CONN = KS_QVAL + KFDB_MAX_WORDS * 8, KS_RES = KS_CONN + KFDB_MAX_SLOTS, KS_UP_END = KS_RES + 64,
    KS_RES_BYTES = 64 + 5 * 4 * (size_t)KFDB_MAX_SLOTS,
    KS_KEY = KS_RES + KS_RES_BYTES, KS_ENTERED = KS_KEY + 8 * (size_t)KFDB_MAX_SLOTS, KS_FIRST = KS_ENTERED + KFDB_MAX_SLOTS,
    KS_SKEY = KS_FIRST + 4 * (size_t)KFDB_MAX_SLOTS, KS_SVAL = KS_SKEY + 8 * (size_t)KFDB_MAX_SLOTS, KS_TOTAL = KS_SVAL + 4 * (size_t)KFDB_MAX_SLOTS
};
#define KFDB_UP_BYTES ((size_t)KS_UP_END)     // pinned h_up mirrors [0, KS_UP_END); it also stages an add: words at KS_QWORD, values at KS_QVAL, slot record at KS_CONN

#define KF_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { db->last_error = std::string(#call) + ": " + hipGetErrorString(e_); return HVO_ERR_HIP; } } while (0)

static int kf_fail(hvo_keyframe_db *db, int rc, const std::string &why) { db->last_error = "key-frame database: " + why; return rc; }

// ------------------------------------------------------------------------------------------------ kernels
// a float as an unsigned key of the same order (every float but NaN)
static __device__ __host__ __forceinline__ unsigned kf_fkey(float f)
{
    unsigned u; memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ float kf_funkey(unsigned k)
{
    const unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return __uint_as_float(u);
}

// positions of KFDB_U words in the ascending q[0 .. n) (LDS), or -1.  top: the largest power of two <= n (0 for n == 0).  The trip count is
// the same for every lane and the KFDB_U searches are independent, so each step issues KFDB_U LDS loads before it waits for the first.
static __device__ __forceinline__ void kf_find(const int *q, int n, int top, const int (&w)[KFDB_U], int (&pos)[KFDB_U])
{
    int lo[KFDB_U];
#pragma unroll
    for (int u = 0; u < KFDB_U; u++) lo[u] = 0;
    for (int step = top; step > 0; step >>= 1) {
#pragma unroll
        for (int u = 0; u < KFDB_U; u++) { const int m = lo[u] + step; if (m <= n && q[m - 1] < w[u]) lo[u] = m; }   // lo = how many of q lie below w
    }
#pragma unroll
    for (int u = 0; u < KFDB_U; u++) pos[u] = (lo[u] < n && q[lo[u]] == w[u]) ? lo[u] : -1;
}

// lane l's double in every lane (l is the same in all lanes)
static __device__ __forceinline__ double kf_readlane(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

static __device__ __forceinline__ int kf_min_common(int max_common) { return (int)((float)max_common * 0.8f); }   // int minCommonWords = maxCommonWords*0.8f

// One wave per slot, four slots per workgroup; the query's word ids lie in LDS (16 KB).  The slot's words are taken KFDB_U x 64 at a time
// with coalesced loads (word u of a lane in round c is c + 64 u + lane), each lane looks its words up in LDS; a ballot's popcount is the
// run's common words and its lowest set lane holds the first common word (the slot's words ascend).  A slot that is erased, or connected
// in the loop form, is "not in the query": words 0.
__global__ __launch_bounds__(256) void k_kfdb_common(KfArgs a)
{
    __shared__ int qw[KFDB_MAX_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nq = max(0, min(*a.q_n, KFDB_MAX_WORDS)), top = nq ? 1 << (31 - __clz(nq)) : 0;
    for (int i = tid; i < nq; i += 256) qw[i] = a.q_word[i];
    __syncthreads();
    const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * KFDB_SPB + wave);
    if (s >= a.n_slots) return;
    const KfSlot *S = a.slot + s;
    const int live = S->live, cnt = max(0, min(S->count, S->cap)), seq = S->seq;
    const long long first = S->first;
    int common = 0; unsigned fw = 0;
    if (live && !a.conn[s] && nq > 0) {
        for (int c = 0; c < cnt; c += 64 * KFDB_U) {
            int w[KFDB_U], pos[KFDB_U];
#pragma unroll
            for (int u = 0; u < KFDB_U; u++) { const int i = c + 64 * u + lane; w[u] = i < cnt ? a.pw[first + i] : 0x7FFFFFFF; }   // (no word id is INT_MAX)
            kf_find(qw, nq, top, w, pos);
#pragma unroll
            for (int u = 0; u < KFDB_U; u++) {
                const unsigned long long m = __ballot(pos[u] >= 0);
                if (m) {
                    if (!common) fw = (unsigned)__shfl(w[u], __builtin_ctzll(m));
                    common += __popcll(m);
                }
            }
        }
    }
    if (lane == 0) {
        const float qnan = __builtin_nanf("");
        a.words[s] = common; a.key[s] = common ? (((unsigned long long)fw << 32) | (unsigned)seq) : ~0ull;
        a.score[s] = qnan; a.acc[s] = qnan; a.best[s] = -1; a.entered[s] = 0; a.first_pos[s] = 0x7FFFFFFF;
        // an integer maximum: no order depends on it.  Thousands of slots share the one address, so a slot that cannot raise the maximum any more
        // (most of them, once the first waves are through) only looks; the counts are taken by k_kfdb_select.
        if (common > __hip_atomic_load(&a.hdr->max_common, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&a.hdr->max_common, common);
    }
}

// One wave per slot with words > min_common (every wave derives min_common from max_common itself; a workgroup none of whose four slots
// passes leaves before it fills LDS).  The per-word terms are formed by the lanes in parallel, KFDB_U x 64 words at a time; then the sum
// runs over the common words strictly left to right in ascending word order: the set lanes of each ballot from the lowest up, the lane's
// term broadcast (v_readlane) and added to ONE running double -- a serial chain, the same in every lane.  That is the order of the
// reference's merge loop, and double addition is not associative, so a tree reduction would be another sum.  The serial tail is at most
// 4096 dependent adds for the few slots that pass: the price of bit equality.  (The terms go through no LDS: a broadcast per term costs
// less than the compaction store and the dependent LDS load it replaces.)  -ffp-contract=off keeps vi * wi out of an FMA.
__global__ __launch_bounds__(256) void k_kfdb_score(KfArgs a)
{
    __shared__ int qw[KFDB_MAX_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int minc = kf_min_common(a.hdr->max_common);
    const int s = __builtin_amdgcn_readfirstlane(blockIdx.x * KFDB_SPB + wave);
    const bool pass = s < a.n_slots && a.words[s] > minc;      // (words > 0 then: the slot is live and in the query)
    if (!__syncthreads_or(pass ? 1 : 0)) return;
    const int nq = max(0, min(*a.q_n, KFDB_MAX_WORDS)), top = nq ? 1 << (31 - __clz(nq)) : 0;
    for (int i = tid; i < nq; i += 256) qw[i] = a.q_word[i];
    __syncthreads();
    if (!pass) return;
    const KfSlot *S = a.slot + s;
    const int cnt = max(0, min(S->count, S->cap));
    const long long first = S->first;
    double sum = 0.0;
    for (int c = 0; c < cnt; c += 64 * KFDB_U) {
        int w[KFDB_U], pos[KFDB_U]; double term[KFDB_U]; bool add[KFDB_U];
#pragma unroll
        for (int u = 0; u < KFDB_U; u++) { const int i = c + 64 * u + lane; w[u] = i < cnt ? a.pw[first + i] : 0x7FFFFFFF; }
        kf_find(qw, nq, top, w, pos);
#pragma unroll
        for (int u = 0; u < KFDB_U; u++) {
            add[u] = pos[u] >= 0; term[u] = 0.0;
            if (add[u]) {
                const double vi = a.q_val[pos[u]], wi = a.pv[first + c + 64 * u + lane];       // v1 is the query, v2 the key frame
                switch (a.scoring) {
                case HVO_VOC_L1_NORM: term[u] = fabs(vi - wi) - fabs(vi) - fabs(wi); break;
                case HVO_VOC_CHI_SQUARE: if (vi + wi != 0.0) term[u] = vi * wi / (vi + wi); else add[u] = false; break;
                case HVO_VOC_BHATTACHARYYA: term[u] = sqrt(vi * wi); break;
                default: term[u] = vi * wi; break;                 // L2 and the dot product
                }
            }
        }
#pragma unroll
        for (int u = 0; u < KFDB_U; u++) {
            unsigned long long m = __ballot(add[u]);
            while (m) { sum += kf_readlane(term[u], __builtin_ctzll(m)); m &= m - 1; }
        }
    }
    if (lane == 0) {
        switch (a.scoring) {
        case HVO_VOC_L1_NORM: sum = -sum / 2.0; break;
        case HVO_VOC_L2_NORM: if (sum >= 1) sum = 1.0; else sum = 1.0 - sqrt(1.0 - sum); break;
        case HVO_VOC_CHI_SQUARE: sum = 2. * sum; break;
        default: break;
        }
        const float si = (float)sum;                                // float si = mpVoc->score(...)
        a.score[s] = si;
        const int in = a.mode == HVO_KFDB_LOOP ? (si >= a.min_score ? 1 : 0) : 1;
        a.entered[s] = (uint8_t)(2 | in);                          // bit 1: scored by this query, bit 0: entered lScoreAndMatch
    }
}

// One lane per entered slot.  A neighbour counts when it is in the query (words > 0: live, sharing a word, not connected); the loop form
// also asks words > min_common of it.  What is added is the score on the neighbour: this query's, or -- in the relocalisation form, when
// this query did not score it -- the KEPT one an earlier query left.  bestAccScore is a maximum of floats, taken as an integer maximum over an order-preserving key; that is
// exact for every float but NaN, and NaN cannot occur: bags hold finite values >= 0 (the entry points refuse others), so every term and
// every score the five scorings form from them is a finite number >= 0 or +inf, and sums of those are never NaN.
__global__ __launch_bounds__(256) void k_kfdb_accumulate(KfArgs a)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_slots || !(a.entered[s] & 1)) return;
    const int minc = kf_min_common(a.hdr->max_common);
    const KfSlot *S = a.slot + s;
    const float si = a.score[s];
    float acc = si, best = si; int bk = s;
    const int nn = max(0, min(S->n_nb, KFDB_NB));
    for (int j = 0; j < nn; j++) {
        const int nb = S->nb[j];
        if (nb < 0 || nb >= a.n_slots) continue;
        const int wn = a.words[nb];
        if (wn <= 0 || (a.mode == HVO_KFDB_LOOP && !(wn > minc))) continue;
        const float sc = (a.entered[nb] & 2) ? a.score[nb] : (a.mode == HVO_KFDB_LOOP ? a.kept[nb].y : a.kept[nb].x);
        acc += sc;
        if (sc > best) { bk = nb; best = sc; }
    }
    a.acc[s] = acc; a.best[s] = bk;
    atomicMax(&a.hdr->best_key, kf_fkey(acc));
}

// ascending bitonic sort of (key, value) pairs by key, P a power of two >= 256, by the 256 threads of the workgroup (bow.hip's bow_sort with
// a payload).  K and V point into LDS or into global scratch.
static __device__ void kf_sort(unsigned long long *K, int *V, int P)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += 256) {
                const int x = t ^ j;
                if (x > t) {
                    const unsigned long long ka = K[t], kb = K[x];
                    if ((ka > kb) == ((t & k) == 0)) { const int va = V[t], vb = V[x]; K[t] = kb; K[x] = ka; V[t] = vb; V[x] = va; }
                }
            }
            __syncthreads();
        }
}

// One workgroup.  The entered slots with acc > 0.75f * bestAccScore are gathered (in any order: the keys are distinct), sorted by the
// discovery key, and an entry is kept when no earlier entry names the same pBestKF (an integer minimum of positions per pBestKF).
__global__ __launch_bounds__(256) void k_kfdb_select(KfArgs a)
{
    __shared__ unsigned long long lkey[KFDB_LDS_SORT];
    __shared__ int lval[KFDB_LDS_SORT];
    __shared__ int sc[257];
    __shared__ int s_n, s_cnt[2];
    const int tid = threadIdx.x;
    const float best_acc = kf_funkey(a.hdr->best_key);
    const float thr = 0.75f * best_acc;                          // float minScoreToRetain = 0.75f*bestAccScore
    if (tid == 0) { s_n = 0; s_cnt[0] = 0; s_cnt[1] = 0; }
    __syncthreads();
    int n_sh = 0, n_sc = 0;                                      // lKFsSharingWords.size() and nscores: integer counts
    for (int s = tid; s < a.n_slots; s += 256) {
        const int e = a.entered[s];
        n_sh += a.words[s] > 0 ? 1 : 0; n_sc += (e >> 1) & 1;
        if ((e & 1) && a.acc[s] > thr) { const int p = atomicAdd(&s_n, 1); a.skey[p] = a.key[s]; a.sval[p] = s; }
    }
    if (n_sh) atomicAdd(&s_cnt[0], n_sh);
    if (n_sc) atomicAdd(&s_cnt[1], n_sc);
    __syncthreads();
    const int n = s_n;
    int P = 256; while (P < n) P <<= 1;                          // n <= n_slots <= KFDB_MAX_SLOTS, a power of two
    unsigned long long *K = a.skey; int *V = a.sval;
    if (P <= KFDB_LDS_SORT) {
        K = lkey; V = lval;
        for (int i = tid; i < P; i += 256) { K[i] = i < n ? a.skey[i] : ~0ull; V[i] = i < n ? a.sval[i] : -1; }
    } else {
        for (int i = n + tid; i < P; i += 256) { K[i] = ~0ull; V[i] = -1; }
    }
    __syncthreads();
    kf_sort(K, V, P);
    for (int p = tid; p < n; p += 256) atomicMin(&a.first_pos[a.best[V[p]]], p);
    __syncthreads();
    const int S = P / 256, p0 = tid * S;
    int c = 0;
    for (int p = p0; p < p0 + S && p < n; p++)
        c += __hip_atomic_load(&a.first_pos[a.best[V[p]]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p ? 1 : 0;
    sc[tid] = c;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int i = 0; i < 256; i++) { const int v = sc[i]; sc[i] = t; t += v; } sc[256] = t; }
    __syncthreads();
    int r = sc[tid];
    for (int p = p0; p < p0 + S && p < n; p++) {
        const int b = a.best[V[p]];
        if (__hip_atomic_load(&a.first_pos[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p) a.cand[r++] = b;
    }
    if (tid == 0) { a.hdr->n_cand = sc[256]; a.hdr->min_common = kf_min_common(a.hdr->max_common); a.hdr->best_acc = best_acc; a.hdr->n_sharing = s_cnt[0]; a.hdr->n_scored = s_cnt[1]; }
    if (sc[256] <= a.cap)                                        // mRelocScore / mLoopScore = si; a refused call leaves them as they were
        for (int s = tid; s < a.n_slots; s += 256)
            if (a.entered[s] & 2) { if (a.mode == HVO_KFDB_LOOP) a.kept[s].y = a.score[s]; else a.kept[s].x = a.score[s]; }
}

// ------------------------------------------------------------------------------------------------ host: storage
static int kf_check_slot(hvo_keyframe_db *db, int slot)
{
    if (slot < 0 || slot >= KFDB_MAX_SLOTS) return kf_fail(db, HVO_ERR_INVALID_ARG, "slot " + std::to_string(slot) + " outside [0, 16384)");
    return HVO_OK;
}

// the slot's record as the host holds it, to the device (through the pinned block); the caller synchronises
static int kf_push_slot(hvo_keyframe_db *db, int slot)
{
    memcpy(db->h_up + KS_CONN, &db->slot[slot], sizeof(KfSlot));
    KF_HIP(hipMemcpyAsync(db->d_slot + slot, db->h_up + KS_CONN, sizeof(KfSlot), hipMemcpyHostToDevice, db->st));
    return HVO_OK;
}

// room for n words in the slot: its own when that is large enough, else a new one at the pool's end (the pool doubles with one device copy)
static int kf_room(hvo_keyframe_db *db, KfSlot &S, int n)
{
    if (S.cap >= n) return HVO_OK;
    const size_t need = ((size_t)std::max(n, 1) + 63) & ~(size_t)63;
    if (db->pool_used + need > db->pool_cap) {
        size_t cap = std::max<size_t>(db->pool_cap * 2, 65536);
        while (cap < db->pool_used + need) cap *= 2;
        int *nw = nullptr; double *nv = nullptr;
        if (hipMalloc((void **)&nw, cap * 4) != hipSuccess || hipMalloc((void **)&nv, cap * 8) != hipSuccess) {
            if (nw) (void)hipFree(nw);
            return kf_fail(db, HVO_ERR_HIP, "hipMalloc of the word pool");
        }
        hipError_t e = hipSuccess;
        if (db->pool_used) {
            e = hipMemcpyAsync(nw, db->d_pw, db->pool_used * 4, hipMemcpyDeviceToDevice, db->st);
            if (e == hipSuccess) e = hipMemcpyAsync(nv, db->d_pv, db->pool_used * 8, hipMemcpyDeviceToDevice, db->st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(db->st);
        if (e != hipSuccess) { (void)hipFree(nw); (void)hipFree(nv); return kf_fail(db, HVO_ERR_HIP, std::string("pool growth: ") + hipGetErrorString(e)); }
        if (db->d_pw) (void)hipFree(db->d_pw);
        if (db->d_pv) (void)hipFree(db->d_pv);
        db->d_pw = nw; db->d_pv = nv; db->pool_cap = cap;
    }
    S.first = (long long)db->pool_used; S.cap = (int)need; db->pool_used += need;
    return HVO_OK;
}

// the checks every add shares; the bag itself is checked by the caller
static int kf_add_check(hvo_keyframe_db *db, int slot, int n_words)
{
    int rc;
    if ((rc = kf_check_slot(db, slot))) return rc;
    if (n_words < 0) return kf_fail(db, HVO_ERR_INVALID_ARG, "a negative word count");
    if (n_words > KFDB_MAX_WORDS) return kf_fail(db, HVO_ERR_UNSUPPORTED, "more than 4096 words in a bag");
    if (db->slot[slot].live) return kf_fail(db, HVO_ERR_INVALID_ARG, "slot " + std::to_string(slot) + " is live (erase it first)");
    return HVO_OK;
}

// a bag as the host passes it: ascending word ids below the vocabulary's word count, finite values >= 0
static int kf_check_bag(hvo_keyframe_db *db, int n, const int32_t *word, const double *value)
{
    if (n < 0) return kf_fail(db, HVO_ERR_INVALID_ARG, "a negative word count");
    if (n > KFDB_MAX_WORDS) return kf_fail(db, HVO_ERR_UNSUPPORTED, "more than 4096 words in a bag");
    if (n > 0 && (!word || !value)) return kf_fail(db, HVO_ERR_INVALID_ARG, "a bag without its arrays");
    for (int i = 0; i < n; i++) {
        if (word[i] < 0 || word[i] >= db->voc_words) return kf_fail(db, HVO_ERR_INVALID_ARG, "word id " + std::to_string(word[i]) + " outside the vocabulary");
        if (i && word[i] <= word[i - 1]) return kf_fail(db, HVO_ERR_INVALID_ARG, "word ids not strictly ascending at position " + std::to_string(i));
        if (!(value[i] >= 0.0) || !std::isfinite(value[i])) return kf_fail(db, HVO_ERR_INVALID_ARG, "a value that is negative or not finite at position " + std::to_string(i));
    }
    return HVO_OK;
}

// after the bag's words lie in the slot's room: the record, the kept scores at 0 (a new key frame; DEFINED BEHAVIOUR, KeyFrame.cc:36 leaves
// them uninitialised), and the one synchronisation of an add
static int kf_add_finish(hvo_keyframe_db *db, int slot, int n_words)
{
    KfSlot &S = db->slot[slot];
    S.count = n_words; S.seq = (int)(db->next_seq & 0x7FFFFFFF); S.live = 1; S.n_nb = 0;
    for (int j = 0; j < KFDB_NB; j++) S.nb[j] = -1;
    int rc;
    if ((rc = kf_push_slot(db, slot))) return rc;
    KF_HIP(hipMemsetAsync(db->d_kept + slot, 0, sizeof(float2), db->st));
    KF_HIP(hipStreamSynchronize(db->st));
    db->next_seq++; db->n_live++; db->n_slots = std::max(db->n_slots, slot + 1);
    return HVO_OK;
}

// ------------------------------------------------------------------------------------------------ host: the query
struct KfQuery {                                                // the bag: on the host (word, value, n) or on the device (d_*)
    int n; const int32_t *word; const double *value;
    const int *d_n; const int *d_word; const double *d_val;
};

static void kf_result_defaults(const hvo_kfdb_params *p, hvo_kfdb_result *res)
{
    res->n_candidates = 0; res->n_sharing = 0; res->max_common = 0; res->min_common = 0; res->n_scored = 0;
    res->best_acc_score = p->mode == HVO_KFDB_LOOP ? p->min_score : 0.f; res->status = HVO_OK;
    const float qnan = nanf("");
    for (int i = 0; i < res->slot_cap; i++) {
        if (res->words) res->words[i] = 0;
        if (res->score) res->score[i] = qnan;
        if (res->acc) res->acc[i] = qnan;
        if (res->best) res->best[i] = -1;
    }
}

static int kf_query(hvo_keyframe_db *db, const KfQuery &q, const hvo_kfdb_params *p, hvo_kfdb_result *res)
{
    if (!p || !res) return kf_fail(db, HVO_ERR_INVALID_ARG, "query without params or result");
    if (p->mode != HVO_KFDB_RELOC && p->mode != HVO_KFDB_LOOP) return kf_fail(db, HVO_ERR_INVALID_ARG, "unknown mode");
    if (db->scoring == HVO_VOC_KL) return kf_fail(db, HVO_ERR_UNSUPPORTED, "KL scoring is not supported (it needs log)");
    if (p->n_connected < 0 || (p->n_connected > 0 && !p->connected)) return kf_fail(db, HVO_ERR_INVALID_ARG, "connected slots: a count without its array");
    if (p->mode == HVO_KFDB_LOOP && !(p->min_score == p->min_score)) return kf_fail(db, HVO_ERR_INVALID_ARG, "min_score is NaN");
    if (res->cap < 0 || (res->cap > 0 && !res->candidate)) return kf_fail(db, HVO_ERR_INVALID_ARG, "candidate array: a capacity without its array");
    const bool views = res->words || res->score || res->acc || res->best;
    if (views && res->slot_cap < db->n_slots) return kf_fail(db, HVO_ERR_INVALID_ARG, "slot_cap below the database's slot count (" + std::to_string(db->n_slots) + ")");
    if (!views && res->slot_cap < 0) return kf_fail(db, HVO_ERR_INVALID_ARG, "a negative slot_cap");
    int rc;
    if (!q.d_word && (rc = kf_check_bag(db, q.n, q.word, q.value))) return rc;
    kf_result_defaults(p, res);
    db->last_ms = 0.f;
    const int ns = db->n_slots;
    if (db->n_live == 0 || (!q.d_word && q.n == 0)) return HVO_OK;       // (the reference's first early return)
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    // ---- one upload
    char *u = db->h_up, *d = db->d_scr;
    KfHdr h0; memset(&h0, 0, sizeof(h0));
    h0.best_key = kf_fkey(p->mode == HVO_KFDB_LOOP ? p->min_score : 0.f); h0.q_n = q.n;
    const size_t o_conn = KS_RES - (((size_t)ns + 63) & ~(size_t)63);                       // slot s's byte at o_conn + s, the header right behind the bytes
    memcpy(u + KS_RES, &h0, sizeof(h0));
    memset(u + o_conn, 0, KS_RES - o_conn);
    if (p->mode == HVO_KFDB_LOOP) for (int i = 0; i < p->n_connected; i++) { const int c = p->connected[i]; if (c >= 0 && c < ns) u[o_conn + c] = 1; }
    KF_HIP(hipMemcpyAsync(d + o_conn, u + o_conn, KS_UP_END - o_conn, hipMemcpyHostToDevice, db->st));
    if (!q.d_word) {                                             // the host form's bag (the used part of its two arrays)
        memcpy(u + KS_QWORD, q.word, (size_t)q.n * 4); memcpy(u + KS_QVAL, q.value, (size_t)q.n * 8);
        KF_HIP(hipMemcpyAsync(d + KS_QWORD, u + KS_QWORD, (size_t)q.n * 4, hipMemcpyHostToDevice, db->st));
        KF_HIP(hipMemcpyAsync(d + KS_QVAL, u + KS_QVAL, (size_t)q.n * 8, hipMemcpyHostToDevice, db->st));
    }
    // ---- the kernels
    char *r = d + KS_RES;
    const size_t stride = ((size_t)ns * 4 + 63) & ~(size_t)63;   // the result block's arrays at this call's slot count: one copy down
    KfArgs a; memset(&a, 0, sizeof(a));
    a.slot = db->d_slot; a.kept = db->d_kept; a.pw = db->d_pw; a.pv = db->d_pv;
    a.q_n = q.d_word ? q.d_n : &((const KfHdr *)r)->q_n; a.q_word = q.d_word ? q.d_word : (const int *)(d + KS_QWORD); a.q_val = q.d_word ? q.d_val : (const double *)(d + KS_QVAL);
    a.n_slots = ns; a.mode = p->mode; a.scoring = db->scoring; a.cap = res->cap; a.min_score = p->min_score;
    a.hdr = (KfHdr *)r; a.cand = (int *)(r + 64); a.words = (int *)(r + 64 + stride); a.score = (float *)(r + 64 + 2 * stride);
    a.acc = (float *)(r + 64 + 3 * stride); a.best = (int *)(r + 64 + 4 * stride);
    a.key = (unsigned long long *)(d + KS_KEY); a.entered = (uint8_t *)(d + KS_ENTERED); a.conn = (const uint8_t *)(d + o_conn); a.first_pos = (int *)(d + KS_FIRST);
    a.skey = (unsigned long long *)(d + KS_SKEY); a.sval = (int *)(d + KS_SVAL);
    const bool timed = hipEventRecord(db->ev[0], db->st) == hipSuccess;
    const int nb = (ns + KFDB_SPB - 1) / KFDB_SPB;
    hipLaunchKernelGGL(k_kfdb_common, dim3(nb), dim3(256), 0, db->st, a);
    hipLaunchKernelGGL(k_kfdb_score, dim3(nb), dim3(256), 0, db->st, a);
    hipLaunchKernelGGL(k_kfdb_accumulate, dim3((ns + 255) / 256), dim3(256), 0, db->st, a);
    hipLaunchKernelGGL(k_kfdb_select, dim3(1), dim3(256), 0, db->st, a);
    const bool timed1 = timed && hipEventRecord(db->ev[1], db->st) == hipSuccess;
    KF_HIP(hipGetLastError());
    // ---- one download, one synchronisation
    const size_t down = 64 + (views ? 5 : 1) * stride;
    KF_HIP(hipMemcpyAsync(db->h_res, r, down, hipMemcpyDeviceToHost, db->st));
    KF_HIP(hipStreamSynchronize(db->st));
    if (timed1 && hipEventElapsedTime(&db->last_ms, db->ev[0], db->ev[1]) != hipSuccess) db->last_ms = 0.f;
    const KfHdr *H = (const KfHdr *)db->h_res;
    if (H->n_cand > res->cap) {                                  // refused whole: k_kfdb_select has left the kept scores as they were
        kf_result_defaults(p, res);
        res->n_candidates = H->n_cand;
        return kf_fail(db, HVO_ERR_CAPACITY, "cap " + std::to_string(res->cap) + " below the " + std::to_string(H->n_cand) + " candidates");
    }
    res->n_candidates = H->n_cand; res->n_sharing = H->n_sharing; res->max_common = H->max_common; res->min_common = H->min_common; res->n_scored = H->n_scored;
    res->best_acc_score = H->best_acc;
    if (H->n_cand) memcpy(res->candidate, db->h_res + 64, (size_t)H->n_cand * 4);
    if (res->words) memcpy(res->words, db->h_res + 64 + stride, (size_t)ns * 4);
    if (res->score) memcpy(res->score, db->h_res + 64 + 2 * stride, (size_t)ns * 4);
    if (res->acc) memcpy(res->acc, db->h_res + 64 + 3 * stride, (size_t)ns * 4);
    if (res->best) memcpy(res->best, db->h_res + 64 + 4 * stride, (size_t)ns * 4);
    return HVO_OK;
}

// a resident frame's bag of words (frame f of the block) as the query or the add reads it; refuses a block that holds none for voc
static int kf_resident_bag(hvo_keyframe_db *db, const hvo_vocabulary *voc, const BowState *b, int f, KfQuery &q)
{
    if (bow_voc_uid(voc) != db->voc_uid) return kf_fail(db, HVO_ERR_INVALID_ARG, "the database was created for another vocabulary");
    if (!b || !b->valid || b->voc_uid != db->voc_uid || f >= b->n)
        return kf_fail(db, HVO_ERR_INVALID_ARG, "the frame holds no bag of words of this vocabulary (compute it first)");
    BowLayout L; bow_layout(b->cap, L);
    const char *blk = b->d_blk + (size_t)f * L.total;
    memset(&q, 0, sizeof(q));
    q.d_n = (const int *)(blk + L.counts) + 1; q.d_word = (const int *)(blk + L.bow_word); q.d_val = (const double *)(blk + L.bow_val);
    return HVO_OK;
}

// ------------------------------------------------------------------------------------------------ the C ABI
extern "C" {

int hvo_keyframe_db_create(const hvo_vocabulary *voc, hvo_keyframe_db **out)
{
    if (!out) return HVO_ERR_INVALID_ARG;
    *out = nullptr;
    if (!voc) return HVO_ERR_INVALID_ARG;
    hvo_vocabulary_desc vd;
    if (hvo_vocabulary_info(voc, &vd) != HVO_OK || vd.device < 0) return HVO_ERR_INVALID_ARG;    // a host-only vocabulary computes nothing
    if (hipSetDevice(vd.device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    hvo_keyframe_db *db = new (std::nothrow) hvo_keyframe_db();
    if (!db) return HVO_ERR_HIP;
    db->device = vd.device; db->scoring = vd.scoring; db->voc_words = vd.n_words; db->voc_uid = bow_voc_uid(voc);
    try { db->slot.assign(KFDB_MAX_SLOTS, KfSlot()); } catch (const std::bad_alloc &) { delete db; return HVO_ERR_HIP; }
    for (KfSlot &S : db->slot) { memset(&S, 0, sizeof(S)); for (int j = 0; j < KFDB_NB; j++) S.nb[j] = -1; }
    bool ok = hipStreamCreateWithFlags(&db->st, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreate(&db->ev[0]) == hipSuccess && hipEventCreate(&db->ev[1]) == hipSuccess;
    ok = ok && hipMalloc((void **)&db->d_slot, sizeof(KfSlot) * KFDB_MAX_SLOTS) == hipSuccess;
    ok = ok && hipMalloc((void **)&db->d_kept, sizeof(float2) * KFDB_MAX_SLOTS) == hipSuccess;
    ok = ok && hipMalloc((void **)&db->d_scr, KS_TOTAL) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&db->h_up, KFDB_UP_BYTES) == hipSuccess && hipHostMalloc((void **)&db->h_res, KS_RES_BYTES) == hipSuccess;
    ok = ok && hipMemsetAsync(db->d_slot, 0, sizeof(KfSlot) * KFDB_MAX_SLOTS, db->st) == hipSuccess;
    ok = ok && hipMemsetAsync(db->d_kept, 0, sizeof(float2) * KFDB_MAX_SLOTS, db->st) == hipSuccess;
    ok = ok && hipStreamSynchronize(db->st) == hipSuccess;
    if (!ok) { hvo_keyframe_db_destroy(db); return HVO_ERR_HIP; }
    *out = db;
    return HVO_OK;
}

void hvo_keyframe_db_destroy(hvo_keyframe_db *db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->st) (void)hipStreamSynchronize(db->st);
    for (void *p : { (void *)db->d_slot, (void *)db->d_kept, (void *)db->d_pw, (void *)db->d_pv, (void *)db->d_scr }) if (p) (void)hipFree(p);
    if (db->h_up) (void)hipHostFree(db->h_up);
    if (db->h_res) (void)hipHostFree(db->h_res);
    for (hipEvent_t e : db->ev) if (e) (void)hipEventDestroy(e);
    if (db->st) (void)hipStreamDestroy(db->st);
    delete db;
}

const char *hvo_keyframe_db_last_error(const hvo_keyframe_db *db) { return db ? db->last_error.c_str() : "null database"; }

// KeyFrameDatabase::add: the slot's bag of words, ascending word ids as hvo_bow returns them
int hvo_keyframe_db_add(hvo_keyframe_db *db, int slot, int n_words, const int32_t *word, const double *value)
{
    if (!db) return HVO_ERR_INVALID_ARG;
    int rc;
    if ((rc = kf_add_check(db, slot, n_words)) || (rc = kf_check_bag(db, n_words, word, value))) return rc;
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    KfSlot &S = db->slot[slot];
    if ((rc = kf_room(db, S, n_words))) return rc;
    if (n_words) {
        memcpy(db->h_up + KS_QWORD, word, (size_t)n_words * 4); memcpy(db->h_up + KS_QVAL, value, (size_t)n_words * 8);
        KF_HIP(hipMemcpyAsync(db->d_pw + S.first, db->h_up + KS_QWORD, (size_t)n_words * 4, hipMemcpyHostToDevice, db->st));
        KF_HIP(hipMemcpyAsync(db->d_pv + S.first, db->h_up + KS_QVAL, (size_t)n_words * 8, hipMemcpyHostToDevice, db->st));
    }
    return kf_add_finish(db, slot, n_words);
}

// the same with the bag hvo_stream_compute_bow left on the frame `ticket`: device to device, only the word count comes down
int hvo_stream_keyframe_db_add(hvo_stream *s, int64_t ticket, const hvo_vocabulary *voc, hvo_keyframe_db *db, int slot)
{
    if (!s || !voc || !db) return HVO_ERR_INVALID_ARG;
    int rc;
    if (db->device != s->p.device) return kf_fail(db, HVO_ERR_INVALID_ARG, "the database lives on another device than the stream");
    StreamSlot *F = slot_of(s, ticket);
    KfQuery q;
    if ((rc = kf_resident_bag(db, voc, F ? &F->bow : nullptr, 0, q))) { s->last_error = db->last_error; return rc; }
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    int *hn = (int *)db->h_res;
    KF_HIP(hipMemcpyAsync(hn, q.d_n, 4, hipMemcpyDeviceToHost, db->st));
    KF_HIP(hipStreamSynchronize(db->st));
    const int n = *hn;
    if (n < 0 || n > F->bow.cap) return kf_fail(db, HVO_ERR_HIP, "the frame's bag of words holds an impossible count");
    if ((rc = kf_add_check(db, slot, n))) return rc;
    KfSlot &S = db->slot[slot];
    if ((rc = kf_room(db, S, n))) return rc;
    if (n) {
        KF_HIP(hipMemcpyAsync(db->d_pw + S.first, q.d_word, (size_t)n * 4, hipMemcpyDeviceToDevice, db->st));
        KF_HIP(hipMemcpyAsync(db->d_pv + S.first, q.d_val, (size_t)n * 8, hipMemcpyDeviceToDevice, db->st));
    }
    return kf_add_finish(db, slot, n);
}

// KeyFrameDatabase::erase: the slot takes part in nothing any more; its room stays with it for the next add.  Erasing a slot that is not live does nothing.
int hvo_keyframe_db_erase(hvo_keyframe_db *db, int slot)
{
    if (!db) return HVO_ERR_INVALID_ARG;
    int rc;
    if ((rc = kf_check_slot(db, slot))) return rc;
    KfSlot &S = db->slot[slot];
    if (!S.live) return HVO_OK;
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    S.live = 0; S.count = 0; S.n_nb = 0;
    if ((rc = kf_push_slot(db, slot))) return rc;
    KF_HIP(hipStreamSynchronize(db->st));
    db->n_live--;
    return HVO_OK;
}

// KeyFrameDatabase::clear: every slot dead, the pool empty (its memory is kept)
int hvo_keyframe_db_clear(hvo_keyframe_db *db)
{
    if (!db) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    KF_HIP(hipMemsetAsync(db->d_slot, 0, sizeof(KfSlot) * KFDB_MAX_SLOTS, db->st));
    KF_HIP(hipMemsetAsync(db->d_kept, 0, sizeof(float2) * KFDB_MAX_SLOTS, db->st));
    KF_HIP(hipStreamSynchronize(db->st));
    for (KfSlot &S : db->slot) { memset(&S, 0, sizeof(S)); for (int j = 0; j < KFDB_NB; j++) S.nb[j] = -1; }
    db->n_slots = 0; db->n_live = 0; db->pool_used = 0;
    return HVO_OK;
}

// the slot's neighbours as GetBestCovisibilityKeyFrames(10) returns them, in that order; ids are kept as passed (a query skips what is out of range or erased)
int hvo_keyframe_db_set_covisible(hvo_keyframe_db *db, int slot, int n, const int32_t *slots)
{
    if (!db) return HVO_ERR_INVALID_ARG;
    int rc;
    if ((rc = kf_check_slot(db, slot))) return rc;
    if (n < 0 || n > KFDB_NB || (n > 0 && !slots)) return kf_fail(db, HVO_ERR_INVALID_ARG, "between 0 and 10 neighbours, with their array");
    KfSlot &S = db->slot[slot];
    if (!S.live) return kf_fail(db, HVO_ERR_INVALID_ARG, "slot " + std::to_string(slot) + " is not live");
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    S.n_nb = n;
    for (int j = 0; j < KFDB_NB; j++) S.nb[j] = j < n ? slots[j] : -1;
    if ((rc = kf_push_slot(db, slot))) return rc;
    KF_HIP(hipStreamSynchronize(db->st));
    return HVO_OK;
}

// read-back of a live slot as the device holds it: its bag and the two kept scores (reloc, loop)
int hvo_keyframe_db_get(const hvo_keyframe_db *cdb, int slot, int cap, int32_t *word, double *value, int32_t *n_words, float score2[2])
{
    hvo_keyframe_db *db = const_cast<hvo_keyframe_db *>(cdb);   // (last_error and the staging are written)
    if (!db) return HVO_ERR_INVALID_ARG;
    int rc;
    if ((rc = kf_check_slot(db, slot))) return rc;
    const KfSlot &S = db->slot[slot];
    if (!S.live) return kf_fail(db, HVO_ERR_INVALID_ARG, "slot " + std::to_string(slot) + " is not live");
    if (n_words) *n_words = S.count;
    if ((word || value) && cap < S.count) return kf_fail(db, HVO_ERR_CAPACITY, "cap below the slot's word count");
    if (hipSetDevice(db->device) != hipSuccess) return kf_fail(db, HVO_ERR_NO_DEVICE, "hipSetDevice");
    char *h = db->h_res;
    KF_HIP(hipMemcpyAsync(h, db->d_kept + slot, sizeof(float2), hipMemcpyDeviceToHost, db->st));
    if (S.count && word) KF_HIP(hipMemcpyAsync(h + 64, db->d_pw + S.first, (size_t)S.count * 4, hipMemcpyDeviceToHost, db->st));
    if (S.count && value) KF_HIP(hipMemcpyAsync(h + 64 + KFDB_MAX_WORDS * 4, db->d_pv + S.first, (size_t)S.count * 8, hipMemcpyDeviceToHost, db->st));
    KF_HIP(hipStreamSynchronize(db->st));
    if (score2) memcpy(score2, h, 8);
    if (S.count && word) memcpy(word, h + 64, (size_t)S.count * 4);
    if (S.count && value) memcpy(value, h + 64 + KFDB_MAX_WORDS * 4, (size_t)S.count * 8);
    return HVO_OK;
}

int hvo_keyframe_db_info(const hvo_keyframe_db *db, hvo_keyframe_db_desc *info)
{
    if (!db || !info) return HVO_ERR_INVALID_ARG;
    info->n_slots = db->n_slots; info->n_live = db->n_live; info->scoring = db->scoring; info->device = db->device;
    info->pooled_words = (int64_t)db->pool_used; info->pool_capacity = (int64_t)db->pool_cap; info->next_sequence = (int64_t)db->next_seq;
    return HVO_OK;
}

// DetectRelocalizationCandidates / DetectLoopCandidates with the bag on the host
int hvo_keyframe_db_query(hvo_keyframe_db *db, int n_words, const int32_t *word, const double *value, const hvo_kfdb_params *p, hvo_kfdb_result *res)
{
    if (!db) return HVO_ERR_INVALID_ARG;
    KfQuery q; memset(&q, 0, sizeof(q));
    q.n = n_words; q.word = word; q.value = value;
    return kf_query(db, q, p, res);
}

// the same with the bag hvo_stream_compute_bow left on the frame `ticket`: nothing of the bag crosses the bus
int hvo_stream_keyframe_db_query(hvo_stream *s, int64_t ticket, const hvo_vocabulary *voc, hvo_keyframe_db *db, const hvo_kfdb_params *p, hvo_kfdb_result *res)
{
    if (!s || !voc || !db) return HVO_ERR_INVALID_ARG;
    if (db->device != s->p.device) return kf_fail(db, HVO_ERR_INVALID_ARG, "the database lives on another device than the stream");
    StreamSlot *F = slot_of(s, ticket);
    KfQuery q; int rc;
    if ((rc = kf_resident_bag(db, voc, F ? &F->bow : nullptr, 0, q)) || (rc = kf_query(db, q, p, res))) s->last_error = db->last_error;
    return rc;
}

// frames 0 .. n-1 of the resident batch (hvo_batch_compute_bow), one query after the other in that order: the kept scores make the order matter
int hvo_batch_keyframe_db_query(hvo_ctx *ctx, const hvo_vocabulary *voc, hvo_keyframe_db *db, int n, const hvo_kfdb_params *p, hvo_kfdb_result *res)
{
    if (!ctx || !voc || !db) return HVO_ERR_INVALID_ARG;
    int rc = HVO_OK;
    if (n < 1 || !p || !res) rc = kf_fail(db, HVO_ERR_INVALID_ARG, "batch query: n >= 1 with n params and n results");
    else if (db->device != ctx->device) rc = kf_fail(db, HVO_ERR_INVALID_ARG, "the database lives on another device than the context");
    for (int f = 0; f < n && !rc; f++) {
        KfQuery q;
        if (!(rc = kf_resident_bag(db, voc, &ctx->bow_batch, f, q))) rc = kf_query(db, q, p + f, res + f);
    }
    if (rc) ctx->last_error = db->last_error;
    return rc;
}

// device time of the last query's four kernels (0 when it launched nothing)
int hvo_keyframe_db_last_kernel_ms(const hvo_keyframe_db *db, float *ms)
{
    if (!db || !ms) return HVO_ERR_INVALID_ARG;
    *ms = db->last_ms;
    return HVO_OK;
}

}   // extern "C"
