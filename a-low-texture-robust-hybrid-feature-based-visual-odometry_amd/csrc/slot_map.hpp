// slot_map.hpp -- what the resident point map (local_points.hip) and the resident line map (local_lines.hip) have in common: the storage of
// a map of slots, the skeleton of a call against it, and the device pieces both calls' kernels are built from.  slot_map.hip holds the host
// functions and the three kernels that are the same for both maps (mark, fill, assign).
//
// Storage.  A map is a table of arrays, each `comps` components of `elem` bytes, component-major over `cap` slots (component c of slot j at
// element [c * cap + j]), with a fill byte for slots nobody has set.  The packed 32-byte descriptor is an array with elem = 32, comps = 1.
// The last array is the flag byte (bit 0 bad, bit 1 has observations; fill = bad).  The host mirror is the truth; storage grows only, by a
// new allocation of every array and one upload of the mirror.  A map adds its table, its typed accessors and the per-slot copies of
// set_many / slot; a call adds its frustum test, its gather, its search and its post stage.
#pragma once
#include "hvo_internal.hpp"
#include "call_stage.hpp"
#include "map_gates.hpp"      // sm_level, sm_predict_level .. sm_pinhole, ham256
#include <string>
#include <vector>

#define SM_BLOCK 256
#define SM_BAD 1
#define SM_OBS 2

struct SmPose { float R[9], t[3], Ow[3], pad; };
struct SmArray { int elem, comps; uint8_t fill; std::vector<uint8_t> h; void *d; };

struct hvo_slot_map {
    const char *name, *max_name; int max_slots;                  // "line map", "HVO_LINE_MAP_MAX_SLOTS" and its value, for the messages
    std::vector<SmArray> arr;                                    // the flags last
    int device = 0;
    hipStream_t st = nullptr;                                    // the map's own uploads
    int n_slots = 0, cap = 0;
    char *d_a = nullptr, *d_b = nullptr; size_t a_bytes = 0, b_bytes = 0;    // the calls' scratch (before / after the in-view counts), grow-only
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
    // the last call's poses: the source of an asynchronous copy, so it outlives the call's helpers.  A call that fails between sm_stage_in
    // and sm_counts_down (only after a HIP failure) returns without draining its stream; the next call may then rewrite this while that
    // copy is pending -- its results were refused anyway.
    std::vector<SmPose> pose;
    std::string last_error;
    hvo_slot_map(const char *name_, const char *max_name_, int max_slots_, std::vector<SmArray> arr_) : name(name_), max_name(max_name_), max_slots(max_slots_), arr(std::move(arr_)) {}
    template <class T> T *host(int k) const { return (T *)arr[k].h.data(); }       // array k of the mirror / of the device, typed
    template <class T> T *dev(int k) const { return (T *)arr[k].d; }
    uint8_t *h_flags() const { return (uint8_t *)arr.back().h.data(); }
    uint8_t *d_flags() const { return (uint8_t *)arr.back().d; }
};

// the resident point map (local_points.hip owns its calls; fuse.hip reads its arrays in place, map_refresh.hip rewrites them)
struct hvo_point_map : hvo_slot_map {
    hvo_point_map() : hvo_slot_map("point map", "HVO_POINT_MAP_MAX_SLOTS", HVO_POINT_MAP_MAX_SLOTS, { { 4, 3 }, { 4, 3 }, { 4, 1 }, { 4, 1 }, { 32, 1 }, { 1, 1, SM_BAD } }) {}
    enum { POS, NRM, MAXD, MIND, DESC };                         // pos, nrm, maxd, mind: floats; desc: 32 bytes packed; then the flags
};

// the resident line map (local_lines.hip owns its calls; map_refresh.hip rewrites its arrays in place)
struct hvo_line_map : hvo_slot_map {
    hvo_line_map() : hvo_slot_map("line map", "HVO_LINE_MAP_MAX_SLOTS", HVO_LINE_MAP_MAX_SLOTS, { { 8, 6 }, { 8, 3 }, { 8, 3 }, { 4, 1 }, { 4, 1 }, { 32, 1 }, { 1, 1, SM_BAD } }) {}
    enum { POS, WVEC, NRM, MAXD, MIND, DESC };                   // pos, wvec, nrm: doubles; maxd, mind: floats; desc: 32 bytes packed; then the flags
};

#define SM_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { m->last_error = std::string(#call) + ": " + hipGetErrorString(e_); return HVO_ERR_HIP; } } while (0)

// ---- the map (slot_map.hip) ----
int sm_init(hvo_slot_map *m, int device, int slots);             // stream, events, room for `slots`; on failure the caller destroys the map
void sm_release(hvo_slot_map *m);                                // everything but the object itself
// set_many in two halves around the caller's typed copy loop: sm_set_begin validates and makes room (the caller returns its value when it
// is not HVO_OK or n == 0); sm_set_end moves n_slots and uploads.  sm_flag_byte is slot i's flag byte from the caller's optional arrays.
int sm_set_begin(hvo_slot_map *m, int first, int n, bool all_given, bool *regrown);
int sm_set_end(hvo_slot_map *m, int first, int n, bool regrown);
static inline uint8_t sm_flag_byte(const uint8_t *observed, const uint8_t *bad, int i) { return (uint8_t)(((bad && bad[i]) ? SM_BAD : 0) | ((!observed || observed[i]) ? SM_OBS : 0)); }
int sm_set_flag(hvo_slot_map *m, int slot, int bit, int on);
int sm_counts(const hvo_slot_map *m, int *n_slots, int *n_good, int *n_observed);
int sm_grow(hvo_slot_map *m, hipStream_t st, char **p, size_t *have, size_t want);
int sm_debug_fill_scratch(hvo_slot_map *m, int fill_byte);      // test door: d_a and d_b at their current sizes

// ---- the call (slot_map.hip) ----
struct SmCarve : StageCarver { SmCarve() : StageCarver(256) {} size_t take(size_t bytes) { return StageCarver::take<char>(bytes).off; } };    // 256-byte pieces of scratch A, by their offsets
// one frame's side of the stage before the in-view counts: nt features with their held slots, ne seen_extra slots, and where they live in scratch A
struct SmFrame { int nt, ne; const int32_t *held, *extra; size_t o_held, o_occ, o_ex, o_win; };
// held below held_min or beyond the map, seen_extra outside the map: last_error = prefix + ": " + text, HVO_ERR_INVALID_ARG
int sm_check_seen(hvo_slot_map *m, const char *prefix, const char *held_text, int held_min, const SmFrame &f);
void sm_carve_frame(SmCarve &c, SmFrame &f);
// the uploads (held, seen_extra, and the poses built into m->pose: Rcw, tcw, mOw = -Rcw^T tcw), the zeroed seen bytes and counts, win = -1.
// The caller's own memsets follow it, not precede it: a copy from pageable memory waits for what the stream holds, so every memset in
// front of the first copy costs a round trip.  Then sm_mark: ev[0] and one mark launch per frame
int sm_stage_in(hvo_slot_map *m, hipStream_t st, char *A, size_t o_pose, size_t o_seen, size_t o_cnt, const std::vector<SmFrame> &fr, const float *Tcw);
int sm_mark(hvo_slot_map *m, hipStream_t st, char *A, size_t o_seen, const std::vector<SmFrame> &fr, int foreign_observed);
// after the caller's frustum and compaction launches: the launch check, ev[1], cnt = nview (nframes) then ntested (nframes), stream drained
int sm_counts_down(hvo_slot_map *m, hipStream_t st, const char *launch_text, const char *d_cnt, int nframes, std::vector<int> &cnt);
void sm_kernel_ms(hvo_slot_map *m, float ms[3]);                  // the three intervals between the four events
// the shared kernels, through enqueue functions (the idiom of match_sbp_enqueue); a launch failure shows in the caller's hipGetLastError
void sm_fill_enqueue(hipStream_t st, int n, int32_t *idx, int32_t *dist);                         // idx = -1, dist = 256
void sm_assign_enqueue(hipStream_t st, int nq, int nt, const int32_t *match_idx, int *win);       // win[match_idx[q]] = max q

// one row of Rcw * X + tcw: the reading of k_project_last (match.hip's gemm3_row)
static __device__ __forceinline__ float sm_row(const float *a, float b0, float b1, float b2, float c)
{
    float t = __fmul_rn(a[0], b0); t = __fadd_rn(t, __fmul_rn(a[1], b1)); t = __fadd_rn(t, __fmul_rn(a[2], b2));
    return (float)((double)t * 1.0 + (double)c * 1.0);
}

// the end of a frustum kernel's round for one frame: the slot's pass flag, the block's survivors and the frame's tested slots
static __device__ __forceinline__ void sm_frustum_tail(bool in, bool pass, bool tested, uint8_t *passflag, int *blockcnt, int *ntested)
{
    if (in) *passflag = pass ? 1 : 0;
    const int np = __syncthreads_count(pass), nt = __syncthreads_count(tested);
    if (threadIdx.x == 0) { *blockcnt = np; if (nt) atomicAdd(ntested, nt); }
}

// the compaction's position, grid (nblocks, frames): *p = this lane's slot passed under frame f; returned is its place among the frame's
// survivors in ASCENDING SLOT ORDER = (sum of the counts of the blocks before) + (wave ballot prefix inside the block).  No atomic decides
// an order.  The last block writes the frame's total.
static __device__ __forceinline__ int sm_compact_pos(const int *blockcnt, int nblocks, int ns, int f, const uint8_t *pass, int *nview, bool *passed)
{
    __shared__ int red[SM_BLOCK / 64], wcnt[SM_BLOCK / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // survivors of the blocks before this one (an integer sum: any order)
    int s = 0;
    for (int k = tid; k < b; k += SM_BLOCK) s += blockcnt[(size_t)f * nblocks + k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const int j = b * SM_BLOCK + tid;
    const size_t src = (size_t)f * ns + (j < ns ? j : 0);
    const bool p = j < ns && pass[src];
    const unsigned long long bm = __ballot(p);
    if (lane == 0) { red[wave] = s; wcnt[wave] = __popcll(bm); }
    __syncthreads();
    int off = 0, before = 0, total = 0;
    for (int w = 0; w < SM_BLOCK / 64; w++) { off += red[w]; before += w < wave ? wcnt[w] : 0; total += wcnt[w]; }
    if (b == nblocks - 1 && tid == 0) nview[f] = off + total;
    *passed = p;
    return off + before + __popcll(bm & ((1ull << lane) - 1ull));
}
