// slot_map.hip -- the host functions and the kernels that the resident point map and the resident line map share (slot_map.hpp says what a
// slot map is; local_points.hip and local_lines.hip say what each adds).
//   k_sm_mark      per frame feature: a held slot that is bad becomes -1; t_occupied = the held slot has observations (or, for the point map,
//                  held is HVO_HELD_FOREIGN_OBSERVED); the held slots and the caller's seen_extra slots are marked seen (plain byte stores of 1)
//   k_sm_fill      match_idx = -1, match_dist = 256
//   k_sm_assign    F.mvpMap...[bestIdx] = the query's slot in query order: the LAST query that matched a feature keeps it, taken as an atomicMax
//                  of the query index per feature (a maximum does not depend on the order of its operands)
#include "slot_map.hpp"
#include <string.h>

static void sm_free_device(hvo_slot_map *m)
{
    for (SmArray &a : m->arr) { if (a.d) (void)hipFree(a.d); a.d = nullptr; }
}

// slots [first, first + n) of the host mirror -> device, array by array, component by component
static int sm_upload(hvo_slot_map *m, int first, int n)
{
    if (n <= 0) return HVO_OK;
    for (SmArray &a : m->arr)
        for (int k = 0; k < a.comps; k++) {
            const size_t at = ((size_t)k * m->cap + first) * a.elem;
            SM_HIP(hipMemcpyAsync((char *)a.d + at, a.h.data() + at, (size_t)n * a.elem, hipMemcpyHostToDevice, m->st));
        }
    SM_HIP(hipStreamSynchronize(m->st));
    return HVO_OK;
}

// room for `want` slots.  The new device arrays are allocated first: when one allocation fails nothing of the map has changed.  After a
// regrowth (*regrown) the device arrays are empty and the caller uploads every slot in use.
static int sm_reserve(hvo_slot_map *m, int want, bool *regrown)
{
    *regrown = false;
    if (want <= m->cap) return HVO_OK;
    int cap = std::max(m->cap, 64);
    while (cap < want) cap *= 2;
    std::vector<void *> nd(m->arr.size(), nullptr);
    for (size_t k = 0; k < nd.size(); k++)
        if (hipMalloc(&nd[k], (size_t)cap * m->arr[k].comps * m->arr[k].elem) != hipSuccess) {
            for (size_t q = 0; q < k; q++) (void)hipFree(nd[q]);
            m->last_error = std::string(m->name) + ": hipMalloc of the slot arrays"; return HVO_ERR_HIP;
        }
    std::vector<std::vector<uint8_t>> nh(nd.size());            // the mirror moves to the new component stride; built whole before anything changes
    for (size_t k = 0; k < nd.size(); k++) {
        const SmArray &a = m->arr[k];
        nh[k].assign((size_t)cap * a.comps * a.elem, a.fill);
        for (int c = 0; c < a.comps && m->n_slots; c++) memcpy(&nh[k][(size_t)c * cap * a.elem], a.h.data() + (size_t)c * m->cap * a.elem, (size_t)m->n_slots * a.elem);
    }
    sm_free_device(m);
    for (size_t k = 0; k < nd.size(); k++) { m->arr[k].h.swap(nh[k]); m->arr[k].d = nd[k]; }
    m->cap = cap; *regrown = true;
    return HVO_OK;
}

int sm_init(hvo_slot_map *m, int device, int slots)
{
    m->device = device;
    if (hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) != hipSuccess) { m->st = nullptr; return HVO_ERR_HIP; }
    for (int k = 0; k < 4; k++) if (hipEventCreate(&m->ev[k]) != hipSuccess) { m->ev[k] = nullptr; return HVO_ERR_HIP; }
    bool regrown;
    return sm_reserve(m, std::max(slots, 1), &regrown);
}

void sm_release(hvo_slot_map *m)
{
    (void)hipSetDevice(m->device);
    if (m->st) { (void)hipStreamSynchronize(m->st); (void)hipStreamDestroy(m->st); }
    for (int k = 0; k < 4; k++) if (m->ev[k]) (void)hipEventDestroy(m->ev[k]);
    sm_free_device(m);
    if (m->d_a) (void)hipFree(m->d_a);
    if (m->d_b) (void)hipFree(m->d_b);
}

int sm_set_begin(hvo_slot_map *m, int first, int n, bool all_given, bool *regrown)
{
    if (!m || first < 0 || n < 0) return HVO_ERR_INVALID_ARG;
    if ((int64_t)first + n > m->max_slots) { m->last_error = std::string(m->name) + ": more than " + m->max_name + " slots"; return HVO_ERR_UNSUPPORTED; }
    if (n == 0) return HVO_OK;
    if (!all_given) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    return sm_reserve(m, first + n, regrown);
}

int sm_set_end(hvo_slot_map *m, int first, int n, bool regrown)
{
    const int old = m->n_slots;                                  // the slots skipped over stay bad (the mirror's default)
    if (first + n > m->n_slots) m->n_slots = first + n;
    if (regrown) return sm_upload(m, 0, m->n_slots);             // fresh device arrays: every slot in use, once
    const int lo = std::min(first, old), hi = first + n;
    return sm_upload(m, lo, hi - lo);
}

int sm_set_flag(hvo_slot_map *m, int slot, int bit, int on)
{
    if (!m || slot < 0 || slot >= m->n_slots) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    uint8_t *fl = m->h_flags();
    fl[slot] = (uint8_t)(on ? (fl[slot] | bit) : (fl[slot] & ~bit));
    SM_HIP(hipMemcpyAsync(m->d_flags() + slot, &fl[slot], 1, hipMemcpyHostToDevice, m->st));
    SM_HIP(hipStreamSynchronize(m->st));
    return HVO_OK;
}

int sm_counts(const hvo_slot_map *m, int *n_slots, int *n_good, int *n_observed)
{
    if (!m) return HVO_ERR_INVALID_ARG;
    const uint8_t *fl = m->h_flags();
    int g = 0, o = 0;
    for (int j = 0; j < m->n_slots; j++) { g += (fl[j] & SM_BAD) ? 0 : 1; o += (fl[j] & SM_OBS) ? 1 : 0; }
    if (n_slots) *n_slots = m->n_slots;
    if (n_good) *n_good = g;
    if (n_observed) *n_observed = o;
    return HVO_OK;
}

int sm_grow(hvo_slot_map *m, hipStream_t st, char **p, size_t *have, size_t want)
{
    if (*have >= want) return HVO_OK;
    SM_HIP(hipStreamSynchronize(st));
    if (*p) (void)hipFree(*p);
    *p = nullptr; *have = 0;
    size_t c = 1 << 20;
    while (c < want) c *= 2;
    SM_HIP(hipMalloc((void **)p, c));
    *have = c;
    return HVO_OK;
}

// Test door behind hvo_debug_point_map_scratch / hvo_debug_line_map_scratch (not product API): both scratch buffers, at the sizes they have,
// set to fill_byte on the map's own stream, which is drained before it returns
int sm_debug_fill_scratch(hvo_slot_map *m, int fill_byte)
{
    if (!m || fill_byte < 0 || fill_byte > 255) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(m->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    SM_HIP(hipDeviceSynchronize());                              // a call's stream is the caller's: nothing of it may still be in flight
    if (m->d_a && m->a_bytes) SM_HIP(hipMemsetAsync(m->d_a, fill_byte, m->a_bytes, m->st));
    if (m->d_b && m->b_bytes) SM_HIP(hipMemsetAsync(m->d_b, fill_byte, m->b_bytes, m->st));
    SM_HIP(hipStreamSynchronize(m->st));
    return HVO_OK;
}

// ---------------------------------------------------------------- kernels ----------------------------------------------------------------

__global__ __launch_bounds__(SM_BLOCK) void k_sm_mark(int nt, int ns, const uint8_t *__restrict__ flags, int32_t *__restrict__ held, uint8_t *__restrict__ t_occ,
                                                        const int32_t *__restrict__ extra, int n_extra, uint8_t *__restrict__ seen, int foreign_observed)
{
    const int i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i < nt) {
        int h = held[i];
        if (h >= ns) h = -1;                                       // (refused on the host before the launch)
        if (h >= 0 && (flags[h] & SM_BAD)) h = -1;                 // Tracking.cc:3235-3238 (points), 3296-3299 (lines)
        held[i] = h;
        t_occ[i] = ((h >= 0 && (flags[h] & SM_OBS)) || (foreign_observed && h == HVO_HELD_FOREIGN_OBSERVED)) ? 1 : 0;    // ORBmatcher.cc:88-90
        if (h >= 0) seen[h] = 1;                                   // mnLastFrameSeen = mCurrentFrame.mnId (3242, 3304)
    } else if (i - nt < n_extra) {
        const int e = extra[i - nt];
        if (e >= 0 && e < ns) seen[e] = 1;
    }
}

__global__ __launch_bounds__(SM_BLOCK) void k_sm_fill(int n, int32_t *__restrict__ idx, int32_t *__restrict__ dist)
{
    const int i = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (i < n) { idx[i] = -1; dist[i] = 256; }
}

__global__ __launch_bounds__(SM_BLOCK) void k_sm_assign(int nq, int nt, const int32_t *__restrict__ match_idx, int *__restrict__ win)
{
    const int q = blockIdx.x * SM_BLOCK + threadIdx.x;
    if (q >= nq) return;
    const int j = match_idx[q];
    if (j >= 0 && j < nt) atomicMax(&win[j], q);
}

void sm_fill_enqueue(hipStream_t st, int n, int32_t *idx, int32_t *dist)
{
    hipLaunchKernelGGL(k_sm_fill, dim3((n + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, st, n, idx, dist);
}

void sm_assign_enqueue(hipStream_t st, int nq, int nt, const int32_t *match_idx, int *win)
{
    hipLaunchKernelGGL(k_sm_assign, dim3((nq + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, st, nq, nt, match_idx, win);
}

// ---------------------------------------------------------------- the call ----------------------------------------------------------------

int sm_check_seen(hvo_slot_map *m, const char *prefix, const char *held_text, int held_min, const SmFrame &f)
{
    const int ns = m->n_slots;
    for (int i = 0; i < f.nt; i++) if (f.held[i] >= ns || f.held[i] < held_min) { m->last_error = std::string(prefix) + ": " + held_text; return HVO_ERR_INVALID_ARG; }
    for (int i = 0; i < f.ne; i++) if (f.extra[i] < 0 || f.extra[i] >= ns) { m->last_error = std::string(prefix) + ": seen_extra names a slot beyond the map"; return HVO_ERR_INVALID_ARG; }
    return HVO_OK;
}

void sm_carve_frame(SmCarve &c, SmFrame &f)
{
    const size_t nt = (size_t)std::max(f.nt, 1);
    f.o_held = c.take(nt * 4); f.o_occ = c.take(nt); f.o_ex = c.take((size_t)std::max(f.ne, 1) * 4); f.o_win = c.take(nt * 4);
}

int sm_stage_in(hvo_slot_map *m, hipStream_t st, char *A, size_t o_pose, size_t o_seen, size_t o_cnt, const std::vector<SmFrame> &fr, const float *Tcw)
{
    const int ns = m->n_slots;
    const size_t F = fr.size(), NS = (size_t)std::max(ns, 1);
    std::vector<SmPose> &pose = m->pose;                           // the map's: the asynchronous copy below reads it after this function has returned
    pose.resize(F);
    for (size_t f = 0; f < F; f++) {
        SmPose &p = pose[f];
        pose_split(Tcw + 12 * f, p.R, p.t, p.Ow);                  // mOw = -Rcw^T tcw
        p.pad = 0.f;
    }
    SM_HIP(hipMemcpyAsync(A + o_pose, pose.data(), F * sizeof(SmPose), hipMemcpyHostToDevice, st));
    SM_HIP(hipMemsetAsync(A + o_seen, 0, F * NS, st));
    SM_HIP(hipMemsetAsync(A + o_cnt, 0, F * 8, st));
    for (const SmFrame &f : fr) {
        if (f.nt) SM_HIP(hipMemcpyAsync(A + f.o_held, f.held, (size_t)f.nt * 4, hipMemcpyHostToDevice, st));
        if (f.ne) SM_HIP(hipMemcpyAsync(A + f.o_ex, f.extra, (size_t)f.ne * 4, hipMemcpyHostToDevice, st));
        SM_HIP(hipMemsetAsync(A + f.o_win, 0xFF, (size_t)std::max(f.nt, 1) * 4, st));
    }
    return HVO_OK;
}

int sm_mark(hvo_slot_map *m, hipStream_t st, char *A, size_t o_seen, const std::vector<SmFrame> &fr, int foreign_observed)
{
    const int ns = m->n_slots;
    SM_HIP(hipEventRecord(m->ev[0], st));
    for (size_t k = 0; k < fr.size(); k++) {
        const SmFrame &f = fr[k];
        const int n = f.nt + f.ne;
        if (n > 0 && ns > 0)
            hipLaunchKernelGGL(k_sm_mark, dim3((n + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, st, f.nt, ns, m->d_flags(), (int32_t *)(A + f.o_held),
                               (uint8_t *)(A + f.o_occ), (const int32_t *)(A + f.o_ex), f.ne, (uint8_t *)(A + o_seen) + k * ns, foreign_observed);
        else if (f.nt > 0)
            SM_HIP(hipMemsetAsync(A + f.o_occ, 0, (size_t)f.nt, st));
    }
    return HVO_OK;
}

int sm_counts_down(hvo_slot_map *m, hipStream_t st, const char *launch_text, const char *d_cnt, int nframes, std::vector<int> &cnt)
{
    if (hipGetLastError() != hipSuccess) { m->last_error = launch_text; return HVO_ERR_HIP; }
    SM_HIP(hipEventRecord(m->ev[1], st));
    cnt.assign(2 * (size_t)nframes, 0);
    SM_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)nframes * 8, hipMemcpyDeviceToHost, st));
    SM_HIP(hipStreamSynchronize(st));
    return HVO_OK;
}

void sm_kernel_ms(hvo_slot_map *m, float ms[3])
{
    for (int k = 0; k < 3; k++) if (hipEventElapsedTime(&ms[k], m->ev[k], m->ev[k + 1]) != hipSuccess) ms[k] = 0.f;
}
