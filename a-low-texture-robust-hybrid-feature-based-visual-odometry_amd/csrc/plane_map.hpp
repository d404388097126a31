// plane_map.hpp -- the resident plane map as plane_assoc.hip (the slots, the pool, the match) and plane_update.hip (the device update of a
// slot's cloud) share it.  The layout of a slot's room is described at the head of plane_assoc.hip.
#pragma once
#include "hvo_internal.hpp"
#include <string>
#include <vector>

#define PA_MAXP 64                 // frame planes per frame = the tail's plane_clouds records
#define PA_CHUNK 1024              // points per wave of the distance pass: 4 dwordx4 per lane and coordinate
#define PA_DIST_WAVES 4

struct PaChunk { long long xoff; int cap, count, slot, pad; };   // xoff: pool index of the chunk's first x; count: points, a multiple of 4

struct PaSlot { size_t first = 0; int cap = 0, npts = 0; };

struct hvo_plane_map {
    int device = 0;
    hipStream_t st = nullptr;                                    // the map's own uploads
    int n_slots = 0, slot_cap = 0;
    std::vector<PaSlot> slot; std::vector<float> h_coef; std::vector<int32_t> h_bad;
    float *d_coef = nullptr; int32_t *d_bad = nullptr;           // slot_cap entries
    float *d_pool = nullptr; size_t pool_cap = 0, pool_used = 0; // floats
    float *h_stage = nullptr; size_t stage_cap = 0;              // pinned: one cloud transposed
    std::vector<PaChunk> chunks; bool chunks_dirty = true;
    PaChunk *d_chunks = nullptr; size_t chunk_cap = 0;
    char *d_scr = nullptr, *h_scr = nullptr; size_t scr_bytes = 0, hscr_bytes = 0;   // the matching calls' scratch, grow-only
    std::string last_error;
};

#define PM_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { m->last_error = std::string(#call) + ": " + hipGetErrorString(e_); return HVO_ERR_HIP; } } while (0)

// plane_assoc.hip: grow the slot table / the point pool (the pool's contents move by one device copy); both return after the copy
int pm_reserve_slots(hvo_plane_map *m, int want);
int pm_reserve_pool(hvo_plane_map *m, size_t want);
// plane_assoc.hip: the map's grow-only scratch (device d_scr, pinned h_scr) at dbytes / hbytes at least.  Growth doubles, so a map whose
// clouds grow frame by frame reallocates a logarithmic number of times; st is drained before a buffer that may be in use is freed.
int pm_scratch(hvo_plane_map *m, hipStream_t st, size_t dbytes, size_t hbytes);
