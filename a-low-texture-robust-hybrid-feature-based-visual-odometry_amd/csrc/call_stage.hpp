// call_stage.hpp -- how an entry point lays out the block it stages through (the context's call arena).  Host-only C++ without HIP headers:
// tools/call_stage_host.cpp includes it from a plain g++ program (tests/test_call_stage.py).
//
// A StageCarver hands out pieces in the order they are asked for, each on a multiple of its alignment.  A StagePiece knows its byte offset,
// its element type and its shape (`rows` rows of `stride` elements); its views are the only casts a site needs: host(h, row) into the host
// block that goes up, dev(d, row) into the arena, down(b, row) into a downloaded copy of the arena's bytes from b.r0 on.  Row `row` starts
// row * stride elements in: candidate j's row is j; component c of candidate j of an array stored by component is row 3 j + c.  What a site
// uploads, clears and copies back are byte ranges between mark()s that it places itself (they may overlap).  Nothing here checks a bound at
// run time: tests/test_call_arena_gpu.py runs every site on a dirty arena.
#pragma once
#include <stddef.h>

static inline size_t stage_align(size_t v, size_t a = 256) { return (v + a - 1) & ~(a - 1); }

struct StageDown { const char *p; size_t r0; };                  // p[0] is the arena's byte r0

template <class T> struct StagePiece {
    size_t off = 0, rows = 0, stride = 1;
    size_t count() const { return rows * stride; }
    size_t bytes() const { return count() * sizeof(T); }
    T *host(char *h, size_t row = 0) const { return (T *)(h + off) + row * stride; }
    T *dev(char *d, size_t row = 0) const { return (T *)(d + off) + row * stride; }
    const T *down(const StageDown &b, size_t row = 0) const { return (const T *)(b.p + (off - b.r0)) + row * stride; }
};

struct StageCarver {
    size_t align, o = 0;
    explicit StageCarver(size_t align_) : align(align_) {}
    // no elements: no space, and the next piece starts here too
    template <class T> StagePiece<T> take(size_t rows, size_t stride = 1) { StagePiece<T> p; p.off = o; p.rows = rows; p.stride = stride; o += stage_align(p.bytes(), align); return p; }
    size_t mark() const { return o; }
};

// Tcw (3 x 4, row-major) -> Rcw, tcw and the camera centre Ow = -Rcw^T tcw: each sum in double from 0, left to right, times -1.0, rounded once
static inline void pose_split(const float Tcw[12], float R[9], float t[3], float Ow[3])
{
    for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) R[3 * r + q] = Tcw[4 * r + q]; t[r] = Tcw[4 * r + 3]; }
    for (int r = 0; r < 3; r++) {
        double s0 = 0;
        for (int q = 0; q < 3; q++) s0 += (double)R[3 * q + r] * (double)t[q];
        Ow[r] = (float)(s0 * -1.0);
    }
}
