// staged_call.hpp -- the mechanics of one staged call, once: the context's call arena and pinned block, upload, clear, the timer, launch
// check, download, synchronisation.  HIP-side companion of call_stage.hpp (which stays host-only): the site keeps its StageCarver layout and
// its marks and says which byte ranges of it go up, are cleared and come down.
//
//   StagedCall sc(ctx, st, "fuse: ", err);
//   if ((rc = sc.begin(total, up_end, r1 - r0))) return rc;      fill sc.h[0, up_end), which is zeroed, through piece.host(sc.h, ..)
//   if ((rc = sc.up(0, up_end)) || (rc = sc.clear(z0, z1))) return rc;
//   sc.tick(); launch; sc.tick(); launch; sc.tick();              sc.ms[i] = device time between tick i and tick i + 1
//   StageDown b; if ((rc = sc.down(r0, r1, &b))) return rc;       read through piece.down(b, ..)
//
// A failing step writes `who` + "arena" / "upload" / "memset" / "launch" / the HIP error string to *err and returns HVO_ERR_HIP.  A failing
// event step costs the times only: ms stays 0, as for a call that launched nothing.  The block at h stays pinned between calls, so the
// copies are asynchronous both ways: nothing may touch h[a, b) between up(a, b) and down(), which is the first synchronisation.
#pragma once
#include "hvo_internal.hpp"
#include "call_stage.hpp"
#include <string.h>
#include <string>

// the context's four events around up to three kernel groups; read() after the stream has drained
struct CallTimer {
    hvo_ctx *ctx; hipStream_t st; int n = 0; bool ok = true;
    CallTimer(hvo_ctx *ctx_, hipStream_t st_) : ctx(ctx_), st(st_) {}
    void tick()
    {
        if (n >= 4) return;
        hipEvent_t &e = ctx->call_ev[n++];
        ok = ok && (e || hipEventCreate(&e) == hipSuccess) && hipEventRecord(e, st) == hipSuccess;
    }
    void read(float ms[3]) const
    {
        for (int i = 0; i < 3; i++) if (!ok || i + 1 >= n || hipEventElapsedTime(&ms[i], ctx->call_ev[i], ctx->call_ev[i + 1]) != hipSuccess) ms[i] = 0.f;
    }
};

struct StagedCall {                                              // one per *_run invocation, on the stack
    hvo_ctx *ctx; hipStream_t st; const char *who; std::string *err; CallTimer timer; size_t up_end = 0;
    char *d = nullptr, *h = nullptr; float ms[3] = { 0.f, 0.f, 0.f };
    StagedCall(hvo_ctx *ctx_, hipStream_t st_, const char *who_, std::string *err_) : ctx(ctx_), st(st_), who(who_), err(err_), timer(ctx_, st_) {}
    int fail(const char *what) { *err = std::string(who) + what; return HVO_ERR_HIP; }
    // d: dev_bytes of the arena; h: up_end bytes that go up, then down_bytes for what comes back (rounded up like the arena, so that a
    // slightly larger call does not pin a new block).  The upload's bytes are zeroed: the sites rely on zero padding.  zero = false is for
    // the two optimisers, which copy every piece whole and upload hundreds of megabytes for a batch of 8192 frames: only their alignment
    // holes carry stale host bytes to the device, where nothing reads them
    int begin(size_t dev_bytes, size_t up_end_, size_t down_bytes, bool zero = true)
    {
        up_end = up_end_;
        d = (char *)hvo_call_arena(ctx, dev_bytes);
        h = (char *)hvo_stage_host(ctx, hvo_arena_capacity(up_end + down_bytes));
        if (!d || !h) return fail("arena");
        if (zero) memset(h, 0, up_end);
        return HVO_OK;
    }
    int up(size_t a, size_t b) { return b > a && hipMemcpyAsync(d + a, h + a, b - a, hipMemcpyHostToDevice, st) != hipSuccess ? fail("upload") : HVO_OK; }
    int clear(size_t a, size_t b, int byte = 0) { return b > a && hipMemsetAsync(d + a, byte, b - a, st) != hipSuccess ? fail("memset") : HVO_OK; }
    void tick() { timer.tick(); }
    // the launch check, the arena's [r0, r1) to h + up_end, the synchronisation, the times
    int down(size_t r0, size_t r1, StageDown *b)
    {
        if (hipGetLastError() != hipSuccess) return fail("launch");
        if ((r1 > r0 && hipMemcpyAsync(h + up_end, d + r0, r1 - r0, hipMemcpyDeviceToHost, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
            return fail(hipGetErrorString(hipGetLastError()));
        timer.read(ms);
        *b = StageDown{ h + up_end, r0 };
        return HVO_OK;
    }
};
