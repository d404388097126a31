// arena.hip -- the two staging blocks of a context, both grow-only: the call arena (device) and the pinned host block.  Every host-array
// entry point stages through them instead of a hipMalloc / hipFree pair per argument: the staged calls through a StagedCall
// (staged_call.hpp), the Frame-tail calls and match.hip's older matchers (arena_begin) directly.  Calls on one context do not overlap and
// each ends in a synchronisation, so a block is free again when the next call asks for it.
#include "hvo_internal.hpp"

// device buffer of at least `bytes` that lives as long as the context
void *hvo_call_arena(hvo_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->call_arena_cap && ctx->call_arena) return ctx->call_arena;
    (void)hipStreamSynchronize(ctx->stream);                     // nothing enqueued may still use the old buffer
    if (ctx->call_arena) (void)hipFree(ctx->call_arena);
    ctx->call_arena = nullptr; ctx->call_arena_cap = 0;
    const size_t cap = hvo_arena_capacity(bytes);
    if (hipMalloc(&ctx->call_arena, cap) != hipSuccess) { ctx->last_error = "hipMalloc(call arena)"; ctx->call_arena = nullptr; return nullptr; }
    ctx->call_arena_cap = cap;
    return ctx->call_arena;
}

// pinned host block of exactly `bytes` when it has to grow (the batch downloads ask for what they need; a staged call rounds up itself)
void *hvo_stage_host(hvo_ctx *ctx, size_t bytes)
{
    if (ctx->h_stage_cap >= bytes) return ctx->h_stage;
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    ctx->h_stage = nullptr; ctx->h_stage_cap = 0;
    if (hipHostMalloc(&ctx->h_stage, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    ctx->h_stage_cap = bytes;
    return ctx->h_stage;
}

// Test doors (tests/test_call_arena_gpu.py), not product API and not in include/hvo.h.  hvo_debug_call_arena grows the arena to min_bytes the
// way a call would, sets its whole capacity to fill_byte when that is >= 0 (on the context's stream, drained before it returns) and reports
// the capacity; hvo_debug_call_arena_peek copies bytes of it back.
extern "C" int hvo_debug_call_arena(hvo_ctx *ctx, int fill_byte, size_t min_bytes, size_t *cap_out)
{
    if (!ctx || fill_byte > 255) return HVO_ERR_INVALID_ARG;
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    if (min_bytes && !hvo_call_arena(ctx, min_bytes)) return HVO_ERR_HIP;
    if (fill_byte >= 0 && ctx->call_arena_cap) {
        if (hipMemsetAsync(ctx->call_arena, fill_byte, ctx->call_arena_cap, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            ctx->last_error = "hvo_debug_call_arena: fill"; return HVO_ERR_HIP;
        }
    }
    if (cap_out) *cap_out = ctx->call_arena_cap;
    return HVO_OK;
}

extern "C" int hvo_debug_call_arena_peek(hvo_ctx *ctx, size_t offset, size_t n, uint8_t *out)
{
    if (!ctx || (n && !out) || offset > ctx->call_arena_cap || n > ctx->call_arena_cap - offset) return HVO_ERR_INVALID_ARG;
    if (n == 0) return HVO_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return HVO_ERR_NO_DEVICE;
    if (hipMemcpyAsync(out, (const char *)ctx->call_arena + offset, n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        ctx->last_error = "hvo_debug_call_arena_peek: copy"; return HVO_ERR_HIP;
    }
    return HVO_OK;
}
