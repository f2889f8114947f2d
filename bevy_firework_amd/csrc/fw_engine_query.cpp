// fw_engine_query.cpp -- the ray-cast query into the context's collider world: fw_ctx_cast_rays / fw_ctx_cast_rays_device
// (include/firework_hip.h: fw_ray_hit has the semantics; fw_k_query.hip runs fw_collide.h's cast, the one the particles use).
//
// Both forms enqueue on the context's MAIN stream, where collider sets, instance sets, refits and every launch that casts rays
// already travel: a query sees the world exactly as of its place among those calls, with no event and no wait of its own.
#include "fw_engine.h"

namespace {

// `b` holds at least n records of 32 bytes (two float4 each); a buffer that is replaced is not in use: the host form waits for
// its own work before it returns
fw_status reserve_records(fw_ctx *ctx, HipBuf<float4> &b, uint64_t n, Mem kind) {
    if (2 * n <= b.cap()) return FW_OK;
    return alloc_buf(ctx, b, (size_t)std::max<uint64_t>(2 * n, 2 * 4096), kind);
}

}  // namespace

extern "C" {

fw_status fw_ctx_cast_rays_device(fw_ctx *ctx, const void *d_rays, uint64_t n, void *d_hits) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!d_rays || !d_hits) return fail(ctx, FW_EINVAL, "fw_ctx_cast_rays_device: null pointer");
    hipSetDevice(ctx->device);
    FW_HIP(ctx, fw_launch_cast_rays(ctx->stream, ctx->g, d_rays, n, d_hits));
    return FW_OK;
}

fw_status fw_ctx_cast_rays(fw_ctx *ctx, const fw_ray *rays, uint64_t n, fw_ray_hit *hits) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!rays || !hits) return fail(ctx, FW_EINVAL, "fw_ctx_cast_rays: null pointer");
    static_assert(sizeof(fw_ray) == 32 && sizeof(fw_ray_hit) == 32, "fw_ray / fw_ray_hit are two float4 each");
    hipSetDevice(ctx->device);
    fw_status st;
    if ((st = reserve_records(ctx, ctx->h_rays, n, Mem::pinned)) || (st = reserve_records(ctx, ctx->h_hits, n, Mem::pinned)) ||
        (st = reserve_records(ctx, ctx->d_rays, n, Mem::device)) || (st = reserve_records(ctx, ctx->d_hits, n, Mem::device)))
        return st;
    const size_t bytes = (size_t)n * sizeof(fw_ray);
    memcpy(ctx->h_rays.get(), rays, bytes);
    FW_HIP(ctx, hipMemcpyAsync(ctx->d_rays, ctx->h_rays, bytes, hipMemcpyHostToDevice, ctx->stream));
    FW_HIP(ctx, fw_launch_cast_rays(ctx->stream, ctx->g, ctx->d_rays, n, ctx->d_hits));
    FW_HIP(ctx, hipMemcpyAsync(ctx->h_hits, ctx->d_hits, bytes, hipMemcpyDeviceToHost, ctx->stream));
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(hits, ctx->h_hits.get(), bytes);
    return FW_OK;
}

}  // extern "C"
