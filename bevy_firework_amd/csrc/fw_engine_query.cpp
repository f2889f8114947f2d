// fw_engine_query.cpp -- the queries into the context's collider world: the ray cast, fw_ctx_cast_rays / fw_ctx_cast_rays_device
// (include/firework_hip.h: fw_ray_hit has the semantics; fw_k_query.hip runs fw_collide.h's cast, the one the particles use), and
// the point projection, fw_ctx_project_points / fw_ctx_project_points_device (fw_point_projection; fw_project.h).
//
// Both forms enqueue on the context's MAIN stream, where collider sets, instance sets, refits and every launch that casts rays
// already travel: a query sees the world exactly as of its place among those calls, with no event and no wait of its own.
#include "fw_engine.h"

namespace {

// `b` holds at least n records of `quads` float4 each (a ray, a hit, a projection: 2; a point: 1); a buffer that is replaced is not
// in use: the host forms wait for their own work before they return, so the two queries share the four buffers
fw_status reserve_records(fw_ctx *ctx, HipBuf<float4> &b, uint64_t n, Mem kind, uint64_t quads = 2) {
    if (quads * n <= b.cap()) return FW_OK;
    return alloc_buf(ctx, b, (size_t)std::max<uint64_t>(quads * n, 2 * 4096), kind);
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

fw_status fw_ctx_project_points_device(fw_ctx *ctx, const void *d_points, uint64_t n, void *d_out) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!d_points || !d_out) return fail(ctx, FW_EINVAL, "fw_ctx_project_points_device: null pointer");
    hipSetDevice(ctx->device);
    FW_HIP(ctx, fw_launch_project_points(ctx->stream, ctx->g, d_points, n, d_out));
    return FW_OK;
}

fw_status fw_ctx_project_points(fw_ctx *ctx, const fw_point *points, uint64_t n, fw_point_projection *out) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!points || !out) return fail(ctx, FW_EINVAL, "fw_ctx_project_points: null pointer");
    static_assert(sizeof(fw_point) == 16 && sizeof(fw_point_projection) == 32, "fw_point is one float4, fw_point_projection two");
    hipSetDevice(ctx->device);
    fw_status st;
    if ((st = reserve_records(ctx, ctx->h_rays, n, Mem::pinned, 1)) || (st = reserve_records(ctx, ctx->h_hits, n, Mem::pinned)) ||
        (st = reserve_records(ctx, ctx->d_rays, n, Mem::device, 1)) || (st = reserve_records(ctx, ctx->d_hits, n, Mem::device)))
        return st;
    const size_t in_bytes = (size_t)n * sizeof(fw_point), out_bytes = (size_t)n * sizeof(fw_point_projection);
    memcpy(ctx->h_rays.get(), points, in_bytes);
    FW_HIP(ctx, hipMemcpyAsync(ctx->d_rays, ctx->h_rays, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    FW_HIP(ctx, fw_launch_project_points(ctx->stream, ctx->g, ctx->d_rays, n, ctx->d_hits));
    FW_HIP(ctx, hipMemcpyAsync(ctx->h_hits, ctx->d_hits, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->h_hits.get(), out_bytes);
    return FW_OK;
}

}  // extern "C"
