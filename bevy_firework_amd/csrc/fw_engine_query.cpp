// fw_engine_query.cpp -- the queries into the context's collider world: the ray cast, fw_ctx_cast_rays / fw_ctx_cast_rays_device
// (include/firework_hip.h: fw_ray_hit has the semantics; fw_k_query.hip runs fw_collide.h's cast, the one the particles use), and
// the point projection, fw_ctx_project_points / fw_ctx_project_points_device (fw_point_projection; fw_project.h).
//
// The four entry points are two helpers, query_device and query_staged, told the record sizes, the launcher and the entry point's
// name.  Both enqueue on the context's MAIN stream, where collider sets, instance sets, refits and every launch that casts rays
// already travel: a query sees the world exactly as of its place among those calls, with no event and no wait of its own.
#include "fw_engine.h"

namespace {

using QueryLaunch = hipError_t (*)(hipStream_t, const FwGlobals &, const void *, uint64_t, void *);

fw_status launch_query(fw_ctx *ctx, QueryLaunch launch, const char *name, const void *d_in, uint64_t n, void *d_out) {
    const hipError_t e = launch(ctx->stream, ctx->g, d_in, n, d_out);
    return e == hipSuccess ? FW_OK : fail(ctx, FW_EHIP, std::string(name) + ": " + hipGetErrorString(e));
}

// the device form: records in device memory, enqueued and never waited for
fw_status query_device(fw_ctx *ctx, QueryLaunch launch, const char *name, const void *d_in, uint64_t n, void *d_out) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!d_in || !d_out) return fail(ctx, FW_EINVAL, std::string(name) + ": null pointer");
    hipSetDevice(ctx->device);
    return launch_query(ctx, launch, name, d_in, n, d_out);
}

// `b` holds at least n records of `quads` float4 each; a buffer that is replaced is not in use: the staged form waits for its own
// work before it returns
fw_status reserve_records(fw_ctx *ctx, HipBuf<float4> &b, uint64_t n, Mem kind, uint64_t quads) {
    if (quads * n <= b.cap()) return FW_OK;
    return alloc_buf(ctx, b, (size_t)std::max<uint64_t>(quads * n, 2 * 4096), kind);
}

// the host form: records of in_size / out_size bytes (whole float4s) in host memory, staged through the context's four query
// buffers; waits
fw_status query_staged(fw_ctx *ctx, QueryLaunch launch, const char *name, const void *in, size_t in_size, uint64_t n, void *out,
                       size_t out_size) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!in || !out) return fail(ctx, FW_EINVAL, std::string(name) + ": null pointer");
    hipSetDevice(ctx->device);
    const uint64_t in_quads = in_size / sizeof(float4), out_quads = out_size / sizeof(float4);
    fw_status st;
    if ((st = reserve_records(ctx, ctx->q_in_h, n, Mem::pinned, in_quads)) || (st = reserve_records(ctx, ctx->q_out_h, n, Mem::pinned, out_quads)) ||
        (st = reserve_records(ctx, ctx->q_in_d, n, Mem::device, in_quads)) || (st = reserve_records(ctx, ctx->q_out_d, n, Mem::device, out_quads)))
        return st;
    const size_t in_bytes = (size_t)n * in_size, out_bytes = (size_t)n * out_size;
    memcpy(ctx->q_in_h.get(), in, in_bytes);
    FW_HIP(ctx, hipMemcpyAsync(ctx->q_in_d, ctx->q_in_h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((st = launch_query(ctx, launch, name, ctx->q_in_d, n, ctx->q_out_d))) return st;
    FW_HIP(ctx, hipMemcpyAsync(ctx->q_out_h, ctx->q_out_d, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->q_out_h.get(), out_bytes);
    return FW_OK;
}

}  // namespace

extern "C" {

fw_status fw_ctx_cast_rays_device(fw_ctx *ctx, const void *d_rays, uint64_t n, void *d_hits) {
    return query_device(ctx, fw_launch_cast_rays, "fw_ctx_cast_rays_device", d_rays, n, d_hits);
}

fw_status fw_ctx_cast_rays(fw_ctx *ctx, const fw_ray *rays, uint64_t n, fw_ray_hit *hits) {
    static_assert(sizeof(fw_ray) == 32 && sizeof(fw_ray_hit) == 32, "fw_ray / fw_ray_hit are two float4 each");
    return query_staged(ctx, fw_launch_cast_rays, "fw_ctx_cast_rays", rays, sizeof(fw_ray), n, hits, sizeof(fw_ray_hit));
}

fw_status fw_ctx_project_points_device(fw_ctx *ctx, const void *d_points, uint64_t n, void *d_out) {
    return query_device(ctx, fw_launch_project_points, "fw_ctx_project_points_device", d_points, n, d_out);
}

fw_status fw_ctx_project_points(fw_ctx *ctx, const fw_point *points, uint64_t n, fw_point_projection *out) {
    static_assert(sizeof(fw_point) == 16 && sizeof(fw_point_projection) == 32, "fw_point is one float4, fw_point_projection two");
    return query_staged(ctx, fw_launch_project_points, "fw_ctx_project_points", points, sizeof(fw_point), n, out, sizeof(fw_point_projection));
}

}  // extern "C"
