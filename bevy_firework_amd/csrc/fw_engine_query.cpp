// fw_engine_query.cpp -- the queries into the context's collider world: the ray cast, fw_ctx_cast_rays / fw_ctx_cast_rays_device
// (include/firework_hip.h: fw_ray_hit has the semantics; fw_k_query.hip runs fw_collide.h's cast, the one the particles use), the
// point projection, fw_ctx_project_points / fw_ctx_project_points_device (fw_point_projection; fw_project.h), and the path query,
// fw_ctx_trace_paths / fw_ctx_trace_paths_device (fw_path_result; fw_trace.h).
//
// The six entry points are two helpers, query_device and query_staged, told the record sizes, the launcher and the entry point's
// name.  Both enqueue on the context's MAIN stream, where collider sets, instance sets, refits and every launch that casts rays
// already travel: a query sees the world exactly as of its place among those calls, with no event and no wait of its own.  A
// launcher is anything callable as (stream, globals, d_in, n, d_out, d_out2); d_out2 is the optional second output (the path query's
// samples), null for everybody else.
#include "fw_engine.h"
#include "fw_trace.h"

namespace {

template <class Launch>
fw_status launch_query(fw_ctx *ctx, const Launch &launch, const char *name, const void *d_in, uint64_t n, void *d_out, void *d_out2) {
    const hipError_t e = launch(ctx->stream, ctx->g, d_in, n, d_out, d_out2);
    return e == hipSuccess ? FW_OK : fail(ctx, FW_EHIP, std::string(name) + ": " + hipGetErrorString(e));
}

// the device form: records in device memory, enqueued and never waited for
template <class Launch>
fw_status query_device(fw_ctx *ctx, const Launch &launch, const char *name, const void *d_in, uint64_t n, void *d_out, void *d_out2 = nullptr) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!d_in || !d_out) return fail(ctx, FW_EINVAL, std::string(name) + ": null pointer");
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    return launch_query(ctx, launch, name, d_in, n, d_out, d_out2);
}

// `b` holds at least n records of `quads` float4 each; a buffer that is replaced is not in use: the staged form waits for its own
// work before it returns
fw_status reserve_records(fw_ctx *ctx, HipBuf<float4> &b, uint64_t n, Mem kind, uint64_t quads) {
    if (quads * n <= b.cap()) return FW_OK;
    return alloc_buf(ctx, b, (size_t)std::max<uint64_t>(quads * n, 2 * 4096), kind);
}

// the host form: records of in_size / out_size bytes (whole float4s) in host memory, staged through the context's query buffers;
// waits.  out2 (may be null): a second output of out2_size bytes per record, staged like the first through buffers of its own --
// nothing is reserved or copied for it when it is null
template <class Launch>
fw_status query_staged(fw_ctx *ctx, const Launch &launch, const char *name, const void *in, size_t in_size, uint64_t n, void *out, size_t out_size,
                       void *out2 = nullptr, size_t out2_size = 0) {
    if (!ctx) return FW_EINVAL;
    if (n == 0) return FW_OK;
    if (!in || !out) return fail(ctx, FW_EINVAL, std::string(name) + ": null pointer");
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    const uint64_t in_quads = in_size / sizeof(float4), out_quads = out_size / sizeof(float4), out2_quads = out2_size / sizeof(float4);
    if (out2_quads == 0) out2 = nullptr;
    fw_status st;
    if ((st = reserve_records(ctx, ctx->q_in_h, n, Mem::pinned, in_quads)) || (st = reserve_records(ctx, ctx->q_out_h, n, Mem::pinned, out_quads)) ||
        (st = reserve_records(ctx, ctx->q_in_d, n, Mem::device, in_quads)) || (st = reserve_records(ctx, ctx->q_out_d, n, Mem::device, out_quads)))
        return st;
    if (out2 && ((st = reserve_records(ctx, ctx->q_out2_h, n, Mem::pinned, out2_quads)) || (st = reserve_records(ctx, ctx->q_out2_d, n, Mem::device, out2_quads))))
        return st;
    const size_t in_bytes = (size_t)n * in_size, out_bytes = (size_t)n * out_size, out2_bytes = (size_t)n * out2_size;
    memcpy(ctx->q_in_h.get(), in, in_bytes);
    FW_HIP(ctx, hipMemcpyAsync(ctx->q_in_d, ctx->q_in_h, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((st = launch_query(ctx, launch, name, ctx->q_in_d, n, ctx->q_out_d, out2 ? ctx->q_out2_d.get() : nullptr))) return st;
    FW_HIP(ctx, hipMemcpyAsync(ctx->q_out_h, ctx->q_out_d, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out2) FW_HIP(ctx, hipMemcpyAsync(ctx->q_out2_h, ctx->q_out2_d, out2_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->q_out_h.get(), out_bytes);
    if (out2) memcpy(out2, ctx->q_out2_h.get(), out2_bytes);
    return FW_OK;
}

hipError_t cast_rays(hipStream_t s, const FwGlobals &g, const void *d_in, uint64_t n, void *d_out, void *) { return fw_launch_cast_rays(s, g, d_in, n, d_out); }
hipError_t project_points(hipStream_t s, const FwGlobals &g, const void *d_in, uint64_t n, void *d_out, void *) {
    return fw_launch_project_points(s, g, d_in, n, d_out);
}

// The path query's launcher: the caller's settings, validated HERE for both forms and carried by value -- they travel on as kernel
// arguments.  A null record, a non-finite dt, more than FW_PATH_MAX_STEPS steps: FW_EINVAL before anything else is looked at.
struct TracePaths {
    FwPathSettings s;
    hipError_t operator()(hipStream_t st, const FwGlobals &g, const void *d_in, uint64_t n, void *d_out, void *d_samples) const {
        return fw_launch_trace_paths(st, g, s, d_in, n, d_out, d_samples);
    }
};
fw_status path_settings(fw_ctx *ctx, const char *name, const fw_path_settings *in, TracePaths *out) {
    if (!ctx) return FW_EINVAL;
    if (!in) return fail(ctx, FW_EINVAL, std::string(name) + ": null settings");
    if (!std::isfinite(in->dt)) return fail(ctx, FW_EINVAL, std::string(name) + ": dt is not finite");
    if (in->n_steps > FW_PATH_MAX_STEPS) return fail(ctx, FW_EINVAL, std::string(name) + ": n_steps exceeds FW_PATH_MAX_STEPS");
    const fw_collision_settings &c = in->collision;
    out->s = FwPathSettings{in->dt, in->n_steps, {in->acceleration[0], in->acceleration[1], in->acceleration[2]}, in->linear_drag,
                            c.enabled ? 1u : 0u, c.destroy_on_collision ? 1u : 0u, c.filter_mask, c.restitution, c.friction};
    return FW_OK;
}

}  // namespace

extern "C" {

fw_status fw_ctx_cast_rays_device(fw_ctx *ctx, const void *d_rays, uint64_t n, void *d_hits) {
    return query_device(ctx, cast_rays, "fw_ctx_cast_rays_device", d_rays, n, d_hits);
}

fw_status fw_ctx_cast_rays(fw_ctx *ctx, const fw_ray *rays, uint64_t n, fw_ray_hit *hits) {
    static_assert(sizeof(fw_ray) == 32 && sizeof(fw_ray_hit) == 32, "fw_ray / fw_ray_hit are two float4 each");
    return query_staged(ctx, cast_rays, "fw_ctx_cast_rays", rays, sizeof(fw_ray), n, hits, sizeof(fw_ray_hit));
}

fw_status fw_ctx_project_points_device(fw_ctx *ctx, const void *d_points, uint64_t n, void *d_out) {
    return query_device(ctx, project_points, "fw_ctx_project_points_device", d_points, n, d_out);
}

fw_status fw_ctx_project_points(fw_ctx *ctx, const fw_point *points, uint64_t n, fw_point_projection *out) {
    static_assert(sizeof(fw_point) == 16 && sizeof(fw_point_projection) == 32, "fw_point is one float4, fw_point_projection two");
    return query_staged(ctx, project_points, "fw_ctx_project_points", points, sizeof(fw_point), n, out, sizeof(fw_point_projection));
}

fw_status fw_ctx_trace_paths_device(fw_ctx *ctx, const fw_path_settings *settings, const void *d_paths, uint64_t n, void *d_out, void *d_samples) {
    TracePaths launch;
    if (const fw_status st = path_settings(ctx, "fw_ctx_trace_paths_device", settings, &launch)) return st;
    return query_device(ctx, launch, "fw_ctx_trace_paths_device", d_paths, n, d_out, d_samples);
}

fw_status fw_ctx_trace_paths(fw_ctx *ctx, const fw_path_settings *settings, const fw_path *paths, uint64_t n, fw_path_result *out, float *samples) {
    static_assert(sizeof(fw_path) == 32 && sizeof(fw_path_result) == 80, "fw_path is two float4, fw_path_result five");
    TracePaths launch;
    if (const fw_status st = path_settings(ctx, "fw_ctx_trace_paths", settings, &launch)) return st;
    return query_staged(ctx, launch, "fw_ctx_trace_paths", paths, sizeof(fw_path), n, out, sizeof(fw_path_result), samples,
                        (size_t)launch.s.n_steps * sizeof(float4));
}

}  // extern "C"
