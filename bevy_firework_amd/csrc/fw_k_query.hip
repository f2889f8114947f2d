// fw_k_query.hip -- the public ray-cast query (fw_ctx_cast_rays / fw_ctx_cast_rays_device): a batch of rays in, nearest hits out,
// against the context's device-resident collider world.  One ray per lane, workgroups of FW_QUERY_BLOCK; a ray is two 16-byte
// loads (fw_ray), a hit two 16-byte stores (fw_ray_hit).
//
// The cast is fw_cast_ray of fw_collide.h itself -- the function the update kernels call -- instantiated with the identity
// policy FwHitId, so distance and normal are what a particle gets for the same ray and kind / index / triangle follow the
// cast's own tie rule (the policy is told when the best hit changes, and only then).
//
// What differs from the particle kernels: the filter mask is per LANE.  fw_cast_ray tests `layers & mask` in front of the wave
// skip's __ballot, so here that branch diverges; the ballot then counts the lanes that passed it and no others -- __ballot
// reports active lanes only -- which is exactly "no ray that takes part can reach this collider".  Lanes past n leave before the
// first load: they are inactive for the whole cast, so they load nothing, store nothing and keep no collider alive for the rest
// of their wave.  Nothing here waits for another workgroup and there is no barrier, so the early exit is safe.
//
// The point query (fw_ctx_project_points / fw_ctx_project_points_device) has the same shape: one point per lane, a point one 16-byte
// load (fw_point), a projection two 16-byte stores (fw_point_projection), the arithmetic fw_project_point of fw_project.h and none
// here; its wave skips count active lanes in the same way.
//
// The path query (fw_ctx_trace_paths / fw_ctx_trace_paths_device) has the same shape again: one path per lane, a path two 16-byte loads
// (fw_path), a result five 16-byte stores (fw_path_result), the arithmetic fw_trace_path of fw_trace.h -- fw_particle_collision told to
// report its hits -- and none here.  What it has that its neighbours do not: its lanes END AT DIFFERENT STEPS.  The rule: a lane whose
// path has ended takes no further part in any cast.  fw_trace_path keeps every step of a path inside `if (still running)`, so such a
// lane is inactive -- not merely ignored -- while the others cast, and the wave skips' __ballot counts the paths still running and no
// others: an expired path keeps no collider alive for the rest of its wave.  The filter mask is the call's, uniform here.  Samples go
// to [step][path], one store per lane and step from inside that loop, behind the block the ended lanes sit out: a wave writes 1 KiB
// contiguously per step, and a lane that has ended goes on storing its final values (without samples it leaves the loop).
#include <hip/hip_runtime.h>

#include "fw_kernels.h"
#include "fw_project.h"
#include "fw_trace.h"

#define FW_QUERY_BLOCK 256
#define FW_QUERY_MAX_LAUNCH (1ull << 30)  // rays per launch: lane indices and the grid stay well inside 32 bits

template <bool MESH>
__global__ __launch_bounds__(FW_QUERY_BLOCK) void fw_k_cast_rays(const FwCollider *colliders, uint32_t n_colliders, const FwMeshInst *meshes,
                                                                 uint32_t n_mesh, const float4 *rays, uint32_t n, float4 *hits) {
    const uint32_t i = blockIdx.x * FW_QUERY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];  // {origin, max_distance}, {dir, filter_mask}
    FwRayHit h;
    FwHitId id;
    fw_cast_ray(colliders, n_colliders, MESH ? meshes : nullptr, MESH ? n_mesh : 0u, __builtin_bit_cast(uint32_t, b.w), fw_v3{a.x, a.y, a.z},
                fw_v3{b.x, b.y, b.z}, a.w, &h, id);
    // (a miss: the cast never touched its best slot or the policy -- distance 0, normal 0, kind FW_HIT_NONE, index = triangle = ~0)
    hits[2 * (size_t)i] = float4{h.distance, h.normal.x, h.normal.y, h.normal.z};
    hits[2 * (size_t)i + 1] = float4{__builtin_bit_cast(float, id.kind), __builtin_bit_cast(float, id.index), __builtin_bit_cast(float, id.tri),
                                     __builtin_bit_cast(float, 0u)};
}

template <bool MESH>
__global__ __launch_bounds__(FW_QUERY_BLOCK) void fw_k_project_points(const FwCollider *colliders, uint32_t n_colliders, const FwMeshInst *meshes,
                                                                      uint32_t n_mesh, const float4 *points, uint32_t n, float4 *out) {
    const uint32_t i = blockIdx.x * FW_QUERY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 a = points[i];  // {position, filter_mask}
    FwProjection p;
    FwHitId id;
    fw_project_point(colliders, n_colliders, MESH ? meshes : nullptr, MESH ? n_mesh : 0u, __builtin_bit_cast(uint32_t, a.w), fw_v3{a.x, a.y, a.z}, &p, id);
    // (nobody answered: the projection left its result and the policy as they start -- point 0, distance 0, FW_HIT_NONE, index = triangle = ~0)
    out[2 * (size_t)i] = float4{p.point.x, p.point.y, p.point.z, p.distance};
    out[2 * (size_t)i + 1] = float4{__builtin_bit_cast(float, id.kind), __builtin_bit_cast(float, id.index), __builtin_bit_cast(float, id.tri),
                                    __builtin_bit_cast(float, p.is_inside)};
}

// where the samples of a launch go: path i of the launch, step k -> at[k * stride + i] (at == null: no samples)
struct FwSampleOut {
    float4 *at;
    uint64_t stride;
};
struct FwStoreSamples {
    bool on;
    float4 *at;  // the lane's own column
    uint64_t stride;
    __device__ __forceinline__ void operator()(uint32_t k, fw_v3 pos, float age) const {
        if (on) at[k * stride] = float4{pos.x, pos.y, pos.z, age};
    }
};

template <bool MESH>
__global__ __launch_bounds__(FW_QUERY_BLOCK) void fw_k_trace_paths(const FwCollider *colliders, uint32_t n_colliders, const FwMeshInst *meshes,
                                                                   uint32_t n_mesh, const float4 *paths, uint32_t n, float4 *out, FwPathSettings s,
                                                                   FwSampleOut smp) {
    const uint32_t i = blockIdx.x * FW_QUERY_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 a = paths[2 * (size_t)i], b = paths[2 * (size_t)i + 1];  // {position, age}, {velocity, lifetime}
    FwPathContacts c;
    const FwStoreSamples store{smp.at != nullptr, smp.at + i, smp.stride};
    const FwPathEnd e = fw_trace_path(colliders, n_colliders, MESH ? meshes : nullptr, MESH ? n_mesh : 0u, s, fw_v3{a.x, a.y, a.z}, fw_v3{b.x, b.y, b.z},
                                      a.w, b.w, c, store);
    // (no contact: the observer is as it started -- point 0, normal 0, FW_HIT_NONE, index = triangle = contact_step = ~0)
    float4 *r = out + 5 * (size_t)i;
    r[0] = float4{e.pos.x, e.pos.y, e.pos.z, e.age};
    r[1] = float4{e.vel.x, e.vel.y, e.vel.z, __builtin_bit_cast(float, e.steps)};
    r[2] = float4{c.point.x, c.point.y, c.point.z, __builtin_bit_cast(float, c.step)};
    r[3] = float4{c.normal.x, c.normal.y, c.normal.z, __builtin_bit_cast(float, e.status)};
    r[4] = float4{__builtin_bit_cast(float, c.who.kind), __builtin_bit_cast(float, c.who.index), __builtin_bit_cast(float, c.who.tri),
                  __builtin_bit_cast(float, c.n)};
}

// what a kernel takes behind its records is the same for every launch of a call -- except where it says otherwise
template <typename T>
static T fw_for_launch(T v, uint64_t) {
    return v;
}
static FwSampleOut fw_for_launch(FwSampleOut v, uint64_t first) {
    if (v.at) v.at += first;
    return v;
}

// The host half of the queries: launches of at most FW_QUERY_MAX_LAUNCH records, each the form without the mesh loop when the world
// holds no instances (as the update kernels pick theirs).  in_quads / out_quads: float4 per input / output record; tail: what the
// kernel takes behind them.
template <typename K, typename... Tail>
static hipError_t fw_launch_query(hipStream_t s, const FwGlobals &g, K with_mesh, K without_mesh, const void *d_in, uint32_t in_quads, uint64_t n,
                                  void *d_out, uint32_t out_quads, Tail... tail) {
    const K kernel = g.n_mesh_inst != 0u ? with_mesh : without_mesh;
    for (uint64_t first = 0; first < n; first += FW_QUERY_MAX_LAUNCH) {
        const uint32_t cnt = (uint32_t)(n - first < FW_QUERY_MAX_LAUNCH ? n - first : FW_QUERY_MAX_LAUNCH);
        const float4 *in = static_cast<const float4 *>(d_in) + in_quads * first;
        float4 *out = static_cast<float4 *>(d_out) + out_quads * first;
        const dim3 grid((cnt + FW_QUERY_BLOCK - 1) / FW_QUERY_BLOCK), block(FW_QUERY_BLOCK);
        hipLaunchKernelGGL(kernel, grid, block, 0, s, g.colliders, g.n_colliders, g.mesh_inst, g.n_mesh_inst, in, cnt, out, fw_for_launch(tail, first)...);
    }
    return hipGetLastError();
}

hipError_t fw_launch_cast_rays(hipStream_t s, const FwGlobals &g, const void *d_rays, uint64_t n, void *d_hits) {
    return fw_launch_query(s, g, fw_k_cast_rays<true>, fw_k_cast_rays<false>, d_rays, 2, n, d_hits, 2);
}

hipError_t fw_launch_project_points(hipStream_t s, const FwGlobals &g, const void *d_points, uint64_t n, void *d_out) {
    return fw_launch_query(s, g, fw_k_project_points<true>, fw_k_project_points<false>, d_points, 1, n, d_out, 2);
}

hipError_t fw_launch_trace_paths(hipStream_t s, const FwGlobals &g, const FwPathSettings &settings, const void *d_paths, uint64_t n, void *d_out,
                                 void *d_samples) {
    return fw_launch_query(s, g, fw_k_trace_paths<true>, fw_k_trace_paths<false>, d_paths, 2, n, d_out, 5, settings,
                           FwSampleOut{static_cast<float4 *>(d_samples), n});
}
