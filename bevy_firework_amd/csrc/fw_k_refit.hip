// fw_k_refit.hip -- the refit of a deformable collider mesh on the device (fw_ctx_update_mesh_vertices): new triangle records
// and boxes from new vertices, in place, over a hierarchy whose shape stays (fw_refit.h has the arithmetic, fw_bvh.h the
// schedule: the nodes sorted by height, leaves first).
//
// A node of height h reads boxes of lower heights only, so the hierarchy is redone level by level, lowest first:
//   * a level of many nodes is one launch of many workgroups; the next level is the next launch of the same stream.  What
//     another workgroup wrote -- on another XCD, whose L2 is not coherent with this one's for plain loads -- is read only
//     across a kernel boundary, which makes it visible; no flag, no counter, no fence.
//   * level sizes never grow with the height (every node of height h + 1 has a child of height h), so from the first level of
//     at most FW_REFIT_TAIL nodes on, ALL remaining levels are one launch of ONE workgroup that puts a __syncthreads() between
//     two levels.  The waves of a workgroup share their CU's vector L1 and the barrier orders their stores and loads at workgroup
//     scope: again nothing a workgroup-scope barrier does not cover.  A small mesh is this launch alone.
//     Two things this rests on: the default (non-tgsplit) mode, in which all waves of a workgroup run on ONE CU behind one
//     write-through L1 -- never build this unit with -mtgsplit; and node loads that stay VECTOR loads (the node index comes from
//     R.order[j], per lane): the scalar cache is not kept coherent with vector stores, so a node must never be read on the scalar path.
// No workgroup ever waits for another: nothing here spins, polls or looks back, so a refit cannot hang whatever else the
// device runs.  A hierarchy of one node (a root that is a leaf) is one level of one node.  A height field of 131 072
// triangles has four levels of more than FW_REFIT_TAIL nodes (35 844, 16 488, 8 912, 4 804): four wide launches and the tail.
//
// Vertices that are already in device memory (fw_ctx_update_mesh_vertices_device) put two launches in front and one behind:
//   fw_k_mesh_bounds       every vertex checked, the referenced ones reduced (fw_mesh_bounds.h): a grid-stride loop, a wave64
//                          butterfly, LDS across the waves of a workgroup, ONE partial per workgroup
//   fw_k_mesh_bounds_fold  one workgroup folds the partials and writes the mesh's record and the pinned report
//   fw_k_mesh_spheres      the bounding spheres of the instances that place the mesh, from the record's box
// under the same rule: partials, record and instance table cross workgroups at kernel boundaries only.
#include <hip/hip_runtime.h>

#include "fw_kernels.h"

#define FW_REFIT_BLOCK 256
#define FW_REFIT_TAIL_BLOCK 1024

// levels [first, first + n) of R.order; n > 1 only in a grid of one workgroup (fw_launch_mesh_refit).  R0.rec (vertices from
// device memory): the pad comes from the record, and a rejected update leaves the tables alone -- the record was written by an
// earlier launch of this stream, every lane reads the same word, so the exit is uniform and comes before any barrier.
__global__ __launch_bounds__(FW_REFIT_TAIL_BLOCK) void fw_k_mesh_refit(FwRefit R0, const uint32_t *level_off, uint32_t first, uint32_t n) {
    FwRefit R = R0;
    if (R0.rec) {
        if (R0.rec->rejected) return;
        R.pad = R0.rec->pad;
    }
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t l = first; l < first + n; l++) {
        const uint32_t end = level_off[l + 1];
        for (uint32_t j = level_off[l] + blockIdx.x * blockDim.x + threadIdx.x; j < end; j += stride) fw_refit_node(R, R.order[j]);
        if (n > 1u) __syncthreads();  // (uniform: n is a kernel argument)
    }
}

hipError_t fw_launch_mesh_refit(hipStream_t s, const FwRefit &R, const uint32_t *d_level_off, const uint32_t *h_level_off,
                                uint32_t n_levels) {
    uint32_t l = 0;
    for (; l < n_levels && h_level_off[l + 1] - h_level_off[l] > FW_REFIT_TAIL; l++) {
        const uint32_t cnt = h_level_off[l + 1] - h_level_off[l];
        hipLaunchKernelGGL(fw_k_mesh_refit, dim3((cnt + FW_REFIT_BLOCK - 1) / FW_REFIT_BLOCK), dim3(FW_REFIT_BLOCK), 0, s, R, d_level_off, l, 1u);
    }
    if (l < n_levels) hipLaunchKernelGGL(fw_k_mesh_refit, dim3(1), dim3(FW_REFIT_TAIL_BLOCK), 0, s, R, d_level_off, l, n_levels - l);
    return hipGetLastError();
}

// ---- vertices from device memory --------------------------------------------------------------------------------------------
// the reduction of fw_mesh_bounds.h across the 64 lanes of a wave: afterwards every lane holds the fold of all of them
__device__ __forceinline__ FwVtxAcc fw_bounds_wave(FwVtxAcc a) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        FwVtxAcc b;
#pragma unroll
        for (int k = 0; k < 3; k++) b.lo[k] = __shfl_xor(a.lo[k], m, 64), b.hi[k] = __shfl_xor(a.hi[k], m, 64);
        b.maxabs = __shfl_xor(a.maxabs, m, 64);
        b.bad = (uint32_t)__shfl_xor((int)a.bad, m, 64);
        a = fw_bounds_combine(a, b);
    }
    return a;
}

// ... and across the waves of a workgroup (blockDim.x a multiple of 64, at most FW_BOUNDS_BLOCK): thread 0 returns the fold
__device__ __forceinline__ FwVtxAcc fw_bounds_block(FwVtxAcc a) {
    __shared__ FwVtxAcc part[FW_BOUNDS_BLOCK / 64];
    a = fw_bounds_wave(a);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0u)
        for (uint32_t w = 1; w < blockDim.x >> 6; w++) a = fw_bounds_combine(a, part[w]);
    return a;
}

__global__ __launch_bounds__(FW_BOUNDS_BLOCK) void fw_k_mesh_bounds(const float *xyz, const uint8_t *referenced, uint32_t n_vertices,
                                                                    FwVtxAcc *partials) {
    FwVtxAcc a = fw_bounds_empty();
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_vertices; v += stride) {
        const float *p = xyz + 3 * (size_t)v;
        fw_bounds_vertex(a, v, p[0], p[1], p[2], referenced[v] != 0);
    }
    a = fw_bounds_block(a);
    if (threadIdx.x == 0u) partials[blockIdx.x] = a;
}

// ONE workgroup: the partials of the launch in front folded, the record and the report written.  Accepted: the record takes the
// new box and pad.  Rejected: counts and report only -- the box stays that of the last accepted shape, or becomes `seed` (the
// host's box, padded) when the mesh's bounds were the host's until this call (use_seed).
__global__ __launch_bounds__(FW_BOUNDS_BLOCK) void fw_k_mesh_bounds_fold(const FwVtxAcc *partials, uint32_t n_partials, FwMeshRecord *rec,
                                                                         FwMeshReport *report, FwMeshSeed seed, uint32_t use_seed) {
    FwVtxAcc a = fw_bounds_empty();
    for (uint32_t i = threadIdx.x; i < n_partials; i += blockDim.x) a = fw_bounds_combine(a, partials[i]);
    a = fw_bounds_block(a);
    if (threadIdx.x != 0u) return;
    const bool rejected = a.bad != FW_MESH_NO_BAD;
    unsigned long long n_applied = rec->n_applied, n_rejected = rec->n_rejected;
    long long first_bad = rec->first_bad;
    if (!rejected) {
        float lo[3], hi[3], pad;
        fw_bounds_finish(a, lo, hi, &pad);
        for (int k = 0; k < 3; k++) rec->lo[k] = lo[k], rec->hi[k] = hi[k];
        rec->pad = pad;
        n_applied++;
    } else {
        if (use_seed) {
            for (int k = 0; k < 3; k++) rec->lo[k] = seed.lo[k], rec->hi[k] = seed.hi[k];
            rec->pad = seed.pad;
        }
        n_rejected++, first_bad = (long long)a.bad;
    }
    rec->rejected = rejected ? 1u : 0u;
    rec->n_applied = n_applied, rec->n_rejected = n_rejected, rec->first_bad = first_bad;
    // the host's view: ordinary stores to pinned memory, like the live-count snapshots (first_bad before the count that
    // announces it; exact after a synchronisation either way)
    report->first_bad = first_bad;
    report->n_applied = n_applied, report->n_rejected = n_rejected;
}

// the spheres of the instances that place the mesh whose tables start at `nodes`, from the record's box.  after_update: the
// launch belongs to an update, which changed nothing when it was rejected.
__global__ __launch_bounds__(FW_REFIT_BLOCK) void fw_k_mesh_spheres(FwMeshInst *inst, uint32_t n_inst, const float4 *nodes,
                                                                    const FwMeshRecord *rec, uint32_t after_update) {
    if (after_update && rec->rejected) return;
    const float lo[3] = {rec->lo[0], rec->lo[1], rec->lo[2]}, hi[3] = {rec->hi[0], rec->hi[1], rec->hi[2]};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_inst; i += gridDim.x * blockDim.x) {
        if (inst[i].nodes != nodes) continue;
        float center[3], radius;
        fw_mesh_inst_sphere(lo, hi, inst[i].position, inst[i].rotation, center, &radius);
        inst[i].center[0] = center[0], inst[i].center[1] = center[1], inst[i].center[2] = center[2];
        inst[i].position[3] = radius;
    }
}

uint32_t fw_mesh_bounds_partials(uint32_t n_vertices) {
    const uint32_t g = (n_vertices + FW_BOUNDS_BLOCK - 1) / FW_BOUNDS_BLOCK;
    return g < 1u ? 1u : g > FW_BOUNDS_MAX_GRID ? FW_BOUNDS_MAX_GRID : g;
}

hipError_t fw_launch_mesh_bounds(hipStream_t s, const float *d_xyz, const uint8_t *d_referenced, uint32_t n_vertices, FwVtxAcc *d_partials,
                                 FwMeshRecord *d_rec, FwMeshReport *h_report, const FwMeshSeed *seed) {
    const uint32_t g = fw_mesh_bounds_partials(n_vertices);
    hipLaunchKernelGGL(fw_k_mesh_bounds, dim3(g), dim3(FW_BOUNDS_BLOCK), 0, s, d_xyz, d_referenced, n_vertices, d_partials);
    hipLaunchKernelGGL(fw_k_mesh_bounds_fold, dim3(1), dim3(FW_BOUNDS_BLOCK), 0, s, d_partials, g, d_rec, h_report, seed ? *seed : FwMeshSeed{},
                       seed ? 1u : 0u);
    return hipGetLastError();
}

hipError_t fw_launch_mesh_spheres(hipStream_t s, FwMeshInst *d_inst, uint32_t n_inst, const float4 *nodes, const FwMeshRecord *d_rec,
                                  bool after_update) {
    if (!n_inst) return hipSuccess;
    const uint32_t g = (n_inst + FW_REFIT_BLOCK - 1) / FW_REFIT_BLOCK;
    hipLaunchKernelGGL(fw_k_mesh_spheres, dim3(g < 64u ? g : 64u), dim3(FW_REFIT_BLOCK), 0, s, d_inst, n_inst, nodes, d_rec,
                       after_update ? 1u : 0u);
    return hipGetLastError();
}
