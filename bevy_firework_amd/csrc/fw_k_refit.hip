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
#include <hip/hip_runtime.h>

#include "fw_kernels.h"

#define FW_REFIT_BLOCK 256
#define FW_REFIT_TAIL_BLOCK 1024

// levels [first, first + n) of R.order; n > 1 only in a grid of one workgroup (fw_launch_mesh_refit)
__global__ __launch_bounds__(FW_REFIT_TAIL_BLOCK) void fw_k_mesh_refit(FwRefit R, const uint32_t *level_off, uint32_t first, uint32_t n) {
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
