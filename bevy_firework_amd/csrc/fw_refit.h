// fw_refit.h -- the refit of a deformable collider mesh (include/firework_hip.h: fw_ctx_update_mesh_vertices): from new vertex
// positions, the triangle records and the boxes of a hierarchy whose SHAPE stays what fw_bvh_build_deformable made it.  The
// arithmetic is the builder's (fw_bvh.cpp), operation for operation, fp32, built with -ffp-contract=off like everything else, so
// a refit with the creation vertices reproduces the creation tables bit for bit.  Plain C++ behind FW_HD: the kernel
// (fw_k_refit.hip) and a CPU test (tests/test_bvh_refit_cpu.py, g++) run the same function per node.
#pragma once
#include <math.h>
#include <stdint.h>
#ifndef FW_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FW_HD __host__ __device__ __forceinline__
#else
#define FW_HD inline
#endif
#endif

struct alignas(16) FwR4 {  // one float4 of the node / triangle tables (fw_bvh.h)
    float x, y, z, w;
};
struct alignas(16) FwSlotIdx {  // per leaf-order triangle slot: its three vertices and its original index
    uint32_t v[3], orig;
};

// one mesh's tables: device pointers in the kernel, host arrays in the CPU test
struct FwRefit {
    FwR4 *nodes;             // 2 per node, preorder; the words escape / leaf are kept, the boxes rewritten
    FwR4 *tris;              // 3 per slot, rewritten
    const FwSlotIdx *slots;  // per slot
    const float *xyz;        // the new vertices, 3 floats each
    const uint32_t *order;   // every node, by height: the leaves first, every interior node behind both its children (FwBvh::order)
    float pad;               // what every leaf box is grown by: the builder's rule over the new vertices (fw_bvh_bounds)
    // vertices from device memory (fw_mesh_bounds.h): the launch takes the pad from this record of the device instead, and does
    // nothing when the record says the update was rejected.  Null: `pad` above holds (the host form, the CPU test)
    const struct FwMeshRecord *rec;
};

// std::min / std::max as the builder calls them
FW_HD float fw_refit_min(float a, float b) { return b < a ? b : a; }
FW_HD float fw_refit_max(float a, float b) { return a < b ? b : a; }
FW_HD uint32_t fw_refit_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// Node i from the new vertices (a leaf: its triangle records too) or from its two children, which must be done: callers go
// through FwRefit::order level by level.  An interior box is the min / max of its children's PADDED boxes; x -> x - pad is
// monotonic in fp32, so that equals the builder's (min over the subtree's vertices) - pad.
FW_HD void fw_refit_node(const FwRefit &R, uint32_t i) {
    const FwR4 n0 = R.nodes[2 * (size_t)i], n1 = R.nodes[2 * (size_t)i + 1];
    const uint32_t leaf = fw_refit_bits(n1.w);
    float lx, ly, lz, hx, hy, hz;
    if (leaf) {
        lx = ly = lz = INFINITY, hx = hy = hz = -INFINITY;
        const uint32_t first = leaf >> 4, last = first + (leaf & 15u);
        for (uint32_t k = first; k < last; k++) {
            const FwSlotIdx s = R.slots[k];
            const float *a = R.xyz + 3 * (size_t)s.v[0], *b = R.xyz + 3 * (size_t)s.v[1], *c = R.xyz + 3 * (size_t)s.v[2];
            const float ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
            const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
            // cross(e1, e2) in fw_cross's operation order; zero area (or an overflow): the record keeps e1 = e2 = 0, which takes
            // fw_cast_ray's `det == 0` arm for every ray -- never hit, never chosen for a normal
            const float nx = e1y * e2z - e2y * e1z, ny = e1z * e2x - e2z * e1x, nz = e1x * e2y - e2x * e1y;
            const float cc = (nx * nx + ny * ny) + nz * nz;
            const bool live = cc > 0.0f && cc < INFINITY;
            R.tris[3 * (size_t)k] = FwR4{ax, ay, az, __builtin_bit_cast(float, s.orig)};
            R.tris[3 * (size_t)k + 1] = live ? FwR4{e1x, e1y, e1z, 0.0f} : FwR4{0.0f, 0.0f, 0.0f, 0.0f};
            R.tris[3 * (size_t)k + 2] = live ? FwR4{e2x, e2y, e2z, 0.0f} : FwR4{0.0f, 0.0f, 0.0f, 0.0f};
            lx = fw_refit_min(lx, fw_refit_min(ax, fw_refit_min(bx, cx))), hx = fw_refit_max(hx, fw_refit_max(ax, fw_refit_max(bx, cx)));
            ly = fw_refit_min(ly, fw_refit_min(ay, fw_refit_min(by, cy))), hy = fw_refit_max(hy, fw_refit_max(ay, fw_refit_max(by, cy)));
            lz = fw_refit_min(lz, fw_refit_min(az, fw_refit_min(bz, cz))), hz = fw_refit_max(hz, fw_refit_max(az, fw_refit_max(bz, cz)));
        }
        lx = lx - R.pad, ly = ly - R.pad, lz = lz - R.pad, hx = hx + R.pad, hy = hy + R.pad, hz = hz + R.pad;
    } else {
        // the children: node i + 1 and the node at its escape
        const uint32_t c0 = i + 1u, c1 = fw_refit_bits(R.nodes[2 * (size_t)c0].w);
        const FwR4 a0 = R.nodes[2 * (size_t)c0], a1 = R.nodes[2 * (size_t)c0 + 1];
        const FwR4 b0 = R.nodes[2 * (size_t)c1], b1 = R.nodes[2 * (size_t)c1 + 1];
        lx = fw_refit_min(a0.x, b0.x), ly = fw_refit_min(a0.y, b0.y), lz = fw_refit_min(a0.z, b0.z);
        hx = fw_refit_max(a1.x, b1.x), hy = fw_refit_max(a1.y, b1.y), hz = fw_refit_max(a1.z, b1.z);
    }
    R.nodes[2 * (size_t)i] = FwR4{lx, ly, lz, n0.w};
    R.nodes[2 * (size_t)i + 1] = FwR4{hx, hy, hz, n1.w};
}
