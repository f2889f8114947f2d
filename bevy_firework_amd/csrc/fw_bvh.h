// fw_bvh.h -- the bounding-volume hierarchy of a collider mesh (include/firework_hip.h: fw_mesh), built on the host.
// Plain C++ with no HIP include: the engine (fw_engine_mesh.cpp) uploads what it builds, and tests/test_bvh_cpu.py compiles
// the builder with g++.
//
// Layout (what fw_cast_ray in fw_collide.h walks): a BVH2 in PREORDER, two float4 per node
//   {lo.xyz, escape}  escape (uint32 bits): index of the first node after this node's subtree, always > the node's own index
//   {hi.xyz, leaf}    leaf (uint32 bits): first triangle << 4 | triangle count (1 .. FW_BVH_LEAF); 0 for an interior node
// An interior node's children are node i + 1 and the node at escape(i + 1).  A walk that goes to i + 1 on a box hit (or tests
// a leaf's triangles and goes to its escape) and to the escape on a miss visits each node at most once and ends after at most
// n_nodes steps, whatever the ray.  The triangles follow in leaf order, three float4 each: {v0.xyz, original index (uint32
// bits)}, {e1.xyz, 0}, {e2.xyz, 0}, with e1 = v1 - v0 and e2 = v2 - v0 in fp32.  Node boxes are padded (FwBvh::pad) so that the
// rounding of the slab test never culls a triangle the triangle test would hit.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#define FW_BVH_LEAF 4   // most triangles per leaf
#define FW_BVH_BINS 16  // SAH bins per axis

struct FwBvh {
    std::vector<float> nodes;  // 8 floats per node
    std::vector<float> tris;   // 12 floats per triangle, leaf order
    uint32_t n_nodes = 0, n_tris = 0;
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};  // the root's box (padded)
    float pad = 0.0f;                                                // what every box was grown by on each side
    // fw_bvh_build_deformable only -- what a refit (fw_refit.h) needs next to the two tables:
    std::vector<uint32_t> slots;      // per leaf-order triangle slot {vertex 0, 1, 2, original index}
    std::vector<int32_t> parent;      // per node (-1: the root)
    std::vector<uint32_t> order;      // every node, sorted by height (a leaf: 0; an interior node: 1 + its higher child)
    std::vector<uint32_t> level_off;  // order[level_off[h] .. level_off[h + 1]) are the nodes of height h; sizes never grow with h
};

// Validates the mesh (xyz[n_vertices][3], indices[n_triangles][3]), drops its zero-area triangles (fp32 c = cross(e1, e2) with
// dot(c, c) == 0 or not finite) and builds the hierarchy with binned SAH.  Returns 0, or -1 with *err set: no vertices, no
// triangles, more than 2^28 triangles, an index >= n_vertices, a non-finite vertex, no triangle of non-zero area.
int fw_bvh_build(const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, FwBvh *out,
                 std::string *err);

// The same hierarchy over ALL triangles, for a mesh whose vertices will move (fw_ctx_create_deformable_mesh): a zero-area
// triangle keeps its slot, its box still bounds its vertices, and its record is {v0, original index} {0} {0} -- e1 = e2 = 0 is
// what no ray hits (fw_cast_ray: det == 0), so the walk needs no test of its own.  The pad is 1e-4 x the largest |coordinate|
// of the vertices that triangles reference, dropped triangles included.  A mesh without zero-area triangles gets the tables
// of fw_bvh_build, bit for bit.  Errors as there (no triangle of non-zero area included: creation still rejects it).
int fw_bvh_build_deformable(const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles, FwBvh *out,
                            std::string *err);

// What the host recomputes from new vertices of a deformable mesh: the pad by the rule above and the root's padded box
// (referenced[v] != 0: some triangle uses vertex v).  Equal to FwBvh::pad / lo / hi of a deformable build over the same vertices.
void fw_bvh_bounds(const float *xyz, const uint8_t *referenced, uint32_t n_vertices, float lo[3], float hi[3], float *pad);
// The same in the ONE pass over the caller's array that fw_ctx_update_mesh_vertices makes: every vertex is checked (the index
// of the first non-finite one is returned, dst then holds nothing of use), copied to dst (the pinned staging; may be null) and,
// where referenced, taken into the bounds.  -1: all finite, lo / hi / pad are set.
int64_t fw_bvh_stage_vertices(const float *xyz, const uint8_t *referenced, uint32_t n_vertices, float *dst, float lo[3], float hi[3],
                              float *pad);
