// fw_mesh_bounds.h -- what fw_ctx_update_mesh_vertices_device needs to know about new vertices that only the device can see
// (include/firework_hip.h: DEFORMABLE MESHES): is every vertex finite, and over the vertices that triangles reference the
// lo / hi / maxabs that give the pad and the root's padded box -- fw_bvh_stage_vertices' pass (fw_bvh.cpp), as a reduction.
// min, max and fabs round nothing, so every partition and order of the vertices folds to the same VALUES; the one thing an
// order can change is the sign of a zero (min(+0, -0) keeps its first operand), and the results are lo - pad, hi + pad and
// 1e-4f * maxabs with pad >= 1e-30f > 0, which take both zeros to the same bits.  Plain C++ behind FW_HD: the kernels
// (fw_k_refit.hip) and a CPU test (tests/test_mesh_bounds_cpu.py, g++) run the same functions.
#pragma once
#include "fw_refit.h"

#define FW_MESH_NO_BAD 0xFFFFFFFFu  // FwVtxAcc::bad: every vertex so far is finite (a vertex index is < 2^32 - 1)

// the state of the reduction: of some subset of the vertices
struct FwVtxAcc {
    float lo[3], hi[3];  // over the referenced vertices of the subset (+inf / -inf: none yet)
    float maxabs;        // largest |coordinate| of them
    uint32_t bad;        // lowest index of a non-finite vertex of the subset, referenced or not
};

// The device's record of a deformable mesh whose vertices come from device memory (allocated by the mesh's first
// fw_ctx_update_mesh_vertices_device).  Written by the one workgroup of fw_k_mesh_bounds_fold; read by the launches behind it.
// lo / hi / pad are those of the LAST ACCEPTED shape: a rejected update leaves them alone.
struct alignas(16) FwMeshRecord {
    float lo[4], hi[4];  // the root's padded box ([3] unused)
    float pad;           // what every box is grown by (fw_bvh.h)
    uint32_t rejected;   // the latest device-form update held a non-finite vertex: its refit and sphere launches do nothing
    uint32_t pad_[2];
    unsigned long long n_applied, n_rejected;  // device-form updates so far
    long long first_bad;                       // lowest non-finite vertex index of the latest rejected one (-1: none yet)
};

// the pinned words fw_ctx_mesh_update_status reads: a copy of the record's counts, stored by the fold launch
struct FwMeshReport {
    unsigned long long n_applied, n_rejected;
    long long first_bad;
};

FW_HD FwVtxAcc fw_bounds_empty() {
    return FwVtxAcc{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0.0f, FW_MESH_NO_BAD};
}

// std::isfinite without <cmath>: exponent bits not all ones
FW_HD bool fw_bounds_finite(float x) { return (fw_refit_bits(x) & 0x7F800000u) != 0x7F800000u; }

// vertex v = (x, y, z) joins the subset.  A non-finite vertex is noted and kept out of the bounds (the update is rejected as
// a whole either way).
FW_HD void fw_bounds_vertex(FwVtxAcc &a, uint32_t v, float x, float y, float z, bool referenced) {
    if (!fw_bounds_finite(x) || !fw_bounds_finite(y) || !fw_bounds_finite(z)) {
        a.bad = v < a.bad ? v : a.bad;
        return;
    }
    if (!referenced) return;
    a.lo[0] = fw_refit_min(a.lo[0], x), a.lo[1] = fw_refit_min(a.lo[1], y), a.lo[2] = fw_refit_min(a.lo[2], z);
    a.hi[0] = fw_refit_max(a.hi[0], x), a.hi[1] = fw_refit_max(a.hi[1], y), a.hi[2] = fw_refit_max(a.hi[2], z);
    a.maxabs = fw_refit_max(a.maxabs, fw_refit_max(fabsf(x), fw_refit_max(fabsf(y), fabsf(z))));
}

// the union of two disjoint subsets
FW_HD FwVtxAcc fw_bounds_combine(const FwVtxAcc &a, const FwVtxAcc &b) {
    FwVtxAcc r;
    for (int k = 0; k < 3; k++) r.lo[k] = fw_refit_min(a.lo[k], b.lo[k]), r.hi[k] = fw_refit_max(a.hi[k], b.hi[k]);
    r.maxabs = fw_refit_max(a.maxabs, b.maxabs);
    r.bad = b.bad < a.bad ? b.bad : a.bad;
    return r;
}

// all vertices folded and none bad: the pad and the root's padded box, as fw_bvh_stage_vertices ends
FW_HD void fw_bounds_finish(const FwVtxAcc &a, float lo[3], float hi[3], float *pad) {
    *pad = fw_refit_max(1e-4f * a.maxabs, 1e-30f);
    for (int k = 0; k < 3; k++) lo[k] = a.lo[k] - *pad, hi[k] = a.hi[k] + *pad;
}

// The sphere of one placed instance (FwMeshInst::center / position[3]: the wave skip of fw_cast_ray) from the root's padded
// box in the mesh's frame and the instance's position / rotation: the arithmetic and the margins of the host's
// bounding_sphere + stage_instances (fw_engine_mesh.cpp), in double.  A degenerate rotation or a non-finite result: radius
// INFINITY around the position -- never skipped.
FW_HD void fw_mesh_inst_sphere(const float lo[3], const float hi[3], const float position[3], const float rotation[4], float center[3],
                               float *radius) {
    double lc[3], r2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const float c = (float)(((double)lo[k] + hi[k]) * 0.5);
        const double h0 = (double)hi[k] - c, h1 = (double)c - lo[k], h = h0 < h1 ? h1 : h0;
        lc[k] = c, r2 += h * h;
    }
    const float mesh_radius = (float)(sqrt(r2) * 1.0001);
    // fw_quat_mul_vec3 in double: v * (w^2 - b.b) + b * (2 v.b) + (b x v) * (2 w)
    const double bx = rotation[0], by = rotation[1], bz = rotation[2], w = rotation[3];
    const double s = bx * bx + by * by + bz * bz + w * w;
    const double k0 = w * w - (bx * bx + by * by + bz * bz), k1 = 2.0 * (lc[0] * bx + lc[1] * by + lc[2] * bz), k2 = 2.0 * w;
    const double cx = by * lc[2] - lc[1] * bz, cy = bz * lc[0] - lc[2] * bx, cz = bx * lc[1] - lc[0] * by;
    const double rc[3] = {lc[0] * k0 + bx * k1 + cx * k2, lc[1] * k0 + by * k1 + cy * k2, lc[2] * k0 + bz * k1 + cz * k2};
    double big = 0.0;
    for (int k = 0; k < 3; k++) {
        const double off = rc[k] / (s * s), m = fabs((double)position[k]) + fabs(off);
        center[k] = (float)(position[k] + off);
        big = big < m ? m : big;
    }
    *radius = (float)(mesh_radius / s * 1.001 + 1e-5 * big);
    if (!(s > 0.0) || !fw_bounds_finite(*radius) || !fw_bounds_finite(center[0] + center[1] + center[2])) {
        *radius = INFINITY;
        center[0] = position[0], center[1] = position[1], center[2] = position[2];
    }
}
