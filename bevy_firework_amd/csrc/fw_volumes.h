// fw_volumes.h -- volume queries (round 29; include/firework_hip.h: VOLUME QUERIES): whether a point lies inside one analytic collider
// record used as a VOLUME.  The six expressions are those fw_project_collider (fw_project.h) returns true by -- through this function -- and fw_ray_collider
// (fw_collide.h) tests for its distance-0 case, operation by operation, fp32, built with -ffp-contract=off like everything else: the
// same operands in the same order, therefore the same bits.  Plain C++ behind FW_HD: the kernel (fw_k_aux.hip: fw_k_volumes) and a host
// test (tests/test_volume_query_cpu.py) compile the same lines.
//
// fw_project_collider (fw_project.h) calls it for its inside answer: ONE definition.  What that function goes on to compute for a point
// outside -- the frame vector o, xz, rr -- it states again from the same operands, and the compiler folds the two statements into one
// evaluation (fw_k_query's resource lines: profiles/r29/volume_resources.txt).
#pragma once
#include "fw_collide.h"

// volumes per tile of fw_k_volumes: lane v mod 64 of the wave keeps the count of volume v
#define FW_VOLUME_TILE 64u
// the most answers (n_places * n_volumes) of one call: each is a one-wave workgroup of fw_k_volumes_fold, a grid whose lanes a uint32 counts
// (include/firework_hip.h states it for the callers; the kernel units do not include that header)
#ifndef FW_VOLUME_MAX_ANSWERS
#define FW_VOLUME_MAX_ANSWERS 0x3FFFFFFull
#endif

// true when x lies inside or on the solid.  Every comparison is false for a NaN operand: a NaN position is inside nothing, and NaN or
// negative extents give whatever the operations give.  `layers` and `bound` are not read.
FW_HD bool fw_collider_contains(const FwCollider &c, fw_v3 x) {
    const fw_v3 cpos{c.position[0], c.position[1], c.position[2]};
    if (c.kind == 0) {  // PLANE: the half-space n.(x - p) <= 0
        const fw_v3 n{c.normal[0], c.normal[1], c.normal[2]};
        return fw_dot3(n, fw_sub3(cpos, x)) > 0.0f;
    }
    if (c.kind == 1) {  // SPHERE
        const fw_v3 v = fw_sub3(x, cpos);
        const float vv = fw_dot3(v, v);
        return vv - c.radius * c.radius <= 0.0f;
    }
    const fw_q4 r{c.rotation[0], c.rotation[1], c.rotation[2], c.rotation[3]};
    const bool aligned = r.x == 0.0f && r.y == 0.0f && r.z == 0.0f && r.w == 1.0f;
    const fw_v3 o = aligned ? fw_sub3(x, cpos) : fw_quat_mul_vec3(fw_q4{-r.x, -r.y, -r.z, r.w}, fw_sub3(x, cpos));
    if (c.kind == 3 || c.kind == 4) {  // CYLINDER, CONE: solids of revolution about the local Y axis
        const float hh = c.half_extents[1], rr = c.radius * c.radius;
        const float xz = o.x * o.x + o.z * o.z;
        if (c.kind == 3) return fabsf(o.y) <= hh && xz - rr <= 0.0f;
        const float k = c.radius / (hh + hh), k2 = k * k;
        const float wy = o.y - hh;
        return o.y >= -hh && wy <= 0.0f && xz - k2 * (wy * wy) <= 0.0f;
    }
    if (c.kind == 5) {  // CAPSULE
        const float hl = c.half_extents[1], rr = c.radius * c.radius;
        const float xz = o.x * o.x + o.z * o.z;
        const float yc = o.y < -hl ? -hl : (o.y > hl ? hl : o.y);
        const float dy = o.y - yc;
        return (xz + dy * dy) - rr <= 0.0f;
    }
    // BOX
    return fabsf(o.x) <= c.half_extents[0] && fabsf(o.y) <= c.half_extents[1] && fabsf(o.z) <= c.half_extents[2];
}
