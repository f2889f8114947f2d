// fw_project.h -- point projection onto the context's collider world (include/firework_hip.h: POINT QUERIES has the semantics,
// operation by operation; this file is that text in fp32, built with -ffp-contract=off like everything else).  FW_HD: the
// query kernel (fw_k_query.hip) runs fw_project_point on the device, tests/test_point_query_cpu.py the same function on the host.
//
// The particle kernels do not include this header: fw_collide.h is used as it is (FwCollider, FwMeshInst, FwHitId, the vector
// helpers) and left unchanged.
#pragma once
#include "fw_collide.h"
#include "fw_volumes.h"

FW_HD float fw_clamp_sym(float x, float h) { return x < -h ? -h : (x > h ? h : x); }

// One analytic collider.  Returns true when x lies inside or on the solid -- fw_collider_contains (fw_volumes.h): the expression
// fw_ray_collider tests for its distance-0 case, kind by kind; what follows states its operands again, which the compiler folds into
// one evaluation.  Otherwise *q is the nearest point of the solid -- in the collider's own frame for the framed
// kinds (BOX, CYLINDER, CONE, CAPSULE), in the world for PLANE and SPHERE -- and *d2 = dot(w, w) with w = o - q in that frame.
FW_HD bool fw_project_collider(const FwCollider &c, fw_v3 x, fw_v3 *q, float *d2) {
    if (fw_collider_contains(c, x)) return true;
    const fw_v3 cpos{c.position[0], c.position[1], c.position[2]};
    fw_v3 o, p;
    if (c.kind == 0) {  // PLANE
        const fw_v3 n{c.normal[0], c.normal[1], c.normal[2]};
        const float s = fw_dot3(n, fw_sub3(x, cpos));
        o = x, p = fw_sub3(x, fw_scale3(n, s));
    } else if (c.kind == 1) {  // SPHERE
        const fw_v3 v = fw_sub3(x, cpos);
        const float vv = fw_dot3(v, v);
        o = x, p = fw_add3(cpos, fw_scale3(v, c.radius / sqrtf(vv)));
    } else {
        const fw_q4 r{c.rotation[0], c.rotation[1], c.rotation[2], c.rotation[3]};
        const bool aligned = r.x == 0.0f && r.y == 0.0f && r.z == 0.0f && r.w == 1.0f;
        o = aligned ? fw_sub3(x, cpos) : fw_quat_mul_vec3(fw_q4{-r.x, -r.y, -r.z, r.w}, fw_sub3(x, cpos));
        if (c.kind == 3 || c.kind == 4) {
            // CYLINDER, CONE: solids of revolution about the local Y axis -- the nearest point of the profile in (r, y), taken back
            const float hh = c.half_extents[1], rr = c.radius * c.radius;
            const float xz = o.x * o.x + o.z * o.z;
            const float r0 = sqrtf(xz);
            // the cylinder's rectangle: r clamped to [0, radius], y to +-hh; the cone's base segment y = -hh, r in [0, radius] ...
            float pr = r0 > c.radius ? c.radius : r0, py = c.kind == 3 ? fw_clamp_sym(o.y, hh) : -hh;
            if (c.kind == 4) {
                // ... then its slant segment from the rim (radius, -hh) to the apex (0, +hh), by a clamped parameter: only when
                // strictly nearer in the profile
                const float br = r0 - pr, by = o.y - py;
                const float db = br * br + by * by;
                const float h = hh + hh;
                const float ur = r0 - c.radius, uy = o.y + hh;
                float t = (uy * h - ur * c.radius) / (rr + h * h);
                t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                const float sr = c.radius - c.radius * t, sy = h * t - hh;
                const float er = r0 - sr, ey = o.y - sy;
                if (er * er + ey * ey < db) pr = sr, py = sy;
            }
            p = r0 == 0.0f ? fw_v3{pr, py, 0.0f} : fw_v3{pr * o.x / r0, py, pr * o.z / r0};
        } else if (c.kind == 5) {  // CAPSULE
            const float hl = c.half_extents[1];
            const float yc = o.y < -hl ? -hl : (o.y > hl ? hl : o.y);
            const float dy = o.y - yc;
            const fw_v3 v{o.x, dy, o.z};
            const float s = c.radius / sqrtf(fw_dot3(v, v));
            p = fw_v3{v.x * s, yc + v.y * s, v.z * s};
        } else {  // BOX
            const float hx = c.half_extents[0], hy = c.half_extents[1], hz = c.half_extents[2];
            p = fw_v3{fw_clamp_sym(o.x, hx), fw_clamp_sym(o.y, hy), fw_clamp_sym(o.z, hz)};
        }
    }
    const fw_v3 w = fw_sub3(o, p);
    *q = p, *d2 = fw_dot3(w, w);
    return false;
}

// a point of a frame (position, rotation xyzw) in the world: R q + position; the identity rotation skips the product
FW_HD fw_v3 fw_frame_to_world(const float *position, const float *rotation, fw_v3 q) {
    const fw_q4 r{rotation[0], rotation[1], rotation[2], rotation[3]};
    const bool aligned = r.x == 0.0f && r.y == 0.0f && r.z == 0.0f && r.w == 1.0f;
    return fw_add3(aligned ? q : fw_quat_mul_vec3(r, q), fw_v3{position[0], position[1], position[2]});
}

struct FwProjection {
    fw_v3 point;
    float distance;
    uint32_t is_inside;
};

// SpatialQuery::project_point(position, solid = true, filter) over the world: the analytic colliders in index order, then the
// mesh instances; the smaller squared distance wins, replacement by strict < (a candidate whose d2 is NaN or +infinity never
// wins).  `id` is told each time the best candidate changes, as in fw_cast_ray.  Returns false when nothing answered.
template <class Id>
FW_HD bool fw_project_point(const FwCollider *colliders, uint32_t n, const FwMeshInst *meshes, uint32_t n_mesh, uint32_t mask, fw_v3 x,
                            FwProjection *out, Id &id) {
    // (the best so far in scalars: fw_cast_ray's note on structs updated through a pointer inside the loop)
    float bd2 = INFINITY, bqx = 0.0f, bqy = 0.0f, bqz = 0.0f;
    uint32_t bsrc = 0u, bidx = 0u;  // who holds the best: 0 nobody, 1 colliders[bidx], 2 meshes[bidx] -- the frame bq is in
    bool inside = false;
    for (uint32_t i = 0; i < n; i++) {
        if (!(colliders[i].layers & mask)) continue;
#ifdef __HIP_DEVICE_COMPILE__
        {
            // A collider NO lane of the wave can get an answer from is skipped by the whole wave (a uniform branch).  Every point of
            // the collider lies within `bound` of its position, so it is at least |x - position| - bound from x; `far` says that
            // this exceeds the lane's best distance D = sqrt(bd2) by more than 5e-5 (D + bound) (the factor on reach^2).  The
            // candidate's d2 is computed from the same x - position with an error of a few
            // ulps of |x - position| + bound, far below that margin: its d2 is strictly greater than bd2 -- it can neither win nor tie
            // -- and a point inside the solid is within `bound`, never far.  No best yet (D infinite), a plane (bound infinite) and
            // NaN operands compare false: no skip.  The ballot counts the lanes that got here and no others: the mask and the
            // leave at the first containing solid are per lane.
            const fw_v3 dc = fw_sub3(x, fw_v3{colliders[i].position[0], colliders[i].position[1], colliders[i].position[2]});
            const float reach = sqrtf(bd2) + colliders[i].bound;
            const bool far = fw_dot3(dc, dc) > reach * reach * 1.0001f + 1e-12f;
            if (__ballot(!far) == 0ull) continue;
        }
#endif
        fw_v3 q;
        float d2;
        if (fw_project_collider(colliders[i], x, &q, &d2)) {  // the lowest containing solid ends the search: nothing beats it
            inside = true;
            id.analytic(i);
            break;
        }
        if (d2 < bd2) {
            bd2 = d2, bqx = q.x, bqy = q.y, bqz = q.z, bsrc = 1u, bidx = i;
            id.analytic(i);
        }
    }
    if (inside) {
        *out = FwProjection{x, 0.0f, 1u};
        return true;
    }
    for (uint32_t m = 0; m < n_mesh; m++) {
        const FwMeshInst &M = meshes[m];
        if (!(M.layers & mask)) continue;
#ifdef __HIP_DEVICE_COMPILE__
        {  // the wave skip of the analytic loop, against the sphere that contains the placed mesh
            const fw_v3 dc = fw_sub3(x, fw_v3{M.center[0], M.center[1], M.center[2]});
            const float reach = sqrtf(bd2) + M.position[3];
            const bool far = fw_dot3(dc, dc) > reach * reach * 1.0001f + 1e-12f;
            if (__ballot(!far) == 0ull) continue;
        }
#endif
        const fw_v3 mpos{M.position[0], M.position[1], M.position[2]};
        const fw_q4 r{M.rotation[0], M.rotation[1], M.rotation[2], M.rotation[3]};
        const bool aligned = r.x == 0.0f && r.y == 0.0f && r.z == 0.0f && r.w == 1.0f;
        const fw_v3 o = aligned ? fw_sub3(x, mpos) : fw_quat_mul_vec3(fw_q4{-r.x, -r.y, -r.z, r.w}, fw_sub3(x, mpos));
        uint32_t borig = 0xFFFFFFFFu;  // the original index of this instance's best triangle so far
        // The stackless preorder walk of fw_bvh.h: into a node (i + 1; a leaf: its triangles, then its escape) unless its box is
        // further from o than the best so far, else to its escape.  Every step moves i forward, so the walk ends after at most
        // n_nodes steps whatever the point -- NaN included (every comparison false: no node is left out).  No per-lane stack.
        //
        // Why the result is that of testing every triangle: a box contains its triangles and FwBvh::pad more on every side, so
        // the distance to the box is at least `pad` (1e-4 of the mesh's largest coordinate) below the distance to any triangle in
        // it, or zero.  The distances as computed differ from the true ones by a few ulps of (|o| + the largest coordinate): for a
        // point near the mesh that is far below the pad, for a point far from it far below 5e-5 of the distance, which is what
        // the factor on bd2 allows.  So a node is left out only when every triangle in it has a computed d2 strictly above bd2:
        // none of them could win or tie.  A box at bit-equal distance is never left out (`>`, and the factor): the tie rule
        // needs its triangles.
        for (uint32_t i = 0; i < M.n_nodes;) {
            const float4 lo = M.nodes[2 * i], hi = M.nodes[2 * i + 1];
            const uint32_t esc = __builtin_bit_cast(uint32_t, lo.w), leaf = __builtin_bit_cast(uint32_t, hi.w);
            const float gx = fmaxf(fmaxf(lo.x - o.x, o.x - hi.x), 0.0f), gy = fmaxf(fmaxf(lo.y - o.y, o.y - hi.y), 0.0f),
                        gz = fmaxf(fmaxf(lo.z - o.z, o.z - hi.z), 0.0f);
            const bool take = !((gx * gx + gy * gy) + gz * gz > bd2 * 1.0001f);
            uint32_t next = esc;
            if (take && leaf == 0u) next = i + 1u;
            if (take && leaf != 0u) {
                const uint32_t first = leaf >> 4, last = first + (leaf & 15u);
                for (uint32_t k = first; k < last; k++) {
                    const float4 a4 = M.tris[3 * k], b4 = M.tris[3 * k + 1], c4 = M.tris[3 * k + 2];
                    const fw_v3 a{a4.x, a4.y, a4.z}, ab{b4.x, b4.y, b4.z}, ac{c4.x, c4.y, c4.z};
                    const fw_v3 cr = fw_cross(ab, ac);
                    const float cc = fw_dot3(cr, cr);
                    if (!(cc > 0.0f && cc < INFINITY)) continue;  // zero area on the stored edges: a collapsed triangle of a deformable mesh
                    // Ericson 5.1.5 on v0, e1, e2: the region of the triangle's plane o falls in gives the barycentric (v, w)
                    const fw_v3 ap = fw_sub3(o, a);
                    const float d1 = fw_dot3(ab, ap), d2 = fw_dot3(ac, ap);
                    const fw_v3 bp = fw_sub3(ap, ab);
                    const float d3 = fw_dot3(ab, bp), d4 = fw_dot3(ac, bp);
                    const fw_v3 cp = fw_sub3(ap, ac);
                    const float d5 = fw_dot3(ab, cp), d6 = fw_dot3(ac, cp);
                    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
                    float v, w;
                    if (d1 <= 0.0f && d2 <= 0.0f) v = 0.0f, w = 0.0f;                                    // vertex 0
                    else if (d3 >= 0.0f && d4 <= d3) v = 1.0f, w = 0.0f;                                  // vertex 1
                    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) v = d1 / (d1 - d3), w = 0.0f;        // edge 0-1
                    else if (d6 >= 0.0f && d5 <= d6) v = 0.0f, w = 1.0f;                                  // vertex 2
                    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) v = 0.0f, w = d2 / (d2 - d6);        // edge 0-2
                    else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {                          // edge 1-2
                        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1.0f - w;
                    } else {                                                                              // the face
                        const float denom = 1.0f / ((va + vb) + vc);
                        v = vb * denom, w = vc * denom;
                    }
                    const fw_v3 q{(a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w};
                    const fw_v3 wv = fw_sub3(o, q);
                    const float t = fw_dot3(wv, wv);
                    const uint32_t orig = __builtin_bit_cast(uint32_t, a4.w);
                    if (t < bd2 || (t == bd2 && borig != 0xFFFFFFFFu && orig < borig)) {
                        bd2 = t, bqx = q.x, bqy = q.y, bqz = q.z, bsrc = 2u, bidx = m, borig = orig;
                        id.triangle(m, orig);
                    }
                }
            }
            i = next > i + 1u ? next : i + 1u;
        }
    }
    if (bsrc == 0u) {
        *out = FwProjection{fw_v3{0.0f, 0.0f, 0.0f}, 0.0f, 0u};
        return false;
    }
    // the winner's point goes back to the world, and the winner alone takes the square root
    fw_v3 q{bqx, bqy, bqz};
    if (bsrc == 2u) q = fw_frame_to_world(meshes[bidx].position, meshes[bidx].rotation, q);
    else if (colliders[bidx].kind >= 2) q = fw_frame_to_world(colliders[bidx].position, colliders[bidx].rotation, q);
    *out = FwProjection{q, sqrtf(bd2), 0u};
    return true;
}
