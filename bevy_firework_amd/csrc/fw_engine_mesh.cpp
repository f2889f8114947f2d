// fw_engine_mesh.cpp -- the collider meshes of a context: fw_ctx_create_mesh / fw_ctx_destroy_mesh / fw_ctx_set_mesh_colliders
// (include/firework_hip.h: fw_mesh_collider has the ray-cast semantics; fw_collide.h walks what is uploaded here; fw_bvh.cpp
// builds the hierarchy)
#include "fw_bvh.h"
#include "fw_engine.h"

namespace {

bool mesh_alive(const fw_ctx *ctx, fw_mesh h) { return h >= 0 && (size_t)h < ctx->meshes.size() && ctx->meshes[h].alive; }

// fw_quat_mul_vec3 in double: v * (w^2 - b.b) + b * (2 v.b) + (b x v) * (2 w)
void quat_mul_vec3_d(const float *q, const double *v, double *out) {
    const double bx = q[0], by = q[1], bz = q[2], w = q[3];
    const double k0 = w * w - (bx * bx + by * by + bz * bz), k1 = 2.0 * (v[0] * bx + v[1] * by + v[2] * bz), k2 = 2.0 * w;
    const double cx = by * v[2] - v[1] * bz, cy = bz * v[0] - v[2] * bx, cz = bx * v[1] - v[0] * by;
    out[0] = v[0] * k0 + bx * k1 + cx * k2, out[1] = v[1] * k0 + by * k1 + cy * k2, out[2] = v[2] * k0 + bz * k1 + cz * k2;
}

}  // namespace

extern "C" {

fw_status fw_ctx_create_mesh(fw_ctx *ctx, const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                             fw_mesh *out) {
    if (out) *out = -1;
    if (!ctx || !out) return fail(ctx, FW_EINVAL, "fw_ctx_create_mesh: bad arguments");
    hipSetDevice(ctx->device);
    try {
        FwBvh bvh;
        std::string why;
        if (fw_bvh_build(xyz, n_vertices, indices, n_triangles, &bvh, &why)) return fail(ctx, FW_EINVAL, "fw_ctx_create_mesh: " + why);
        fw_ctx::MeshHost m;
        fw_status st;
        if ((st = alloc_buf(ctx, m.nodes, (size_t)bvh.n_nodes * 2)) || (st = alloc_buf(ctx, m.tris, (size_t)bvh.n_tris * 3))) return st;
        FW_HIP(ctx, hipMemcpy(m.nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(float), hipMemcpyHostToDevice));
        FW_HIP(ctx, hipMemcpy(m.tris, bvh.tris.data(), bvh.tris.size() * sizeof(float), hipMemcpyHostToDevice));
        m.n_nodes = bvh.n_nodes, m.n_tris = bvh.n_tris;
        double r2 = 0.0;
        for (int k = 0; k < 3; k++) {
            m.center[k] = (float)(((double)bvh.lo[k] + bvh.hi[k]) * 0.5);
            const double h = std::max((double)bvh.hi[k] - m.center[k], (double)m.center[k] - bvh.lo[k]);
            r2 += h * h;
        }
        m.radius = (float)(std::sqrt(r2) * 1.0001);
        m.alive = true;
        fw_mesh h = -1;
        for (size_t i = 0; i < ctx->meshes.size() && h < 0; i++)
            if (!ctx->meshes[i].alive) h = (fw_mesh)i;
        if (h < 0) {
            ctx->meshes.emplace_back();
            h = (fw_mesh)ctx->meshes.size() - 1;
        }
        ctx->meshes[h] = std::move(m);
        *out = h;
        return FW_OK;
    } catch (const std::bad_alloc &) {
        return fail(ctx, FW_ENOMEM, "fw_ctx_create_mesh: out of host memory");
    }
}

fw_status fw_ctx_destroy_mesh(fw_ctx *ctx, fw_mesh mesh) {
    if (!ctx) return FW_EINVAL;
    if (!mesh_alive(ctx, mesh)) return fail(ctx, FW_EINVAL, "fw_ctx_destroy_mesh: unknown mesh handle");
    if (std::find(ctx->mesh_set.begin(), ctx->mesh_set.end(), mesh) != ctx->mesh_set.end())
        return fail(ctx, FW_EINVAL, "fw_ctx_destroy_mesh: the current instance set places this mesh");
    hipSetDevice(ctx->device);
    fw_status st = sync(ctx);  // (frames in flight may still walk it under an older instance set)
    if (st) return st;
    ctx->meshes[mesh] = fw_ctx::MeshHost{};
    return FW_OK;
}

fw_status fw_ctx_set_mesh_colliders(fw_ctx *ctx, const fw_mesh_collider *inst, uint32_t n) {
    if (!ctx || (n && !inst)) return fail(ctx, FW_EINVAL, "bad mesh instance set");
    for (uint32_t i = 0; i < n; i++)
        if (!mesh_alive(ctx, inst[i].mesh)) return fail(ctx, FW_EINVAL, "fw_ctx_set_mesh_colliders: unknown mesh handle");
    hipSetDevice(ctx->device);
    // staged in pinned memory and copied by the stream itself, like fw_ctx_set_colliders: moving instances every frame does not
    // stall the frames in flight
    const int slot = (int)(ctx->mesh_seq++ & 1u);
    if (ctx->mesh_pending[slot]) {
        FW_HIP(ctx, hipEventSynchronize(ctx->ev_mesh[slot]));
        ctx->mesh_pending[slot] = false;
    }
    if (!ctx->ev_mesh[slot]) FW_HIP(ctx, ctx->ev_mesh[slot].create());
    const size_t ncap = std::max<size_t>(16, (size_t)n * 2);
    fw_status st;
    if (n > ctx->h_mesh_inst[slot].cap() && (st = alloc_buf(ctx, ctx->h_mesh_inst[slot], ncap, Mem::pinned))) return st;
    if (n > ctx->d_mesh_inst.cap()) {  // a larger set than ever before: the one case that waits (kernels in flight read the old table)
        HipBuf<FwMeshInst> nb;         // (made before the old table goes: a failure keeps the previous set)
        if ((st = alloc_buf(ctx, nb, ncap)) || (st = sync(ctx))) return st;
        ctx->d_mesh_inst = std::move(nb);
        ctx->g.mesh_inst = ctx->d_mesh_inst;
    }
    std::vector<fw_mesh> set(n);
    for (uint32_t i = 0; i < n; i++) {
        const fw_mesh_collider &c = inst[i];
        const fw_ctx::MeshHost &m = ctx->meshes[c.mesh];
        FwMeshInst &d = ctx->h_mesh_inst[slot][i];
        d = FwMeshInst{};
        memcpy(d.position, c.position, sizeof c.position);
        memcpy(d.rotation, c.rotation, sizeof c.rotation);
        d.nodes = m.nodes, d.tris = m.tris, d.n_nodes = m.n_nodes, d.layers = c.layers;
        // the sphere that contains the placed mesh (the wave skip of fw_cast_ray): a ray meets the instance where
        // R^-1 (x - position) lies in the mesh, R^-1 scaling lengths by s = |rotation|^2 -- centre position + R c / s, radius r / s
        const double s = (double)c.rotation[0] * c.rotation[0] + (double)c.rotation[1] * c.rotation[1] +
                         (double)c.rotation[2] * c.rotation[2] + (double)c.rotation[3] * c.rotation[3];
        const double lc[3] = {m.center[0], m.center[1], m.center[2]};
        double rc[3];
        quat_mul_vec3_d(c.rotation, lc, rc);
        double big = 0.0;
        for (int k = 0; k < 3; k++) {
            d.center[k] = (float)(c.position[k] + rc[k] / (s * s));
            big = std::max(big, std::fabs((double)c.position[k]) + std::fabs(rc[k] / (s * s)));
        }
        d.position[3] = (float)(m.radius / s * 1.001 + 1e-5 * big);
        if (!(s > 0.0) || !std::isfinite(d.position[3]) || !std::isfinite(d.center[0] + d.center[1] + d.center[2]))
            d.position[3] = INFINITY, memcpy(d.center, c.position, sizeof c.position);  // (never skipped)
        set[i] = c.mesh;
    }
    if (n) {
        FW_HIP(ctx, hipMemcpyAsync(ctx->d_mesh_inst, ctx->h_mesh_inst[slot], n * sizeof(FwMeshInst), hipMemcpyHostToDevice, ctx->stream));
        FW_HIP(ctx, hipEventRecord(ctx->ev_mesh[slot], ctx->stream));
        ctx->mesh_pending[slot] = true;
    }
    ctx->mesh_set.swap(set);
    ctx->g.n_mesh_inst = n;
    ctx->fc_ok = false, ctx->boxes_epoch = 0;
    return FW_OK;
}

}  // extern "C"
