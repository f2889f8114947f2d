// fw_engine_mesh.cpp -- the collider meshes of a context: fw_ctx_create_mesh / fw_ctx_create_deformable_mesh /
// fw_ctx_update_mesh_vertices / fw_ctx_update_mesh_vertices_device / fw_ctx_mesh_update_status / fw_ctx_destroy_mesh /
// fw_ctx_set_mesh_colliders
// (include/firework_hip.h: fw_mesh_collider has the ray-cast semantics; fw_collide.h walks what is uploaded here; fw_bvh.cpp
// builds the hierarchy; fw_k_refit.hip redoes its boxes and triangles from new vertices)
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

// the sphere around the root's (padded) box, in the mesh's own frame
void bounding_sphere(const float *lo, const float *hi, float *center, float *radius) {
    double r2 = 0.0;
    for (int k = 0; k < 3; k++) {
        center[k] = (float)(((double)lo[k] + hi[k]) * 0.5);
        const double h = std::max((double)hi[k] - center[k], (double)center[k] - lo[k]);
        r2 += h * h;
    }
    *radius = (float)(std::sqrt(r2) * 1.0001);
}

fw_status create_mesh(fw_ctx *ctx, const char *who, bool deformable, const float *xyz, uint32_t n_vertices, const uint32_t *indices,
                      uint32_t n_triangles, fw_mesh *out) {
    if (out) *out = -1;
    if (!ctx || !out) return fail(ctx, FW_EINVAL, std::string(who) + ": bad arguments");
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    try {
        FwBvh bvh;
        std::string why;
        if (deformable ? fw_bvh_build_deformable(xyz, n_vertices, indices, n_triangles, &bvh, &why)
                       : fw_bvh_build(xyz, n_vertices, indices, n_triangles, &bvh, &why))
            return fail(ctx, FW_EINVAL, std::string(who) + ": " + why);
        fw_ctx::MeshHost m;  // (a failure below releases what it holds so far: the context stays as it was)
        fw_status st;
        if ((st = alloc_buf(ctx, m.nodes, (size_t)bvh.n_nodes * 2)) || (st = alloc_buf(ctx, m.tris, (size_t)bvh.n_tris * 3))) return st;
        FW_HIP(ctx, hipMemcpy(m.nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(float), hipMemcpyHostToDevice));
        FW_HIP(ctx, hipMemcpy(m.tris, bvh.tris.data(), bvh.tris.size() * sizeof(float), hipMemcpyHostToDevice));
        m.n_nodes = bvh.n_nodes, m.n_tris = bvh.n_tris;
        bounding_sphere(bvh.lo, bvh.hi, m.center, &m.radius);
        memcpy(m.lo, bvh.lo, sizeof m.lo), memcpy(m.hi, bvh.hi, sizeof m.hi), m.pad = bvh.pad;
        if (deformable) {
            const size_t nf = (size_t)n_vertices * 3;
            if ((st = alloc_buf(ctx, m.slots, (size_t)bvh.n_tris)) || (st = alloc_buf(ctx, m.order, (size_t)bvh.n_nodes)) ||
                (st = alloc_buf(ctx, m.level_off, bvh.level_off.size())) || (st = alloc_buf(ctx, m.xyz, nf)) ||
                (st = alloc_buf(ctx, m.h_xyz.h[0], nf, Mem::pinned)) || (st = alloc_buf(ctx, m.h_xyz.h[1], nf, Mem::pinned)))
                return st;
            FW_HIP(ctx, hipMemcpy(m.slots, bvh.slots.data(), bvh.slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            FW_HIP(ctx, hipMemcpy(m.order, bvh.order.data(), bvh.order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            FW_HIP(ctx, hipMemcpy(m.level_off, bvh.level_off.data(), bvh.level_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            FW_HIP(ctx, hipMemcpy(m.xyz, xyz, nf * sizeof(float), hipMemcpyHostToDevice));
            m.h_level_off = std::move(bvh.level_off);
            m.referenced.assign(n_vertices, 0);
            for (size_t i = 0; i < (size_t)n_triangles * 3; i++) m.referenced[indices[i]] = 1;
            m.deformable = true, m.n_vertices = n_vertices;
        }
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
        return fail(ctx, FW_ENOMEM, std::string(who) + ": out of host memory");
    }
}

// the staging slot of the next set, free and large enough for n instances (the one wait: the copy before the previous one)
fw_status reserve_staging(fw_ctx *ctx, uint32_t n, FwMeshInst **out = nullptr) {
    return ctx->h_mesh_inst.take(ctx, n, std::max<size_t>(16, (size_t)n * 2), out);
}

// The instance set into the staging slot of its turn and, as one copy, into the context's stream, like fw_ctx_set_colliders -- moving
// instances every frame does not stall the frames in flight.  The device table must hold n.
fw_status stage_instances(fw_ctx *ctx, const fw_mesh_collider *inst, uint32_t n) {
    FwMeshInst *h;
    fw_status st = reserve_staging(ctx, n, &h);
    if (st) return st;
    for (uint32_t i = 0; i < n; i++) {
        const fw_mesh_collider &c = inst[i];
        const fw_ctx::MeshHost &m = ctx->meshes[c.mesh];
        FwMeshInst &d = h[i];
        d = FwMeshInst{};
        memcpy(d.position, c.position, sizeof c.position);
        memcpy(d.rotation, c.rotation, sizeof c.rotation);
        d.nodes = m.nodes, d.tris = m.tris, d.n_nodes = m.n_nodes, d.layers = c.layers;
        if (m.dev_bounds) {  // only the device knows this mesh's box: never skipped until fw_k_mesh_spheres (below) has been there
            d.position[3] = INFINITY, memcpy(d.center, c.position, sizeof c.position);
            continue;
        }
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
    }
    if (n) {
        FW_HIP(ctx, hipMemcpyAsync(ctx->d_mesh_inst, h, n * sizeof(FwMeshInst), hipMemcpyHostToDevice, ctx->stream));
        if ((st = ctx->h_mesh_inst.commit(ctx, ctx->stream))) return st;
        // behind the copy, in the same stream: the spheres of the meshes whose bounds are the device's, one launch per such mesh
        for (uint32_t i = 0; i < n; i++) {
            fw_ctx::MeshHost &m = ctx->meshes[inst[i].mesh];
            if (!m.dev_bounds || m.sphere_stamp == ctx->h_mesh_inst.turn) continue;
            m.sphere_stamp = ctx->h_mesh_inst.turn;
            FW_HIP(ctx, fw_launch_mesh_spheres(ctx->stream, ctx->d_mesh_inst, n, m.nodes, m.d_rec, false));
        }
    }
    return FW_OK;
}

// what only a mesh whose vertices come from device memory needs, made by its first fw_ctx_update_mesh_vertices_device:
// fw_ctx::kMeshDeviceAllocs allocations, all or none (a failure releases what it got and leaves the mesh as it was)
fw_status reserve_device_form(fw_ctx *ctx, fw_ctx::MeshHost &m) {
    if (m.d_rec) return FW_OK;
    HipBuf<FwMeshRecord> rec;
    HipBuf<FwVtxAcc> partials;
    HipBuf<uint8_t> referenced;
    HipBuf<FwMeshReport> report;
    fw_status st;
    if ((st = alloc_buf(ctx, rec, 1)) || (st = alloc_buf(ctx, partials, fw_mesh_bounds_partials(m.n_vertices))) ||
        (st = alloc_buf(ctx, referenced, m.n_vertices)) || (st = alloc_buf(ctx, report, 1, Mem::pinned)))
        return st;
    FwMeshRecord r{};
    r.first_bad = -1;
    *report.get() = FwMeshReport{0ull, 0ull, -1ll};
    FW_HIP(ctx, hipMemcpy(rec, &r, sizeof r, hipMemcpyHostToDevice));
    FW_HIP(ctx, hipMemcpy(referenced, m.referenced.data(), m.n_vertices, hipMemcpyHostToDevice));
    m.d_rec = std::move(rec), m.d_partials = std::move(partials), m.d_referenced = std::move(referenced), m.h_report = std::move(report);
    return FW_OK;
}

}  // namespace

extern "C" {

fw_status fw_ctx_create_mesh(fw_ctx *ctx, const float *xyz, uint32_t n_vertices, const uint32_t *indices, uint32_t n_triangles,
                             fw_mesh *out) {
    return create_mesh(ctx, "fw_ctx_create_mesh", false, xyz, n_vertices, indices, n_triangles, out);
}

fw_status fw_ctx_create_deformable_mesh(fw_ctx *ctx, const float *xyz, uint32_t n_vertices, const uint32_t *indices,
                                        uint32_t n_triangles, fw_mesh *out) {
    return create_mesh(ctx, "fw_ctx_create_deformable_mesh", true, xyz, n_vertices, indices, n_triangles, out);
}

fw_status fw_ctx_update_mesh_vertices(fw_ctx *ctx, fw_mesh mesh, const float *xyz, uint32_t n_vertices) {
    if (!ctx) return FW_EINVAL;
    if (!mesh_alive(ctx, mesh)) return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices: unknown mesh handle");
    fw_ctx::MeshHost &m = ctx->meshes[mesh];
    if (!m.deformable) return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices: the mesh was not created as deformable");
    if (!xyz || n_vertices != m.n_vertices) return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices: the vertex count differs from the creation's");
    const size_t nf = (size_t)n_vertices * 3;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    const bool placed = std::find(ctx->mesh_set.begin(), ctx->mesh_set.end(), mesh) != ctx->mesh_set.end();
    fw_status st;  // (the one allocation an update can need comes first: a failure leaves the mesh as it was)
    if (placed && (st = reserve_staging(ctx, (uint32_t)ctx->mesh_insts.size()))) return st;
    // the staging slot of this call's turn (sized at creation), then ONE pass over the caller's array: finite check, copy into the
    // slot, bounds and pad (a refused call leaves the slot unused: its turn comes again)
    float *h, lo[3], hi[3], pad;
    if ((st = m.h_xyz.take(ctx, nf, nf, &h))) return st;
    const int64_t bad = fw_bvh_stage_vertices(xyz, m.referenced.data(), n_vertices, h, lo, hi, &pad);
    if (bad >= 0) return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices: non-finite vertex " + std::to_string(bad));
    FW_HIP(ctx, hipMemcpyAsync(m.xyz, h, nf * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if ((st = m.h_xyz.commit(ctx, ctx->stream))) return st;
    // The refit behind the copy, IN PLACE: nodes and triangles are rewritten where the frames walk them.  That is safe because
    // every launch that casts rays runs on this same stream (a colliding ring or small type never goes to the side stream:
    // launch_fifo, fw_ctx::small_last_side), so the frames enqueued before this call have read the old shape before the refit
    // starts, and the frames after it start when it is done.
    FwRefit R{};
    R.nodes = reinterpret_cast<FwR4 *>(m.nodes.get()), R.tris = reinterpret_cast<FwR4 *>(m.tris.get());
    R.slots = m.slots, R.xyz = m.xyz, R.order = m.order, R.pad = pad;
    FW_HIP(ctx, fw_launch_mesh_refit(ctx->stream, R, m.level_off, m.h_level_off.data(), (uint32_t)m.h_level_off.size() - 1));
    // the instances of the current set that place this mesh carry its bounding sphere: restaged, in the same stream order
    // (the host's sphere changes for good only once they are on their way)
    // (the bounds are the host's again, whatever device-form updates came before)
    const float center0[3] = {m.center[0], m.center[1], m.center[2]}, radius0 = m.radius;
    const bool dev0 = m.dev_bounds;
    bounding_sphere(lo, hi, m.center, &m.radius);
    m.dev_bounds = false;
    if (placed && (st = stage_instances(ctx, ctx->mesh_insts.data(), (uint32_t)ctx->mesh_insts.size()))) {
        memcpy(m.center, center0, sizeof center0), m.radius = radius0, m.dev_bounds = dev0;
        return st;
    }
    memcpy(m.lo, lo, sizeof lo), memcpy(m.hi, hi, sizeof hi), m.pad = pad;
    drop_forecast_and_boxes(ctx);
    return FW_OK;
}

fw_status fw_ctx_update_mesh_vertices_device(fw_ctx *ctx, fw_mesh mesh, const void *d_xyz, uint32_t n_vertices) {
    if (!ctx) return FW_EINVAL;
    if (!mesh_alive(ctx, mesh)) return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices_device: unknown mesh handle");
    fw_ctx::MeshHost &m = ctx->meshes[mesh];
    if (!m.deformable) return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices_device: the mesh was not created as deformable");
    if (!d_xyz || n_vertices != m.n_vertices)
        return fail(ctx, FW_EINVAL, "fw_ctx_update_mesh_vertices_device: the vertex count differs from the creation's");
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st;  // (the allocations of a mesh's first call come first: a failure leaves the mesh as it was, for both forms)
    if ((st = reserve_device_form(ctx, m))) return st;
    // Everything below is launches into the context's stream: no wait, no pass over the vertices, no copy of them.
    //   1. bounds: every vertex checked, the referenced ones reduced; one workgroup folds the partials into the record and the
    //      report.  A record that has held the host's box until now takes it when this update is rejected (the seed), so that it
    //      always describes the last accepted shape.
    //   2. the refit, gathering straight from d_xyz, with the record's pad -- nothing when the record says rejected.
    //   3. the spheres of the instances that place the mesh, in place in the device table -- nothing when rejected.
    // In-place is safe for the reason the host form gives: every launch that casts rays runs on this stream.
    FwMeshSeed seed;
    memcpy(seed.lo, m.lo, sizeof m.lo), memcpy(seed.hi, m.hi, sizeof m.hi), seed.pad = m.pad;
    FW_HIP(ctx, fw_launch_mesh_bounds(ctx->stream, static_cast<const float *>(d_xyz), m.d_referenced, n_vertices, m.d_partials, m.d_rec,
                                      m.h_report, m.dev_bounds ? nullptr : &seed));
    FwRefit R{};
    R.nodes = reinterpret_cast<FwR4 *>(m.nodes.get()), R.tris = reinterpret_cast<FwR4 *>(m.tris.get());
    R.slots = m.slots, R.xyz = static_cast<const float *>(d_xyz), R.order = m.order, R.rec = m.d_rec;
    FW_HIP(ctx, fw_launch_mesh_refit(ctx->stream, R, m.level_off, m.h_level_off.data(), (uint32_t)m.h_level_off.size() - 1));
    m.dev_bounds = true;
    if (std::find(ctx->mesh_set.begin(), ctx->mesh_set.end(), mesh) != ctx->mesh_set.end())
        FW_HIP(ctx, fw_launch_mesh_spheres(ctx->stream, ctx->d_mesh_inst, ctx->g.n_mesh_inst, m.nodes, m.d_rec, true));
    drop_forecast_and_boxes(ctx);
    return FW_OK;
}

fw_status fw_ctx_mesh_update_status(fw_ctx *ctx, fw_mesh mesh, uint64_t *n_applied, uint64_t *n_rejected, int64_t *first_bad_vertex) {
    if (!ctx) return FW_EINVAL;
    if (!mesh_alive(ctx, mesh)) return fail(ctx, FW_EINVAL, "fw_ctx_mesh_update_status: unknown mesh handle");
    const fw_ctx::MeshHost &m = ctx->meshes[mesh];
    if (!m.deformable) return fail(ctx, FW_EINVAL, "fw_ctx_mesh_update_status: the mesh was not created as deformable");
    const volatile FwMeshReport *r = m.h_report.get();  // (null: no device-form update yet)
    if (n_applied) *n_applied = r ? r->n_applied : 0;
    if (n_rejected) *n_rejected = r ? r->n_rejected : 0;
    if (first_bad_vertex) *first_bad_vertex = r ? r->first_bad : -1;
    return FW_OK;
}

fw_status fw_ctx_destroy_mesh(fw_ctx *ctx, fw_mesh mesh) {
    if (!ctx) return FW_EINVAL;
    if (!mesh_alive(ctx, mesh)) return fail(ctx, FW_EINVAL, "fw_ctx_destroy_mesh: unknown mesh handle");
    if (std::find(ctx->mesh_set.begin(), ctx->mesh_set.end(), mesh) != ctx->mesh_set.end())
        return fail(ctx, FW_EINVAL, "fw_ctx_destroy_mesh: the current instance set places this mesh");
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
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
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    const size_t ncap = std::max<size_t>(16, (size_t)n * 2);
    fw_status st;
    try {
        std::vector<fw_mesh> set(n);
        std::vector<fw_mesh_collider> insts(inst, inst + n);
        for (uint32_t i = 0; i < n; i++) set[i] = inst[i].mesh;
        if ((st = reserve_staging(ctx, n))) return st;
        if (n > ctx->d_mesh_inst.cap()) {  // a larger set than ever before: the one case that waits (kernels in flight read the old table)
            HipBuf<FwMeshInst> nb;         // (made before the old table goes: a failure keeps the previous set)
            if ((st = alloc_buf(ctx, nb, ncap)) || (st = sync(ctx))) return st;
            ctx->d_mesh_inst = std::move(nb);
            ctx->g.mesh_inst = ctx->d_mesh_inst;
        }
        if ((st = stage_instances(ctx, inst, n))) return st;
        ctx->mesh_set.swap(set);
        ctx->mesh_insts.swap(insts);
    } catch (const std::bad_alloc &) {
        return fail(ctx, FW_ENOMEM, "fw_ctx_set_mesh_colliders: out of host memory");
    }
    ctx->g.n_mesh_inst = n;
    drop_forecast_and_boxes(ctx);
    return FW_OK;
}

}  // extern "C"
