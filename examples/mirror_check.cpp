// mirror_check.cpp -- a scenario that touches most of the C++ host mirror (include/firework.hpp): three particle types,
// Global / OnDemand / Nested entries, every curve kind, modifier, transforms, parent velocity, destroyed-particle
// handler, collisions against an analytic world, fused AABB tracking; with the argument `mesh` also against triangle meshes (one
// mesh placed twice, the set replaced and a mesh destroyed half way), and with `deform` against the same meshes created deformable,
// their vertices moved every fifth frame (create_deformable_mesh / update_mesh_vertices); `deform_device` is `deform` with the new
// vertices handed over in DEVICE memory (update_mesh_vertices_device: copied there on the context's stream, no wait) and one more
// line, the device's verdict on the sheet's updates (mesh_update_status); `query` is `mesh` with a batch of 512 rays cast into the
// collider world behind every tenth frame (cast_rays, and cast_rays_device through device buffers of its own) and one more line
// per such frame: the rays that hit something and the digest of the hit records of either form; `capsule` is a scenario of its own -- a
// small fixed world of capsules (both constructors, identity and rotated, one on another layer) over a ground slab, one colliding
// spawner, a batch of rays every tenth frame (tests/test_cpp_host_capsule.py runs the same through the Python mirror); `project` is
// another -- a fixed small world (one collider of each kind plus one mesh instance), a fixed list of points projected onto it
// (project_points, and project_points_device through device buffers of its own), every field's bits printed per point
// (tests/test_cpp_host_project.py); `paths` another -- the same world, a fixed list of hypothetical particles traced through it
// (trace_paths, trace_paths_device), every field's bits printed per path (tests/test_cpp_host_paths.py); `sorted` another -- one spawner whose
// instance records are sorted by view depth every tenth frame through all three forms (tests/test_cpp_host_sorted.py).  Prints, every tenth frame, the live counts and an
// FNV-1a digest of every particle record; tests/test_cpp_host.py runs the same scenario through the Python mirror and
// expects the same lines: both mirrors marshal the reference's settings into the C ABI the same way.
//
//   make -C examples && ./examples/mirror_check
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "firework.hpp"

using namespace firework;

static uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// `mirror_check capsule`: Collider::capsule / Collider::capsule_endpoints through set_colliders, particles that bounce off them, rays
// that name them
static int capsule_scenario() {
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        const std::vector<Collider> world = {
            Collider::Box({0.0f, -0.5f, 0.0f}, {4.0f, 0.5f, 4.0f}),
            Collider::capsule({0.25f, 0.875f, 0.125f}, 0.375f, 1.0f),
            Collider::capsule({-0.75f, 1.0f, 0.5f}, 0.25f, 1.5f, Quat{0.30151135f, 0.0f, 0.30151135f, 0.90453404f}, 3u),
            Collider::capsule_endpoints({-1.0f, 0.25f, -1.0f}, {1.5f, 0.5f, -0.375f}, 0.1875f),
            Collider::capsule_endpoints({1.0f, 2.0f, 1.0f}, {1.125f, 0.75f, 1.0f}, 0.125f, 2u),
            Collider::capsule_endpoints({2.0f, 0.5f, 0.0f}, {2.0f, 0.5f, 0.0f}, 0.5f)};
        app.set_colliders(world);
        ParticleSpawner sp;
        sp.particle_settings.resize(1);
        {
            ParticleSettings &p = sp.particle_settings[0];
            p.lifetime = RandF32::constant(0.75f);
            p.linear_drag = 0.125f;
            p.has_collision_settings = true;
            p.collision_settings = ParticleCollisionSettings{0.5f, 0.25f, false, 1u};
        }
        sp.emission_settings.resize(1);
        {
            EmissionSettings &e = sp.emission_settings[0];
            e.particle_index = 0;
            e.emission_pacing = EmissionPacing::rate(2000.0f);
            e.emission_shape = EmissionShape::Sphere(0.75f);
            e.initial_velocity = {{1.0f, 6.0f}, {0.0f, -1.0f, 0.0f}, 0.0f};
        }
        ParticleSpawnerData *d = app.spawn(sp, Transform{{0.25f, 3.0f, 0.125f}, {}}, 7u);
        std::vector<fw_ray> rays(256);
        for (size_t i = 0; i < rays.size(); i++) {
            fw_ray &r = rays[i];
            r.origin[0] = -2.0f + (float)(i % 16) * 0.25f, r.origin[1] = 3.0f, r.origin[2] = -1.5f + (float)(i / 16) * 0.1875f;
            r.max_distance = 6.0f;
            r.dir[0] = i % 2 ? 0.6f : 0.0f, r.dir[1] = i % 2 ? -0.8f : -1.0f, r.dir[2] = 0.0f;
            r.filter_mask = 1u + (uint32_t)(i % 3);
        }
        const float dt = 1.0f / 60.0f;
        for (int fr = 0; fr < 40; fr++) {
            app.update(dt);
            if (fr % 10 != 9) continue;
            const auto ps = d->particles(0);
            const std::vector<fw_ray_hit> hits = app.cast_rays(rays);
            unsigned per[6] = {0, 0, 0, 0, 0, 0};
            for (const fw_ray_hit &h : hits)
                if (h.kind == FW_HIT_COLLIDER && h.index < 6) per[h.index]++;
            std::printf("frame %d count %u %016llx hits %u %u %u %u %u %u %016llx\n", fr, d->counts()[0],
                        (unsigned long long)fnv(ps.data(), ps.size() * sizeof(fw_particle)), per[0], per[1], per[2], per[3], per[4], per[5],
                        (unsigned long long)fnv(hits.data(), hits.size() * sizeof(fw_ray_hit)));
        }
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}

// `mirror_check project`: one collider of each kind and one mesh instance, 96 points on a lattice through and around them (every
// operand exact in fp32), the three filter masks by turns; one line per point with the bits of every field of its projection
static int project_scenario() {
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        app.set_colliders({Collider::Plane({0.0f, -1.0f, 0.0f}, {0.0f, 1.0f, 0.0f}), Collider::Sphere({1.0f, 0.5f, 0.0f}, 0.75f, 2u),
                           Collider::Box({-2.0f, 0.0f, 0.0f}, {0.5f, 1.0f, 0.5f}, Quat{0.0f, 0.38268343f, 0.0f, 0.92387953f}),
                           Collider::Cylinder({0.0f, 0.5f, -2.0f}, 0.5f, 1.5f, {}, 3u),
                           Collider::Cone({2.0f, 0.0f, 2.0f}, 0.75f, 2.0f, Quat{0.0f, 0.0f, 0.19509032f, 0.98078528f}),
                           Collider::capsule({-0.75f, 1.0f, 1.5f}, 0.25f, 1.5f, Quat{0.30151135f, 0.0f, 0.30151135f, 0.90453404f}, 2u)});
        const fw_mesh ramp = app.create_mesh({-2.0f, -0.25f, -2.0f, 2.0f, -0.25f, -2.0f, 2.0f, 0.25f, 2.0f, -2.0f, 0.25f, 2.0f}, {0, 2, 1, 0, 3, 2});
        app.set_mesh_colliders({MeshCollider{ramp, {0.5f, 1.75f, 0.0f}, Quat{0.0f, 0.38268343f, 0.0f, 0.92387953f}, 3u}});
        std::vector<fw_point> points(96);
        for (size_t i = 0; i < points.size(); i++) {
            fw_point &p = points[i];
            p.position[0] = -3.0f + (float)(i % 8) * 0.875f, p.position[1] = -1.5f + (float)((i / 8) % 4) * 1.125f, p.position[2] = -2.5f + (float)(i / 32) * 2.25f;
            p.filter_mask = 1u + (uint32_t)(i % 3);
        }
        const std::vector<fw_point_projection> host = app.project_points(points);
        std::vector<fw_point_projection> from_device(points.size());
        void *d_points = nullptr, *d_out = nullptr;
        if (hipMalloc(&d_points, points.size() * sizeof(fw_point)) != hipSuccess || hipMalloc(&d_out, points.size() * sizeof(fw_point_projection)) != hipSuccess)
            throw Error(FW_EHIP, "hipMalloc");
        hipStream_t st = (hipStream_t)app.stream();
        if (hipMemcpyAsync(d_points, points.data(), points.size() * sizeof(fw_point), hipMemcpyHostToDevice, st) != hipSuccess) throw Error(FW_EHIP, "hipMemcpyAsync");
        app.project_points_device(d_points, points.size(), d_out);
        if (hipMemcpyAsync(from_device.data(), d_out, points.size() * sizeof(fw_point_projection), hipMemcpyDeviceToHost, st) != hipSuccess)
            throw Error(FW_EHIP, "hipMemcpyAsync");
        app.synchronize();
        (void)hipFree(d_points), (void)hipFree(d_out);
        for (size_t i = 0; i < host.size(); i++) {
            uint32_t w[8];
            std::memcpy(w, &host[i], sizeof w);
            std::printf("point %zu %08x %08x %08x %08x %08x %08x %08x %08x\n", i, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        }
        std::printf("host %016llx device %016llx\n", (unsigned long long)fnv(host.data(), host.size() * sizeof(fw_point_projection)),
                    (unsigned long long)fnv(from_device.data(), from_device.size() * sizeof(fw_point_projection)));
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}

// `mirror_check paths`: the world of `project`, 96 hypothetical particles on the same lattice thrown down and sideways (every operand
// exact in fp32), traced for 24 steps under gravity, drag, restitution and friction (trace_paths with samples, and trace_paths_device
// through device buffers of its own); one line per path with the bits of every field of its result
static int paths_scenario() {
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        app.set_colliders({Collider::Plane({0.0f, -1.0f, 0.0f}, {0.0f, 1.0f, 0.0f}), Collider::Sphere({1.0f, 0.5f, 0.0f}, 0.75f, 2u),
                           Collider::Box({-2.0f, 0.0f, 0.0f}, {0.5f, 1.0f, 0.5f}, Quat{0.0f, 0.38268343f, 0.0f, 0.92387953f}),
                           Collider::Cylinder({0.0f, 0.5f, -2.0f}, 0.5f, 1.5f, {}, 3u),
                           Collider::Cone({2.0f, 0.0f, 2.0f}, 0.75f, 2.0f, Quat{0.0f, 0.0f, 0.19509032f, 0.98078528f}),
                           Collider::capsule({-0.75f, 1.0f, 1.5f}, 0.25f, 1.5f, Quat{0.30151135f, 0.0f, 0.30151135f, 0.90453404f}, 2u)});
        const fw_mesh ramp = app.create_mesh({-2.0f, -0.25f, -2.0f, 2.0f, -0.25f, -2.0f, 2.0f, 0.25f, 2.0f, -2.0f, 0.25f, 2.0f}, {0, 2, 1, 0, 3, 2});
        app.set_mesh_colliders({MeshCollider{ramp, {0.5f, 1.75f, 0.0f}, Quat{0.0f, 0.38268343f, 0.0f, 0.92387953f}, 3u}});
        fw_path_settings settings{};
        settings.dt = 0.03125f, settings.n_steps = 24u, settings.acceleration[1] = -9.75f, settings.linear_drag = 0.125f;
        settings.collision.enabled = 1, settings.collision.restitution = 0.5f, settings.collision.friction = 0.25f, settings.collision.filter_mask = 3u;
        std::vector<fw_path> paths(96);
        for (size_t i = 0; i < paths.size(); i++) {
            fw_path &p = paths[i];
            p.position[0] = -3.0f + (float)(i % 8) * 0.875f, p.position[1] = -1.5f + (float)((i / 8) % 4) * 1.125f, p.position[2] = -2.5f + (float)(i / 32) * 2.25f;
            p.velocity[0] = 1.5f - (float)(i % 5) * 0.75f, p.velocity[1] = -0.5f * (float)(i % 4), p.velocity[2] = (float)(i % 3) - 1.0f;
            p.age = 0.0625f * (float)(i % 2), p.lifetime = 0.25f + 0.125f * (float)(i % 7);
        }
        std::vector<float> samples;
        const std::vector<fw_path_result> host = app.trace_paths(settings, paths, &samples);
        std::vector<fw_path_result> from_device(paths.size());
        std::vector<float> samples_from_device(samples.size());
        void *d_paths = nullptr, *d_out = nullptr, *d_samples = nullptr;
        if (hipMalloc(&d_paths, paths.size() * sizeof(fw_path)) != hipSuccess || hipMalloc(&d_out, paths.size() * sizeof(fw_path_result)) != hipSuccess ||
            hipMalloc(&d_samples, samples.size() * sizeof(float)) != hipSuccess)
            throw Error(FW_EHIP, "hipMalloc");
        hipStream_t st = (hipStream_t)app.stream();
        if (hipMemcpyAsync(d_paths, paths.data(), paths.size() * sizeof(fw_path), hipMemcpyHostToDevice, st) != hipSuccess) throw Error(FW_EHIP, "hipMemcpyAsync");
        app.trace_paths_device(settings, d_paths, paths.size(), d_out, d_samples);
        if (hipMemcpyAsync(from_device.data(), d_out, paths.size() * sizeof(fw_path_result), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(samples_from_device.data(), d_samples, samples.size() * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess)
            throw Error(FW_EHIP, "hipMemcpyAsync");
        app.synchronize();
        (void)hipFree(d_paths), (void)hipFree(d_out), (void)hipFree(d_samples);
        for (size_t i = 0; i < host.size(); i++) {
            uint32_t w[20];
            std::memcpy(w, &host[i], sizeof w);
            std::printf("path %zu", i);
            for (uint32_t x : w) std::printf(" %08x", x);
            std::printf("\n");
        }
        std::printf("host %016llx device %016llx samples %016llx device %016llx\n", (unsigned long long)fnv(host.data(), host.size() * sizeof(fw_path_result)),
                    (unsigned long long)fnv(from_device.data(), from_device.size() * sizeof(fw_path_result)),
                    (unsigned long long)fnv(samples.data(), samples.size() * sizeof(float)),
                    (unsigned long long)fnv(samples_from_device.data(), samples_from_device.size() * sizeof(float)));
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}

// `mirror_check sorted`: one spawner (a sphere of sparks under gravity and drag), and every tenth frame its instance records sorted by
// view depth in both orders through all three forms (instances_sorted; pack_instances_sorted_device and depth_order_device through
// device buffers of its own): one line per frame and order with the digest of each
static int sorted_scenario() {
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        ParticleSpawner sp;
        sp.particle_settings.resize(1);
        sp.particle_settings[0].lifetime = RandF32::constant(0.75f);
        sp.particle_settings[0].linear_drag = 0.125f;
        sp.emission_settings.resize(1);
        {
            EmissionSettings &e = sp.emission_settings[0];
            e.particle_index = 0;
            e.emission_pacing = EmissionPacing::rate(2000.0f);
            e.emission_shape = EmissionShape::Sphere(0.75f);
            e.initial_velocity = {{1.0f, 6.0f}, {0.0f, 1.0f, 0.0f}, 0.5f};
        }
        ParticleSpawnerData *d = app.spawn(sp, Transform{{0.25f, 3.0f, 0.125f}, {}}, 7u);
        const uint64_t cap = 4096;
        void *d_rec = nullptr, *d_ord = nullptr;
        if (hipMalloc(&d_rec, cap * sizeof(fw_particle_instance)) != hipSuccess || hipMalloc(&d_ord, cap * sizeof(uint32_t)) != hipSuccess)
            throw Error(FW_EHIP, "hipMalloc");
        hipStream_t st = (hipStream_t)app.stream();
        const float dt = 1.0f / 60.0f;
        for (int fr = 0; fr < 40; fr++) {
            app.update(dt);
            if (fr % 10 != 9) continue;
            const auto unsorted = d->instances(0);
            for (uint32_t order : {(uint32_t)FW_SORT_BACK_TO_FRONT, (uint32_t)FW_SORT_FRONT_TO_BACK}) {
                fw_sort_view view{};
                view.eye[0] = 0.25f, view.eye[1] = 3.5f, view.eye[2] = 0.125f;
                view.forward[0] = 0.5f, view.forward[1] = -0.25f, view.forward[2] = 1.0f;
                view.order = order;
                const auto host = d->instances_sorted(view, 0);
                const uint64_t ub_r = app.pack_instances_sorted_device(*d, view, d_rec, cap);
                const uint64_t ub_o = app.depth_order_device(*d, view, d_ord, cap);
                std::vector<fw_particle_instance> rec(host.size());
                std::vector<uint32_t> ord(host.size());
                if (host.size() > cap || ub_r < host.size() || ub_o < host.size()) throw Error(FW_EHIP, "bound below the count");
                if (hipMemcpyAsync(rec.data(), d_rec, rec.size() * sizeof(fw_particle_instance), hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipMemcpyAsync(ord.data(), d_ord, ord.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess)
                    throw Error(FW_EHIP, "hipMemcpyAsync");
                app.synchronize();
                std::printf("frame %d order %u count %zu unsorted %016llx host %016llx device %016llx index %016llx\n", fr, order, host.size(),
                            (unsigned long long)fnv(unsorted.data(), unsorted.size() * sizeof(fw_particle_instance)),
                            (unsigned long long)fnv(host.data(), host.size() * sizeof(fw_particle_instance)),
                            (unsigned long long)fnv(rec.data(), rec.size() * sizeof(fw_particle_instance)),
                            (unsigned long long)fnv(ord.data(), ord.size() * sizeof(uint32_t)));
            }
        }
        (void)hipFree(d_rec), (void)hipFree(d_ord);
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}

// `mirror_check aabbs`: three spawners -- two sphere emitters of different rates and an OnDemand one that is fed in frame 15 -- and every
// tenth frame their boxes through all three forms (ParticleSpawnerData::aabb per spawner; ParticleSystemPlugin::aabbs and ::aabbs_device
// over a list that names one spawner twice): one line per frame with the `any` flags, the digest of the batched records of either form
// and the digest of the records the per-spawner calls make
static int aabbs_scenario() {
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        std::vector<ParticleSpawnerData *> ds;
        for (int k = 0; k < 3; k++) {
            ParticleSpawner sp;
            sp.particle_settings.resize(1);
            sp.particle_settings[0].lifetime = RandF32::constant(0.75f);
            sp.particle_settings[0].linear_drag = 0.125f;
            sp.emission_settings.resize(1);
            EmissionSettings &e = sp.emission_settings[0];
            e.particle_index = 0;
            e.emission_pacing = k == 2 ? EmissionPacing::OnDemand() : EmissionPacing::rate(k == 0 ? 2000.0f : 150.0f);
            e.emission_shape = EmissionShape::Sphere(0.75f);
            e.initial_velocity = {{1.0f, 6.0f}, {0.0f, 1.0f, 0.0f}, 0.5f};
            ds.push_back(app.spawn(sp, Transform{{0.25f + 4.0f * (float)k, 3.0f, 0.125f}, {}}, 7u + (uint32_t)k));
        }
        const std::vector<ParticleSpawnerData *> list = {ds[2], ds[0], ds[1], ds[0]};
        void *d_rec = nullptr;
        if (hipMalloc(&d_rec, list.size() * sizeof(fw_aabb)) != hipSuccess) throw Error(FW_EHIP, "hipMalloc");
        hipStream_t st = (hipStream_t)app.stream();
        const float dt = 1.0f / 60.0f;
        for (int fr = 0; fr < 40; fr++) {
            if (fr == 15) ds[2]->queue_particles(33);
            app.update(dt);
            if (fr % 10 != 9) continue;
            app.aabbs_device(list, d_rec);  // (right behind the step: no wait in between)
            const std::vector<fw_aabb> host = app.aabbs(list);
            std::vector<fw_aabb> dev(list.size()), single(list.size());
            if (hipMemcpyAsync(dev.data(), d_rec, dev.size() * sizeof(fw_aabb), hipMemcpyDeviceToHost, st) != hipSuccess) throw Error(FW_EHIP, "hipMemcpyAsync");
            app.synchronize();
            for (size_t i = 0; i < list.size(); i++) {
                Vec3 mn, mx;
                single[i] = fw_aabb{};
                single[i].any = list[i]->aabb(mn, mx) ? 1 : 0;
                single[i].min[0] = mn.x, single[i].min[1] = mn.y, single[i].min[2] = mn.z;
                single[i].max[0] = mx.x, single[i].max[1] = mx.y, single[i].max[2] = mx.z;
            }
            std::printf("frame %d any %d%d%d%d host %016llx device %016llx single %016llx\n", fr, host[0].any, host[1].any, host[2].any, host[3].any,
                        (unsigned long long)fnv(host.data(), host.size() * sizeof(fw_aabb)), (unsigned long long)fnv(dev.data(), dev.size() * sizeof(fw_aabb)),
                        (unsigned long long)fnv(single.data(), single.size() * sizeof(fw_aabb)));
        }
        (void)hipFree(d_rec);
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}

// `mirror_check volumes`: the three spawners of `aabbs` and every tenth frame how many of their particles lie inside six volumes -- a
// half-space that holds everything, then one of every other kind, three of them rotated -- through ParticleSystemPlugin::count_in_volumes
// and ::count_in_volumes_device over a list that names one spawner twice, once by its type and once by -1: one line per frame with the
// counts inside the half-space and the digest of the counts of either form
static int volumes_scenario() {
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        std::vector<ParticleSpawnerData *> ds;
        for (int k = 0; k < 3; k++) {
            ParticleSpawner sp;
            sp.particle_settings.resize(1);
            sp.particle_settings[0].lifetime = RandF32::constant(0.75f);
            sp.particle_settings[0].linear_drag = 0.125f;
            sp.emission_settings.resize(1);
            EmissionSettings &e = sp.emission_settings[0];
            e.particle_index = 0;
            e.emission_pacing = k == 2 ? EmissionPacing::OnDemand() : EmissionPacing::rate(k == 0 ? 2000.0f : 150.0f);
            e.emission_shape = EmissionShape::Sphere(0.75f);
            e.initial_velocity = {{1.0f, 6.0f}, {0.0f, 1.0f, 0.0f}, 0.5f};
            ds.push_back(app.spawn(sp, Transform{{0.25f + 4.0f * (float)k, 3.0f, 0.125f}, {}}, 7u + (uint32_t)k));
        }
        const std::vector<ParticleSystemPlugin::VolumePlace> list = {{ds[2], -1}, {ds[0], 0}, {ds[1], -1}, {ds[0], -1}};
        const Quat q{0.5f, 0.5f, 0.5f, 0.5f};
        const std::vector<Collider> volumes = {Collider::Plane({0.0f, 1000.0f, 0.0f}, {0.0f, 1.0f, 0.0f}), Collider::Sphere({0.25f, 3.25f, 0.125f}, 0.625f),
                                               Collider::Box({4.25f, 3.25f, 0.125f}, {0.5f, 0.625f, 0.375f}, q), Collider::Cylinder({0.25f, 3.25f, 0.125f}, 0.625f, 1.0f),
                                               Collider::Cone({0.25f, 3.25f, 0.125f}, 0.75f, 1.5f, q), Collider::capsule({8.25f, 3.25f, 0.125f}, 0.375f, 0.75f, q)};
        const size_t n = list.size() * volumes.size();
        void *d_cnt = nullptr;
        if (hipMalloc(&d_cnt, n * sizeof(uint32_t)) != hipSuccess) throw Error(FW_EHIP, "hipMalloc");
        hipStream_t st = (hipStream_t)app.stream();
        const float dt = 1.0f / 60.0f;
        for (int fr = 0; fr < 40; fr++) {
            if (fr == 15) ds[2]->queue_particles(33);
            app.update(dt);
            if (fr % 10 != 9) continue;
            app.count_in_volumes_device(list, volumes, d_cnt);  // (right behind the step: no wait in between)
            const std::vector<uint32_t> host = app.count_in_volumes(list, volumes);
            std::vector<uint32_t> dev(n);
            if (hipMemcpyAsync(dev.data(), d_cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess) throw Error(FW_EHIP, "hipMemcpyAsync");
            app.synchronize();
            std::printf("frame %d all %u %u %u %u host %016llx device %016llx\n", fr, host[0], host[volumes.size()], host[2 * volumes.size()], host[3 * volumes.size()],
                        (unsigned long long)fnv(host.data(), n * sizeof(uint32_t)), (unsigned long long)fnv(dev.data(), n * sizeof(uint32_t)));
        }
        (void)hipFree(d_cnt);
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "volumes") == 0) return volumes_scenario();
    if (argc > 1 && std::strcmp(argv[1], "aabbs") == 0) return aabbs_scenario();
    if (argc > 1 && std::strcmp(argv[1], "sorted") == 0) return sorted_scenario();
    if (argc > 1 && std::strcmp(argv[1], "project") == 0) return project_scenario();
    if (argc > 1 && std::strcmp(argv[1], "paths") == 0) return paths_scenario();
    if (argc > 1 && std::strcmp(argv[1], "capsule") == 0) return capsule_scenario();
    // `mirror_check mesh`: the same scenario with triangle meshes in the collider world (create, place twice, replace, destroy)
    // `mirror_check deform`: ... with both meshes deformable: the ramp's far edge rises every fifth frame, then the sheet's apex
    // `mirror_check deform_device`: ... with those vertices taken from device memory
    const bool deform_device = argc > 1 && std::strcmp(argv[1], "deform_device") == 0;
    const bool deform = deform_device || (argc > 1 && std::strcmp(argv[1], "deform") == 0);
    // `mirror_check query`: the `mesh` scenario, and ray-cast queries into its collider world
    const bool query = argc > 1 && std::strcmp(argv[1], "query") == 0;
    const bool with_meshes = deform || query || (argc > 1 && std::strcmp(argv[1], "mesh") == 0);
    try {
        ParticleSystemPlugin app(0, /*seed*/ 0x00C0FFEE);
        // new vertices of a deformable mesh, in host memory or (deform_device) through a device buffer of their own per update --
        // a stand-in for the output of a GPU pass -- filled on the context's stream; freed at the end
        std::vector<void *> device_buffers;
        auto move_vertices = [&](fw_mesh m, const std::vector<float> &xyz) {
            if (!deform_device) return app.update_mesh_vertices(m, xyz);
            void *d = nullptr;
            if (hipMalloc(&d, xyz.size() * sizeof(float)) != hipSuccess) throw Error(FW_EHIP, "hipMalloc");
            device_buffers.push_back(d);
            // (pageable source: the runtime has taken the values when the call returns)
            if (hipMemcpyAsync(d, xyz.data(), xyz.size() * sizeof(float), hipMemcpyHostToDevice, (hipStream_t)app.stream()) != hipSuccess)
                throw Error(FW_EHIP, "hipMemcpyAsync");
            app.update_mesh_vertices_device(m, d, (uint32_t)(xyz.size() / 3));
        };
        // the rays of `query`: a grid 3 above the scene, straight down and slanted by turns, the three filter masks by turns (every
        // operand exact in fp32)
        std::vector<fw_ray> rays(query ? 512 : 0);
        for (size_t i = 0; i < rays.size(); i++) {
            fw_ray &r = rays[i];
            r.origin[0] = -3.0f + (float)(i % 32) * 0.1875f, r.origin[1] = 3.0f, r.origin[2] = -3.0f + (float)(i / 32) * 0.375f;
            r.max_distance = 6.0f;
            r.dir[0] = i % 2 ? 0.6f : 0.0f, r.dir[1] = i % 2 ? -0.8f : -1.0f, r.dir[2] = 0.0f;
            r.filter_mask = 1u + (uint32_t)(i % 3);
        }
        void *d_rays = nullptr, *d_hits = nullptr;
        if (query && (hipMalloc(&d_rays, rays.size() * sizeof(fw_ray)) != hipSuccess || hipMalloc(&d_hits, rays.size() * sizeof(fw_ray_hit)) != hipSuccess))
            throw Error(FW_EHIP, "hipMalloc");
        app.track_aabbs(true);
        app.set_colliders({Collider::Plane({0.0f, -1.0f, 0.0f}, {0.0f, 1.0f, 0.0f}), Collider::Sphere({1.0f, 0.5f, 0.0f}, 0.75f, 2u),
                           Collider::Box({-2.0f, 0.0f, 0.0f}, {0.5f, 1.0f, 0.5f}, Quat{0.0f, 0.38268343f, 0.0f, 0.92387953f})});
        // a ramp of two triangles under the pebbles: as it is on layer 1, and turned about Y a little higher on layer 2
        fw_mesh ramp = -1, sheet = -1;
        if (deform) ramp = app.create_deformable_mesh({-2.0f, -0.25f, -2.0f, 2.0f, -0.25f, -2.0f, 2.0f, 0.25f, 2.0f, -2.0f, 0.25f, 2.0f}, {0, 2, 1, 0, 3, 2});
        if (with_meshes) {
            if (!deform) ramp = app.create_mesh({-2.0f, -0.25f, -2.0f, 2.0f, -0.25f, -2.0f, 2.0f, 0.25f, 2.0f, -2.0f, 0.25f, 2.0f}, {0, 2, 1, 0, 3, 2});
            app.set_mesh_colliders({MeshCollider{ramp, {0.0f, -0.25f, 0.0f}, {}, 1u},
                                    MeshCollider{ramp, {0.5f, 0.25f, 0.0f}, Quat{0.0f, 0.38268343f, 0.0f, 0.92387953f}, 2u}});
        }
        ParticleSpawner sp;
        sp.particle_settings.resize(3);
        uint64_t destroyed_seen = 0;
        {
            ParticleSettings &p = sp.particle_settings[0];  // sparks: one lifetime value, reports its dead
            p.lifetime = RandF32::constant(0.4f);
            p.initial_scale = {0.5f, 2.0f};
            p.scale_curve = FireworkCurve::even_samples({1.0f, 2.0f, 0.5f});
            p.base_color = FireworkGradient::uneven_samples({{0.0f, {10, 7, 1, 1}}, {0.7f, {3, 1, 1, 1}}, {1.0f, {0.1f, 0.1f, 0.1f, 0}}});
            p.linear_drag = 0.3f;
            p.particles_destroyed = [&](const std::vector<fw_particle> &dead) { destroyed_seen += dead.size(); };
        }
        {
            ParticleSettings &p = sp.particle_settings[1];  // smoke: children of the sparks, lifetime range
            p.lifetime = {0.2f, 0.6f};
            p.acceleration = {0.0f, 0.5f, 0.0f};
            p.scale_curve = FireworkCurve::uneven_samples({{0.0f, 1.0f}, {0.8f, 1.2f}, {1.0f, 0.0f}});
            p.emissive_color = FireworkGradient::even_samples({{4, 2, 0, 1}, {0, 0, 0, 1}});
            p.angular_drag = 0.1f;
            p.angular_acceleration = {0.1f, 0.0f, -0.2f};
        }
        {
            ParticleSettings &p = sp.particle_settings[2];  // pebbles: bounce in the collider world
            p.lifetime = {0.5f, 0.9f};
            p.has_collision_settings = true;
            p.collision_settings = ParticleCollisionSettings{0.6f, 0.2f, false, 3u};
            p.pbr = true;
        }
        sp.emission_settings.resize(4);
        {
            EmissionSettings &e = sp.emission_settings[0];
            e.particle_index = 0;
            e.emission_pacing = EmissionPacing::rate(5000.0f);
            e.emission_shape = EmissionShape::Sphere(0.5f);
            e.initial_velocity = {{1.0f, 6.0f}, {0.0f, 1.0f, 0.0f}, 0.0f};
            e.initial_velocity_radial = {1.0f, 2.0f};
        }
        {
            EmissionSettings &e = sp.emission_settings[1];
            e.particle_index = 1;
            e.emission_pacing = EmissionPacing::CountOverDuration(8.0f, 1.0f, 0.1f, 0.9f);
            e.emission_mode = EmissionMode::Nested(0);
            e.inherit_parent_velocity = false;
        }
        {
            EmissionSettings &e = sp.emission_settings[2];
            e.particle_index = 2;
            e.emission_pacing = EmissionPacing::OnDemand();
            e.emission_shape = EmissionShape::Circle({0.0f, 0.0f, 1.0f}, 2.0f);
            e.initial_velocity = {{0.0f, 3.0f}, {0.0f, -1.0f, 0.0f}, 0.0f};
            e.initial_rotation = {0.0f, 0.38941834f, 0.0f, 0.92106099f};
        }
        {
            EmissionSettings &e = sp.emission_settings[3];
            e.particle_index = 2;
            e.emission_pacing = EmissionPacing::OneShot(700);
        }
        ParticleSpawnerData *d = app.spawn(sp, Transform{{0.0f, 1.0f, 0.0f}, {}}, 42u);
        d->set_modifier(EffectModifier{2.0f, 0.5f});
        d->set_parent_velocity({0.5f, 0.0f, -0.25f});
        const float dt = 1.0f / 60.0f;
        for (int fr = 0; fr < 60; fr++) {
            if (fr == 0 || fr == 7 || fr == 8 || fr == 31) d->queue_particles(500 + 10 * fr);
            if (deform && fr % 5 == 0 && fr < 30) {  // the ramp's far edge at 0.25 + fr / 40 (exact in fp32), in both places it is placed
                const float y = 0.25f + 0.125f * (float)(fr / 5);
                move_vertices(ramp, {-2.0f, -0.25f, -2.0f, 2.0f, -0.25f, -2.0f, 2.0f, y, 2.0f, -2.0f, y, 2.0f});
            }
            if (deform && fr % 5 == 0 && fr > 30)  // the sheet's apex rises
                move_vertices(sheet, {-3.0f, 0.0f, -3.0f, 3.0f, 0.0f, -3.0f, 0.0f, 0.5f + 0.25f * (float)(fr / 5 - 6), 3.0f});
            if (with_meshes && fr == 30) {  // another mesh takes the ramp's place (layers 1 | 2, tilted about Z); the ramp is destroyed
                sheet = deform ? app.create_deformable_mesh({-3.0f, 0.0f, -3.0f, 3.0f, 0.0f, -3.0f, 0.0f, 0.5f, 3.0f}, {0, 2, 1})
                               : app.create_mesh({-3.0f, 0.0f, -3.0f, 3.0f, 0.0f, -3.0f, 0.0f, 0.5f, 3.0f}, {0, 2, 1});
                app.set_mesh_colliders({MeshCollider{sheet, {1.0f, 1.5f, 3.0f}, Quat{0.0f, 0.0f, 0.19509032f, 0.98078528f}, 3u}});
                app.destroy_mesh(ramp);
            }
            if (fr == 20) d->set_transform(Transform{{1.0f, 2.0f, 3.0f}, Quat{0.0f, 0.0f, 0.38268343f, 0.92387953f}});
            app.update(dt);
            if (fr % 10 != 9) continue;
            const auto c = d->counts();
            std::printf("frame %d counts %u %u %u", fr, c[0], c[1], c[2]);
            for (uint32_t t = 0; t < 3; t++) {
                const auto ps = d->particles(t);
                std::printf(" %016llx", (unsigned long long)fnv(ps.data(), ps.size() * sizeof(fw_particle)));
            }
            Vec3 mn, mx;
            const bool any = d->aabb(mn, mx);
            const float box[6] = {mn.x, mn.y, mn.z, mx.x, mx.y, mx.z};
            std::printf(" aabb %d %016llx active %d\n", any ? 1 : 0, (unsigned long long)fnv(box, sizeof box), d->active() ? 1 : 0);
            if (query) {
                const std::vector<fw_ray_hit> hits = app.cast_rays(rays);
                std::vector<fw_ray_hit> from_device(rays.size());
                hipStream_t st = (hipStream_t)app.stream();
                if (hipMemcpyAsync(d_rays, rays.data(), rays.size() * sizeof(fw_ray), hipMemcpyHostToDevice, st) != hipSuccess)
                    throw Error(FW_EHIP, "hipMemcpyAsync");
                app.cast_rays_device(d_rays, rays.size(), d_hits);
                if (hipMemcpyAsync(from_device.data(), d_hits, rays.size() * sizeof(fw_ray_hit), hipMemcpyDeviceToHost, st) != hipSuccess)
                    throw Error(FW_EHIP, "hipMemcpyAsync");
                app.synchronize();
                unsigned n_coll = 0, n_mesh = 0;
                for (const fw_ray_hit &h : hits) n_coll += h.kind == FW_HIT_COLLIDER, n_mesh += h.kind == FW_HIT_MESH;
                std::printf("query frame %d colliders %u meshes %u host %016llx device %016llx\n", fr, n_coll, n_mesh,
                            (unsigned long long)fnv(hits.data(), hits.size() * sizeof(fw_ray_hit)),
                            (unsigned long long)fnv(from_device.data(), from_device.size() * sizeof(fw_ray_hit)));
            }
        }
        std::printf("destroyed reported %llu\n", (unsigned long long)destroyed_seen);
        if (deform_device) {
            app.synchronize();
            const auto s = app.mesh_update_status(sheet);
            std::printf("sheet device updates %llu %llu %lld\n", (unsigned long long)s.applied, (unsigned long long)s.rejected, (long long)s.first_bad_vertex);
            for (void *d : device_buffers) (void)hipFree(d);
        }
        if (query) (void)hipFree(d_rays), (void)hipFree(d_hits);
    } catch (const Error &e) {
        std::fprintf(stderr, "firework error %d: %s\n", (int)e.status, e.what());
        return 1;
    }
    return 0;
}
