// fw_trace.h -- the path query's arithmetic (include/firework_hip.h: PATH QUERIES; fw_ctx_trace_paths / fw_ctx_trace_paths_device): one
// hypothetical particle through n_steps frames of update_particles (reference src/core.rs:594-643) restricted to age, position and
// velocity.  fw_trace_path is the step loop for ONE path and nothing else: the collision is fw_particle_collision of fw_collide.h
// itself -- the function the update kernels call -- told to report its hits (FwPathContacts), the velocity step the expression of
// fw_integrate_store (fw_dev.h).  FW_HD: the kernel (fw_k_query.hip) and a host program (tests) compile the same lines.
#pragma once
#include "fw_collide.h"

// fw_path_settings as the kernel takes it (fw_engine_query.cpp fills it from the caller's record, once per call)
struct FwPathSettings {
    float dt;
    uint32_t n_steps;
    float acc[3];
    float lin_drag;
    uint32_t coll_on, coll_kill, coll_mask;
    float coll_restitution, coll_friction;
};

enum { FW_TRACE_RUNNING = 0, FW_TRACE_EXPIRED = 1, FW_TRACE_DESTROYED = 2 };  // FW_PATH_* of the header

// the observer of fw_particle_collision that keeps the FIRST contact of a path and counts them all
struct FwPathContacts {
    using Id = FwHitId;
    fw_v3 point{0.0f, 0.0f, 0.0f}, normal{0.0f, 0.0f, 0.0f};
    uint32_t step = 0xFFFFFFFFu, now = 0u, n = 0u;  // step of the first contact; the step under way
    FwHitId who;                                    // (starts as the miss: FW_HIT_NONE, index = triangle = ~0)
    FW_HD void hit(fw_v3 at, fw_v3 nrm, float, const FwHitId &id) {
        if (n == 0u) point = at, normal = nrm, step = now, who = id;
        n++;
    }
};

struct FwPathEnd {  // fw_path_result without its contact fields (those are FwPathContacts')
    fw_v3 pos, vel;
    float age;
    uint32_t steps, status;
};

// Sample: told {position, age} after every step (fw_path_result's SAMPLES; a path that has ended repeats its final values), or
// nothing at all -- `on` false, and a path that has ended leaves the loop
struct FwNoSamples {
    static constexpr bool on = false;
    FW_HD void operator()(uint32_t, fw_v3, float) const {}
};

template <class Sample>
FW_HD FwPathEnd fw_trace_path(const FwCollider *colliders, uint32_t n_colliders, const FwMeshInst *meshes, uint32_t n_mesh, const FwPathSettings &s,
                              fw_v3 pos, fw_v3 vel, float age, float lifetime, FwPathContacts &contacts, const Sample &sample) {
    uint32_t steps = 0u, status = FW_TRACE_RUNNING;
    for (uint32_t k = 0; k < s.n_steps; k++) {
        // a path that has ended stays out of the block below: on the device its lane is INACTIVE for every cast the others still run
        if (status == FW_TRACE_RUNNING) {
            age += s.dt;  // core.rs:594
            if (age >= lifetime) {
                status = FW_TRACE_EXPIRED;  // core.rs:595-599: position and velocity as they were, the advanced age
            } else {
                bool killed = false;
                if (s.coll_on != 0u) {
                    contacts.now = k;
                    killed = fw_particle_collision(&pos, &vel, s.dt, s.coll_restitution, s.coll_friction, s.coll_kill != 0u, s.coll_mask, colliders,
                                                   n_colliders, meshes, n_mesh, contacts);
                } else {
                    pos = fw_v3{pos.x + vel.x * s.dt, pos.y + vel.y * s.dt, pos.z + vel.z * s.dt};
                }
                if (killed) {
                    status = FW_TRACE_DESTROYED;
                } else {
                    vel = fw_v3{vel.x + (s.acc[0] - vel.x * s.lin_drag) * s.dt, vel.y + (s.acc[1] - vel.y * s.lin_drag) * s.dt,
                                vel.z + (s.acc[2] - vel.z * s.lin_drag) * s.dt};
                    steps++;
                }
            }
        } else if (!sample.on) {
            break;
        }
        sample(k, pos, age);
    }
    return FwPathEnd{pos, vel, age, steps, status};
}
