"""The path query (include/firework_hip.h: PATH QUERIES) in numpy float32, composed from what the suite already holds and nothing
restated: a step's collision is golden/np_sim.particle_collision itself, run with a cast in np_sim.cast_ray's place that knows every
kind -- capsule_ref.cast_ray_identity, which casts each collider and instance ALONE (np_sim for kinds 0-4, capsule_ref for capsules,
mesh_ref.cast_instance for meshes) and keeps the strictly nearer: the tie rule, and WHO was hit -- the velocity step is the expression
of np_sim.Spawner.update, and the triangle of a mesh hit is found the way tests/test_gpu_ray_query.py finds it: the lowest original
index that, evaluated alone by the header's Moeller-Trumbore, gives the reported distance.

The contacts are taken from the reference while it runs: the cast put in np_sim.cast_ray's place notes every hit it returns to an
ACTIVE particle.  Which particles are active in a sub-step, and their velocity, are particle_collision's own locals (`act`, `vel`),
read from its frame -- not recomputed here (asserted present, by name and shape, at every cast).  np_sim.cast_ray is replaced for
the duration of trace_paths only and restored in a `finally`; the suite runs its tests one at a time in one thread, so nobody else
calls np_sim in between -- and a call that did would meet the assert on the caller.  A helper, not a test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import capsule_ref  # noqa: E402
import mesh_ref  # noqa: E402
from mesh_ref import np_sim  # noqa: E402

from bevy_firework_amd import settings as S  # noqa: E402

f32 = np.float32
NONE = 0xFFFFFFFF


def world_of(colliders, instances=()):
    """what trace_paths takes as its world: settings.Collider of any kind and mesh_ref.Instance"""
    return mesh_ref.World(list(colliders), list(instances))


def _triangle(inst, o, d, md, t):
    """ORIGINAL index of the triangle of `inst` the rays o + t d hit: the lowest that alone gives the distance t, bit for bit"""
    q = np.asarray(inst.rotation, dtype=f32)
    ol = (o - np.asarray(inst.position, dtype=f32)).astype(f32)
    dl = d
    if not (q[0] == 0 and q[1] == 0 and q[2] == 0 and q[3] == 1):
        qi = np.broadcast_to(np.array([-q[0], -q[1], -q[2], q[3]], dtype=f32), (len(o), 4))
        ol, dl = np_sim.quat_mul_vec3(qi, ol), np_sim.quat_mul_vec3(qi, d)
    m = inst.mesh
    T = len(m.v0)
    dot3, cross3 = mesh_ref.dot3, mesh_ref.cross3
    with np.errstate(all="ignore"):
        O, D = np.broadcast_to(ol[:, None, :], (len(o), T, 3)), np.broadcast_to(dl[:, None, :], (len(o), T, 3))
        E1, E2 = np.broadcast_to(m.e1[None], O.shape), np.broadcast_to(m.e2[None], O.shape)
        p = cross3(D, E2)
        det = dot3(E1, p)
        inv = (f32(1.0) / det).astype(f32)
        s = (O - m.v0[None]).astype(f32)
        u = (dot3(s, p) * inv).astype(f32)
        qv = cross3(s, E1)
        v = (dot3(D, qv) * inv).astype(f32)
        tt = (dot3(E2, qv) * inv).astype(f32)
        mg = np.fmin((((mesh_ref.WT_K * mesh_ref.abs1(s)).astype(f32) * m.ee[None]).astype(f32) * np.abs(inv)).astype(f32), mesh_ref.WT_CAP)  # WATERTIGHT
        ok = ((det != 0) & (u >= -mg) & (v >= -mg) & ((u + v).astype(f32) <= (f32(1.0) + mg).astype(f32)) & (tt >= 0) & (tt <= md[:, None])
              & (tt == t[:, None]))
    assert ok.any(axis=1).all(), "a mesh hit no triangle reproduces"
    return m.orig[np.argmax(ok, axis=1)].astype(np.uint32)


class _Contacts:
    """np_sim.cast_ray's stand-in for one trace: casts with identity and notes what particle_collision's active particles hit"""

    def __init__(self, n):
        self.point, self.normal = np.zeros((n, 3), dtype=f32), np.zeros((n, 3), dtype=f32)
        self.step = np.full(n, NONE, dtype=np.uint32)
        self.kind = np.zeros(n, dtype=np.int32)
        self.index, self.triangle = np.full(n, NONE, dtype=np.uint32), np.full(n, NONE, dtype=np.uint32)
        self.count = np.zeros(n, dtype=np.uint32)
        self.now, self.who = 0, None  # the step under way; which paths the particles of this call are

    def __call__(self, world, mask, origin, d, max_distance):
        caller = sys._getframe(1)
        assert caller.f_code is np_sim.particle_collision.__code__, "the recording cast is for np_sim.particle_collision's casts only"
        missing = [k for k in ("act", "vel") if k not in caller.f_locals]
        assert not missing, f"np_sim.particle_collision no longer holds its active mask / velocity in locals named {missing}: trace_ref reads them"
        act, vel = caller.f_locals["act"], caller.f_locals["vel"]
        assert act.shape == (len(origin),) and act.dtype == bool and vel.shape == origin.shape, "np_sim.particle_collision's `act` / `vel` changed their meaning"
        md = np.broadcast_to(np.asarray(max_distance, dtype=f32), (len(origin),))
        found, t, nrm, kind, index = capsule_ref.cast_ray_identity(world, mask, origin, d, md)
        hit = np.flatnonzero(act & found)
        w = self.who[hit]
        first = self.count[w] == 0
        hf, wf = hit[first], w[first]
        if len(hf):
            with np.errstate(all="ignore"):
                # distance > 0: after pos += normalize_or_zero(vel) * distance (np_sim.particle_collision's pos_r before the nudge);
                # distance == 0: the position before the push-out
                moved = (origin[hf] + (np_sim.normalize_or_zero(vel[hf]) * t[hf][:, None]).astype(f32)).astype(f32)
            self.point[wf] = np.where((t[hf] == 0)[:, None], origin[hf], moved)
            self.normal[wf], self.step[wf], self.kind[wf], self.index[wf] = nrm[hf], self.now, kind[hf], index[hf].astype(np.uint32)
            for i, inst in enumerate(world.instances):
                sel = (kind[hf] == S.HIT_MESH) & (index[hf] == i)
                if sel.any():
                    self.triangle[wf[sel]] = _triangle(inst, origin[hf][sel], d[hf][sel], md[hf][sel], t[hf][sel])
        self.count[w] += 1
        return found, t, nrm


def trace_paths(world, settings, paths, samples=False):
    """fw_ctx_trace_paths over world_of(...): settings a settings.PathSettings, paths settings.PATH_DTYPE records ->
    settings.PATH_RESULT_DTYPE records (and samples[n_steps, n, 4])"""
    paths = np.asarray(paths, dtype=S.PATH_DTYPE)
    n, dt, cs = len(paths), f32(settings.dt), settings.collision_settings
    pos, vel = paths["position"].astype(f32).copy(), paths["velocity"].astype(f32).copy()
    age, life = paths["age"].astype(f32).copy(), paths["lifetime"].astype(f32)
    status, steps = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    c = _Contacts(n)
    smp = np.zeros((int(settings.n_steps), n, 4), dtype=f32)
    acc, drag = np.asarray(settings.acceleration, dtype=f32), f32(settings.linear_drag)
    held, np_sim.cast_ray = np_sim.cast_ray, c
    try:
        with np.errstate(all="ignore"):
            for k in range(int(settings.n_steps)):
                run = np.flatnonzero(status == S.PATH_RUNNING)
                age[run] = (age[run] + dt).astype(f32)
                dead = age[run] >= life[run]
                status[run[dead]] = S.PATH_EXPIRED
                run = run[~dead]
                if cs is not None:
                    c.now, c.who = k, run
                    pos[run], vel[run], kill = np_sim.particle_collision(pos[run], vel[run], dt, cs, world)
                    status[run[kill]] = S.PATH_DESTROYED
                    run = run[~kill]
                else:
                    pos[run] = (pos[run] + (vel[run] * dt).astype(f32)).astype(f32)
                v = vel[run]
                vel[run] = (v + ((acc - (v * drag).astype(f32)).astype(f32) * dt).astype(f32)).astype(f32)  # np_sim.Spawner.update
                steps[run] += 1
                smp[k, :, :3], smp[k, :, 3] = pos, age
    finally:
        np_sim.cast_ray = held
    out = np.zeros(n, dtype=S.PATH_RESULT_DTYPE)
    out["position"], out["age"], out["velocity"], out["steps"], out["status"] = pos, age, vel, steps, status
    out["contact_point"], out["contact_step"], out["contact_normal"] = c.point, c.step, c.normal
    out["kind"], out["index"], out["triangle"], out["n_contacts"] = c.kind, c.index, c.triangle, c.count
    return (out, smp) if samples else out
