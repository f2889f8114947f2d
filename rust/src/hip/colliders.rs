//! The world `particle_collision` casts its rays into (core.rs:744-800), mirrored into the backend's device-resident set of
//! analytic colliders and triangle meshes (UNVERIFIED SOURCE: no Rust toolchain in the build image).
//!
//! The reference asks avian's `SpatialQuery` (arbitrary parry shapes behind a CPU broadphase, core.rs:756-765).  The backend
//! keeps planes, spheres, oriented boxes, cylinders, cones and capsules on the GPU (`fw_collider`), and triangle meshes placed by
//! instances (`fw_mesh_collider`; ray-cast semantics of both in `include/firework_hip.h`).  Entities opt in with the
//! `ParticleCollider` marker; both sets are replaced EVERY frame -- the calls do not wait for the frames in flight, a new set
//! travels as one small copy in the context's stream -- so moving bodies cost what the reference's per-frame query costs.
//! `Collider::trimesh*`, heightfields and convex polyhedra become meshes: their triangles, scaled by the collider's scale, are
//! uploaded once per (entity, scale) and freed when the entity (or its collider) goes away.  A capsule is the sixth analytic kind
//! (`FW_COLLIDER_CAPSULE`, mapped from the segment's endpoints and radius); a compound shape is flattened -- each child's isometry
//! composed with the body's, each child pushed as its own `fw_collider` or mesh instance, and the entity repeated in the parallel
//! `Vec<Entity>`s (`ColliderEntities`) so that `fw_ray_hit.index` still finds it.
use super::ffi::*;
use super::HipBackend;
use avian3d::prelude::*;
use bevy::prelude::*;
use std::collections::HashMap;

/// "particles bounce off this collider"
#[derive(Component, Default)]
pub struct ParticleCollider;

/// `SpatialQueryFilter::excluded_entities` (core.rs:247, 764) has no counterpart on the device (include/firework_hip.h): entities
/// listed here are sent with NO membership bit, so no particle type's mask selects them -- the one exclusion the backend can honour,
/// and it holds for every particle type of the context.  A filter that excludes an entity for ONE type only keeps that spawner on
/// the CPU systems.
#[derive(Resource, Default)]
pub struct ParticleColliderExclusions(pub bevy::platform::collections::HashSet<Entity>);

/// The device meshes of the mesh-shaped colliders, by entity: the scale they were baked with and the handle
/// (`fw_ctx_create_mesh`).  A system-local: the cache lives and dies with `hip_sync_colliders`.
#[derive(Default)]
pub struct MeshCache(HashMap<Entity, ([u32; 3], fw_mesh)>);

/// The triangles of a mesh-shaped collider in its own frame (unscaled), or None for every other shape.
fn mesh_triangles(shape: &SharedShape) -> Option<(Vec<[f32; 3]>, Vec<[u32; 3]>)> {
    let pts = |v: &[avian3d::parry::math::Point<f32>]| v.iter().map(|p| [p.x, p.y, p.z]).collect::<Vec<_>>();
    if let Some(m) = shape.as_trimesh() {
        Some((pts(m.vertices()), m.indices().to_vec()))                                  // Collider::trimesh*
    } else if let Some(h) = shape.as_heightfield() {
        let (v, i) = h.to_trimesh();                                                     // Collider::heightfield
        Some((pts(&v), i))
    } else if let Some(c) = shape.as_convex_polyhedron() {
        let (v, i) = c.to_trimesh();                                                     // Collider::convex_hull / convex_decomposition pieces
        Some((pts(&v), i))
    } else {
        None
    }
}

/// The entities behind the two sets as last sent, in the sets' order: `fw_ray_hit.index` counts in `analytic` (FW_HIT_COLLIDER)
/// or in `meshes` (FW_HIT_MESH).  A compound's entity appears once per child.
#[derive(Resource, Default)]
pub struct ColliderEntities { pub analytic: Vec<Entity>, pub meshes: Vec<Entity> }

/// One analytic primitive placed by `iso` (parry isometry, in the body's frame) under the body's transform `t`; None for a shape
/// with no analytic counterpart.
fn analytic_collider(shape: &dyn avian3d::parry::shape::Shape, t: &Transform, iso: Option<&avian3d::parry::math::Isometry<f32>>, layers: u32) -> Option<fw_collider> {
    // the child's isometry composed with the body's: position = T + R * child.translation, rotation = R * child.rotation
    let (cp, cr) = iso.map_or((Vec3::ZERO, Quat::IDENTITY), |i| {
        (Vec3::new(i.translation.x, i.translation.y, i.translation.z), Quat::from_xyzw(i.rotation.i, i.rotation.j, i.rotation.k, i.rotation.w))
    });
    let (pos, rot) = (t.translation + t.rotation * cp, t.rotation * cr);
    let base = fw_collider {
        kind: 0, layers, position: pos.to_array(), rotation: rot.to_array(), normal: [0., 1., 0.], radius: 0., half_extents: [0.; 3],
    };
    if let Some(b) = shape.as_ball() {
        Some(fw_collider { kind: FW_COLLIDER_SPHERE, radius: b.radius, ..base })                                    // Collider::sphere
    } else if let Some(c) = shape.as_cuboid() {
        Some(fw_collider { kind: FW_COLLIDER_BOX, half_extents: [c.half_extents.x, c.half_extents.y, c.half_extents.z], ..base }) // ::cuboid
    } else if let Some(c) = shape.as_cylinder() {
        Some(fw_collider { kind: FW_COLLIDER_CYLINDER, radius: c.radius, half_extents: [0., c.half_height, 0.], ..base })   // ::cylinder (textures.rs:195)
    } else if let Some(c) = shape.as_cone() {
        Some(fw_collider { kind: FW_COLLIDER_CONE, radius: c.radius, half_extents: [0., c.half_height, 0.], ..base })       // ::cone (textures.rs:211)
    } else if let Some(c) = shape.as_capsule() {
        // ::capsule / ::capsule_endpoints: parry keeps the SEGMENT (a, b) and the radius, in any direction of the shape's frame:
        // position = the midpoint, rotation = the arc from +Y to b - a (the identity for a ball-like capsule, a == b), each under (pos, rot)
        let (a, b) = (Vec3::new(c.segment.a.x, c.segment.a.y, c.segment.a.z), Vec3::new(c.segment.b.x, c.segment.b.y, c.segment.b.z));
        let d = b - a;
        let arc = if d.length() > 0. { Quat::from_rotation_arc(Vec3::Y, d / d.length()) } else { Quat::IDENTITY };
        Some(fw_collider {
            kind: FW_COLLIDER_CAPSULE, radius: c.radius, half_extents: [0., 0.5 * d.length(), 0.],
            position: (pos + rot * ((a + b) * 0.5)).to_array(), rotation: (rot * arc).to_array(), ..base
        })
    } else if let Some(h) = shape.as_halfspace() {
        let n = rot * Vec3::new(h.normal.x, h.normal.y, h.normal.z);
        Some(fw_collider { kind: FW_COLLIDER_PLANE, normal: n.to_array(), ..base })                                  // ::half_space
    } else {
        None
    }
}

pub fn hip_sync_colliders(
    backend: NonSend<HipBackend>, excluded: Option<Res<ParticleColliderExclusions>>, mut meshes: Local<MeshCache>,
    mut entities: ResMut<ColliderEntities>,
    q: Query<(Entity, Ref<Collider>, &GlobalTransform, Option<&CollisionLayers>), With<ParticleCollider>>,
) {
    let mut set = Vec::<fw_collider>::new();
    let mut insts = Vec::<fw_mesh_collider>::new();
    let mut stale = Vec::<fw_mesh>::new(); // meshes the new instance set no longer places: freed once it is in
    let mut seen = Vec::<Entity>::new();
    entities.analytic.clear();
    entities.meshes.clear();
    for (entity, collider, gt, layers) in &q {
        let t = gt.compute_transform();
        let out = excluded.as_ref().is_some_and(|x| x.0.contains(&entity));
        let layers = if out { 0 } else { layers.map_or(1, |l| l.memberships.0) };
        // a mesh-shaped collider: its triangles with the collider's scale baked in (instances carry no scale), cached
        let scale = collider.scale();
        let key = [scale.x.to_bits(), scale.y.to_bits(), scale.z.to_bits()];
        // (a trimesh whose vertices change every frame -- `collider.is_changed()` with the same topology -- would be forwarded to
        // `fw_ctx_update_mesh_vertices` of a mesh made by `fw_ctx_create_deformable_mesh` here instead of being created anew;
        // vertices that a GPU pass of the host has written, e.g. skinning output in a wgpu buffer shared with HIP, go through
        // `fw_ctx_update_mesh_vertices_device` once that pass is ordered in front of `fw_ctx_stream`, and what the device decided
        // about them -- a non-finite vertex rejects the update there -- is read back with `fw_ctx_mesh_update_status`)
        let cached = meshes.0.get(&entity).copied().filter(|(k, _)| *k == key && !collider.is_changed());
        let mesh = match cached {
            Some((_, m)) => Some(m),
            None => mesh_triangles(collider.shape()).and_then(|(v, i)| {
                let xyz: Vec<f32> = v.iter().flat_map(|p| [p[0] * scale.x, p[1] * scale.y, p[2] * scale.z]).collect();
                let idx: Vec<u32> = i.iter().flatten().copied().collect();
                let mut m: fw_mesh = -1;
                let st = unsafe { fw_ctx_create_mesh(backend.ctx, xyz.as_ptr(), v.len() as u32, idx.as_ptr(), i.len() as u32, &mut m) };
                if backend.check(st).is_err() { return None; } // (FW_EINVAL: no triangle of non-zero area -- nothing to collide with)
                if let Some((_, old)) = meshes.0.insert(entity, (key, m)) { stale.push(old); }
                Some(m)
            }),
        };
        if let Some(m) = mesh {
            seen.push(entity);
            insts.push(fw_mesh_collider { mesh: m, layers, position: t.translation.to_array(), rotation: t.rotation.to_array() });
            entities.meshes.push(entity);
            continue;
        }
        let shape = collider.shape_scaled();
        if let Some(compound) = shape.as_compound() {
            // Collider::compound: a list of placed primitives -- flattened, the entity once per child.  (A mesh-shaped child would be
            // created and cached like a mesh-shaped collider, keyed by (entity, child index), and pushed to `insts` under the composed
            // isometry; children with no counterpart are left out like such colliders.)
            for (iso, child) in compound.shapes() {
                if let Some(c) = analytic_collider(child.as_ref(), &t, Some(iso), layers) {
                    set.push(c);
                    entities.analytic.push(entity);
                }
            }
        } else if let Some(c) = analytic_collider(shape.as_ref(), &t, None, layers) {
            set.push(c);
            entities.analytic.push(entity);
        }
    }
    // entities that left the query (despawned, marker or collider removed, or no longer mesh-shaped): their meshes go too
    meshes.0.retain(|e, (_, m)| { let keep = seen.contains(e); if !keep { stale.push(*m); } keep });
    unsafe {
        let _ = backend.check(fw_ctx_set_colliders(backend.ctx, set.as_ptr(), set.len() as u32));
        let _ = backend.check(fw_ctx_set_mesh_colliders(backend.ctx, insts.as_ptr(), insts.len() as u32));
        // (fw_ctx_destroy_mesh refuses a mesh the current set places and waits for the frames in flight: only after the new
        // set, and only when a mesh-shaped collider went away or changed)
        for m in stale { let _ = backend.check(fw_ctx_destroy_mesh(backend.ctx, m)); }
    }
}
