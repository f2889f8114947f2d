//! `extern "C"` binding of `libfirework_hip.so` -- one item per entry point of `include/firework_hip.h` (ABI version 5).
//!
//! UNVERIFIED SOURCE: the image this backend was built in has no Rust toolchain.  `tests/test_abi_cpu.py` checks that the
//! functions declared here are exactly the ones the header declares and the library exports; the struct layouts follow the
//! `#[repr(C)]` mirrors the Python / C++ hosts are tested with (`bevy_firework_amd/_ffi.py`, `include/firework.hpp`).
//! The same text is section 2 of INTEGRATION.md.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct fw_ctx { _private: [u8; 0] }
pub type fw_spawner = i32;

#[repr(C)] #[derive(Clone, Copy)] pub struct fw_rand_f32 { pub min: f32, pub max: f32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_rand_vec3 { pub magnitude: fw_rand_f32, pub direction: [f32; 3], pub spread: f32 }
#[repr(C)] pub struct fw_curve    { pub kind: i32, pub n: i32, pub times: *const f32, pub values: *const f32 }
#[repr(C)] pub struct fw_gradient { pub kind: i32, pub n: i32, pub times: *const f32, pub rgba: *const f32 }

#[repr(C)] pub struct fw_particle_settings {          // ParticleSettings, core.rs:99-142
    pub lifetime: fw_rand_f32, pub scale_curve: fw_curve, pub initial_scale: fw_rand_f32,
    pub acceleration: [f32; 3], pub angular_acceleration: [f32; 3], pub linear_drag: f32, pub angular_drag: f32,
    pub base_color: fw_gradient, pub emissive_color: fw_gradient,
    pub pbr: i32, pub report_destroyed: i32, pub capacity: u32,
    pub collision: fw_collision_settings,             // collision_settings: Option<..>, core.rs:137-138
}
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct fw_collision_settings {   // ParticleCollisionSettings, core.rs:240-248
    pub enabled: i32, pub restitution: f32, pub friction: f32, pub destroy_on_collision: i32, pub filter_mask: u32,
}
pub const FW_COLLIDER_PLANE: i32 = 0; pub const FW_COLLIDER_SPHERE: i32 = 1; pub const FW_COLLIDER_BOX: i32 = 2;
pub const FW_COLLIDER_CYLINDER: i32 = 3; pub const FW_COLLIDER_CONE: i32 = 4;
pub const FW_COLLIDER_CAPSULE: i32 = 5;   // half_extents[1] = half the SEGMENT (parry's half_height), radius = radius; axis = local Y
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_collider {   // one analytic collider of the device-resident world
    pub kind: i32, pub layers: u32, pub position: [f32; 3], pub rotation: [f32; 4], pub normal: [f32; 3],
    pub radius: f32, pub half_extents: [f32; 3],
}
pub type fw_mesh = i32;
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_mesh_collider {   // one placed instance of a collider mesh
    pub mesh: fw_mesh, pub layers: u32, pub position: [f32; 3], pub rotation: [f32; 4],
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_ray {             // one ray of fw_ctx_cast_rays (32 bytes)
    pub origin: [f32; 3], pub max_distance: f32, pub dir: [f32; 3], pub filter_mask: u32,
}
pub const FW_HIT_NONE: i32 = 0; pub const FW_HIT_COLLIDER: i32 = 1; pub const FW_HIT_MESH: i32 = 2;
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_ray_hit {         // its nearest hit (32 bytes); index: position in the set sent
    pub distance: f32, pub normal: [f32; 3], pub kind: i32, pub index: u32, pub triangle: u32, pub reserved: u32,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_point {           // one point of fw_ctx_project_points (16 bytes)
    pub position: [f32; 3], pub filter_mask: u32,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_point_projection { // the nearest point of the world to it (32 bytes); kind / index / triangle as fw_ray_hit
    pub point: [f32; 3], pub distance: f32, pub kind: i32, pub index: u32, pub triangle: u32, pub is_inside: u32,
}
pub const FW_PATH_RUNNING: u32 = 0; pub const FW_PATH_EXPIRED: u32 = 1; pub const FW_PATH_DESTROYED: u32 = 2;
pub const FW_PATH_MAX_STEPS: u32 = 4096;
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_path_settings {   // what a batch of fw_ctx_trace_paths shares; collision.enabled = 0: no casts
    pub dt: f32, pub n_steps: u32, pub acceleration: [f32; 3], pub linear_drag: f32, pub collision: fw_collision_settings,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_path {            // one hypothetical particle (32 bytes)
    pub position: [f32; 3], pub age: f32, pub velocity: [f32; 3], pub lifetime: f32,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_path_result {     // where it ended, its first contact (80 bytes); kind / index / triangle as fw_ray_hit
    pub position: [f32; 3], pub age: f32, pub velocity: [f32; 3], pub steps: u32,
    pub contact_point: [f32; 3], pub contact_step: u32, pub contact_normal: [f32; 3], pub status: u32,
    pub kind: i32, pub index: u32, pub triangle: u32, pub n_contacts: u32,
}
#[repr(C)] pub struct fw_emission_settings {          // EmissionSettings, core.rs:144-162
    pub particle_index: i32, pub pacing_kind: i32, pub oneshot_count: u64,
    pub count: f32, pub duration: f32, pub offset_start: f32, pub offset_end: f32,
    pub mode: i32, pub target_particle_type: i32,
    pub shape_kind: i32, pub shape_radius: f32, pub shape_normal: [f32; 3],
    pub initial_velocity: fw_rand_vec3, pub initial_velocity_radial: fw_rand_f32,
    pub inherit_parent_velocity: i32, pub initial_rotation: [f32; 4], pub initial_angular_velocity: fw_rand_vec3,
}
#[repr(C)] pub struct fw_spawner_desc {               // ParticleSpawner, core.rs:178-185
    pub particle_settings: *const fw_particle_settings, pub n_particle_settings: u32,
    pub emission_settings: *const fw_emission_settings, pub n_emission_settings: u32,
    pub starts_enabled: i32, pub uid: u32,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_particle {   // ParticleData, core.rs:305-321
    pub position: [f32; 3], pub velocity: [f32; 3], pub rotation: [f32; 4], pub angular_velocity: [f32; 3],
    pub initial_scale: f32, pub scale: f32, pub age: f32, pub lifetime: f32,
    pub base_color: [f32; 4], pub emissive_color: [f32; 4], pub pbr: i32,
}
#[repr(C)] #[derive(Clone, Copy, bytemuck::Pod, bytemuck::Zeroable)]
pub struct fw_particle_instance {                      // == render::ParticleInstance, render.rs:95-103
    pub position: [f32; 3], pub scale: f32, pub rotation: [f32; 4], pub base_color: [f32; 4], pub emissive_color: [f32; 4],
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_sort_view {       // the camera of a depth sort (32 bytes); order: FW_SORT_*, reserved: 0
    pub eye: [f32; 3], pub order: u32, pub forward: [f32; 3], pub reserved: u32,
}
#[repr(C)] #[derive(Clone, Copy, Default)] pub struct fw_aabb {     // one box of fw_ctx_aabbs[_device] (32 bytes); any: 0 = no particle, reserved: written as 0
    pub min: [f32; 3], pub any: i32, pub max: [f32; 3], pub reserved: u32,
}
#[repr(C)] #[derive(Clone, Copy)] pub struct fw_volume_place {     // one place of fw_ctx_count_in_volumes[_device] (8 bytes); r#type: -1 = every particle type of the spawner
    pub spawner: fw_spawner, pub r#type: i32,
}
pub const FW_VOLUME_MAX_ANSWERS: u64 = 0x3FF_FFFF;     // the most answers (n_places * n_volumes) of one volume query
pub const FW_SORT_BACK_TO_FRONT: u32 = 0;
pub const FW_SORT_FRONT_TO_BACK: u32 = 1;

extern "C" {
    pub fn fw_abi_version() -> c_int;
    pub fn fw_ctx_create(device: c_int, seed: u32, stream: *mut c_void, out: *mut *mut fw_ctx) -> c_int;
    pub fn fw_ctx_destroy(ctx: *mut fw_ctx) -> c_int;
    pub fn fw_last_error(ctx: *const fw_ctx) -> *const c_char;
    pub fn fw_ctx_stream(ctx: *const fw_ctx) -> *mut c_void;
    pub fn fw_ctx_synchronize(ctx: *mut fw_ctx) -> c_int;
    pub fn fw_ctx_set_colliders(ctx: *mut fw_ctx, colliders: *const fw_collider, n: u32) -> c_int;
    pub fn fw_ctx_create_mesh(ctx: *mut fw_ctx, xyz: *const f32, n_vertices: u32, indices: *const u32, n_triangles: u32, out: *mut fw_mesh) -> c_int;
    pub fn fw_ctx_create_deformable_mesh(ctx: *mut fw_ctx, xyz: *const f32, n_vertices: u32, indices: *const u32, n_triangles: u32, out: *mut fw_mesh) -> c_int;
    pub fn fw_ctx_update_mesh_vertices(ctx: *mut fw_ctx, mesh: fw_mesh, xyz: *const f32, n_vertices: u32) -> c_int;
    pub fn fw_ctx_update_mesh_vertices_device(ctx: *mut fw_ctx, mesh: fw_mesh, d_xyz: *const c_void, n_vertices: u32) -> c_int;
    pub fn fw_ctx_mesh_update_status(ctx: *mut fw_ctx, mesh: fw_mesh, n_applied: *mut u64, n_rejected: *mut u64, first_bad_vertex: *mut i64) -> c_int;
    pub fn fw_ctx_destroy_mesh(ctx: *mut fw_ctx, mesh: fw_mesh) -> c_int;
    pub fn fw_ctx_set_mesh_colliders(ctx: *mut fw_ctx, instances: *const fw_mesh_collider, n: u32) -> c_int;
    pub fn fw_ctx_cast_rays(ctx: *mut fw_ctx, rays: *const fw_ray, n: u64, hits: *mut fw_ray_hit) -> c_int;
    pub fn fw_ctx_cast_rays_device(ctx: *mut fw_ctx, d_rays: *const c_void, n: u64, d_hits: *mut c_void) -> c_int;
    pub fn fw_ctx_project_points(ctx: *mut fw_ctx, points: *const fw_point, n: u64, out: *mut fw_point_projection) -> c_int;
    pub fn fw_ctx_project_points_device(ctx: *mut fw_ctx, d_points: *const c_void, n: u64, d_out: *mut c_void) -> c_int;
    pub fn fw_ctx_trace_paths(ctx: *mut fw_ctx, settings: *const fw_path_settings, paths: *const fw_path, n: u64, out: *mut fw_path_result, samples: *mut f32) -> c_int;
    pub fn fw_ctx_trace_paths_device(ctx: *mut fw_ctx, settings: *const fw_path_settings, d_paths: *const c_void, n: u64, d_out: *mut c_void, d_samples: *mut c_void) -> c_int;
    pub fn fw_spawner_create(ctx: *mut fw_ctx, desc: *const fw_spawner_desc, out: *mut fw_spawner) -> c_int;
    pub fn fw_spawner_update_settings(ctx: *mut fw_ctx, h: fw_spawner, desc: *const fw_spawner_desc) -> c_int;
    pub fn fw_spawner_destroy(ctx: *mut fw_ctx, h: fw_spawner) -> c_int;
    pub fn fw_spawner_set_origin(ctx: *mut fw_ctx, h: fw_spawner, t: *const f32, r_xyzw: *const f32) -> c_int;
    pub fn fw_ctx_set_origins(ctx: *mut fw_ctx, n: u32, handles: *const fw_spawner, translations: *const f32, rotations_xyzw: *const f32) -> c_int;
    pub fn fw_spawner_set_parent_velocity(ctx: *mut fw_ctx, h: fw_spawner, v: *const f32) -> c_int;
    pub fn fw_spawner_set_modifier(ctx: *mut fw_ctx, h: fw_spawner, scale: f32, speed: f32) -> c_int;
    pub fn fw_spawner_queue(ctx: *mut fw_ctx, h: fw_spawner, count: u64) -> c_int;
    pub fn fw_ctx_set_parent_velocities(ctx: *mut fw_ctx, n: u32, handles: *const fw_spawner, velocities: *const f32) -> c_int;
    pub fn fw_ctx_set_modifiers(ctx: *mut fw_ctx, n: u32, handles: *const fw_spawner, scales: *const f32, speeds: *const f32) -> c_int;
    pub fn fw_ctx_queue(ctx: *mut fw_ctx, n: u32, handles: *const fw_spawner, counts: *const u64) -> c_int;
    pub fn fw_step(ctx: *mut fw_ctx, dt: f32) -> c_int;
    pub fn fw_spawner_counts(ctx: *mut fw_ctx, h: fw_spawner, per_type: *mut u32, n_types: u32) -> c_int;
    pub fn fw_spawner_active(ctx: *mut fw_ctx, h: fw_spawner, out: *mut i32) -> c_int;
    pub fn fw_spawner_poll_finished(ctx: *mut fw_ctx, h: fw_spawner, out: *mut i32) -> c_int;
    pub fn fw_spawner_read_particles(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, out: *mut fw_particle, cap: u64, n: *mut u64) -> c_int;
    pub fn fw_spawner_read_last_emitted(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, emission: u32, out: *mut f32, cap: u64, n: *mut u64) -> c_int;
    pub fn fw_spawner_write_particles(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, input: *const fw_particle, n: u64) -> c_int;
    pub fn fw_spawner_write_last_emitted(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, emission: u32, input: *const f32, n: u64) -> c_int;
    pub fn fw_spawner_read_destroyed(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, out: *mut fw_particle, cap: u64, n: *mut u64) -> c_int;
    pub fn fw_spawner_pack_instances(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, out: *mut fw_particle_instance, cap: u64, n: *mut u64) -> c_int;
    pub fn fw_spawner_pack_instances_device(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, d_out: *mut c_void, cap: u64, n_ub: *mut u64) -> c_int;
    pub fn fw_spawner_attach_instances(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, d_out: *mut c_void, cap: u64) -> c_int;
    pub fn fw_spawner_attach_instances_window(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, d_out: *mut c_void, cap: u64) -> c_int;
    pub fn fw_spawner_instance_window(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, first: *mut u64, count: *mut u64) -> c_int;
    pub fn fw_ctx_depth_order_device(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, view: *const fw_sort_view, d_order: *mut c_void, cap: u64, n_ub: *mut u64) -> c_int;
    pub fn fw_ctx_pack_instances_sorted_device(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, view: *const fw_sort_view, d_out: *mut c_void, cap: u64, n_ub: *mut u64) -> c_int;
    pub fn fw_ctx_pack_instances_sorted(ctx: *mut fw_ctx, h: fw_spawner, ty: u32, view: *const fw_sort_view, out: *mut fw_particle_instance, cap: u64, n: *mut u64) -> c_int;
    pub fn fw_spawner_aabb(ctx: *mut fw_ctx, h: fw_spawner, min: *mut f32, max: *mut f32, any: *mut i32) -> c_int;
    pub fn fw_ctx_track_aabbs(ctx: *mut fw_ctx, enable: i32) -> c_int;
    pub fn fw_ctx_aabbs(ctx: *mut fw_ctx, n: u32, handles: *const fw_spawner, out: *mut fw_aabb) -> c_int;
    pub fn fw_ctx_aabbs_device(ctx: *mut fw_ctx, n: u32, handles: *const fw_spawner, d_out: *mut c_void) -> c_int;
    pub fn fw_ctx_count_in_volumes(ctx: *mut fw_ctx, n_places: u32, places: *const fw_volume_place, n_volumes: u32, volumes: *const fw_collider, out: *mut u32) -> c_int;
    pub fn fw_ctx_count_in_volumes_device(ctx: *mut fw_ctx, n_places: u32, places: *const fw_volume_place, n_volumes: u32, volumes: *const fw_collider, d_out: *mut c_void) -> c_int;
    pub fn fw_ctx_live_count(ctx: *mut fw_ctx, out: *mut u64) -> c_int;
    pub fn fw_ctx_live_count_device(ctx: *mut fw_ctx, d_out_u64: *mut c_void) -> c_int;
    pub fn fw_ctx_live_count_ring(ctx: *mut fw_ctx, d_ring_u64: *mut c_void, n_slots: u32) -> c_int;
    pub fn fw_ctx_last_step_updated(ctx: *mut fw_ctx, out: *mut u64) -> c_int;
    pub fn fw_compute_emission_count(t: f32, last: f32, dur: f32, start: f32, end: f32, per_cycle: f32, next: *mut f32) -> u64;
}
