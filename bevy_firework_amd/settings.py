"""Host-side mirror of the reference's settings types for the particle hot path.

Names, defaults and argument meaning follow the reference so tests read like its
own code (paths relative to /root/reference):

  EmissionPacing / EmissionMode / SpawnTransformMode   src/core.rs:11-73
  ParticleSettings / EmissionSettings / ParticleSpawner src/core.rs:99-238
  EffectModifier                                       src/core.rs:323-336
  FireworkCurve / FireworkGradient                     src/curve.rs:8-75,171-239
  EmissionShape                                        src/emission_shape.rs:6-15
  RandF32 / RandVec3                                   bevy_utilitarian 0.10.0 (not in tree)

These are plain data holders: no simulation arithmetic lives here.  The HIP
backend (``bevy_firework_amd.system``) flattens them into the C ABI of
``include/firework_hip.h``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

Vec3 = Tuple[float, float, float]
Quat = Tuple[float, float, float, float]  # xyzw
Rgba = Tuple[float, float, float, float]


WHITE: Rgba = (1.0, 1.0, 1.0, 1.0)  # LinearRgba::WHITE
BLACK: Rgba = (0.0, 0.0, 0.0, 1.0)  # LinearRgba::BLACK
QUAT_IDENTITY: Quat = (0.0, 0.0, 0.0, 1.0)


@dataclass(frozen=True)
class RandF32:
    min: float
    max: float

    @staticmethod
    def constant(value: float) -> "RandF32":
        return RandF32(value, value)


@dataclass(frozen=True)
class RandVec3:
    magnitude: RandF32
    direction: Vec3
    spread: float

    @staticmethod
    def constant(value: Sequence[float]) -> "RandVec3":
        # bevy_utilitarian: direction = v.normalize_or_zero(), magnitude = |v|, spread = 0 (fp32)
        v = np.asarray(value, dtype=np.float32)
        length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], dtype=np.float32)
        with np.errstate(divide="ignore"):
            rcp = np.float32(1.0) / length
        if np.isfinite(rcp) and rcp > 0:
            d = v * rcp
        else:
            d = np.zeros(3, dtype=np.float32)
        return RandVec3(RandF32.constant(float(length)), (float(d[0]), float(d[1]), float(d[2])), 0.0)


CURVE_CONSTANT, CURVE_EVEN, CURVE_UNEVEN = 0, 1, 2


@dataclass(frozen=True)
class FireworkCurve:
    """FireworkCurve<f32> (curve.rs:8-12); domain [0, 1]."""

    kind: int
    values: Tuple[float, ...]
    times: Tuple[float, ...] = ()

    @staticmethod
    def constant(sample: float) -> "FireworkCurve":
        return FireworkCurve(CURVE_CONSTANT, (float(sample),))

    @staticmethod
    def even_samples(samples: Sequence[float]) -> "FireworkCurve":
        samples = tuple(float(s) for s in samples)
        if len(samples) == 0:
            raise ValueError("Cannot create curve from 0 samples")  # panic! at curve.rs:61
        if len(samples) == 1:
            return FireworkCurve.constant(samples[0])
        return FireworkCurve(CURVE_EVEN, samples)

    @staticmethod
    def uneven_samples(samples: Sequence[Tuple[float, float]]) -> "FireworkCurve":
        samples = list(samples)
        if len(samples) == 0:
            raise ValueError("Cannot create curve from 0 samples")  # panic! at curve.rs:45
        if len(samples) == 1:
            return FireworkCurve.constant(samples[0][1])
        return FireworkCurve(CURVE_UNEVEN, tuple(float(v) for _, v in samples), tuple(float(t) for t, _ in samples))


@dataclass(frozen=True)
class FireworkGradient:
    """FireworkGradient<LinearRgba> (curve.rs:171-175); domain [0, 1]."""

    kind: int
    colors: Tuple[Rgba, ...]
    times: Tuple[float, ...] = ()

    @staticmethod
    def constant(sample: Rgba) -> "FireworkGradient":
        return FireworkGradient(CURVE_CONSTANT, (tuple(float(c) for c in sample),))

    @staticmethod
    def even_samples(samples: Sequence[Rgba]) -> "FireworkGradient":
        samples = tuple(tuple(float(c) for c in s) for s in samples)
        if len(samples) == 0:
            raise ValueError("Cannot create curve from 0 samples")  # panic! at curve.rs:227
        if len(samples) == 1:
            return FireworkGradient.constant(samples[0])
        return FireworkGradient(CURVE_EVEN, samples)

    @staticmethod
    def uneven_samples(samples: Sequence[Tuple[float, Rgba]]) -> "FireworkGradient":
        samples = list(samples)
        if len(samples) == 0:
            raise ValueError("Cannot create curve from 0 samples")  # panic! at curve.rs:211
        if len(samples) == 1:
            return FireworkGradient.constant(samples[0][1])
        return FireworkGradient(
            CURVE_UNEVEN,
            tuple(tuple(float(c) for c in s) for _, s in samples),
            tuple(float(t) for t, _ in samples),
        )


PACING_ONESHOT, PACING_ONDEMAND, PACING_COUNT_OVER_DURATION = 0, 1, 2


@dataclass(frozen=True)
class EmissionPacing:
    """EmissionPacing (core.rs:12-44)."""

    kind: int
    oneshot_count: int = 0
    count: float = 0.0
    duration: float = 1.0
    offset_start: float = 0.0
    offset_end: float = 1.0

    @staticmethod
    def OneShot(count: int) -> "EmissionPacing":
        return EmissionPacing(PACING_ONESHOT, oneshot_count=int(count))

    @staticmethod
    def OnDemand() -> "EmissionPacing":
        return EmissionPacing(PACING_ONDEMAND)

    @staticmethod
    def CountOverDuration(count: float, duration: float, offset_start: float, offset_end: float) -> "EmissionPacing":
        return EmissionPacing(PACING_COUNT_OVER_DURATION, 0, count, duration, offset_start, offset_end)

    @staticmethod
    def rate(rate: float) -> "EmissionPacing":  # core.rs:36-43
        return EmissionPacing.CountOverDuration(rate, 1.0, 0.0, 1.0)

    def is_one_shot(self) -> bool:
        return self.kind == PACING_ONESHOT


MODE_GLOBAL, MODE_NESTED = 0, 1


@dataclass(frozen=True)
class EmissionMode:
    """EmissionMode (core.rs:47-54)."""

    kind: int = MODE_GLOBAL
    target_particle_type: int = 0

    @staticmethod
    def Global() -> "EmissionMode":
        return EmissionMode(MODE_GLOBAL)

    @staticmethod
    def Nested(target_particle_type: int) -> "EmissionMode":
        return EmissionMode(MODE_NESTED, int(target_particle_type))


SHAPE_POINT, SHAPE_SPHERE, SHAPE_CIRCLE = 0, 1, 2


@dataclass(frozen=True)
class EmissionShape:
    """EmissionShape (emission_shape.rs:6-15)."""

    kind: int = SHAPE_POINT
    radius: float = 0.0
    normal: Vec3 = (0.0, 1.0, 0.0)

    @staticmethod
    def Point() -> "EmissionShape":
        return EmissionShape(SHAPE_POINT)

    @staticmethod
    def Sphere(radius: float) -> "EmissionShape":
        return EmissionShape(SHAPE_SPHERE, float(radius))

    @staticmethod
    def Circle(normal: Vec3, radius: float) -> "EmissionShape":
        return EmissionShape(SHAPE_CIRCLE, float(radius), tuple(float(c) for c in normal))


class SpawnTransformMode:
    """SpawnTransformMode (core.rs:66-73)."""

    Global = 0
    Local = 1


@dataclass(frozen=True)
class ParticleCollisionSettings:
    """ParticleCollisionSettings (core.rs:240-248, feature physics_avian).  ``filter_mask`` stands in for the
    SpatialQueryFilter: a collider takes part when ``filter_mask & collider.layers`` is non-zero."""

    restitution: float = 0.0
    friction: float = 0.0
    destroy_on_collision: bool = False
    filter_mask: int = 0xFFFFFFFF


COLLIDER_PLANE, COLLIDER_SPHERE, COLLIDER_BOX, COLLIDER_CYLINDER, COLLIDER_CONE, COLLIDER_CAPSULE = 0, 1, 2, 3, 4, 5


@dataclass(frozen=True)
class Collider:
    """One analytic collider of the world particle_collision casts its rays into (core.rs:744-800).  The reference
    asks avian's SpatialQuery; this backend keeps a device-resident set of planes / spheres / boxes / cylinders / cones /
    capsules instead
    (include/firework_hip.h: fw_collider has the ray-cast semantics)."""

    kind: int
    position: Vec3 = (0.0, 0.0, 0.0)
    rotation: Quat = QUAT_IDENTITY
    normal: Vec3 = (0.0, 1.0, 0.0)
    radius: float = 0.0
    half_extents: Vec3 = (0.0, 0.0, 0.0)
    layers: int = 1

    @staticmethod
    def Plane(point: Vec3, normal: Vec3, layers: int = 1) -> "Collider":
        n = np.asarray(normal, dtype=np.float64)
        n = n / np.linalg.norm(n)
        return Collider(COLLIDER_PLANE, tuple(float(c) for c in point), normal=tuple(float(c) for c in n.astype(np.float32)),
                        layers=layers)

    @staticmethod
    def Sphere(center: Vec3, radius: float, layers: int = 1) -> "Collider":
        return Collider(COLLIDER_SPHERE, tuple(float(c) for c in center), radius=float(radius), layers=layers)

    @staticmethod
    def Box(center: Vec3, half_extents: Vec3, rotation: Quat = QUAT_IDENTITY, layers: int = 1) -> "Collider":
        return Collider(COLLIDER_BOX, tuple(float(c) for c in center), tuple(float(c) for c in rotation),
                        half_extents=tuple(float(c) for c in half_extents), layers=layers)

    @staticmethod
    def Cylinder(center: Vec3, radius: float, height: float, rotation: Quat = QUAT_IDENTITY, layers: int = 1) -> "Collider":
        """avian's Collider::cylinder(radius, height) (examples/textures.rs:195): the axis is the collider's local Y"""
        return Collider(COLLIDER_CYLINDER, tuple(float(c) for c in center), tuple(float(c) for c in rotation), radius=float(radius),
                        half_extents=(0.0, float(height) * 0.5, 0.0), layers=layers)

    @staticmethod
    def Cone(center: Vec3, radius: float, height: float, rotation: Quat = QUAT_IDENTITY, layers: int = 1) -> "Collider":
        """avian's Collider::cone(radius, height) (examples/textures.rs:211): base disc at local y = -height / 2, apex at +height / 2"""
        return Collider(COLLIDER_CONE, tuple(float(c) for c in center), tuple(float(c) for c in rotation), radius=float(radius),
                        half_extents=(0.0, float(height) * 0.5, 0.0), layers=layers)

    @staticmethod
    def Capsule(center: Vec3, radius: float, length: float, rotation: Quat = QUAT_IDENTITY, layers: int = 1) -> "Collider":
        """avian's Collider::capsule(radius, length): every point within ``radius`` of a segment of ``length`` along the collider's
        local Y (half_extents[1] = length / 2: half the SEGMENT, parry's half_height -- not half the total height)"""
        return Collider(COLLIDER_CAPSULE, tuple(float(c) for c in center), tuple(float(c) for c in rotation), radius=float(radius),
                        half_extents=(0.0, float(length) * 0.5, 0.0), layers=layers)

    @staticmethod
    def CapsuleEndpoints(a: Vec3, b: Vec3, radius: float, layers: int = 1) -> "Collider":
        """avian's Collider::capsule_endpoints(radius, a, b): the segment from ``a`` to ``b``.  position = the midpoint, rotation = the
        arc from +Y to b - a (the identity when a == b, half a turn about X when b - a points straight down), in float32 operation by operation as firework::Collider::capsule_endpoints
        does it, so that both mirrors hand the library the same bits"""
        f = np.float32
        a, b = np.asarray(a, dtype=f), np.asarray(b, dtype=f)
        mid = ((a + b).astype(f) * f(0.5)).astype(f)
        d = (b - a).astype(f)
        ln = np.sqrt(f(f(f(d[0] * d[0]) + f(d[1] * d[1])) + f(d[2] * d[2]))).astype(f)
        rot = (0.0, 0.0, 0.0, 1.0)
        if ln > 0:
            u = (d / ln).astype(f)
            # (cross(+Y, u), 1 + dot(+Y, u)), normalised; below the equator 1 + u.y cancels, and (u.x^2 + u.z^2) / (1 - u.y) is
            # the same number without the cancellation; nothing left of it -- b - a along -Y -- is half a turn about X
            s2 = f(f(u[2] * u[2]) + f(u[0] * u[0]))
            w = f(f(1.0) + u[1]) if u[1] >= 0 else f(s2 / f(f(1.0) - u[1]))
            n2 = f(s2 + f(w * w))
            if n2 > 0:
                inv = f(f(1.0) / np.sqrt(n2).astype(f))
                rot = (float(f(u[2] * inv)), 0.0, float(f(f(-u[0]) * inv)), float(f(w * inv)))
            else:
                rot = (1.0, 0.0, 0.0, 0.0)
        else:
            ln = f(0.0)
        return Collider(COLLIDER_CAPSULE, tuple(float(c) for c in mid), rot, radius=float(radius),
                        half_extents=(0.0, float(f(ln * f(0.5))), 0.0), layers=layers)


@dataclass(frozen=True)
class MeshCollider:
    """One placed instance of a triangle mesh of the collider world (avian's Collider::trimesh and the shapes that become
    triangles): ``mesh`` is a handle from ParticleSystem.create_mesh; the mesh's scale is baked into its vertices
    (include/firework_hip.h: fw_mesh_collider has the ray-cast semantics -- a two-sided surface, no inside)."""

    mesh: int
    position: Vec3 = (0.0, 0.0, 0.0)
    rotation: Quat = QUAT_IDENTITY
    layers: int = 1


@dataclass
class ParticleSettings:
    """ParticleSettings (core.rs:99-142); defaults core.rs:187-211.

    Render-only fields (textures, fade_edge, fade_scene, blend_mode) are carried
    for API parity but never reach the simulation.  ``particles_destroyed``
    stands in for ``event_handlers.particles_destroyed`` (core.rs:164-167): a
    callable receiving the destroyed ParticleData records after ``update``.
    """

    lifetime: RandF32 = RandF32.constant(5.0)
    scale_curve: FireworkCurve = FireworkCurve.constant(1.0)
    initial_scale: RandF32 = RandF32.constant(1.0)
    acceleration: Vec3 = (0.0, -9.81, 0.0)
    angular_acceleration: Vec3 = (0.0, 0.0, 0.0)
    linear_drag: float = 0.2
    angular_drag: float = 0.2
    base_color: FireworkGradient = FireworkGradient.constant(WHITE)
    emissive_color: FireworkGradient = FireworkGradient.constant(BLACK)
    fade_edge: float = 0.7
    fade_scene: float = 1.0
    blend_mode: str = "Blend"
    pbr: bool = False
    particles_destroyed: Optional[object] = None
    collision_settings: Optional[ParticleCollisionSettings] = None  # core.rs:137-138
    capacity: int = 0  # backend knob: device slots for this type (0 = derived)


@dataclass
class EmissionSettings:
    """EmissionSettings (core.rs:144-162); defaults core.rs:213-227."""

    particle_index: int = 0
    emission_pacing: EmissionPacing = EmissionPacing.rate(5.0)
    emission_mode: EmissionMode = EmissionMode.Global()
    emission_shape: EmissionShape = EmissionShape.Point()
    initial_velocity: RandVec3 = RandVec3.constant((0.0, 0.0, 0.0))
    initial_velocity_radial: RandF32 = RandF32.constant(0.0)
    inherit_parent_velocity: bool = True
    initial_rotation: Quat = QUAT_IDENTITY
    initial_angular_velocity: RandVec3 = RandVec3.constant((0.0, 0.0, 0.0))


@dataclass
class ParticleSpawner:
    """ParticleSpawner (core.rs:178-185); defaults core.rs:229-238."""

    particle_settings: List[ParticleSettings] = field(default_factory=lambda: [ParticleSettings()])
    emission_settings: List[EmissionSettings] = field(default_factory=lambda: [EmissionSettings()])
    starts_enabled: bool = True
    spawn_transform_mode: int = SpawnTransformMode.Global


@dataclass
class EffectModifier:
    """EffectModifier (core.rs:323-336)."""

    scale: float = 1.0
    speed: float = 1.0


@dataclass
class Transform:
    """The two Transform fields spawn_particles reads (core.rs:432-435, 441, 454)."""

    translation: Vec3 = (0.0, 0.0, 0.0)
    rotation: Quat = QUAT_IDENTITY


# numpy dtype of one ParticleData record as exchanged with the backend and the
# oracle (fw_particle in include/firework_hip.h; core.rs:305-321).
PARTICLE_DTYPE = np.dtype(
    [
        ("position", np.float32, 3),
        ("velocity", np.float32, 3),
        ("rotation", np.float32, 4),
        ("angular_velocity", np.float32, 3),
        ("initial_scale", np.float32),
        ("scale", np.float32),
        ("age", np.float32),
        ("lifetime", np.float32),
        ("base_color", np.float32, 4),
        ("emissive_color", np.float32, 4),
        ("pbr", np.int32),
    ]
)
assert PARTICLE_DTYPE.itemsize == 104

# ParticleInstance (render.rs:95-103)
INSTANCE_DTYPE = np.dtype(
    [
        ("position", np.float32, 3),
        ("scale", np.float32),
        ("rotation", np.float32, 4),
        ("base_color", np.float32, 4),
        ("emissive_color", np.float32, 4),
    ]
)
assert INSTANCE_DTYPE.itemsize == 64

# fw_aabb (include/firework_hip.h: BATCHED BOXES): the record ParticleSystem.aabb_records returns, one per listed spawner
AABB_DTYPE = np.dtype(
    [
        ("min", np.float32, 3),
        ("any", np.int32),
        ("max", np.float32, 3),
        ("reserved", np.uint32),
    ]
)
assert AABB_DTYPE.itemsize == 32

# fw_volume_place (include/firework_hip.h: VOLUME QUERIES): one place of ParticleSystem.count_in_volumes -- a spawner handle and one of
# its particle types, or -1 for all of them
VOLUME_PLACE_DTYPE = np.dtype([("spawner", np.int32), ("type", np.int32)])
assert VOLUME_PLACE_DTYPE.itemsize == 8

# fw_sort_view (include/firework_hip.h: DEPTH-SORTED INSTANCES): the camera SpawnerData.instances_sorted sorts for
SORT_BACK_TO_FRONT, SORT_FRONT_TO_BACK = 0, 1


@dataclass
class SortView:
    """fw_sort_view: depth = (position - eye) . forward in fp32 (forward used as given, not normalised); `order` says which end is drawn
    first (SORT_*; back to front is what an alpha-blended draw wants); reserved must be 0."""

    eye: Vec3 = (0.0, 0.0, 0.0)
    forward: Vec3 = (0.0, 0.0, -1.0)
    order: int = SORT_BACK_TO_FRONT
    reserved: int = 0


# fw_ray / fw_ray_hit (include/firework_hip.h): the records of ParticleSystem.cast_rays
RAY_DTYPE = np.dtype(
    [
        ("origin", np.float32, 3),
        ("max_distance", np.float32),
        ("dir", np.float32, 3),
        ("filter_mask", np.uint32),
    ]
)
assert RAY_DTYPE.itemsize == 32
HIT_NONE, HIT_COLLIDER, HIT_MESH = 0, 1, 2
RAY_HIT_DTYPE = np.dtype(
    [
        ("distance", np.float32),
        ("normal", np.float32, 3),
        ("kind", np.int32),
        ("index", np.uint32),
        ("triangle", np.uint32),
        ("reserved", np.uint32),
    ]
)
assert RAY_HIT_DTYPE.itemsize == 32

# fw_point / fw_point_projection (include/firework_hip.h: POINT QUERIES): the records of ParticleSystem.project_points
POINT_DTYPE = np.dtype(
    [
        ("position", np.float32, 3),
        ("filter_mask", np.uint32),
    ]
)
assert POINT_DTYPE.itemsize == 16
POINT_PROJECTION_DTYPE = np.dtype(
    [
        ("point", np.float32, 3),
        ("distance", np.float32),
        ("kind", np.int32),
        ("index", np.uint32),
        ("triangle", np.uint32),
        ("is_inside", np.uint32),
    ]
)
assert POINT_PROJECTION_DTYPE.itemsize == 32

# fw_path_settings / fw_path / fw_path_result (include/firework_hip.h: PATH QUERIES): the records of ParticleSystem.trace_paths
PATH_RUNNING, PATH_EXPIRED, PATH_DESTROYED = 0, 1, 2
PATH_MAX_STEPS = 4096


@dataclass
class PathSettings:
    """fw_path_settings: what a batch of traced paths shares -- the step, how many of them, and the three settings of a particle type
    a step reads (ParticleSettings.acceleration / linear_drag / collision_settings; None: no casts, position += velocity * dt)."""

    dt: float
    n_steps: int
    acceleration: Vec3 = (0.0, 0.0, 0.0)
    linear_drag: float = 0.0
    collision_settings: Optional[ParticleCollisionSettings] = None


PATH_DTYPE = np.dtype(
    [
        ("position", np.float32, 3),
        ("age", np.float32),
        ("velocity", np.float32, 3),
        ("lifetime", np.float32),
    ]
)
assert PATH_DTYPE.itemsize == 32
PATH_RESULT_DTYPE = np.dtype(
    [
        ("position", np.float32, 3),
        ("age", np.float32),
        ("velocity", np.float32, 3),
        ("steps", np.uint32),
        ("contact_point", np.float32, 3),
        ("contact_step", np.uint32),
        ("contact_normal", np.float32, 3),
        ("status", np.uint32),
        ("kind", np.int32),
        ("index", np.uint32),
        ("triangle", np.uint32),
        ("n_contacts", np.uint32),
    ]
)
assert PATH_RESULT_DTYPE.itemsize == 80
