// fw_update_path.h -- which update path a particle type runs on (FIFO ring / range ring / compacting), stated once:
// the knobs the rule reads (FwPathPolicy), what it reads of one type of one descriptor (FwTypeFacts), the rule (fw_choose_path) and
// the census of the context's segments by path (FwPathCensus), which the rule reads and the launches pick their kernels from.
// Plain host C++: no HIP call, nothing of the engine (fw_ctx, SegHost).  The engine (fw_engine_build.cpp: choose_segment_path;
// fw_engine_paths.cpp: fifo_may_become_range; fw_engine.h: SegPathEdit) and a host test that holds the rule against a model of its own
// and the census against its recount (tests/test_cpp_host_update_path.py) compile the same lines.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/firework_hip.h"
#include "fw_kernels.h"

constexpr uint32_t kMaxFifoSegs = FW_FIFO_PER_LAUNCH;  // FIFO segments per context: one launch (beyond: fw_path_spills)

// ---- the census: how many segments of the context carry each SegHost flag a launch shape or the rule depends on
enum FwPathBit : uint32_t {
    FW_PATH_IN_USE = 1u << 0,
    FW_PATH_FIFO = 1u << 1,
    FW_PATH_RANGE = 1u << 2,
    FW_PATH_FEW_RING = 1u << 3,
    FW_PATH_SPILLED = 1u << 4,
    FW_PATH_SMALL = 1u << 5,
    FW_PATH_SMALL_OK = 1u << 6,
    FW_PATH_COLLIDES = 1u << 7,  // (counted only together with FW_PATH_SMALL: n_small_coll)
    FW_PATH_INST = 1u << 8,      // SegHost::inst != nullptr
    FW_PATH_SOLO = 1u << 9,
};

// Changes only through add / remove of one segment's bits: a segment whose flags change is taken out with its old bits and put back
// with its new ones (the engine: SegPathEdit, and nobody else).  A count that is one bit's alone may also move by that bit alone --
// add(FW_PATH_SOLO) is one increment once the constant is folded --; FW_PATH_SMALL and FW_PATH_COLLIDES count together and never so.
struct FwPathCensus {
    uint32_t n_in_use = 0;      // SegHost::in_use segments
    uint32_t n_fifo = 0;        // FIFO rings (at most kMaxFifoSegs: their records travel in kernel arguments)
    uint32_t n_range = 0;       // range rings
    uint32_t n_few = 0;         // ... that are rings only because the context holds few segments (SegHost::few_ring)
    uint32_t n_spilled = 0;     // ... that qualify for a FIFO ring one launch has no room for (SegHost::spilled)
    uint32_t n_small = 0;       // types on the wave-per-type kernel
    uint32_t n_small_ok = 0;    // ... and those that qualify for it
    uint32_t n_small_coll = 0;  // types on the kernel that have collision settings: its COLL instantiation
    uint32_t n_inst = 0;        // segments with an instance buffer attached: which instantiation the small launch runs
    uint32_t n_solo = 0;        // SegHost::solo segments
    // the context has outgrown the few-segments rule: no new small rings until it is back at half of range_few (a context whose
    // spawners come and go around the limit would convert rings at every crossing)
    bool few_blocked = false;

    static constexpr int kCounts = 10;
    void add(uint32_t bits) {
        n_in_use += bits & FW_PATH_IN_USE ? 1u : 0u, n_fifo += bits & FW_PATH_FIFO ? 1u : 0u, n_range += bits & FW_PATH_RANGE ? 1u : 0u;
        n_few += bits & FW_PATH_FEW_RING ? 1u : 0u, n_spilled += bits & FW_PATH_SPILLED ? 1u : 0u, n_small += bits & FW_PATH_SMALL ? 1u : 0u;
        n_small_ok += bits & FW_PATH_SMALL_OK ? 1u : 0u, n_small_coll += small_coll(bits), n_inst += bits & FW_PATH_INST ? 1u : 0u;
        n_solo += bits & FW_PATH_SOLO ? 1u : 0u;
    }
    // false, and nothing changed: some count the bits ask for is zero -- they were never added
    bool remove(uint32_t bits) {
        FwPathCensus one;
        one.add(bits);
        if (n_in_use < one.n_in_use || n_fifo < one.n_fifo || n_range < one.n_range || n_few < one.n_few || n_spilled < one.n_spilled ||
            n_small < one.n_small || n_small_ok < one.n_small_ok || n_small_coll < one.n_small_coll || n_inst < one.n_inst || n_solo < one.n_solo)
            return false;
        n_in_use -= one.n_in_use, n_fifo -= one.n_fifo, n_range -= one.n_range, n_few -= one.n_few, n_spilled -= one.n_spilled;
        n_small -= one.n_small, n_small_ok -= one.n_small_ok, n_small_coll -= one.n_small_coll, n_inst -= one.n_inst, n_solo -= one.n_solo;
        return true;
    }
    // The hysteresis of the few-segments rule (FwPathPolicy::range_few).  A spawner was built: blocked once the context holds more
    // than range_few segments, or a FIFO ring next to small rings (a context in which one comes and goes would otherwise convert its
    // small rings at every arrival).  true: the small rings leave now (drop_few_rings)
    bool spawner_built(uint32_t range_few) {
        if (n_in_use > range_few) few_blocked = true;
        const bool drop = n_few != 0 && (n_fifo != 0 || n_in_use > range_few);
        if (drop) few_blocked = true;
        return drop;
    }
    // ... a segment was released: free again at half of range_few
    void segment_released(uint32_t range_few) {
        if (n_in_use <= range_few / 2) few_blocked = false;
    }
    // the ten counts in the order of the fields, then few_blocked (fw_debug_path_census)
    void words(uint32_t out[kCounts + 1]) const {
        const uint32_t w[kCounts + 1] = {n_in_use, n_fifo, n_range, n_few, n_spilled, n_small, n_small_ok, n_small_coll, n_inst, n_solo, few_blocked ? 1u : 0u};
        for (int i = 0; i <= kCounts; i++) out[i] = w[i];
    }
    bool operator==(const FwPathCensus &o) const {
        uint32_t a[kCounts + 1], b[kCounts + 1];
        words(a), o.words(b);
        for (int i = 0; i <= kCounts; i++)
            if (a[i] != b[i]) return false;
        return true;
    }
    // the census of these segments, counted afresh; few_blocked is history, not a count: the caller's
    static FwPathCensus recount(const uint32_t *bits, size_t n, bool few_blocked) {
        FwPathCensus c;
        for (size_t i = 0; i < n; i++) c.add(bits[i]);
        c.few_blocked = few_blocked;
        return c;
    }

private:
    static uint32_t small_coll(uint32_t bits) { return (bits & (FW_PATH_SMALL | FW_PATH_COLLIDES)) == (FW_PATH_SMALL | FW_PATH_COLLIDES) ? 1u : 0u; }
};

// ---- the knobs of a context the rule reads (fw_ctx keeps and parses them; fw_engine.h: path_policy)
struct FwPathPolicy {
    bool use_fifo = true;             // FW_FIFO=0: one-lifetime types take the range or the compacting path
    uint32_t fifo_min = 32768;        // smallest capacity that makes a FIFO ring (FW_FIFO_MIN)
    bool fifo_nested = true;          // FW_FIFO_NESTED=0: not in spawners with Nested entries
    uint32_t fifo_small_tiles = 384;  // FIFO launches of fewer four-round tiles use one-round tiles (FW_FIFO_SMALL)
    bool use_ageless = true;          // FW_AGELESS=0: no ring runs under the age rule
    bool use_range = true;            // FW_RANGE=0: lifetime-range types take the compacting path
    uint32_t range_min = 8192;        // smallest capacity that makes a range ring (FW_RANGE_MIN)
    uint32_t range_few = 192;         // ... but for a context of up to this many segments, no FIFO ring among them (FW_RANGE_FEW; 0: off)
};

// ---- what the rule reads of type t of a descriptor
struct FwTypeFacts {
    uint32_t capacity = 0;                 // derived or given (derive_capacity)
    float life_min = 0.f, life_max = 0.f;  // fw_particle_settings::lifetime
    float life_lo_safe = 0.f;              // fw_life_lo_safe of them
    bool collides = false;                 // collision settings, or curve keys beyond the LDS staging (bigkeys): the feature kernels
    bool coll_inplace = false;             // ... without destroy_on_collision and with keys that fit: the COLL forms of the ring kernels
    uint32_t n_lplanes = 0;                // Nested entries that emit FROM the type (one last_emitted_age plane each)
    bool nested_fed = false;               // a Nested entry emits ONTO the type: the device alone knows its count
    uint32_t n_feeders = 0;                // entries that feed the type
    uint32_t n_global_feed = 0;            // ... the Global ones among them: each may add one op to a frame
    bool any_nested = false;               // the spawner has a Nested entry
    bool self_nested = false;              // ... one whose particles emit onto their own type
    bool mixed_feed = false;               // the type receives Nested children AND Global particles
    bool no_rings = false;                 // the spawner was poisoned: its rebuilt types stay off the in-place paths
};

// every particle of the type outlives a step of dt < this: lifetime = u * (max - min) + min, u in [0, 1), two ulps of margin for the
// rounding of the lerp; NaN when the range is not finite (never provably safe)
inline float fw_life_lo_safe(float life_min, float life_max) {
    if (!isfinite(life_min) || !isfinite(life_max)) return NAN;
    return nextafterf(nextafterf(life_max < life_min ? life_max : life_min, -INFINITY), -INFINITY);
}
// lifetime = lerp(min, max, u), u in [0, 1): no particle lives longer (std::max's choice of operand where one is NaN)
inline float fw_life_bound(float life_min, float life_max) { return life_min < life_max ? life_max : life_min; }

// one pass over the emission entries.  bigkeys: the type's curve keys exceed FW_KEYS_MAX floats
inline FwTypeFacts fw_type_facts(const fw_spawner_desc *d, uint32_t t, uint32_t capacity, bool bigkeys, bool no_rings) {
    const fw_particle_settings &p = d->particle_settings[t];
    FwTypeFacts f;
    f.capacity = capacity, f.no_rings = no_rings;
    f.life_min = p.lifetime.min, f.life_max = p.lifetime.max, f.life_lo_safe = fw_life_lo_safe(p.lifetime.min, p.lifetime.max);
    f.collides = p.collision.enabled != 0 || bigkeys;
    f.coll_inplace = p.collision.enabled != 0 && p.collision.destroy_on_collision == 0 && !bigkeys;
    for (uint32_t i = 0; i < d->n_emission_settings; i++) {
        const fw_emission_settings &e = d->emission_settings[i];
        const bool nested = e.mode == FW_MODE_NESTED, feeds = (uint32_t)e.particle_index == t;
        f.n_lplanes += nested && (uint32_t)e.target_particle_type == t ? 1u : 0u;
        f.nested_fed |= nested && feeds;
        f.n_feeders += feeds ? 1u : 0u;
        f.n_global_feed += e.mode == FW_MODE_GLOBAL && feeds ? 1u : 0u;
        f.any_nested |= nested;
        f.self_nested |= nested && e.target_particle_type == e.particle_index;
    }
    f.mixed_feed = f.nested_fed && f.n_global_feed != 0;
    return f;
}

// ---- the reasons, one predicate each
// an in-place ring at all: rings are switched on for the spawner; no particle of it emits onto its own type (a parent would see this
// frame's children as parents); the type does not receive Nested children AND Global particles (the Global ones would have to be
// placed behind a live count only the device knows); a colliding type only where a bounce changes neither age, lifetime nor order
inline bool fw_path_ring_ok(const FwTypeFacts &f) { return !f.no_rings && !f.self_nested && !f.mixed_feed && (!f.collides || f.coll_inplace); }
// a FIFO ring's particles all die in the order they were born: ONE finite lifetime value
inline bool fw_path_one_lifetime(const FwTypeFacts &f) { return f.life_min == f.life_max && isfinite(f.life_min); }
// a ring's spawn ops of a frame travel in the kernel arguments of its launch (FwInlineOps): a type fed by more Global entries takes
// the range or the compacting path, whose tiles read op tables from memory
inline bool fw_path_ops_fit_arguments(const FwTypeFacts &f) { return f.n_global_feed <= FW_INLINE_OPS; }
// ring slots are computed in 32 bits: head + index stays far from 2^32
inline bool fw_path_fifo_capacity_ok(uint32_t capacity) { return capacity < 0x40000000u; }
// more one-lifetime types than one FIFO launch holds: this one takes a range ring -- if it qualifies for one --, the FIFO rings of the
// context follow it at the end of the build (spill_fifo_rings), and while such rings exist further one-lifetime types join them.
// n_fifo and n_spilled count the types built BEFORE this one
inline bool fw_path_spills(const FwPathCensus &c) { return c.n_spilled != 0 || c.n_fifo >= kMaxFifoSegs; }
// a context of FEW segments, no FIFO ring among them, runs a small type on a range ring too (one kind of launch per frame).  n_in_use
// already counts the type being built
inline bool fw_path_few_segments(const FwPathPolicy &p, const FwPathCensus &c) {
    return p.range_few != 0 && !c.few_blocked && c.n_in_use <= p.range_few && c.n_fifo == 0;
}
// what a range ring asks that a type which already is a FIFO ring may fail (fifo_may_become_range shares these with the rule): range
// rings are on, at most two last_emitted_age planes (the old tiles carry them in registers), every particle provably outlives some
// step, slots addressed as 32-bit byte offsets into a float4 plane
inline bool fw_path_range_basics(const FwPathPolicy &p, bool no_rings, uint32_t n_lplanes, float life_lo_safe, uint32_t capacity) {
    return p.use_range && !no_rings && n_lplanes <= 2 && life_lo_safe > 0.0f && capacity <= FW_RANGE_MAX_CAPACITY;
}
// The few-nested exception: the capacity of a type that receives Nested children is derived from its parents' CAPACITY -- the host
// cannot bound their number -- and passes fifo_min for a handful of parents already (examples/textures.rs: 55 bullet cases, 110 puffs,
// 32 768 slots).  In a context of few segments such a type stays with its small parent type on range rings unless its derived
// capacity is really large.  (the two products are 32-bit ones)
inline bool fw_path_few_nested(const FwPathPolicy &p, const FwPathCensus &c, const FwTypeFacts &f) {
    return f.nested_fed && fw_path_few_segments(p, c) && f.capacity < 8u * p.fifo_min && f.capacity < p.range_min * 32u &&
           fw_path_range_basics(p, f.no_rings, f.n_lplanes, f.life_lo_safe, f.capacity);
}
// Position + age in four planes -- the layout the age rule needs -- only for a ring that can ever run under it: fed by Global entries
// alone, no Nested entry on it, no collisions, and large enough by itself for a streaming launch.  Everybody else keeps the float4
// (profiles/r18/ageless_ab.txt)
inline bool fw_path_q0_planes(const FwPathPolicy &p, const FwTypeFacts &f) {
    return p.use_ageless && p.fifo_small_tiles != 0u && !f.any_nested && !f.nested_fed && f.n_lplanes == 0 && !f.collides &&
           (uint64_t)f.capacity >= (uint64_t)p.fifo_small_tiles * FW_TILE;
}

struct FwPathChoice {
    bool fifo = false, range = false;  // neither: the compacting path (or, small_eligible, the wave-per-type kernel)
    bool few_ring = false;             // a range ring below range_min or by the few-nested exception: leaves with the other small rings
    bool spilled = false;              // a range ring that qualifies for a FIFO ring
    bool fifo_mat = false, fifo_dev = false, range_mat = false, range_dev = false;  // SegHost: rings of spawners with Nested entries
    bool q0pl = false;
    bool win_ok = false;               // the host bounds the live count by a lifetime window
};

// The rule.  `c` is the census as build_spawner's segment loop leaves it in front of the type: n_in_use counts the type being built,
// n_fifo and n_spilled the types built before it -- those of the same spawner included.
inline FwPathChoice fw_choose_path(const FwPathPolicy &p, const FwPathCensus &c, const FwTypeFacts &f) {
    FwPathChoice r;
    r.win_ok = !f.nested_fed && isfinite(fw_life_bound(f.life_min, f.life_max));
    const bool fifo_type = p.use_fifo && fw_path_ring_ok(f) && fw_path_one_lifetime(f) && fw_path_ops_fit_arguments(f) && f.capacity >= p.fifo_min &&
                           fw_path_fifo_capacity_ok(f.capacity) && (!f.any_nested || p.fifo_nested);
    const bool spill = fifo_type && fw_path_spills(c);
    const bool few_nested = fifo_type && !spill && fw_path_few_nested(p, c, f);
    r.fifo = fifo_type && !spill && !few_nested;
    if (r.fifo) {
        r.win_ok = false;  // (the cohort replay gives the exact count)
        r.fifo_mat = f.any_nested, r.fifo_dev = f.nested_fed;
        r.q0pl = fw_path_q0_planes(p, f);
    }
    // Range ring: any finite lifetime range -- a single value included, for the types a FIFO launch has no room for
    r.range = !r.fifo && fw_path_ring_ok(f) && isfinite(f.life_min) && isfinite(f.life_max) &&
              fw_path_range_basics(p, f.no_rings, f.n_lplanes, f.life_lo_safe, f.capacity) && (f.capacity >= p.range_min || fw_path_few_segments(p, c));
    if (r.range) {
        r.few_ring = f.capacity < p.range_min || few_nested;
        r.spilled = spill;
        r.range_mat = f.n_lplanes != 0, r.range_dev = f.nested_fed;
        if (r.range_dev) r.win_ok = false;
    }
    return r;
}
