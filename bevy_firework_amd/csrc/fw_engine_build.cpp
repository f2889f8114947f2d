// fw_engine_build.cpp -- sync_spawner_data (core.rs:343-365): descriptors -> device tables of one spawner (build_spawner), and back (release_spawner_segments)
// (host engine of libfirework_hip.so: fw_engine.h lists its translation units; there is no CPU simulation path in this library)
#include "fw_engine.h"

namespace fwh {

void copy_curve(CurveCopy &dst, int32_t kind, int32_t n, const float *times, const float *values, int stride) {
    dst.kind = kind;
    dst.n = n;
    dst.values.assign(values, values + (size_t)n * stride);
    dst.times.assign((size_t)n, 0.f);
    if (times && kind == FW_CURVE_UNEVEN) dst.times.assign(times, times + n);
    if (kind == FW_CURVE_UNEVEN && n >= 2) {
        // bevy_math UnevenCore::new: drop non-finite times, stable sort by time, dedup keeping the first
        std::vector<int> idx;
        for (int i = 0; i < n; i++)
            if (std::isfinite(dst.times[i])) idx.push_back(i);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return dst.times[a] < dst.times[b]; });
        std::vector<float> t, v;
        for (int i : idx) {
            if (!t.empty() && t.back() == dst.times[i]) continue;
            t.push_back(dst.times[i]);
            v.insert(v.end(), dst.values.begin() + (size_t)i * stride, dst.values.begin() + (size_t)(i + 1) * stride);
        }
        dst.times = t;
        dst.values = v;
        dst.n = (int32_t)t.size();
    }
    if (dst.n == 1) dst.kind = FW_CURVE_CONSTANT;  // curve.rs:46-49: one sample -> ConstantCurve
}

fw_status validate_desc(fw_ctx *ctx, const fw_spawner_desc *d) {
    if (!d) return fail(ctx, FW_EINVAL, "null descriptor");
    // (Vec<ParticleSettings> / Vec<EmissionSettings> of any length, core.rs:178-185; the counts are 32-bit here)
    if ((d->n_particle_settings && !d->particle_settings) || (d->n_emission_settings && !d->emission_settings))
        return fail(ctx, FW_EINVAL, "null settings array");
    for (uint32_t i = 0; i < d->n_particle_settings; i++) {
        const fw_particle_settings &p = d->particle_settings[i];
        const int32_t ns[3] = {p.scale_curve.n, p.base_color.n, p.emissive_color.n};
        const int32_t ks[3] = {p.scale_curve.kind, p.base_color.kind, p.emissive_color.kind};
        const void *vs[3] = {p.scale_curve.values, p.base_color.rgba, p.emissive_color.rgba};
        const void *ts[3] = {p.scale_curve.times, p.base_color.times, p.emissive_color.times};
        for (int k = 0; k < 3; k++) {
            if (ns[k] < 1) return fail(ctx, FW_EINVAL, "Cannot create curve from 0 samples");  // curve.rs:45,61,211,227
            if (ks[k] < 0 || ks[k] > 2 || !vs[k]) return fail(ctx, FW_EINVAL, "bad curve kind / null values");
            if (ks[k] == FW_CURVE_UNEVEN && !ts[k]) return fail(ctx, FW_EINVAL, "uneven curve without times");
            if (ks[k] == FW_CURVE_UNEVEN && ns[k] >= 2) {
                // UnevenCore::new drops non-finite times and duplicates; with fewer than two left it returns
                // Err(NotEnoughSamples) and the reference's `.unwrap()` panics (curve.rs:50,67,217,232)
                const float *tt = (const float *)ts[k];
                int distinct = 0;
                for (int a = 0; a < ns[k]; a++) {
                    if (!std::isfinite(tt[a])) continue;
                    bool dup = false;
                    for (int b = 0; b < a; b++) dup |= std::isfinite(tt[b]) && tt[b] == tt[a];
                    distinct += dup ? 0 : 1;
                }
                if (distinct < 2) return fail(ctx, FW_EINVAL, "uneven curve needs at least 2 distinct finite times");
            }
        }
    }
    for (uint32_t i = 0; i < d->n_emission_settings; i++) {
        const fw_emission_settings &e = d->emission_settings[i];
        if (e.particle_index < 0 || (uint32_t)e.particle_index >= d->n_particle_settings)
            return fail(ctx, FW_EINVAL, "emission_settings.particle_index out of range");  // index panic core.rs:392
        if (e.mode == FW_MODE_NESTED &&
            (e.target_particle_type < 0 || (uint32_t)e.target_particle_type >= d->n_particle_settings))
            return fail(ctx, FW_EINVAL, "target_particle_type out of range");  // index panic core.rs:488
        if (e.mode != FW_MODE_GLOBAL && e.mode != FW_MODE_NESTED) return fail(ctx, FW_EINVAL, "bad emission mode");
        if (e.pacing_kind < 0 || e.pacing_kind > 2) return fail(ctx, FW_EINVAL, "bad pacing kind");
        if (e.shape_kind < 0 || e.shape_kind > 2) return fail(ctx, FW_EINVAL, "bad shape kind");
    }
    return FW_OK;
}

// capacity heuristic: expected live count from the emitters feeding a type, x1.25 + slack
uint32_t derive_capacity(const fw_spawner_desc *d, uint32_t t, const std::vector<uint32_t> &caps, double *expect_live) {
    const fw_particle_settings &p = d->particle_settings[t];
    const uint32_t FW_CAP_ROUND = std::max<uint32_t>(FW_TILE, fw_range_young_tile());  // every kernel's tile divides a capacity
    if (p.capacity && !expect_live) return round_up(std::max<uint32_t>(p.capacity, FW_TILE), FW_CAP_ROUND);
    const double life = std::max(0.0, (double)std::max(p.lifetime.min, p.lifetime.max));
    double need = 0;
    for (uint32_t i = 0; i < d->n_emission_settings; i++) {
        const fw_emission_settings &e = d->emission_settings[i];
        if ((uint32_t)e.particle_index != t) continue;
        if (e.mode == FW_MODE_GLOBAL) {
            if (e.pacing_kind == FW_PACING_ONESHOT)
                need += (double)e.oneshot_count;
            else if (e.pacing_kind == FW_PACING_COUNT_OVER_DURATION && e.duration > 0 && e.count > 0)
                need += (double)e.count / e.duration * (life + 0.05) + 2 * (double)e.count / e.duration / 30.0;
        } else if (e.pacing_kind == FW_PACING_COUNT_OVER_DURATION && e.count > 0) {
            const fw_particle_settings &pp = d->particle_settings[e.target_particle_type];
            const double plife = std::max(1e-3, (double)std::min(pp.lifetime.min, pp.lifetime.max));
            const double pcap = caps[e.target_particle_type] ? caps[e.target_particle_type] : kMinCapacity;
            need += pcap * (double)e.count * std::max(1.0, life / plife + 0.1);
        }
    }
    if (expect_live) *expect_live = need;  // (what the emitters sustain: SegHost::expect_live)
    if (p.capacity) return round_up(std::max<uint32_t>(p.capacity, FW_TILE), FW_CAP_ROUND);
    need = need * 1.25 + kMinCapacity;
    if (need > 3.0e9) need = 3.0e9;
    return round_up((uint32_t)need, FW_CAP_ROUND);
}

void fill_randvec3(const fw_rand_vec3 &r, float &mn, float &mx, float &spread, float dir[4], float arc[4]) {
    mn = r.magnitude.min, mx = r.magnitude.max, spread = r.spread;
    dir[0] = r.direction[0], dir[1] = r.direction[1], dir[2] = r.direction[2], dir[3] = 0.f;
    fw_q4 q = fw_quat_from_rotation_arc(fw_v3{0.f, 1.f, 0.f}, fw_v3{r.direction[0], r.direction[1], r.direction[2]});
    arc[0] = q.x, arc[1] = q.y, arc[2] = q.z, arc[3] = q.w;
}

// ---- The axis-spin rule (round 12; SegHost::axis, FW_TYPE_IDX_AXIS in fw_device.h) -------------------------------------------------
// Decides, when a spawner is built, whether every particle of type t turns about ONE coordinate axis k for ever.  Then the other two
// components -- call them a and b -- of its angular velocity and of its rotation are +0 (bits 0x00000000) after every update, and a
// FIFO ring of the type neither loads nor stores those four planes (fw_update_fifo_body): it puts +0 in the registers and runs the
// same fw_integrate_store, whose per-plane bit test then finds nothing to store.
// Conditions (all tested below; "+0" always means the bit pattern, -0 fails):
//   (C1) every entry that feeds the type: angular-velocity spread not > 0 (the `dir` arm of fw_randvec3), direction a and b +0,
//        direction k finite, magnitude min and max finite with the sign bit clear;
//   (C2) every such entry: initial_rotation a and b +0, k and w finite;
//   (C3) the type: angular_acceleration a and b +0, k == 0; angular_drag finite with the sign bit clear;
//   (C4) wmax = max over the entries of |dir k| * max(mag.min, mag.max) is finite;
//   per frame (axis_dt_ok): dt finite with the sign bit clear, 0.25f * (wmax * dt)^2 < 0.6f in fp32, drag * dt <= 1.
// Proof, for the arithmetic as compiled (fp32, round to nearest, no fast-math; -ffp-contract may fuse a product into the sum that
// follows it, it never reorders sums).  Two facts about zeros are all it needs: (Z1) (+0) * p = +0 for finite p with the sign bit
// clear, and (+0) * p is a zero of some sign for any finite p; (Z2) a sum -- fused or not -- of zeros, one of which is +0, is +0:
// round to nearest gives -0 only when EVERY addend is -0, and x - y adds -y.
//   Spawn (fw_spawn_one): m = u * (max - min) + min with u in [0, 1).  max - min is finite, the exact value lies between min and max,
//   both >= +0, rounding is monotonic and an exact 0 from a non-trivial sum is +0; fused or not, m is finite with the sign bit clear
//   (u = 0 and max < min give -0 + min with min > 0).  angular velocity = dir * m: components a, b are (+0) * m = +0 by Z1;
//   |component k| <= |dir k| * max(min, max) <= wmax (monotonic rounding).  rotation = initial_rotation: a, b +0, k, w finite.
//   Update, induction step (fw_integrate_store): assume w_a = w_b = +0, |w_k| <= wmax, q_a = q_b = +0, q_k and q_w finite.
//   - v = w * dt: v_a = v_b = (+0) * dt = +0 (Z1: dt finite, sign clear -- a negative dt or -0 would give -0, hence the test).
//   - fw_quat_step: h2 = 0.25 * (v_x^2 + v_y^2 + v_z^2); the two zero squares are +0 and add nothing, however the sum is fused, so
//     h2 = 0.25 * fl(v_k^2) <= 0.25 * fl(fl(wmax * dt)^2) < 0.6 by monotonic rounding: EVERY lane of every wave of the ring takes the
//     polynomial arm (the ballot is over lanes of this type only: every caller reaches fw_integrate_store under `if (alive)` /
//     `if (mine)`, so the ballot sees the ring's own live lanes and nothing else -- a caller that ran it on unmasked lanes would void
//     this step), the libm arm -- cos(h) < 0 there could make every addend of a sum
//     below -0 -- is never entered.  On [0, 0.6) the polynomial values are sh in [0.45, 0.5] and c in [0.7, 1]: finite, positive.
//     dq_a = dq_b = (+0) * sh = +0 (Z1), dq_k = v_k * sh finite, dq_w = c > 0.
//   - fw_quat_mul(dq, q) (fw_math.h): the x, y and z sums each START with dq.w * q.<same component>.  For component a that is
//     c * (+0) = +0 (Z1); the other three products each contain dq_a, dq_b, q_a or q_b -- a +0 times a finite number -- so they are
//     zeros of some sign.  Sums are evaluated left to right, every partial sum contains that first +0: by Z2 each is +0, whichever
//     products the compiler fuses.  The same for b.  So q'_a = q'_b = +0.  q'_k, q'_w stay finite: |q'| <= |q| (1 + 8 eps) per update,
//     finite for more than 10^8 updates of one particle at worst-case rounding.
//   - angular velocity, component a: w_a + (acc_a - drag * w_a) * dt.  drag * (+0) = +0 (Z1), (+0) - (+0) = +0, or fused
//     fma(-drag, +0, +0) = (-0) + (+0) = +0 (Z2); (+0) * dt = +0; (+0) + (+0) = +0, or fma(+0, dt, +0) = +0.  The same for b.
//     Component k: acc_k is a zero, t = drag * w_k * dt has the sign of w_k and |t| <= |w_k| (1 + 3 eps) since drag * dt <= 1,
//     so |w_k - t| <= |w_k| <= wmax: the bound on h2 holds in every later frame.
// `full` lanes (a particle's first update) and every spawn path store all planes, so the planes hold the true values -- the zeros
// included -- at all times; readers never look at the rule, and a frame that runs without it loads what is there.  After such a
// frame (libm arm, or a drag that overshoots) a plane may hold -0: the rule does not come back (launch_fifo).
static uint32_t f32_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}
static uint32_t axis_spin_rule(const fw_spawner_desc *d, uint32_t t, float *wmax_out) {
    const fw_particle_settings &p = d->particle_settings[t];
    if (!std::isfinite(p.angular_drag) || std::signbit(p.angular_drag)) return 0u;  // (C3)
    for (uint32_t k = 0; k < 3; k++) {
        const uint32_t a = (k + 1) % 3, b = (k + 2) % 3;
        if (f32_bits(p.angular_acceleration[a]) != 0u || f32_bits(p.angular_acceleration[b]) != 0u || p.angular_acceleration[k] != 0.f) continue;
        bool ok = true, fed = false;
        float wmax = 0.f;
        for (uint32_t i = 0; i < d->n_emission_settings && ok; i++) {
            const fw_emission_settings &e = d->emission_settings[i];
            if ((uint32_t)e.particle_index != t) continue;
            fed = true;
            const fw_rand_vec3 &w = e.initial_angular_velocity;
            ok = !(w.spread > 0.f) && f32_bits(w.direction[a]) == 0u && f32_bits(w.direction[b]) == 0u && std::isfinite(w.direction[k]) &&
                 std::isfinite(w.magnitude.min) && std::isfinite(w.magnitude.max) && !std::signbit(w.magnitude.min) && !std::signbit(w.magnitude.max) &&  // (C1)
                 f32_bits(e.initial_rotation[a]) == 0u && f32_bits(e.initial_rotation[b]) == 0u && std::isfinite(e.initial_rotation[k]) &&
                 std::isfinite(e.initial_rotation[3]);  // (C2)
            if (ok) wmax = std::max(wmax, std::fabs(w.direction[k]) * std::max(w.magnitude.min, w.magnitude.max));
        }
        if (ok && fed && std::isfinite(wmax)) {  // (C4)
            *wmax_out = wmax;
            return k + 1u;
        }
    }
    return 0u;
}
// the per-frame half of the rule: this dt keeps every particle of the ring inside the proof
bool axis_dt_ok(const SegHost &S, float dt) {
    if (!std::isfinite(dt) || std::signbit(dt)) return false;
    const float v = S.axis_wmax * dt, h2 = 0.25f * (v * v);
    return h2 < 0.6f && S.axis_drag * dt <= 1.0f;
}

// FW_TYPE_NOSPIN (fw_device.h): no particle of type t can ever turn -- no angular acceleration, a finite angular drag (0 * inf = NaN,
// core.rs:648-650 would turn a zero angular velocity into NaN), and every entry that feeds the type spawns with zero angular velocity
// and the same rotation, which const_rot receives
static bool nospin_rule(const fw_spawner_desc *d, uint32_t t, float const_rot[4]) {
    const fw_particle_settings &p = d->particle_settings[t];
    if (!(p.angular_acceleration[0] == 0.f && p.angular_acceleration[1] == 0.f && p.angular_acceleration[2] == 0.f && std::isfinite(p.angular_drag)))
        return false;
    const fw_emission_settings *first = nullptr;
    for (uint32_t i = 0; i < d->n_emission_settings; i++) {
        const fw_emission_settings &e = d->emission_settings[i];
        if ((uint32_t)e.particle_index != t) continue;
        if (!(e.initial_angular_velocity.magnitude.min == 0.f && e.initial_angular_velocity.magnitude.max == 0.f &&
              (!first || memcmp(first->initial_rotation, e.initial_rotation, sizeof e.initial_rotation) == 0)))
            return false;
        if (!first) first = &e;
    }
    if (!first) return false;
    // (+ 0.0f: a negative zero component becomes +0, which is what from_scaled_axis(0) * rotation makes of it in all but contrived
    // cases; every reader then sees the same bits)
    for (int c = 0; c < 4; c++) const_rot[c] = first->initial_rotation[c] + 0.0f;
    return true;
}

uint32_t pad4(uint32_t n) { return (n + 3u) & ~3u; }

// ---- build_spawner: the device tables (types, keys, emits, segments) of one spawner, step by step.  The order of the device
// allocations and copies is part of the contract: tests/test_gpu_resources.py walks FW_FAIL_ALLOC=k over it.

// a device table with room for `need` entries, the first `used` kept (amortised growth, zero-filled) and its FwGlobals view
template <typename B, typename V>
static fw_status reserve_table(fw_ctx *ctx, B &b, size_t need, size_t used, V **view) {
    return need <= b.cap() ? FW_OK : grow_buf(ctx, b, std::max<size_t>(need, b.cap() * 2 + 64), true, used, view);
}

// room in every table of the context for nt more types and ne more emission entries
static fw_status reserve_tables(fw_ctx *ctx, uint32_t nt, uint32_t ne) {
    if (ctx->levels.size() < ne) ctx->levels.resize(ne);
    fw_status st;
    if ((st = reserve_table(ctx, ctx->d_types, ctx->n_types + nt, ctx->n_types, &ctx->g.types))) return st;
    if ((st = reserve_table(ctx, ctx->d_type_coll, ctx->n_types + nt, ctx->n_types, &ctx->g.type_coll))) return st;
    if ((st = reserve_table(ctx, ctx->d_emits, ctx->n_emits + ne, ctx->n_emits, &ctx->g.emits))) return st;
    if ((st = reserve_table(ctx, ctx->d_emit_serial, ctx->n_emit_slots + ne, ctx->n_emit_slots, &ctx->g.emit_serial))) return st;
    if ((st = reserve_table(ctx, ctx->d_nest_start, ctx->n_emit_slots + ne, ctx->n_emit_slots, &ctx->g.nest_start))) return st;
    if (ctx->nest_ticket_base.size() < ctx->n_emit_slots + ne) ctx->nest_ticket_base.resize(ctx->n_emit_slots + ne, 0u);
    if ((st = reserve_table(ctx, ctx->d_segs, ctx->segs.size() + nt, ctx->segs.size(), &ctx->g.segs))) return st;
    return ensure_max_seg(ctx, (uint32_t)ctx->segs.size() + nt);
}

// what the steps of one type's build hand each other
struct TypeBuild {
    uint32_t t = 0, capacity = 0;
    FwType dt{};
    FwTypeColl dc{};
    bool nospin = false, bigkeys = false;
    std::vector<float> keys;
    uint32_t type_idx = 0, keys_cap = 0;
    uint32_t si = kNoSeg;
};

// the host's copy of the type's settings (descriptors are copied, never kept) and the device records FwType / FwTypeColl, but for
// what the next steps add: the key offsets, FW_TYPE_DERIVED
static void make_type_records(const fw_ctx *ctx, const fw_spawner_desc *d, TypeHost &T, TypeBuild &b) {
    const fw_particle_settings &p = d->particle_settings[b.t];
    T.ps = p;
    copy_curve(T.scale, p.scale_curve.kind, p.scale_curve.n, p.scale_curve.times, p.scale_curve.values, 1);
    copy_curve(T.base, p.base_color.kind, p.base_color.n, p.base_color.times, p.base_color.rgba, 4);
    copy_curve(T.emis, p.emissive_color.kind, p.emissive_color.n, p.emissive_color.times, p.emissive_color.rgba, 4);
    T.life_lo_safe = fw_life_lo_safe(p.lifetime.min, p.lifetime.max);
    T.ps.scale_curve.times = T.ps.scale_curve.values = nullptr;
    T.ps.base_color.times = T.ps.base_color.rgba = nullptr;
    T.ps.emissive_color.times = T.ps.emissive_color.rgba = nullptr;

    FwType &dt = b.dt;
    memcpy(dt.acc, p.acceleration, sizeof dt.acc);
    memcpy(dt.angacc, p.angular_acceleration, sizeof dt.angacc);
    dt.lin_drag = p.linear_drag, dt.ang_drag = p.angular_drag;
    dt.sc_kind = T.scale.kind, dt.sc_n = T.scale.n;
    dt.bc_kind = T.base.kind, dt.bc_n = T.base.n;
    dt.em_kind = T.emis.kind, dt.em_n = T.emis.n;
    dt.pbr = p.pbr, dt.report_destroyed = p.report_destroyed;
    b.nospin = ctx->use_nospin && nospin_rule(d, b.t, dt.const_rot);
    if (b.nospin) dt.flags |= FW_TYPE_NOSPIN;
    b.dc.coll_flags = (p.collision.enabled ? FW_COLL_ENABLED : 0u) | (p.collision.enabled && p.collision.destroy_on_collision ? FW_COLL_DESTROY : 0u);
    b.dc.coll_mask = p.collision.filter_mask;
    b.dc.coll_restitution = p.collision.restitution, b.dc.coll_friction = p.collision.friction;
}

// the curve keys of the type, packed; a type index (a released one first) and a window of the key pool: the first released one that
// is large enough, or fresh floats at the end
static fw_status pack_keys_take_window(fw_ctx *ctx, const TypeHost &T, TypeBuild &b) {
    std::vector<float> &keys = b.keys;
    FwType &dt = b.dt;
    auto put = [&](const std::vector<float> &v, uint32_t padded) {
        uint32_t off = (uint32_t)keys.size();
        keys.insert(keys.end(), v.begin(), v.end());
        keys.resize(off + padded, 0.f);
        return off;
    };
    put(T.scale.times, pad4(T.scale.n));
    dt.o_sc_v = put(T.scale.values, pad4(T.scale.n));
    dt.o_bc_t = put(T.base.times, pad4(T.base.n));
    dt.o_bc_v = put(T.base.values, 4 * T.base.n);
    dt.o_em_t = put(T.emis.times, pad4(T.emis.n));
    dt.o_em_v = put(T.emis.values, 4 * T.emis.n);
    if (keys.size() >= (1u << 30)) return fail(ctx, FW_EINVAL, "curve keys exceed 2^30 floats");
    b.bigkeys = keys.size() > FW_KEYS_MAX;  // beyond the LDS staging area of the streaming kernels
    if (!ctx->free_types.empty()) {
        b.type_idx = ctx->free_types.back();
        ctx->free_types.pop_back();
    } else {
        b.type_idx = ctx->n_types++;
    }
    uint32_t kwin_off = 0;
    for (size_t fi = 0; fi < ctx->free_keys.size(); fi++)
        if (ctx->free_keys[fi].second >= keys.size()) {
            kwin_off = ctx->free_keys[fi].first, b.keys_cap = ctx->free_keys[fi].second;
            ctx->free_keys.erase(ctx->free_keys.begin() + (long)fi);
            break;
        }
    if (!b.keys_cap) {
        b.keys_cap = std::max<uint32_t>(64u, pad4((uint32_t)keys.size()));
        if (fw_status st = reserve_table(ctx, ctx->d_keys, ctx->keys_end + b.keys_cap, ctx->keys_end, &ctx->g.keys)) return st;
        kwin_off = (uint32_t)ctx->keys_end;
        ctx->keys_end += b.keys_cap;
    }
    dt.keys_off = kwin_off;
    dt.keys_len = (uint32_t)keys.size();
    return FW_OK;
}

// The segment: the slot, its type index, its key window and the spawner's reference to it are recorded BEFORE anything that can fail,
// so that release_spawner_segments undoes a build that stops half-way (nothing leaks, nothing dangles).  Then what the type's records
// say of the segment, and the records themselves go to the device.
static fw_status take_segment_slot(fw_ctx *ctx, SpawnerHost &sp, int h, const fw_spawner_desc *d, TypeBuild &b) {
    const fw_particle_settings &p = d->particle_settings[b.t];
    FwType &dt = b.dt;
    uint32_t si = (uint32_t)ctx->segs.size();
    for (uint32_t k = 0; k < ctx->segs.size(); k++)
        if (!ctx->segs[k].in_use) {
            si = k;
            break;
        }
    if (si == ctx->segs.size()) ctx->segs.push_back(SegHost{});
    SegHost &S = ctx->segs[si];
    {
        SegPathEdit edit(ctx, S);
        S = SegHost{};
        S.in_use = true, S.spawner = h, S.type = (int)b.t, S.type_idx = b.type_idx;
    }
    ctx->big_dirty = true;
    S.keys_off = dt.keys_off, S.keys_len = dt.keys_len, S.keys_cap = b.keys_cap, S.bigkeys = b.bigkeys;
    sp.seg[b.t] = b.si = si;
    S.nospin = b.nospin, S.n_xplanes = b.nospin ? 1u : 0u;
    if (ctx->use_axis && !b.nospin) S.axis = axis_spin_rule(d, b.t, &S.axis_wmax), S.axis_drag = p.angular_drag;
    if (b.type_idx > FW_TYPE_IDX_MASK) return fail(ctx, FW_EINVAL, "more particle types than a type index holds");
    // scale and colours are left to the readers from the first frame on (fw_ctx::derive_all; wants_derived: not for a type that
    // runs on the collision kernels)
    S.derived = ctx->use_derived && ctx->derive_all && !(p.collision.enabled != 0 || b.bigkeys);
    if (S.derived) dt.flags |= FW_TYPE_DERIVED;
    memcpy(S.const_rot, dt.const_rot, sizeof S.const_rot);
    FW_HIP(ctx, hipMemcpy(ctx->d_keys + dt.keys_off, b.keys.data(), b.keys.size() * sizeof(float), hipMemcpyHostToDevice));
    FW_HIP(ctx, hipMemcpy(ctx->d_types + b.type_idx, &dt, sizeof dt, hipMemcpyHostToDevice));
    FW_HIP(ctx, hipMemcpy(ctx->d_type_coll + b.type_idx, &b.dc, sizeof b.dc, hipMemcpyHostToDevice));
    return FW_OK;
}

// Which update path the type runs on: the rule (fw_update_path.h: fw_choose_path, from the knobs, the census as it stands -- this
// segment counted as in use, its path not yet -- and the facts of the type) and what the choice means for the segment and the context
static fw_status choose_segment_path(fw_ctx *ctx, const SpawnerHost &sp, const fw_spawner_desc *d, const TypeBuild &b) {
    const fw_particle_settings &p = d->particle_settings[b.t];
    const TypeHost &T = sp.types[b.t];
    SegHost &S = ctx->segs[b.si];
    const FwTypeFacts f = fw_type_facts(d, b.t, b.capacity, b.bigkeys, sp.no_rings);
    const FwPathChoice c = fw_choose_path(path_policy(ctx), ctx->census, f);
    for (uint32_t i = 0; i < d->n_emission_settings; i++)  // the emission entry each last_emitted_age plane belongs to
        if (d->emission_settings[i].mode == FW_MODE_NESTED && (uint32_t)d->emission_settings[i].target_particle_type == b.t)
            S.lplane_emission.push_back((int32_t)i);
    S.auto_capacity = p.capacity == 0;
    S.life_bound = (double)fw_life_bound(p.lifetime.min, p.lifetime.max);
    S.one_feeder = f.n_feeders == 1 && f.n_global_feed == 1;
    fw_status st;
    SegPathEdit edit(ctx, S);
    S.n_lplanes = f.n_lplanes, S.nested_fed = f.nested_fed, S.collides = f.collides, S.coll_inplace = f.coll_inplace;
    S.fifo = c.fifo, S.range = c.range, S.few_ring = c.few_ring, S.spilled = c.spilled;
    S.fifo_mat = c.fifo_mat, S.fifo_dev = c.fifo_dev, S.range_mat = c.range_mat, S.range_dev = c.range_dev;
    S.q0pl = c.q0pl, S.win_ok = c.win_ok;
    if (S.fifo) {
        if (S.fifo_dev && (st = alloc_buf(ctx, S.h_report, kReportRing, Mem::pinned, true))) return st;
        S.fifo_life = 0.0f * (p.lifetime.max - p.lifetime.min) + p.lifetime.min;  // u * (max - min) + min, any u
        memcpy(S.fifo_move, p.acceleration, 3 * sizeof(float)), S.fifo_move[3] = p.linear_drag;  // (what the type's record holds)
        S.fifo_wm = (T.base.kind != 0 ? 1 : 0) | (T.emis.kind != 0 ? 2 : 0) | (T.scale.kind != 0 ? 4 : 0);
    }
    if (S.range) {
        S.range_life_lo = T.life_lo_safe;
        ctx->range_life_max = std::max(ctx->range_life_max, S.range_life_lo);
        ctx->r_force = true;
        if (S.range_dev) {
            ctx->range_age_keep = std::max(ctx->range_age_keep, (float)(S.life_bound * 1.01 + 1e-3));
            if ((st = alloc_buf(ctx, S.h_report, kReportRing, Mem::pinned, true))) return st;
        }
    }
    return FW_OK;
}

// the particle memory of the segment, and what the host keeps next to it: the colours its planes are filled with, what its emitters
// sustain; a small type joins the wave-per-type kernel
static fw_status alloc_type_buffers(fw_ctx *ctx, const SpawnerHost &sp, const fw_spawner_desc *d, const std::vector<uint32_t> &caps, const TypeBuild &b) {
    const TypeHost &T = sp.types[b.t];
    SegHost &S = ctx->segs[b.si];
    for (int c = 0; c < 4; c++) {  // the first key is the colour at age 0 (and, for one key, at every age)
        S.fill_bc[c] = T.base.values.empty() ? 0.f : T.base.values[c];
        S.fill_em[c] = T.emis.values.empty() ? 0.f : T.emis.values[c];
    }
    S.colors_dirty = false;
    double expect = 0.0;
    derive_capacity(d, b.t, caps, &expect);
    S.expect_live = (float)std::min(expect, 3.0e9);
    SegBufs nb;
    if (fw_status st = alloc_seg_buffers(ctx, S, b.capacity, S.ring(), d->particle_settings[b.t].report_destroyed != 0, nb)) return st;
    S.take(std::move(nb));
    if (small_eligible(ctx, S)) enter_small(ctx, S);  // (the wave-per-type kernel)
    return FW_OK;
}

// the segment's record goes to the device; its counters start at zero
static fw_status upload_segment_zeroed(fw_ctx *ctx, uint32_t si) {
    if (fw_status st = upload_seg(ctx, si)) return st;
    const uint32_t zero2[2] = {0, 0};
    for (int r = 0; r < 2; r++) {
        FW_HIP(ctx, hipMemcpy(ctx->g.count + (size_t)r * ctx->max_seg + si, zero2, 4, hipMemcpyHostToDevice));
        FW_HIP(ctx, hipMemcpy(ctx->g.spawned + (size_t)r * ctx->max_seg + si, zero2, 4, hipMemcpyHostToDevice));
        FW_HIP(ctx, hipMemcpy(ctx->g.appended + (size_t)r * ctx->max_seg + si, zero2, 4, hipMemcpyHostToDevice));
        FW_HIP(ctx, hipMemcpy(ctx->g.rold + (size_t)r * ctx->max_seg + si, zero2, 4, hipMemcpyHostToDevice));
    }
    FW_HIP(ctx, hipMemcpy(ctx->g.ndestroyed + si, zero2, 4, hipMemcpyHostToDevice));
    FW_HIP(ctx, hipMemcpy(ctx->g.range_ticket + si, zero2, 4, hipMemcpyHostToDevice));  // (S.ticket_base is 0: a fresh SegHost)
    return FW_OK;
}

// the emission entries: their host clocks (sync_spawner_data core.rs:350-358) and their device records
static fw_status build_emit_records(fw_ctx *ctx, SpawnerHost &sp, const fw_spawner_desc *d, const std::vector<uint64_t> *carry_serial) {
    for (uint32_t i = 0; i < d->n_emission_settings; i++) {
        EmissionHost &E = sp.em[i];
        const fw_emission_settings &e = d->emission_settings[i];
        E.es = e;
        E.between = (e.offset_end - e.offset_start) / e.count;
        E.last_emission = 0.f, E.time_passed_in_cycle = 0.f;
        E.enabled = d->starts_enabled != 0;
        E.emits_on_other_particles = e.mode == FW_MODE_NESTED;
        E.dst_seg = sp.seg[e.particle_index];
        E.life_lo_safe = sp.types[e.particle_index].life_lo_safe;
        E.serial = carry_serial && i < carry_serial->size() ? (*carry_serial)[i] : 0;
        const fw_particle_settings &p = d->particle_settings[e.particle_index];
        FwEmit de{};
        de.shape_kind = e.shape_kind, de.shape_radius = e.shape_radius;
        de.uid = d->uid, de.emission_index = i;
        fw_q4 sa = fw_quat_from_rotation_arc(fw_v3{0.f, 1.f, 0.f},
                                             fw_v3{e.shape_normal[0], e.shape_normal[1], e.shape_normal[2]});
        de.shape_arc[0] = sa.x, de.shape_arc[1] = sa.y, de.shape_arc[2] = sa.z, de.shape_arc[3] = sa.w;
        fill_randvec3(e.initial_velocity, de.v_mag_min, de.v_mag_max, de.v_spread, de.v_dir, de.v_arc);
        fill_randvec3(e.initial_angular_velocity, de.w_mag_min, de.w_mag_max, de.w_spread, de.w_dir, de.w_arc);
        de.inherit = e.inherit_parent_velocity;
        de.type_idx = ctx->segs[sp.seg[e.particle_index]].type_idx;
        memcpy(de.init_rot, e.initial_rotation, sizeof de.init_rot);
        de.radial_min = e.initial_velocity_radial.min, de.radial_max = e.initial_velocity_radial.max;
        de.iscale_min = p.initial_scale.min, de.iscale_max = p.initial_scale.max;
        de.life_min = p.lifetime.min, de.life_max = p.lifetime.max;
        de.n_count = e.count, de.n_start = e.offset_start, de.n_end = e.offset_end;
        de.n_lplane = 0;
        if (e.mode == FW_MODE_NESTED) {
            const SegHost &P = ctx->segs[sp.seg[e.target_particle_type]];
            for (uint32_t k = 0; k < P.n_lplanes; k++)
                if (P.lplane_emission[k] == (int32_t)i) de.n_lplane = k;
        }
        if (!ctx->free_emits.empty()) {
            E.emit_idx = ctx->free_emits.back();
            ctx->free_emits.pop_back();
        } else {
            E.emit_idx = ctx->n_emits++;
        }
        if (!ctx->free_emit_slots.empty()) {
            E.emit_slot = ctx->free_emit_slots.back();
            ctx->free_emit_slots.pop_back();
        } else {
            E.emit_slot = ctx->n_emit_slots++;
        }
        E.assigned = true;
        FW_HIP(ctx, hipMemcpy(ctx->d_emits + E.emit_idx, &de, sizeof de, hipMemcpyHostToDevice));
        const unsigned long long s0 = E.serial;
        FW_HIP(ctx, hipMemcpy(ctx->d_emit_serial + E.emit_slot, &s0, sizeof s0, hipMemcpyHostToDevice));
        const uint32_t t0 = 0u;
        FW_HIP(ctx, hipMemcpy(ctx->d_nest_start + E.emit_slot, &t0, sizeof t0, hipMemcpyHostToDevice));
        ctx->nest_ticket_base[E.emit_slot] = 0u;
    }
    return FW_OK;
}

// ring types other particles' entries emit from that need no materialisation (SegHost::virt_parent)
static fw_status mark_virtual_parents(fw_ctx *ctx, const SpawnerHost &sp, const fw_spawner_desc *d) {
    for (uint32_t t = 0; t < d->n_particle_settings; t++) {
        SegHost &S = ctx->segs[sp.seg[t]];
        if (!S.ring() || S.nested_fed || S.n_lplanes > 2) continue;
        if (S.n_lplanes == 0) {  // (no entry emits from it or onto it: nothing in a Nested pass ever looks at its particles)
            S.virt_parent = true;
            continue;
        }
        const fw_particle_settings &p = d->particle_settings[t];
        bool ok = std::min(p.lifetime.min, p.lifetime.max) > 0.0f;
        for (uint32_t k = 0; k < S.n_lplanes && ok; k++) {
            const fw_emission_settings &e = d->emission_settings[S.lplane_emission[k]];
            ok = e.pacing_kind == FW_PACING_COUNT_OVER_DURATION && e.count > 0.0f && e.offset_start >= 0.0f && e.offset_end >= e.offset_start &&
                 std::isfinite(e.count) && std::isfinite(e.offset_end);
        }
        S.virt_parent = ok;
        if (fw_status st = ok ? upload_seg(ctx, sp.seg[t]) : FW_OK) return st;
    }
    return FW_OK;
}

// What the new segments mean for the context as a whole (callers of build_spawner have synchronised it): the arrays sized by the
// segments; FIFO rings that follow a spilled type onto range rings; small rings that leave because the context is no longer one of
// few segments without a FIFO ring (FwPathCensus::spawner_built); the small-type kernel's mode
static fw_status context_follow_ups(fw_ctx *ctx) {
    fw_status st;
    if ((st = ensure_range_arrays(ctx))) return st;
    if ((st = ensure_tile_arrays(ctx))) return st;
    if (ctx->segs.size() > ctx->small_cap) {  // the small-type list (fw_ctx::d_small): room for every segment slot; fw_step never allocates
        if ((st = sync(ctx))) return st;
        const size_t ncap = ctx->segs.size() * 2 + 256;
        ctx->small_cap = 0, ctx->small_fence.forget();
        if ((st = alloc_buf(ctx, ctx->d_small, ncap)) || (st = alloc_buf(ctx, ctx->h_small, ncap, Mem::pinned))) return st;
        ctx->small_cap = ncap, ctx->small_dirty = true;
    }
    if (ctx->census.n_spilled && ctx->census.n_fifo && (st = spill_fifo_rings(ctx))) return st;
    if (ctx->census.spawner_built(ctx->range_few) && (st = drop_few_rings(ctx))) return st;
    update_small_mode(ctx);
    return FW_OK;
}

fw_status build_spawner(fw_ctx *ctx, int h, const fw_spawner_desc *d, const std::vector<uint64_t> *carry_serial) {
    SpawnerHost &sp = ctx->spawners[h];
    drop_forecast_and_boxes(ctx);
    ctx->tab_force = true;
    const uint32_t nt = d->n_particle_settings, ne = d->n_emission_settings;
    sp.uid = d->uid;
    sp.starts_enabled = d->starts_enabled;
    sp.types.assign(nt, TypeHost{});
    sp.em.assign(ne, EmissionHost{});
    sp.seg.assign(nt, kNoSeg);
    fw_status st;
    if ((st = reserve_tables(ctx, nt, ne))) return st;

    std::vector<uint32_t> caps(nt, 0);
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t t = 0; t < nt; t++) caps[t] = derive_capacity(d, t, caps);

    for (uint32_t t = 0; t < nt; t++) {
        TypeBuild b;
        b.t = t, b.capacity = caps[t];
        make_type_records(ctx, d, sp.types[t], b);
        if ((st = pack_keys_take_window(ctx, sp.types[t], b))) return st;
        if ((st = take_segment_slot(ctx, sp, h, d, b))) return st;
        if ((st = choose_segment_path(ctx, sp, d, b))) return st;
        if ((st = alloc_type_buffers(ctx, sp, d, caps, b))) return st;
        if ((st = upload_segment_zeroed(ctx, b.si))) return st;
    }
    if ((st = build_emit_records(ctx, sp, d, carry_serial))) return st;
    if ((st = mark_virtual_parents(ctx, sp, d))) return st;
    sp.initialized = true;
    return context_follow_ups(ctx);
}

fw_status release_spawner_segments(fw_ctx *ctx, SpawnerHost &sp) {
    drop_forecast_and_boxes(ctx);
    ctx->tab_force = true;
    for (int i = 0; i < kSnapRing; i++) ctx->snap_pending[i] = false;  // rows in flight describe the old segments
    for (const EmissionHost &e : sp.em) {
        if (!e.assigned) continue;  // a build that failed half-way
        ctx->free_emits.push_back(e.emit_idx);
        ctx->free_emit_slots.push_back(e.emit_slot);
    }
    sp.em.clear();
    hipError_t e = hipSuccess;  // (the release goes on: the first failure is reported at the end)
    for (uint32_t si : sp.seg) {
        if (si == kNoSeg) continue;
        SegHost &S = ctx->segs[si];
        if (!S.in_use) continue;
        ctx->free_types.push_back(S.type_idx);
        if (S.keys_cap) ctx->free_keys.push_back({S.keys_off, S.keys_cap});
        if (S.range) ctx->r_force = true;
        if (S.small) ctx->small_dirty = true;
        ctx->big_dirty = true;
        {
            SegPathEdit edit(ctx, S);
            S = SegHost{};  // (releases its buffers)
        }
        ctx->census.segment_released(ctx->range_few);
        const uint32_t zero = 0;
        for (int r = 0; r < 2 && e == hipSuccess; r++) e = hipMemcpy(ctx->g.count + (size_t)r * ctx->max_seg + si, &zero, 4, hipMemcpyHostToDevice);
    }
    sp.seg.clear();
    update_small_mode(ctx);
    if (e != hipSuccess) return fail(ctx, FW_EHIP, std::string("hipMemcpy(live count of a released segment): ") + hipGetErrorString(e));
    return FW_OK;
}


}  // namespace fwh
