// fw_engine_api.cpp -- the C ABI of include/firework_hip.h other than fw_step (+ the debug hooks of firework_hip_debug.h)
// (host engine of libfirework_hip.so: fw_engine.h lists its translation units; there is no CPU simulation path in this library)
#include "fw_engine.h"

thread_local std::string fwh::g_create_error;  // (fw_last_error(nullptr): per calling thread, like errno)

// Is `p` inside a mapping of this process that the host may write?  (The runtime reserves the device's address range in the host's
// address space whether or not the memory behind an address is reachable through the BAR: a reserved-only page is mapped PROT_NONE,
// and a store to it would be a SIGSEGV, not an error code -- so the page's permissions are read from /proc/self/maps, once, when a
// context is created.)
static bool host_maps_writable(const void *p) {
    FILE *f = fopen("/proc/self/maps", "r");
    if (!f) return false;
    char line[512];
    bool ok = false;
    const unsigned long long a = (unsigned long long)(uintptr_t)p;
    while (fgets(line, sizeof line, f)) {
        unsigned long long lo = 0, hi = 0;
        char perms[8] = {0};
        if (sscanf(line, "%llx-%llx %7s", &lo, &hi, perms) == 3 && a >= lo && a < hi) {
            ok = perms[0] == 'r' && perms[1] == 'w';
            break;
        }
    }
    fclose(f);
    return ok;
}

// the streams, events and buffers of a new context (fw_ctx_create: knobs read); a failure leaves them to ~fw_ctx
static fw_status create_resources(fw_ctx *ctx, hipStream_t stream) {
    if (stream)
        ctx->stream.borrow(stream);
    else
        FW_HIP(ctx, ctx->stream.create());
    FW_HIP(ctx, ctx->copy_stream.create());
    FW_HIP(ctx, ctx->fifo_stream.create());
    for (HipEvent *ev : {&ctx->ev_side, &ctx->ev_main}) FW_HIP(ctx, ev->create());
    for (int i = 0; i < kParamRing; i++) FW_HIP(ctx, ctx->ev_copied[i].create());
    fw_status st;
    if ((st = alloc_buf(ctx, ctx->h_done, 8, Mem::pinned, true))) return st;
    ctx->h_err = ctx->h_done + 4, ctx->g.err_host = ctx->h_err;
    if ((st = alloc_buf(ctx, ctx->gm.err, 16, Mem::device, true, &ctx->g.err)) ||
        (st = alloc_buf(ctx, ctx->gm.stats, FW_STAT_SLOTS, Mem::device, true, &ctx->g.stats)) ||
        (st = alloc_buf(ctx, ctx->d_aabb, 256 * 8)) || (st = alloc_buf(ctx, ctx->d_total, 8)))
        return st;
    for (int i = 0; i < kParamRing && ctx->param_bar; i++)
        if ((st = alloc_buf(ctx, ctx->b_param[i], kBarParamBytes, Mem::fine))) return st;
    return ensure_max_seg(ctx, 1024);
}

fw_ctx::~fw_ctx() {
    // (work in flight may still use what the members release)
    for (hipStream_t s : {(hipStream_t)stream, (hipStream_t)copy_stream, (hipStream_t)fifo_stream})
        if (s) (void)hipStreamSynchronize(s);
}

// What the entry points that read or write a spawner's particles open with: the spawner, the call's own argument check (args_ok,
// which may look at the spawner), the sticky status of a poisoned one, the device -- and then what the call needs before it touches
// particle state: nothing (it enqueues behind what is in flight), sync(ctx), join_side(ctx) or read_counts(ctx, r.c).  begin_call
// returns false when the call ends there, with r.st; otherwise r.st is FW_OK or, after Then::counts alone, FW_ECAPACITY (a type
// overflowed: the call goes on and reports it at its end, unless a later error takes precedence).
// Ages: whether the call reads or copies particles.  Ages::write -- a ring under the age rule gets its ages written back first
// (ensure_ages; nothing where none is stale).  Ages::leave -- the call looks at counts, records or last_emitted planes only: a stale
// age plane stays stale, and a host that polls every frame keeps the rule.  Ages::ages -- the call reads positions, ages and what
// derives from them, never rotation or angular velocity (fw_spawner_aabb, what a culling host calls every frame): the ages are
// written back, a deferred spin (ensure_spin) stays deferred.  Ages::write replays that too.
enum class Then { nothing, sync, join, counts };
enum class Ages { leave, ages, write };
struct SpawnerCall {
    SpawnerHost *sp = nullptr;
    std::vector<uint32_t> c;  // per segment (Then::counts)
    fw_status st = FW_OK;
};
template <typename ArgsOk>
static bool begin_call(fw_ctx *ctx, fw_spawner h, SpawnerCall &r, Then then, Ages ages, ArgsOk args_ok) {
    r.sp = get_spawner(ctx, h);
    if (!r.sp || !args_ok(*r.sp)) return r.st = FW_EINVAL, false;
    if (poll_device_error(ctx), r.sp->poisoned) return r.st = poisoned_status(ctx), false;
    hipSetDevice(ctx->device);
    if ((r.st = flush_withheld(ctx))) return false;  // (a withheld frame goes to the stream before anybody looks: fw_ctx::withheld)
    for (size_t t = 0; ages != Ages::leave && t < r.sp->seg.size(); t++)
        if ((ages == Ages::write && (r.st = ensure_spin(ctx, r.sp->seg[t]))) || (r.st = ensure_ages(ctx, r.sp->seg[t]))) return false;
    r.st = then == Then::sync ? sync(ctx) : then == Then::join ? join_side(ctx) : then == Then::counts ? read_counts(ctx, r.c) : FW_OK;
    return !r.st || (then == Then::counts && r.st == FW_ECAPACITY);
}

// Everything enqueued on top of a poisoned spawner's invalid state has finished (the caller synchronised): what those frames
// reported again is not news, and the segment slots the report names are about to be reused or released.  (But the word may by now
// name ANOTHER spawner, healthy so far -- one word, the last writer wins: mark it before the report is dropped)
static fw_status clear_poison_report(fw_ctx *ctx) {
    poll_device_error(ctx);
    ctx->h_err[0] = ctx->h_err[1] = 0ull;
    const uint32_t zero = 0;
    FW_HIP(ctx, hipMemcpy(ctx->g.err, &zero, sizeof zero, hipMemcpyHostToDevice));
    return FW_OK;
}

static void recount_poisoned(fw_ctx *ctx) {  // (fw_step looks for invalid spawners only while some exist)
    ctx->n_poisoned = 0;
    for (const SpawnerHost &x : ctx->spawners) ctx->n_poisoned += (x.alive && x.poisoned) ? 1u : 0u;
}

// the batch setters' handle array: every handle names a live spawner, or nothing is set (msg: the setter's own text)
static fw_status check_handles(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const char *msg) {
    for (uint32_t i = 0; i < n; i++)
        if (!get_spawner(ctx, handles[i])) return fail(ctx, FW_EINVAL, msg);
    return FW_OK;
}

// the last_emitted_age plane a segment keeps for an emission entry; -1: none, the entry never reads it
static int lplane_of(const SegHost &S, uint32_t emission_index) {
    int plane = -1;
    for (uint32_t k = 0; k < S.n_lplanes; k++)
        if (S.lplane_emission[k] == (int32_t)emission_index) plane = (int)k;
    return plane;
}

// the running total of particles that entered update_particles: the sum of the stat slots (the caller synchronised)
static fw_status read_stat_total(fw_ctx *ctx, uint64_t *total) {
    unsigned long long slots[FW_STAT_SLOTS];
    FW_HIP(ctx, hipMemcpy(slots, ctx->g.stats, sizeof slots, hipMemcpyDeviceToHost));
    *total = 0;
    for (unsigned long long v : slots) *total += v;
    return FW_OK;
}

extern "C" {


int fw_abi_version(void) { return FW_ABI_VERSION; }

const char *fw_last_error(const fw_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

uint64_t fw_compute_emission_count(float t, float last, float dur, float start, float end, float per_cycle,
                                   float *next_last) {
    float nl = 0.f;
    const uint64_t n = fw_emission_count(t, last, dur, start, end, per_cycle, &nl);
    if (next_last) *next_last = nl;
    return n;
}

fw_status fw_ctx_create(int device, uint32_t seed, void *stream, fw_ctx **out) {
    if (!out) return FW_EINVAL;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("no HIP device available (") + hipGetErrorString(e) +
                         "); this backend has no CPU fallback";
        return FW_ENODEV;
    }
    if (device < 0 || device >= ndev) {
        g_create_error = "device index out of range";
        return FW_EINVAL;
    }
    if ((e = hipSetDevice(device)) != hipSuccess) {
        g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return FW_ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("kernels are built for gfx950 only; device is ") + prop.gcnArchName;
        return FW_ENODEV;
    }
    fw_ctx *ctx = new fw_ctx();
    ctx->device = device;
    ctx->seed = seed;
    // A/B and debugging switches (firework_hip_debug.h): read only when FW_ENABLE_KNOBS=1 -- a product process does not change
    // behaviour because of a stray environment variable
    const char *knobs_on = getenv("FW_ENABLE_KNOBS");
    auto getenv = [&](const char *name) -> const char * { return (knobs_on && atoi(knobs_on) != 0) ? ::getenv(name) : nullptr; };
#ifdef FW_AB
    if (const char *m = getenv("FW_FAIL_ALLOC")) ctx->fail_alloc = strtoull(m, nullptr, 10);
#endif
    {  // fw_ctx::param_bar: device memory the host can write (large BAR) -- asked of the runtime, then tried once
        int large_bar = 0;
        HipBuf<char> probe;
        if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, device) == hipSuccess && large_bar != 0 &&
            alloc_buf(ctx, probe, 4096, Mem::fine) == FW_OK) {
            hipPointerAttribute_t at{};
            ctx->param_bar = hipPointerGetAttributes(&at, probe) == hipSuccess && at.type == hipMemoryTypeDevice && host_maps_writable(probe);
        }
        (void)hipGetLastError();
        ctx->err.clear();  // (no BAR memory is no error)
    }
    ctx->g.seed = seed;
    // -- path selectors: every one of them names a path the product takes by itself under some workload; the tests force each
    if (const char *m = getenv("FW_UPDATE_MODE")) ctx->update_mode = !strcmp(m, "split") ? FW_MODE_SPLIT : FW_MODE_FUSED;
    if (const char *m = getenv("FW_FORECAST")) ctx->use_forecast = atoi(m) != 0;
    if (const char *m = getenv("FW_TF")) ctx->use_tf = atoi(m) != 0;
    if (const char *m = getenv("FW_TF_MIN_TILES")) ctx->tf_min_tiles = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_STREAM")) ctx->use_stream = atoi(m) != 0;
    if (const char *m = getenv("FW_STATIC_NEW")) ctx->use_static_new = atoi(m) != 0;  // 0: always count + look back
    if (const char *m = getenv("FW_SPIN_LIMIT")) ctx->spin_limit = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_FIFO")) ctx->use_fifo = atoi(m) != 0;
    if (const char *m = getenv("FW_FIFO_MIN")) ctx->fifo_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_FIFO_SMALL")) ctx->fifo_small_tiles = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_FIFO_STREAM")) ctx->use_fifo_stream = atoi(m) != 0;
    if (const char *m = getenv("FW_RANGE")) ctx->use_range = atoi(m) != 0;
    if (const char *m = getenv("FW_RANGE_MIN")) ctx->range_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_RANGE_FEW")) ctx->range_few = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_RANGE_SMALL")) ctx->range_small_tiles = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_RANGE_YOUNG_BIG")) ctx->range_young_big = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_NOSPIN")) ctx->use_nospin = atoi(m) != 0;
    if (const char *m = getenv("FW_AXIS_SPIN")) ctx->use_axis = atoi(m) != 0;
    if (const char *m = getenv("FW_AGELESS")) ctx->use_ageless = atoi(m) != 0;
    if (const char *m = getenv("FW_SPIN_DEFER")) ctx->use_spin_defer = atoi(m) != 0;
    if (const char *m = getenv("FW_SPIN_DEFER_MIN")) ctx->spin_defer_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_SPIN_DEFER_AFTER")) ctx->spin_defer_after = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_SPIN_LOG")) ctx->spin_log_cap = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_SPINLESS")) ctx->use_spinless = atoi(m) != 0;
    if (const char *m = getenv("FW_WHOLE_TILES")) ctx->use_whole_tiles = atoi(m) != 0;
    if (const char *m = getenv("FW_NEWBORN_SPIN")) ctx->newborn_spin = atoi(m) != 0;
    if (const char *m = getenv("FW_FUSE2")) ctx->use_fuse2 = atoi(m) != 0;
    if (const char *m = getenv("FW_FUSE2_MIN")) ctx->fuse2_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_FUSE_DEPTH")) ctx->fuse_depth = (uint32_t)std::min(std::max(atoi(m), 2), (int)FW_FUSE_MAX);
    if (const char *m = getenv("FW_FUSE_DEEP_MIN")) ctx->fuse_deep_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_FUSE_WIDE_MIN")) ctx->fuse_wide_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_FUSE_FAR_DEPTH")) ctx->fuse_far_depth = (uint32_t)std::min(std::max(atoi(m), (int)FW_FUSE_MAX), (int)FW_FUSE_FAR);
    if (const char *m = getenv("FW_FUSE_FAR_MIN")) ctx->fuse_far_min = (uint32_t)strtoul(m, nullptr, 10);
    // 0: scale / colour planes always stored; 1: not stored for types with an attached instance buffer; 2 (default): for no type
    if (const char *m = getenv("FW_DERIVED")) ctx->use_derived = atoi(m) != 0, ctx->derive_all = atoi(m) >= 2;
    if (const char *m = getenv("FW_NEST_FUSE")) ctx->nest_fuse = atoi(m) != 0;
    if (const char *m = getenv("FW_SMALL")) ctx->use_small = atoi(m) != 0;
    if (const char *m = getenv("FW_SMALL_MAX")) ctx->small_max = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_SMALL_MIN")) ctx->small_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_WIDE_MAX")) ctx->wide_max = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_WIDE_MIN")) ctx->wide_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_WIDE_MID")) ctx->wide_mid = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_WAVE_ALL_MIN")) ctx->wave_all_min = (uint32_t)strtoul(m, nullptr, 10);
    if (const char *m = getenv("FW_HOST_FAST")) ctx->host_fast = atoi(m) != 0;
    if (const char *m = getenv("FW_PARAM_BAR")) ctx->param_bar = ctx->param_bar && atoi(m) != 0;
    if (const char *m = getenv("FW_NT_MB")) ctx->nt_bytes = (uint64_t)atoll(m) << 20;
    if (const char *m = getenv("FW_NT_WO_MB")) ctx->nt_wo_bytes = ctx->nt_wo_bytes_range = (uint64_t)atoll(m) << 20;
#ifdef FW_AB
    // -- the experiment surface: only in the `make ab` build (libfirework_hip_ab.so; the tools load it through FW_LIB_PATH)
    if (const char *m = getenv("FW_DEBUG")) ctx->dbg = (uint32_t)atoi(m);
    if (const char *m = getenv("FW_FIFO_NESTED")) ctx->fifo_nested = atoi(m) != 0;
    if (const char *m = getenv("FW_RANGE_SPREAD_NEW")) ctx->range_spread_new = atoi(m) != 0;
    if (const char *m = getenv("FW_AABB")) ctx->track_aabb = atoi(m) != 0;  // same as fw_ctx_track_aabbs(ctx, 1)
    ctx->trace = getenv("FW_TRACE") != nullptr;
    if (const char *m = getenv("FW_HOST_PROF")) ctx->host_prof = atoi(m) != 0, ctx->host_prof_skip = atoi(m) > 1 ? (uint64_t)atoi(m) : 0;
#endif
    if (create_resources(ctx, (hipStream_t)stream) != FW_OK) {
        g_create_error = ctx->err;
        delete ctx;
        return FW_EHIP;
    }
    *out = ctx;
    return FW_OK;
}

fw_status fw_ctx_destroy(fw_ctx *ctx) {
    if (!ctx) return FW_EINVAL;
    hipSetDevice(ctx->device);
    drop_withheld(ctx);  // (a withheld frame goes with the particles)
    if (ctx->host_prof && ctx->prof_frames) {
        static const char *names[10] = {"windows+reset", "spawner loop", "tile table", "commit", "args", "op tables", "launch", "post", "", ""};
        fprintf(stderr, "[fw] host half of fw_step over %llu frames (ns per frame):", (unsigned long long)ctx->prof_frames);
        for (int i = 0; i < 8; i++) fprintf(stderr, "  %s %.0f", names[i], ctx->prof_ns[i] / (double)ctx->prof_frames);
        fprintf(stderr, "\n[fw] table uploads: general %llu, range %llu over %llu frames\n", (unsigned long long)ctx->tab_seq,
                (unsigned long long)ctx->r_uploads, (unsigned long long)ctx->frame);
        fprintf(stderr, "[fw] host records: SegHost %zu B, SpawnerHost %zu B (entry at %zu), EmissionHost %zu B, FwOp %zu B\n", sizeof(SegHost),
                sizeof(SpawnerHost), (size_t)((const char *)&ctx->spawners.data()->em.one_ - (const char *)ctx->spawners.data()),
                sizeof(EmissionHost), sizeof(FwOp));
    }
    delete ctx;
    return FW_OK;
}

void *fw_ctx_stream(const fw_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

fw_status fw_ctx_synchronize(fw_ctx *ctx) {
    if (!ctx) return FW_EINVAL;
    fw_status st = sync(ctx);
    if (st) return st;
    return check_device_errors(ctx);
}

// An fw_collider as the device reads it (fw_collide.h: FwCollider) -- a member of the collider world (fw_ctx_set_colliders) or a volume
// (fw_ctx_count_in_volumes)
static bool collider_kind_ok(const fw_collider &c) { return c.kind >= FW_COLLIDER_PLANE && c.kind <= FW_COLLIDER_CAPSULE; }
static FwCollider collider_record(const fw_collider &c) {
    FwCollider d{};
    d.kind = c.kind, d.layers = c.layers, d.radius = c.radius;
    // (the sphere around `position` that contains it: a wave skips a collider none of its rays can reach, fw_cast_ray)
    d.bound = c.kind == FW_COLLIDER_SPHERE ? c.radius
              : c.kind == FW_COLLIDER_BOX ? std::sqrt(c.half_extents[0] * c.half_extents[0] + c.half_extents[1] * c.half_extents[1] + c.half_extents[2] * c.half_extents[2]) * 1.0001f
              : (c.kind == FW_COLLIDER_CYLINDER || c.kind == FW_COLLIDER_CONE) ? std::sqrt(c.radius * c.radius + c.half_extents[1] * c.half_extents[1]) * 1.0001f  // (the rim of a cap / of the base)
              : c.kind == FW_COLLIDER_CAPSULE ? (c.half_extents[1] + c.radius) * 1.0001f  // (the poles of the caps)
                            : INFINITY;
    if (!(d.bound >= 0.0f)) d.bound = INFINITY;  // (NaN / negative extents: never skipped)
    memcpy(d.position, c.position, sizeof c.position);
    memcpy(d.rotation, c.rotation, sizeof c.rotation);
    memcpy(d.normal, c.normal, sizeof c.normal);
    memcpy(d.half_extents, c.half_extents, sizeof c.half_extents);
    return d;
}

fw_status fw_ctx_set_colliders(fw_ctx *ctx, const fw_collider *colliders, uint32_t n) {
    if (!ctx || (n && !colliders)) return fail(ctx, FW_EINVAL, "bad collider set");
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    for (uint32_t i = 0; i < n; i++)
        if (!collider_kind_ok(colliders[i])) return fail(ctx, FW_EINVAL, "unknown collider kind");
    // The reference asks the live physics world every frame (core.rs:756-765): a set that changes every frame must not
    // stall the frames in flight.  The new set is staged in pinned memory and copied by the stream itself.
    // (the wait of take: for the copy of two sets ago, long done unless the caller replaces the set in a tight loop)
    const size_t ncap = std::max<size_t>(64, (size_t)n * 2);
    FwCollider *h;
    fw_status st = ctx->h_coll.take(ctx, n, ncap, &h);
    if (st) return st;
    if (n > ctx->d_colliders.cap()) {  // a larger world than ever before: the one case that waits (kernels in flight read the old table)
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->d_colliders, ncap, Mem::device, false, &ctx->g.colliders))) return st;
    }
    for (uint32_t i = 0; i < n; i++) h[i] = collider_record(colliders[i]);
    if (n) {
        FW_HIP(ctx, hipMemcpyAsync(ctx->d_colliders, h, n * sizeof(FwCollider), hipMemcpyHostToDevice, ctx->stream));
        if ((st = ctx->h_coll.commit(ctx, ctx->stream))) return st;
    }
    ctx->n_colliders = n;
    ctx->g.n_colliders = n;
    drop_forecast_and_boxes(ctx);
    return FW_OK;
}

fw_status fw_spawner_create(fw_ctx *ctx, const fw_spawner_desc *desc, fw_spawner *out) {
    if (!ctx || !out) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = validate_desc(ctx, desc);
    if (st) return st;
    if ((st = sync(ctx))) return st;
    int h = -1;
    for (size_t i = 0; i < ctx->spawners.size(); i++)
        if (!ctx->spawners[i].alive) {
            h = (int)i;
            break;
        }
    if (h < 0) {
        ctx->spawners.push_back(SpawnerHost{});
        h = (int)ctx->spawners.size() - 1;
    }
    ctx->spawners[h] = SpawnerHost{};
    ctx->spawners[h].alive = true;
    st = build_spawner(ctx, h, desc, nullptr);
    if (st) {
        release_spawner_segments(ctx, ctx->spawners[h]);
        ctx->spawners[h].alive = false;
        return st;
    }
    *out = h;
    return FW_OK;
}

fw_status fw_spawner_update_settings(fw_ctx *ctx, fw_spawner h, const fw_spawner_desc *desc) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = validate_desc(ctx, desc);
    if (st) return st;
    if ((st = sync(ctx))) return st;
    if (sp->poisoned && (st = clear_poison_report(ctx))) return st;
    // RNG streams never replay: carry the serials of surviving emission indices
    std::vector<uint64_t> serials;
    for (const EmissionHost &e : sp->em) {
        unsigned long long s = e.serial;
        if (e.es.mode == FW_MODE_NESTED)
            hipMemcpy(&s, ctx->d_emit_serial + e.emit_slot, sizeof s, hipMemcpyDeviceToHost);
        serials.push_back(s);
    }
    // (no ensure_spin / ensure_ages here: the spawner's particles are dropped with its segments, and build_spawner starts every SegHost --
    // its spin log and cohorts included -- from SegHost{}: nothing is left that a deferred spin could be replayed into)
    if ((st = release_spawner_segments(ctx, *sp))) return st;
    const bool finished_notified = sp->finished_notified;
    SpawnerHost keep = *sp;
    *sp = SpawnerHost{};
    sp->alive = true;
    sp->manual_queued_count = keep.manual_queued_count;
    memcpy(sp->origin_pos, keep.origin_pos, sizeof keep.origin_pos);
    memcpy(sp->origin_rot, keep.origin_rot, sizeof keep.origin_rot);
    memcpy(sp->parent_vel, keep.parent_vel, sizeof keep.parent_vel);
    sp->mod_scale = keep.mod_scale, sp->mod_speed = keep.mod_speed;
    sp->no_rings = keep.no_rings || keep.poisoned;  // (rebuilt after an internal error: compacting path only from now on)
    st = build_spawner(ctx, h, desc, &serials);
    if (st) {
        // the old particle types are gone and the new ones could not be built: the handle dies (every later call on
        // it returns FW_EINVAL) instead of pointing at segments that do not exist
        const std::string why = ctx->err;
        release_spawner_segments(ctx, ctx->spawners[h]);
        ctx->spawners[h] = SpawnerHost{};
        ctx->err = why + " (spawner destroyed: its settings could not be rebuilt)";
        return st;
    }
    ctx->spawners[h].finished_notified = finished_notified;
    recount_poisoned(ctx);
    return st;
}

fw_status fw_spawner_destroy(fw_ctx *ctx, fw_spawner h) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = sync(ctx);
    if (st) return st;
    if (sp->poisoned && (st = clear_poison_report(ctx))) return st;
    if ((st = release_spawner_segments(ctx, *sp))) return st;
    *sp = SpawnerHost{};
    recount_poisoned(ctx);
    return FW_OK;
}

fw_status fw_spawner_set_origin(fw_ctx *ctx, fw_spawner h, const float t[3], const float r[4]) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp || !t || !r) return FW_EINVAL;
    memcpy(sp->origin_pos, t, sizeof sp->origin_pos);
    memcpy(sp->origin_rot, r, sizeof sp->origin_rot);
    return FW_OK;
}

fw_status fw_ctx_set_origins(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const float *translations,
                             const float *rotations_xyzw) {
    if (!ctx || (n && (!handles || !translations || !rotations_xyzw))) return FW_EINVAL;
    if (fw_status st = check_handles(ctx, n, handles, "fw_ctx_set_origins: invalid spawner handle")) return st;
    for (uint32_t i = 0; i < n; i++) {
        SpawnerHost &sp = ctx->spawners[(size_t)handles[i]];
        memcpy(sp.origin_pos, translations + (size_t)i * 3, sizeof sp.origin_pos);
        memcpy(sp.origin_rot, rotations_xyzw + (size_t)i * 4, sizeof sp.origin_rot);
    }
    return FW_OK;
}

fw_status fw_spawner_set_parent_velocity(fw_ctx *ctx, fw_spawner h, const float v[3]) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp || !v) return FW_EINVAL;
    memcpy(sp->parent_vel, v, sizeof sp->parent_vel);
    return FW_OK;
}

fw_status fw_spawner_set_modifier(fw_ctx *ctx, fw_spawner h, float scale, float speed) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp) return FW_EINVAL;
    sp->mod_scale = scale, sp->mod_speed = speed;
    return FW_OK;
}

fw_status fw_spawner_queue(fw_ctx *ctx, fw_spawner h, uint64_t count) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp) return FW_EINVAL;
    sp->manual_queued_count += count;  // core.rs:284-286
    return FW_OK;
}

fw_status fw_ctx_set_parent_velocities(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const float *velocities) {
    if (!ctx || (n && (!handles || !velocities))) return FW_EINVAL;
    if (fw_status st = check_handles(ctx, n, handles, "fw_ctx_set_parent_velocities: invalid spawner handle")) return st;
    for (uint32_t i = 0; i < n; i++) memcpy(ctx->spawners[(size_t)handles[i]].parent_vel, velocities + (size_t)i * 3, 3 * sizeof(float));
    return FW_OK;
}

fw_status fw_ctx_set_modifiers(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const float *scales, const float *speeds) {
    if (!ctx || (n && (!handles || !scales || !speeds))) return FW_EINVAL;
    if (fw_status st = check_handles(ctx, n, handles, "fw_ctx_set_modifiers: invalid spawner handle")) return st;
    for (uint32_t i = 0; i < n; i++) {
        SpawnerHost &sp = ctx->spawners[(size_t)handles[i]];
        sp.mod_scale = scales[i], sp.mod_speed = speeds[i];
    }
    return FW_OK;
}

fw_status fw_ctx_queue(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const uint64_t *counts) {
    if (!ctx || (n && (!handles || !counts))) return FW_EINVAL;
    if (fw_status st = check_handles(ctx, n, handles, "fw_ctx_queue: invalid spawner handle")) return st;
    for (uint32_t i = 0; i < n; i++) ctx->spawners[(size_t)handles[i]].manual_queued_count += counts[i];  // core.rs:284-286
    return FW_OK;
}

// ---- outputs -----------------------------------------------------------------------------
fw_status fw_spawner_counts(fw_ctx *ctx, fw_spawner h, uint32_t *per_type, uint32_t n_types) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::leave, [&](const SpawnerHost &) { return per_type != nullptr; })) return r.st;
    for (uint32_t t = 0; t < n_types && t < r.sp->seg.size(); t++) per_type[t] = r.c[r.sp->seg[t]];
    return r.st;
}

fw_status fw_spawner_active(fw_ctx *ctx, fw_spawner h, int32_t *out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::leave, [&](const SpawnerHost &) { return out != nullptr; })) return r.st;
    *out = spawner_active(ctx, *r.sp, r.c) ? 1 : 0;
    return r.st;
}

fw_status fw_spawner_poll_finished(fw_ctx *ctx, fw_spawner h, int32_t *out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::leave, [&](const SpawnerHost &) { return out != nullptr; })) return r.st;
    bool all_empty = true;
    for (uint32_t si : r.sp->seg) all_empty &= r.c[si] == 0;
    *out = 0;
    if (all_empty && !spawner_active(ctx, *r.sp, r.c) && r.sp->initialized && !r.sp->finished_notified) {  // core.rs:679-686
        r.sp->finished_notified = true;
        *out = 1;
    }
    return r.st;
}

static fw_status stage_buffer(fw_ctx *ctx, size_t bytes, void **out) {
    if (bytes > ctx->d_stage.cap()) {
        const size_t nb = (std::max<size_t>(bytes + bytes / 4, (size_t)1 << 20) + 65535u) & ~(size_t)65535u;
        fw_status st;
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->d_stage, nb))) return st;
    }
    *out = ctx->d_stage;
    return FW_OK;
}

// the first min(n, cap) particles of a segment as fw_particle records, through the staging buffer
static fw_status read_records(fw_ctx *ctx, const FwSegView &v, uint32_t n, int32_t pbr, fw_particle *out, uint64_t cap) {
    const uint64_t m = std::min<uint64_t>(n, cap);
    if (!m || !out) return FW_OK;
    void *tmp = nullptr;
    fw_status st = stage_buffer(ctx, m * sizeof(fw_particle), &tmp);
    if (st) return st;
    hipError_t e = fw_launch_gather(ctx->stream, v, (uint32_t)m, pbr, tmp);
    // (the copy goes through the stream the kernel ran on, then one wait for both)
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, m * sizeof(fw_particle), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    FW_HIP(ctx, e);
    return FW_OK;
}

fw_status fw_spawner_read_particles(fw_ctx *ctx, fw_spawner h, uint32_t type, fw_particle *out, uint64_t cap,
                                    uint64_t *n_out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::write, [&](const SpawnerHost &sp) { return type < sp.seg.size(); })) return r.st;
    const uint32_t n = r.c[r.sp->seg[type]];
    if (n_out) *n_out = n;
    // (the counts are exact and the stream has been waited for: the host places particle 0 itself)
    fw_status st2 = read_records(ctx, seg_view_exact(ctx, r.sp->seg[type], ctx->parity, n), n, r.sp->types[type].ps.pbr, out, cap);
    return st2 ? st2 : r.st;
}

fw_status fw_spawner_read_last_emitted(fw_ctx *ctx, fw_spawner h, uint32_t type, uint32_t emission_index, float *out,
                                       uint64_t cap, uint64_t *n_out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::leave, [&](const SpawnerHost &sp) { return type < sp.seg.size() && emission_index < sp.em.size(); })) return r.st;
    const SegHost &S = ctx->segs[r.sp->seg[type]];
    const uint32_t n = r.c[r.sp->seg[type]];
    if (n_out) *n_out = n;
    const uint64_t m = std::min<uint64_t>(n, cap);
    if (!m || !out) return r.st;
    const int plane = lplane_of(S, emission_index);
    if (plane < 0) {
        for (uint64_t i = 0; i < m; i++) out[i] = FW_F32_MIN;  // never touched: still vec![f32::MIN; n] (core.rs:467)
        return r.st;
    }
    const char *pl = S.buf[ctx->parity] + FW_OFF_L((size_t)S.capacity, plane);
    const uint32_t h0 = ring_head_exact(S, n);  // a ring: from the head to the end of the buffer, then from slot 0
    const uint64_t m1 = std::min<uint64_t>(m, S.capacity - h0);
    FW_HIP(ctx, hipMemcpy(out, pl + (size_t)h0 * sizeof(float), m1 * sizeof(float), hipMemcpyDeviceToHost));
    if (m > m1) FW_HIP(ctx, hipMemcpy(out + m1, pl, (m - m1) * sizeof(float), hipMemcpyDeviceToHost));
    return r.st;
}

fw_status fw_spawner_write_particles(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_particle *in, uint64_t n) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::sync, Ages::write, [&](const SpawnerHost &sp) { return type < sp.seg.size() && !(n && !in) && n <= 0xF0000000ull; }))
        return r.st;
    fw_status st;
    const uint32_t si = r.sp->seg[type];
    drop_forecast_and_boxes(ctx);
    if ((st = fifo_to_general(ctx, si))) return st;  // ages and lifetimes will be whatever the caller writes
    leave_small(ctx, ctx->segs[si]);                  // (any number of particles, any colours: the compacting kernels take it from here)
    if ((st = leave_nospin(ctx, si))) return st;      // ... and so will rotations and angular velocities
    ctx->segs[si].axis = 0;                           // (... about any axis: the axis-spin rule is void for good)
    // ... and scales and colours: the planes are stored and read again until every particle has been through an update
    // (an attached buffer keeps receiving records; the mode comes back after the next step)
    if ((st = set_derived(ctx, si, false, false))) return st;
    ctx->segs[si].derive_pending = wants_derived(ctx, ctx->segs[si]);
    if (n > ctx->segs[si].capacity) {
        ctx->segs[si].ub = 0;
        const uint32_t zero = 0;
        FW_HIP(ctx, hipMemcpy(count_slot(ctx, si), &zero, 4, hipMemcpyHostToDevice));
        if ((st = grow_segment(ctx, si, (uint32_t)n))) return st;
    }
    SegHost &S = ctx->segs[si];
    if (n) {
        void *tmp = nullptr;
        if ((st = stage_buffer(ctx, n * sizeof(fw_particle), &tmp))) return st;
        hipError_t e = hipMemcpyAsync(tmp, in, n * sizeof(fw_particle), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = fw_launch_scatter(ctx->stream, S.buf[ctx->parity], S.capacity, (uint32_t)n, S.n_lplanes, tmp);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        FW_HIP(ctx, e);
    }
    const uint32_t n32 = (uint32_t)n;
    FW_HIP(ctx, hipMemcpy(count_slot(ctx, si), &n32, 4, hipMemcpyHostToDevice));
    S.ub = n32;
    S.win_ok = false;  // ages and lifetimes are now whatever the caller wrote
    S.colors_dirty = true, ctx->colors_dirty = true;  // and so are the colours: the next update writes them all
    for (int i = 0; i < kSnapRing; i++) ctx->snap_pending[i] = false;
    return FW_OK;
}

fw_status fw_spawner_write_last_emitted(fw_ctx *ctx, fw_spawner h, uint32_t type, uint32_t emission_index,
                                        const float *in, uint64_t n) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::sync, Ages::leave, [&](const SpawnerHost &sp) { return type < sp.seg.size() && emission_index < sp.em.size() && !(n && !in); }))
        return r.st;
    if (fw_status st = fifo_to_general(ctx, r.sp->seg[type])) return st;  // (caller-written state: the general path takes over)
    const SegHost &S = ctx->segs[r.sp->seg[type]];
    const int plane = lplane_of(S, emission_index);
    if (plane < 0) return FW_OK;  // entry never reads it
    const uint64_t m = std::min<uint64_t>(n, S.capacity);
    if (m)
        FW_HIP(ctx, hipMemcpy(S.buf[ctx->parity] + FW_OFF_L((size_t)S.capacity, plane), in, m * sizeof(float),
                              hipMemcpyHostToDevice));
    return FW_OK;
}

fw_status fw_spawner_read_destroyed(fw_ctx *ctx, fw_spawner h, uint32_t type, fw_particle *out, uint64_t cap,
                                    uint64_t *n_out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::sync, Ages::leave, [&](const SpawnerHost &sp) { return type < sp.seg.size(); })) return r.st;
    const SegHost &S = ctx->segs[r.sp->seg[type]];
    uint32_t n = 0;
    if (S.destroyed) FW_HIP(ctx, hipMemcpy(&n, ctx->g.ndestroyed + r.sp->seg[type], 4, hipMemcpyDeviceToHost));
    if (n_out) *n_out = n;
    // (a range ring fills its records from the END of the buffer, the youngest dead first: the last n are in list order)
    const char *first = S.destroyed + (S.dead_at_end && n <= S.capacity ? (size_t)(S.capacity - n) * sizeof(fw_particle) : (size_t)0);
    // (the update wrote them as fw_particle records: a plain copy)
    const uint64_t m = std::min<uint64_t>(n, cap);
    if (m && out) FW_HIP(ctx, hipMemcpy(out, first, m * sizeof(fw_particle), hipMemcpyDeviceToHost));
    return FW_OK;
}

fw_status fw_spawner_pack_instances_device(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap,
                                           uint64_t *n_upper_bound) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::nothing, Ages::write, [&](const SpawnerHost &sp) { return type < sp.seg.size() && d_out; })) return r.st;
    const uint32_t si = r.sp->seg[type];
    const SegHost &S = ctx->segs[si];
    const uint32_t ub = (uint32_t)std::min<uint64_t>(S.nested_fed ? S.capacity : std::min(S.ub, S.capacity), cap);
    if (n_upper_bound) *n_upper_bound = ub;
    if (S.fifo || S.small) {  // (whose launches may run on the ring stream)
        fw_status jst = join_side(ctx);
        if (jst) return jst;
    }
    // (no synchronisation: the kernel reads the count -- and a range ring's old part -- from the device)
    FW_HIP(ctx, fw_launch_pack_instances(ctx->stream, seg_view(ctx, si, ctx->parity), count_slot(ctx, si), ub, d_out));
    return FW_OK;
}

static fw_status attach_instances(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap, bool window) {
    SpawnerCall r;  // (Then::sync: kernels in flight hold the old record)
    if (!begin_call(ctx, h, r, Then::sync, Ages::write, [&](const SpawnerHost &sp) { return type < sp.seg.size() && !(d_out && !cap); })) return r.st;
    SpawnerHost *const sp = r.sp;
    // ... and whatever the caller enqueued on ITS streams to initialise the buffer has happened before a frame writes to it
    // (the context's streams are non-blocking ones: nothing else orders them against, say, a fill on the null stream)
    if (d_out) FW_HIP(ctx, hipDeviceSynchronize());
    fw_status st;
    if (d_out && !window && ctx->segs[sp->seg[type]].range) {
        // records at index `list position` counted from 0: a tile of a range ring only knows that once the whole old part
        // has been counted -- such a type continues on the compacting path (the windowed attach keeps it a ring)
        if ((st = fifo_to_general(ctx, sp->seg[type]))) return st;
    }
    SegHost &S = ctx->segs[sp->seg[type]];
    // (a small type keeps its kernel: fw_k_update_small<INST> writes the records of its survivors itself)
    {
        SegPathEdit edit(ctx, S);
        S.inst = (char *)d_out;
    }
    S.inst_cap = d_out ? (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull) : 0u;
    S.inst_window = d_out != nullptr && window;
    if (S.range) ctx->r_force = true;  // (the range descriptors carry FW_TYPE_IDX_NOLIFE: derived AND no buffer attached)
    // the records carry scale and colours from now on: the update stops storing the three planes that would duplicate them
    // (every reader of those planes evaluates them instead, so a buffer smaller than the live count loses nothing either);
    // colliding types stay as they are (the feature path)
    const bool derive = wants_derived(ctx, S);
    S.derive_pending = derive && S.colors_dirty;  // (particles written by the caller, not updated yet: one frame later)
    if ((st = set_derived(ctx, sp->seg[type], derive && !S.colors_dirty))) return st;
    return upload_seg(ctx, sp->seg[type]);
}

fw_status fw_spawner_attach_instances(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap) {
    return attach_instances(ctx, h, type, d_out, cap, false);
}

fw_status fw_spawner_attach_instances_window(fw_ctx *ctx, fw_spawner h, uint32_t type, void *d_out, uint64_t cap) {
    return attach_instances(ctx, h, type, d_out, cap, true);
}

fw_status fw_spawner_instance_window(fw_ctx *ctx, fw_spawner h, uint32_t type, uint64_t *first, uint64_t *count) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::leave, [&](const SpawnerHost &sp) { return type < sp.seg.size() && first && count; })) return r.st;
    const uint32_t si = r.sp->seg[type];
    const SegHost &S = ctx->segs[si];
    uint32_t dead = 0;
    // a range ring's update numbers its records from the particles it destroys (fw_k_update_range): they sit behind them
    if (S.dead_at_end && S.inst_window) FW_HIP(ctx, hipMemcpy(&dead, ctx->g.ndestroyed + si, 4, hipMemcpyDeviceToHost));
    *first = dead, *count = r.c[si];
    return r.st;
}

fw_status fw_spawner_pack_instances(fw_ctx *ctx, fw_spawner h, uint32_t type, fw_particle_instance *out, uint64_t cap,
                                    uint64_t *n_out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::write, [&](const SpawnerHost &sp) { return type < sp.seg.size(); })) return r.st;
    const uint32_t n = r.c[r.sp->seg[type]];
    if (n_out) *n_out = n;
    const uint64_t m = std::min<uint64_t>(n, cap);
    if (!m || !out) return r.st;
    void *tmp = nullptr;
    fw_status sst = stage_buffer(ctx, m * sizeof(fw_particle_instance), &tmp);
    if (sst) return sst;
    uint64_t ub = 0;
    fw_status st2 = fw_spawner_pack_instances_device(ctx, h, type, tmp, m, &ub);
    hipError_t e = hipMemcpyAsync(out, tmp, m * sizeof(fw_particle_instance), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    FW_HIP(ctx, e);
    return st2 ? st2 : r.st;
}

// ---- depth-sorted records (firework_hip.h: DEPTH-SORTED INSTANCES; fw_sort.h, fw_k_sort.hip)
static_assert(sizeof(fw_sort_view) == 32 && sizeof(FwSortView) == sizeof(fw_sort_view), "fw_sort_view: 32 bytes, mirrored by FwSortView");
static bool sort_view_ok(const fw_sort_view *view) { return view && view->order <= FW_SORT_FRONT_TO_BACK && view->reserved == 0u; }

// The two device forms: fw_spawner_pack_instances_device's prologue, then keys -> sort -> (records: the gather; order: the sorted
// indices straight into d_out), all on the context's stream.  An order reads positions only, which no launch defers: Ages::leave.
static fw_status sorted_device(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, void *d_out, uint64_t cap, uint64_t *n_upper_bound,
                               bool records) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::nothing, records ? Ages::write : Ages::leave,
                    [&](const SpawnerHost &sp) { return type < sp.seg.size() && d_out && sort_view_ok(view); }))
        return r.st;
    const uint32_t si = r.sp->seg[type];
    const SegHost &S = ctx->segs[si];
    const uint32_t ub = (uint32_t)std::min<uint64_t>(S.nested_fed ? S.capacity : std::min(S.ub, S.capacity), cap);
    const size_t words = fw_sort_scratch_words(ub);
    if (words > ctx->d_sort.cap()) {  // more than any call before: the one case that waits (launches in flight may use the old scratch)
        fw_status st;
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->d_sort, (words + words / 4 + 16383u) & ~(size_t)16383u))) return st;
    }
    if (n_upper_bound) *n_upper_bound = ub;
    if (S.fifo || S.small) {  // (whose launches may run on the ring stream)
        fw_status jst = join_side(ctx);
        if (jst) return jst;
    }
    FwSortView sv;
    memcpy(&sv, view, sizeof sv);
    const FwSegView v = seg_view(ctx, si, ctx->parity);
    uint32_t *const scratch = ctx->d_sort;
    // (no synchronisation: every launch reads the count -- and a range ring's old part -- from the device)
    FW_HIP(ctx, fw_launch_depth_keys(ctx->stream, v, count_slot(ctx, si), ub, sv, scratch, scratch + ub));
    FW_HIP(ctx, fw_launch_sort_pairs(ctx->stream, count_slot(ctx, si), ub, scratch, records ? nullptr : (uint32_t *)d_out));
    if (records) FW_HIP(ctx, fw_launch_pack_instances_sorted(ctx->stream, v, count_slot(ctx, si), ub, scratch + ub, d_out));
    return FW_OK;
}

fw_status fw_ctx_depth_order_device(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, void *d_order, uint64_t cap,
                                    uint64_t *n_upper_bound) {
    return sorted_device(ctx, h, type, view, d_order, cap, n_upper_bound, false);
}

fw_status fw_ctx_pack_instances_sorted_device(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, void *d_out, uint64_t cap,
                                              uint64_t *n_upper_bound) {
    return sorted_device(ctx, h, type, view, d_out, cap, n_upper_bound, true);
}

fw_status fw_ctx_pack_instances_sorted(fw_ctx *ctx, fw_spawner h, uint32_t type, const fw_sort_view *view, fw_particle_instance *out, uint64_t cap,
                                       uint64_t *n_out) {
    SpawnerCall r;
    if (!begin_call(ctx, h, r, Then::counts, Ages::write, [&](const SpawnerHost &sp) { return type < sp.seg.size() && sort_view_ok(view); })) return r.st;
    const uint32_t n = r.c[r.sp->seg[type]];
    if (n_out) *n_out = n;
    const uint64_t m = std::min<uint64_t>(n, cap);
    if (!m || !out) return r.st;
    void *tmp = nullptr;
    fw_status st = stage_buffer(ctx, m * sizeof(fw_particle_instance), &tmp);
    if (st) return st;
    uint64_t ub = 0;
    if ((st = sorted_device(ctx, h, type, view, tmp, m, &ub, true))) return st;
    hipError_t e = hipMemcpyAsync(out, tmp, m * sizeof(fw_particle_instance), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    FW_HIP(ctx, e);
    return r.st;
}

fw_status fw_spawner_aabb(fw_ctx *ctx, fw_spawner h, float out_min[3], float out_max[3], int32_t *any) {
    SpawnerCall call;  // (Then::join: the query kernels run on the main stream and may read rings)
    if (!begin_call(ctx, h, call, Then::join, Ages::ages, [&](const SpawnerHost &) { return out_min && out_max; })) return call.st;
    const SpawnerHost *const sp = call.sp;
    if (!ctx->h_aabb)
        if (fw_status st = alloc_buf(ctx, ctx->h_aabb, 8, Mem::pinned)) return st;
    // the query kernels take up to eight particle types at a time (their segment list rides in the kernel arguments): a
    // spawner with more is answered in chunks, folded here -- min / max are exact and order-independent
    const size_t nt = sp->seg.size();
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    bool got = false;
    fw_status keep = FW_OK;
    for (size_t t0 = 0; t0 < nt || t0 == 0; t0 += 8) {
        const uint32_t n = (uint32_t)std::min<size_t>(8, nt - std::min(nt, t0));
        if (!n) break;
        bool any_ring = false;  // rings (and types a wave / workgroup of fw_k_update_small updates) leave no per-tile boxes: the two-pass query reads them
        FwSegView views[8];
        for (uint32_t t = 0; t < n; t++) {
            const SegHost &S = ctx->segs[sp->seg[t0 + t]];
            any_ring |= S.ring() || S.small;
            views[t] = seg_view(ctx, sp->seg[t0 + t], ctx->parity);
        }
        if (ctx->boxes_epoch && ctx->d_tile_first && !any_ring) {
            // the last update left the box of every tile's survivors (fw_ctx_track_aabbs): fold those -- one small launch
            FW_HIP(ctx, fw_launch_aabb_from_tiles(ctx->stream, ctx->g, sp->seg.data() + t0, n, ctx->parity, ctx->boxes_epoch,
                                                  ctx->d_tile_first, ctx->h_aabb));
        } else {
            // two launches over the particles, the result lands in pinned memory: one synchronisation, no copies
            FW_HIP(ctx, fw_launch_aabb(ctx->stream, ctx->g, sp->seg.data() + t0, views, n, ctx->parity, ctx->d_aabb, ctx->h_aabb));
        }
        fw_status st = sync(ctx);
        if (!st) st = check_device_errors(ctx);
        if (st && st != FW_ECAPACITY) return st;
        if (st) keep = st;
        const volatile float *r = ctx->h_aabb;
        if (r[3] != 0.0f) {
            for (int c = 0; c < 3; c++) {
                mn[c] = got ? std::min(mn[c], (float)r[c]) : (float)r[c];
                mx[c] = got ? std::max(mx[c], (float)r[4 + c]) : (float)r[4 + c];
            }
            got = true;
        } else if (!got && t0 + 8 >= nt) {  // nothing anywhere: report the last chunk's (empty) box as before
            for (int c = 0; c < 3; c++) mn[c] = r[c], mx[c] = r[4 + c];
        }
    }
    if (any) *any = got ? 1 : 0;
    for (int c = 0; c < 3; c++) out_min[c] = mn[c], out_max[c] = mx[c];
    return keep;
}

fw_status fw_ctx_track_aabbs(fw_ctx *ctx, int32_t enable) {
    if (!ctx) return FW_EINVAL;
    ctx->track_aabb = enable != 0;
    if (!enable) ctx->boxes_epoch = 0;
    // (per-tile boxes are left by the compacting kernels' tiles; rings and small types are answered by the two-pass query)
    return FW_OK;
}

// ---- the boxes of many spawners in one call (firework_hip.h: BATCHED BOXES; fw_boxes.h, fw_k_boxes / fw_k_boxes_fold)
static_assert(sizeof(fw_aabb) == 32 && sizeof(FwBoxPlace) == 16 && sizeof(FwBoxEntry) % 16 == 0, "fw_aabb: 32 bytes; the two tables share one 16-byte aligned copy");

// What the batched boxes and the volume queries share, behind their argument checks (n > 0, every place names a live spawner and, unless
// its type is -1 -- every particle type of the spawner --, one of its types): fw_spawner_aabb's prologue for the whole list at once -- a
// withheld group goes out once, with `ages` (Ages::ages) stale ages are written back, a deferred spin stays deferred either way, the side
// stream is joined once where a listed segment's launches may run there --, then one entry per listed (spawner, type) segment and one
// place per list position into the staging slot of this turn, with room for `extra` bytes behind them (16-byte aligned: whatever else
// the call sends along in the same copy), and the plan.  Host work per listed segment, none per particle; nothing is enqueued but what the
// prologue flushes.
struct ListedPlan {
    char *h = nullptr, *d = nullptr;        // the staging slot of this turn, the device table it feeds
    size_t bytes = 0, places = 0, extra = 0;  // of the slot in all; where the places and the extra bytes start
    uint32_t entries = 0;
    uint64_t chunks = 0;
};
// (the list: `places`, or -- null -- every type of handles[i])
static fw_status plan_listed(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const fw_volume_place *places, bool ages, size_t extra, const char *who,
                             ListedPlan *out) {
    const auto at = [&](uint32_t i) { return places ? places[i] : fw_volume_place{handles[i], -1}; };
    poll_device_error(ctx);
    size_t ne = 0;
    for (uint32_t i = 0; i < n; i++) {
        const fw_volume_place pl = at(i);
        const SpawnerHost &sp = ctx->spawners[(size_t)pl.spawner];
        if (sp.poisoned) return poisoned_status(ctx);
        ne += pl.type < 0 ? sp.seg.size() : 1u;
    }
    if (n > FW_BOX_MAX_CHUNKS || ne > 0xFFFFFFFFull) return fail(ctx, FW_EINVAL, std::string(who) + ": more places than one batch holds");
    hipSetDevice(ctx->device);
    fw_status st;
    if ((st = flush_withheld(ctx))) return st;  // (fw_ctx::withheld)
    // the listed segments of place i, in type order
    const auto each_seg = [&](uint32_t i, auto &&f) -> fw_status {
        const fw_volume_place pl = at(i);
        const std::vector<uint32_t> &seg = ctx->spawners[(size_t)pl.spawner].seg;
        for (size_t t = pl.type < 0 ? 0 : (size_t)pl.type, t1 = pl.type < 0 ? seg.size() : t + 1; t < t1; t++)
            if (fw_status fst = f(seg[t])) return fst;
        return FW_OK;
    };
    bool side = false;  // a listed segment is a FIFO ring or a small type: its launches may run on the ring stream
    for (uint32_t i = 0; i < n; i++)
        if ((st = each_seg(i, [&](uint32_t si) -> fw_status {
                side |= ctx->segs[si].fifo || ctx->segs[si].small;
                return ages ? ensure_ages(ctx, si) : FW_OK;
            })))
            return st;
    if (side && (st = join_side(ctx))) return st;
    out->places = ne * sizeof(FwBoxEntry), out->extra = out->places + (size_t)n * sizeof(FwBoxPlace), out->bytes = out->extra + extra;
    if ((st = ctx->boxes.h_tab.take(ctx, out->bytes, std::max<size_t>(out->bytes * 2, 16384), &out->h, &ctx->boxes.d_tab))) return st;
    out->d = ctx->boxes.d_tab;
    FwBoxEntry *const tab = reinterpret_cast<FwBoxEntry *>(out->h);
    std::vector<uint32_t> &first = ctx->boxes.place_first;
    try {
        first.resize((size_t)n + 1);
    } catch (const std::bad_alloc &) {
        return fail(ctx, FW_ENOMEM, std::string(who) + ": out of host memory");
    }
    uint32_t e = 0;
    for (uint32_t i = 0; i < n; i++) {
        first[i] = e;
        (void)each_seg(i, [&](uint32_t si) -> fw_status {
            const SegHost &S = ctx->segs[si];
            FwBoxEntry &E = tab[e++];
            E.v = seg_view(ctx, si, ctx->parity), E.d_count = count_slot(ctx, si);
            E.bound = S.nested_fed ? S.capacity : std::min(S.ub, S.capacity);  // (the bound of fw_spawner_pack_instances_device)
            E.chunk0 = 0;
            return FW_OK;
        });
    }
    first[n] = e;
    out->entries = e;
    out->chunks = fw_boxes_plan(tab, e, first.data(), n, reinterpret_cast<FwBoxPlace *>(out->h + out->places));
    if (out->chunks > FW_BOX_MAX_CHUNKS) return fail(ctx, FW_EINVAL, std::string(who) + ": more particles than one batch holds");
    return FW_OK;
}

// The batched boxes behind plan_listed: every handle a place of all its types, ages written back; ONE copy, two launches; `records`: n
// fw_aabb records the fold kernel writes, device or pinned host memory.  Waits only to grow.
static fw_status boxes_enqueue(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, void *records, const char *who) {
    ListedPlan P;
    fw_status st;
    if ((st = plan_listed(ctx, n, handles, nullptr, true, 0, who, &P))) return st;
    const uint64_t total = P.chunks;
    if (total * 8 > ctx->boxes.d_part.cap()) {  // more than any call before: the one case that waits (launches in flight may use the old scratch)
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->boxes.d_part, (size_t)((total + total / 4 + 1023u) & ~1023ull) * 8))) return st;
    }
    FW_HIP(ctx, hipMemcpyAsync(P.d, P.h, P.bytes, hipMemcpyHostToDevice, ctx->stream));
    uint32_t launches = 0;
    // (no synchronisation: the kernels read every count -- and a range ring's old part -- from the device)
    const hipError_t le = fw_launch_boxes(ctx->stream, reinterpret_cast<const FwBoxEntry *>(P.d), P.entries, reinterpret_cast<const FwBoxPlace *>(P.d + P.places), n,
                                          (uint32_t)total, ctx->boxes.d_part, records, &launches);
    ctx->boxes.launches += launches, ctx->boxes.last_chunks = total;
    if ((st = ctx->boxes.h_tab.commit(ctx, ctx->stream))) return st;  // (behind the kernels: they read the device table the slot fed)
    FW_HIP(ctx, le);
    return FW_OK;
}

static fw_status boxes_args(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, const void *out, const char *bad_handle) {
    if (!ctx || (n && (!handles || !out))) return FW_EINVAL;
    return check_handles(ctx, n, handles, bad_handle);
}

fw_status fw_ctx_aabbs(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, fw_aabb *out) {
    if (fw_status st = boxes_args(ctx, n, handles, out, "fw_ctx_aabbs: invalid spawner handle")) return st;
    if (!n) return FW_OK;
    fw_status st;
    if ((size_t)n * 8 > ctx->boxes.h_out.cap()) {  // (nothing of an earlier call may still be on its way into the old records)
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->boxes.h_out, std::max<size_t>(64, (size_t)n * 2) * 8, Mem::pinned))) return st;
    }
    if ((st = boxes_enqueue(ctx, n, handles, ctx->boxes.h_out.get(), "fw_ctx_aabbs"))) return st;
    // the records land in pinned memory: one synchronisation for the whole batch, then a host copy
    st = sync(ctx);
    if (!st) st = check_device_errors(ctx);
    if (st && st != FW_ECAPACITY) return st;
    memcpy(out, ctx->boxes.h_out.get(), (size_t)n * sizeof(fw_aabb));
    return st;
}

fw_status fw_ctx_aabbs_device(fw_ctx *ctx, uint32_t n, const fw_spawner *handles, void *d_out) {
    if (fw_status st = boxes_args(ctx, n, handles, d_out, "fw_ctx_aabbs_device: invalid spawner handle")) return st;
    if (n && (reinterpret_cast<uintptr_t>(d_out) & 15u)) return fail(ctx, FW_EINVAL, "fw_ctx_aabbs_device: d_out is not 16-byte aligned");
    if (!n) return FW_OK;
    return boxes_enqueue(ctx, n, handles, d_out, "fw_ctx_aabbs_device");
}

// ---- the particles inside analytic volumes (firework_hip.h: VOLUME QUERIES; fw_volumes.h, fw_k_volumes / fw_k_volumes_fold)
static_assert(sizeof(fw_volume_place) == 8 && sizeof(FwCollider) % 16 == 0, "fw_volume_place: 8 bytes; the volume records ride behind the two tables in one 16-byte aligned copy");

// The arguments of both forms: FW_OK with *none set where there is nothing to answer
static fw_status volumes_args(fw_ctx *ctx, uint32_t n_places, const fw_volume_place *places, uint32_t n_volumes, const fw_collider *volumes, const void *out,
                              bool *none) {
    if (!ctx) return FW_EINVAL;
    *none = !n_places || !n_volumes;
    if (*none) return FW_OK;
    if (!places || !volumes || !out) return fail(ctx, FW_EINVAL, "fw_ctx_count_in_volumes: null places, volumes or output");
    if ((uint64_t)n_places * n_volumes > FW_VOLUME_MAX_ANSWERS) return fail(ctx, FW_EINVAL, "fw_ctx_count_in_volumes: more than FW_VOLUME_MAX_ANSWERS answers");
    for (uint32_t i = 0; i < n_places; i++) {
        const SpawnerHost *sp = get_spawner(ctx, places[i].spawner);
        if (!sp) return fail(ctx, FW_EINVAL, "fw_ctx_count_in_volumes: invalid spawner handle");
        if (places[i].type < -1 || (places[i].type >= 0 && (size_t)places[i].type >= sp->seg.size()))
            return fail(ctx, FW_EINVAL, "fw_ctx_count_in_volumes: no such particle type");
    }
    for (uint32_t i = 0; i < n_volumes; i++)
        if (!collider_kind_ok(volumes[i])) return fail(ctx, FW_EINVAL, "fw_ctx_count_in_volumes: unknown volume kind");
    return FW_OK;
}

// Both forms behind plan_listed, WITHOUT the age step -- the kernels read positions only: stale ages stay stale --: the volume records
// converted into the slot behind the two tables, ONE copy, two launches; `counts`: n_places * n_volumes uint32 the fold kernel writes,
// device or pinned host memory.  Waits only to grow the scratch (chunks * volumes words) or the tables.
static fw_status volumes_enqueue(fw_ctx *ctx, uint32_t n_places, const fw_volume_place *places, uint32_t n_volumes, const fw_collider *volumes, void *counts) {
    ListedPlan P;
    fw_status st;
    if ((st = plan_listed(ctx, n_places, nullptr, places, false, (size_t)n_volumes * sizeof(FwCollider), "fw_ctx_count_in_volumes", &P))) return st;
    FwCollider *const rec = reinterpret_cast<FwCollider *>(P.h + P.extra);
    for (uint32_t i = 0; i < n_volumes; i++) rec[i] = collider_record(volumes[i]);
    const uint64_t words = P.chunks * n_volumes;
    if (words > ctx->volumes.d_part.cap()) {  // more than any call before: the one case that waits (launches in flight may use the old scratch)
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->volumes.d_part, (size_t)((words + words / 4 + 1023u) & ~1023ull)))) return st;
    }
    FW_HIP(ctx, hipMemcpyAsync(P.d, P.h, P.bytes, hipMemcpyHostToDevice, ctx->stream));
    uint32_t launches = 0;
    // (no synchronisation: the kernels read every count -- and a range ring's old part -- from the device)
    const hipError_t le = fw_launch_volumes(ctx->stream, reinterpret_cast<const FwBoxEntry *>(P.d), P.entries, reinterpret_cast<const FwBoxPlace *>(P.d + P.places), n_places,
                                            (uint32_t)P.chunks, reinterpret_cast<const FwCollider *>(P.d + P.extra), n_volumes, ctx->volumes.d_part, counts, &launches);
    ctx->volumes.launches += launches, ctx->volumes.last_chunks = P.chunks;
    if ((st = ctx->boxes.h_tab.commit(ctx, ctx->stream))) return st;  // (behind the kernels: they read the device table the slot fed)
    FW_HIP(ctx, le);
    return FW_OK;
}

fw_status fw_ctx_count_in_volumes(fw_ctx *ctx, uint32_t n_places, const fw_volume_place *places, uint32_t n_volumes, const fw_collider *volumes, uint32_t *out) {
    bool none;
    fw_status st = volumes_args(ctx, n_places, places, n_volumes, volumes, out, &none);
    if (st || none) return st;
    const size_t n = (size_t)n_places * n_volumes;
    if (n > ctx->volumes.h_out.cap()) {  // (nothing of an earlier call may still be on its way into the old words)
        if ((st = sync(ctx)) || (st = alloc_buf(ctx, ctx->volumes.h_out, std::max<size_t>(256, n * 2), Mem::pinned))) return st;
    }
    if ((st = volumes_enqueue(ctx, n_places, places, n_volumes, volumes, ctx->volumes.h_out.get()))) return st;
    // the counts land in pinned memory: one synchronisation for the whole call, then a host copy
    st = sync(ctx);
    if (!st) st = check_device_errors(ctx);
    if (st && st != FW_ECAPACITY) return st;
    memcpy(out, ctx->volumes.h_out.get(), n * sizeof(uint32_t));
    return st;
}

fw_status fw_ctx_count_in_volumes_device(fw_ctx *ctx, uint32_t n_places, const fw_volume_place *places, uint32_t n_volumes, const fw_collider *volumes, void *d_out) {
    bool none;
    const fw_status st = volumes_args(ctx, n_places, places, n_volumes, volumes, d_out, &none);
    if (st || none) return st;
    if (reinterpret_cast<uintptr_t>(d_out) & 3u) return fail(ctx, FW_EINVAL, "fw_ctx_count_in_volumes_device: d_out is not 4-byte aligned");
    return volumes_enqueue(ctx, n_places, places, n_volumes, volumes, d_out);
}

fw_status fw_ctx_live_count(fw_ctx *ctx, uint64_t *out) {
    if (!ctx || !out) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    std::vector<uint32_t> c;
    fw_status st = read_counts(ctx, c);
    if (st && st != FW_ECAPACITY) return st;
    uint64_t t = 0;
    for (size_t i = 0; i < c.size(); i++)
        if (ctx->segs[i].in_use) t += c[i];
    *out = t;
    return st;
}

fw_status fw_ctx_live_count_device(fw_ctx *ctx, void *d_out_u64) {
    if (!ctx || !d_out_u64) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status jst = join_side(ctx);  // the counts of ring segments are written by the side stream's launches
    if (jst) return jst;
    FW_HIP(ctx, fw_launch_total(ctx->stream, count_slot(ctx), (uint32_t)ctx->segs.size(), (unsigned long long *)d_out_u64));
    return FW_OK;
}

fw_status fw_ctx_live_count_ring(fw_ctx *ctx, void *d_ring_u64, uint32_t n_slots) {
    if (!ctx || (d_ring_u64 && n_slots < 2)) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = sync(ctx);
    if (!st && d_ring_u64) FW_HIP(ctx, hipDeviceSynchronize());  // (the caller's zero-fill of the ring, on whatever stream)
    if (st) return st;
    ctx->live_ring = (unsigned long long *)d_ring_u64;
    ctx->live_ring_n = d_ring_u64 ? n_slots : 0;
    ctx->live_ring_frames = 0;
    if (d_ring_u64) FW_HIP(ctx, fw_memset_done(d_ring_u64, 0, (size_t)n_slots * sizeof(unsigned long long)));
    return FW_OK;
}

fw_status fw_ctx_last_step_updated(fw_ctx *ctx, uint64_t *out) {
    if (!ctx || !out) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = sync(ctx);
    if (st) return st;
    return read_stat_total(ctx, out);
}

fw_status fw_ctx_kernel_timing(fw_ctx *ctx, int32_t enable) {
    if (!ctx) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = sync(ctx);
    if (st) return st;
    if (enable && ctx->tev.empty()) {
        std::vector<HipEvent> tev(kTimingEvents);
        for (HipEvent &ev : tev) FW_HIP(ctx, ev.create(hipEventDefault));
        ctx->tev = std::move(tev);
    }
    if (enable) {
        // for reference only: what an empty hipEventRecord pair on the stream costs (the timed launches do not use
        // marker packets: their events are attached to the dispatch, see fw_launch_update)
        const int n = 64;
        for (int i = 0; i < n; i++) {
            FW_HIP(ctx, hipEventRecord(ctx->tev[2 * i], ctx->stream));
            FW_HIP(ctx, hipEventRecord(ctx->tev[2 * i + 1], ctx->stream));
        }
        FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
        double tot = 0;
        for (int i = 8; i < n; i++) {
            float t = 0;
            FW_HIP(ctx, hipEventElapsedTime(&t, ctx->tev[2 * i], ctx->tev[2 * i + 1]));
            tot += t;
        }
        ctx->tev_overhead_ms = tot / (n - 8);
    }
    ctx->timing = enable != 0;
    ctx->tev_used = 0, ctx->tev_frames = 0;
    return read_stat_total(ctx, &ctx->timing_particles_start);
}

fw_status fw_ctx_kernel_timing_read(fw_ctx *ctx, double *ms_total, uint64_t *launches, uint64_t *particles) {
    if (!ctx) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    fw_status st = sync(ctx);
    if (st) return st;
    double ms = 0;
    for (size_t i = 0; i + 1 < ctx->tev_used; i += 2) {
        float t = 0;
        FW_HIP(ctx, hipEventElapsedTime(&t, ctx->tev[i], ctx->tev[i + 1]));
        ms += t;
    }
    const uint64_t nl = ctx->tev_frames;  // frames: a frame's update may be several launches (FIFO + general), all summed
    if (ms_total) *ms_total = ms;
    if (launches) *launches = nl;
    uint64_t now = 0;
    if ((st = read_stat_total(ctx, &now))) return st;
    if (particles) *particles = now - ctx->timing_particles_start;
    return FW_OK;
}

// profiling hook (not in the public header): per-tile timestamps of the last update (and, with `prev`, of the one
// before it: the two are kept apart by launch parity) when FW_DEBUG & 8
fw_status fw_debug_read_timestamps2(fw_ctx *ctx, unsigned long long *out, unsigned long long *prev, uint64_t max_tiles,
                                    uint64_t *n_tiles) {
    if (!ctx || !ctx->g.dbg_ts) return FW_EINVAL;
    fw_status st = sync(ctx);
    if (st) return st;
    const uint64_t n = std::min<uint64_t>(max_tiles, ctx->total_tiles_dev);
    if (n_tiles) *n_tiles = n;
    const uint32_t last = (uint32_t)(ctx->frame & 1u);  // epoch of the last launch = frame (after the increment)
    const size_t stride = (size_t)ctx->total_tiles_dev * 8;
    if (n && out)
        FW_HIP(ctx, hipMemcpy(out, ctx->g.dbg_ts + 32768 + last * stride, n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (n && prev)
        FW_HIP(ctx, hipMemcpy(prev, ctx->g.dbg_ts + 32768 + (last ^ 1u) * stride, n * 8 * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost));
    return FW_OK;
}
// ... and of the last range-ring launch: 8 words per workgroup {start, 0, 0, end of wave 0, role_k, segment, 0, 0}
fw_status fw_debug_read_range_timestamps(fw_ctx *ctx, unsigned long long *out, uint64_t max_tiles, uint64_t *n_tiles) {
    if (!ctx || !ctx->d_rts) return FW_EINVAL;
    fw_status st = sync(ctx);
    if (st) return st;
    const uint64_t n = std::min<uint64_t>(max_tiles, ctx->r_total);
    if (n_tiles) *n_tiles = n;
    if (n && out) FW_HIP(ctx, hipMemcpy(out, ctx->d_rts, n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FW_OK;
}
// {~earliest workgroup start [64], latest workgroup end [64]} of the last 256 update launches (slot = epoch & 255);
// *epoch = the last launch's.  out512: room for 32768 words.
fw_status fw_debug_read_launches(fw_ctx *ctx, unsigned long long *out512, uint32_t *epoch) {
    if (!ctx || !ctx->g.dbg_ts || !out512) return FW_EINVAL;
    fw_status st = sync(ctx);
    if (st) return st;
    FW_HIP(ctx, hipMemcpy(out512, ctx->g.dbg_ts, 32768 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (epoch) *epoch = ctx->frame ? frame_epoch(ctx->frame - 1) : 0u;
    return FW_OK;
}
// which update path a particle type is on: *mode = 1 FIFO ring (in place), 0 general (compacting); *moved_bytes = the
// bytes one update of a live particle reads and writes on that path; *algorithmic_bytes = the part of them that carries
// state the update needs or changes (SURVEY.md 8(d)'s convention: a float4 plane rewritten for three changed components
// moves 4 bytes -- initial_scale, lifetime -- that are not algorithmic)
fw_status fw_debug_update_path(fw_ctx *ctx, fw_spawner h, uint32_t type, int32_t *mode, uint32_t *moved_bytes,
                               uint32_t *algorithmic_bytes) {
    SpawnerHost *sp = get_spawner(ctx, h);
    if (!sp || type >= sp->seg.size()) return FW_EINVAL;
    const SegHost &S = ctx->segs[sp->seg[type]];
    const TypeHost &T = sp->types[type];
    if (mode) *mode = S.fifo ? 1 : (S.range ? 2 : (S.small ? ((S.wide && !ctx->wave_all_on) ? 4 : 3) : 0));
    const uint32_t colours = (T.base.kind != 0 ? 16u : 0u) + (T.emis.kind != 0 ? 16u : 0u);  // one-key gradients: never rewritten
    uint32_t moved, algo;
    if (S.ring()) {
        // in place: position+age and velocity always; rotation only where some emitter makes the particles spin (or the
        // type accelerates them), angular velocity only if it then changes; scale unless its curve is constant
        bool spins = false;
        for (const EmissionHost &E : sp->em)
            if ((uint32_t)E.es.particle_index == type)
                spins |= !(E.es.initial_angular_velocity.magnitude.min == 0.f && E.es.initial_angular_velocity.magnitude.max == 0.f);
        const float *aa = T.ps.angular_acceleration;
        const bool acc = aa[0] != 0.f || aa[1] != 0.f || aa[2] != 0.f;
        const uint32_t q2 = (spins || acc) ? 16u : 0u, q3 = ((spins && T.ps.angular_drag != 0.f) || acc) ? 16u : 0u;
        // (a type that cannot turn: neither the rotation nor the angular-velocity / lifetime plane is read)
        // (round 6: Q1 / Q3 are component planes -- velocity and angular velocity move as 12 bytes each way, the constants that
        // shared their float4, initial_scale and lifetime, stay where they are: every byte moved is algorithmic)
        moved = (S.nospin ? 28u : 56u) + 28u + q2 + (q3 ? 12u : 0u) + (T.scale.kind != 0 ? 4u : 0u) + colours;
        // (round 12, a FIFO ring under the axis-spin rule -- SegHost::axis: of rotation and angular velocity only the axis' component
        // and the rotation's w move: 8 + 4 bytes in, 8 out, 4 more where the drag changes the angular velocity.  The figure of a
        // frame whose dt the rule covers; the range kernel loads every plane.)
        if (S.fifo && S.axis != 0u) moved = 28u + 12u + 28u + (spins ? 8u : 0u) + (q3 ? 4u : 0u) + (T.scale.kind != 0 ? 4u : 0u) + colours;
        // (round 18, a FIFO ring whose latest launch ran under the age rule -- SegHost::ageless_last: the age plane moved neither way)
        if (S.fifo && S.ageless_last) moved -= 8u;
        // (round 19, ... and deferred its spin -- SegHost::spin_last: of rotation and angular velocity nothing moved either way)
        if (S.fifo && S.spin_last && S.axis != 0u) moved -= 12u + (spins ? 8u : 0u) + (q3 ? 4u : 0u);
        algo = moved;
        // (a range ring: the part of the list that may lose particles, a fifth of configs[2], is compacted in place and reads and
        // rewrites every plane it keeps, the 4-byte lifetime included: the figure is the young part's)
        // (initial_scale -- and in a range ring the lifetime -- are read where somebody evaluates the scale: a type whose planes are
        // stored, an attached instance buffer.  Otherwise the young tile at the boundary to the old part alone reads the lifetimes, for the
        // consistency check: FW_TYPE_IDX_NOLIFE)
        if (!S.derived || S.inst != nullptr) moved += S.range ? 8u : 4u, algo += S.range ? 8u : 4u;
    } else {
        // compacting: every state plane lands at a new slot (+ the last_emitted planes of a Nested parent, read and written);
        // a type that cannot turn keeps no rotation plane: -16 B read, -16 B written,
        // ... and its lifetimes in a 4-byte plane instead of Q3: -32 B again, +4 B read, +4 B written
        moved = 64u + 64u + 4u + colours + 8u * S.n_lplanes - (S.nospin ? 32u + 32u - 8u : 0u);
        algo = moved - 8u;
    }
    if (S.derived) {  // scale and colour planes are not stored (the instance record carries them: +64 B written per particle)
        const uint32_t skipped = colours + ((S.ring() && T.scale.kind == 0) ? 0u : 4u);
        moved -= std::min(moved, skipped), algo -= std::min(algo, skipped);
    }
    // an attached instance buffer: the update also writes the 64-byte ParticleInstance record of every survivor (render.rs:95-103)
    if (S.inst != nullptr) moved += 64u, algo += 64u;
    // (rounds 22 and 23, a FIFO ring whose latest launch ran several frames of it -- SegHost::fuse_last, never with an instance buffer: one
    // load and one store of every plane the launch moves for that many updates of the particle)
    if (S.fifo && S.fuse_last >= 2u) moved /= S.fuse_last, algo /= S.fuse_last;
    if (moved_bytes) *moved_bytes = moved;
    if (algorithmic_bytes) *algorithmic_bytes = algo;
    return FW_OK;
}
// frames with Nested entries so far: those whose entries ran inside the FIFO launch (FwFifoNest) / those that ran the separate
// fw_k_spawn / fw_k_nest passes
fw_status fw_debug_nest_frames(fw_ctx *ctx, uint64_t *fused, uint64_t *separate) {
    if (!ctx) return FW_EINVAL;
    if (fused) *fused = ctx->fused_nest_frames;
    if (separate) *separate = ctx->nest_pass_frames;
    return FW_OK;
}
fw_status fw_debug_tile_scratch(fw_ctx *ctx, uint64_t *table_tiles, uint64_t *scratch_tiles) {
    if (!ctx) return FW_EINVAL;
    if (table_tiles) *table_tiles = ctx->total_tiles_dev;
    if (scratch_tiles) *scratch_tiles = ctx->tiles_cap;
    return FW_OK;
}
fw_status fw_debug_recovered_rings(fw_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return FW_EINVAL;
    *n = ctx->recovered_rings;
    return FW_OK;
}
// launches of fw_k_fifo_ages so far (ensure_ages: a ring under the age rule had its ages written back)
fw_status fw_debug_age_launches(fw_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return FW_EINVAL;
    *n = ctx->age_tab.launches;
    return FW_OK;
}
// launches of fw_k_fifo_spin so far (ensure_spin: a ring whose spin was deferred had its log replayed)
fw_status fw_debug_spin_launches(fw_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return FW_EINVAL;
    *n = ctx->spin_tab.launches;
    return FW_OK;
}
// FIFO launches so far that ran a SPINLESS form of fw_k_update_fifo (launch_fifo: FwFifoArgs::spinless)
fw_status fw_debug_spinless_launches(fw_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return FW_EINVAL;
    *n = ctx->spinless_launches;
    return FW_OK;
}
// spin-less FIFO launches so far in which the host's evaluation of fw_fifo_tile_whole found a whole ring tile, and those tiles
fw_status fw_debug_path_census(fw_ctx *ctx, uint32_t *kept, uint32_t *recounted) {
    if (!ctx) return FW_EINVAL;
    if (kept) ctx->census.words(kept);
    if (recounted) {
        std::vector<uint32_t> bits;
        for (const SegHost &S : ctx->segs) bits.push_back(path_bits(S));
        FwPathCensus::recount(bits.data(), bits.size(), ctx->census.few_blocked).words(recounted);
    }
    return FW_OK;
}

fw_status fw_debug_whole_tiles(fw_ctx *ctx, uint64_t *launches, uint64_t *tiles) {
    if (!ctx) return FW_EINVAL;
    if (launches) *launches = ctx->whole_launches;
    if (tiles) *tiles = ctx->whole_tiles;
    return FW_OK;
}
// FIFO launches so far whose spawning workgroups deferred the spin of the particles they spawned (fw_spin_newborn_deferred, fw_spin.h)
fw_status fw_debug_newborn_spin(fw_ctx *ctx, uint64_t *launches) {
    if (!ctx || !launches) return FW_EINVAL;
    *launches = ctx->newborn_launches;
    return FW_OK;
}
// FIFO launches so far that ran two or more frames in one pass (fw_ctx::withheld, FwFifoArgs::fused) / withheld frames that went to the stream alone
fw_status fw_debug_fuse2(fw_ctx *ctx, uint64_t *fused, uint64_t *flushed) {
    if (!ctx) return FW_EINVAL;
    if (fused) *fused = ctx->fused_launches;
    if (flushed) *flushed = ctx->fuse2_flushed;
    return FW_OK;
}
// ... and the frames those launches ran: a launch of depth D counts D
fw_status fw_debug_fuse_frames(fw_ctx *ctx, uint64_t *frames) {
    if (!ctx || !frames) return FW_EINVAL;
    *frames = ctx->fuse_frames;
    return FW_OK;
}
fw_status fw_debug_tf_frames(fw_ctx *ctx, uint64_t *n) {
    if (!ctx || !n) return FW_EINVAL;
    *n = ctx->tf_frames;
    return FW_OK;
}
fw_status fw_debug_param_bar(fw_ctx *ctx, int32_t *on) {  // fw_ctx::param_bar
    if (!ctx || !on) return FW_EINVAL;
    *on = ctx->param_bar ? 1 : 0;
    return FW_OK;
}
// the batched boxes: launches of fw_k_boxes / fw_k_boxes_fold so far, the chunks of the latest call, list positions per chunk (fw_boxes.h)
fw_status fw_debug_aabb_batch(fw_ctx *ctx, uint64_t *launches, uint64_t *chunks, uint32_t *chunk_size) {
    if (!ctx) return FW_EINVAL;
    if (launches) *launches = ctx->boxes.launches;
    if (chunks) *chunks = ctx->boxes.last_chunks;
    if (chunk_size) *chunk_size = FW_BOX_CHUNK;
    return FW_OK;
}
// the volume queries: launches of fw_k_volumes / fw_k_volumes_fold so far, the chunks of the latest call, list positions per chunk
// (fw_boxes.h), volumes per tile (fw_volumes.h)
fw_status fw_debug_volume_query(fw_ctx *ctx, uint64_t *launches, uint64_t *chunks, uint32_t *chunk_size, uint32_t *volume_tile) {
    if (!ctx) return FW_EINVAL;
    if (launches) *launches = ctx->volumes.launches;
    if (chunks) *chunks = ctx->volumes.last_chunks;
    if (chunk_size) *chunk_size = FW_BOX_CHUNK;
    if (volume_tile) *volume_tile = FW_VOLUME_TILE;
    return FW_OK;
}
fw_status fw_debug_read_timestamps(fw_ctx *ctx, unsigned long long *out, uint64_t max_tiles, uint64_t *n_tiles) {
    return fw_debug_read_timestamps2(ctx, out, nullptr, max_tiles, n_tiles);
}

fw_status fw_ctx_kernel_timing_overhead(fw_ctx *ctx, double *ms_per_pair) {
    if (!ctx || !ms_per_pair) return FW_EINVAL;
    *ms_per_pair = ctx->tev_overhead_ms;
    return FW_OK;
}

fw_status fw_ctx_measure_copy_bandwidth(fw_ctx *ctx, uint64_t bytes, int32_t iters, double *bytes_per_s) {
    if (!ctx || !bytes_per_s || bytes < 4096 || iters < 1) return FW_EINVAL;
    hipSetDevice(ctx->device);
    if (fw_status fst = flush_withheld(ctx)) return fst;  // (fw_ctx::withheld)
    bytes &= ~(uint64_t)0xFFF;
    HipBuf<char> a, b;
    fw_status st = alloc_buf(ctx, a, bytes);
    if (st) return st;
    if (alloc_buf(ctx, b, bytes)) return fail(ctx, FW_ENOMEM, "copy probe allocation: " + ctx->err);
    fw_memset_done(a, 1, bytes);
    fw_memset_done(b, 0, bytes);
    HipEvent e0, e1;
    e0.create(hipEventDefault), e1.create(hipEventDefault);
    for (int i = 0; i < 3; i++) fw_launch_copy_probe(ctx->stream, a, b, bytes);
    hipEventRecord(e0, ctx->stream);
    for (int i = 0; i < iters; i++) fw_launch_copy_probe(ctx->stream, (i & 1) ? b : a, (i & 1) ? a : b, bytes);
    hipEventRecord(e1, ctx->stream);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    FW_HIP(ctx, e);
    *bytes_per_s = 2.0 * (double)bytes * iters / (ms * 1e-3);
    return FW_OK;
}

}  // extern "C"
