// fw_engine.h -- the host engine's own records and the functions its translation units share (internal: nothing here is ABI).
//
// Division of labour:
//   host   - owns the control block of every spawner: emission clocks, enabled flags,
//            the OnDemand queue (ParticleSpawnerData minus `particles`, reference
//            src/core.rs:261-303) and evaluates compute_emission_count for Global
//            entries (src/core.rs:396-428, 553-575) in bit-exact fp32;
//   device - owns all particle state (fw_device.h) and runs spawn + update +
//            compaction; Nested entries are counted per parent on the device.
// A frame is: [params H2D on the copy stream] -> spawn kernel(s) -> update kernel, all
// asynchronous; live counts come back through a pinned snapshot ring that the update
// kernel writes directly (no memcpy in the frame).
//
// There is no CPU simulation path in this library.
//
// The engine is six translation units (round 5; one 4 300-line file until then), along the seams of the work:
//   fw_engine_mem.cpp    device / pinned memory of a context, exact counts, the error words of the update kernels
//   fw_engine_paths.cpp  which update path a particle type is on (FIFO ring / range ring / small / compacting): the transitions
//                        between them with live particles, the capacity policy, the tile table of the compacting launch and
//                        the workgroup table of the range launch
//   fw_engine_build.cpp  sync_spawner_data (core.rs:343-365): descriptors -> device tables of one spawner, and back
//   fw_engine_step.cpp   fw_step and the plan of a frame: mode exits, lifetime windows, emission clocks, ring-op routing, the
//                        tile table -- everything that can still be rolled back
//   fw_engine_launch.cpp the enqueue of a planned frame (FwFrame): op tables, cohort replay, every launch, the frame's bookkeeping
//   fw_engine_api.cpp    every other entry point of include/firework_hip.h (+ the debug hooks), the depth-sorted records, the batched boxes and the
//                        volume queries (which ask about the particles, not the collider world) among them
//   fw_engine_mesh.cpp   the collider meshes: fw_ctx_create_mesh / fw_ctx_create_deformable_mesh / fw_ctx_update_mesh_vertices /
//                        fw_ctx_destroy_mesh / fw_ctx_set_mesh_colliders (the
//                        hierarchy itself is built by fw_bvh.cpp, plain C++)
//   fw_engine_query.cpp  the queries into the collider world: fw_ctx_cast_rays[_device], fw_ctx_project_points[_device]
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <deque>
#include <mutex>
#include <new>
#include <vector>

#include <sys/mman.h>
#include <immintrin.h>

#include "../../include/firework_hip.h"
#include "../../include/firework_hip_debug.h"
#include "fw_kernels.h"
#include "fw_math.h"
#include "fw_ages.h"
#include "fw_spin.h"
#include "fw_fuse2.h"
#include "fw_withheld.h"
#include "fw_update_path.h"
#include "fw_sort.h"
#include "fw_boxes.h"
#include "fw_volumes.h"

namespace fwh {

// hipMemset runs on the null stream and may return before the fill has happened; the streams of a context are
// non-blocking ones, which the null stream does not order itself against: a kernel enqueued right after would race the fill
// (seen with two processes on the GPU: a fresh context's first frames read the forecast entries a previous context had left
// in the recycled allocation).  Every fill of this file is part of an allocation (rare): wait for it.
inline hipError_t fw_memset_done(void *p, int v, size_t bytes) {
    hipError_t e = hipMemset(p, v, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

// ---- owning handles of the HIP resources a context holds.  Move-only; each releases what it holds when it is reset, assigned
// or destroyed, with the call that matches how it was allocated.  They convert to the raw handle, which is what the kernels,
// the launches and FwGlobals see.  None of them reads the environment or the device: a buffer gets memory through alloc_buf /
// grow_buf only (below fw_ctx).
enum class Mem : uint8_t {
    device,  // hipMalloc
    fine,    // hipExtMallocWithFlags(hipDeviceMallocFinegrained): device memory the host writes through the large BAR
    pinned,  // hipHostMalloc
};

template <typename T>
class HipBuf {
public:
    HipBuf() : n_(0), kind_(0) {}
    HipBuf(HipBuf &&o) noexcept : p_(o.p_), n_(o.n_), kind_(o.kind_) { o.p_ = nullptr, o.n_ = 0; }
    HipBuf &operator=(HipBuf &&o) noexcept {
        if (this != &o) reset(), p_ = o.p_, n_ = o.n_, kind_ = o.kind_, o.p_ = nullptr, o.n_ = 0;
        return *this;
    }
    ~HipBuf() { reset(); }
    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t cap() const { return n_; }  // elements
    void reset() {
        if (p_) (void)((Mem)kind_ == Mem::pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, n_ = 0;
    }
    // (what alloc_buf hands over: memory of n elements allocated as `kind`)
    void adopt(void *p, size_t n, Mem kind) { reset(), p_ = static_cast<T *>(p), n_ = n, kind_ = (size_t)kind; }

private:
    T *p_ = nullptr;
    size_t n_ : 62, kind_ : 2;  // (16 bytes: SegHost holds three)
};

class HipEvent {
public:
    HipEvent() = default;
    HipEvent(HipEvent &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    HipEvent &operator=(HipEvent &&o) noexcept {
        if (this != &o) reset(), e_ = o.e_, o.e_ = nullptr;
        return *this;
    }
    ~HipEvent() { reset(); }
    operator hipEvent_t() const { return e_; }
    hipError_t create(unsigned flags = hipEventDisableTiming) {
        reset();
        return hipEventCreateWithFlags(&e_, flags);
    }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

// a stream the context created (destroyed with it) or the caller's (fw_ctx_create(.., stream, ..): never destroyed here)
class HipStream {
public:
    HipStream() = default;
    HipStream(const HipStream &) = delete;
    HipStream &operator=(const HipStream &) = delete;
    ~HipStream() { reset(); }
    operator hipStream_t() const { return s_; }
    bool owned() const { return own_; }
    hipError_t create() {
        reset();
        own_ = true;
        return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    }
    void borrow(hipStream_t s) { reset(), s_ = s; }
    void reset() {
        if (s_ && own_) (void)hipStreamDestroy(s_);
        s_ = nullptr, own_ = false;
    }

private:
    hipStream_t s_ = nullptr;
    bool own_ = false;
};

// ---- what is in flight, on top of the handles.  The host hands small tables to the device by writing pinned memory and enqueueing ONE
// hipMemcpyAsync (or a kernel that reads the memory in place) on a stream: no frame in flight stalls.  The one invariant of every such
// site: the pinned memory -- and a single device table it feeds -- is not rewritten while the copy or kernel that reads it may still be
// running.  A Fence holds it: whoever enqueues the reader marks the fence behind it, whoever writes the memory next waits first (a
// single branch unless that reader was enqueued since the last wait), and whoever has waited for everything (sync) before the buffers
// are replaced forgets it.  (methods: below FW_HIP)
class Fence {
public:
    fw_status wait(fw_ctx *ctx) { return pending_ ? wait_pending(ctx) : FW_OK; }
    fw_status mark(fw_ctx *ctx, hipStream_t stream);  // (creates the event on first use)
    void forget() { pending_ = false; }

private:
    fw_status wait_pending(fw_ctx *ctx);
    HipEvent ev_;
    bool pending_ = false;
};

// N pinned staging slots used in turn, a fence each: with two, a set that changes every call is written while the previous one is still
// on its way, and a call waits only for the copy N calls back.  take: the slot of this turn, free and grown to hold n elements (the
// only allocation); commit: the copy went to `stream` -- only now is the turn used up (a call that is refused in between finds the
// same slot again).  With `dev`, the single device table the slot feeds grows with it, all or nothing, behind a sync: the capacity of
// the pair is the smaller of the two.
template <typename T, int N>
struct Staging {
    HipBuf<T> h[N];
    Fence fence[N];
    uint64_t turn = 0;  // commits so far
    fw_status take(fw_ctx *ctx, size_t n, size_t grow_to, T **out = nullptr, HipBuf<T> *dev = nullptr);
    fw_status commit(fw_ctx *ctx, hipStream_t stream);
};

constexpr int kParamRing = 8;    // per-frame parameter buffers in flight
#ifndef FW_BAR_PARAM_KB
#define FW_BAR_PARAM_KB 64
#endif
constexpr size_t kBarParamBytes = (size_t)FW_BAR_PARAM_KB << 10;  // fw_ctx::b_param
constexpr int kSnapRing = 8;     // live-count snapshots in flight
constexpr int kSnapEvery = 4;    // frames between snapshots
constexpr int kTabRing = 4;      // staging buffers for tile-table uploads
constexpr uint64_t kResidentSlots = 1024;  // fw_k_update workgroups resident at once on MI355X (256 CUs x 4)
constexpr uint32_t kMinCapacity = 4096;
constexpr uint32_t kNoSeg = 0xFFFFFFFFu;  // SpawnerHost::seg entry not built yet
constexpr uint64_t kMaxSpawnPerOp = 1ull << 30;
constexpr uint32_t kTimingEvents = 4096;
constexpr size_t kMaxCohorts = 16384;    // spawn cohorts a FIFO segment tracks before it gives the mode up (tiny dt)
constexpr uint32_t kReportRing = 32768;  // pinned per-frame cohort sizes of a ring that receives Nested children (> kMaxCohorts)

extern thread_local std::string g_create_error;  // (fw_last_error(nullptr): per calling thread, like errno; fw_engine_api.cpp)

// Host memory the per-frame loops of fw_step stream through -- the segment and spawner records, every segment's lifetime
// window.  As ordinary heap blocks they sit on thousands of 4 KB pages (one window ring per emitter alone): past ~3000
// emitters the loops missed the TLB on most records (2048 emitters: 28 ns each, 4096: 39 ns).  They come from 2 MB-aligned
// chunks instead, which the kernel is asked to back with huge pages (madvise: a no-op where transparent huge pages are off).
// One process-wide pool: blocks of 1536 << k bytes (a window ring of 64 << k entries) on free lists, larger requests mapped
// on their own; chunks are never returned (destroyed contexts leave their blocks on the lists).  Thread-safe: contexts may be
// driven from different threads.
class HugePool {
public:
    static void *alloc(size_t bytes) {
        if (bytes > kMaxBlock) return map(bytes);
        const int c = cls(bytes);
        std::lock_guard<std::mutex> lk(mu());
        Node *&head = lists()[c];
        if (head) {
            Node *n = head;
            head = n->next;
            return n;
        }
        const size_t sz = kBase << c;
        char *&cur = chunk_cur(), *&end = chunk_end();
        if (cur == nullptr || (size_t)(end - cur) < sz) {
            // (what is left of the old chunk goes to the lists of the classes it still fits)
            while (cur && (size_t)(end - cur) >= kBase) {
                int k = 0;
                while (k + 1 < kClasses && (kBase << (k + 1)) <= (size_t)(end - cur)) k++;
                Node *n = reinterpret_cast<Node *>(cur);
                n->next = lists()[k], lists()[k] = n;
                cur += kBase << k;
            }
            cur = static_cast<char *>(map(kChunk));
            if (!cur) return nullptr;
            end = cur + kChunk;
        }
        void *p = cur;
        cur += sz;
        return p;
    }
    static void free(void *p, size_t bytes) {
        if (!p) return;
        if (bytes > kMaxBlock) {
            munmap(p, (bytes + kHuge - 1) / kHuge * kHuge);
            return;
        }
        std::lock_guard<std::mutex> lk(mu());
        Node *n = static_cast<Node *>(p);
        n->next = lists()[cls(bytes)], lists()[cls(bytes)] = n;
    }

private:
    struct Node {
        Node *next;
    };
    static constexpr size_t kBase = 1536, kHuge = 2u << 20, kChunk = 8u << 20;
    static constexpr int kClasses = 11;  // 1.5 KB ... 1.5 MB
    static constexpr size_t kMaxBlock = kBase << (kClasses - 1);
    static int cls(size_t bytes) {
        int c = 0;
        while ((kBase << c) < bytes) c++;
        return c;
    }
    static std::mutex &mu() {
        static std::mutex m;
        return m;
    }
    static Node **lists() {
        static Node *l[kClasses] = {};
        return l;
    }
    static char *&chunk_cur() {
        static char *p = nullptr;
        return p;
    }
    static char *&chunk_end() {
        static char *p = nullptr;
        return p;
    }
    // `bytes` rounded up to 2 MB, aligned to 2 MB, huge pages requested
    static void *map(size_t bytes) {
        const size_t len = (bytes + kHuge - 1) / kHuge * kHuge;
        char *raw = static_cast<char *>(mmap(nullptr, len + kHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
        if (raw == MAP_FAILED) return nullptr;
        char *al = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(raw) + kHuge - 1) / kHuge * kHuge);
        if (al > raw) munmap(raw, (size_t)(al - raw));
        if (al + len < raw + len + kHuge) munmap(al + len, (size_t)(raw + len + kHuge - (al + len)));
        madvise(al, len, MADV_HUGEPAGE);
        return al;
    }
};

template <typename T>
struct HugeAlloc {
    using value_type = T;
    HugeAlloc() = default;
    template <typename U>
    HugeAlloc(const HugeAlloc<U> &) {}
    T *allocate(size_t n) {
        void *p = HugePool::alloc(n * sizeof(T));
        if (!p) throw std::bad_alloc();
        return static_cast<T *>(p);
    }
    void deallocate(T *p, size_t n) { HugePool::free(p, n * sizeof(T)); }
    template <typename U>
    bool operator==(const HugeAlloc<U> &) const { return true; }
    template <typename U>
    bool operator!=(const HugeAlloc<U> &) const { return false; }
};

struct CurveCopy {
    int32_t kind = 0, n = 0;
    std::vector<float> times, values;  // values: n (curve) or 4n (gradient)
};

struct TypeHost {
    fw_particle_settings ps{};
    CurveCopy scale, base, emis;
    // every particle of this type outlives a step of dt < life_lo_safe: lifetime = u * (max - min) + min, u in [0, 1),
    // two ulps of margin for the rounding of the lerp; NaN when the range is not finite (never provably safe)
    float life_lo_safe = 0.f;
};

struct EmissionHost {
    // ---- what fw_step's spawner loop touches: this state and the head of `es` (pacing, counts, mode: its first 40 bytes),
    // next to each other (with thousands of emitters the loop is bound by the cache lines it streams, not its arithmetic)
    // EmissionData (reference src/core.rs:261-267)
    float last_emission = 0.f, time_passed_in_cycle = 0.f;
    uint64_t serial = 0;      // RNG stream position (Global entries; Nested ones live on the device)
    uint32_t emit_idx = 0;    // -> FwEmit
    uint32_t emit_slot = 0;   // -> device serial counter (Nested)
    uint32_t dst_seg = 0;     // segment of es.particle_index (cached: the frame loop then touches only this record)
    float life_lo_safe = 0.f; // TypeHost::life_lo_safe of es.particle_index
    float between = 0.f;      // (es.offset_end - es.offset_start) / es.count: fw_emission_count_unit
    bool enabled = false, emits_on_other_particles = false;
    bool assigned = false;    // emit_idx / emit_slot are owned by this entry
    fw_emission_settings es{};
};

// The emission entries of a spawner.  ONE entry -- by far the most common spawner -- lives inside the spawner's own record
// (no heap block, no pointer to chase: the spawner array is then all the frame loop streams); more entries live in a vector.
struct EmVec {
    uint32_t n_ = 0;
    EmissionHost one_;
    std::vector<EmissionHost> more_;
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    EmissionHost *data() { return n_ > 1 ? more_.data() : &one_; }
    const EmissionHost *data() const { return n_ > 1 ? more_.data() : &one_; }
    EmissionHost &operator[](size_t i) { return data()[i]; }
    const EmissionHost &operator[](size_t i) const { return data()[i]; }
    EmissionHost *begin() { return data(); }
    EmissionHost *end() { return data() + n_; }
    const EmissionHost *begin() const { return data(); }
    const EmissionHost *end() const { return data() + n_; }
    void assign(size_t n, const EmissionHost &v) {
        more_.clear();
        one_ = v;
        if (n > 1) more_.assign(n, v);
        n_ = (uint32_t)n;
    }
    void clear() { assign(0, EmissionHost{}); }
};

// A queue in ONE pooled allocation (HugePool), a power of two of entries: in the steady state every frame pops one entry and
// pushes one per segment; a std::deque pays its chunk bookkeeping and two dependent pointer hops for each -- 30 us per frame
// with 2048 emitters.
template <typename T>
struct Ring {
    std::vector<T, HugeAlloc<T>> v;
    uint32_t head = 0, n = 0;
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    T &front() { return v[head]; }
    T &back() { return v[(head + n - 1) & (uint32_t)(v.size() - 1)]; }
    void pop_front() { head = (head + 1) & (uint32_t)(v.size() - 1), n--; }
    void pop_back() { n--; }
    void clear() { head = n = 0; }
    void push_back(const T &x) {
        if (n == v.size()) {  // grow to the next power of two, oldest entry first
            std::vector<T, HugeAlloc<T>> w(v.empty() ? 64 : v.size() * 2);
            for (uint32_t i = 0; i < n; i++) w[i] = v[(head + i) & (uint32_t)(v.size() - 1)];
            v.swap(w), head = 0;
        }
        v[(head + n) & (uint32_t)(v.size() - 1)] = x, n++;
    }
};

// The particle memory of a segment, as alloc_seg_buffers makes it: ONE allocation (a ring, updated in place: buf[0] == buf[1]; two
// buffers otherwise) and the destroyed-record buffer.  Held by the caller until nothing else can fail, then handed to SegHost::take.
struct SegBufs {
    HipBuf<char> mem, destroyed;
    char *buf[2] = {nullptr, nullptr};  // (views into mem)
    uint32_t capacity = 0;
};

struct alignas(64) SegHost {
    // Lifetime window: a particle is destroyed by the update in which age >= lifetime (core.rs:590-592), and
    // lifetime <= life_bound, so everything alive was spawned less than life_bound of simulated time ago.  The sum of
    // the Global spawn counts inside that window bounds the live count without any device feedback.
    struct Spawned {
        double t;        // simulated time at the spawn
        uint64_t n;
        uint64_t frame;  // frame of the spawn (the device's ages are fp32 sums: the error grows with the steps taken)
    };
    using Window = Ring<Spawned>;
    // ---- what the per-frame loops of fw_step touch, in ONE cache line (with thousands of segments those loops are
    // bound by how many lines they stream, not by their arithmetic)
    bool in_use = false;
    bool nested_fed = false;    // receives Nested children: count not host-predictable
    bool collides = false;      // the type has collision settings (core.rs:137-138): frames run the collision path
    bool coll_inplace = false;  // ... without destroy_on_collision: a bounce changes neither age, lifetime nor order
                                // (core.rs:607-643), so the type may live in a ring (the COLL instantiations of the ring kernels)
                                // (also set for a type whose curve keys exceed the LDS staging area: the same feature
                                // kernels read them from device memory -- SegHost::bigkeys)
    bool auto_capacity = false; // capacity was derived (fw_particle_settings.capacity == 0): the library may grow it
    bool win_ok = false;
    bool dead_at_end = false;   // the last step left this type's destroyed records at the END of its buffer (a range ring's
                                // update fills them from there, the youngest dead first: fw_k_update_range)
    bool solo = false;          // a small type ONE Global entry feeds: its frame-begin work (lifetime window, bound) happens where
                                // fw_step's spawner loop makes its op -- the record is streamed once per frame, not twice (FwPathCensus::n_solo)
    uint32_t capacity = 0;
    uint32_t ub = 0;            // upper bound of the device count (after this frame's spawns)
    uint32_t frame_spawn = 0;   // Global particles appended this frame
    uint32_t dev_count = 0;     // nested_fed: live count of the latest snapshot row (growth trigger)
    uint32_t dev_epoch = 0;     //   ... the frame that row describes, and
    float dev_rate = 0.f;       //   ... how fast the count was growing between the last two rows (particles per frame, >= 0)
    uint32_t snap_count = 0;    // nested_fed: ... the same count, kept together with
    uint64_t snap_cum = 0;      //   cum_spawn of the frame that row describes: Global particles since then are host-known
    uint64_t cum_spawn = 0;     // Global particles ever appended (host-known)
    uint64_t win_sum = 0;
    // ---- second line: the window itself and the segment's mode (both per-frame loops look at them)
    double life_bound = 0.0;
    char *inst = nullptr;       // caller-owned device buffer of ParticleInstance records (fw_spawner_attach_instances)
    Window win;
    bool fifo = false;          // FIFO ring (below)
    bool range = false;         // range ring (below)
    bool fifo_mat = false, fifo_dev = false, range_mat = false, range_dev = false, virt_parent = false;  // (below)
    // ---- the rest
    int spawner = -1, type = -1;
    uint32_t type_idx = 0, n_lplanes = 0;
    uint32_t keys_off = 0, keys_len = 0;  // key pool window of the segment's type
    uint32_t keys_cap = 0;                // ... and the floats reserved for it (returned to fw_ctx::free_keys with the type)
    bool bigkeys = false;                 // more keys than the streaming kernels stage in LDS (FW_KEYS_MAX floats)
    std::vector<int32_t> lplane_emission;  // [n_lplanes] the emission entry each last_emitted_age plane belongs to
    char *buf[2] = {nullptr, nullptr};     // (views into `mem`, at the end of the record)
    HipBuf<char> destroyed;                // the destroyed records
    uint32_t inst_cap = 0;
    // colours of the type at age 0: what both colour planes are filled with when the buffers are allocated, so that a
    // constant gradient's plane never has to be written by the update (FwOutWin::wr5 / wr6)
    float fill_bc[4] = {0, 0, 0, 0}, fill_em[4] = {0, 0, 0, 0};
    bool colors_dirty = false;  // the caller wrote particles (any colours) into the current buffer
    // FIFO ring (fw_kernels.h: FwFifoSeg): a type with a single lifetime value, Global emission only, no collisions.
    // ONE buffer (buf[0] == buf[1]); logical particle i sits in slot (head + i) mod capacity; `ub` is the EXACT live
    // count.  The host replays the fp32 age of every spawn cohort (same additions as the device), which tells it how
    // many particles each update destroys -- always the oldest ones.
    uint32_t head = 0;
    float fifo_life = 0.f;  // the lifetime every particle of the type gets (core.rs:455 with min == max)
    float fifo_move[4] = {0.f, 0.f, 0.f, 0.f};  // FwType::acc[0 .. 2] and lin_drag of the type: FwFuseArgs::move of the ring (round 30)
    int32_t fifo_wm = 0;    // FwFifoArgs::write_mask of the type
    // FW_TYPE_NOSPIN (fw_device.h): no particle of the type can turn; the rotation plane is neither read nor written
    bool nospin = false;
    float const_rot[4] = {0.f, 0.f, 0.f, 1.f};
    // The axis-spin rule (fw_engine_build.cpp: axis_spin_rule; FW_TYPE_IDX_AXIS): 0, or k + 1 when every particle of the type spins
    // about coordinate axis k.  launch_fifo sets the bits of a frame whose dt the proof covers (axis_dt_ok); the first frame that
    // voids the proof, the caller rewriting the particles, or the ring leaving the FIFO kernel (fifo_to_general, fifo_to_range)
    // clears the property for good: it is never set again after build_spawner.
    uint32_t axis = 0;
    float axis_wmax = 0.f;  // |angular velocity| of every particle of the type is at most this, for ever
    float axis_drag = 0.f;  // the type's angular_drag (finite, >= +0)
    // ... and keeps its lifetimes in one more 4-byte plane behind the n_lplanes last_emitted_age planes instead of in Q3
    // (allocated with the type, kept when the type leaves the mode)
    uint32_t n_xplanes = 0;
    struct Cohort {
        uint32_t n;
        float age;
        uint64_t frame = 0;  // frame the cohort was added in
        bool known = true;   // false: a cohort of Nested children whose size the device has not been asked for yet
        uint64_t spin_from = 0;  // first entry of `spin`'s log the cohort's particles have not had applied (fw_spin.h; read while spin.stale)
    };
    std::deque<Cohort> coh;  // oldest first
    // The age rule (fw_device.h: FW_TYPE_IDX_AGELESS): the ring's latest launches neither loaded nor stored the age plane -- the cohort
    // ages above stand for it.  ensure_ages writes them back (fw_k_fifo_ages) before anybody reads the plane, before a launch that
    // does not carry the bit, and before the ring is copied or changes its kind.  ageless_last: the latest launch carried the bit.
    bool ages_stale = false, ageless_last = false;
    // The deferred spin (fw_spin.h; FW_TYPE_IDX_NOSPIN together with FW_TYPE_IDX_AXIS): the ring's latest launches under the age rule AND
    // the axis rule left rotation and angular velocity of the particles they did not spawn alone and logged their dt.  ensure_spin
    // replays the log per particle (fw_k_fifo_spin) before anybody reads those planes, before a launch that does not defer, and before
    // the ring is copied, changes its kind or gets a new type record.  spin_streak: consecutive launches that met every condition of
    // the rule since anybody last asked for the planes (fw_ctx::spin_defer_after); spin_last: the latest launch was deferred.
    FwSpinBook spin;
    uint32_t spin_streak = 0;
    bool spin_last = false;
    uint32_t fuse_last = 0;  // the frames of the ring the latest launch ran in one pass, 2 .. FW_FUSE_FAR, or 0: one, unfused (fw_ctx::withheld): fw_debug_update_path
    bool q0pl = false;  // the ring keeps Q0 (position, age) as four component planes (FwSeg::cpl bit 2): set where the ring is built
    // A ring in a spawner WITH Nested entries: in frames that run the Nested pass its new particles are materialised in
    // the ring before the update (fw_k_spawn / fw_k_nest address it through the head) and fw_k_update_fifo gives them
    // their first update (FwFifoSeg::mat).  fifo_dev: the type receives Nested children -- its live count is known to the
    // device only, and the size of each frame's cohort reaches the host through a pinned ring (h_report[frame %
    // kReportRing] = {epoch, added}) long before the host needs it: when the cohort's age reaches the lifetime.
    HipBuf<unsigned long long> h_report;  // (pinned)
    // Range ring (fw_kernels.h: FwRangeRec): a type whose lifetime is a RANGE, Global emission only, no collisions, in a
    // spawner without Nested entries.  ONE buffer (buf[0] == buf[1]) used as a ring: [old survivors | young]; the young
    // part -- slot of its first particle, its size, its spawn cohorts -- is host-known exactly (the host made every spawn
    // count and replays the fp32 age of every cohort: fw_ctx::birth_age); the size of the old part is the device's
    // count minus young_n.  `ub` bounds the total as for any segment (lifetime window, snapshots).
    // (what the range pass of every frame reads and writes, next to each other)
    uint32_t young_lo = 0, young_n = 0;
    float range_life_lo = 0.f;  // every particle outlives an update that leaves its age below this (TypeHost::life_lo_safe)
    struct YCohort {
        uint64_t frame;  // frame of the spawn
        uint32_t n;
    };
    Ring<YCohort> ycoh;  // the young cohorts, oldest first
    bool few_ring = false;  // a range ring below fw_ctx::range_min: only because the context holds few segments (fw_ctx::range_few)
    bool spilled = false;   // a range ring that qualifies for a FIFO ring: the context holds more such types than one FIFO launch (FwPathCensus::n_spilled)
    // A SMALL type (fw_k_small.hip, round 5): a few hundred particles, updated by ONE WAVE (four types per workgroup) instead of a
    // workgroup of the compacting kernels -- no tile table entry, no forecast.  Same buffers and layout as a compacting segment:
    // entering and leaving the mode is this flag (FwPathCensus::n_small, small_eligible / leave_small).
    bool small = false;
    bool small_ok = false;    // ... qualifies for it (small_eligible); `small` follows the context's mode (fw_ctx::small_on)
    bool wide = false;        // ... as a WIDE type: up to a few thousand particles, a workgroup instead of a wave (fw_ctx::wide_max)
    bool wide_big = false;    // ... one that sustains more than fw_ctx::wide_mid particles: on the kernel only among wide_min types
    bool one_feeder = false;  // exactly one emission entry (a Global one) spawns into the type (SegHost::solo)
    float expect_live = 0.f;  // live particles the emitters that feed the type sustain (what derive_capacity derives the capacity from)
    uint32_t r_old = 0, r_new = 0, r_young = 0;  // workgroups of each role the device table provides for the segment
    uint32_t r_low[3] = {0, 0, 0};               // frames in a row a role's need has been far below what is provided
    uint32_t r_need[3] = {0, 0, 0};              // what each role needed in the latest frame (the table keeps more: fit())
    uint32_t r_status_base = 0;                  // first look-back word of its OLD workgroups in the current table
    uint32_t ticket_base = 0;                    // value of FwGlobals::range_ticket[segment] at the start of the next launch (START tickets)
    // ... in a spawner WITH Nested entries (core.rs:471-546):
    //   range_mat  other particles' entries emit FROM this type: in frames that run a Nested pass its Global particles are
    //              materialised behind the young part by fw_k_spawn before the pass (core.rs:488) and fw_k_update_range
    //              gives them their first update (FW_RREC_MAT);
    //   range_dev  the type RECEIVES Nested children: its live count -- hence the size of its young part -- is known to the
    //              device only (FW_RREC_DEV).  The host still knows where the young part STARTS: cohorts join the old part a
    //              lifetime.min after they were added, and by then the update of their frame has long left their size in the
    //              pinned ring h_report (as for a FIFO ring that receives children).
    // A ring type other particles' entries emit from whose Global particles need NOT be in memory for the frame's Nested pass:
    // every Nested entry on it is a CountOverDuration with count > 0 and 0 <= offset_start <= offset_end, and the type's
    // lifetimes are positive -- then compute_emission_count(age 0, last f32::MIN, ..) emits nothing for a particle born this
    // frame (core.rs:553-575: since = min(0, end) - start <= 0) and only leaves `next` in its last_emitted_age, which the lane
    // that spawns the particle inside the ring's update kernel computes itself (fw_init_last_emitted).  Such a type is spawned
    // in its update kernel in EVERY frame: a steady Nested frame is fw_k_nest + the update, without fw_k_spawn.
    struct DCohort {
        uint64_t frame;
        uint32_t n;
        bool known;
    };
    std::deque<DCohort> dcoh;   // range_dev: the young cohorts, oldest first (sizes unknown until they are needed)
    std::deque<YCohort> gcoh;   // range_dev: cohorts that have joined the old part and may still hold survivors (their bound)
    uint64_t gcoh_sum = 0;
    uint32_t rold_seen = 0;     // the old part's size as of the last exact read (refresh_counts_exact): FwGlobals::rold
    uint32_t r_young_main = 0;  // range_dev: young tiles the current table keeps in front (the rest: probably idle, at its end)
    bool ring() const { return fifo || range; }
    // FwSeg::cpl: bit 0 -- a ring, Q1 / Q3 in component planes; bit 1 -- a FIFO ring, the rotation (Q2) as well.  A range ring keeps Q2 as a
    // float4 plane (fifo_to_range transposes it where it stands).
    // (round 18: bit 2 -- a FIFO ring that may run under the age rule, SegHost::q0pl: Q0 as well; fifo_to_range transposes that one too)
    uint32_t cpl_bits() const { return ring() ? (fifo ? (q0pl ? 7u : 3u) : 1u) : 0u; }  // one buffer, particle 0 not in slot 0
    // ... but in this slot, as a launch that is ENQUEUED now has to be told (behind updates that may still be in flight): a FIFO ring's
    // head; a range ring's first YOUNG slot -- the device subtracts the old part, whose size only it knows (FwGlobals::rold)
    uint32_t enqueue_head() const { return fifo ? head : (range ? young_lo : 0u); }
    // FW_TYPE_DERIVED (fw_device.h): the planes S4 / Q5 / Q6 are not stored by the update; every reader evaluates scale and
    // colours from age / lifetime / initial_scale (an attached instance buffer receives them in its records).  Every type but
    // colliding ones and those whose curve keys exceed the LDS staging (fw_ctx::derive_all, wants_derived)
    bool derived = false;
    // ... but not yet: the caller wrote particles (any scale, any colours), and those that die in the very next step carry
    // what was written in their destroyed records -- the planes are read for one more frame, then the mode starts
    bool derive_pending = false;
    bool derive_ready = false;  // ... that frame has been enqueued: the flag flips at the start of the next fw_step
    // the attached buffer is a WINDOWED one (fw_spawner_attach_instances_window): the caller draws d_out[first, first + count)
    // and asks for `first` -- which lets a range ring keep its path (its tiles know a record's index counted from the
    // particles the update destroys, not from 0)
    bool inst_window = false;
    // where the lifetime of particle i is when the type cannot turn: a plane index (compacting / range segments), or
    // 0xFFFFFFFF = the one value fifo_life (a FIFO ring)
    uint32_t life_plane() const { return (nospin && !fifo) ? n_lplanes : 0xFFFFFFFFu; }
    HipBuf<char> mem;  // the particle allocation (SegBufs; no frame reads it)
    // the segment's particle memory becomes `b` (what it held is released)
    void take(SegBufs &&b) {
        mem = std::move(b.mem), destroyed = std::move(b.destroyed);
        buf[0] = b.buf[0], buf[1] = b.buf[1], capacity = b.capacity;
    }
};

struct alignas(64) SpawnerHost {
    // ---- first line: what every frame reads of a spawner; the entries follow (EmVec: one entry is inline)
    bool alive = false;
    bool initialized = false, finished_notified = false;
    // An internal error of an update kernel (FwGlobals::err_host) named one of this spawner's particle types: its particle
    // state can no longer be trusted -- an in-place ring update that went wrong has overwritten its own input and cannot be
    // redone.  Sticky: fw_step refuses to run and every call that reads or writes the spawner's particles returns FW_EHIP
    // until fw_spawner_update_settings rebuilds it (which drops all particles, core.rs:343-365) or it is destroyed.
    bool poisoned = false;
    // ... and the rebuilt spawner keeps its particle types off the in-place ring paths
    bool no_rings = false;
    uint64_t manual_queued_count = 0;
    float origin_pos[3] = {0, 0, 0}, origin_rot[4] = {0, 0, 0, 1}, parent_vel[3] = {0, 0, 0};
    float mod_scale = 1.f, mod_speed = 1.f;
    EmVec em;
    // ---- the rest
    uint32_t uid = 0;
    int32_t starts_enabled = 1;
    std::vector<TypeHost> types;
    std::vector<uint32_t> seg;  // per type
};

}  // namespace fwh
using namespace fwh;

// The Global ops of one emission index: a growable array that owns its storage -- or, in a frame that will most likely hand the
// kernels an op TABLE (small types: fw_k_update_small reads its ops from pinned host memory), writes straight into the pinned
// parameter slot the kernels will read (FwFrame::pre_slot): 96 bytes per emitter that are written once instead of written,
// read and written again.
struct OpList {
    FwOp *p = nullptr;
    size_t n = 0, cap = 0;
    bool lent = false;  // p points into a parameter slot, not into `own`
    std::vector<FwOp> own;
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    FwOp *begin() { return p; }
    FwOp *end() { return p + n; }
    const FwOp *begin() const { return p; }
    const FwOp *end() const { return p + n; }
    FwOp *data() { return p; }
    FwOp &operator[](size_t i) { return p[i]; }
    const FwOp &operator[](size_t i) const { return p[i]; }
    void clear() {
        n = 0;
        if (lent) lent = false, p = own.data(), cap = own.size();
    }
    void borrow(FwOp *mem, size_t c) { p = mem, cap = c, n = 0, lent = true; }  // (of an empty list)
    void reserve_own(size_t c) {  // contents move into (larger) storage of the list's own
        c = std::max<size_t>(std::max<size_t>(c, n), 64);
        if (!lent) {
            if (c <= cap) return;
            own.resize(c);  // (keeps the contents)
        } else {
            if (own.size() < c) own.resize(c);
            if (n) memcpy(own.data(), p, n * sizeof(FwOp));
            lent = false;
        }
        p = own.data(), cap = own.size();
    }
    FwOp &push_slot() {  // the next op, to be filled in place (NOT zeroed)
        if (n == cap) reserve_own(cap * 2);
        return p[n++];
    }
    void push_back(const FwOp &x) { push_slot() = x; }
    void append(const FwOp *b, const FwOp *e) {
        for (; b != e; ++b) push_back(*b);
    }
};

struct FwLevel {  // ops of one emission index (spawn order inside a frame: core.rs:377-428)
    OpList g;
    std::vector<FwNestOp> n;
};

struct fw_ctx {
    std::vector<FwLevel> levels;  // per-frame scratch of fw_step: one entry per emission index in use
    OpList ops_scratch;
    std::vector<uint32_t> grow_scratch;  // fw_step: Nested-fed segments past half their capacity
    // device staging of the record-format copies (read_particles / write_particles / pack_instances): ONE allocation that
    // only ever grows, instead of a hipMalloc + hipFree pair per call (each a device-wide synchronisation and an address-
    // space change; profiles/r02/shared_gpu.txt)
    HipBuf<char> d_stage;
    // scratch of the depth sort (fw_ctx_depth_order_device, fw_ctx_pack_instances_sorted[_device]; fw_sort.h: fw_sort_scratch_words): two
    // (key, idx) pairs and the histogram table, laid out per call; only ever grows, and growing is the one case in which those calls wait
    HipBuf<uint32_t> d_sort;
    bool seg_kind_changed = false;       // a ring left its mode inside the current fw_step (realloc_segment)
    bool derive_ready_any = false;       // some SegHost::derive_ready is set
    // undo log of fw_step's host half: spawn_particles is all-or-nothing per frame in the reference, so a frame that
    // cannot be enqueued (limit exceeded, allocation failure) must leave clocks, queues and RNG serials untouched
    struct EmUndo {
        uint32_t spawner, entry;
        float last_emission, time_passed_in_cycle;
        bool enabled;
        uint64_t serial;
    };
    struct SpUndo {
        uint32_t spawner;
        uint64_t manual_queued_count;
    };
    std::vector<EmUndo> undo_em;
    std::vector<SpUndo> undo_sp;
    int device = 0;
    uint32_t seed = 0;
    HipStream stream, copy_stream;
    // Rings next to compacting segments: the ring launch and the general launch of a frame touch disjoint segments, so the
    // ring launch goes to a stream of its own and the two run concurrently (in one stream the second launch waits for the
    // first to drain: 1M ring particles + one small compacting emitter cost 39.8 us per frame, 29.4 with everything on the
    // general path).  Each chain is in order on its own stream; they are joined where the other stream (or the caller's
    // work on it) looks at ring data -- no event in a steady-state frame.  Not used while a ring has an attached instance
    // buffer, belongs to a spawner with Nested entries (fw_k_spawn / fw_k_nest on the main stream feed it) or a live-count
    // ring is registered.  FW_FIFO_STREAM=0: everything on the one stream.
    HipStream fifo_stream;
    HipEvent ev_side, ev_main;
    bool use_fifo_stream = true;
    bool side_dirty = false;      // ring launches on the side stream that the main stream has not waited for
    bool fifo_last_side = false;  // where the previous frame's ring launch went
    bool main_reads_ring = false; // work enqueued on the main stream since then reads ring data (must finish first)
    std::string err;
    int update_mode = FW_MODE_FUSED;
    uint32_t spin_limit = 1u << 16;
    uint32_t dbg = 0;  // FW_DEBUG: profiling-only kernel ablations (results are wrong when set)
    uint64_t recovered_rings = 0;  // rings sent to the compacting path because a cohort report was missing (fw_step: recoverable)

    std::vector<SpawnerHost, HugeAlloc<SpawnerHost>> spawners;  // (HugePool: huge pages)
    std::vector<SegHost, HugeAlloc<SegHost>> segs;
    uint32_t n_types = 0, n_emits = 0, n_emit_slots = 0;
    // table slots of destroyed / rebuilt spawners, reused by the next build (a type owns the key window
    // [type_idx * FW_KEYS_MAX, +FW_KEYS_MAX) of the key pool, so windows are recycled with their type)
    std::vector<uint32_t> free_types, free_emits, free_emit_slots;
    // the key pool: every type owns a window sized for its own curves (any number of samples, curve.rs:40-75)
    size_t keys_end = 0;                                      // floats handed out so far
    std::vector<std::pair<uint32_t, uint32_t>> free_keys;     // {offset, length} of windows of released types

    // the kernels' view of the context: its pointers are views of the owners below (and of d_segs .. d_colliders), each written
    // where its owner is (re)allocated
    FwGlobals g{};
    struct {
        HipBuf<uint32_t> count, spawned, appended, rold;  // [2][max_seg]
        HipBuf<uint32_t> ndestroyed, range_ticket;        // [max_seg]
        HipBuf<uint32_t> tile_cnt, tile_off, err;
        HipBuf<unsigned long long> tile_status, dbg_ts, nest_status, nest_ticket, stats;
        HipBuf<float> tile_box;
    } gm;
    HipBuf<FwSeg> d_segs;
    HipBuf<FwType> d_types;
    HipBuf<FwTypeColl> d_type_coll;
    HipBuf<float> d_keys;
    HipBuf<FwEmit> d_emits;
    HipBuf<unsigned long long> d_emit_serial;
    HipBuf<uint32_t> d_nest_start;               // FwGlobals::nest_start: START tickets of the Nested entries (one per emit slot)
    std::vector<uint32_t> nest_ticket_base;      // ... and the value each has at the start of the next launch that uses it
    uint32_t max_seg = 0;
    size_t tiles_cap = 0;

    // per-frame parameter ring (pinned host + device copies)
    size_t param_bytes = 0;
    HipBuf<char> h_param[kParamRing];  // (pinned)
    HipBuf<char> d_param[kParamRing];
    HipEvent ev_copied[kParamRing];
    Fence consumed[kParamRing];  // marked behind the last launch that reads the slot (end_frame; a small launch on the side stream)
    // Global-only frames with more ops than fit the kernel arguments: the kernel reads the op table straight from the
    // pinned ring slot (no copy, no events); a slot is free again once the launch after its frame has started, which
    // that launch reports through a pinned word (FwUpdateArgs::done_tag).
    HipBuf<unsigned long long> h_done;         // pinned; written by workgroup 0 of every update launch
    unsigned long long *h_err = nullptr;       // pinned; FwGlobals::err_host (h_done + 4: the same allocation); [1]: the device's
                                               // error flags are set (fw_flag)
    std::string poison_msg;                    // what poll_device_error saw
    uint32_t n_poisoned = 0;                   // spawners ever marked (fw_step scans for live ones only while non-zero)
    uint64_t slot_frame[kParamRing] = {};      // frame that last used the slot through the zero-copy path (+1; 0 = free)

    // live-count snapshots written by the update kernel into pinned host memory
    // Live-count snapshots: the update kernel stores {epoch, count} of each segment into a pinned row with one 8-byte
    // store; the host recognises a finished row by its tag -- no event, no packet between launches.
    HipBuf<unsigned long long> h_snap;  // [kSnapRing][max_seg] (pinned)
    bool snap_pending[kSnapRing] = {};
    bool snap_seen[kSnapRing] = {};
    uint32_t snap_epoch[kSnapRing] = {};
    std::vector<uint64_t> snap_cum[kSnapRing];  // cum_spawn of every segment when the frame was enqueued

    // device-resident segment -> tile table
    HipBuf<uint32_t> d_tile_first;
    size_t tile_first_cap = 0;  // (of d_tile_first, d_tile_keys, h_tab and h_keys)
    std::vector<uint32_t> tiles_dev;
    uint32_t total_tiles_dev = 0;
    HipBuf<uint32_t> h_tab[kTabRing];  // (pinned staging: h_keys, h_desc too)
    HipBuf<uint2> d_tile_keys;  // per segment: {keys_off, keys_len}
    HipBuf<uint2> h_keys[kTabRing];
    HipBuf<uint4> d_tile_desc;  // per tile: {segment, first tile, tile count, 0}
    HipBuf<uint4> h_desc[kTabRing];
    size_t tile_desc_cap = 0;
    Fence tab_fence[kTabRing];  // one per slot, over its three arrays
    uint64_t tab_seq = 0, ring_seq = 0;
    uint32_t vt_rounds = 1;  // new-particle tile size of the current frame (rounds of 256)
    bool tab_force = false;  // a segment was (re)built: re-send the descriptors even if the tile counts are equal

    // survivor forecast sums (update kernels)
    uint32_t fc_sums_prev = 0;    // format of the forecast the last forecast frame produced
    HipBuf<uint4> d_fce;          // [2][tiles_cap] forecast entries of small segments (double-buffered)
    HipBuf<unsigned long long> d_fc;      // three rotating buffers of forecast sums: S[tiles_cap] | S2[tiles_cap / 64 + 1] | tag
    size_t fc_len = 0;          // elements per buffer
    uint64_t fc_seq = 0;        // forecast-producing frames so far (buffer rotation)
    bool fc_dirty = false;      // the tile table changed: clear all three buffers before the next forecast frame
    bool fc_ok = false;        // the previous frame left a forecast that still describes the device state
    uint32_t fc_dt_bits = 0;   // ... computed for this dt
    uint64_t fc_tab_seq = 0;   // ... under this tile table
    bool use_forecast = true;  // FW_FORECAST=0 disables (A/B, debugging)
    // Threshold forecast (round 6, fw_kernels.h: FwUpdateArgs::fc_theta, fw_k_fc_resolve): a dt that does NOT repeat used to send every
    // compacting frame through the decoupled look-back (configs[2] on this path: 400 us per frame against 247 with a forecast).
    // Once the host has seen dt change, forecast frames of tf_min_tiles tiles or more (per-tile entries only) also leave, per tile,
    // the survivors a step of theta = 1.25 dt would destroy; the next frame, whatever its dt below that theta, runs fw_k_fc_resolve
    // (a wave per tile: ~3 us) in front of the streaming kernel instead of the look-back schedule.  A dt at or beyond theta, a
    // changed tile table, sums-format forecasts and small frames (a look-back costs them less than a launch) take the look-back as before.
    // FW_TF=0 switches it off, FW_TF_MIN_TILES=n (the tests: 0).
    bool use_tf = true;
    uint32_t tf_min_tiles = 768;  // (tools/r06_tf_min_tiles.py: 977 tiles 30.1 -> 22.2 us per frame, 256 tiles 17.0 -> 18.2)
    HipBuf<uint4> d_fct;        // [2][tiles_cap] headers, double-buffered like d_fce
    HipBuf<float2> d_fcl;       // [2][tiles_cap][FW_TF_K] (age, lifetime) of the risky survivors
    size_t tf_cap = 0;          // tiles_cap the two arrays were allocated for (0: not yet)
    uint32_t tf_armed = 0;      // frames left in which producers write lists (re-armed whenever dt differs from the last frame's)
    float tf_prev_theta = 0.0f; // theta the PREVIOUS forecast frame's lists were made for (0: it made none)
    uint64_t tf_frames = 0;     // frames that ran fw_k_fc_resolve + the streaming schedule instead of the look-back
    bool use_static_new = true;  // static output slots for new particles when all of them survive (FW_STATIC_NEW)
    bool use_stream = true;    // FW_STREAM=0: forecast frames keep the count-park-store kernel (A/B)
    // AABB fused into the update (fw_ctx_track_aabbs): per-tile boxes of the last update, valid while nothing touched
    // the state or the tile table since
    bool track_aabb = false;
    uint32_t boxes_epoch = 0;  // epoch of the update that left valid boxes (0 = none)
    bool colors_dirty = false; // some SegHost::colors_dirty is set
    bool use_fifo = true;      // FW_FIFO=0: constant-lifetime types take the general (compacting) path too (A/B, tests)
    bool fifo_nested = true;   // FW_FIFO_NESTED=0: ... those of spawners with Nested entries do (A/B)
    bool use_nospin = true;    // FW_NOSPIN=0: every type keeps its rotation plane (A/B)
    bool use_ageless = true;   // FW_AGELESS=0: no ring runs under the age rule (A/B in one build)
    // the cohort table of the latest ensure_ages: written in pinned memory, copied to the device in the stream of the kernel that reads
    // it; the fence is marked behind that kernel, main stream or side stream (the next table goes through the same pinned AND device words)
    struct CohortTable {
        Staging<char, 1> h;
        HipBuf<char> d;
        uint64_t launches = 0;  // fw_debug_age_launches / fw_debug_spin_launches
    };
    CohortTable age_tab;
    // the deferred spin of FIFO rings nobody reads (fw_spin.h).  FW_SPIN_DEFER=0: no ring defers (A/B in one build); spin_defer_min:
    // live particles from which a ring may (FW_SPIN_DEFER_MIN; the size from which a launch counts as bound by bandwidth);
    // spin_defer_after: qualifying launches in a row, with nobody asking for the planes, before the first deferred one
    // (FW_SPIN_DEFER_AFTER: a host that reads every few frames never pays a replay; 32 = the smallest power of two not below the cost of
    // one replay of the 1 M ring after a full lifetime unread over the kernel time a deferred frame saves, 72 us / 2.9 us, profiles/r19);
    // spin_log_cap: frames a ring may fall behind
    // (FW_SPIN_LOG: bounds the replay loop and the table).  The table and the log of the latest ensure_spin travel like the age table.
    bool use_spin_defer = true;
    uint32_t spin_defer_min = 384u * FW_TILE, spin_defer_after = 32u, spin_log_cap = 256u;
    CohortTable spin_tab;
    // FIFO launches none of whose ring tiles touches rotation or angular velocity run the kernel form compiled for that (FwFifoArgs::
    // spinless).  FW_SPINLESS=0: they keep the form that finds out per workgroup (A/B in one build)
    bool use_spinless = true;
    uint64_t spinless_launches = 0;  // fw_debug_spinless_launches
    // ... and their WHOLE ring tiles -- every slot a particle that lives through the launch (fw_fifo_tile_whole, fw_fuse2.h) -- take an arm of
    // the fused forms that issues all of a tile's loads first and never waits for a store (FwFifoArgs::fuse_pad[FW_FIFO_WHOLE], round 26).
    // FW_WHOLE_TILES=0: every tile keeps the streaming loop (A/B in one build).  whole_launches / whole_tiles: fw_debug_whole_tiles
    bool use_whole_tiles = true;
    uint64_t whole_launches = 0, whole_tiles = 0;
    // The particles a deferring launch spawns into the ring owe their spin to the log too (fw_spin_newborn_deferred, fw_spin.h; round 27):
    // the spawning workgroups run no spin step, the cohort points at the frame's own log entry.  FW_NEWBORN_SPIN=1: the eager rule of
    // rounds 19 to 26, in the host's pointer and the kernel's flag together (A/B in one build).  newborn_launches: fw_debug_newborn_spin
    bool newborn_spin = false;
    uint64_t newborn_launches = 0;
    // Up to fuse_depth frames of unread rings in one launch (fw_fuse2.h).  A frame whose only GPU work would be one spin-less
    // FIFO launch of rings that all deferred their spin in it -- each with at least fuse2_min live particles (FW_FUSE2_MIN: its own knob, the
    // default of spin_defer_min) -- is WITHHELD: all of its bookkeeping done, the complete launch kept here instead of enqueued.  The next
    // fw_step's launch takes it in when it qualifies too and the group passes the rule (fw_fuse_push): it runs the group -- or, while the
    // group is short of its depth, is withheld with it: `withheld` holds the GROUP so far, the fused launch of its frames.  The depth is two
    // frames; min(fuse_depth, FW_FUSE_NARROW) where every ring of the launch holds fuse_deep_min live particles (FW_FUSE_DEEP_MIN); and
    // fuse_depth (FW_FUSE_DEPTH, 2 .. FW_FUSE_MAX) where every ring holds fuse_wide_min as well (FW_FUSE_WIDE_MIN, round 24): a deeper group
    // pays where the pass over the planes dominates the launch.  (No depth above four has been measured between 768 tiles and the
    // headline's 983 333 particles: fuse_wide_min reuses fuse_deep_min's figure for want of another.)  Anything else that touches the
    // stream or particle state enqueues the group first (flush_withheld): one frame exactly as built, two to FW_FUSE_MAX - 1 as ONE fused launch.
    // FW_FUSE2=0: nothing is withheld.
    bool use_fuse2 = true;
    uint32_t fuse2_min = 384u * FW_TILE;
    uint32_t fuse_depth = FW_FUSE_MAX, fuse_deep_min = 768u * FW_TILE, fuse_wide_min = 768u * FW_TILE;
    // The far tier (round 32): a group may grow beyond FW_FUSE_MAX frames, up to fuse_far_depth (FW_FUSE_FAR_DEPTH, FW_FUSE_MAX .. FW_FUSE_FAR;
    // FW_FUSE_MAX: the tier is off), where fuse_depth is FW_FUSE_MAX (the knob unset, or 8), the launch takes the forms that defer their
    // newborns' spin (not FW_NEWBORN_SPIN=1: the tier has no eager kernels) and every ring of it holds fuse_far_min live particles
    // (FW_FUSE_FAR_MIN; 768 tiles like the two thresholds above, and as unmeasured between that and the headline's size).  In such a launch,
    // and in no other, a frame's op that continues the group's last op of its ring is merged into it (fw_op_continues, fw_withheld.h): the
    // launch carries FW_INLINE_OPS ops, so a ring with a still emitter reaches sixteen frames and one whose emitter moves every frame
    // closes at eight, as before.  (Below the threshold two rings with one op each close at four frames; above it they may reach sixteen.)
    uint32_t fuse_far_depth = FW_FUSE_FAR_DEFAULT, fuse_far_min = 768u * FW_TILE;
    FwWithheld withheld;  // (fw_withheld.h: the group and its transitions; launch_fifo offers, flush_withheld takes, drop_withheld drops)
    // fw_debug_fuse2: launches that ran two or more frames / withheld frames enqueued alone; fw_debug_fuse_frames: frames run by fused launches
    uint64_t fused_launches = 0, fuse2_flushed = 0, fuse_frames = 0;
    bool use_axis = true;      // FW_AXIS_SPIN=0: no ring runs under the axis-spin rule (A/B in one build)
    bool use_derived = true;   // FW_DERIVED=0: every type stores its scale / colour planes, attached instance buffer or not (A/B)
    // Round 6: scale, base colour and emissive colour are pure functions of (age, lifetime, initial_scale) (core.rs:601-605,
    // 652-655) -- the update of EVERY type whose curves fit the LDS staging stops storing them (36 of the 100 B a configs[2]
    // particle moved), not only of types with an attached instance buffer: the renderer extracts visible spawners only
    // (render.rs:382-403), the planes were written for nobody in every other frame.  FW_DERIVED=1: only with a buffer attached
    // (rounds 3-5; a share of the test functions keeps that form under the suite).
    bool derive_all = true;
    // Smallest (derived or given) capacity that makes a type a FIFO ring (FW_FIFO_MIN; the tests set 0).  Below a few
    // tens of thousands of particles a frame is launch latency whatever the path.  Next to compacting segments the ring
    // launch runs on its own stream (fifo_stream) and wins at any size (tools/fifo_threshold.py, tools/mixed_context.py);
    // where it cannot -- attached instance buffers, Nested spawners, a registered live-count ring -- the two launches of
    // a mixed context run one after the other and a small ring costs a few microseconds more than it saves.
    uint32_t fifo_small_tiles = 384;  // FIFO launches of a context with fewer four-round tiles than this use one-round tiles (FW_FIFO_SMALL)
    uint32_t fifo_min = 32768;
    // The segments of the context by update path (fw_update_path.h: n_in_use, n_fifo, n_range, n_few, n_spilled, n_small, n_small_ok,
    // n_small_coll, n_inst, n_solo and the few_blocked hysteresis).  Everybody reads its fields; it changes through SegPathEdit alone (below)
    FwPathCensus census;
    // A context with MORE one-lifetime types than one FIFO launch holds (round 5).  The ninth used to land on a range ring next to
    // eight FIFO rings: two kinds of launch per frame, one after the other -- 9 emitters of 22 000 particles 20.7 us per frame
    // where nine range rings take 13.2 (profiles/r04/few_small_emitters.txt).  Now the type that does not fit takes a range ring
    // AND every FIFO ring of the context becomes one where it stands (fifo_to_range: no copy, particles and order kept; build time,
    // the context is synchronised): one kind of launch again.  While such rings exist, further one-lifetime types join them.
    // ---- small types (SegHost::small): the wave-per-type kernel.  A type is one when it is built (or when it leaves a small ring:
    // drop_few_rings) if the emitters that feed it sustain at most small_max / 2 particles and nothing else claims it (no ring, no
    // Nested entry on or from it, no collisions, no instance buffer, no per-tile AABBs); it leaves for good when its live bound
    // passes small_max (it simply becomes a compacting segment: same buffers).  FW_SMALL=0 / FW_SMALL_MAX=n
    bool use_small = true;
    uint32_t small_max = 768;
    // The kernel pays from a few hundred small types on: a wave walks its type's list round by round, ~15.6 us per launch whatever the
    // number of types up to ~600, where a workgroup per type (the compacting kernels) takes 11.9 us for 96 types, 14.3 for 256, 18.9
    // for 512 (profiles/r05/mid_emitters_paths.txt).  The context runs its eligible types (SegHost::small_ok, n_small_ok of them) on
    // the kernel from small_min of them on and takes them off it again below three quarters of that (update_small_mode: when a
    // spawner is built or destroyed -- the context is synchronised then; the flag flips, nothing is copied).  FW_SMALL_MIN
    // WIDE types: emitters that sustain up to wide_max particles (hundreds of emitters of a thousand particles: two workgroups per
    // type on the compacting kernels, each a chain of tile table -> forecast -> count -> look-back) are walked by ONE workgroup of the
    // same kernel, the same launch; a narrow type whose bound passes small_max becomes a wide one, a wide one leaves the mode past
    // 2 x wide_max.  FW_WIDE_MAX; 0: no wide types
    // ... in contexts of wide_min eligible types or more (with the same hysteresis as small_min): 1024 x 600 / 1024 x 1000 particles 26 /
    // 31 us per launch against 29 / 53 on the compacting kernels, but 512 x 1500 24 against 20.5 (profiles/r05/wide_sweep.txt,
    // wide_ablations.txt): one workgroup walks a type's rounds one after the other, the compacting kernels spread them over several
    // workgroups -- which pays until those no longer fit the chip at once.  FW_WIDE_MIN
    // Types of up to wide_mid particles (four rounds of a workgroup) gain from a third of that on already: 256 x 600 14.9 against 16.8 us
    // per frame, 384 x 1000 19.3 against 23.1, 512 x 1000 20.3 against 25.6 (profiles/r05/mid_paths_sweep.txt); larger ones -- 1500
    // particles, six rounds -- lose up to 512 types (24.3 against 21.2) and win where the compacting launch no longer fits the chip.
    // Round 6 (tools/threshold_sweep.py, tools/r06_wave_vs_workgroup.py): from about as many types as the chip has SIMDs (1024) a WAVE per
    // type beats a WORKGROUP per type at EVERY size the kernel takes -- 1024 x 1000 particles 23.2 against 34.8 us per frame, 2048 x
    // 1000 39.1 against 58.0, 2048 x 2000 58.6 against 85.9, 1024 x 300 20.3 against 28.5 -- while at 512 types the workgroup wins from
    // 1000 particles on (16.4 against 19.1) and 768 types are a draw (profiles/r06/wave_vs_workgroup.txt): every SIMD holds a wave
    // of its own either way, and the workgroup form pays a barrier and an LDS exchange per round for parallelism nobody lacks.  From
    // wave_all_min eligible types on (off again below five sixths of it) the wide types of the context are laid out in the wave
    // role: the same kernel, the same launch, only the list's partition (FwSmallArgs::n_narrow) moves.  FW_WAVE_ALL_MIN; 0: never
    uint32_t wave_all_min = 896;
    bool wave_all_on = false;
    uint32_t wide_min = 768;
    bool wide_on = false;      // wide types of more than wide_mid particles run on the kernel
    bool wide_mid_on = false;  // ... those of up to wide_mid do
    uint32_t wide_mid = 1400;
    uint32_t wide_max = 2048;
    uint32_t n_narrow = 0;   // of small_list (narrow types first)
    uint32_t small_min = 352;
    // In frames that run the collision passes (materialise -> count -> scan -> update: four dependent launches on the main stream, 49 us
    // for a destroy_on_collision type of 20 000 particles) the small launch -- which touches nothing those passes touch -- runs next to
    // them on the ring stream (fifo_stream): 512 / 2048 small emitters next to such a type 66.9 / 84.3 -> 53.1 / 67.3 us per frame
    // (profiles/r05/nested_among_small_side.txt).  Not in frames whose separate passes are a Nested entry's only: those are bound by the
    // host's launches, and the extra event costs more than the overlap gives (44.4 -> 48.0).  Under the rules of a ring launch there:
    // own stream only, no live-count ring, no colliding small type (a new collider set travels in the main stream), not in a frame that
    // re-sends the list (a type left the mode: the compacting launch of this very frame updates it).
    // Its op table is then recycled by an event on that stream, not by the main stream's "frame started" word.
    bool small_last_side = false;
    bool small_on = false;
    // ... and the host half of their frames (thousands of emitters: the frame is bound by the cache lines fw_step streams).
    // A SOLO segment (SegHost::solo: a small type with one Global feeder) is not visited by the per-segment pass at the start of a
    // frame: what that pass does for it -- expire the lifetime window, tighten the bound -- happens in the spawner loop, right
    // before its op is made, and its frame_spawn stays 0 (its one op of the frame carries the count).  The pass walks `big_list`
    // (every other segment in use) instead of the segment array.  A segment becomes solo in the first frame-begin pass after it
    // became small, never before (the pass still owes it one ordinary frame begin).  FW_HOST_FAST=0: no solo segments, no ops
    // written in place (OpList).
    bool host_fast = true;
    std::vector<uint32_t> big_list;
    bool big_dirty = true;
    std::vector<uint32_t> small_list;   // the segments, ascending (rebuilt when small_dirty)
    bool small_dirty = true;
    HipBuf<uint32_t> d_small, h_small;  // device list / pinned staging
    size_t small_cap = 0;               // (of both)
    Fence small_fence;                  // (of h_small)
    std::vector<FwOp> fifo_ops;  // this frame's Global ops that feed FIFO segments (spawned inside fw_k_update_fifo)
    std::vector<std::pair<uint32_t, FwOp>> range_mat_ops;  // the same for range rings other particles' entries emit from
    std::vector<std::pair<uint32_t, FwOp>> fifo_mat_ops;  // {emission index, op}: rings of spawners with Nested entries -- the
                                                         // Nested pass of the frame, if there is one, must find them in memory
    uint64_t tev_frames = 0;   // frames timed so far (a frame may take several update launches)
    // ---- range rings (SegHost::range)
    bool use_range = true;       // FW_RANGE=0: lifetime-range types take the compacting path (A/B, tests)
    uint32_t range_min = 8192;   // smallest capacity that makes one (FW_RANGE_MIN; the tests use 0): a range ring costs a
                                 // small segment three workgroups where the compacting path needs one.  Swept on many equal
                                 // emitters (profiles/r04/range_min_sweep.txt): 8192 is where the one-round tiles start to win
    // A context with FEW segments -- the reference's own regime: examples/sparks.rs is one spawner of ~730 particles -- runs a small
    // type on a range ring too: one emitter of 733 particles 13.2 -> 9.1 us per frame, 8-64 such emitters 16 -> 10-11
    // (profiles/r04/few_small_emitters.txt), where with thousands of small emitters the compacting path wins (range_min above).
    // Up to range_few segments in use, no FIFO ring among them (a FIFO launch and a range launch run one after the other), such a
    // type becomes a range ring whatever its size (SegHost::few_ring); the spawner that takes the context past either condition
    // sends those rings to the compacting path (drop_few_rings: build time, the context is synchronised).  FW_RANGE_FEW; 0: off
    uint32_t range_few = 192;  // (64 until the range launch read its records from device memory: profiles/r05/mid_emitters_paths.txt)
    // A range launch whose rings hold fewer than range_small_tiles four-round tiles in all (FW_RANGE_SMALL; not with a ring whose
    // count only the device knows), or with a colliding ring, runs on OLD / YOUNG tiles of ONE round (fw_k_update_range: TR): a
    // quarter of hysteresis, a change re-sends the table.
    uint32_t range_small_tiles = 384;
    bool range_small = false;
    // Rounds of the YOUNG workgroups of a four-round launch, chosen per launch (round 5): tiles of 512 slots (2) when the range
    // rings of the context hold range_young_big particles each or more on average (hysteresis of a quarter; a change re-sends the
    // table), 1024 (4) otherwise and always with an attached instance buffer.  FW_RANGE_YOUNG_BIG=n (0: never).
    // Round 6: never -- with 56 instead of 100 bytes per particle a 512-slot tile keeps too few bytes in flight (configs[2] 199 us per
    // frame on 512-slot tiles, 185 on 1024-slot ones; 2048-slot ones -- FW_RANGE_YR=8 -- lose 2 %); the rule of round 5 was 32768.
    uint32_t range_young_rounds = 4;
    uint32_t range_young_big = 0;
    std::vector<FwOp> range_ops;  // this frame's Global ops that feed range rings
    // age, BEFORE the current frame's update, of a particle born in frame f -- the same for every segment of the context:
    // born with age 0, then one fp32 addition per frame (core.rs:594), exactly the device's additions
    struct BirthAge {
        uint64_t frame;
        float age;
    };
    std::deque<BirthAge> birth_age;  // oldest first; only frames some range ring may still hold young particles of
    float range_life_max = 0.f;      // largest SegHost::range_life_lo in the context
    float range_age_keep = 0.f;      // largest lifetime.max of a range ring that receives Nested children (plus a margin)
    HipBuf<FwRangeDesc> d_rdesc;     // device table: one descriptor per workgroup of the range launch
    HipBuf<FwRangeDesc> h_rdesc;     // pinned staging of it
    size_t rdesc_cap = 0;            // (of both and d_rstatus)
    uint32_t r_total = 0;            // workgroups of the range launch
    bool r_force = true;             // a range segment was (re)built: re-send the table
    Fence rtab_fence;                // (of h_rdesc)
    HipBuf<unsigned long long> d_rstatus;     // look-back words of the OLD workgroups
    HipBuf<char> h_rparam[kParamRing];        // per-frame records + ops, written by the host, read by the kernel in place
    // ... in DEVICE memory the host writes through the large BAR (fine-grained, hipExtMallocWithFlags) when the platform maps it, in
    // pinned host memory otherwise: a workgroup's record is the first thing its loads depend on, and read over the bus it costs
    // every launch ~3 us of dead time (tools/barwrite.hip, profiles/r05/rparam_ab.txt: one sparks.rs emitter 8.9 -> 5.7 us per frame,
    // one GPU's share of configs[4] 90.3 -> 85.9, configs[2] 318 -> 311).  The host only ever WRITES such a buffer (write-combining
    // stores, a fence, one read-back of the last word before the launch: posted writes may not pass it).  FW_PARAM_BAR=0: pinned.
    bool param_bar = false;
    // ... and so do op TABLES of at most kBarParamBytes (a few hundred emitters on the compacting / wave-per-type launches: their
    // workgroups read a header and an op each before they can spawn); larger tables stay in pinned memory, written in place
    // (OpList): with thousands of emitters the frame is bound by the host, and write-combining stores cost it more than cached ones
    HipBuf<char> b_param[kParamRing];
    bool range_spread_new = true;   // FW_RANGE_SPREAD_NEW=0: a segment's NEW workgroups all in front of its YOUNG ones (A/B)
    // An in-place ring launch (FIFO / range) that streams more than nt_bytes uses the fully non-temporal form of its kernel:
    // several times the 256 MiB Infinity Cache, where allocating lines that cannot survive until the next frame only costs.
    // One that streams more than nt_wo_bytes -- no longer all of it fits -- stores the planes no update reads back (scale,
    // colours) non-temporally, so that the cache keeps what the next frame reads (fw_dev.h: fw_ld4w; knobs FW_NT_MB=n,
    // FW_NT_WO_MB=n: 0 = always)
    uint64_t nt_bytes = 768ull << 20;  // (crossover measured at 0.65-0.85 GB for both kernels: profiles/r03/nt_sweep.txt)
    // (the write-only form measured over 50-970 MB, profiles/r03/nt_sweep_wo.txt: range rings gain from the smallest size on
    // (-1..4 % below 250 MB, -10..16 % at 320-425 MB); the FIFO kernel's non-temporal forms carry the generic write mask, which
    // costs 1-2 % where everything fits the cache, and gain from ~300 MB on (-10..16 % at 480-650 MB))
    uint64_t nt_wo_bytes = 280ull << 20, nt_wo_bytes_range = 64ull << 20;
    HipBuf<unsigned long long> d_rts;     // FW_DEBUG & 8: per-workgroup timestamps of the last range launch
    std::vector<uint32_t> range_scratch;
    size_t rparam_bytes = 0;
    uint64_t rslot_frame[kParamRing] = {};    // frame that last used the slot (+1; 0 = free)
    uint64_t rring_seq = 0;
    uint64_t r_uploads = 0;  // times the range table was re-sent (FW_HOST_PROF prints it)

    uint32_t nest_seq = 0;  // launches of fw_k_nest so far (tag of their look-back words)
    // Nested entries whose two particle types live in FIFO rings of one launch run INSIDE that launch (fw_kernels.h: FwFifoNest):
    // a steady configs[3] frame is ONE launch instead of fw_k_nest + a gap + the update.  FW_NEST_FUSE=0: always the separate pass
    bool nest_fuse = true;
    uint64_t fused_nest_frames = 0, nest_pass_frames = 0;  // frames of either kind so far (fw_debug_nest_frames)
    // FW_HOST_PROF=1: time spent in the sections of fw_step's host half (printed when the context is destroyed)
    bool trace = false;  // FW_TRACE
    bool host_prof = false;
    uint64_t host_prof_skip = 0;  // FW_HOST_PROF=n (n > 1): frames to skip first (fill, table uploads)
    double prof_ns[10] = {};
    uint64_t prof_frames = 0;
    uint64_t frame = 0;
    double sim_time = 0.0;  // sum of the dt of every step so far (lifetime windows)
    uint32_t parity = 0;
    unsigned long long stats_before_last = 0;
    bool stats_valid = false;

    // kernel timing
    bool timing = false;
    std::vector<HipEvent> tev;
    size_t tev_used = 0;
    uint64_t timing_particles_start = 0;
    double tev_overhead_ms = 0;  // duration of an empty hipEvent pair on this stream

    unsigned long long *live_ring = nullptr;  // caller-owned device ring of per-frame live totals
    uint32_t live_ring_n = 0;
    uint64_t live_ring_frames = 0;            // frames written since the ring was registered

    HipBuf<FwCollider> d_colliders;     // device-resident analytic colliders (fw_ctx_set_colliders)
    uint32_t n_colliders = 0;
    // a new set travels as ONE copy in the context's stream (ordered behind the frames that read the old set, in front of the
    // frames that will read the new one: no synchronisation)
    Staging<FwCollider, 2> h_coll;
    // collider meshes (fw_engine_mesh.cpp): the meshes behind fw_mesh handles, and the instance set, staged and copied like the
    // analytic set
    struct MeshHost {
        bool alive = false;
        HipBuf<float4> nodes, tris;  // fw_bvh.h layout
        uint32_t n_nodes = 0, n_tris = 0;
        float center[3] = {0.0f, 0.0f, 0.0f}, radius = 0.0f;  // a sphere that contains the mesh, in its own frame
        // a deformable mesh (fw_ctx_create_deformable_mesh) keeps what fw_ctx_update_mesh_vertices needs: the refit's tables
        // (fw_refit.h) and the device vertices; the new vertices are staged in pinned memory and travel as one copy in the
        // context's stream like an instance set.  All of it is allocated at creation: an update allocates nothing.
        bool deformable = false;
        uint32_t n_vertices = 0;
        HipBuf<FwSlotIdx> slots;
        HipBuf<uint32_t> order, level_off;
        HipBuf<float> xyz;
        Staging<float, 2> h_xyz;
        std::vector<uint32_t> h_level_off;  // the host's copy: which levels get a launch of their own (fw_launch_mesh_refit)
        std::vector<uint8_t> referenced;    // per vertex: some triangle uses it (the pad and the bounding sphere go by these)
        float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f}, pad = 0.0f;  // the root's padded box and the pad, as the host last knew them
        // vertices from device memory (fw_ctx_update_mesh_vertices_device): what the device then has to find out itself.  Allocated
        // and uploaded by the mesh's FIRST such call (kMeshDeviceAllocs allocations), not at creation; later calls allocate nothing.
        HipBuf<FwMeshRecord> d_rec;        // bounds, pad, rejected flag, counts (fw_mesh_bounds.h)
        HipBuf<FwVtxAcc> d_partials;       // one per workgroup of fw_k_mesh_bounds
        HipBuf<uint8_t> d_referenced;      // `referenced` on the device
        HipBuf<FwMeshReport> h_report;     // pinned: the counts as the device last stored them (fw_ctx_mesh_update_status)
        // the bounds are the device's (d_rec) since a device-form update; center / radius / lo / hi above are stale until a
        // host-form update takes them back.  stage_instances then stages the mesh's instances as never skipped and has
        // fw_k_mesh_spheres fix them behind the copy.
        bool dev_bounds = false;
        uint64_t sphere_stamp = 0;  // stage_instances: the instance set (fw_ctx::h_mesh_inst.turn) this mesh's sphere launch was last enqueued for
    };
    static constexpr int kMeshDeviceAllocs = 4;  // d_rec, d_partials, d_referenced, h_report
    std::vector<MeshHost> meshes;
    std::vector<fw_mesh> mesh_set;  // the meshes the current instance set places (fw_ctx_destroy_mesh refuses them)
    std::vector<fw_mesh_collider> mesh_insts;  // ... and the set itself as the caller gave it: restaged when a placed mesh deforms
    HipBuf<FwMeshInst> d_mesh_inst;
    Staging<FwMeshInst, 2> h_mesh_inst;
    // the host forms of the queries (fw_engine_query.cpp: query_staged): pinned staging and device buffers for the input and the
    // output records, grown on demand and kept; the device forms need nothing of their own
    HipBuf<float4> q_in_h, q_out_h, q_in_d, q_out_d;
    HipBuf<float4> q_out2_h, q_out2_d;  // ... and for the optional second output (the path query's samples): untouched until one is asked for
    HipBuf<float> d_aabb;      // 256 partial boxes of the AABB query
    HipBuf<float> h_aabb;      // pinned result {min.xyz, any, max.xyz, -}
    // the batched boxes (fw_ctx_aabbs[_device]; fw_boxes.h): the entry and place tables of a call travel as ONE copy in the context's
    // stream, staged like a collider set; the scratch of partial boxes and the host form's pinned records only ever grow (growing is
    // the one case in which the device form waits)
    struct {
        Staging<char, 2> h_tab;
        HipBuf<char> d_tab;
        HipBuf<float> d_part;              // one partial box {min.xyz, -, max.xyz, -} per chunk
        HipBuf<float> h_out;               // pinned: the fw_aabb records of the host form
        std::vector<uint32_t> place_first; // per-call scratch: the first entry of every output place
        uint64_t launches = 0, last_chunks = 0;  // fw_debug_aabb_batch
    } boxes;
    // the volume queries (fw_ctx_count_in_volumes[_device]; fw_volumes.h): their tables and volume records travel through boxes.h_tab /
    // boxes.d_tab -- the same plan, one slot per call whoever makes it; the scratch of per-chunk counts ([volume][chunk] words) and the
    // host form's pinned counts are their own and only ever grow
    struct {
        HipBuf<uint32_t> d_part;
        HipBuf<uint32_t> h_out;
        uint64_t launches = 0, last_chunks = 0;  // fw_debug_volume_query
    } volumes;
    HipBuf<unsigned long long> d_total;
    HipBuf<uint32_t> d_segids;

    // `ab` build, FW_FAIL_ALLOC=k: the k-th allocation of the context fails (hipErrorOutOfMemory, no HIP call) -- the failure paths
    // under test
    uint64_t fail_alloc = 0, n_alloc = 0;

    fw_ctx() = default;
    fw_ctx(const fw_ctx &) = delete;
    fw_ctx &operator=(const fw_ctx &) = delete;
    ~fw_ctx();  // waits for the context's streams; the members then release themselves
};

namespace fwh {


#define FW_HIP(ctx, call)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return FW_EHIP;                                                                          \
        }                                                                                            \
    } while (0)

inline fw_status fail(fw_ctx *ctx, fw_status s, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return s;
}

inline uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

// the device state changed under the host: the survivor forecast of the previous frame and the per-tile boxes describe it no longer
inline void drop_forecast_and_boxes(fw_ctx *ctx) { ctx->fc_ok = false, ctx->boxes_epoch = 0; }

// ---- which update path a segment is on (fw_update_path.h): the context's knobs as the rule reads them, a segment's share of the census,
// and the ONE way that share changes
inline FwPathPolicy path_policy(const fw_ctx *ctx) {
    FwPathPolicy p;
    p.use_fifo = ctx->use_fifo, p.fifo_min = ctx->fifo_min, p.fifo_nested = ctx->fifo_nested, p.fifo_small_tiles = ctx->fifo_small_tiles;
    p.use_ageless = ctx->use_ageless, p.use_range = ctx->use_range, p.range_min = ctx->range_min, p.range_few = ctx->range_few;
    return p;
}
inline uint32_t path_bits(const SegHost &S) {
    return (S.in_use ? FW_PATH_IN_USE : 0u) | (S.fifo ? FW_PATH_FIFO : 0u) | (S.range ? FW_PATH_RANGE : 0u) | (S.few_ring ? FW_PATH_FEW_RING : 0u) |
           (S.spilled ? FW_PATH_SPILLED : 0u) | (S.small ? FW_PATH_SMALL : 0u) | (S.small_ok ? FW_PATH_SMALL_OK : 0u) |
           (S.collides ? FW_PATH_COLLIDES : 0u) | (S.inst != nullptr ? FW_PATH_INST : 0u) | (S.solo ? FW_PATH_SOLO : 0u);
}
// Whoever changes one of the SegHost flags path_bits reads does so inside the scope of one of these: the segment's share leaves the
// census when the scope opens and comes back, as the flags then stand, when it closes -- on every way out, a failure's included, which is
// what lets release_spawner_segments undo a build that stopped half-way.  Dirty flags (tab_force, r_force, ...) stay with the site.
class SegPathEdit {
public:
    SegPathEdit(fw_ctx *ctx, const SegHost &S) : census_(ctx->census), S_(S) { (void)census_.remove(path_bits(S_)); }
    SegPathEdit(const SegPathEdit &) = delete;
    SegPathEdit &operator=(const SegPathEdit &) = delete;
    ~SegPathEdit() { census_.add(path_bits(S_)); }

private:
    FwPathCensus &census_;
    const SegHost &S_;
};
// ... but for fw_step's frame-begin pass, which makes a small type with one feeder a solo one (segment_pass): one increment
inline void seg_becomes_solo(fw_ctx *ctx, SegHost &S) { S.solo = true, ctx->census.add(FW_PATH_SOLO); }

// The one allocation call of the engine: `bytes` of `kind` memory (fw_ctx::fail_alloc: the `ab` build's simulated failure).
inline hipError_t hip_alloc(fw_ctx *ctx, void **p, size_t bytes, Mem kind, const char **call) {
    *p = nullptr;
    *call = kind == Mem::device ? "hipMalloc" : kind == Mem::fine ? "hipExtMallocWithFlags" : "hipHostMalloc";
    if (ctx->fail_alloc && ++ctx->n_alloc == ctx->fail_alloc) {
        fprintf(stderr, "[fw] FW_FAIL_ALLOC: allocation %llu fails\n", (unsigned long long)ctx->n_alloc);
        return hipErrorOutOfMemory;
    }
    return kind == Mem::device ? hipMalloc(p, bytes)
           : kind == Mem::fine ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained)
                               : hipHostMalloc(p, bytes, hipHostMallocDefault);
}

// `b` gets a fresh buffer of n elements of `kind` memory, zeroed on request; what it held is released first.  A failure leaves
// it empty and returns FW_EHIP with the failing call's text.  `view` (a FwGlobals pointer) follows the buffer either way.
template <typename T, typename V = T>
fw_status alloc_buf(fw_ctx *ctx, HipBuf<T> &b, size_t n, Mem kind = Mem::device, bool zero = false, V **view = nullptr) {
    b.reset();
    if (view) *view = nullptr;
    void *p = nullptr;
    const char *call = "";
    hipError_t e = hip_alloc(ctx, &p, n * sizeof(T), kind, &call);
    if (e == hipSuccess) {
        b.adopt(p, n, kind);
        if (zero && kind == Mem::device) e = fw_memset_done(p, 0, n * sizeof(T)), call = "hipMemset";
        if (zero && kind != Mem::device) memset(p, 0, n * sizeof(T));  // (the host writes pinned and BAR memory itself)
    }
    if (e != hipSuccess) {
        b.reset();
        return fail(ctx, FW_EHIP, std::string(call) + "(" + std::to_string(n * sizeof(T)) + " bytes): " + hipGetErrorString(e));
    }
    if (view) *view = b.get();
    return FW_OK;
}

// `b` (device memory) moves to a new buffer of n elements, zeroed on request, that starts with its first `used` elements.  A
// failure leaves it as it was (FW_EHIP with the failing call's text).
template <typename T, typename V = T>
fw_status grow_buf(fw_ctx *ctx, HipBuf<T> &b, size_t n, bool zero, size_t used, V **view = nullptr) {
    HipBuf<T> nb;
    fw_status st = alloc_buf(ctx, nb, n, Mem::device, zero);
    if (st) return st;
    if (used) FW_HIP(ctx, hipMemcpy(nb.get(), b.get(), used * sizeof(T), hipMemcpyDeviceToDevice));
    b = std::move(nb);
    if (view) *view = b.get();
    return FW_OK;
}

inline fw_status Fence::wait_pending(fw_ctx *ctx) {
    FW_HIP(ctx, hipEventSynchronize(ev_));
    pending_ = false;
    return FW_OK;
}
inline fw_status Fence::mark(fw_ctx *ctx, hipStream_t stream) {
    if (!ev_) FW_HIP(ctx, ev_.create());
    FW_HIP(ctx, hipEventRecord(ev_, stream));
    pending_ = true;
    return FW_OK;
}

fw_status sync(fw_ctx *ctx);  // (fw_engine_mem.cpp)
// the withheld frames (fw_ctx::withheld) go to the stream -- one exactly as built, two to FW_FUSE_MAX - 1 as one fused launch --: before anything else that
// touches the stream or particle state
fw_status flush_withheld(fw_ctx *ctx);  // (fw_engine_launch.cpp)
// ... or is dropped with the particles it would have updated (the spawner is rebuilt, the context destroyed)
void drop_withheld(fw_ctx *ctx);
template <typename T, int N>
fw_status Staging<T, N>::take(fw_ctx *ctx, size_t n, size_t grow_to, T **out, HipBuf<T> *dev) {
    HipBuf<T> &b = h[turn % N];
    fw_status st = fence[turn % N].wait(ctx);
    if (st) return st;
    if (n > (dev ? std::min(b.cap(), dev->cap()) : b.cap())) {
        if (dev && (st = sync(ctx))) return st;
        if ((st = alloc_buf(ctx, b, grow_to, Mem::pinned)) || (dev && (st = alloc_buf(ctx, *dev, grow_to)))) return st;
    }
    if (out) *out = b;
    return FW_OK;
}
template <typename T, int N>
fw_status Staging<T, N>::commit(fw_ctx *ctx, hipStream_t stream) {
    fw_status st = fence[turn % N].mark(ctx, stream);
    if (!st) turn++;
    return st;
}

// The epoch of frame f: the tag of every word its launches publish (snapshot rows, cohort reports, forecast sums) -- 30 bits, never 0
inline uint32_t frame_epoch(uint64_t f) {
    const uint32_t e = (uint32_t)((f + 1) & 0x3FFFFFFFu);
    return e ? e : 1u;
}

// Cohort reports (SegHost::h_report): the update of frame f leaves {epoch, size of the cohort it added} in row f % kReportRing.
inline bool report_landed(const SegHost &S, uint64_t f) {
    const volatile unsigned long long *row = S.h_report + (f % kReportRing);
    return (uint32_t)(*row >> 32) == frame_epoch(f);
}
// ... spins a while for the row; false: still missing (what a wait for the stream costs, and what a row missing after it means,
// is the caller's to decide)
inline bool wait_report(const SegHost &S, uint64_t f) {
    const volatile unsigned long long *row = S.h_report + (f % kReportRing);
    const uint32_t ep = frame_epoch(f);
    for (int spin = 0; (uint32_t)(*row >> 32) != ep && spin < 100000; spin++) __builtin_ia32_pause();
    return (uint32_t)(*row >> 32) == ep;
}

// age of a particle born in frame f before this frame's update (fw_ctx::birth_age: one entry per frame, contiguous)
inline float birth_age_before(const fw_ctx *ctx, uint64_t f) {
    if (ctx->birth_age.empty() || f < ctx->birth_age.front().frame) return INFINITY;  // (long graduated)
    const size_t i = (size_t)(f - ctx->birth_age.front().frame);
    return i < ctx->birth_age.size() ? ctx->birth_age[i].age : 0.0f;  // this frame's own cohort: born with age 0
}

struct OpHdr {  // FwUpdateArgs::seg_op_first: per segment {first op, one past its last, particles they spawn in all, 0}
    uint32_t o0, o1, n, pad;
};

// One frame of fw_step, on the stack: what its plan (fw_engine_step.cpp) hands its enqueue (fw_engine_launch.cpp), and what the
// phases of the enqueue hand each other.  The plan can still be rolled back; nothing of the enqueue can.
struct FwFrame {
    float dt = 0.f;
    uint32_t dt_bits = 0;
    uint32_t p = 0;  // parity of the frame's input buffers
    uint32_t n_seg = 0, total_tiles = 0;
    bool new_static = false;  // cleared by any Global op whose particles might not survive this step
    // (noted by the first pass over the segments: whether a particle type collides, whether a compacting segment has an
    // instance buffer attached, and what decides the tile size of the ring launches)
    bool any_coll = false, any_inst_general = false;
    struct {
        uint64_t fifo_parts = 0, range_parts = 0;
        bool fifo_dev = false, fifo_coll = false, fifo_inst = false, range_dev = false, range_coll = false, range_inst = false;
    } ring_stats;
    // the op table the spawner loop writes in place, in a parameter slot taken before it (fw_engine_step.cpp: take_op_slot)
    int pre_slot = -1;
    OpHdr *pre_hdr = nullptr;
    size_t pre_tracked = 0;  // ops of levels[0].g whose headers are up to date
    bool pre_hdr_ok = false;
    size_t n_g = 0, n_n = 0;  // the frame's Global / Nested ops
    bool nested_frame = false;  // some emission level holds a Nested op
    bool fuse = false;          // ... and they all run inside the FIFO launch (plan_fuse)
    FwNestOp fuse_plan[FW_FIFO_NEST_MAX];
    uint32_t n_fuse = 0;
    int frame_mode = FW_MODE_FUSED;
    bool legacy = false;    // the separate spawn / nest passes run
    bool fc_frame = false;  // the general launch leaves a survivor forecast for the next frame
    FwUpdateArgs a{};
    FwInlineOps inl;
    int spawn_form = FW_SPAWN_NONE;
    int slot = -1;  // the parameter slot the main stream's launches read, recycled by an event at the end of the frame
    // the op table of the small launch (fw_k_update_small): the frame's table in Global-only frames, one of its own in frames that
    // run the separate passes
    const uint4 *small_hdr = nullptr;
    const FwOp *small_ops = nullptr;
    int small_tslot = -1;  // ... the parameter slot it lives in, in the latter case
    int snap = -1;         // the snapshot row the frame's launches fill (-1: none)
    bool timed = false;    // a launch of the frame carries a timing pair
    bool fifo_launched = false, range_launched = false, small_launched = false;
    bool quiet = false;  // the frame's only GPU work can be one FIFO launch: it may be withheld, or take the withheld one in (enqueue_frame)
    std::chrono::steady_clock::time_point prof_t;
    // FW_HOST_PROF: the time since the previous point goes to column i
    void prof(fw_ctx *ctx, int i) {
        if (!ctx->host_prof) return;
        const auto now = std::chrono::steady_clock::now();
        if (ctx->frame < ctx->host_prof_skip) {
            prof_t = now;
            return;
        }
        ctx->prof_ns[i] += std::chrono::duration<double, std::nano>(now - prof_t).count();
        prof_t = now;
    }
};

// ---- shared functions (definitions: see the list of translation units above; sync: declared above Staging::take)
fw_status join_side(fw_ctx *ctx);
// a FIFO ring whose age plane is stale (SegHost::ages_stale) gets it written back; stream: where the kernel goes -- null: the main
// stream, which first waits for the ring launches on the side stream (join_side)
fw_status ensure_ages(fw_ctx *ctx, uint32_t si, hipStream_t stream = nullptr);
bool ageless_dt_ok(float dt);
// ... and a FIFO ring whose spin is deferred (SegHost::spin) gets its log replayed.  keep_streak: the log reached its cap -- the ring
// goes on deferring; everybody else asks because the planes are wanted, and the ring has to earn the rule again (spin_defer_after)
fw_status ensure_spin(fw_ctx *ctx, uint32_t si, hipStream_t stream = nullptr, bool keep_streak = false);
bool spin_dt_ok(float dt);
fw_status ensure_max_seg(fw_ctx *ctx, uint32_t need);
uint32_t seg_live_tiles(const SegHost &s);
uint32_t seg_tiles(const SegHost &s, uint32_t vt_rounds = 1);
fw_status ensure_tile_arrays(fw_ctx *ctx);
fw_status ensure_range_arrays(fw_ctx *ctx);
uint32_t ring_head_exact(const SegHost &S, uint32_t count);
FwSegView seg_view(const fw_ctx *ctx, uint32_t si, uint32_t parity);
FwSegView seg_view_exact(const fw_ctx *ctx, uint32_t si, uint32_t parity, uint32_t count);
fw_status ensure_param_ring(fw_ctx *ctx, size_t bytes);
fw_status wait_slot_free(fw_ctx *ctx, uint64_t &tag);
fw_status acquire_slot(fw_ctx *ctx, int *out);
fw_status ensure_ring(fw_ctx *ctx, FwFrame &fr, size_t bytes);
fw_status enqueue_frame(fw_ctx *ctx, FwFrame &fr);
fw_status upload_seg(fw_ctx *ctx, uint32_t si);
fw_status alloc_seg_buffers(fw_ctx *ctx, const SegHost &s, uint32_t capacity, bool ring, bool want_destroyed, SegBufs &out);
fw_status refresh_rold(fw_ctx *ctx);
fw_status refresh_counts_exact(fw_ctx *ctx);
fw_status check_device_errors(fw_ctx *ctx);
fw_status realloc_segment(fw_ctx *ctx, uint32_t si, uint32_t ncap, bool make_general);
fw_status grow_segment(fw_ctx *ctx, uint32_t si, uint32_t need, bool at_least_double = true);
bool nested_fed_wants_growth(const SegHost &S);
fw_status fifo_to_general(fw_ctx *ctx, uint32_t si);
bool small_eligible(const fw_ctx *ctx, const SegHost &S);
void enter_small(fw_ctx *ctx, SegHost &S);
void leave_small(fw_ctx *ctx, SegHost &S);
void update_small_mode(fw_ctx *ctx);
void small_deactivate(fw_ctx *ctx, SegHost &S);  // off the kernel, still eligible (update_small_mode; a narrow type that became wide while wide_on is off)
fw_status drop_few_rings(fw_ctx *ctx);
bool fifo_may_become_range(const fw_ctx *ctx, const SegHost &S);
fw_status fifo_to_range(fw_ctx *ctx, uint32_t si);
fw_status spill_fifo_rings(fw_ctx *ctx);
fw_status leave_nospin(fw_ctx *ctx, uint32_t si);
bool axis_dt_ok(const SegHost &S, float dt);
fw_status set_derived(fw_ctx *ctx, uint32_t si, bool on, bool refill = true);
// the live count of segment si, as the kernels keep it, at the current parity (si = 0: the row of all segments)
static inline uint32_t *count_slot(const fw_ctx *ctx, uint32_t si = 0) { return ctx->g.count + (size_t)ctx->parity * ctx->max_seg + si; }
// does the type's update leave scale and colours to its readers?  (colliding types -- and `bigkeys` ones, which run on their
// kernels -- stay as they are: the feature path reads the stored planes)
static inline bool wants_derived(const fw_ctx *ctx, const SegHost &S) {
    return ctx->use_derived && !S.collides && (ctx->derive_all || S.inst != nullptr);
}
fw_status grow_nested_children(fw_ctx *ctx, SpawnerHost &sp, uint32_t parent_type, int depth = 0);
void copy_curve(CurveCopy &dst, int32_t kind, int32_t n, const float *times, const float *values, int stride);
fw_status validate_desc(fw_ctx *ctx, const fw_spawner_desc *d);
uint32_t derive_capacity(const fw_spawner_desc *d, uint32_t t, const std::vector<uint32_t> &caps, double *expect_live = nullptr);
void fill_randvec3(const fw_rand_vec3 &r, float &mn, float &mx, float &spread, float dir[4], float arc[4]);
uint32_t pad4(uint32_t n);
fw_status build_spawner(fw_ctx *ctx, int h, const fw_spawner_desc *d, const std::vector<uint64_t> *carry_serial);
fw_status release_spawner_segments(fw_ctx *ctx, SpawnerHost &sp);
fw_status update_tile_table(fw_ctx *ctx);
fw_status upload_range_table(fw_ctx *ctx, uint32_t n_seg);
bool poll_device_error(fw_ctx *ctx);
fw_status poisoned_status(fw_ctx *ctx);
fw_status poison_segment(fw_ctx *ctx, uint32_t si, const std::string &what);
SpawnerHost *get_spawner(fw_ctx *ctx, fw_spawner h);
void poll_snapshots(fw_ctx *ctx);
fw_status read_counts(fw_ctx *ctx, std::vector<uint32_t> &out);
bool spawner_active(const fw_ctx *ctx, const SpawnerHost &sp, const std::vector<uint32_t> &counts);

}  // namespace fwh
