// fw_k_aux.hip -- readback / upload (AoS <-> planes), plane fills, render hand-off (fw_k_pack, fw_k_depth_keys), AABB queries, live totals, the copy-bandwidth probe
// (gfx950 only; device helpers in fw_dev.h, launch interface in fw_kernels.h)
#include "fw_dev.h"
#include "fw_ages.h"
#include "fw_spin.h"
#include "fw_sort.h"
#include "fw_boxes.h"
#include "fw_volumes.h"

// ---------------------------------------------------------------------------------
// readback / upload / render hand-off helpers
// ---------------------------------------------------------------------------------

// ---- a segment through its view (FwSegView, fw_kernels.h): the ONE place the readers below decode a segment's storage
// slot of particle 0 (a range ring -- d_rold -- keeps the size of its old part on the device: FwGlobals::rold) ...
__device__ __forceinline__ uint32_t fw_view_head(const FwSegView &v) {
    return v.d_rold ? fw_range_head(v.head, *v.d_rold, v.capacity) : v.head;
}
// ... and of particle li, given that one
__device__ __forceinline__ uint32_t fw_view_slot(const FwSegView &v, uint32_t head, uint32_t li) { return fw_ring_slot(head, li, v.capacity); }
// lifetime of slot i: Q3.w, or -- a type that cannot turn -- its plane, or -- a FIFO ring of such a type -- the type's one value
__device__ __forceinline__ float fw_view_life(const FwSegView &v, uint32_t i) {
    if (v.nospin && v.life_plane == 0xFFFFFFFFu) return v.life_const;
    return fw_load_lifetime(v.buf, v.capacity, v.life_plane, i, v.nospin != 0u, v.cpl != 0u);
}
// position + age (a FIFO ring: component planes, FwSegView::cpl bit 2)
__device__ __forceinline__ float4 fw_view_q0(const FwSegView &v, uint32_t i) { return fw_ldq0(v.buf, v.capacity, i, v.cpl); }
// the position alone (the volume queries): three component loads where Q0 is four planes -- the age plane of a FIFO ring, which may be
// stale under the age rule, is not touched --, the one float4 everywhere else
__device__ __forceinline__ fw_v3 fw_view_pos(const FwSegView &v, uint32_t i) {
    const char *q0 = v.buf + FW_OFF_Q0(v.capacity);
    if (v.cpl & FW_CPL_Q0) {
        const size_t cp = FW_CP(v.capacity);
        return fw_v3{fw_ld1(q0, i), fw_ld1(q0 + cp, i), fw_ld1(q0 + 2 * cp, i)};
    }
    const float4 q = fw_ld4(q0, i);
    return fw_v3{q.x, q.y, q.z};
}
// velocity + initial_scale, angular velocity + lifetime (cannot turn: 0), rotation (cannot turn: the type's one)
__device__ __forceinline__ float4 fw_view_q1(const FwSegView &v, uint32_t i) { return fw_ldq(v.buf + FW_OFF_Q1(v.capacity), v.capacity, i, v.cpl != 0u); }
__device__ __forceinline__ float fw_view_q1w(const FwSegView &v, uint32_t i) { return fw_ldq_w(v.buf + FW_OFF_Q1(v.capacity), v.capacity, i, v.cpl != 0u); }
__device__ __forceinline__ float4 fw_view_q3(const FwSegView &v, uint32_t i) {
    return !v.nospin ? fw_ldq(v.buf + FW_OFF_Q3(v.capacity), v.capacity, i, v.cpl != 0u) : make_float4(0.0f, 0.0f, 0.0f, fw_view_life(v, i));
}
__device__ __forceinline__ float4 fw_view_rot(const FwSegView &v, uint32_t i) {
    return v.nospin ? v.rot : fw_ldq(v.buf + FW_OFF_Q2(v.capacity), v.capacity, i, (v.cpl & 2u) != 0u);
}
// scale and colours of slot i (age: its Q0.w): what the planes hold, or -- FW_TYPE_DERIVED: the planes are not maintained --
// what the last update computed, again
__device__ __forceinline__ void fw_view_look(const FwSegView &v, uint32_t i, float age, float4 *bc, float4 *em, float *sc) {
    *sc = fw_ld1(v.buf + FW_OFF_S4(v.capacity), i), *bc = fw_ld4(v.buf + FW_OFF_Q5(v.capacity), i), *em = fw_ld4(v.buf + FW_OFF_Q6(v.capacity), i);
    if (v.derived) fw_derived_values(*v.derived, v.keys + v.derived->keys_off, age, fw_view_life(v, i), fw_view_q1w(v, i), bc, em, sc);
}
// ... and the scale alone
__device__ __forceinline__ float fw_view_scale(const FwSegView &v, uint32_t i, float age) {
    const float sc = fw_ld1(v.buf + FW_OFF_S4(v.capacity), i);
    if (!v.derived) return sc;
    const FwType &T = *v.derived;
    const float *keys = v.keys + T.keys_off;
    return fw_view_q1w(v, i) * fw_curve_sample(T.sc_kind, T.sc_n, keys, keys + T.o_sc_v, age / fw_view_life(v, i));
}

// SoA planes -> fw_particle records (26 x 4 B)
__global__ void fw_k_gather(FwSegView v, uint32_t n, int32_t pbr, float *out) {
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n) return;
    const uint32_t i = fw_view_slot(v, fw_view_head(v), li);
    const float4 q0 = fw_view_q0(v, i), q1 = fw_view_q1(v, i), q2 = fw_view_rot(v, i), q3 = fw_view_q3(v, i);
    float4 bc, em;
    float sc;
    fw_view_look(v, i, q0.w, &bc, &em, &sc);
    float *r = out + (size_t)li * 26;
    r[0] = q0.x, r[1] = q0.y, r[2] = q0.z;
    r[3] = q1.x, r[4] = q1.y, r[5] = q1.z;
    r[6] = q2.x, r[7] = q2.y, r[8] = q2.z, r[9] = q2.w;
    r[10] = q3.x, r[11] = q3.y, r[12] = q3.z;
    r[13] = q1.w, r[14] = sc, r[15] = q0.w, r[16] = q3.w;
    r[17] = bc.x, r[18] = bc.y, r[19] = bc.z, r[20] = bc.w;
    r[21] = em.x, r[22] = em.y, r[23] = em.z, r[24] = em.w;
    reinterpret_cast<int32_t *>(r)[25] = pbr;
}

__global__ void fw_k_scatter(char *buf, uint32_t C, uint32_t n, uint32_t n_lplanes, const float *in) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = in + (size_t)i * 26;
    fw_st4(buf + FW_OFF_Q0(C), i, make_float4(r[0], r[1], r[2], r[15]));
    fw_st4(buf + FW_OFF_Q1(C), i, make_float4(r[3], r[4], r[5], r[13]));  // (the caller's particles: always a segment of the compacting path -- float4 planes)
    fw_st4(buf + FW_OFF_Q2(C), i, make_float4(r[6], r[7], r[8], r[9]));
    fw_st4(buf + FW_OFF_Q3(C), i, make_float4(r[10], r[11], r[12], r[16]));
    fw_st4(buf + FW_OFF_Q5(C), i, make_float4(r[17], r[18], r[19], r[20]));
    fw_st4(buf + FW_OFF_Q6(C), i, make_float4(r[21], r[22], r[23], r[24]));
    reinterpret_cast<float *>(buf + FW_OFF_S4(C))[i] = r[14];
    for (uint32_t k = 0; k < n_lplanes; k++) reinterpret_cast<float *>(buf + FW_OFF_L(C, k))[i] = FW_F32_MIN;
}

// both colour planes of a fresh buffer pair filled with the type's colours at age 0: for a constant gradient that is
// the colour of every particle for ever (FwOutWin::wr5 / wr6), for any other it is simply overwritten
__global__ void fw_k_fill_colors(char *buf0, char *buf1, uint32_t C, float4 bc, float4 em) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C) return;
    fw_st4(buf0 + FW_OFF_Q5(C), i, bc), fw_st4(buf0 + FW_OFF_Q6(C), i, em);
    if (buf1) fw_st4(buf1 + FW_OFF_Q5(C), i, bc), fw_st4(buf1 + FW_OFF_Q6(C), i, em);
}

// a type leaves FW_TYPE_DERIVED (its instance buffer is detached): scale and colour planes of every slot, evaluated from
// the slot's age / lifetime / initial_scale -- what the updates would have stored
__global__ void fw_k_rederive(FwSegView v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.capacity) return;
    const float4 q0 = fw_view_q0(v, i);
    float4 bc, em;
    float sc;
    fw_derived_values(*v.derived, v.keys + v.derived->keys_off, q0.w, fw_view_life(v, i), fw_view_q1w(v, i), &bc, &em, &sc);
    fw_st4(v.buf + FW_OFF_Q5(v.capacity), i, bc), fw_st4(v.buf + FW_OFF_Q6(v.capacity), i, em), fw_st1(v.buf + FW_OFF_S4(v.capacity), i, sc);
}
hipError_t fw_launch_rederive(hipStream_t s, const FwSegView &v) {
    if (!v.derived) return hipErrorInvalidValue;
    if (!v.capacity) return hipSuccess;
    hipLaunchKernelGGL(fw_k_rederive, dim3((v.capacity + 255) / 256), dim3(256), 0, s, v);
    return hipGetLastError();
}

// The age plane of a FIFO ring whose launches ran under the age rule (FW_TYPE_IDX_AGELESS, fw_device.h), written back from the host's
// cohorts: logical particle li < live gets the age of its cohort (fw_ages.h) in slot (head + li) mod capacity of the plane.
__global__ void fw_k_fifo_ages(char *buf, uint32_t C, uint32_t head, uint32_t live, const FwAgeEntry *tab, uint32_t n) {
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    float age;
    if (!fw_age_of(tab, n, live, li, &age)) return;
    fw_st1(buf + FW_OFF_Q0(C) + 3 * FW_CP(C), fw_ring_slot(head, li, C), age);
}
hipError_t fw_launch_fifo_ages(hipStream_t s, char *buf, uint32_t capacity, uint32_t head, uint32_t live, const void *d_table, uint32_t n) {
    if (!live || !n || live > capacity || head >= capacity) return hipSuccess;
    hipLaunchKernelGGL(fw_k_fifo_ages, dim3((live + 255) / 256), dim3(256), 0, s, buf, capacity, head, live, (const FwAgeEntry *)d_table, n);
    return hipGetLastError();
}

// The spin of a FIFO ring whose launches deferred it (FW_TYPE_IDX_NOSPIN with FW_TYPE_IDX_AXIS, fw_device.h), replayed from the host's log:
// logical particle li < live has had every update's spin step except those of log entries [from, log_n) (fw_spin.h: per cohort).  One
// load of the three planes the axis rule moves, fw_spin_step once per pending dt -- the statements and the registers of the update
// that skipped it: the axis' own component and the rotation's w loaded, +0 everywhere else --, one store.  Every logged dt passed
// axis_dt_ok: each lane takes fw_quat_step's polynomial arm whoever shares its wave (axis_spin_rule, fw_engine_build.cpp), so the
// grouping of lanes, which differs from the update's, changes no bit.  (The update stores a plane only where a bit of it changed in
// some lane of the wave; storing the same values unconditionally leaves the same planes.)
// (T.angacc is +0 / 0 in every ring that reaches this kernel: axis_spin_rule's C3 refuses a type with an angular acceleration, along the
// axis included, so the replay of an ACCELERATING ring is not a tested path -- whoever relaxes C3 has to add that test.)
__global__ void fw_k_fifo_spin(char *buf, uint32_t C, uint32_t head, uint32_t live, const FwType *type, uint32_t axis, const FwSpinEntry *tab,
                               uint32_t n, uint32_t log_n) {
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    const float *log = reinterpret_cast<const float *>(tab + n);
    uint32_t from = 0;
    const uint32_t steps = fw_spin_steps(tab, n, live, log_n, li, &from);
    if (!steps) return;
    const FwType T = *type;
    const uint32_t s = fw_ring_slot(head, li, C), k = axis - 1u;
    char *p2 = buf + FW_OFF_Q2(C), *p3 = buf + FW_OFF_Q3(C);
    const size_t cp = FW_CP(C);
    const float rk = fw_ld1(p2 + k * cp, s), wk = fw_ld1(p3 + k * cp, s);
    float4 q2 = make_float4(k == 0u ? rk : 0.0f, k == 1u ? rk : 0.0f, k == 2u ? rk : 0.0f, fw_ld1(p2 + 3 * cp, s));
    float4 q3 = make_float4(k == 0u ? wk : 0.0f, k == 1u ? wk : 0.0f, k == 2u ? wk : 0.0f, 0.0f);
    for (uint32_t e = from; e < log_n; e++) {
        const FwSpin sp = fw_spin_step(T, log[e], q2, q3);
        q2 = make_float4(sp.rot.x, sp.rot.y, sp.rot.z, sp.rot.w), q3 = make_float4(sp.wx, sp.wy, sp.wz, 0.0f);
    }
    fw_st1(p2 + k * cp, s, k == 0u ? q2.x : k == 1u ? q2.y : q2.z);
    fw_st1(p2 + 3 * cp, s, q2.w);
    fw_st1(p3 + k * cp, s, k == 0u ? q3.x : k == 1u ? q3.y : q3.z);
}
hipError_t fw_launch_fifo_spin(hipStream_t s, char *buf, uint32_t capacity, uint32_t head, uint32_t live, const FwType *type, uint32_t axis,
                               const void *d_table, uint32_t n, uint32_t log_n) {
    if (live > capacity || (capacity && head >= capacity) || axis < 1u || axis > 3u || !type) return hipErrorInvalidValue;  // (never a silent skip)
    if (!live || !n || !log_n) return hipSuccess;  // nothing pending
    hipLaunchKernelGGL(fw_k_fifo_spin, dim3((live + 255) / 256), dim3(256), 0, s, buf, capacity, head, live, type, axis, (const FwSpinEntry *)d_table, n,
                       log_n);
    return hipGetLastError();
}

// a type leaves FW_TYPE_NOSPIN: its rotation plane, which nobody maintained, gets the constant rotation in every slot
// (cpl: FwSegView::cpl -- bit 1: a FIFO ring, the rotation in component planes, fw_dev.h)
__global__ void fw_k_fill_rotation(char *buf0, char *buf1, uint32_t C, float4 rot, uint32_t cpl) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C) return;
    fw_stq(buf0 + FW_OFF_Q2(C), C, i, rot, (cpl & 2u) != 0u);
    if (buf1) fw_stq(buf1 + FW_OFF_Q2(C), C, i, rot, (cpl & 2u) != 0u);
}

// a 4-byte plane filled with one value (the lifetime plane of a ring that becomes a compacting segment)
__global__ void fw_k_fill_plane1(char *buf0, char *buf1, size_t plane_off, uint32_t C, float v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C) return;
    fw_st1(buf0 + plane_off, i, v);
    if (buf1) fw_st1(buf1 + plane_off, i, v);
}
// a type leaves FW_TYPE_NOSPIN: Q3 = {0, 0, 0, lifetime} again -- what a reader of the no-spin view sees, stored; buf1 (or null):
// the same for the segment's other buffer
__global__ void fw_k_restore_q3(FwSegView v, char *buf1) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.capacity) return;
    fw_stq(v.buf + FW_OFF_Q3(v.capacity), v.capacity, i, fw_view_q3(v, i), v.cpl != 0u);
    if (!buf1) return;
    FwSegView w = v;
    w.buf = buf1;
    fw_stq(w.buf + FW_OFF_Q3(w.capacity), w.capacity, i, fw_view_q3(w, i), w.cpl != 0u);
}

// ParticleInstance packing (reference src/render.rs:95-115): {pos, scale, rot, base, emissive}
// SoA planes -> ParticleInstance records (render.rs:95-115).  Loads are plane-wise coalesced; the 64-byte records are
// transposed through LDS so that every store instruction of a wave writes 1 KiB of consecutive bytes (a lane writing
// its own record with four float4 stores would touch 64 lines a quarter at a time).
// SORTED (depth-sorted records, fw_sort.h): record j is that of list particle order[j] -- the indices the sort of fw_k_sort.hip left,
// each below n (clamped all the same: no address depends on trusting them) -- instead of list particle j; everything else is the same
// statements.
template <bool SORTED>
__global__ __launch_bounds__(256) void fw_k_pack(FwSegView v, const uint32_t *d_count, uint32_t n_upper, const uint32_t *order, float4 *out) {
    __shared__ float4 s_rec[256 * 4];
    const uint32_t head = fw_view_head(v);
    const uint32_t n = min(*d_count, n_upper);
    const uint32_t tid = threadIdx.x;
    for (uint32_t b = blockIdx.x * 256u; b < n; b += gridDim.x * 256u) {
        const uint32_t j = min(b + tid, n - 1u);
        const uint32_t i = fw_view_slot(v, head, SORTED ? min(order[j], n - 1u) : j);
        const float4 q0 = fw_view_q0(v, i), q2 = fw_view_rot(v, i);
        float4 q5, q6;
        float sc;
        fw_view_look(v, i, q0.w, &q5, &q6, &sc);
        s_rec[tid * 4 + 0] = make_float4(q0.x, q0.y, q0.z, sc);
        s_rec[tid * 4 + 1] = q2;
        s_rec[tid * 4 + 2] = q5;
        s_rec[tid * 4 + 3] = q6;
        __syncthreads();
        const uint32_t cnt4 = min(256u, n - b) * 4u;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t e = k * 256u + tid;
            if (e < cnt4) out[(size_t)b * 4 + e] = s_rec[e];
        }
        __syncthreads();
    }
}

// The sort key of every particle of the first min(*d_count, n_upper) of a segment (fw_sort.h: view depth of the position the pack writes
// into its record, mapped to 32 bits that sort ascending) and the particle's own list index beside it: what fw_k_sort.hip orders.
__global__ __launch_bounds__(256) void fw_k_depth_keys(FwSegView v, const uint32_t *d_count, uint32_t n_upper, FwSortView sv, uint32_t *key, uint32_t *idx) {
    const uint32_t head = fw_view_head(v);
    const uint32_t n = min(*d_count, n_upper);
    for (uint32_t li = blockIdx.x * 256u + threadIdx.x; li < n; li += gridDim.x * 256u) {
        const float4 q0 = fw_view_q0(v, fw_view_slot(v, head, li));
        key[li] = fw_sort_key(q0.x, q0.y, q0.z, sv), idx[li] = li;
    }
}

__device__ __forceinline__ void fw_atomic_minf(float *addr, float v) {
    int *ia = reinterpret_cast<int *>(addr);
    int old = __hip_atomic_load(ia, RLX, AGENT);
    while (v < __int_as_float(old)) {
        const int assumed = old;
        old = atomicCAS(ia, assumed, __float_as_int(v));
        if (old == assumed) break;
    }
}
__device__ __forceinline__ void fw_atomic_maxf(float *addr, float v) {
    int *ia = reinterpret_cast<int *>(addr);
    int old = __hip_atomic_load(ia, RLX, AGENT);
    while (v > __int_as_float(old)) {
        const int assumed = old;
        old = atomicCAS(ia, assumed, __float_as_int(v));
        if (old == assumed) break;
    }
}

// update_aabbs reduction (reference src/render.rs:677-703): min/max over position -/+ scale.
// blockIdx.y = segment of the spawner; out6 = {min xyz, max xyz}, pre-set to {+MAX, -MAX}.
// update_aabbs (render.rs:677-703) in two launches and no atomics: workgroups reduce position -/+ scale over their slice
// of every particle type of the spawner into one partial box each; a single workgroup folds the partials and leaves
// {min.xyz, any, max.xyz, -} in PINNED host memory, so the query costs one stream synchronisation and no copies.
struct FwSegList {
    uint32_t n;
    uint32_t id[8];  // FW_MAX_TYPES
    FwSegView v[8];  // (fw_k_aabb only: the other two fold what somebody else read)
};
// What the three kernels end in: every lane's {min.xyz, max.xyz} folded over the workgroup (WG lanes) -- over the wave, then across
// the waves through LDS; lane c < 6 returns component c of the result
template <uint32_t WG>
__device__ __forceinline__ float fw_box_fold(float v[6]) {
    __shared__ float s_m[WG / 64][6];
#pragma unroll
    for (int c = 0; c < 6; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float other = __shfl_xor(v[c], o, 64);
            v[c] = c < 3 ? fminf(v[c], other) : fmaxf(v[c], other);
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int c = 0; c < 6; c++) s_m[wave][c] = v[c];
    __syncthreads();
    float r = 0.0f;
    if (threadIdx.x < 6) {
        const uint32_t c = threadIdx.x;
        r = s_m[0][c];
        for (uint32_t w = 1; w < WG / 64; w++) r = c < 3 ? fminf(r, s_m[w][c]) : fmaxf(r, s_m[w][c]);
    }
    return r;
}
// ... and the answer in pinned host memory: {min.xyz, any, max.xyz, -}
template <uint32_t WG>
__device__ __forceinline__ void fw_box_answer(const FwGlobals &g, const FwSegList &L, uint32_t parity, float v[6], float *host8) {
    const float r = fw_box_fold<WG>(v);
    if (threadIdx.x < 6) host8[threadIdx.x < 3 ? threadIdx.x : threadIdx.x + 1u] = r;
    if (threadIdx.x == 0) {
        uint32_t any = 0;
        for (uint32_t k = 0; k < L.n; k++) any |= g.count[parity * g.max_seg + L.id[k]];
        host8[3] = any ? 1.0f : 0.0f;
    }
}
#define FW_AABB_BLOCKS 256u
__global__ __launch_bounds__(FW_BLOCK) void fw_k_aabb(FwGlobals g, FwSegList L, uint32_t parity, float *part8) {
    float m[6] = {3.40282347e+38f, 3.40282347e+38f, 3.40282347e+38f, FW_F32_MIN, FW_F32_MIN, FW_F32_MIN};
    for (uint32_t k = 0; k < L.n; k++) {
        const FwSegView &v = L.v[k];
        const uint32_t n = g.count[parity * g.max_seg + L.id[k]];
        const uint32_t head = fw_view_head(v);
        for (uint32_t li = blockIdx.x * FW_BLOCK + threadIdx.x; li < n; li += gridDim.x * FW_BLOCK) {
            const uint32_t i = fw_view_slot(v, head, li);
            const float4 q0 = fw_view_q0(v, i);
            const float sc = fw_view_scale(v, i, q0.w);
            m[0] = fminf(m[0], q0.x - sc), m[1] = fminf(m[1], q0.y - sc), m[2] = fminf(m[2], q0.z - sc);
            m[3] = fmaxf(m[3], q0.x + sc), m[4] = fmaxf(m[4], q0.y + sc), m[5] = fmaxf(m[5], q0.z + sc);
        }
    }
    const float r = fw_box_fold<FW_BLOCK>(m);
    if (threadIdx.x < 6) part8[blockIdx.x * 8u + threadIdx.x] = r;
}
__global__ __launch_bounds__(FW_AABB_BLOCKS) void fw_k_aabb_fold(FwGlobals g, FwSegList L, uint32_t parity,
                                                                 const float *part8, float *host8) {
    float v[6];
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] = part8[threadIdx.x * 8u + c];
    fw_box_answer<FW_AABB_BLOCKS>(g, L, parity, v, host8);
}

// fw_spawner_aabb from the per-tile boxes the last update left (fw_tile_box_flush): one workgroup folds the boxes of the
// spawner's segments -- a few hundred 32-byte records -- and leaves {min.xyz, any, max.xyz, -} in pinned host memory.
__global__ __launch_bounds__(FW_BLOCK) void fw_k_aabb_from_tiles(FwGlobals g, FwSegList L, uint32_t parity, uint32_t epoch,
                                                                 const uint32_t *seg_tile_first, float *host8) {
    float v[6] = {3.40282347e+38f, 3.40282347e+38f, 3.40282347e+38f, FW_F32_MIN, FW_F32_MIN, FW_F32_MIN};
    const float4 *boxes = reinterpret_cast<const float4 *>(g.tile_box);
    for (uint32_t k = 0; k < L.n; k++) {
        const uint32_t seg = L.id[k];
        const uint32_t t0 = seg_tile_first[seg], t1 = seg_tile_first[seg + 1];
        for (uint32_t t = t0 + threadIdx.x; t < t1; t += FW_BLOCK) {
            const float4 lo = boxes[(size_t)t * 2], hi = boxes[(size_t)t * 2 + 1];
            if (__float_as_uint(lo.w) != epoch) continue;  // a tile that held no particles in the last update
            v[0] = fminf(v[0], lo.x), v[1] = fminf(v[1], lo.y), v[2] = fminf(v[2], lo.z);
            v[3] = fmaxf(v[3], hi.x), v[4] = fmaxf(v[4], hi.y), v[5] = fmaxf(v[5], hi.z);
        }
    }
fw_box_answer<FW_BLOCK>(g, L, parity, v, host8);
}

// The boxes of MANY spawners in two launches (fw_ctx_aabbs[_device]; fw_boxes.h): the host lists every (spawner, type) segment once
// per output place it belongs to -- view, count word, upper bound, running sum of chunks -- and one WAVE takes one chunk of
// FW_BOX_CHUNK list positions of one segment: a 733-particle emitter occupies two waves, not fw_k_aabb's 256 workgroups.  The wave
// finds its entry by binary search, reads the device's count and leaves the box of [first, first + chunk) below min(count, bound)
// -- fw_k_aabb's initial values where that is empty -- in its own 32-byte slot of the scratch.  No atomics, nobody waits for anybody.
__global__ __launch_bounds__(64) void fw_k_boxes(const FwBoxEntry *tab, uint32_t n_entries, float *part8) {
    const uint32_t chunk = blockIdx.x;
    uint32_t first;
    const FwBoxEntry &E = tab[fw_boxes_locate(tab, n_entries, chunk, &first)];
    const FwSegView v = E.v;
    const uint32_t n = min(*E.d_count, E.bound);
    const uint32_t end = (n > first && n - first > FW_BOX_CHUNK) ? first + FW_BOX_CHUNK : n;
    float m[6] = {3.40282347e+38f, 3.40282347e+38f, 3.40282347e+38f, FW_F32_MIN, FW_F32_MIN, FW_F32_MIN};
    const uint32_t head = fw_view_head(v);
    for (uint32_t li = first + threadIdx.x; li < end; li += 64u) {
        const uint32_t i = fw_view_slot(v, head, li);
        const float4 q0 = fw_view_q0(v, i);
        const float sc = fw_view_scale(v, i, q0.w);
        m[0] = fminf(m[0], q0.x - sc), m[1] = fminf(m[1], q0.y - sc), m[2] = fminf(m[2], q0.z - sc);
        m[3] = fmaxf(m[3], q0.x + sc), m[4] = fmaxf(m[4], q0.y + sc), m[5] = fmaxf(m[5], q0.z + sc);
    }
    const float r = fw_box_fold<64>(m);
    if (threadIdx.x < 6) part8[(size_t)chunk * 8u + (threadIdx.x < 3 ? threadIdx.x : threadIdx.x + 1u)] = r;  // {min.xyz, -, max.xyz, -}
}
// ... and one wave per output place folds the partial boxes of the place's chunks, ORs the counts of its entries for `any` and writes
// the fw_aabb record {min.xyz, any, max.xyz, 0} -- to device memory, or to pinned host memory (the host form: no copy)
__global__ __launch_bounds__(64) void fw_k_boxes_fold(const FwBoxEntry *tab, const FwBoxPlace *places, const float *part8, float *out8) {
    const FwBoxPlace P = places[blockIdx.x];
    float m[6] = {3.40282347e+38f, 3.40282347e+38f, 3.40282347e+38f, FW_F32_MIN, FW_F32_MIN, FW_F32_MIN};
    for (uint32_t c = P.c0 + threadIdx.x; c < P.c1; c += 64u) {
        const float4 lo = reinterpret_cast<const float4 *>(part8)[(size_t)c * 2], hi = reinterpret_cast<const float4 *>(part8)[(size_t)c * 2 + 1];
        m[0] = fminf(m[0], lo.x), m[1] = fminf(m[1], lo.y), m[2] = fminf(m[2], lo.z);
        m[3] = fmaxf(m[3], hi.x), m[4] = fmaxf(m[4], hi.y), m[5] = fmaxf(m[5], hi.z);
    }
    uint32_t any = 0;
    for (uint32_t e = P.e0 + threadIdx.x; e < P.e1; e += 64u) any |= *tab[e].d_count;
    const int got = __any(any != 0u);
    const float r = fw_box_fold<64>(m);
    float *rec = out8 + (size_t)blockIdx.x * 8u;
    if (threadIdx.x < 6) rec[threadIdx.x < 3 ? threadIdx.x : threadIdx.x + 1u] = r;
    if (threadIdx.x == 0) reinterpret_cast<int32_t *>(rec)[3] = got ? 1 : 0, reinterpret_cast<uint32_t *>(rec)[7] = 0u;
}

// VOLUME QUERIES (fw_ctx_count_in_volumes[_device]; fw_volumes.h): how many particles of every listed place lie inside every listed
// volume, in two launches.  The chunks are the batched boxes' (fw_boxes.h: the same entry table, plan and locate): one WAVE takes one chunk
// of FW_BOX_CHUNK list positions of one segment.  A lane loads its FW_BOX_CHUNK / 64 positions ONCE -- positions only, fw_view_pos -- and
// keeps which of them lie below min(count, bound) as bits; the volumes then pass by in tiles of FW_VOLUME_TILE FwCollider records through
// LDS, every lane tests its positions against the one record the wave is at, the wave adds its ballots, and lane v mod 64 keeps the count
// of volume v.  Each tile ends in one store per lane into the scratch, which is laid out [volume][chunk]: the fold reads the chunks of
// one (place, volume) side by side.  A chunk beyond the device's count tests nothing and stores zeros.  No atomics, no memset, nobody
// waits for anybody.
constexpr uint32_t FW_VOL_PER_LANE = FW_BOX_CHUNK / 64u;
static_assert(FW_BOX_CHUNK % 64u == 0 && FW_VOL_PER_LANE >= 1u && FW_VOL_PER_LANE <= 32u, "a lane keeps the validity of its positions as bits of one word");
static_assert(FW_VOLUME_TILE == 64u, "lane v mod 64 keeps the count of volume v");
__global__ __launch_bounds__(64) void fw_k_volumes(const FwBoxEntry *tab, uint32_t n_entries, const FwCollider *vols, uint32_t n_vol, uint32_t total_chunks,
                                                   uint32_t *part) {
    __shared__ FwCollider s_vol[FW_VOLUME_TILE];
    const uint32_t chunk = blockIdx.x, lane = threadIdx.x;
    uint32_t first;
    const FwBoxEntry &E = tab[fw_boxes_locate(tab, n_entries, chunk, &first)];
    const FwSegView v = E.v;
    const uint32_t n = min(*E.d_count, E.bound);
    const uint32_t end = (n > first && n - first > FW_BOX_CHUNK) ? first + FW_BOX_CHUNK : n;
    const uint32_t head = fw_view_head(v);
    fw_v3 p[FW_VOL_PER_LANE];
    uint32_t valid = 0u;
#pragma unroll
    for (uint32_t k = 0; k < FW_VOL_PER_LANE; k++) {
        const uint32_t li = first + k * 64u + lane;
        p[k] = fw_v3{0.0f, 0.0f, 0.0f};
        if (li < end) p[k] = fw_view_pos(v, fw_view_slot(v, head, li)), valid |= 1u << k;
    }
    for (uint32_t v0 = 0; v0 < n_vol; v0 += FW_VOLUME_TILE) {
        const uint32_t m = min(FW_VOLUME_TILE, n_vol - v0);
        if (lane < m) s_vol[lane] = vols[v0 + lane];
        __syncthreads();
        uint32_t mine = 0u;
        for (uint32_t j = 0; j < (end > first ? m : 0u); j++) {
            const FwCollider c = s_vol[j];
            uint32_t cnt = 0u;
#pragma unroll
            for (uint32_t k = 0; k < FW_VOL_PER_LANE; k++) cnt += (uint32_t)__popcll(__ballot(((valid >> k) & 1u) != 0u && fw_collider_contains(c, p[k])));
            if (lane == j) mine = cnt;
        }
        if (lane < m) part[(size_t)(v0 + lane) * total_chunks + chunk] = mine;
        __syncthreads();  // (the next tile overwrites the records)
    }
}
// ... and one wave per ANSWER (place p, volume v: workgroup p * n_vol + v) adds the counts of the place's chunks, which lie side by side
// in the volume's row of the scratch, and writes out[p * n_vol + v] -- to device memory, or to pinned host memory (the host form: no copy)
__global__ __launch_bounds__(64) void fw_k_volumes_fold(const FwBoxPlace *places, const uint32_t *part, uint32_t n_vol, uint32_t total_chunks, uint32_t *out) {
    const FwBoxPlace P = places[blockIdx.x / n_vol];
    const uint32_t *row = part + (size_t)(blockIdx.x % n_vol) * total_chunks;
    uint32_t s = 0u;
    for (uint32_t c = P.c0 + threadIdx.x; c < P.c1; c += 64u) s += row[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ void fw_k_total(const uint32_t *counts, uint32_t n_seg, unsigned long long *out) {
    __shared__ unsigned long long s[4];
    unsigned long long t = 0;
    for (uint32_t i = threadIdx.x; i < n_seg; i += blockDim.x) t += counts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63u) == 0) s[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) *out = s[0] + s[1] + s[2] + s[3];
}

// float4 streaming copy: the measured-roofline probe (bytes read + written per second).  Shape chosen by a sweep on
// MI355X at 1 GiB -> 1 GiB (tools/membw <MiB> copy, profiles/r02/copy_sweep.txt): grid-strided, four float4 per lane in
// flight, non-temporal loads and stores, 16384 workgroups: 6.34 TB/s (plain one-float4 grid-stride: 4.9; hipMemcpy D2D: 5.0).
__global__ __launch_bounds__(FW_BLOCK) void fw_k_copy(const float4 *src, float4 *dst, size_t n4) {
    constexpr int U = 4;
    const size_t stride = (size_t)gridDim.x * FW_BLOCK * U;
    const FW_GLOBAL fw_f4 *s = reinterpret_cast<const FW_GLOBAL fw_f4 *>(reinterpret_cast<uintptr_t>(src));
    FW_GLOBAL fw_f4 *d = reinterpret_cast<FW_GLOBAL fw_f4 *>(reinterpret_cast<uintptr_t>(dst));
    for (size_t i = (size_t)blockIdx.x * FW_BLOCK * U + threadIdx.x; i < n4; i += stride) {
        fw_f4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t j = i + (size_t)u * FW_BLOCK;
            if (j < n4) v[u] = __builtin_nontemporal_load(&s[j]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t j = i + (size_t)u * FW_BLOCK;
            if (j < n4) __builtin_nontemporal_store(v[u], &d[j]);
        }
    }
}

// ---- launch wrappers

hipError_t fw_launch_gather(hipStream_t s, const FwSegView &v, uint32_t n, int32_t pbr, void *d_out) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(fw_k_gather, dim3((n + 255) / 256), dim3(256), 0, s, v, n, pbr, (float *)d_out);
    return hipGetLastError();
}

hipError_t fw_launch_scatter(hipStream_t s, char *buf, uint32_t capacity, uint32_t n, uint32_t n_lplanes,
                             const void *d_in) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(fw_k_scatter, dim3((n + 255) / 256), dim3(256), 0, s, buf, capacity, n, n_lplanes,
                       (const float *)d_in);
    return hipGetLastError();
}

hipError_t fw_launch_fill_colors(hipStream_t s, char *buf0, char *buf1, uint32_t capacity, const float bc[4], const float em[4]) {
    if (!capacity) return hipSuccess;
    hipLaunchKernelGGL(fw_k_fill_colors, dim3((capacity + 255) / 256), dim3(256), 0, s, buf0, buf1, capacity,
                       make_float4(bc[0], bc[1], bc[2], bc[3]), make_float4(em[0], em[1], em[2], em[3]));
    return hipGetLastError();
}

hipError_t fw_launch_fill_plane1(hipStream_t s, char *buf0, char *buf1, size_t plane_off, uint32_t capacity, float v) {
    if (!capacity) return hipSuccess;
    hipLaunchKernelGGL(fw_k_fill_plane1, dim3((capacity + 255) / 256), dim3(256), 0, s, buf0, buf1, plane_off, capacity, v);
    return hipGetLastError();
}
hipError_t fw_launch_restore_q3(hipStream_t s, char *buf0, char *buf1, uint32_t capacity, uint32_t life_plane, float life_const, uint32_t cpl) {
    if (!capacity) return hipSuccess;
    FwSegView v{};  // (the segment as its readers see it until the flag goes: no spin)
    v.buf = buf0, v.capacity = capacity, v.cpl = cpl, v.nospin = 1u, v.life_plane = life_plane, v.life_const = life_const;
    hipLaunchKernelGGL(fw_k_restore_q3, dim3((capacity + 255) / 256), dim3(256), 0, s, v, buf1);
    return hipGetLastError();
}

hipError_t fw_launch_fill_rotation(hipStream_t s, char *buf0, char *buf1, uint32_t capacity, const float rot[4], uint32_t cpl) {
    if (!capacity) return hipSuccess;
    hipLaunchKernelGGL(fw_k_fill_rotation, dim3((capacity + 255) / 256), dim3(256), 0, s, buf0, buf1, capacity,
                       make_float4(rot[0], rot[1], rot[2], rot[3]), cpl);
    return hipGetLastError();
}

hipError_t fw_launch_pack_instances(hipStream_t s, const FwSegView &v, const uint32_t *d_count, uint32_t n_upper, void *d_out) {
    if (!n_upper) return hipSuccess;
    uint32_t blocks = (n_upper + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(fw_k_pack<false>, dim3(blocks), dim3(256), 0, s, v, d_count, n_upper, (const uint32_t *)nullptr, (float4 *)d_out);
    return hipGetLastError();
}

hipError_t fw_launch_depth_keys(hipStream_t s, const FwSegView &v, const uint32_t *d_count, uint32_t n_upper, const FwSortView &sv, uint32_t *d_key,
                                uint32_t *d_idx) {
    if (!n_upper) return hipSuccess;
    hipLaunchKernelGGL(fw_k_depth_keys, dim3(std::min((n_upper + 255u) / 256u, 8192u)), dim3(256), 0, s, v, d_count, n_upper, sv, d_key, d_idx);
    return hipGetLastError();
}

hipError_t fw_launch_pack_instances_sorted(hipStream_t s, const FwSegView &v, const uint32_t *d_count, uint32_t n_upper, const uint32_t *d_order,
                                           void *d_out) {
    if (!n_upper) return hipSuccess;
    if (!d_order) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fw_k_pack<true>, dim3(std::min((n_upper + 255u) / 256u, 8192u)), dim3(256), 0, s, v, d_count, n_upper, d_order, (float4 *)d_out);
    return hipGetLastError();
}

hipError_t fw_launch_aabb(hipStream_t s, const FwGlobals &g, const uint32_t *seg_ids, const FwSegView *views, uint32_t n_segs,
                          uint32_t parity, float *d_part, float *h_out8) {
    if (!n_segs || n_segs > 8u) return hipErrorInvalidValue;  // FW_MAX_TYPES
    FwSegList L{};
    L.n = n_segs;
    for (uint32_t i = 0; i < n_segs; i++) L.id[i] = seg_ids[i], L.v[i] = views[i];
    hipLaunchKernelGGL(fw_k_aabb, dim3(FW_AABB_BLOCKS), dim3(FW_BLOCK), 0, s, g, L, parity, d_part);
    hipLaunchKernelGGL(fw_k_aabb_fold, dim3(1), dim3(FW_AABB_BLOCKS), 0, s, g, L, parity, (const float *)d_part, h_out8);
    return hipGetLastError();
}

hipError_t fw_launch_aabb_from_tiles(hipStream_t s, const FwGlobals &g, const uint32_t *seg_ids, uint32_t n_segs,
                                     uint32_t parity, uint32_t epoch, const uint32_t *d_seg_tile_first, float *h_out8) {
    if (!n_segs || n_segs > 8u) return hipErrorInvalidValue;  // FW_MAX_TYPES
    FwSegList L{};
    L.n = n_segs;
    for (uint32_t i = 0; i < n_segs; i++) L.id[i] = seg_ids[i];
    hipLaunchKernelGGL(fw_k_aabb_from_tiles, dim3(1), dim3(FW_BLOCK), 0, s, g, L, parity, epoch, d_seg_tile_first, h_out8);
    return hipGetLastError();
}

hipError_t fw_launch_boxes(hipStream_t s, const FwBoxEntry *d_tab, uint32_t n_entries, const FwBoxPlace *d_places, uint32_t n_places,
                           uint32_t total_chunks, float *d_part, void *out_records, uint32_t *launches) {
    *launches = 0;
    if (!n_places) return hipSuccess;
    if (total_chunks > FW_BOX_MAX_CHUNKS || (total_chunks && !n_entries)) return hipErrorInvalidValue;
    if (total_chunks) {  // (no listed type can hold a particle: nothing to read, the fold alone answers)
        hipLaunchKernelGGL(fw_k_boxes, dim3(total_chunks), dim3(64), 0, s, d_tab, n_entries, d_part);
        ++*launches;
    }
    hipLaunchKernelGGL(fw_k_boxes_fold, dim3(n_places), dim3(64), 0, s, d_tab, d_places, (const float *)d_part, (float *)out_records);
    ++*launches;
    return hipGetLastError();
}

hipError_t fw_launch_volumes(hipStream_t s, const FwBoxEntry *d_tab, uint32_t n_entries, const FwBoxPlace *d_places, uint32_t n_places, uint32_t total_chunks,
                             const FwCollider *d_volumes, uint32_t n_volumes, uint32_t *d_part, void *out_counts, uint32_t *launches) {
    *launches = 0;
    if (!n_places || !n_volumes) return hipSuccess;
    if (total_chunks > FW_BOX_MAX_CHUNKS || (total_chunks && !n_entries) || (uint64_t)n_places * n_volumes > FW_VOLUME_MAX_ANSWERS) return hipErrorInvalidValue;
    if (total_chunks) {  // (no listed type can hold a particle: nothing to read, the fold alone answers -- with zeros)
        hipLaunchKernelGGL(fw_k_volumes, dim3(total_chunks), dim3(64), 0, s, d_tab, n_entries, d_volumes, n_volumes, total_chunks, d_part);
        ++*launches;
    }
    hipLaunchKernelGGL(fw_k_volumes_fold, dim3(n_places * n_volumes), dim3(64), 0, s, d_places, (const uint32_t *)d_part, n_volumes, total_chunks, (uint32_t *)out_counts);
    ++*launches;
    return hipGetLastError();
}

hipError_t fw_launch_total(hipStream_t s,const uint32_t *counts, uint32_t n_seg, unsigned long long *d_out) {
    hipLaunchKernelGGL(fw_k_total, dim3(1), dim3(256), 0, s, counts, n_seg, d_out);
    return hipGetLastError();
}

hipError_t fw_launch_copy_probe(hipStream_t s, const void *src, void *dst, size_t bytes) {
    hipLaunchKernelGGL(fw_k_copy, dim3(16384), dim3(FW_BLOCK), 0, s, (const float4 *)src, (float4 *)dst, bytes / 16);
    return hipGetLastError();
}

