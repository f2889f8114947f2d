// fw_sort.h -- depth-sorted instance records (round 20; include/firework_hip.h: DEPTH-SORTED INSTANCES): the view depth of a position and
// the 32-bit key the radix sort of fw_k_sort.hip orders by, and the shape of that sort (elements per workgroup, rows of its histogram
// table) the engine sizes its scratch from.  Plain C++ behind FW_HD: the key kernel (fw_k_depth_keys, fw_k_aux.hip) and a host test
// (tests/test_depth_sort_cpu.py) compile the same lines, as with fw_ages.h.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef FW_HD
#ifdef __HIPCC__
#define FW_HD __host__ __device__ __forceinline__
#else
#define FW_HD inline
#endif
#endif

// fw_sort_view (firework_hip.h) as the kernels take it: by value, in the kernel arguments
struct FwSortView {
    float eye[3];
    uint32_t order;  // FW_SORT_BACK_TO_FRONT = 0, FW_SORT_FRONT_TO_BACK = 1
    float forward[3];
    uint32_t reserved;
};

// depth of position p along `forward` from `eye`: fp32, every operation rounded (-ffp-contract=off), `forward` as given
FW_HD float fw_sort_depth(float px, float py, float pz, const FwSortView &s) {
    const float dx = px - s.eye[0], dy = py - s.eye[1], dz = pz - s.eye[2];
    const float xx = dx * s.forward[0], yy = dy * s.forward[1], zz = dz * s.forward[2];
    const float xy = xx + yy;
    return xy + zz;
}

// the key of a depth: ascending key = drawn first.  -0 and +0 tie; a NaN is drawn last in either order (0xFFFFFFFF, which no other
// depth reaches: the image of `a` is [0x007FFFFF, 0xFF800000])
FW_HD uint32_t fw_sort_key_of_depth(float d, uint32_t order) {
    if (d != d) return 0xFFFFFFFFu;
    uint32_t b;
    memcpy(&b, &d, 4);
    if (d == 0.0f) b = 0u;
    const uint32_t a = (b >> 31) ? ~b : (b | 0x80000000u);
    return order == 1u ? a : ~a;
}

FW_HD uint32_t fw_sort_key(float px, float py, float pz, const FwSortView &s) { return fw_sort_key_of_depth(fw_sort_depth(px, py, pz, s), s.order); }

// ---- the shape of the sort: four stable passes of FW_SORT_BITS bits, least significant digit first.  A workgroup of FW_SORT_WG lanes
// takes FW_SORT_TILE consecutive elements in FW_SORT_ROUNDS rounds of one element per lane; the histogram table has one row per digit
// and one column per workgroup (digit-major: entry [digit][workgroup]).
#define FW_SORT_BITS 8u
#define FW_SORT_DIGITS 256u
#define FW_SORT_PASSES 4u
#define FW_SORT_WG 256u
#define FW_SORT_ROUNDS 8u
#define FW_SORT_TILE (FW_SORT_WG * FW_SORT_ROUNDS)  // 2048

inline uint32_t fw_sort_tiles(uint32_t n_upper) { return (uint32_t)(((uint64_t)n_upper + FW_SORT_TILE - 1u) / FW_SORT_TILE); }
// uint32 words of scratch a sort of up to n_upper elements uses: two (key, idx) pairs, the histogram table, one row of digit totals
inline size_t fw_sort_scratch_words(uint32_t n_upper) { return (size_t)n_upper * 4u + (size_t)fw_sort_tiles(n_upper) * FW_SORT_DIGITS + FW_SORT_DIGITS; }
