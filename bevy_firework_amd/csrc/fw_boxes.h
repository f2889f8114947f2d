// fw_boxes.h -- batched bounding boxes (round 25; include/firework_hip.h: BATCHED BOXES): how the particle lists of many (spawner, type)
// segments are cut into CHUNKS of FW_BOX_CHUNK consecutive list positions, one wave of fw_k_boxes each (fw_k_aux.hip).  The host plans --
// every entry's upper bound to a running sum of chunk counts, every output place's range of entries and chunks -- and the device locates:
// a wave finds the entry and the first list position of its chunk by binary search in that sum.  Plain C++ behind FW_HD: the engine
// (fw_engine_api.cpp: boxes_enqueue), the kernel and a host test (tests/test_aabb_batch_cpu.py) compile the same lines, as with fw_sort.h.
#pragma once
#include <stdint.h>

#ifndef FW_HD
#ifdef __HIPCC__
#define FW_HD __host__ __device__ __forceinline__
#else
#define FW_HD inline
#endif
#endif

// list positions per chunk: 8 per lane of the wave that owns it.  Swept 512 / 1024 / 2048 on one MI355X (profiles/r25/aabb_batch.txt): 512
// is the fastest or within noise at every shape measured (512 x 8192 spawners: 69.8 / 77.1 / 104.2 us per batched call)
#ifndef FW_BOX_CHUNK
#define FW_BOX_CHUNK 512u
#endif
// the most chunks -- and output places -- of one batch: each is a one-wave workgroup of a grid whose lanes a uint32 counts
#define FW_BOX_MAX_CHUNKS 0x3FFFFFFull

// an output place: its entries [e0, e1) of the entry table and their chunks [c0, c1)
struct FwBoxPlace {
    uint32_t e0, e1, c0, c1;
};

// chunks that cover list positions [0, bound): none for an entry that can hold no particle
FW_HD uint32_t fw_boxes_chunks(uint32_t bound) { return bound / FW_BOX_CHUNK + (bound % FW_BOX_CHUNK ? 1u : 0u); }

// The plan.  An entry (any record with `bound` and `chunk0`) gets the running sum of the chunks in front of it; places[p] describes the
// entries [place_first[p], place_first[p + 1]).  Returns the chunks in all -- the caller refuses more than FW_BOX_MAX_CHUNKS, beyond
// which chunk0 no longer holds the sum.
template <typename E>
FW_HD uint64_t fw_boxes_plan(E *tab, uint32_t n_entries, const uint32_t *place_first, uint32_t n_places, FwBoxPlace *places) {
    uint64_t sum = 0;
    uint32_t p = 0;
    for (uint32_t e = 0; e <= n_entries; e++) {
        // (every place that starts here -- a spawner without particle types owns no entry -- and the end of the one before it)
        for (; p <= n_places && place_first[p] == e; p++) {
            if (p > 0) places[p - 1].e1 = e, places[p - 1].c1 = (uint32_t)sum;
            if (p < n_places) places[p].e0 = e, places[p].c0 = (uint32_t)sum;
        }
        if (e == n_entries) break;
        tab[e].chunk0 = (uint32_t)sum;
        sum += fw_boxes_chunks(tab[e].bound);
    }
    return sum;
}

// The locate function.  chunk < the plan's total: the entry that owns it -- the LAST one whose running sum does not exceed it, which
// skips the empty entries that share a sum with their successor -- and, in *first, the list position the chunk starts at.
template <typename E>
FW_HD uint32_t fw_boxes_locate(const E *tab, uint32_t n_entries, uint32_t chunk, uint32_t *first) {
    uint32_t lo = 0, hi = n_entries;  // tab[lo].chunk0 <= chunk (tab[0].chunk0 == 0); every entry from hi on starts beyond it
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tab[mid].chunk0 <= chunk)
            lo = mid;
        else
            hi = mid;
    }
    *first = (chunk - tab[lo].chunk0) * FW_BOX_CHUNK;
    return lo;
}
