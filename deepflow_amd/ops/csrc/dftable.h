// Global open-addressing tables on a 64-bit key, shared by the HIP
// translation units of libdfgpu.so. Device-only, internal linkage (like
// dfhash.h): each unit gets its own copy.
//
// Rules for every table claimed through this header:
//  - EMPTY_KEY = 0 is reserved; a caller maps a zero hash to 1 first.
//  - a slot is claimed with one atomicCAS on its key word. Ids are SLOT
//    INDICES: there is no id counter and no second word to wait on. What
//    hangs off a slot is either written by the claimer alone and read in a
//    later launch, or is an atomicMin/Max/Add word the host initialised.
//  - the hit path is a plain load. Keys only ever go EMPTY -> h and never
//    change again, so a stale read can only show EMPTY where h already
//    stands; the CAS that follows returns the true word and `old == h`
//    counts as a hit. A stale non-empty word is the slot's final word.
//  - probe loops are bounded by the table size. A full table returns
//    ROW_NONE; the caller counts the row in its `drops` word and goes on.
//    Nothing spins or waits for another workgroup.
//  - the start slot is the caller's: stored ids (stack, app and dictionary
//    ids) are slot indices, so the units that start at `h & mask` and those
//    that start at `mix64(h) & mask` must each stay as they are.
//
// Kept apart on purpose:
//  - ru_claim_h (dfgpu.hip) verifies the raw key words behind the hash, publishes them
//    with a release store and gives up after RU_MAX_PROBES.
//  - group_claim (dfquery.hip) writes the raw key words inside its claim branch; routed
//    through `claimed` the flag stays live across the probe loop and costs
//    k_query_agg and k_qpart_agg registers.
//  - the LDS pre-aggregation tables (ru_pass in dfgpu.hip, agg_vals_lds in
//    dfquery.hip, the edge table of k_trace_fold in dftrace.hip) probe a fixed number of steps and
//    spill to the global table.
// intern_probe_wave (dfgpu.hip) elects a lane and then calls intern_probe, which
// claims through table_claim.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "l7_layout.h"  // DICT_ID_INVALID
#include "dfhash.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr uint64_t EMPTY_KEY = 0ull;
constexpr uint32_t ROW_NONE = 0xFFFFFFFFu;
constexpr uint32_t BLOCK = 256;

// a full table and an absent dictionary id are one value to every caller
static_assert(ROW_NONE == DICT_ID_INVALID, "ROW_NONE is DICT_ID_INVALID");

inline uint32_t grid_for(uint64_t total, uint32_t per_block = BLOCK) {
    return (uint32_t)((total + per_block - 1) / per_block);
}

// probe-or-insert; returns the slot of h, or ROW_NONE when the table is
// full. *claimed (optional) tells whether this thread inserted h.
DEV uint32_t table_claim(uint64_t* keys, uint32_t cap_mask, uint64_t h,
                         uint32_t start_slot, bool* claimed = nullptr) {
    if (claimed) *claimed = false;
    uint32_t slot = start_slot;
    for (uint32_t probe = 0; probe <= cap_mask; probe++) {
        uint64_t cur = keys[slot];
        if (cur == h) return slot;
        if (cur == EMPTY_KEY) {
            uint64_t old = atomicCAS((unsigned long long*)&keys[slot],
                                     EMPTY_KEY, h);
            if (old == EMPTY_KEY) {
                if (claimed) *claimed = true;
                return slot;
            }
            if (old == h) return slot;
            // lost the race to a different key: keep probing
        }
        slot = (slot + 1) & cap_mask;
    }
    return ROW_NONE;
}

// read-only probe (a later launch than the inserts); ROW_NONE = not there
DEV uint32_t table_find(const uint64_t* keys, uint32_t cap_mask, uint64_t h,
                        uint32_t start_slot) {
    uint32_t slot = start_slot;
    for (uint32_t probe = 0; probe <= cap_mask; probe++) {
        uint64_t cur = keys[slot];
        if (cur == h) return slot;
        if (cur == EMPTY_KEY) return ROW_NONE;
        slot = (slot + 1) & cap_mask;
    }
    return ROW_NONE;
}

// key -> lowest row that carries it. `h` is the already-mixed, non-zero
// key; `base` selects one of several tables of `cap` slots laid end to end.
struct FirstRowIdx {
    uint64_t* keys;
    uint32_t* rows;              // host-initialised to ROW_NONE
    unsigned long long* drops;
    uint32_t cap;                // per table, power of two
};

DEV void first_row_insert(const FirstRowIdx& ix, uint64_t base, uint64_t h,
                          uint32_t row) {
    uint32_t cap_mask = ix.cap - 1;
    uint32_t slot = table_claim(ix.keys + base, cap_mask, h,
                                (uint32_t)(mix64(h) & cap_mask));
    if (slot == ROW_NONE) atomicAdd(ix.drops, 1ull);
    else atomicMin(&ix.rows[base + slot], row);
}

DEV uint32_t first_row_find(const FirstRowIdx& ix, uint64_t base,
                            uint64_t h) {
    uint32_t cap_mask = ix.cap - 1;
    uint32_t slot = table_find(ix.keys + base, cap_mask, h,
                               (uint32_t)(mix64(h) & cap_mask));
    return slot == ROW_NONE ? ROW_NONE : ix.rows[base + slot];
}

}  // namespace
