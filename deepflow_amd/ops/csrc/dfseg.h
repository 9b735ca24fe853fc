// Device view of one L7 segment and the rules for reading it that more
// than one unit needs: the pooled strings of a row and the trace / span
// keys. Trace-id filters (dfquery.hip), the trace map (dftrace.hip) and flow
// groups (dfflow.hip) agree with each other because they all take their
// keys from here. Internal linkage (like dfhash.h); device code, but for
// the two host functions that carry the view across the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "l7_layout.h"
#include "dfhash.h"

namespace {

// seed of every pooled-string hash (host twin: query/spec.py
// STR_FILTER_SEED)
constexpr uint64_t STR_FILTER_SEED = 0x5157A15E5EEDull;

// An entry point that does not use a member leaves it null.
struct SegView {
    const uint64_t* u64c;
    const uint32_t* u32c;
    const uint8_t* u8c;
    const uint32_t* didc;      // [L7_DID_N, stride]
    // KnowledgeGraph table for query-time join (SmartEncoding: the 24
    // per-row KG id columns are NOT materialized — they are a pure
    // function of the row's (epc, ip) key, resolved here by probing the
    // GPU-resident platform table instead of spending 96 B/span of HBM)
    const uint64_t* kg_tk;
    const uint32_t* kg_tv;     // [cap, KG_VALS_N]
    uint32_t kg_mask;
    const int32_t* attr_pool;  // variable attr-id pool
    const uint32_t* attr_start;  // [stride] row block offsets into attr_pool
    const uint8_t* attr_cnt;   // [stride]
    const uint64_t* str_rowref;  // [stride] (pool_off<<16 | total_len)
    const int16_t* str_lens;   // [n_pool_cols, stride]
    const uint8_t* pool;       // segment string pool
    uint64_t stride;
    uint64_t n_rows;
};

// Across the C ABI the view travels as the address of a host struct of this
// very layout (ops/gpu_ops.py SegViewC, filled by seg_view()). It is read
// here, before the launch; kernels take the SegView by value.
inline SegView seg_view_load(const void* seg) {
    SegView s;
    __builtin_memcpy(&s, seg, sizeof(SegView));
    return s;
}

// offsetof every member, in declaration order: with sizeof, what a test
// holds the Python mirror against (df_seg_view_offsets in dfquery.hip)
constexpr uint32_t SEG_VIEW_MEMBERS = 15;
inline void seg_view_offsets(uint32_t* out) {
    const uint32_t offs[SEG_VIEW_MEMBERS] = {
        offsetof(SegView, u64c), offsetof(SegView, u32c),
        offsetof(SegView, u8c), offsetof(SegView, didc),
        offsetof(SegView, kg_tk), offsetof(SegView, kg_tv),
        offsetof(SegView, kg_mask), offsetof(SegView, attr_pool),
        offsetof(SegView, attr_start), offsetof(SegView, attr_cnt),
        offsetof(SegView, str_rowref), offsetof(SegView, str_lens),
        offsetof(SegView, pool), offsetof(SegView, stride),
        offsetof(SegView, n_rows)};
    for (uint32_t i = 0; i < SEG_VIEW_MEMBERS; i++) out[i] = offs[i];
}

// pooled string `idx` of a row: pointer + length
DEV const uint8_t* seg_pool_str(const SegView& s, uint64_t row, uint32_t idx,
                                uint32_t& len) {
    uint64_t off = STR_REF_OFF(s.str_rowref[row]);
    for (uint32_t c = 0; c < idx; c++)
        off += (uint16_t)s.str_lens[(uint64_t)c * s.stride + row];
    len = (uint16_t)s.str_lens[(uint64_t)idx * s.stride + row];
    return s.pool + off;
}

// its hash; 0 = empty string
DEV uint64_t seg_pool_hash(const SegView& s, uint64_t row, uint32_t idx) {
    uint32_t len;
    const uint8_t* p = seg_pool_str(s, row, idx, len);
    return len ? str_hash(p, len, STR_FILTER_SEED) : 0;
}

// SRC_TRACE128 idx 0: mix64(hi) ^ lo of the binary trace id, or the hash of
// the pooled text where the id was absent or not hex
DEV uint64_t seg_trace_key(const SegView& s, uint64_t row) {
    uint64_t hi = s.u64c[(uint64_t)L7_U64_TRACE_HI * s.stride + row];
    uint64_t lo = s.u64c[(uint64_t)L7_U64_TRACE_LO * s.stride + row];
    return (hi | lo) ? (mix64(hi) ^ lo)
                     : seg_pool_hash(s, row, L7_POOL_TRACE_ID);
}

// SRC_TRACE128 idx 1: the binary span id, with the same fallback
DEV uint64_t seg_span_key(const SegView& s, uint64_t row) {
    uint64_t v = s.u64c[(uint64_t)L7_U64_SPAN_ID_B * s.stride + row];
    return v ? v : seg_pool_hash(s, row, L7_POOL_SPAN_ID);
}

}  // namespace
