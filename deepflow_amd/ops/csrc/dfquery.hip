// dfquery — the DF-SQL query path on gfx950: K7 filtered hash group-by (the
// querier hot path; replaces the ClickHouse-side GROUP BY of the reference
// design), its radix-partitioned variant for high cardinality, K15 exact
// distinct counts, the row select and the rocPRIM sort of the percentile
// path. Every kernel reads a segment through SegView (dfseg.h) and a
// host-built QuerySpec; all of them name a group by group_hash() below.
// Table rules are in dftable.h.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "dftable.h"
#include "dfseg.h"

namespace {

// key/agg source families
enum {
    SRC_U64 = 0, SRC_U32, SRC_U8, SRC_DID, SRC_KG, SRC_ATTR_VAL,
    SRC_TIME_BUCKET, SRC_CONST0, SRC_STR_HASH,
    // filter-only: exists(slot): name_id == v0 && value_id == v1
    SRC_ATTR_MATCH,
    // binary OTel ids (idx 0 = trace_id, 1 = span_id): mix64(hi)^lo of the
    // binary columns, or the pooled-string hash for non-hex fallbacks
    SRC_TRACE128,
};
// filter ops
// OP_INSET / OP_NOT_INSET (K16): v0 is the device address of a u32 bitmap,
// v1 its length in bits; the value is a member when it is below v1 and its
// bit is set. A value outside the bitmap (DICT_ID_INVALID among them) is
// not in the set, so it fails OP_INSET and passes OP_NOT_INSET.
enum { OP_EQ = 0, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_BETWEEN,
       OP_INSET, OP_NOT_INSET };
// agg ops
enum { AGGOP_COUNT = 0, AGGOP_SUM, AGGOP_MIN, AGGOP_MAX };

// group 0 terms AND together; groups >= 1 are OR-clauses: the row must
// satisfy at least one term of every present group (CNF — covers
// `(a=1 OR a=2)` and `x IN (...)`)
struct QTerm { uint8_t family; uint8_t op; uint16_t idx; uint8_t group;
               uint64_t v0, v1; };
struct QKey  { uint8_t family; uint16_t idx; uint32_t bucket; };  // bucket: seconds per bucket for SRC_TIME_BUCKET
struct QAgg  { uint8_t op; uint8_t family; uint16_t idx; };

#define QMAX_TERMS 16
#define QMAX_KEYS 4
#define QMAX_AGGS 8

struct QuerySpec {
    QTerm terms[QMAX_TERMS];
    QKey keys[QMAX_KEYS];
    QAgg aggs[QMAX_AGGS];
    uint32_t n_terms, n_keys, n_aggs;
    uint64_t time_base_s;
};

// epc/ip column indices are identical in the L7 and L4 u32 layouts
// (vtap, ip4_0, ip4_1, epc_0, epc_1 — asserted in the layout headers)
DEV uint64_t kg_join(const SegView& s, uint64_t row, uint16_t idx) {
    if (s.kg_tk == nullptr) return 0;
    uint32_t side = idx / KG_VALS_N, j = idx % KG_VALS_N;
    uint32_t epc = s.u32c[(uint64_t)(3 + side) * s.stride + row];
    uint32_t ip = s.u32c[(uint64_t)(1 + side) * s.stride + row];
    uint64_t k = ((uint64_t)epc << 32) | ip;
    uint32_t slot = table_find(s.kg_tk, s.kg_mask, k,
                               (uint32_t)(mix64(k) & s.kg_mask));
    return slot == ROW_NONE ? 0 : s.kg_tv[(uint64_t)slot * KG_VALS_N + j];
}

DEV uint64_t src_value(const SegView& s, uint64_t row, uint8_t family,
                       uint16_t idx, uint32_t bucket, uint64_t time_base_s) {
    switch (family) {
        case SRC_U64: return s.u64c[(uint64_t)idx * s.stride + row];
        case SRC_U32: return s.u32c[(uint64_t)idx * s.stride + row];
        case SRC_U8:  return s.u8c[(uint64_t)idx * s.stride + row];
        case SRC_DID: return s.didc[(uint64_t)idx * s.stride + row];
        case SRC_KG:  return kg_join(s, row, idx);
        case SRC_ATTR_VAL: {
            // idx is the attr slot (0..cnt-1); value ids follow name ids in
            // the row's attr-pool block
            uint32_t cnt = s.attr_cnt[row];
            if (idx >= cnt) return DICT_ID_INVALID;
            return (uint32_t)s.attr_pool[s.attr_start[row] + cnt + idx];
        }
        case SRC_TIME_BUCKET: {
            uint64_t t_s = s.u64c[L7_U64_START_TIME * s.stride + row] / 1000000000ull;
            uint64_t rel = t_s > time_base_s ? t_s - time_base_s : 0;
            return bucket ? (rel / bucket) * bucket : rel;
        }
        case SRC_STR_HASH:
            return seg_pool_hash(s, row, idx);
        case SRC_TRACE128:
            return idx == 0 ? seg_trace_key(s, row) : seg_span_key(s, row);
        default: return 0;
    }
}

DEV bool eval_terms(const SegView& s, uint64_t row, const QuerySpec& q) {
    uint32_t need = 0, have = 0;
    for (uint32_t t = 0; t < q.n_terms; t++) {
        const QTerm& term = q.terms[t];
        if (term.family == SRC_ATTR_MATCH) {
            uint32_t cnt = s.attr_cnt[row];
            uint32_t start = s.attr_start[row];
            bool okm = false;
            for (uint32_t a = 0; a < cnt && !okm; a++)
                okm = (uint32_t)s.attr_pool[start + a] == (uint32_t)term.v0 &&
                      (uint32_t)s.attr_pool[start + cnt + a] ==
                          (uint32_t)term.v1;
            if (term.op == OP_NE) okm = !okm;
            if (term.group == 0) {
                if (!okm) return false;
            } else {
                uint32_t bit = 1u << (term.group & 31);
                need |= bit;
                if (okm) have |= bit;
            }
            continue;
        }
        uint64_t v = src_value(s, row, term.family, term.idx, 0, q.time_base_s);
        bool ok;
        switch (term.op) {
            case OP_EQ: ok = v == term.v0; break;
            case OP_NE: ok = v != term.v0; break;
            case OP_LT: ok = v < term.v0; break;
            case OP_LE: ok = v <= term.v0; break;
            case OP_GT: ok = v > term.v0; break;
            case OP_GE: ok = v >= term.v0; break;
            case OP_BETWEEN: ok = v >= term.v0 && v <= term.v1; break;
            case OP_INSET:
            case OP_NOT_INSET: {
                bool in = v < term.v1 &&
                    ((reinterpret_cast<const uint32_t*>(term.v0)[v >> 5]
                      >> (v & 31)) & 1);
                ok = in == (term.op == OP_INSET);
                break;
            }
            default: ok = true;
        }
        if (term.group == 0) {
            if (!ok) return false;
        } else {
            uint32_t bit = 1u << (term.group & 31);
            need |= bit;
            if (ok) have |= bit;
        }
    }
    return (have & need) == need;
}

// The name of a group, on every path: the direct kernel, both passes of the
// partitioned one and K15 land rows of one key tuple in one slot of one
// table only because they all come through here (host twin:
// tests/query_cases.py group_hash).
constexpr uint64_t GROUP_HASH_SEED = 0x243F6A8885A308D3ull;
// EMPTY_KEY marks a free slot: the tuple that hashes to it is stored as this
constexpr uint64_t GROUP_HASH_OF_ZERO = 1;

DEV uint64_t group_hash_mix(uint64_t h, uint32_t k, uint64_t key) {
    return mix64(h ^ key ^ ((uint64_t)k << 56));
}

DEV uint64_t group_hash_end(uint64_t h) {
    if (h == EMPTY_KEY) h = GROUP_HASH_OF_ZERO;
    return h;
}

DEV uint64_t group_hash(const uint64_t* kraw, uint32_t n_keys) {
    uint64_t h = GROUP_HASH_SEED;
    for (uint32_t k = 0; k < n_keys; k++) h = group_hash_mix(h, k, kraw[k]);
    return group_hash_end(h);
}

// The key values of a segment row into kraw[QMAX_KEYS]; -> their group
// hash. Each value is read and mixed in one pass, so a caller that never
// looks at kraw (the partition passes that only want a bucket) keeps no
// key value alive. kraw is the caller's own array: saying so keeps the
// stores to it from ordering the segment reads, and the kernels close to
// the code they had with this loop written out in each of them.
DEV uint64_t row_group_hash(const SegView& s, const QuerySpec& q,
                            uint64_t row, uint64_t* __restrict__ kraw) {
    uint64_t h = GROUP_HASH_SEED;
    for (uint32_t k = 0; k < q.n_keys; k++) {
        kraw[k] = src_value(s, row, q.keys[k].family, q.keys[k].idx,
                            q.keys[k].bucket, q.time_base_s);
        h = group_hash_mix(h, k, kraw[k]);
    }
    return group_hash_end(h);
}

// group table: gkeys u64 hash (claim word), graw [cap, QMAX_KEYS] raw key
// values, gvals [cap, QMAX_AGGS] u64 accumulators (min encoded as ~v).
// group claim: load-first probe, CAS on empty (shared by both agg paths).
// A full table (every slot probed, none free or matching) yields
// GROUP_FULL: the caller counts the row as overflow instead of merging it
// into another group; the host reruns with a larger table.
constexpr uint32_t GROUP_FULL = ROW_NONE;

DEV uint32_t group_claim(uint64_t h, const uint64_t* kraw, uint32_t n_keys,
                         uint64_t* gkeys, uint64_t* graw,
                         uint32_t cap_mask) {
    uint32_t slot = (uint32_t)(h & cap_mask);
    for (uint32_t probe = 0; probe <= cap_mask; probe++) {
        uint64_t cur = gkeys[slot];
        if (cur == h) return slot;
        if (cur == EMPTY_KEY) {
            uint64_t old = atomicCAS((unsigned long long*)&gkeys[slot],
                                     EMPTY_KEY, h);
            if (old == EMPTY_KEY) {
                for (uint32_t k = 0; k < n_keys; k++)
                    graw[(uint64_t)slot * QMAX_KEYS + k] = kraw[k];
                return slot;
            }
            if (old == h) return slot;
        }
        slot = (slot + 1) & cap_mask;
    }
    return GROUP_FULL;
}

constexpr uint32_t QAGG_NSLOT = 512;
// "no COUNT aggregate in the spec" marker for agg_count_slot()
constexpr uint32_t NO_COUNT_AGG = 0xFFFFFFFFu;

// A COUNT accumulator already is the per-slot row tally the overflow
// report needs; only specs without one pay for the separate lrows add.
DEV uint32_t agg_count_slot(const QuerySpec& q) {
    for (uint32_t a = 0; a < q.n_aggs; a++)
        if (q.aggs[a].op == AGGOP_COUNT) return a;
    return NO_COUNT_AGG;
}

// what an accumulator of `op` holds before its first value
DEV unsigned long long agg_identity(uint32_t op) {
    return op == AGGOP_MIN ? ~0ull : 0ull;
}

// One accumulate step. Inlined into each caller, so every copy still sees
// whether its accumulator is LDS or global. That rests on the inliner, and
// was checked in the gfx950 assembly: k_query_agg and k_qpart_agg issue
// ds_add_u64 / ds_min_u64 / ds_max_u64 on the LDS path and the unit holds
// no flat atomic. Handing both kinds to ONE call site behind a runtime pointer
// forces FLAT atomics on the LDS path (the compiler can no longer prove
// addrspace(3)) — measured 2.7x slower on the direct kernel.
DEV void agg_accum(unsigned long long* acc, uint32_t op,
                   unsigned long long v) {
    if (op == AGGOP_COUNT || op == AGGOP_SUM) atomicAdd(acc, v);
    else if (op == AGGOP_MIN) atomicMin(acc, v);
    else atomicMax(acc, v);
}

// One row's LDS-table aggregation (shared by the direct and the
// partitioned kernels): probe/claim the block-local table, accumulate;
// on LDS saturation fall through to the global table directly.
DEV void agg_vals_lds(const QuerySpec& q, uint64_t h,
                      const uint64_t* kraw, const uint64_t* varr,
                      uint64_t* lkey, uint32_t* lgslot, uint32_t* lrows,
                      unsigned long long (*lagg)[QMAX_AGGS],
                      uint64_t* gkeys, uint64_t* graw,
                      unsigned long long* gvals, uint32_t cap_mask,
                      uint32_t cnt_a, uint32_t* overflow) {
    uint32_t slot = (uint32_t)h & (QAGG_NSLOT - 1);
    uint32_t gslot = 0xFFFFFFFFu;
    for (uint32_t probe = 0; probe < 16; probe++) {
        uint64_t cur = lkey[slot];
        if (cur == EMPTY_KEY) {
            uint64_t old = atomicCAS((unsigned long long*)&lkey[slot],
                                     (unsigned long long)EMPTY_KEY,
                                     (unsigned long long)h);
            if (old == EMPTY_KEY) {
                lgslot[slot] = group_claim(h, kraw, q.n_keys, gkeys, graw,
                                           cap_mask);
                __threadfence_block();
                cur = h;
            } else {
                cur = old;
            }
        }
        if (cur == h) {
            gslot = slot;
            break;
        }
        slot = (slot + 1) & (QAGG_NSLOT - 1);
    }
    if (gslot != 0xFFFFFFFFu) {
        if (cnt_a == NO_COUNT_AGG) atomicAdd(&lrows[gslot], 1u);
        for (uint32_t a = 0; a < q.n_aggs; a++)
            agg_accum(&lagg[gslot][a], q.aggs[a].op, varr[a]);
    } else {  // LDS table saturated for this key: go global directly
        uint32_t g = group_claim(h, kraw, q.n_keys, gkeys, graw, cap_mask);
        if (g == GROUP_FULL) {
            atomicAdd(overflow, 1u);
            return;
        }
        unsigned long long* acc = &gvals[(uint64_t)g * QMAX_AGGS];
        for (uint32_t a = 0; a < q.n_aggs; a++)
            agg_accum(&acc[a], q.aggs[a].op, varr[a]);
    }
}

DEV void agg_row_lds(const SegView& s, const QuerySpec& q, uint64_t row,
                     uint64_t* lkey, uint32_t* lgslot, uint32_t* lrows,
                     unsigned long long (*lagg)[QMAX_AGGS],
                     uint64_t* gkeys, uint64_t* graw,
                     unsigned long long* gvals, uint32_t cap_mask,
                     uint32_t cnt_a, uint32_t* overflow) {
    uint64_t kraw[QMAX_KEYS];
    uint64_t h = row_group_hash(s, q, row, kraw);
    uint64_t varr[QMAX_AGGS];
    for (uint32_t a = 0; a < q.n_aggs; a++)
        varr[a] = q.aggs[a].op == AGGOP_COUNT ? 1
            : src_value(s, row, q.aggs[a].family, q.aggs[a].idx, 0,
                        q.time_base_s);
    agg_vals_lds(q, h, kraw, varr, lkey, lgslot, lrows, lagg, gkeys, graw,
                 gvals, cap_mask, cnt_a, overflow);
}

DEV void agg_lds_init(const QuerySpec& q, uint64_t* lkey, uint32_t* lrows,
                      unsigned long long (*lagg)[QMAX_AGGS]) {
    for (uint32_t sl = threadIdx.x; sl < QAGG_NSLOT; sl += blockDim.x) {
        lkey[sl] = EMPTY_KEY;
        lrows[sl] = 0;
        for (uint32_t a = 0; a < q.n_aggs; a++)
            lagg[sl][a] = agg_identity(q.aggs[a].op);
    }
}

DEV void agg_lds_flush(const QuerySpec& q, const uint64_t* lkey,
                       const uint32_t* lgslot, const uint32_t* lrows,
                       unsigned long long (*lagg)[QMAX_AGGS],
                       unsigned long long* gvals, uint32_t cnt_a,
                       uint32_t* overflow) {
    for (uint32_t sl = threadIdx.x; sl < QAGG_NSLOT; sl += blockDim.x) {
        if (lkey[sl] == EMPTY_KEY) continue;
        if (lgslot[sl] == GROUP_FULL) {
            // the group never got a global slot: report its rows
            uint32_t rows = cnt_a == NO_COUNT_AGG ? lrows[sl]
                                                  : (uint32_t)lagg[sl][cnt_a];
            atomicAdd(overflow, rows);
            continue;
        }
        unsigned long long* acc = &gvals[(uint64_t)lgslot[sl] * QMAX_AGGS];
        for (uint32_t a = 0; a < q.n_aggs; a++) {
            uint32_t op = q.aggs[a].op;
            unsigned long long v = lagg[sl][a];
            // an accumulator nothing reached costs no global atomic
            if (v != agg_identity(op)) agg_accum(&acc[a], op, v);
        }
    }
}

__global__ void k_query_agg(SegView s, QuerySpec q, uint32_t n, uint64_t base_row,
                            uint64_t* __restrict__ gkeys,
                            uint64_t* __restrict__ graw,
                            unsigned long long* __restrict__ gvals,
                            uint32_t cap_mask,
                            uint32_t* __restrict__ overflow) {
    // Grid-strided scan with an LDS-resident group table: each workgroup
    // aggregates its stripe into shared memory (~40 KB of the 160 KB/CU
    // LDS: 512 slots x (key + global-slot + row tally + 8 accumulators)) and flushes
    // once at the end — global atomics drop from per-row to
    // per-(block x live slot). Groups are identified by the 64-bit mixed
    // key hash (same convention as the global table); the LDS claimant
    // registers the group globally immediately, so raw keys never stage
    // in LDS. Rows whose key misses the table (very high per-block
    // cardinality) fall back to per-lane global accumulation.
    __shared__ uint64_t lkey[QAGG_NSLOT];
    __shared__ uint32_t lgslot[QAGG_NSLOT];
    __shared__ uint32_t lrows[QAGG_NSLOT];
    __shared__ unsigned long long lagg[QAGG_NSLOT][QMAX_AGGS];
    const uint32_t cnt_a = agg_count_slot(q);
    agg_lds_init(q, lkey, lrows, lagg);
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t row = base_row + i;
        if (!eval_terms(s, row, q)) continue;
        agg_row_lds(s, q, row, lkey, lgslot, lrows, lagg, gkeys, graw,
                    gvals, cap_mask, cnt_a, overflow);
    }
    __syncthreads();
    agg_lds_flush(q, lkey, lgslot, lrows, lagg, gvals, cnt_a, overflow);
}

// ---- K15: exact distinct counts per group (Uniq / UniqExact) ----
// A second pass over the rows k_query_agg saw, into the same group table:
// guniq[slot][u] lines up with gvals[slot] because both kernels take the
// group's hash h from row_group_hash(). What is counted is the number of
// distinct (group, value tuple) PAIRS, each identified by a 64-bit hash
// that is claimed once in a query-scoped table `pkeys` (dftable.h rules):
//
//   vh   = UNIQ_SEED ^ ((u + 1) * 0x9E3779B97F4A7C15)       for item u
//   vh   = mix64(vh ^ value_j ^ (j << 56))                  for each arg j
//   pair = mix64(h ^ vh), 0 -> 1
//
// (host twin: query/spec.py UNIQ_SEED; tests/uniq_cases.py pair_hash).
// value_j is src_value() of the argument with bucket 0. The thread whose
// CAS claims the pair adds 1 to its group's counter; everybody else who
// meets the pair, in this launch or a later one on the same tables, adds
// nothing. Two different pairs with one 64-bit hash count once.
#define QMAX_UNIQ 4
#define QMAX_UNIQ_ARGS 4

struct QUniqCol { uint8_t family; uint16_t idx; };
struct QUniq { QUniqCol cols[QMAX_UNIQ_ARGS]; uint32_t n_args; };
struct UniqSpec { QUniq items[QMAX_UNIQ]; uint32_t n_uniq; };

constexpr uint64_t UNIQ_SEED = 0x13198A2E03707344ull;
constexpr uint64_t UNIQ_ITEM_MUL = 0x9E3779B97F4A7C15ull;
// Block-local filter of recently seen pairs: direct-mapped, 4096 x 8 B =
// 32 KB of LDS. The index is bits 32..43 of the pair hash: the pair table
// starts its probe at the low bits of mix64(pair) and the group tables use
// the low bits of h, so these bits are spent nowhere else.
constexpr uint32_t UNIQ_FILTER_SLOTS = 4096;
constexpr uint32_t UNIQ_FILTER_SHIFT = 32;
// Fewer, longer-lived workgroups than k_query_agg: a filter slot pays off
// only when its block meets the pair again, and 4 blocks x 32 KB still fit
// a CU's LDS.
constexpr uint32_t UNIQ_MAX_BLOCKS = 1024;

// One atomicAdd per (wave, counter) instead of one per lane. With few
// groups every claimed pair lands on the same guniq word, and 4M adds to one
// address were the whole kernel (48 ms against 0.1 ms for k_query_agg,
// the rate of one contended L2 word). Each round the lanes here that
// share the first lane's counter index elect their lowest lane, which adds
// their number; a round retires at least one lane, so 64 rounds retire
// every lane of the wave. Which lanes the compiler keeps together at this
// point only decides how much is merged: every lane is counted once,
// either in its cohort's popcount or by the add of its own below.
DEV void uniq_count_add(unsigned long long* guniq, uint32_t idx) {
    for (uint32_t r = 0; r < 64; r++) {
        uint32_t first = __builtin_amdgcn_readfirstlane(idx);
        // the vote is taken by every lane still in the loop, on the
        // predicate itself: a ballot of `true` inside the branch came back
        // with lanes of other counters in it
        bool mine = idx == first;
        unsigned long long peers = __ballot(mine);
        if (mine) {
            if ((threadIdx.x & 63) == (uint32_t)__ffsll(peers) - 1)
                atomicAdd(&guniq[idx], (unsigned long long)__popcll(peers));
            return;
        }
    }
    atomicAdd(&guniq[idx], 1ull);
}

template <bool FILTER>
__global__ void __launch_bounds__(256)
k_query_uniq(SegView s, QuerySpec q, UniqSpec us, uint32_t n,
             uint64_t base_row,
             uint64_t* __restrict__ gkeys, uint64_t* __restrict__ graw,
             uint32_t cap_mask,
             unsigned long long* __restrict__ guniq,  // [cap][QMAX_UNIQ]
             uint64_t* __restrict__ pkeys, uint32_t pcap_mask,
             uint32_t* __restrict__ overflow) {  // [0] group, [1] pair table
    // The filter may say "not seen" of a pair that was seen (an evicted or
    // raced slot: one redundant global probe, which finds the pair claimed)
    // but never "seen" of one that was not: a slot only ever holds a whole
    // pair hash that some thread of this block stored on its way to
    // table_claim, or 0, which no pair equals. Whole, because the slot is
    // one naturally aligned 8-byte word read and written by relaxed atomic
    // load/store (one ds_read_b64 / ds_write_b64 each): C++ atomics do
    // not tear, so a read returns what ONE store wrote, never the halves
    // of two. No ordering is needed: the storing thread goes on to claim
    // the pair itself, whoever else skips it.
    __shared__ uint64_t seen[FILTER ? UNIQ_FILTER_SLOTS : 1];
    if (FILTER) {
        for (uint32_t sl = threadIdx.x; sl < UNIQ_FILTER_SLOTS;
             sl += blockDim.x)
            seen[sl] = EMPTY_KEY;
        __syncthreads();
    }
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t row = base_row + i;
        if (!eval_terms(s, row, q)) continue;
        uint64_t kraw[QMAX_KEYS];
        uint64_t h = row_group_hash(s, q, row, kraw);
        for (uint32_t u = 0; u < us.n_uniq; u++) {
            const QUniq& it = us.items[u];
            uint64_t vh = UNIQ_SEED ^ ((uint64_t)(u + 1) * UNIQ_ITEM_MUL);
            for (uint32_t j = 0; j < it.n_args; j++)
                vh = mix64(vh ^ src_value(s, row, it.cols[j].family,
                                          it.cols[j].idx, 0, q.time_base_s)
                           ^ ((uint64_t)j << 56));
            uint64_t pair = mix64(h ^ vh);
            if (pair == EMPTY_KEY) pair = 1;
            if (FILTER) {
                uint32_t fi = (uint32_t)(pair >> UNIQ_FILTER_SHIFT) &
                              (UNIQ_FILTER_SLOTS - 1);
                if (__hip_atomic_load(&seen[fi], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP) == pair)
                    continue;
                __hip_atomic_store(&seen[fi], pair, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            bool claimed;
            uint32_t ps = table_claim(pkeys, pcap_mask, pair,
                                      (uint32_t)(mix64(pair) & pcap_mask),
                                      &claimed);
            if (ps == ROW_NONE) {
                atomicAdd(&overflow[1], 1u);
                continue;
            }
            if (!claimed) continue;
            uint32_t g = group_claim(h, kraw, q.n_keys, gkeys, graw,
                                     cap_mask);
            if (g == GROUP_FULL) atomicAdd(&overflow[0], 1u);
            else uniq_count_add(guniq, g * QMAX_UNIQ + u);
        }
    }
}

// ---- radix-partitioned group-by (high cardinality) ----
// When the key cardinality is far above QAGG_NSLOT, the direct kernel
// spills most rows to per-row global atomics. The partitioned path
// buckets rows by 8 hash bits first, then aggregates one bucket per
// workgroup group: each block then sees ~1/256th of the distinct keys,
// so the LDS table holds them all (zero spill up to ~128k groups).
constexpr uint32_t QPART_NB = 256;
constexpr uint32_t QPART_SHIFT = 40;

DEV uint32_t qpart_bucket(uint64_t h) {
    return (uint32_t)(h >> QPART_SHIFT) & (QPART_NB - 1);
}

// The count pass and the first scatter pass want the bucket alone: the key
// values row_group_hash() hands them are never read, and their stores go.
__global__ void k_qpart_count(SegView s, QuerySpec q, uint32_t n,
                              uint64_t base_row,
                              uint32_t* __restrict__ counts) {
    __shared__ uint32_t lc[QPART_NB];
    for (uint32_t i = threadIdx.x; i < QPART_NB; i += blockDim.x)
        lc[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t row = base_row + i;
        if (!eval_terms(s, row, q)) continue;
        uint64_t kraw[QMAX_KEYS];
        atomicAdd(&lc[qpart_bucket(row_group_hash(s, q, row, kraw))], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < QPART_NB; i += blockDim.x)
        if (lc[i]) atomicAdd(&counts[i], lc[i]);
}

// The scatter stores the COMPUTED per-row payload (key values +
// aggregate operands), not row ids: pass 3 then reads each bucket as a
// dense sequential stripe. Scattering ids instead was measured SLOWER
// than the direct kernel (the bucketed pass degenerates into random
// 8-byte gathers across the whole segment).
__global__ void k_qpart_scatter(SegView s, QuerySpec q, uint32_t n,
                                uint64_t base_row,
                                uint32_t* __restrict__ cursors,
                                uint64_t* __restrict__ out_pay) {
    // two-pass block staging over a CONTIGUOUS per-block stripe: count
    // the stripe's bucket histogram in LDS, reserve one contiguous
    // chunk per (block, bucket) with a single global atomic each, then
    // write. A naive per-row atomicAdd on 256 global cursors serializes
    // 30M RMWs onto 4 cache lines.
    __shared__ uint32_t lc[QPART_NB];
    __shared__ uint32_t lbase[QPART_NB];
    uint32_t w = q.n_keys + q.n_aggs;
    uint64_t per = ((uint64_t)n + gridDim.x - 1) / gridDim.x;
    uint64_t lo = (uint64_t)blockIdx.x * per;
    uint64_t hi = lo + per < n ? lo + per : n;
    for (uint32_t i = threadIdx.x; i < QPART_NB; i += blockDim.x)
        lc[i] = 0;
    __syncthreads();
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint64_t row = base_row + i;
        if (!eval_terms(s, row, q)) continue;
        uint64_t kraw[QMAX_KEYS];
        atomicAdd(&lc[qpart_bucket(row_group_hash(s, q, row, kraw))], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < QPART_NB; i += blockDim.x) {
        uint32_t c = lc[i];
        lbase[i] = c ? atomicAdd(&cursors[i], c) : 0u;
        lc[i] = 0;
    }
    __syncthreads();
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        uint64_t row = base_row + i;
        if (!eval_terms(s, row, q)) continue;
        uint64_t kraw[QMAX_KEYS];
        uint32_t b = qpart_bucket(row_group_hash(s, q, row, kraw));
        uint32_t pos = lbase[b] + atomicAdd(&lc[b], 1u);
        uint64_t* dst = out_pay + (uint64_t)pos * w;
        for (uint32_t k = 0; k < q.n_keys; k++) dst[k] = kraw[k];
        for (uint32_t a = 0; a < q.n_aggs; a++)
            dst[q.n_keys + a] = q.aggs[a].op == AGGOP_COUNT ? 1
                : src_value(s, row, q.aggs[a].family, q.aggs[a].idx, 0,
                            q.time_base_s);
    }
}

// Single-block exclusive scan over the QPART_NB per-bucket counts, between
// the count and the scatter pass. Out: counts[b] = cursors[b] = the offset
// at which bucket b starts in the payload. The scatter then advances
// cursors[b] by one per row, so when it is done cursors[b] is where bucket b
// ends, while counts[b] still says where it starts.
__global__ void k_qpart_prefix(uint32_t* counts, uint32_t* cursors) {
    __shared__ uint32_t vals[QPART_NB];
    uint32_t i = threadIdx.x;
    vals[i] = counts[i];
    __syncthreads();
    // simple serial scan by lane 0 (256 values; latency-trivial)
    if (i == 0) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < QPART_NB; k++) {
            counts[k] = acc;
            cursors[k] = acc;
            acc += vals[k];
        }
    }
}

__global__ void k_qpart_agg(QuerySpec q,
                            const uint64_t* __restrict__ pay,
                            const uint32_t* __restrict__ starts,
                            const uint32_t* __restrict__ ends,
                            uint64_t* __restrict__ gkeys,
                            uint64_t* __restrict__ graw,
                            unsigned long long* __restrict__ gvals,
                            uint32_t cap_mask,
                            uint32_t blocks_per_bucket,
                            uint32_t* __restrict__ overflow) {
    __shared__ uint64_t lkey[QAGG_NSLOT];
    __shared__ uint32_t lgslot[QAGG_NSLOT];
    __shared__ uint32_t lrows[QAGG_NSLOT];
    __shared__ unsigned long long lagg[QAGG_NSLOT][QMAX_AGGS];
    const uint32_t cnt_a = agg_count_slot(q);
    agg_lds_init(q, lkey, lrows, lagg);
    __syncthreads();
    uint32_t w = q.n_keys + q.n_aggs;
    uint32_t bucket = blockIdx.x / blocks_per_bucket;
    uint32_t sub = blockIdx.x % blocks_per_bucket;
    uint32_t lo = starts[bucket], hi = ends[bucket];
    // rows were pre-filtered and their payload materialized by the
    // scatter pass: this is a dense sequential read, no SegView access
    for (uint64_t j = lo + (uint64_t)sub * blockDim.x + threadIdx.x;
         j < hi; j += (uint64_t)blocks_per_bucket * blockDim.x) {
        const uint64_t* row = pay + j * w;
        agg_vals_lds(q, group_hash(row, q.n_keys), row, row + q.n_keys,
                     lkey, lgslot, lrows, lagg, gkeys, graw, gvals,
                     cap_mask, cnt_a, overflow);
    }
    __syncthreads();
    agg_lds_flush(q, lkey, lgslot, lrows, lagg, gvals, cnt_a, overflow);
}

// non-aggregated SELECT: emit matching row ids (bounded)
__global__ void k_query_select(SegView s, QuerySpec q, uint32_t n, uint64_t base_row,
                               uint64_t* __restrict__ out_rows,
                               uint32_t* __restrict__ out_ctr, uint32_t out_cap) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t row = base_row + i;
    if (!eval_terms(s, row, q)) return;
    uint32_t e = atomicAdd(out_ctr, 1u);
    if (e < out_cap) out_rows[e] = row;
}

// The one way a host-built spec reaches a kernel: copy the bytes, then
// refuse, before any launch, what the kernels would index their fixed-size
// arrays with, read past the segment with, or mask a probe with. `cap` is
// the group table's slot count; an entry point without a table leaves it.
int load_spec(QuerySpec& q, const void* spec, const SegView& s, uint32_t n,
              uint64_t base_row, uint32_t cap = 1) {
    __builtin_memcpy(&q, spec, sizeof(QuerySpec));
    bool ok = q.n_terms <= QMAX_TERMS && q.n_keys <= QMAX_KEYS &&
              q.n_aggs <= QMAX_AGGS && base_row + n <= s.stride &&
              cap != 0 && (cap & (cap - 1)) == 0;
    return ok ? 0 : (int)hipErrorInvalidValue;
}

}  // namespace

// C API (ctypes), as in dfgpu.hip: the HIP stream as uint64, hipError_t as
// int, launches async on that stream. `seg` is a host SegView
// (ops/gpu_ops.py seg_view), `spec` host-built QuerySpec bytes; both are
// read before the call returns. A bad spec is hipErrorInvalidValue and
// n == 0 is a success, either way without a launch.
extern "C" {

int df_query_agg(const void* seg, const void* spec, uint32_t n,
                 uint64_t base_row,
                 void* gkeys, void* graw, void* gvals, uint32_t cap,
                 void* overflow,  // u32: rows whose group found no slot
                 uint64_t stream) {
    SegView s = seg_view_load(seg);
    QuerySpec q;
    if (int rc = load_spec(q, spec, s, n, base_row, cap)) return rc;
    if (n == 0) return 0;
    // grid-stride kernel: bounded grid so each workgroup amortizes its
    // LDS group table over many rows (still >> 256 workgroups: 4096
    // covers all 8 XCDs with deep occupancy)
    uint32_t blocks = grid_for(n);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_query_agg, dim3(blocks), dim3(BLOCK), 0, STREAM(stream),
                       s, q, n, base_row, (uint64_t*)gkeys, (uint64_t*)graw,
                       (unsigned long long*)gvals, cap - 1,
                       (uint32_t*)overflow);
    return (int)hipGetLastError();
}

// K15 distinct counts: one launch per segment into the group table of
// df_query_agg plus a query-scoped pair table (`pcap` slots, power of
// two). overflow[0]: claimed pairs whose group found no slot; overflow[1]:
// pairs that found no slot in the pair table. Either one non-zero means
// "rerun with fresh, larger tables". use_filter = 0 runs without the
// block-local LDS filter (same results; benchmarks/query_uniq.py).
int df_query_uniq(const void* seg, const void* spec, const void* uspec,
                  uint32_t n, uint64_t base_row,
                  void* gkeys, void* graw, uint32_t cap, void* guniq,
                  void* pkeys, uint32_t pcap, void* overflow,
                  uint32_t use_filter, uint64_t stream) {
    SegView s = seg_view_load(seg);
    QuerySpec q;
    if (int rc = load_spec(q, spec, s, n, base_row, cap)) return rc;
    UniqSpec us;
    __builtin_memcpy(&us, uspec, sizeof(UniqSpec));
    // the kernel indexes items and columns by these counts too, and masks
    // its pair probes with pcap - 1
    if (us.n_uniq > QMAX_UNIQ ||
        cap > (1u << 28) ||  // counter indices (slot * QMAX_UNIQ + u) are u32
        pcap == 0 || (pcap & (pcap - 1)))
        return (int)hipErrorInvalidValue;
    for (uint32_t u = 0; u < us.n_uniq; u++)
        if (us.items[u].n_args > QMAX_UNIQ_ARGS)
            return (int)hipErrorInvalidValue;
    if (n == 0 || us.n_uniq == 0) return 0;
    uint32_t blocks = grid_for(n);
    if (blocks > UNIQ_MAX_BLOCKS) blocks = UNIQ_MAX_BLOCKS;
    auto kernel = use_filter ? k_query_uniq<true> : k_query_uniq<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(BLOCK), 0, STREAM(stream),
                       s, q, us, n, base_row, (uint64_t*)gkeys,
                       (uint64_t*)graw, cap - 1, (unsigned long long*)guniq,
                       (uint64_t*)pkeys, pcap - 1, (uint32_t*)overflow);
    return (int)hipGetLastError();
}

uint32_t df_uniq_spec_size() { return sizeof(UniqSpec); }

// the constants tests/uniq_cases.py rebuilds the pair hash and the filter
// index from
void df_uniq_consts(uint64_t* seed, uint64_t* item_mul,
                    uint32_t* filter_slots, uint32_t* filter_shift) {
    *seed = UNIQ_SEED; *item_mul = UNIQ_ITEM_MUL;
    *filter_slots = UNIQ_FILTER_SLOTS; *filter_shift = UNIQ_FILTER_SHIFT;
}

// Radix-partitioned aggregation in four launches on the stream, no host
// sync: count rows per bucket, scan, scatter the rows' payload bucket by
// bucket into row_scratch (u64[n * (n_keys + n_aggs)]), aggregate.
// counts / cursors: QPART_NB u32 device words each, counts zeroed by the
// caller.
int df_qpart_agg(const void* seg, const void* spec, uint32_t n,
                 uint64_t base_row,
                 void* counts, void* cursors, void* row_scratch,
                 void* gkeys, void* graw, void* gvals, uint32_t cap,
                 void* overflow,  // u32: rows whose group found no slot
                 uint64_t stream) {
    SegView s = seg_view_load(seg);
    QuerySpec q;
    if (int rc = load_spec(q, spec, s, n, base_row, cap)) return rc;
    if (n == 0) return 0;
    uint32_t blocks = grid_for(n);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_qpart_count, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), s, q, n, base_row,
                       (uint32_t*)counts);
    // counts[b] and cursors[b] both become bucket b's start
    hipLaunchKernelGGL(k_qpart_prefix, dim3(1), dim3(QPART_NB), 0,
                       STREAM(stream), (uint32_t*)counts,
                       (uint32_t*)cursors);
    // cursors[b] moves on to bucket b's end
    hipLaunchKernelGGL(k_qpart_scatter, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), s, q, n, base_row,
                       (uint32_t*)cursors, (uint64_t*)row_scratch);
    // starts = counts, ends = cursors
    constexpr uint32_t BPB = 16;
    hipLaunchKernelGGL(k_qpart_agg, dim3(QPART_NB * BPB), dim3(BLOCK), 0,
                       STREAM(stream), q, (const uint64_t*)row_scratch,
                       (const uint32_t*)counts, (const uint32_t*)cursors,
                       (uint64_t*)gkeys, (uint64_t*)graw,
                       (unsigned long long*)gvals, cap - 1, BPB,
                       (uint32_t*)overflow);
    return (int)hipGetLastError();
}

int df_query_select(const void* seg, const void* spec, uint32_t n,
                    uint64_t base_row,
                    void* out_rows, void* out_ctr, uint32_t out_cap,
                    uint64_t stream) {
    SegView s = seg_view_load(seg);
    QuerySpec q;
    if (int rc = load_spec(q, spec, s, n, base_row)) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_query_select, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       s, q, n, base_row, (uint64_t*)out_rows, (uint32_t*)out_ctr,
                       out_cap);
    return (int)hipGetLastError();
}

// rocPRIM device radix sort of u64 keys (grouped-percentile path: the
// composite (group << 44 | value) sort replaces torch.argsort on the
// quantile gather — VERDICT r1 #8). Two-phase: *temp_bytes == 0 sizes
// the temp buffer; second call sorts in place (double-buffered).
int df_sort_u64(void* data, void* data_alt, uint32_t n, void* temp,
                uint64_t* temp_bytes, uint64_t stream) {
    size_t bytes = (size_t)*temp_bytes;
    rocprim::double_buffer<uint64_t> keys((uint64_t*)data,
                                          (uint64_t*)data_alt);
    hipError_t rc = rocprim::radix_sort_keys(
        temp == nullptr ? nullptr : temp, bytes, keys, n, 0, 64,
        STREAM(stream));
    if (rc != hipSuccess) return (int)rc;
    *temp_bytes = bytes;
    if (temp != nullptr && keys.current() != (uint64_t*)data) {
        // result landed in the alternate buffer: copy back
        (void)hipMemcpyAsync(data, data_alt, (size_t)n * 8,
                             hipMemcpyDeviceToDevice, STREAM(stream));
    }
    return 0;
}

int df_spec_sizes(uint32_t* qterm, uint32_t* qkey, uint32_t* qagg, uint32_t* qspec) {
    *qterm = sizeof(QTerm); *qkey = sizeof(QKey); *qagg = sizeof(QAgg);
    *qspec = sizeof(QuerySpec);
    return 0;
}

// what ops/gpu_ops.py SegViewC is checked against: sizeof, and offsetof
// of every member in declaration order (SEG_VIEW_MEMBERS words)
uint32_t df_seg_view_size() { return sizeof(SegView); }
void df_seg_view_offsets(uint32_t* out) { seg_view_offsets(out); }

// out[0..1]: OP_INSET, OP_NOT_INSET (query/spec.py carries the same two)
void df_query_set_ops(uint32_t* out) {
    out[0] = OP_INSET;
    out[1] = OP_NOT_INSET;
}

}  // extern "C"
