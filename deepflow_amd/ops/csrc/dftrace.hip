// dftrace — K10: bulk trace-tree assembly and the service trace map.
//
// Links every span of a time window to its parent (a hash join on three
// relations), measures each span's depth, and folds the result into a
// per-trace summary table and a service->service edge table. Host twin and
// semantics: query/tracemap.py.
//
// Four launches per query, separated by kernel boundaries (nothing spins):
//   k_trace_extract  per segment, one thread per row: window + trace-key
//                    test, join keys into flat arrays indexed by GLOBAL row
//                    (scan order), inserts into the three first-row indexes
//   k_trace_link     one thread per row: parent row + link kind
//   k_trace_depth    bounded walk up the parent array
//   k_trace_fold     per-trace table + edge table (edges pre-aggregated per
//                    block in LDS: a handful of groups fed by every row)
// Only k_trace_extract sees segments; the rest read the flat arrays.
//
// Rules: wave = 64 lanes, blocks are multiples of 64; table rules are in
// dftable.h, segment access in dfseg.h. Particular to this unit:
//  - no kernel reads in the same launch what another workgroup wrote.
//  - table values are atomicMin/Max/Add words initialised by the host.
//  - an index key is the 64-bit mix of (trace key, join key, relation); two
//    different pairs with one mix would share a slot, the same 64-bit
//    identity the dictionary and the flame nodes already accept.
#include "dftable.h"
#include "dfseg.h"

namespace {

// depth walk bound; python twin query/tracemap.py MAX_TRACE_HOPS
constexpr uint32_t MAX_TRACE_HOPS = 4096;

enum { REL_SPAN = 0, REL_SYSCALL, REL_TCP, REL_N };
enum { LINK_NONE = 0, LINK_SPAN, LINK_SYSCALL, LINK_TCP };
// per-trace value words (python twin: tracemap.TV_*)
enum { TV_SPANS = 0, TV_ROOTS, TV_UNROOTED, TV_MAX_DEPTH, TV_ERRORS,
       TV_START_MIN, TV_END_MAX, TV_ROOT_ROW, TV_FIRST_ROW, TV_N };
// per-edge value words (python twin: tracemap.EV_*)
enum { EV_CALLS = 0, EV_SPAN, EV_SYSCALL, EV_TCP, EV_ERRORS, EV_DUR_NS,
       EV_N };

// query-scoped flat columns, indexed by global row
struct TraceFlat {
    uint64_t* tkey;     // trace key (0 = row does not take part)
    uint64_t* pkey;     // parent span key
    uint64_t* sreq;     // syscall_trace_id_request
    uint64_t* start;
    uint64_t* end;
    uint32_t* tcp;      // req_tcp_seq
    uint32_t* svc;      // service_name dictionary id
    uint8_t* tap;       // tap_side
    uint8_t* status;    // response_status
};

// three first-row indexes in one FirstRowIdx, relation r at
// [r * cap, (r + 1) * cap)
DEV uint64_t pair_key(uint64_t tkey, uint64_t k, uint32_t rel) {
    uint64_t h = mix64(mix64(tkey + rel) ^ k);
    return h ? h : 1ull;
}

DEV void idx_insert(const FirstRowIdx& ix, uint32_t rel, uint64_t tkey,
                    uint64_t k, uint32_t row) {
    first_row_insert(ix, (uint64_t)rel * ix.cap, pair_key(tkey, k, rel), row);
}

DEV uint32_t idx_find(const FirstRowIdx& ix, uint32_t rel, uint64_t tkey,
                      uint64_t k) {
    return first_row_find(ix, (uint64_t)rel * ix.cap, pair_key(tkey, k, rel));
}

// one thread per segment row
__global__ void k_trace_extract(SegView s, uint32_t base_row,
                                uint64_t time_start, uint64_t time_end,
                                TraceFlat f, FirstRowIdx ix) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (uint32_t)s.n_rows) return;
    uint32_t g = base_row + r;
    uint64_t start = s.u64c[(uint64_t)L7_U64_START_TIME * s.stride + r];
    uint64_t tkey = 0;
    if (start >= time_start && start <= time_end) tkey = seg_trace_key(s, r);
    f.tkey[g] = tkey;
    if (tkey == 0) return;
    uint64_t skey = seg_span_key(s, r);
    // parent id: the decoder's rule for span ids, applied to the pooled text
    uint32_t plen;
    const uint8_t* pp = seg_pool_str(s, r, L7_POOL_PARENT_SPAN_ID, plen);
    uint64_t pkey = 0;
    if (plen) {
        bool hex = plen == 16 && hex_parse64_with(
            [&](uint32_t i) -> uint8_t { return pp[i]; }, pkey);
        if (!hex) pkey = str_hash(pp, plen, STR_FILTER_SEED);
    }
    uint64_t sreq = s.u64c[(uint64_t)L7_U64_SYSCALL_REQ * s.stride + r];
    uint64_t sresp = s.u64c[(uint64_t)L7_U64_SYSCALL_RESP * s.stride + r];
    uint32_t tcp = s.u32c[(uint64_t)L7_U32_REQ_TCP_SEQ * s.stride + r];
    uint8_t tap = s.u8c[(uint64_t)L7_U8_TAP_SIDE * s.stride + r];
    f.pkey[g] = pkey;
    f.sreq[g] = sreq;
    f.start[g] = start;
    f.end[g] = s.u64c[(uint64_t)L7_U64_END_TIME * s.stride + r];
    f.tcp[g] = tcp;
    f.svc[g] = s.didc[(uint64_t)L7_DID_SERVICE_NAME * s.stride + r];
    f.tap[g] = tap;
    f.status[g] = s.u8c[(uint64_t)L7_U8_STATUS * s.stride + r];
    if (skey) idx_insert(ix, REL_SPAN, tkey, skey, g);
    if (sresp) idx_insert(ix, REL_SYSCALL, tkey, sresp, g);
    if (tcp && tap == 1) idx_insert(ix, REL_TCP, tkey, tcp, g);
}

// one thread per global row
__global__ void k_trace_link(TraceFlat f, FirstRowIdx ix, uint32_t n,
                             uint32_t* __restrict__ parent,
                             uint8_t* __restrict__ kind) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    uint64_t tkey = f.tkey[g];
    if (tkey == 0) return;
    uint32_t p = ROW_NONE;
    uint8_t k = LINK_NONE;
    uint64_t pkey = f.pkey[g];
    if (pkey) {
        uint32_t c = idx_find(ix, REL_SPAN, tkey, pkey);
        if (c != ROW_NONE && c != g) { p = c; k = LINK_SPAN; }
    }
    if (p == ROW_NONE) {
        uint64_t sreq = f.sreq[g];
        if (sreq) {
            uint32_t c = idx_find(ix, REL_SYSCALL, tkey, sreq);
            if (c != ROW_NONE && c != g) { p = c; k = LINK_SYSCALL; }
        }
    }
    if (p == ROW_NONE && f.tap[g] != 1) {
        uint32_t tcp = f.tcp[g];
        if (tcp) {
            uint32_t c = idx_find(ix, REL_TCP, tkey, tcp);
            if (c != ROW_NONE && c != g) { p = c; k = LINK_TCP; }
        }
    }
    parent[g] = p;
    kind[g] = k;
}

// one thread per global row; depth -1 = no root within MAX_TRACE_HOPS
__global__ void k_trace_depth(const uint64_t* __restrict__ tkey,
                              const uint32_t* __restrict__ parent,
                              uint32_t n, int32_t* __restrict__ depth) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || tkey[g] == 0) return;
    uint32_t cur = g, d = 0;
    uint32_t p = parent[cur];
    while (p != ROW_NONE && d < MAX_TRACE_HOPS) {
        cur = p;   // a parent is a participating row < n (k_trace_link)
        d++;
        p = parent[cur];
    }
    depth[g] = p == ROW_NONE ? (int32_t)d : -1;
}

// Edge key: each half is the dictionary id + 1 (wrapping, so
// DICT_ID_INVALID -> 0) and the whole is offset by one more to stay clear
// of EMPTY_KEY. Ids are slot indices below the dictionary capacity, so a
// half never reaches 0xFFFFFFFF and the offset cannot wrap.
DEV uint64_t edge_key(uint32_t psvc, uint32_t csvc) {
    return (((uint64_t)(uint32_t)(psvc + 1u) << 32) |
            (uint32_t)(csvc + 1u)) + 1ull;
}

struct EdgeTable {
    uint64_t* keys;              // [cap]
    unsigned long long* vals;    // [cap, EV_N]
    unsigned long long* drops;
    uint32_t cap_mask;
};

DEV void edge_add_global(const EdgeTable& et, uint64_t key,
                         const unsigned long long* v) {
    uint32_t slot = table_claim(et.keys, et.cap_mask, key,
                                (uint32_t)(mix64(key) & et.cap_mask));
    if (slot == ROW_NONE) { atomicAdd(et.drops, v[EV_CALLS]); return; }
    unsigned long long* acc = et.vals + (uint64_t)slot * EV_N;
    for (int i = 0; i < EV_N; i++)
        if (v[i]) atomicAdd(&acc[i], v[i]);
}

constexpr uint32_t FOLD_ROWS_PER_BLOCK = 4096;  // 16 rows per thread
constexpr uint32_t EDGE_LSLOT = 512;            // 28 KiB of LDS per block
constexpr uint32_t EDGE_LPROBE = 8;

// block-strided over FOLD_ROWS_PER_BLOCK consecutive rows. Per-trace words
// go straight to global atomics (many groups, few rows each); edges (few
// groups, every linked row) are summed in an LDS table first and flushed
// once per block. A row whose edge finds no LDS slot within EDGE_LPROBE
// steps adds to the global table directly.
__global__ void __launch_bounds__(256)
k_trace_fold(TraceFlat f, const uint32_t* __restrict__ parent,
             const uint8_t* __restrict__ kind,
             const int32_t* __restrict__ depth, uint32_t n,
             uint64_t* __restrict__ tkeys,
             unsigned long long* __restrict__ tvals, uint32_t tcap_mask,
             unsigned long long* __restrict__ tdrops, EdgeTable et) {
    __shared__ unsigned long long lkey[EDGE_LSLOT];
    __shared__ unsigned long long lval[EDGE_LSLOT * EV_N];
    for (uint32_t i = threadIdx.x; i < EDGE_LSLOT; i += blockDim.x)
        lkey[i] = EMPTY_KEY;
    for (uint32_t i = threadIdx.x; i < EDGE_LSLOT * EV_N; i += blockDim.x)
        lval[i] = 0;
    __syncthreads();
    uint64_t row0 = (uint64_t)blockIdx.x * FOLD_ROWS_PER_BLOCK;
    for (uint32_t it = 0; it < FOLD_ROWS_PER_BLOCK / BLOCK; it++) {
        uint64_t g64 = row0 + (uint64_t)it * BLOCK + threadIdx.x;
        if (g64 >= n) break;
        uint32_t g = (uint32_t)g64;
        uint64_t tkey = f.tkey[g];
        if (tkey == 0) continue;
        uint32_t p = parent[g];
        int32_t d = depth[g];
        uint8_t st = f.status[g];
        bool err = st == STATUS_SERVER_ERROR || st == STATUS_CLIENT_ERROR;
        uint64_t start = f.start[g], end = f.end[g];
        uint32_t slot = table_claim(tkeys, tcap_mask, tkey,
                                    (uint32_t)(mix64(tkey) & tcap_mask));
        if (slot == ROW_NONE) {
            atomicAdd(tdrops, 1ull);
        } else {
            unsigned long long* tv = tvals + (uint64_t)slot * TV_N;
            atomicAdd(&tv[TV_SPANS], 1ull);
            if (d < 0) atomicAdd(&tv[TV_UNROOTED], 1ull);
            else if (d > 0) atomicMax(&tv[TV_MAX_DEPTH],
                                      (unsigned long long)d);
            if (p == ROW_NONE) {
                atomicAdd(&tv[TV_ROOTS], 1ull);
                atomicMin(&tv[TV_ROOT_ROW], (unsigned long long)g);
            }
            if (err) atomicAdd(&tv[TV_ERRORS], 1ull);
            atomicMin(&tv[TV_START_MIN], (unsigned long long)start);
            atomicMax(&tv[TV_END_MAX], (unsigned long long)end);
            atomicMin(&tv[TV_FIRST_ROW], (unsigned long long)g);
        }
        if (p == ROW_NONE) continue;
        uint8_t k = kind[g];
        unsigned long long v[EV_N];
        v[EV_CALLS] = 1;
        v[EV_SPAN] = k == LINK_SPAN;
        v[EV_SYSCALL] = k == LINK_SYSCALL;
        v[EV_TCP] = k == LINK_TCP;
        v[EV_ERRORS] = err;
        v[EV_DUR_NS] = end > start ? end - start : 0;
        uint64_t ek = edge_key(f.svc[p], f.svc[g]);
        uint32_t ls = (uint32_t)(mix64(ek) & (EDGE_LSLOT - 1));
        bool placed = false;
        for (uint32_t probe = 0; probe < EDGE_LPROBE && !placed; probe++) {
            unsigned long long cur = lkey[ls];
            if (cur == EMPTY_KEY)
                cur = atomicCAS(&lkey[ls], EMPTY_KEY,
                                (unsigned long long)ek);
            if (cur == EMPTY_KEY || cur == ek) placed = true;
            else ls = (ls + 1) & (EDGE_LSLOT - 1);
        }
        if (placed) {
            for (int i = 0; i < EV_N; i++)
                if (v[i]) atomicAdd(&lval[ls * EV_N + i], v[i]);
        } else {
            edge_add_global(et, ek, v);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < EDGE_LSLOT; i += blockDim.x) {
        unsigned long long ek = lkey[i];
        if (ek != EMPTY_KEY) edge_add_global(et, ek, &lval[i * EV_N]);
    }
}

inline TraceFlat flat_of(const uint64_t* p) {
    return TraceFlat{(uint64_t*)p[0], (uint64_t*)p[1], (uint64_t*)p[2],
                     (uint64_t*)p[3], (uint64_t*)p[4], (uint32_t*)p[5],
                     (uint32_t*)p[6], (uint8_t*)p[7], (uint8_t*)p[8]};
}

}  // namespace

extern "C" {

uint32_t df_trace_max_hops() { return MAX_TRACE_HOPS; }

// seg = a host SegView (dfseg.h); flat = 9 device pointers in TraceFlat
// order
int df_trace_extract(const void* seg, uint32_t base_row,
                     uint64_t time_start, uint64_t time_end,
                     const uint64_t* flat, void* idx_keys, void* idx_rows,
                     void* drops, uint32_t idx_cap, uint64_t stream) {
    SegView s = seg_view_load(seg);
    if (s.n_rows == 0) return 0;
    FirstRowIdx ix{(uint64_t*)idx_keys, (uint32_t*)idx_rows,
                   (unsigned long long*)drops, idx_cap};
    hipLaunchKernelGGL(k_trace_extract, dim3(grid_for(s.n_rows)), dim3(BLOCK),
                       0, STREAM(stream), s, base_row, time_start, time_end,
                       flat_of(flat), ix);
    return (int)hipGetLastError();
}

int df_trace_link(const uint64_t* flat, const void* idx_keys,
                  const void* idx_rows, uint32_t idx_cap, uint32_t n,
                  void* parent, void* kind, uint64_t stream) {
    if (n == 0) return 0;
    FirstRowIdx ix{(uint64_t*)idx_keys, (uint32_t*)idx_rows, nullptr,
                   idx_cap};
    hipLaunchKernelGGL(k_trace_link, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), flat_of(flat), ix, n,
                       (uint32_t*)parent,
                       (uint8_t*)kind);
    return (int)hipGetLastError();
}

int df_trace_depth(const void* tkey, const void* parent, uint32_t n,
                   void* depth, uint64_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_trace_depth, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), (const uint64_t*)tkey,
                       (const uint32_t*)parent, n, (int32_t*)depth);
    return (int)hipGetLastError();
}

int df_trace_fold(const uint64_t* flat, const void* parent, const void* kind,
                  const void* depth, uint32_t n, void* tkeys, void* tvals,
                  uint32_t tcap, void* ekeys, void* evals, uint32_t ecap,
                  void* drops, uint64_t stream) {
    if (n == 0) return 0;
    EdgeTable et{(uint64_t*)ekeys, (unsigned long long*)evals,
                 (unsigned long long*)drops, ecap - 1};
    hipLaunchKernelGGL(k_trace_fold,
                       dim3(grid_for(n, FOLD_ROWS_PER_BLOCK)), dim3(BLOCK),
                       0, STREAM(stream), flat_of(flat),
                       (const uint32_t*)parent,
                       (const uint8_t*)kind, (const int32_t*)depth, n,
                       (uint64_t*)tkeys, (unsigned long long*)tvals,
                       tcap - 1, (unsigned long long*)drops, et);
    return (int)hipGetLastError();
}

}  // extern "C"
