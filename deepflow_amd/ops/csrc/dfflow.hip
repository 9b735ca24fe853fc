// dfflow — K12: flow groups. Partitions every span of a time window into
// the connected components of "shares a join key" (trace id, syscall trace
// id, tcp sequence pair, x-request-id), so spans that carry no trace id are
// tied to each other and to instrumented spans. A hash join followed by a
// parallel union-find. Host twin and semantics: query/flowgroups.py.
//
// Four launches per query, separated by kernel boundaries (nothing spins):
//   k_flow_extract  per segment, one thread per row: window test, join keys
//                   into flat arrays indexed by GLOBAL row (scan order),
//                   inserts of every key into ONE first-row index
//   k_flow_union    one thread per row: for each key, the index's first row
//                   is united with the row in label[] (min-root hooking)
//   k_flow_flatten  group[g] = root of g
//   k_flow_fold     per-group summary words, indexed directly by group id
// Only k_flow_extract sees segments; the rest read the flat arrays.
// k_flow_index is the insert half of k_flow_extract over flat columns that
// are already on the device (kernel tests; not on the query path).
//
// Rules: wave = 64 lanes, blocks are multiples of 64; table rules are in
// dftable.h, segment access in dfseg.h. Particular to this unit:
//  - no kernel reads in the same launch what another workgroup wrote, with
//    the one exception below.
//  - an index key is the 64-bit mix of (key space, join key); two different
//    pairs with one mix would share a slot, the same 64-bit identity K10
//    already accepts.
//
// The exception: k_flow_union reads label[] words that other workgroups
// write in the same launch. That is sound without any ordering because
//  - label[x] <= x always holds (the host writes label[x] = x, and every
//    write puts a smaller value),
//  - values only decrease,
//  - every hook is an atomicCAS(&label[r], r, lo) that succeeds only while
//    r is still a root, so a stale read costs a failed CAS and a retry,
//    never a wrong hook; a stale parent is an older ancestor, still an
//    ancestor, and a walk from it reaches the same root,
//  - a walk strictly descends and therefore terminates,
//  - a CAS failure means another thread made progress; nothing waits.
// Every access to label[] in that kernel is an atomic RMW or a relaxed
// agent-scope atomic load (served by L2/memory, not by a CU's L1, which no
// other CU's store refreshes). The later launches read it plainly.
#include "dftable.h"
#include "dfseg.h"

namespace {

// key spaces (python twin: flowgroups.REL_*); bit r of `via` = space r
enum { REL_TRACE = 0, REL_SYSCALL, REL_TCP, REL_XREQ, REL_N };
// per-group value words (python twin: flowgroups.GV_*)
enum { GV_SPANS = 0, GV_TRACED, GV_ERRORS, GV_START_MIN, GV_END_MAX,
       GV_FIRST_TRACED_ROW, GV_VIA_TRACE, GV_VIA_SYSCALL, GV_VIA_TCP,
       GV_VIA_XREQ, GV_N };
constexpr uint32_t FLOW_KEYS_PER_ROW = 6;

// query-scoped flat columns, indexed by global row. Only `part` is written
// for a row outside the window.
struct FlowFlat {
    uint8_t* part;      // 1 = row takes part
    uint64_t* tkey;     // trace key (0 = none)
    uint64_t* sreq;     // syscall_trace_id_request
    uint64_t* sresp;    // syscall_trace_id_response
    uint64_t* tcp;      // req_tcp_seq | resp_tcp_seq << 32 (0 = req is 0)
    uint64_t* x0;       // hash of x_request_id_0 (0 = empty)
    uint64_t* x1;       // hash of x_request_id_1
    uint64_t* start;
    uint64_t* end;
    uint8_t* status;    // response_status
};

// one first-row index (FirstRowIdx at base 0) for all key spaces
DEV uint64_t flow_key(uint32_t rel, uint64_t k) {
    uint64_t h = mix64(mix64(0xF10Full + rel) ^ k);
    return h ? h : 1ull;
}

DEV void idx_insert(const FirstRowIdx& ix, uint32_t rel, uint64_t k,
                    uint32_t row) {
    if (k) first_row_insert(ix, 0, flow_key(rel, k), row);
}

DEV uint32_t idx_find(const FirstRowIdx& ix, uint32_t rel, uint64_t k) {
    return first_row_find(ix, 0, flow_key(rel, k));
}

// the (up to) six keys of a row, in a fixed order: trace, syscall request,
// syscall response, tcp pair, x-request-id 0, x-request-id 1
struct RowKeys {
    uint64_t k[FLOW_KEYS_PER_ROW];
};

// key space of key i
DEV uint32_t key_rel(uint32_t i) {
    return i == 0 ? REL_TRACE : i <= 2 ? REL_SYSCALL
         : i == 3 ? REL_TCP : REL_XREQ;
}

DEV RowKeys load_keys(const FlowFlat& f, uint32_t g) {
    RowKeys r;
    r.k[0] = f.tkey[g];
    r.k[1] = f.sreq[g];
    r.k[2] = f.sresp[g];
    r.k[3] = f.tcp[g];
    r.k[4] = f.x0[g];
    r.k[5] = f.x1[g];
    return r;
}

DEV void insert_keys(const FirstRowIdx& ix, const RowKeys& r, uint32_t g) {
    for (uint32_t i = 0; i < FLOW_KEYS_PER_ROW; i++)
        idx_insert(ix, key_rel(i), r.k[i], g);
}

// one thread per segment row
__global__ void k_flow_extract(SegView s, uint32_t base_row,
                               uint64_t time_start, uint64_t time_end,
                               FlowFlat f, FirstRowIdx ix) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (uint32_t)s.n_rows) return;
    uint32_t g = base_row + r;
    uint64_t start = s.u64c[(uint64_t)L7_U64_START_TIME * s.stride + r];
    bool part = start >= time_start && start <= time_end;
    f.part[g] = part;
    if (!part) return;
    RowKeys k;
    k.k[0] = seg_trace_key(s, r);
    k.k[1] = s.u64c[(uint64_t)L7_U64_SYSCALL_REQ * s.stride + r];
    k.k[2] = s.u64c[(uint64_t)L7_U64_SYSCALL_RESP * s.stride + r];
    uint32_t req = s.u32c[(uint64_t)L7_U32_REQ_TCP_SEQ * s.stride + r];
    uint32_t resp = s.u32c[(uint64_t)L7_U32_RESP_TCP_SEQ * s.stride + r];
    k.k[3] = req ? ((uint64_t)req | ((uint64_t)resp << 32)) : 0;
    k.k[4] = seg_pool_hash(s, r, L7_POOL_X_REQUEST_ID_0);
    k.k[5] = seg_pool_hash(s, r, L7_POOL_X_REQUEST_ID_1);
    f.tkey[g] = k.k[0];
    f.sreq[g] = k.k[1];
    f.sresp[g] = k.k[2];
    f.tcp[g] = k.k[3];
    f.x0[g] = k.k[4];
    f.x1[g] = k.k[5];
    f.start[g] = start;
    f.end[g] = s.u64c[(uint64_t)L7_U64_END_TIME * s.stride + r];
    f.status[g] = s.u8c[(uint64_t)L7_U8_STATUS * s.stride + r];
    insert_keys(ix, k, g);
}

// one thread per global row: the index inserts alone, from the flat columns
__global__ void k_flow_index(FlowFlat f, FirstRowIdx ix, uint32_t n) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || !f.part[g]) return;
    insert_keys(ix, load_keys(f, g), g);
}

DEV uint32_t label_load(uint32_t* label, uint32_t x) {
    return __hip_atomic_load(&label[x], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}

// root of x, halving the path on the way: label[x] moves from its parent to
// its grandparent by CAS (a smaller ancestor, so every invariant holds; a
// lost CAS is ignored)
DEV uint32_t find_root(uint32_t* label, uint32_t x) {
    for (;;) {
        uint32_t p = label_load(label, x);
        if (p == x) return x;
        uint32_t gp = label_load(label, p);
        if (gp == p) return p;
        atomicCAS(&label[x], p, gp);
        x = gp;
    }
}

// lock-free min-root hooking: the higher root is hung below the lower one.
// Each retry starts strictly below where the last one stood, so the loop
// ends; afterwards a and b have one root for good.
DEV void unite(uint32_t* label, uint32_t a, uint32_t b) {
    for (;;) {
        a = find_root(label, a);
        b = find_root(label, b);
        if (a == b) return;
        uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        uint32_t old = atomicCAS(&label[hi], hi, lo);
        if (old == hi) return;
        a = old;    // hi was hooked meanwhile, below `old` < hi
        b = lo;
    }
}

// one thread per global row. rep < n: only rows below n were inserted.
__global__ void k_flow_union(FlowFlat f, FirstRowIdx ix, uint32_t n,
                             uint32_t* label, uint8_t* __restrict__ via) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || !f.part[g]) return;
    RowKeys r = load_keys(f, g);
    uint32_t v = 0;
    for (uint32_t i = 0; i < FLOW_KEYS_PER_ROW; i++) {
        if (r.k[i] == 0) continue;
        uint32_t rep = idx_find(ix, key_rel(i), r.k[i]);
        if (rep == ROW_NONE || rep == g || rep >= n) continue;
        v |= 1u << key_rel(i);
        unite(label, g, rep);
    }
    via[g] = (uint8_t)v;
}

// one thread per global row; label[] is complete (previous launch)
__global__ void k_flow_flatten(const uint32_t* __restrict__ label,
                               uint32_t n, uint32_t* __restrict__ group) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    uint32_t x = g, p = label[x];
    while (p != x) {    // p < x: strictly descending
        x = p;
        p = label[x];
    }
    group[g] = x;
}

// one thread per global row; gvals [n, GV_N], row = group id (< n)
__global__ void k_flow_fold(FlowFlat f, const uint32_t* __restrict__ group,
                            const uint8_t* __restrict__ via, uint32_t n,
                            unsigned long long* __restrict__ gvals) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || !f.part[g]) return;
    uint32_t grp = group[g];
    if (grp >= n) return;
    unsigned long long* gv = gvals + (uint64_t)grp * GV_N;
    uint8_t st = f.status[g];
    uint32_t v = via[g];
    atomicAdd(&gv[GV_SPANS], 1ull);
    if (f.tkey[g]) {
        atomicAdd(&gv[GV_TRACED], 1ull);
        atomicMin(&gv[GV_FIRST_TRACED_ROW], (unsigned long long)g);
    }
    if (st == STATUS_SERVER_ERROR || st == STATUS_CLIENT_ERROR)
        atomicAdd(&gv[GV_ERRORS], 1ull);
    atomicMin(&gv[GV_START_MIN], (unsigned long long)f.start[g]);
    atomicMax(&gv[GV_END_MAX], (unsigned long long)f.end[g]);
    for (uint32_t r = 0; r < REL_N; r++)
        if (v & (1u << r)) atomicAdd(&gv[GV_VIA_TRACE + r], 1ull);
}

inline FlowFlat flat_of(const uint64_t* p) {
    return FlowFlat{(uint8_t*)p[0], (uint64_t*)p[1], (uint64_t*)p[2],
                    (uint64_t*)p[3], (uint64_t*)p[4], (uint64_t*)p[5],
                    (uint64_t*)p[6], (uint64_t*)p[7], (uint64_t*)p[8],
                    (uint8_t*)p[9]};
}

}  // namespace

extern "C" {

uint32_t df_flow_gv_n() { return GV_N; }
uint32_t df_flow_rel_n() { return REL_N; }
uint32_t df_flow_keys_per_row() { return FLOW_KEYS_PER_ROW; }

// seg = a host SegView (dfseg.h); flat = 10 device pointers in FlowFlat
// order; idx_cap a power of two
int df_flow_extract(const void* seg, uint32_t base_row, uint64_t time_start,
                    uint64_t time_end, const uint64_t* flat, void* idx_keys,
                    void* idx_rows, void* drops, uint32_t idx_cap,
                    uint64_t stream) {
    SegView s = seg_view_load(seg);
    if (s.n_rows == 0) return 0;
    FirstRowIdx ix{(uint64_t*)idx_keys, (uint32_t*)idx_rows,
                   (unsigned long long*)drops, idx_cap};
    hipLaunchKernelGGL(k_flow_extract, dim3(grid_for(s.n_rows)), dim3(BLOCK),
                       0, STREAM(stream), s, base_row, time_start, time_end,
                       flat_of(flat), ix);
    return (int)hipGetLastError();
}

int df_flow_index(const uint64_t* flat, void* idx_keys, void* idx_rows,
                  void* drops, uint32_t idx_cap, uint32_t n,
                  uint64_t stream) {
    if (n == 0) return 0;
    FirstRowIdx ix{(uint64_t*)idx_keys, (uint32_t*)idx_rows,
                   (unsigned long long*)drops, idx_cap};
    hipLaunchKernelGGL(k_flow_index, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), flat_of(flat), ix, n);
    return (int)hipGetLastError();
}

// label: host-initialised to label[g] = g
int df_flow_union(const uint64_t* flat, const void* idx_keys,
                  const void* idx_rows, uint32_t idx_cap, uint32_t n,
                  void* label, void* via, uint64_t stream) {
    if (n == 0) return 0;
    FirstRowIdx ix{(uint64_t*)idx_keys, (uint32_t*)idx_rows, nullptr,
                   idx_cap};
    hipLaunchKernelGGL(k_flow_union, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), flat_of(flat), ix, n,
                       (uint32_t*)label, (uint8_t*)via);
    return (int)hipGetLastError();
}

int df_flow_flatten(const void* label, uint32_t n, void* group,
                    uint64_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_flow_flatten, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), (const uint32_t*)label, n,
                       (uint32_t*)group);
    return (int)hipGetLastError();
}

// gvals: [n, GV_N], zeroed, the two min words all-ones
int df_flow_fold(const uint64_t* flat, const void* group, const void* via,
                 uint32_t n, void* gvals, uint64_t stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_flow_fold, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), flat_of(flat),
                       (const uint32_t*)group, (const uint8_t*)via, n,
                       (unsigned long long*)gvals);
    return (int)hipGetLastError();
}

}  // extern "C"
