// dfgpu — CDNA4 (gfx950) HIP kernels for the MI355X-native ingest hot
// path. This replaces the reference's CPU-side ingester decode
// (server/ingester/flow_log/decoder/decoder.go), PlatformInfoTable hash join
// (server/libs/grpc/grpc_platformdata.go), flow_tag LRU dedup
// (server/ingester/flow_tag/flow_tag_writer.go) and time-window metric
// aggregation — redesigned as GPU kernels over HBM-resident columnar
// segments, plus the bit-pack codec of cold segments. The ClickHouse
// group-by the reference's querier pushes down
// (server/querier/engine/clickhouse) is dfquery.hip.
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//  - wave = 64 lanes; block sizes are multiples of 64.
//  - decode is thread-per-record (protobuf varint streams are sequential per
//    record); records land in L2/L3 so byte-granularity reads amortize.
//  - all cross-workgroup state (hash tables, counters) uses device-scope
//    atomics; no inter-workgroup ordering is assumed (XCD L2s not coherent).
//  - dictionary/table IDs are SLOT INDICES: a claim is one atomicCAS on the
//    64-bit key; no ID counter, no spin-waiting on a second word. The
//    rules and the one probe-or-insert are in dftable.h.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC
#include <hip/hip_runtime.h>
#include "dftable.h"
#include "l7_decode.h"
#include "l4_decode.h"

namespace {

// ----------------------------------------------------------------------
// K1 / K1b: protobuf decode, thread-per-record. The per-record parsers
// (and the malformed-record contract) are in l7_decode.h / l4_decode.h,
// which also compile for the host.
// ----------------------------------------------------------------------

__global__ void k_decode_l7(const uint8_t* __restrict__ payload,
                            const uint32_t* __restrict__ offs,
                            const uint32_t* __restrict__ lens,
                            uint32_t n, L7Cols cols) {
    uint32_t rid = blockIdx.x * blockDim.x + threadIdx.x;
    if (rid >= n) return;
    ByteStream bs;
    bs.init(payload);
    decode_l7_record(bs, offs[rid], lens[rid], rid, cols);
}

__global__ void k_decode_l4(const uint8_t* __restrict__ payload,
                            const uint32_t* __restrict__ offs,
                            const uint32_t* __restrict__ lens,
                            uint32_t n, L4Cols cols) {
    uint32_t rid = blockIdx.x * blockDim.x + threadIdx.x;
    if (rid >= n) return;
    ByteStream bs;
    bs.init(payload);
    decode_l4_record(bs, offs[rid], lens[rid], rid, cols);
}

// ----------------------------------------------------------------------
// K5: flow_metrics table family (reference libs/flow-metrics/tag.go
// 443-523: network{,_map}.{1s,1m}, application{,_map}.{1s,1m},
// traffic_policy.1m — per-table Code bitmask selects tag columns).
//
// Exact keys: each table keeps three arrays — tkeys[cap] holds the 64-bit
// mixed hash of the key tuple (the CAS claim word), traw[cap][RU_MAX_KEYS]
// holds the raw tuple words for verification/harvest, tvals[cap][nv] the
// accumulators. A reader that matches the hash verifies the raw words; if
// the claimant has not published them yet it simply probes on and claims a
// fresh slot with the same tuple (no spin — intra-wave spinning on another
// lane's store can deadlock the wave on CDNA's exec-mask divergence
// model); duplicate slots for one tuple are merged exactly at harvest.
// This removes the round-1 masked-pack collisions (vtap&0xFFF etc.).
// ----------------------------------------------------------------------

#define RU_MAX_KEYS 8
constexpr uint64_t RU_SENTINEL = 0xFFFFFFFFFFFFFFFFull;

// host-built per-table key spec (the Code-bitmask analog)
struct RuSpec {
    uint32_t interval_s;            // time bucket width (1, 60, ...)
    uint32_t n_keys;                // key sources after the time bucket
    uint8_t fam[RU_MAX_KEYS];       // 0=u64 1=u32 2=u8
    uint8_t idx[RU_MAX_KEYS];
    uint8_t require_nonzero;        // 1-based key index that must be != 0
                                    // (traffic_policy: acl_gid), 0 = off
    uint8_t use_lds;                // per-block LDS pre-aggregation: on for
                                    // low-cardinality tables where global
                                    // atomics would serialize on hot slots
};

enum { NAGG_BYTE_TX = 0, NAGG_BYTE_RX, NAGG_PKT_TX, NAGG_PKT_RX,
       NAGG_NEW_FLOW, NAGG_CLOSED_FLOW, NAGG_RTT_SUM, NAGG_RTT_CNT,
       NAGG_RTT_MAX, NAGG_RETRANS, NAGG_NVALS };

template <typename ColsT>
DEV uint64_t ru_src(const ColsT& c, uint64_t row, uint8_t fam, uint8_t idx) {
    switch (fam) {
        case 0: return c.u64c[(uint64_t)idx * c.stride + row];
        case 1: return c.u32c[(uint64_t)idx * c.stride + row];
        default: return c.u8c[(uint64_t)idx * c.stride + row];
    }
}

// claim a slot for the raw tuple kw[0..nw); returns slot or ~0u.
// Probes are bounded: once a table region is saturated the row is DROPPED
// and counted (drops tensor) instead of walking the whole table — a full
// table must degrade to a watermark drop, not an O(cap) scan per row
// (the reference throttles/evicts at capacity too).
#define RU_MAX_PROBES 128u
DEV uint64_t ru_hash(const uint64_t* kw, uint32_t nw) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint32_t w = 0; w < nw; w++) h = mix64(h ^ kw[w]);
    return h == EMPTY_KEY ? 1 : h;
}

DEV uint32_t ru_claim_h(const uint64_t* kw, uint32_t nw, uint64_t h,
                        uint64_t* tkeys, uint64_t* traw, uint32_t cap_mask) {
    uint32_t slot = (uint32_t)(h & cap_mask);
    uint32_t max_probes = cap_mask < RU_MAX_PROBES ? cap_mask : RU_MAX_PROBES;
    for (uint32_t probe = 0; probe <= max_probes; probe++) {
        uint64_t cur = tkeys[slot];
        if (cur == EMPTY_KEY) {
            uint64_t old = atomicCAS((unsigned long long*)&tkeys[slot],
                                     EMPTY_KEY, h);
            if (old == EMPTY_KEY) {
                uint64_t* r = &traw[(uint64_t)slot * RU_MAX_KEYS];
                for (uint32_t w = nw; w-- > 1;)
                    __hip_atomic_store(&r[w], kw[w], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                // word 0 published last with release: a reader that sees
                // it non-sentinel sees the full tuple
                __hip_atomic_store(&r[0], kw[0], __ATOMIC_RELEASE,
                                   __HIP_MEMORY_SCOPE_AGENT);
                return slot;
            }
            cur = old;
        }
        if (cur == h) {
            const uint64_t* r = &traw[(uint64_t)slot * RU_MAX_KEYS];
            uint64_t w0 = __hip_atomic_load(&r[0], __ATOMIC_ACQUIRE,
                                            __HIP_MEMORY_SCOPE_AGENT);
            // w0 is a bucketed relative time — never the sentinel. If the
            // claimant has not published yet, fall through and claim a
            // duplicate slot (merged at harvest) instead of spinning.
            if (w0 == kw[0]) {
                bool match = true;
                for (uint32_t w = 1; w < nw; w++)
                    match = match &&
                        __hip_atomic_load(&r[w], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT) == kw[w];
                if (match) return slot;
            }
        }
        slot = (slot + 1) & cap_mask;
    }
    return 0xFFFFFFFFu;
}

DEV uint32_t ru_claim(const uint64_t* kw, uint32_t nw,
                      uint64_t* tkeys, uint64_t* traw, uint32_t cap_mask) {
    return ru_claim_h(kw, nw, ru_hash(kw, nw), tkeys, traw, cap_mask);
}

// build the raw key tuple for one row; false = row not eligible
template <typename ColsT>
DEV bool ru_build_key(const ColsT& cols, uint64_t row, uint64_t time_base_s,
                      const RuSpec& ru, uint64_t* kw) {
    uint64_t t_s = cols.u64c[0 * cols.stride + row] / 1000000000ull;
    uint64_t rel = t_s > time_base_s ? t_s - time_base_s : 0;
    if (ru.interval_s > 1) rel = (rel / ru.interval_s) * ru.interval_s;
    kw[0] = rel;
    for (uint32_t k = 0; k < ru.n_keys; k++)
        kw[1 + k] = ru_src(cols, row, ru.fam[k], ru.idx[k]);
    return !(ru.require_nonzero && kw[ru.require_nonzero] == 0);
}

template <typename ColsT>
DEV uint32_t ru_key_claim(const ColsT& cols, uint64_t row, uint64_t time_base_s,
                          const RuSpec& ru, uint64_t* tkeys, uint64_t* traw,
                          uint32_t cap_mask, unsigned long long* drops) {
    uint64_t kw[RU_MAX_KEYS + 1];
    if (!ru_build_key(cols, row, time_base_s, ru, kw))
        return 0xFFFFFFFEu;  // row not eligible for this table
    uint32_t slot = ru_claim(kw, ru.n_keys + 1, tkeys, traw, cap_mask);
    if (slot == 0xFFFFFFFFu) atomicAdd(drops, 1ull);
    return slot;
}

// multi-table spec: one launch updates every table of a family
// (one pass over the row columns instead of one launch per table —
// k_rollup_l7 was 63% of device time as 4 launches, r2 profile)
#define RU_MAX_TABLES 6
struct RuMulti {
    RuSpec ru[RU_MAX_TABLES];
    uint32_t n_tables;
};
struct RuTablePtrs {
    uint64_t* tkeys[RU_MAX_TABLES];
    uint64_t* traw[RU_MAX_TABLES];
    unsigned long long* tvals[RU_MAX_TABLES];
    uint32_t cap_mask[RU_MAX_TABLES];
    unsigned long long* drops[RU_MAX_TABLES];
};

// ----------------------------------------------------------------------
// LDS pre-aggregation pass: realistic streams concentrate millions of
// rows into a handful of 1s/1m rollup groups, so straight global atomics
// serialize on hot slots (measured: 63% of device time). Each workgroup
// aggregates its stripe into a 256-slot LDS table (claimant stores the
// row id so the flush can rebuild the raw tuple), then flushes once —
// global traffic drops from per-row to per-(block x live-slot). Fn maps
// (acc, row) -> atomic accumulate and works on both LDS and global
// pointers (generic address space).
// ----------------------------------------------------------------------
#define RU_NSLOT 256
#define RU_LDS_PROBES 8

template <typename ColsT, int NV, typename Fn, typename Merge>
DEV void ru_pass(const ColsT& cols, uint32_t n, uint64_t time_base_s,
                 const RuSpec& ru, uint64_t* tkeys, uint64_t* traw,
                 unsigned long long* tvals, uint32_t cap_mask,
                 unsigned long long* drops, Fn&& accum, Merge&& merge,
                 uint64_t* lkey, int* lrow, unsigned long long* lagg) {
    const uint32_t stride_g = gridDim.x * blockDim.x;
    if (ru.use_lds) {
        for (uint32_t s = threadIdx.x; s < RU_NSLOT; s += blockDim.x) {
            lkey[s] = 0;
            lrow[s] = -1;
            for (int v = 0; v < NV; v++) lagg[s * NV + v] = 0;
        }
        __syncthreads();
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride_g) {
        uint64_t row = cols.base_row + i;
        uint64_t kw[RU_MAX_KEYS + 1];
        if (!ru_build_key(cols, row, time_base_s, ru, kw)) continue;
        uint64_t h = ru_hash(kw, ru.n_keys + 1);
        bool done = false;
        if (ru.use_lds) {
            uint32_t s = (uint32_t)(h & (RU_NSLOT - 1));
            for (uint32_t probe = 0; probe < RU_LDS_PROBES; probe++) {
                uint64_t cur = lkey[s];
                if (cur == 0) {
                    uint64_t old = atomicCAS((unsigned long long*)&lkey[s],
                                             0ull, h);
                    if (old == 0) lrow[s] = (int)i;
                    cur = old == 0 ? h : old;
                }
                if (cur == h) {
                    accum(&lagg[(uint64_t)s * NV], row);
                    done = true;
                    break;
                }
                s = (s + 1) & (RU_NSLOT - 1);
            }
        }
        if (!done) {
            uint32_t slot = ru_claim_h(kw, ru.n_keys + 1, h, tkeys, traw,
                                       cap_mask);
            if (slot == 0xFFFFFFFFu) {
                atomicAdd(drops, 1ull);
                continue;
            }
            accum(&tvals[(uint64_t)slot * NV], row);
        }
    }
    if (ru.use_lds) {
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < RU_NSLOT; s += blockDim.x) {
            if (lkey[s] == 0) continue;
            uint64_t row = cols.base_row + (uint32_t)lrow[s];
            uint64_t kw[RU_MAX_KEYS + 1];
            ru_build_key(cols, row, time_base_s, ru, kw);
            uint32_t slot = ru_claim_h(kw, ru.n_keys + 1, lkey[s], tkeys,
                                       traw, cap_mask);
            if (slot == 0xFFFFFFFFu) {
                atomicAdd(drops, 1ull);
                continue;
            }
            merge(&tvals[(uint64_t)slot * NV], &lagg[(uint64_t)s * NV]);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
k_rollup_l4(const L4Cols cols, uint32_t n, uint64_t time_base_s,
            RuMulti mu, RuTablePtrs tp) {
    __shared__ uint64_t lkey[RU_NSLOT];
    __shared__ int lrow[RU_NSLOT];
    __shared__ unsigned long long lagg[RU_NSLOT * NAGG_NVALS];
    auto accum = [&](unsigned long long* acc, uint64_t row) {
        atomicAdd(&acc[NAGG_BYTE_TX],
                  cols.u64c[L4_U64_BYTE_TX * cols.stride + row]);
        atomicAdd(&acc[NAGG_BYTE_RX],
                  cols.u64c[L4_U64_BYTE_RX * cols.stride + row]);
        atomicAdd(&acc[NAGG_PKT_TX],
                  cols.u64c[L4_U64_PACKET_TX * cols.stride + row]);
        atomicAdd(&acc[NAGG_PKT_RX],
                  cols.u64c[L4_U64_PACKET_RX * cols.stride + row]);
        if (cols.u8c[L4_U8_IS_NEW_FLOW * cols.stride + row])
            atomicAdd(&acc[NAGG_NEW_FLOW], 1ull);
        if (cols.u8c[L4_U8_CLOSE_TYPE * cols.stride + row])
            atomicAdd(&acc[NAGG_CLOSED_FLOW], 1ull);
        uint32_t rtt = cols.u32c[L4_U32_RTT * cols.stride + row];
        if (rtt) {
            atomicAdd(&acc[NAGG_RTT_SUM], (unsigned long long)rtt);
            atomicAdd(&acc[NAGG_RTT_CNT], 1ull);
            atomicMax(&acc[NAGG_RTT_MAX], (unsigned long long)rtt);
        }
        uint64_t retrans = cols.u32c[L4_U32_RETRANS_TX * cols.stride + row] +
                           cols.u32c[L4_U32_RETRANS_RX * cols.stride + row];
        if (retrans) atomicAdd(&acc[NAGG_RETRANS], retrans);
    };
    auto merge = [&](unsigned long long* acc, unsigned long long* part) {
        for (int v = 0; v < NAGG_NVALS; v++) {
            if (part[v] == 0) continue;
            if (v == NAGG_RTT_MAX) atomicMax(&acc[v], part[v]);
            else atomicAdd(&acc[v], part[v]);
        }
    };
    for (uint32_t t = 0; t < mu.n_tables; t++)
        ru_pass<L4Cols, NAGG_NVALS>(cols, n, time_base_s, mu.ru[t],
                                    tp.tkeys[t], tp.traw[t], tp.tvals[t],
                                    tp.cap_mask[t], tp.drops[t], accum,
                                    merge, lkey, lrow, lagg);
}

// generic raw-tuple batch insert (agent Document ingest; ops: 0=sum 1=max)
__global__ void k_rollup_insert(const uint64_t* __restrict__ kws,  // [n, nw]
                                const unsigned long long* __restrict__ vals,  // [n, nv]
                                const uint8_t* __restrict__ ops,   // [nv]
                                uint32_t n, uint32_t nw, uint32_t nv,
                                uint64_t* __restrict__ tkeys,
                                uint64_t* __restrict__ traw,
                                unsigned long long* __restrict__ tvals,
                                uint32_t cap_mask,
                                unsigned long long* __restrict__ drops) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t kw[RU_MAX_KEYS + 1];
    for (uint32_t w = 0; w < nw; w++) kw[w] = kws[(uint64_t)i * nw + w];
    uint32_t slot = ru_claim(kw, nw, tkeys, traw, cap_mask);
    if (slot == 0xFFFFFFFFu) { atomicAdd(drops, 1ull); return; }
    unsigned long long* acc = &tvals[(uint64_t)slot * nv];
    for (uint32_t v = 0; v < nv; v++) {
        unsigned long long x = vals[(uint64_t)i * nv + v];
        if (!x) continue;
        if (ops[v] == 0) atomicAdd(&acc[v], x);
        else atomicMax(&acc[v], x);
    }
}

// Interval flush without a host round trip: one grid-stride pass packs
// every occupied slot of a table into dense staging rows (out_keys [cap,
// nw], out_vals [cap, nv]; order undefined, readers sort and merge) and
// puts every slot back into its freshly constructed state: tkeys 0, tvals
// 0, all RU_MAX_KEYS words of traw the sentinel, so ru_claim_h never sees
// a stale word 0 behind a reused hash. hdr[0] counts the rows written
// (one atomicAdd per wave: ballot + prefix popcount), hdr[1] takes the
// drops counter; hdr is zero on entry. Stream order is the only
// synchronisation: no rollup kernel runs alongside.
__global__ void __launch_bounds__(256)
k_rollup_drain(uint64_t* __restrict__ tkeys, uint64_t* __restrict__ traw,
               unsigned long long* __restrict__ tvals,
               unsigned long long* __restrict__ drops,
               uint32_t cap, uint32_t nw, uint32_t nv,
               uint64_t* __restrict__ out_keys,
               unsigned long long* __restrict__ out_vals,
               unsigned long long* __restrict__ hdr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride_g = (uint64_t)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hdr[1] = *drops;
        *drops = 0;
    }
    // base is the slot of the wave's lane 0, so the loop bound is
    // wave-uniform and all 64 lanes reach the ballot together
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x +
                         (threadIdx.x - lane);
         base < cap; base += stride_g) {
        const uint64_t slot = base + lane;
        const bool in = slot < cap;
        const bool live = in && tkeys[slot] != EMPTY_KEY;
        const unsigned long long m = __ballot(live);
        unsigned long long first = 0;
        if (lane == 0 && m)
            first = atomicAdd(&hdr[0], (unsigned long long)__popcll(m));
        first = __shfl(first, 0);
        uint64_t* r = &traw[slot * RU_MAX_KEYS];
        unsigned long long* a = &tvals[slot * nv];
        if (live) {
            const uint64_t o = first + __popcll(m & ((1ull << lane) - 1ull));
            for (uint32_t w = 0; w < nw; w++) out_keys[o * nw + w] = r[w];
            for (uint32_t v = 0; v < nv; v++) out_vals[o * nv + v] = a[v];
        }
        if (in) {
            tkeys[slot] = EMPTY_KEY;
            for (uint32_t w = 0; w < RU_MAX_KEYS; w++) r[w] = RU_SENTINEL;
            for (uint32_t v = 0; v < nv; v++) a[v] = 0;
        }
    }
}

// ----------------------------------------------------------------------
// Data-plane shard routing: gather selected records into a packed
// per-destination buffer for the RCCL all-to-all (one wave per record,
// lanes copy bytes strided — records are 100-500 B, so a wave64 gets
// coalesced 64 B segments).
// ----------------------------------------------------------------------
__global__ void k_gather_records(const uint8_t* __restrict__ src,
                                 const uint32_t* __restrict__ offs,
                                 const uint32_t* __restrict__ lens,
                                 const uint32_t* __restrict__ sel,
                                 const uint64_t* __restrict__ dst_off,
                                 uint32_t m, uint8_t* __restrict__ out) {
    uint32_t waves = blockDim.x / 64;
    uint32_t rec = blockIdx.x * waves + (threadIdx.x / 64);
    uint32_t lane = threadIdx.x % 64;
    if (rec >= m) return;
    uint32_t r = sel[rec];
    const uint8_t* s = src + offs[r];
    uint8_t* d = out + dst_off[rec];
    uint32_t n = lens[r];
    for (uint32_t b = lane; b < n; b += 64) d[b] = s[b];
}

// ----------------------------------------------------------------------
// K2: KnowledgeGraph (epc,ip) -> resource-id join.
//     Open-addressing table: keys u64 ((epc<<32)|ip), vals KG_VALS_N x u32.
// ----------------------------------------------------------------------

__global__ void k_kg_build(const uint64_t* __restrict__ keys,
                           const uint32_t* __restrict__ vals,  // [n, KG_VALS_N]
                           uint32_t n,
                           uint64_t* __restrict__ tkeys,
                           uint32_t* __restrict__ tvals,       // [cap, KG_VALS_N]
                           uint32_t cap_mask) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t k = keys[i];
    if (k == EMPTY_KEY) return;
    uint32_t slot = table_claim(tkeys, cap_mask, k,
                                (uint32_t)(mix64(k) & cap_mask));
    if (slot == ROW_NONE) return;
    // last-writer-wins value update (platform data refresh semantics)
    for (int j = 0; j < KG_VALS_N; j++)
        tvals[(uint64_t)slot * KG_VALS_N + j] = vals[(uint64_t)i * KG_VALS_N + j];
}

__global__ void k_kg_probe(const uint32_t* __restrict__ epc0,
                           const uint32_t* __restrict__ ip0,
                           const uint32_t* __restrict__ epc1,
                           const uint32_t* __restrict__ ip1,
                           uint32_t n,
                           const uint64_t* __restrict__ tkeys,
                           const uint32_t* __restrict__ tvals,
                           uint32_t cap_mask,
                           uint32_t* __restrict__ out,  // [2*KG_VALS_N, stride]
                           uint64_t stride, uint64_t base_row) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t row = base_row + i;
    for (int side = 0; side < 2; side++) {
        uint64_t k = side == 0
            ? (((uint64_t)epc0[i] << 32) | ip0[i])
            : (((uint64_t)epc1[i] << 32) | ip1[i]);
        uint32_t slot = table_find(tkeys, cap_mask, k,
                                   (uint32_t)(mix64(k) & cap_mask));
        for (int j = 0; j < KG_VALS_N; j++)
            out[((uint64_t)(side * KG_VALS_N + j)) * stride + row] =
                slot != ROW_NONE ? tvals[(uint64_t)slot * KG_VALS_N + j] : 0u;
    }
}

// ----------------------------------------------------------------------
// K3: string interning (SmartEncoding dictionary). One shared table for all
// domains; key = hash(domain, bytes); DICT ID == slot index (stable within a
// shard). New entries are emitted as (slot, packed batch ref) for the host to
// harvest into the id->string dictionary + flow_tag write path.
// ----------------------------------------------------------------------

// probe-or-insert from `h & mask` (dictionary ids are slot indices).
// Newly claimed slots are emitted for host harvest.
DEV uint32_t intern_probe(uint64_t h, uint64_t ref, uint8_t domain,
                          uint64_t* tkeys, uint32_t cap_mask,
                          uint64_t* emit, uint32_t* emit_ctr,
                          uint32_t emit_cap) {
    bool claimed;
    uint32_t slot = table_claim(tkeys, cap_mask, h, (uint32_t)(h & cap_mask),
                                &claimed);
    if (claimed) {
        uint32_t e = atomicAdd(emit_ctr, 1u);
        if (e < emit_cap) {
            emit[(uint64_t)e * 2] = ((uint64_t)domain << 56) | slot;
            emit[(uint64_t)e * 2 + 1] = ref;
        }
    }
    return slot;
}

// wave-cooperative variant: when every active lane holds the same hash
// (common for low-cardinality columns: req_type, version, attr names),
// lane 0 probes once and broadcasts.
DEV uint32_t intern_probe_wave(uint64_t h, uint64_t ref, uint8_t domain,
                               bool active,
                               uint64_t* tkeys, uint32_t cap_mask,
                               uint64_t* emit, uint32_t* emit_ctr,
                               uint32_t emit_cap) {
    uint64_t h0 = __shfl(h, 0);
    bool uniform = __all(!active || h == h0);
    if (uniform) {
        uint32_t slot = DICT_ID_INVALID;
        // some lane that is active must probe; lowest active lane does
        uint64_t act_mask = __ballot(active);
        if (act_mask == 0) return DICT_ID_INVALID;
        uint32_t leader = (uint32_t)__ffsll((unsigned long long)act_mask) - 1;
        if ((threadIdx.x & 63) == leader)
            slot = intern_probe(h, ref, domain, tkeys, cap_mask, emit,
                                emit_ctr, emit_cap);
        slot = __shfl((int)slot, leader);
        return slot;
    }
    if (!active) return DICT_ID_INVALID;
    return intern_probe(h, ref, domain, tkeys, cap_mask, emit, emit_ctr,
                        emit_cap);
}

__global__ void k_intern_many(const uint8_t* __restrict__ payload,
                              const uint64_t* __restrict__ refs,  // [*, stride]
                              const uint16_t* __restrict__ ref_rows,  // [C] row in refs per column
                              const uint8_t* __restrict__ domains,  // [C]
                              uint32_t C, uint32_t n,
                              uint64_t ref_stride, uint64_t ref_base_row,
                              uint64_t* __restrict__ tkeys, uint32_t cap_mask,
                              uint64_t* __restrict__ emit,
                              uint32_t* __restrict__ emit_ctr, uint32_t emit_cap,
                              uint32_t* __restrict__ out_ids,  // [C, out_stride]
                              uint64_t out_stride, uint64_t out_base_row) {
    uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t total = (uint64_t)C * n;
    if (gid >= total) return;
    uint32_t c = (uint32_t)(gid / n);
    uint32_t i = (uint32_t)(gid % n);
    uint64_t ref = refs[(uint64_t)ref_rows[c] * ref_stride + ref_base_row + i];
    uint32_t len = STR_REF_LEN(ref);
    uint64_t off = STR_REF_OFF(ref);
    bool active = len != 0;
    uint64_t h = 0;
    uint8_t dom = domains[c];
    if (active)
        h = str_hash(payload + off, len, 0x9E3779B97F4A7C15ull * (dom + 1));
    uint32_t slot = intern_probe_wave(h, ref, dom, active, tkeys, cap_mask,
                                      emit, emit_ctr, emit_cap);
    // out block is pre-initialized to DICT_ID_INVALID; only write hits
    if (active)
        out_ids[c * out_stride + out_base_row + i] = slot;
    else
        out_ids[c * out_stride + out_base_row + i] = DICT_ID_INVALID;
}

// attr interning: one thread per row, looping over the row's attr_cnt
// (name, value) pairs — avoids launching MAX_ATTRS*2 threads per row when
// the typical count is ~4. Names are wave-uniform per iteration.
__global__ void k_intern_attrs(const uint8_t* __restrict__ payload,
                               const uint64_t* __restrict__ attr_refs,  // SCRATCH [2*MAX, ref_stride]
                               const uint8_t* __restrict__ attr_cnt,
                               uint32_t n, uint64_t stride, uint64_t base_row,
                               uint64_t ref_stride,
                               uint64_t* __restrict__ tkeys, uint32_t cap_mask,
                               uint64_t* __restrict__ emit,
                               uint32_t* __restrict__ emit_ctr, uint32_t emit_cap,
                               const uint32_t* __restrict__ attr_start,  // [n] row block offsets (global)
                               int32_t* __restrict__ attr_pool) {  // segment attr-id pool
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool in_range = i < n;
    uint64_t row = base_row + (in_range ? i : 0);
    uint32_t cnt = in_range ? attr_cnt[row] : 0;
    uint32_t pbase = in_range ? attr_start[i] : 0;
    // wave-max so all lanes iterate together for the uniform-name fast path
    uint32_t maxc = cnt;
    for (int d = 32; d > 0; d >>= 1)
        maxc = max(maxc, (uint32_t)__shfl_xor((int)maxc, d));
    for (uint32_t a = 0; a < maxc; a++) {
        bool act = in_range && a < cnt;
        // names (wave-uniform in the common schema-stable case)
        uint64_t nref = act ? attr_refs[(uint64_t)a * ref_stride + i] : 0;
        uint32_t nlen = STR_REF_LEN(nref);
        uint64_t h = 0;
        if (act && nlen)
            h = str_hash(payload + STR_REF_OFF(nref), nlen,
                         0x9E3779B97F4A7C15ull * (DICT_DOM_ATTR_NAME + 1));
        uint32_t slot = intern_probe_wave(h, nref, DICT_DOM_ATTR_NAME,
                                          act && nlen, tkeys, cap_mask,
                                          emit, emit_ctr, emit_cap);
        if (act)
            attr_pool[pbase + a] = nlen ? (int32_t)slot : -1;
        // values (high cardinality -> per-lane probes)
        uint64_t vref = act
            ? attr_refs[(uint64_t)(L7_MAX_ATTRS + a) * ref_stride + i] : 0;
        uint32_t vlen = STR_REF_LEN(vref);
        if (act) {
            uint32_t vslot = DICT_ID_INVALID;
            if (vlen) {
                uint64_t vh = str_hash(payload + STR_REF_OFF(vref), vlen,
                    0x9E3779B97F4A7C15ull * (DICT_DOM_ATTR_VALUE + 1));
                vslot = intern_probe(vh, vref, DICT_DOM_ATTR_VALUE, tkeys,
                                     cap_mask, emit, emit_ctr, emit_cap);
            }
            attr_pool[pbase + cnt + a] = (int32_t)vslot;
        }
    }
}

// ----------------------------------------------------------------------
// K4: string pool gather. Pass 1 computes per-row pooled byte count; host
// runs an exclusive cumsum (torch); pass 2 copies bytes into the segment
// pool and rewrites refs to pool-relative offsets.
// ----------------------------------------------------------------------

__global__ void k_pool_lens(const uint64_t* __restrict__ strc,  // [L7_STR_N, stride]
                            const uint8_t* __restrict__ pool_cols,  // [npc]
                            uint32_t npc, uint32_t n,
                            uint64_t stride, uint64_t base_row,
                            uint32_t* __restrict__ row_len) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t total = 0;
    for (uint32_t c = 0; c < npc; c++)
        total += STR_REF_LEN(strc[(uint64_t)pool_cols[c] * stride + base_row + i]);
    row_len[i] = total;
}

__global__ void k_pool_gather(const uint8_t* __restrict__ payload,
                              const uint64_t* __restrict__ strc,  // scratch
                              const uint8_t* __restrict__ pool_cols,
                              uint32_t npc, uint32_t n,
                              uint64_t stride, uint64_t base_row,
                              const uint64_t* __restrict__ row_start,  // exclusive cumsum
                              uint8_t* __restrict__ pool, uint64_t pool_base,
                              uint64_t* __restrict__ out_rowref,  // [out_stride] segment
                              int16_t* __restrict__ out_lens,     // [npc, out_stride]
                              uint64_t out_stride, uint64_t out_base_row) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t dst0 = pool_base + row_start[i];
    uint64_t dst = dst0;
    for (uint32_t c = 0; c < npc; c++) {
        uint64_t r = strc[(uint64_t)pool_cols[c] * stride + base_row + i];
        uint32_t len = STR_REF_LEN(r);
        uint64_t src = STR_REF_OFF(r);
        for (uint32_t b = 0; b < len; b++) pool[dst + b] = payload[src + b];
        out_lens[(uint64_t)c * out_stride + out_base_row + i] = (int16_t)len;
        dst += len;
    }
    out_rowref[out_base_row + i] = STR_REF_PACK(dst0, dst - dst0);
}

// ----------------------------------------------------------------------
// K5 (application side): flow_metrics application{,_map} rollups from L7
// rows (reference: flow_metrics unmarshaller -> application tables).
// Exact keys via ru_key_claim (see the table-family section above).
// ----------------------------------------------------------------------

enum { AGG_REQ = 0, AGG_RESP, AGG_ERR_C, AGG_ERR_S, AGG_RRT_SUM, AGG_RRT_CNT, AGG_RRT_MAX, AGG_NVALS };

__global__ void __launch_bounds__(256)
k_rollup_l7(const L7Cols cols, uint32_t n, uint64_t time_base_s,
            RuMulti mu, RuTablePtrs tp) {
    __shared__ uint64_t lkey[RU_NSLOT];
    __shared__ int lrow[RU_NSLOT];
    __shared__ unsigned long long lagg[RU_NSLOT * AGG_NVALS];
    auto accum = [&](unsigned long long* acc, uint64_t row) {
        uint8_t status = cols.u8c[L7_U8_STATUS * cols.stride + row];
        uint8_t mtype = cols.u8c[L7_U8_MSG_TYPE * cols.stride + row];
        uint64_t rrt = cols.u64c[L7_U64_RRT * cols.stride + row];
        // msg_type: 0=request,1=response,2=session(both)
        if (mtype == 0 || mtype == 2) atomicAdd(&acc[AGG_REQ], 1ull);
        if (mtype == 1 || mtype == 2) atomicAdd(&acc[AGG_RESP], 1ull);
        if (status == 4) atomicAdd(&acc[AGG_ERR_C], 1ull);
        if (status == 3) atomicAdd(&acc[AGG_ERR_S], 1ull);
        if (rrt) {
            atomicAdd(&acc[AGG_RRT_SUM], (unsigned long long)rrt);
            atomicAdd(&acc[AGG_RRT_CNT], 1ull);
            atomicMax(&acc[AGG_RRT_MAX], (unsigned long long)rrt);
        }
    };
    auto merge = [&](unsigned long long* acc, unsigned long long* part) {
        for (int v = 0; v < AGG_NVALS; v++) {
            if (part[v] == 0) continue;
            if (v == AGG_RRT_MAX) atomicMax(&acc[v], part[v]);
            else atomicAdd(&acc[v], part[v]);
        }
    };
    for (uint32_t t = 0; t < mu.n_tables; t++)
        ru_pass<L7Cols, AGG_NVALS>(cols, n, time_base_s, mu.ru[t],
                                   tp.tkeys[t], tp.traw[t], tp.tvals[t],
                                   tp.cap_mask[t], tp.drops[t], accum,
                                   merge, lkey, lrow, lagg);
}

// ----------------------------------------------------------------------
// cold-segment bit packing: fixed-width pack of (value - base) streams.
// Word-centric pack (each thread owns one output u32 — no atomics, fully
// coalesced writes); value-centric unpack. A constant column packs to
// bits==0 (no payload at all). Extends the HBM hot window several-fold
// for demoted segments (reference analog: ClickHouse column codecs
// T64/DoubleDelta on cold parts).
// ----------------------------------------------------------------------
__global__ void k_pack_bits(const uint32_t* __restrict__ src, uint32_t n,
                            uint32_t base, uint32_t bits,
                            uint32_t* __restrict__ out,
                            uint32_t out_words) {
    uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= out_words) return;
    uint64_t bit0 = (uint64_t)w * 32u;
    uint32_t i = (uint32_t)(bit0 / bits);
    uint32_t acc = 0;
    for (; i < n; i++) {
        uint64_t vb = (uint64_t)i * bits;
        if (vb >= bit0 + 32u) break;
        if (vb + bits <= bit0) continue;  // first value may start earlier
        uint64_t v = (uint64_t)(src[i] - base);
        int64_t sh = (int64_t)vb - (int64_t)bit0;
        if (sh >= 0)
            acc |= (uint32_t)(v << sh);
        else
            acc |= (uint32_t)(v >> (uint32_t)(-sh));
    }
    out[w] = acc;
}

__global__ void k_unpack_bits(const uint32_t* __restrict__ packed,
                              uint32_t n, uint32_t base, uint32_t bits,
                              uint32_t* __restrict__ out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t vb = (uint64_t)i * bits;
    uint32_t w = (uint32_t)(vb >> 5), off = (uint32_t)(vb & 31u);
    uint64_t lo = packed[w];
    uint64_t hi = (off + bits > 32u) ? packed[w + 1] : 0ull;
    uint64_t v = ((hi << 32) | lo) >> off;
    uint32_t mask = bits >= 32u ? 0xFFFFFFFFu : ((1u << bits) - 1u);
    out[i] = base + (uint32_t)(v & mask);
}

}  // namespace

// ----------------------------------------------------------------------
// C API (ctypes). All functions take the HIP stream as uint64 and return
// hipError_t as int; launches are async on that stream.
// ----------------------------------------------------------------------

extern "C" {

int df_gpu_ready() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess && n > 0; }

int df_decode_l7(const void* payload, const void* offs, const void* lens,
                 uint32_t n,
                 void* u64c, void* u32c, void* u8c, void* strc,
                 void* attrc, void* attr_cnt,
                 uint64_t stride, uint64_t base_row, uint64_t scratch_stride,
                 uint64_t stream) {
    L7Cols cols{(uint64_t*)u64c, (uint32_t*)u32c, (uint8_t*)u8c, (uint64_t*)strc,
                (uint64_t*)attrc, (uint8_t*)attr_cnt, stride, base_row,
                scratch_stride};
    hipLaunchKernelGGL(k_decode_l7, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint8_t*)payload, (const uint32_t*)offs,
                       (const uint32_t*)lens, n, cols);
    return (int)hipGetLastError();
}

int df_decode_l4(const void* payload, const void* offs, const void* lens,
                 uint32_t n, void* u64c, void* u32c, void* u8c, void* strc,
                 uint64_t stride, uint64_t base_row, uint64_t scratch_stride,
                 uint64_t stream) {
    L4Cols cols{(uint64_t*)u64c, (uint32_t*)u32c, (uint8_t*)u8c,
                (uint64_t*)strc, stride, base_row, scratch_stride};
    hipLaunchKernelGGL(k_decode_l4, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint8_t*)payload, (const uint32_t*)offs,
                       (const uint32_t*)lens, n, cols);
    return (int)hipGetLastError();
}

// specs: n_tables x RuSpec bytes; ptrs: per-table
// [tkeys, traw, tvals, drops] device pointers + caps
static void ru_multi_fill(const void* specs, uint32_t n_tables,
                          const uint64_t* ptrs, const uint32_t* caps,
                          RuMulti& mu, RuTablePtrs& tp) {
    mu.n_tables = n_tables;
    for (uint32_t t = 0; t < n_tables; t++) {
        __builtin_memcpy(&mu.ru[t], (const uint8_t*)specs + t * sizeof(RuSpec),
                         sizeof(RuSpec));
        tp.tkeys[t] = (uint64_t*)ptrs[t * 4 + 0];
        tp.traw[t] = (uint64_t*)ptrs[t * 4 + 1];
        tp.tvals[t] = (unsigned long long*)ptrs[t * 4 + 2];
        tp.drops[t] = (unsigned long long*)ptrs[t * 4 + 3];
        tp.cap_mask[t] = caps[t] - 1;
    }
}

int df_rollup_l4(void* u64c, void* u32c, void* u8c, uint64_t stride,
                 uint64_t base_row, uint32_t n, uint64_t time_base_s,
                 const void* specs, uint32_t n_tables, const void* ptrs,
                 const void* caps, uint64_t stream) {
    L4Cols cols{(uint64_t*)u64c, (uint32_t*)u32c, (uint8_t*)u8c,
                nullptr, stride, base_row};
    RuMulti mu;
    RuTablePtrs tp;
    ru_multi_fill(specs, n_tables, (const uint64_t*)ptrs,
                  (const uint32_t*)caps, mu, tp);
    uint32_t blocks = grid_for(n);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_rollup_l4, dim3(blocks), dim3(BLOCK), 0, STREAM(stream),
                       cols, n, time_base_s, mu, tp);
    return (int)hipGetLastError();
}

int df_rollup_insert(const void* kws, const void* vals, const void* ops,
                     uint32_t n, uint32_t nw, uint32_t nv,
                     void* tkeys, void* traw, void* tvals, uint32_t cap,
                     void* drops, uint64_t stream) {
    hipLaunchKernelGGL(k_rollup_insert, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream),
                       (const uint64_t*)kws, (const unsigned long long*)vals,
                       (const uint8_t*)ops, n, nw, nv, (uint64_t*)tkeys,
                       (uint64_t*)traw, (unsigned long long*)tvals, cap - 1,
                       (unsigned long long*)drops);
    return (int)hipGetLastError();
}

// hdr: u64[2], zero on entry; out_keys [cap, nw], out_vals [cap, nv]
int df_rollup_drain(void* tkeys, void* traw, void* tvals, void* drops,
                    uint32_t cap, uint32_t nw, uint32_t nv,
                    void* out_keys, void* out_vals, void* hdr,
                    uint64_t stream) {
    if (cap == 0 || (cap & (cap - 1)) != 0 || nw == 0 || nw > RU_MAX_KEYS)
        return (int)hipErrorInvalidValue;
    // a few waves per SIMD on every CU; the pass is a plain stream over
    // the table, so more blocks than that only add launch overhead
    uint32_t blocks = grid_for(cap);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_rollup_drain, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), (uint64_t*)tkeys, (uint64_t*)traw,
                       (unsigned long long*)tvals,
                       (unsigned long long*)drops, cap, nw, nv,
                       (uint64_t*)out_keys, (unsigned long long*)out_vals,
                       (unsigned long long*)hdr);
    return (int)hipGetLastError();
}

int df_gather_records(const void* src, const void* offs, const void* lens,
                      const void* sel, const void* dst_off, uint32_t m,
                      void* out, uint64_t stream) {
    uint32_t waves = BLOCK / 64;
    uint32_t blocks = (m + waves - 1) / waves;
    hipLaunchKernelGGL(k_gather_records, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), (const uint8_t*)src,
                       (const uint32_t*)offs, (const uint32_t*)lens,
                       (const uint32_t*)sel, (const uint64_t*)dst_off, m,
                       (uint8_t*)out);
    return (int)hipGetLastError();
}

int df_kg_build(const void* keys, const void* vals, uint32_t n,
                void* tkeys, void* tvals, uint32_t cap, uint64_t stream) {
    hipLaunchKernelGGL(k_kg_build, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint64_t*)keys, (const uint32_t*)vals, n,
                       (uint64_t*)tkeys, (uint32_t*)tvals, cap - 1);
    return (int)hipGetLastError();
}

int df_kg_probe(const void* epc0, const void* ip0, const void* epc1, const void* ip1,
                uint32_t n, const void* tkeys, const void* tvals, uint32_t cap,
                void* out, uint64_t stride, uint64_t base_row, uint64_t stream) {
    hipLaunchKernelGGL(k_kg_probe, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint32_t*)epc0, (const uint32_t*)ip0,
                       (const uint32_t*)epc1, (const uint32_t*)ip1, n,
                       (const uint64_t*)tkeys, (const uint32_t*)tvals, cap - 1,
                       (uint32_t*)out, stride, base_row);
    return (int)hipGetLastError();
}

int df_intern_many(const void* payload, const void* refs, const void* ref_rows,
                   const void* domains,
                   uint32_t C, uint32_t n, uint64_t ref_stride, uint64_t ref_base_row,
                   void* tkeys, uint32_t cap,
                   void* emit, void* emit_ctr, uint32_t emit_cap,
                   void* out_ids, uint64_t out_stride, uint64_t out_base_row,
                   uint64_t stream) {
    uint64_t total = (uint64_t)C * n;
    hipLaunchKernelGGL(k_intern_many, dim3(grid_for(total)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint8_t*)payload, (const uint64_t*)refs,
                       (const uint16_t*)ref_rows,
                       (const uint8_t*)domains, C, n, ref_stride, ref_base_row,
                       (uint64_t*)tkeys, cap - 1,
                       (uint64_t*)emit, (uint32_t*)emit_ctr, emit_cap,
                       (uint32_t*)out_ids, out_stride, out_base_row);
    return (int)hipGetLastError();
}

int df_intern_attrs(const void* payload, const void* attr_refs,
                    const void* attr_cnt, uint32_t n, uint64_t stride,
                    uint64_t base_row, uint64_t ref_stride,
                    void* tkeys, uint32_t cap,
                    void* emit, void* emit_ctr, uint32_t emit_cap,
                    const void* attr_start, void* attr_pool,
                    uint64_t stream) {
    hipLaunchKernelGGL(k_intern_attrs, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream),
                       (const uint8_t*)payload, (const uint64_t*)attr_refs,
                       (const uint8_t*)attr_cnt, n, stride, base_row,
                       ref_stride, (uint64_t*)tkeys, cap - 1,
                       (uint64_t*)emit, (uint32_t*)emit_ctr, emit_cap,
                       (const uint32_t*)attr_start, (int32_t*)attr_pool);
    return (int)hipGetLastError();
}

int df_pool_lens(const void* strc, const void* pool_cols, uint32_t npc, uint32_t n,
                 uint64_t stride, uint64_t base_row, void* row_len, uint64_t stream) {
    hipLaunchKernelGGL(k_pool_lens, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint64_t*)strc, (const uint8_t*)pool_cols, npc, n,
                       stride, base_row, (uint32_t*)row_len);
    return (int)hipGetLastError();
}

int df_pool_gather(const void* payload, const void* strc, const void* pool_cols,
                   uint32_t npc, uint32_t n, uint64_t stride, uint64_t base_row,
                   const void* row_start, void* pool, uint64_t pool_base,
                   void* out_rowref, void* out_lens,
                   uint64_t out_stride, uint64_t out_base_row,
                   uint64_t stream) {
    hipLaunchKernelGGL(k_pool_gather, dim3(grid_for(n)), dim3(BLOCK), 0, STREAM(stream),
                       (const uint8_t*)payload, (const uint64_t*)strc,
                       (const uint8_t*)pool_cols, npc, n, stride, base_row,
                       (const uint64_t*)row_start, (uint8_t*)pool, pool_base,
                       (uint64_t*)out_rowref, (int16_t*)out_lens,
                       out_stride, out_base_row);
    return (int)hipGetLastError();
}

int df_rollup_l7(void* u64c, void* u32c, void* u8c, uint64_t stride,
                 uint64_t base_row, uint32_t n, uint64_t time_base_s,
                 const void* specs, uint32_t n_tables, const void* ptrs,
                 const void* caps, uint64_t stream) {
    L7Cols cols{(uint64_t*)u64c, (uint32_t*)u32c, (uint8_t*)u8c,
                nullptr, nullptr, nullptr, stride, base_row};
    RuMulti mu;
    RuTablePtrs tp;
    ru_multi_fill(specs, n_tables, (const uint64_t*)ptrs,
                  (const uint32_t*)caps, mu, tp);
    uint32_t blocks = grid_for(n);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_rollup_l7, dim3(blocks), dim3(BLOCK), 0, STREAM(stream),
                       cols, n, time_base_s, mu, tp);
    return (int)hipGetLastError();
}

int df_pack_bits(const void* src, uint32_t n, uint32_t base, uint32_t bits,
                 void* out, uint32_t out_words, uint64_t stream) {
    hipLaunchKernelGGL(k_pack_bits, dim3(grid_for(out_words)), dim3(BLOCK),
                       0, STREAM(stream), (const uint32_t*)src, n, base,
                       bits, (uint32_t*)out, out_words);
    return (int)hipGetLastError();
}

int df_unpack_bits(const void* packed, uint32_t n, uint32_t base,
                   uint32_t bits, void* out, uint64_t stream) {
    hipLaunchKernelGGL(k_unpack_bits, dim3(grid_for(n)), dim3(BLOCK), 0,
                       STREAM(stream), (const uint32_t*)packed, n, base,
                       bits, (uint32_t*)out);
    return (int)hipGetLastError();
}

}  // extern "C"
