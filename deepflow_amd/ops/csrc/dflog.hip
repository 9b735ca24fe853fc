// dflog — K11: GPU-resident application-log store and substring search.
//
// Replaces the host path of ingest/applog_pipeline.py (one Python dict per
// line, an interpreter loop over every stored row per search) with: raw
// payload bytes kept in an HBM pool exactly as they arrived, thread-per-line
// parsing into row columns, and a flat, bandwidth-bound scan of the pool per
// query.
//
// Rules: wave = 64 lanes, blocks are multiples of 64; table rules are in
// dftable.h. Particular to this unit:
//  - app ids are slot indices of a table probed from `h & mask`. The
//    claimer alone writes the slot's metadata and nobody reads it before
//    the next launch.
//  - 64-bit hash identity is accepted for app names as it is for every
//    other dictionary here.
//
// Flat scan, not row scan: k_log_scan walks pool bytes, not rows. Bodies
// are 0..kilobytes long; a thread-per-row matcher would diverge on length
// and load each lane's bytes from an unrelated address. The flat scan
// stages a fixed tile with 16-byte loads, tests every start position from
// LDS and only maps the (rare) hits back to a row with a binary search over
// body_off, which is non-decreasing in row index.
//
// K13, regex search: k_log_regex is the same flat scan with a DFA walk from
// every start position in place of the compare. The pattern's tables (up
// to 32 KiB) are staged in LDS beside the tile: 17168 bytes of static LDS
// plus the tables as dynamic LDS, 50192 bytes at the most. The largest
// pattern leaves three workgroups (12 waves) per CU, a small one as many
// as k_log_scan has; see the kernel.
//
// K14, log patterns: k_log_patterns hashes the template of every selected
// body (one lane per row) and groups the rows in a query-scoped table, with
// a per-block LDS table in front of it; see the kernel.
#include <string.h>
#include "dftable.h"

namespace {

constexpr uint64_t LOG_APP_SEED = 0x4C4F474150504944ull;    // "LOGAPPID"

constexpr uint32_t LOG_TILE = 16384;        // match start positions per block
constexpr uint32_t LOG_MAX_NEEDLES = 8;
constexpr uint32_t LOG_MAX_NEEDLE = 128;
// staged bytes: tile + the longest needle's overhang, in whole 16-byte
// chunks, so every LDS index the compare loop can form is initialised
constexpr uint32_t LOG_STAGE_CHUNKS = (LOG_TILE + LOG_MAX_NEEDLE) / 16;
// positions handled per block iteration: each lane owns one dword
constexpr uint32_t LOG_STRIDE = BLOCK * 4;

// histogram tables of up to this many (bucket, severity) cells are
// pre-aggregated per block in LDS (16 KiB of u32 counters); larger ones,
// up to 4096 buckets x 8, go straight to global atomics
constexpr uint32_t LOG_HIST_LDS_CELLS = 4096;
constexpr uint32_t LOG_HIST_LDS_BUCKETS = LOG_HIST_LDS_CELLS / 8;
constexpr uint32_t LOG_SELECT_MAX_BLOCKS = 2048;

DEV uint8_t fold_ascii(uint8_t c) {
    return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c;
}

// four bytes at once: set 0x20 in every byte that is 'A'..'Z'
DEV uint32_t fold_ascii4(uint32_t x) {
    uint32_t t = x & 0x7f7f7f7fu;
    uint32_t ge = t + 0x3f3f3f3fu;          // bit 7 set when byte >= 0x41
    uint32_t gt = t + 0x25252525u;          // bit 7 set when byte >= 0x5b
    uint32_t m = ge & ~gt & ~x & 0x80808080u;
    return x | (m >> 2);
}

template <uint32_t N>
DEV bool word_is(const uint8_t* s, uint32_t len, const char (&w)[N]) {
    if (len != N - 1) return false;
    for (uint32_t i = 0; i < N - 1; i++)
        if (fold_ascii(s[i]) != (uint8_t)w[i]) return false;
    return true;
}

// SEVERITIES of ingest/applog_pipeline.py; anything else is 6 (info)
DEV uint8_t severity_of(const uint8_t* s, uint32_t len) {
    if (word_is(s, len, "debug")) return 7;
    if (word_is(s, len, "info")) return 6;
    if (word_is(s, len, "warn")) return 4;
    if (word_is(s, len, "warning")) return 4;
    if (word_is(s, len, "error")) return 3;
    if (word_is(s, len, "fatal")) return 2;
    if (word_is(s, len, "critical")) return 2;
    return 6;
}

struct LogApps {
    uint64_t* tkeys;          // [cap]
    int64_t* app_off;         // [cap] offset of the claimer's token in pool
    int32_t* app_len;         // [cap]
    unsigned long long* drops;
    uint32_t cap_mask;
};

struct LogRows {
    int64_t* time;
    uint8_t* severity;
    uint32_t* agent_id;
    uint16_t* log_type;
    uint32_t* app_id;
    int64_t* body_off;
    int32_t* body_len;
};

// one thread per stripped, non-empty line. pool already holds the batch at
// [base, ...); line_off is relative to base. pre_* == nullptr: parse
// '<ts> <severity> <app> <body...>' as line.split(" ", 3) does. Otherwise
// the line is app bytes followed by body bytes and pre_* carry the rest.
__global__ void k_log_ingest(const uint8_t* __restrict__ pool, uint64_t base,
                             const int64_t* __restrict__ line_off,
                             const int32_t* __restrict__ line_len,
                             uint32_t n_lines,
                             const int32_t* __restrict__ pre_app_len,
                             const int64_t* __restrict__ pre_time,
                             const uint8_t* __restrict__ pre_sev,
                             int64_t now, uint32_t agent_id,
                             uint32_t log_type, LogApps apps, LogRows rows,
                             uint64_t base_row) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    uint64_t off = base + (uint64_t)line_off[i];
    uint32_t len = (uint32_t)line_len[i];
    const uint8_t* s = pool + off;

    int64_t ts = now;
    uint8_t sev = 6;
    uint32_t a_at = 0, a_len = 0;       // app token, relative to the line
    uint32_t b_at = 0;                  // body start, relative to the line
    if (pre_app_len) {
        a_len = (uint32_t)pre_app_len[i];
        if (a_len > len) a_len = len;
        b_at = a_len;
        ts = pre_time[i];
        sev = pre_sev[i];
    } else {
        uint32_t sp[3];
        uint32_t found = 0;
        for (uint32_t p = 0; p < len && found < 3; p++)
            if (s[p] == 0x20) sp[found++] = p;
        if (found == 3 && sp[0] >= 1 && sp[0] <= 18) {
            uint64_t v = 0;
            bool digits = true;
            for (uint32_t p = 0; p < sp[0]; p++) {
                uint8_t c = s[p];
                if (c < '0' || c > '9') { digits = false; break; }
                v = v * 10 + (c - '0');
            }
            if (digits) {
                ts = (int64_t)v;
                sev = severity_of(s + sp[0] + 1, sp[1] - sp[0] - 1);
                a_at = sp[1] + 1;
                a_len = sp[2] - sp[1] - 1;
                b_at = sp[2] + 1;
            }
        }
    }

    uint64_t h = str_hash(s + a_at, a_len, LOG_APP_SEED);
    bool claimed;
    uint32_t aid = table_claim(apps.tkeys, apps.cap_mask, h,
                               (uint32_t)(h & apps.cap_mask), &claimed);
    if (aid == DICT_ID_INVALID) {
        atomicAdd(apps.drops, 1ull);
    } else if (claimed) {
        apps.app_off[aid] = (int64_t)(off + a_at);
        apps.app_len[aid] = (int32_t)a_len;
    }

    uint64_t row = base_row + i;
    rows.time[row] = ts;
    rows.severity[row] = sev;
    rows.agent_id[row] = agent_id;
    rows.log_type[row] = (uint16_t)log_type;
    rows.app_id[row] = aid;
    rows.body_off[row] = (int64_t)(off + b_at);
    rows.body_len[row] = (int32_t)(len - b_at);
}

// needles of one query, passed by value as a kernel argument
struct LogNeedles {
    uint8_t bytes[LOG_MAX_NEEDLES][LOG_MAX_NEEDLE];
    uint32_t len[LOG_MAX_NEEDLES];
    uint32_t n;
    uint32_t maxlen;
};

// last row in [lo, hi) whose body_off <= p, or -1
DEV int64_t last_row_le(const int64_t* __restrict__ body_off, int64_t lo,
                        int64_t hi, int64_t p) {
    while (lo < hi) {
        int64_t mid = lo + ((hi - lo) >> 1);
        if (body_off[mid] <= p) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// Block b owns match starts in [scan_lo + b*TILE, scan_lo + (b+1)*TILE),
// clipped at scan_hi. scan_lo is a multiple of 16 and the pool's capacity
// is too, so every 16-byte load that starts below scan_hi is in bounds.
__global__ __launch_bounds__(BLOCK)
void k_log_scan(const uint8_t* __restrict__ pool, uint64_t scan_lo,
                uint64_t scan_hi,
                const int64_t* __restrict__ body_off,
                const int32_t* __restrict__ body_len, uint64_t n_rows,
                LogNeedles nd, uint32_t fold, uint32_t* __restrict__ mask) {
    __shared__ uint4 s_tile4[LOG_STAGE_CHUNKS];
    __shared__ uint8_t s_needle[LOG_MAX_NEEDLES][LOG_MAX_NEEDLE];
    __shared__ uint32_t s_first[LOG_MAX_NEEDLES];
    __shared__ uint32_t s_fmask[LOG_MAX_NEEDLES];
    __shared__ int64_t s_rlo, s_rhi;

    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = scan_lo + (uint64_t)blockIdx.x * LOG_TILE;
    if (t0 >= scan_hi) return;                        // uniform per block
    const uint64_t left = scan_hi - t0;
    const uint32_t n_start = left < LOG_TILE ? (uint32_t)left : LOG_TILE;
    const uint64_t want = (uint64_t)LOG_TILE + nd.maxlen - 1;
    const uint32_t stage = left < want ? (uint32_t)left : (uint32_t)want;
    const uint32_t chunks = (stage + 15) / 16;

    const uint4* src = reinterpret_cast<const uint4*>(pool + t0);
    for (uint32_t c = tid; c < LOG_STAGE_CHUNKS; c += BLOCK) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (c < chunks) {
            v = src[c];
            if (fold) {
                v.x = fold_ascii4(v.x); v.y = fold_ascii4(v.y);
                v.z = fold_ascii4(v.z); v.w = fold_ascii4(v.w);
            }
        }
        s_tile4[c] = v;
    }
    for (uint32_t b = tid; b < LOG_MAX_NEEDLES * LOG_MAX_NEEDLE; b += BLOCK)
        s_needle[b / LOG_MAX_NEEDLE][b % LOG_MAX_NEEDLE] =
            nd.bytes[b / LOG_MAX_NEEDLE][b % LOG_MAX_NEEDLE];
    if (tid < LOG_MAX_NEEDLES) {
        uint32_t L = tid < nd.n ? nd.len[tid] : 0;
        uint32_t w = 0, m = 0;
        for (uint32_t b = 0; b < 4 && b < L; b++) {
            w |= (uint32_t)nd.bytes[tid][b] << (8 * b);
            m |= 0xffu << (8 * b);
        }
        s_first[tid] = w;
        s_fmask[tid] = m;
    }
    if (tid == 0) {
        // rows that can hold a byte of this tile: [s_rlo, s_rhi]
        int64_t hi = last_row_le(body_off, 0, (int64_t)n_rows,
                                 (int64_t)(t0 + n_start - 1));
        int64_t lo = hi < 0 ? 0
                   : last_row_le(body_off, 0, hi + 1, (int64_t)t0);
        s_rlo = lo < 0 ? 0 : lo;
        s_rhi = hi;
    }
    __syncthreads();
    const int64_t rlo = s_rlo, rhi = s_rhi;
    if (rhi < 0) return;                              // uniform per block

    const uint32_t* tile32 = reinterpret_cast<const uint32_t*>(s_tile4);
    const uint8_t* tile8 = reinterpret_cast<const uint8_t*>(s_tile4);
    const uint32_t n_needles = nd.n;

    // the row of this thread's previous hit: tested first, so a dense
    // needle does not pay a binary search per hit
    int64_t cr = -1, c_lo = 0, c_hi = 0;

    for (uint32_t it = 0; it * LOG_STRIDE < n_start; it++) {
        uint32_t q0 = it * LOG_STRIDE + tid * 4;
        if (q0 >= n_start) continue;
        uint64_t w64 = (uint64_t)tile32[q0 / 4]
                     | ((uint64_t)tile32[q0 / 4 + 1] << 32);
        for (uint32_t j = 0; j < 4; j++) {
            uint32_t q = q0 + j;
            if (q >= n_start) break;
            uint32_t w = (uint32_t)(w64 >> (8 * j));
            for (uint32_t k = 0; k < n_needles; k++) {
                if ((w & s_fmask[k]) != s_first[k]) continue;
                uint32_t L = nd.len[k];
                if (q + L > stage) continue;
                bool eq = true;
                for (uint32_t b = 4; b < L; b++)
                    if (tile8[q + b] != s_needle[k][b]) { eq = false; break; }
                if (!eq) continue;
                int64_t p = (int64_t)(t0 + q);
                if (!(cr >= 0 && c_lo <= p && p + (int64_t)L <= c_hi)) {
                    int64_t r = last_row_le(body_off, rlo, rhi + 1, p);
                    if (r < 0) continue;
                    cr = r;
                    c_lo = body_off[r];
                    c_hi = c_lo + body_len[r];
                    if (p + (int64_t)L > c_hi) continue;
                }
                uint32_t bit = 1u << k;
                // a stale read only costs a redundant atomic
                if (!(__atomic_load_n(&mask[cr], __ATOMIC_RELAXED) & bit))
                    atomicOr(&mask[cr], bit);
            }
        }
    }
}

// thread per row (grid-stride): filter flag + optional histogram
__global__ __launch_bounds__(BLOCK)
void k_log_select(const int64_t* __restrict__ time,
                  const uint8_t* __restrict__ severity,
                  const uint32_t* __restrict__ app_id,
                  const uint32_t* __restrict__ mask, uint64_t n_rows,
                  uint32_t severity_max, int64_t t_lo, int64_t t_hi,
                  uint32_t use_app, uint64_t app_key,
                  const uint64_t* __restrict__ tkeys, uint32_t app_cap,
                  uint32_t need, uint8_t* __restrict__ flags,
                  unsigned long long* __restrict__ hist, uint64_t interval,
                  uint32_t n_buckets) {
    __shared__ uint32_t s_hist[LOG_HIST_LDS_CELLS];
    const bool in_lds = hist && n_buckets <= LOG_HIST_LDS_BUCKETS;
    const uint32_t cells = n_buckets * 8;
    if (in_lds) {
        for (uint32_t c = threadIdx.x; c < cells; c += BLOCK) s_hist[c] = 0;
        __syncthreads();
    }
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
         r < n_rows; r += step) {
        uint32_t sev = severity[r];
        int64_t ts = time[r];
        bool ok = sev <= severity_max && ts >= t_lo && ts <= t_hi
                  && (mask[r] & need) == need;
        if (ok && use_app) {
            uint32_t a = app_id[r];
            ok = a < app_cap && tkeys[a] == app_key;
        }
        flags[r] = ok ? 1 : 0;
        if (ok && hist) {
            uint64_t b = (uint64_t)(ts - t_lo) / interval;
            if (b < n_buckets) {
                uint32_t cell = (uint32_t)b * 8 + (sev > 7 ? 7 : sev);
                if (in_lds) atomicAdd(&s_hist[cell], 1u);
                else atomicAdd(&hist[cell], 1ull);
            }
        }
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < cells; c += BLOCK) {
            uint32_t v = s_hist[c];
            if (v) atomicAdd(&hist[c], (unsigned long long)v);
        }
    }
}

// ---------------------------------------------------------------- K13
// Regex search: the flat scan with a DFA walk in place of the compare.
// The host (query/logregex.py) compiles the pattern to an anchored DFA over
// byte classes; trying every start position makes it a search. State 0 is
// dead, state 1 the start; an entry of `next` carries the target state in
// its low 15 bits and "the target accepts" in bit 15, so a step is one
// class lookup and one table lookup, both in LDS.
constexpr uint32_t LOG_RE_OVERHANG = 256;           // tuning, not semantics
constexpr uint32_t LOG_RE_TABLE_BYTES = 32 * 1024;  // n_states*n_classes*2
constexpr uint32_t LOG_RE_MAX_PATTERN = 256;
constexpr uint32_t LOG_RE_MAX_CLASSES = 64;
constexpr uint32_t LOG_RE_STAGE_CHUNKS = (LOG_TILE + LOG_RE_OVERHANG) / 16;
// the uploaded tables: class_of u8[256], then next u16[n_states*n_classes]
constexpr uint32_t LOG_RE_BLOB_CHUNKS = (256 + LOG_RE_TABLE_BYTES) / 16;
constexpr uint32_t LOG_RE_BIT = 1u << 8;            // needles keep bits 0..7
constexpr uint32_t RE_ACCEPT = 1u << 15;
constexpr uint32_t RE_STATE = RE_ACCEPT - 1;
constexpr uint32_t RE_ANCHOR_START = 1, RE_ANCHOR_END = 2,
                   RE_END_BEFORE_NL = 4, RE_NULLABLE = 8;
static_assert(LOG_RE_OVERHANG % 16 == 0, "staged in 16-byte chunks");
static_assert(LOG_RE_STAGE_CHUNKS * 16 + LOG_RE_BLOB_CHUNKS * 16 + 512 + 16
              <= 64 * 1024, "static + dynamic LDS of k_log_regex");

// Block b owns match starts in [scan_lo + b*TILE, scan_lo + (b+1)*TILE),
// clipped at scan_hi, as in k_log_scan, and stages tile + overhang. A match
// has no length limit: a walk still alive at the end of the staged bytes
// goes on byte by byte from the pool, up to the end of its row.
//
// Bounds. LDS: every tile index is < stage. Global: every pool index is
// < body_off[r] + body_len[r] <= scan_hi (= the pool's length) for the row
// r the walk started in; the 16-byte staging loads start below scan_hi and
// the pool's capacity is a multiple of 16. Nothing reads at or past
// scan_hi otherwise. Table indices are state * n_classes + class with
// state < n_states and class < n_classes by construction of the tables
// (LogRegex asserts it), inside the staged blob.
//
// Without anchor_end the shortest accept from a start decides: if it ends
// past the row's end, no match from that start lies inside the row. With
// anchor_end the walk runs to the row's end and tests the accept bit there
// (or one byte earlier when that byte is \n and `$` allows it). With
// anchor_start only a row's first byte can start a match, so the block
// walks its rows instead of its positions. A match of length 0 is the
// host's business (GpuLogStore._flags); empty bodies are skipped here.
//
// LDS: 16640 (tile) + 512 (first-step table) + 16 static, and the tables
// as dynamic LDS sized to the pattern: 256 + n_states * n_classes * 2
// bytes in 16-byte chunks, 33024 at the most. That is 50192 bytes for the
// largest pattern, under the 64 KiB a workgroup may have; of the CU's
// 160 KiB it leaves three workgroups, 12 waves per CU (3 per SIMD). A
// pattern with tables of a few hundred bytes leaves eight workgroups, the
// 32 waves a CU holds. The walk is latency-bound on dependent LDS reads,
// which is what those waves have to hide.
__global__ __launch_bounds__(BLOCK)
void k_log_regex(const uint8_t* __restrict__ pool, uint64_t scan_lo,
                 uint64_t scan_hi,
                 const int64_t* __restrict__ body_off,
                 const int32_t* __restrict__ body_len, uint64_t n_rows,
                 const uint4* __restrict__ blob, uint32_t n_states,
                 uint32_t nc, uint32_t flags, uint32_t* __restrict__ mask) {
    __shared__ uint4 s_tile4[LOG_RE_STAGE_CHUNKS];
    extern __shared__ uint4 s_blob4[];      // blob_chunks of them
    __shared__ uint16_t s_start[256];       // next[start state] by byte
    __shared__ int64_t s_rlo, s_rhi;

    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = scan_lo + (uint64_t)blockIdx.x * LOG_TILE;
    if (t0 >= scan_hi) return;                        // uniform per block
    const uint64_t left = scan_hi - t0;
    const uint32_t n_start = left < LOG_TILE ? (uint32_t)left : LOG_TILE;
    const uint64_t want = (uint64_t)LOG_TILE + LOG_RE_OVERHANG;
    const uint32_t stage = left < want ? (uint32_t)left : (uint32_t)want;
    const uint32_t chunks = (stage + 15) / 16;

    const uint4* src = reinterpret_cast<const uint4*>(pool + t0);
    for (uint32_t c = tid; c < chunks; c += BLOCK) s_tile4[c] = src[c];
    const uint32_t blob_chunks = (256 + n_states * nc * 2 + 15) / 16;
    for (uint32_t c = tid; c < blob_chunks; c += BLOCK) s_blob4[c] = blob[c];
    if (tid == 0) {
        // rows that can hold a byte of this tile: [s_rlo, s_rhi]
        int64_t hi = last_row_le(body_off, 0, (int64_t)n_rows,
                                 (int64_t)(t0 + n_start - 1));
        int64_t lo = hi < 0 ? 0
                   : last_row_le(body_off, 0, hi + 1, (int64_t)t0);
        s_rlo = lo < 0 ? 0 : lo;
        s_rhi = hi;
    }
    __syncthreads();
    const int64_t rlo = s_rlo, rhi = s_rhi;
    if (rhi < 0) return;                              // uniform per block

    const uint32_t* tile32 = reinterpret_cast<const uint32_t*>(s_tile4);
    const uint8_t* tile8 = reinterpret_cast<const uint8_t*>(s_tile4);
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(s_blob4);
    const uint16_t* nxt = reinterpret_cast<const uint16_t*>(s_blob4) + 128;
    for (uint32_t b = tid; b < 256; b += BLOCK)
        s_start[b] = nxt[nc + cls[b]];
    __syncthreads();

    const bool anchor_end = flags & RE_ANCHOR_END;
    const bool nl_ok = flags & RE_END_BEFORE_NL;
    const uint32_t nullable = (flags & RE_NULLABLE) ? 1 : 0;
    const int64_t tile_lo = (int64_t)t0, tile_hi = (int64_t)(t0 + n_start);

    // Both walks take pool offsets g >= t0 and read the bytes below
    // t0 + stage from LDS, the rest from the pool (two loops, so that
    // neither load has to be a flat one).
    const int64_t stage_hi = (int64_t)(t0 + stage);
    // from state st (not accepting) at pool offset g: is there an accept
    // whose last byte lies below end?
    auto shortest = [&](int64_t g, uint32_t st, int64_t end) -> bool {
        const int64_t lds_end = end < stage_hi ? end : stage_hi;
        for (; g < lds_end; g++) {
            uint32_t e = nxt[st * nc + cls[tile8[(uint64_t)g - t0]]];
            if (!e) return false;
            if (e & RE_ACCEPT) return true;
            st = e;
        }
        for (; g < end; g++) {
            uint32_t e = nxt[st * nc + cls[pool[g]]];
            if (!e) return false;
            if (e & RE_ACCEPT) return true;
            st = e;
        }
        return false;
    };
    // does [p, end) as a whole, or without its final \n, end in an accept?
    auto to_end = [&](int64_t p, int64_t end) -> bool {
        uint32_t st = 1, acc = nullable, acc_before = 0;
        uint8_t last = 0;
        auto eat = [&](uint8_t b, bool is_last) -> bool {
            if (is_last) { acc_before = acc; last = b; }
            uint32_t e = nxt[st * nc + cls[b]];
            st = e & RE_STATE;
            acc = e >> 15;
            return e != 0;
        };
        const int64_t lds_end = end < stage_hi ? end : stage_hi;
        int64_t g = p;
        bool alive = true;
        for (; alive && g < lds_end; g++)
            alive = eat(tile8[(uint64_t)g - t0], g == end - 1);
        for (; alive && g < end; g++)
            alive = eat(pool[g], g == end - 1);
        return acc || (nl_ok && acc_before && last == '\n');
    };
    auto mark = [&](int64_t r) {
        // a stale read only costs a redundant atomic
        if (!(__atomic_load_n(&mask[r], __ATOMIC_RELAXED) & LOG_RE_BIT))
            atomicOr(&mask[r], LOG_RE_BIT);
    };

    if (flags & RE_ANCHOR_START) {
        // a row is owned by the block its body starts in. Of rows that tie
        // on body_off all but the last are empty and cannot match.
        for (int64_t r = rlo + tid; r <= rhi; r += BLOCK) {
            int64_t p = body_off[r];
            int64_t end = p + body_len[r];
            if (p < tile_lo || p >= tile_hi || p >= end) continue;
            if (anchor_end ? to_end(p, end) : shortest(p, 1, end)) mark(r);
        }
        return;
    }

    // the row of this thread's previous lookup: body [c_lo, c_hi), and
    // c_next, where the next row's body starts. Between c_hi and c_next lie
    // header bytes, which belong to no body.
    int64_t cr = -1, c_lo = 0, c_hi = 0, c_next = 0;
    auto row_of = [&](int64_t p) -> bool {
        if (!(cr >= 0 && c_lo <= p && p < c_next)) {
            int64_t r = last_row_le(body_off, rlo, rhi + 1, p);
            if (r < 0) return false;
            cr = r;
            c_lo = body_off[r];
            c_hi = c_lo + body_len[r];
            c_next = (uint64_t)(r + 1) < n_rows ? body_off[r + 1]
                                                 : INT64_MAX;
        }
        return p < c_hi;
    };

    for (uint32_t it = 0; it * LOG_STRIDE < n_start; it++) {
        uint32_t q0 = it * LOG_STRIDE + tid * 4;
        if (q0 >= n_start) continue;
        uint32_t w = tile32[q0 / 4];
        for (uint32_t j = 0; j < 4; j++) {
            uint32_t q = q0 + j;
            if (q >= n_start) break;
            // almost every start dies here, on its first byte
            uint32_t e = s_start[(w >> (8 * j)) & 0xff];
            if (!e) continue;
            int64_t p = (int64_t)(t0 + q);
            if (anchor_end) {
                if (row_of(p) && to_end(p, c_hi)) mark(cr);
                continue;
            }
            // walk the staged bytes first; the row is looked up only for
            // a start that got somewhere
            uint32_t pos = q + 1;
            while (!(e & RE_ACCEPT) && pos < stage) {
                e = nxt[e * nc + cls[tile8[pos]]];
                if (!e) break;
                pos++;
            }
            if (!e || !row_of(p)) continue;
            if (e & RE_ACCEPT) {
                if ((int64_t)(t0 + pos) > c_hi) continue;
            } else if (!shortest((int64_t)(t0 + pos), e, c_hi)) {
                continue;               // alive at the end of the stage
            }
            mark(cr);
        }
    }
}

// ---------------------------------------------------------- retention
// Evicting the `first` oldest rows is a prefix cut, out of place: the row
// columns lose their first `first` entries and the pool loses the bytes
// below
//     cut = (body_off[first-1] + body_len[first-1]) & ~15,
// the end of the last evicted body rounded down to 16 (the whole pool when
// every row goes). The new pool is [arena | old bytes cut..pool_len).
//
// Why nothing a kept row needs lies below cut. k_log_ingest places row i's
// body at [off + b_at, off + len): it always runs to the end of the line,
// for parsed lines, free-form lines and the pre_* layout alike, and the
// header and the app token lie inside the line before it. Lines of a batch
// do not overlap and come in increasing offset (split_log_lines yields
// them sorted, _ingest_row_run lays them end to end), and a batch starts
// at the pool's length, past every earlier line. So the line of row
// `first` starts at or after the end of body first-1 >= cut, and so does
// everything of every later row.
//
// What does lie below cut and is still needed: app names. A slot records
// where its *claimer's* token lies (app_off), and the claimer may be
// evicted while later rows keep the id. Every live slot (tkeys != 0) whose
// app_off < cut has its name copied into the arena at the front of the new
// pool; names that an earlier eviction put into an arena lie below cut and
// move again. A slot with app_off >= cut keeps pointing into the copied
// suffix, whoever claimed it (the rounding can leave the last evicted
// row's token above cut; its bytes are copied with the suffix), and is
// rebased like a body: new = old - cut + arena. Tokens of distinct slots
// are disjoint byte ranges that start below cut and end before cut + 16
// (a token ends before its body does), so the packed arena, padded to 16,
// is at most cut + 16 and the new pool at most 16 bytes longer than the
// old one; the wrapper sizes the new pool from the arena it read back.
//
// Arena bytes sit below body_off[0]: last_row_le gives -1 there, so the
// scans attribute a hit inside a relocated name to no row, as they do for
// header bytes. body_off stays non-decreasing (one constant is added).
//
// tkeys, app_len and drops are not touched: app ids are slot indices.

// pass 1, thread per app slot: bump-allocate arena bytes. reloc[s] = new
// offset of the slot's name, or -1 for a slot that is empty or stays in the
// suffix. out[0] (zeroed on the stream before the launch) ends as the
// packed arena length, out[1] is the cut, so the host learns both from one
// copy. Every thread derives the cut from the same two words.
__global__ __launch_bounds__(BLOCK)
void k_log_evict_plan(const uint64_t* __restrict__ tkeys,
                      const int64_t* __restrict__ app_off,
                      const int32_t* __restrict__ app_len, uint32_t cap,
                      const int64_t* __restrict__ body_off,
                      const int32_t* __restrict__ body_len, uint64_t first,
                      uint64_t n_rows, int64_t pool_len,
                      int64_t* __restrict__ reloc,
                      unsigned long long* __restrict__ out) {
    const int64_t cut = first == n_rows ? pool_len
        : (body_off[first - 1] + body_len[first - 1]) & ~(int64_t)15;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        out[1] = (unsigned long long)cut;
    const uint32_t step = gridDim.x * BLOCK;
    for (uint32_t s = blockIdx.x * BLOCK + threadIdx.x; s < cap; s += step) {
        int64_t to = -1;
        if (tkeys[s] != EMPTY_KEY && app_off[s] < cut)
            to = (int64_t)atomicAdd(&out[0],
                                    (unsigned long long)(uint32_t)app_len[s]);
        reloc[s] = to;
    }
}

// pass 2, one flat grid-stride index space: [0, cap) are app slots (copy a
// relocated name and point the slot at it, or rebase the slot), [cap,
// cap + n_keep) are kept rows (new_col[r] = old_col[r + first]). Names are
// tokens of a line, tens of bytes: a byte loop per thread, as in
// k_log_ingest. app_off is updated in place; each slot is read and written
// by one thread only.
//
// Bounds. A name is read from [off, off + len) of the old pool only when
// that lies inside [0, old_len), and written to [to, to + len) of the new pool
// only when that lies inside [0, arena); pass 1 hands out disjoint ranges
// that sum to *arena_len <= arena. Row r reads old_col[r + first] with
// r + first < first + n_keep = the old row count.
__global__ __launch_bounds__(BLOCK)
void k_log_evict(const uint8_t* __restrict__ old_pool,
                 uint8_t* __restrict__ new_pool, int64_t old_len,
                 int64_t cut, int64_t arena,
                 const uint64_t* __restrict__ tkeys,
                 int64_t* __restrict__ app_off,
                 const int32_t* __restrict__ app_len,
                 const int64_t* __restrict__ reloc, uint32_t cap,
                 LogRows src, LogRows dst, uint64_t first, uint64_t n_keep) {
    const int64_t shift = arena - cut;
    const uint64_t total = (uint64_t)cap + n_keep;
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < total;
         i += step) {
        if (i < cap) {
            if (tkeys[i] == EMPTY_KEY) continue;
            const int64_t to = reloc[i];
            const int64_t off = app_off[i];
            if (to < 0) {
                app_off[i] = off + shift;
                continue;
            }
            const int64_t len = (int64_t)(uint32_t)app_len[i];
            if (off >= 0 && off + len <= old_len && to + len <= arena)
                for (int64_t b = 0; b < len; b++)
                    new_pool[to + b] = old_pool[off + b];
            app_off[i] = to;
        } else {
            const uint64_t r = i - cap, o = r + first;
            dst.time[r] = src.time[o];
            dst.severity[r] = src.severity[o];
            dst.agent_id[r] = src.agent_id[o];
            dst.log_type[r] = src.log_type[o];
            dst.app_id[r] = src.app_id[o];
            dst.body_off[r] = src.body_off[o] + shift;
            dst.body_len[r] = src.body_len[o];
        }
    }
}

// ---------------------------------------------------------------- K14
// Log patterns: group the selected rows by the template of their body.
// query/logpattern.py is the definition; this is its one-pass form. A body
// is cut into tokens at delimiter bytes, a token that holds an ASCII digit
// collapses to one WILDCARD symbol, and the key is FNV-1a over the symbols
// (bytes 0..255, WILDCARD, TRUNC), finished with mix64. `saved` is h as it
// stood after the last delimiter, so a token that turns out to hold a digit
// is taken back with one assignment.
//
// Row scan, not flat scan: unlike a substring match, the key depends on
// where the body starts, and every selected body is read exactly once. One
// lane per row; adjacent lanes' rows are adjacent in the pool, so a wave's
// loads fall into one contiguous region of a few KiB, and the prefix cap
// bounds the divergence on length.
constexpr uint32_t LOG_PAT_PREFIX = 512;
constexpr uint32_t LOG_PAT_WILDCARD = 0x100, LOG_PAT_TRUNC = 0x101;
constexpr uint64_t LOG_PAT_FNV_OFFSET = 0xCBF29CE484222325ull;
constexpr uint64_t LOG_PAT_FNV_PRIME = 0x100000001B3ull;
// per-block pre-aggregation table: 5 KiB of LDS
constexpr uint32_t LOG_PAT_LSLOT = 256;
constexpr uint32_t LOG_PAT_LPROBE = 8;

// one bit per byte base..base+63: every byte <= 0x20 and "'(),;:=[]{}|
constexpr uint64_t pat_delim_bits(uint32_t base) {
    const char set[] = "\"'(),;:=[]{}|";
    uint64_t m = 0;
    for (uint32_t i = 0; i < 64; i++) {
        uint32_t c = base + i;
        bool d = c <= 0x20;
        for (uint32_t k = 0; k + 1 < sizeof(set); k++)
            d = d || c == (uint8_t)set[k];
        if (d) m |= 1ull << i;
    }
    return m;
}
constexpr uint64_t LOG_PAT_DELIM_LO = pat_delim_bits(0);
constexpr uint64_t LOG_PAT_DELIM_HI = pat_delim_bits(64);

DEV bool pat_is_delim(uint32_t c) {         // bytes >= 0x80 are literals
    return c < 128
        && (((c < 64 ? LOG_PAT_DELIM_LO : LOG_PAT_DELIM_HI) >> (c & 63)) & 1);
}

DEV uint64_t pat_fold(uint64_t h, uint32_t sym) {
    return (h ^ sym) * LOG_PAT_FNV_PRIME;
}

// Key of the body at pool[off, off + len). The bytes come in aligned
// 16-byte chunks; of each chunk only the bytes inside the body's prefix are
// looked at.
// Bounds: a chunk starts at a multiple of 16 below off + n <= pool_len <=
// the pool's capacity, which is a multiple of 16 (as the pool's base is),
// so the chunk ends inside the capacity. A row that does not lie inside
// [0, pool_len) is read as far as pool_len and no further.
DEV uint64_t pattern_key(const uint8_t* __restrict__ pool, uint64_t pool_len,
                         int64_t body_off, int32_t body_len) {
    uint64_t h = LOG_PAT_FNV_OFFSET, saved = h;
    bool digit = false;
    const uint64_t off = body_off < 0 ? pool_len : (uint64_t)body_off;
    const uint32_t len = body_len < 0 ? 0 : (uint32_t)body_len;
    uint64_t end = off + (len < LOG_PAT_PREFIX ? len : LOG_PAT_PREFIX);
    if (end > pool_len) end = pool_len;
    for (uint64_t a = off & ~15ull; a < end; a += 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(pool + a);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t lo = a < off ? (uint32_t)(off - a) : 0;
        const uint32_t hi = end - a < 16 ? (uint32_t)(end - a) : 16;
#pragma unroll
        for (uint32_t b = 0; b < 16; b++) {
            if (b < lo || b >= hi) continue;
            const uint32_t c = (w[b / 4] >> (8 * (b % 4))) & 0xffu;
            if (pat_is_delim(c)) {
                if (digit) h = pat_fold(saved, LOG_PAT_WILDCARD);
                digit = false;
                h = pat_fold(h, c);
                saved = h;
            } else {
                h = pat_fold(h, c);
                digit = digit || (c >= '0' && c <= '9');
            }
        }
    }
    if (digit) h = pat_fold(saved, LOG_PAT_WILDCARD);
    if (len > LOG_PAT_PREFIX) h = pat_fold(h, LOG_PAT_TRUNC);
    h = mix64(h);
    return h ? h : 1ull;                    // never EMPTY_KEY
}

// query-scoped table: slot = pattern. count is zeroed, first_row is
// ROW_NONE and last_row 0 before the launch (last_row means something only
// where count != 0).
struct PatTable {
    uint64_t* keys;              // [cap]
    unsigned long long* count;   // [cap]
    uint32_t* first_row;         // [cap] atomicMin
    uint32_t* last_row;          // [cap] atomicMax
    unsigned long long* drops;   // rows whose pattern found the table full
    uint32_t cap_mask;
};

// The table only fills: a key that once found it full finds it full ever
// after, and a key that holds a slot is found by every later probe. So a
// pattern either gets all of its rows counted or all of them dropped.
DEV void pat_add_global(const PatTable& pt, uint64_t key, uint32_t n,
                        uint32_t rmin, uint32_t rmax) {
    uint32_t slot = table_claim(pt.keys, pt.cap_mask, key,
                                (uint32_t)(mix64(key) & pt.cap_mask));
    if (slot == ROW_NONE) {
        atomicAdd(pt.drops, (unsigned long long)n);
        return;
    }
    atomicAdd(&pt.count[slot], (unsigned long long)n);
    atomicMin(&pt.first_row[slot], rmin);
    atomicMax(&pt.last_row[slot], rmax);
}

// thread per row (grid-stride). A handful of patterns usually carry most
// rows: counts, lowest and highest row are merged per block in an LDS table
// and flushed once per block, as the edges of k_trace_fold are. A row whose
// key finds no LDS slot within LOG_PAT_LPROBE steps goes to the global
// table directly; sums, minima and maxima do not care which way a row took.
// out_key (optional, u64 per row): the key of every selected row.
__global__ __launch_bounds__(BLOCK)
void k_log_patterns(const uint8_t* __restrict__ pool, uint64_t pool_len,
                    const int64_t* __restrict__ body_off,
                    const int32_t* __restrict__ body_len,
                    const uint8_t* __restrict__ flags, uint64_t n_rows,
                    PatTable pt, uint64_t* __restrict__ out_key) {
    __shared__ unsigned long long lkey[LOG_PAT_LSLOT];
    __shared__ uint32_t lcnt[LOG_PAT_LSLOT];
    __shared__ uint32_t lmin[LOG_PAT_LSLOT];
    __shared__ uint32_t lmax[LOG_PAT_LSLOT];
    for (uint32_t i = threadIdx.x; i < LOG_PAT_LSLOT; i += BLOCK) {
        lkey[i] = EMPTY_KEY;
        lcnt[i] = 0;
        lmin[i] = ROW_NONE;
        lmax[i] = 0;
    }
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * BLOCK;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
         r < n_rows; r += step) {
        if (!flags[r]) continue;
        const uint64_t key = pattern_key(pool, pool_len, body_off[r],
                                         body_len[r]);
        if (out_key) out_key[r] = key;
        const uint32_t row = (uint32_t)r;       // n_rows < ROW_NONE
        uint32_t ls = (uint32_t)(mix64(key) & (LOG_PAT_LSLOT - 1));
        bool placed = false;
        for (uint32_t probe = 0; probe < LOG_PAT_LPROBE && !placed; probe++) {
            unsigned long long cur = lkey[ls];
            if (cur == EMPTY_KEY)
                cur = atomicCAS(&lkey[ls], EMPTY_KEY,
                                (unsigned long long)key);
            if (cur == EMPTY_KEY || cur == key) placed = true;
            else ls = (ls + 1) & (LOG_PAT_LSLOT - 1);
        }
        if (placed) {
            atomicAdd(&lcnt[ls], 1u);
            atomicMin(&lmin[ls], row);
            atomicMax(&lmax[ls], row);
        } else {
            pat_add_global(pt, key, 1, row, row);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < LOG_PAT_LSLOT; i += BLOCK) {
        unsigned long long key = lkey[i];
        if (key != EMPTY_KEY)
            pat_add_global(pt, key, lcnt[i], lmin[i], lmax[i]);
    }
}

}  // namespace

extern "C" {

uint32_t df_log_tile_bytes() { return LOG_TILE; }
uint32_t df_log_re_overhang() { return LOG_RE_OVERHANG; }
// out[0..2]: table bytes, pattern bytes, byte classes
void df_log_re_limits(uint32_t* out) {
    out[0] = LOG_RE_TABLE_BYTES;
    out[1] = LOG_RE_MAX_PATTERN;
    out[2] = LOG_RE_MAX_CLASSES;
}
uint64_t df_log_app_seed() { return LOG_APP_SEED; }
uint32_t df_log_hist_lds_buckets() { return LOG_HIST_LDS_BUCKETS; }

int df_log_ingest(const void* pool, uint64_t base, const void* line_off,
                  const void* line_len, uint32_t n_lines,
                  const void* pre_app_len, const void* pre_time,
                  const void* pre_sev, int64_t now, uint32_t agent_id,
                  uint32_t log_type,
                  void* tkeys, uint32_t cap, void* app_off, void* app_len,
                  void* drops,
                  void* row_time, void* row_sev, void* row_agent,
                  void* row_type, void* row_app, void* row_boff,
                  void* row_blen, uint64_t base_row, uint64_t stream) {
    if (n_lines == 0) return 0;
    LogApps apps{(uint64_t*)tkeys, (int64_t*)app_off, (int32_t*)app_len,
                 (unsigned long long*)drops, cap - 1};
    LogRows rows{(int64_t*)row_time, (uint8_t*)row_sev, (uint32_t*)row_agent,
                 (uint16_t*)row_type, (uint32_t*)row_app, (int64_t*)row_boff,
                 (int32_t*)row_blen};
    hipLaunchKernelGGL(k_log_ingest, dim3(grid_for(n_lines)), dim3(BLOCK),
                       0, STREAM(stream),
                       (const uint8_t*)pool, base, (const int64_t*)line_off,
                       (const int32_t*)line_len, n_lines,
                       (const int32_t*)pre_app_len, (const int64_t*)pre_time,
                       (const uint8_t*)pre_sev, now, agent_id, log_type,
                       apps, rows, base_row);
    return (int)hipGetLastError();
}

// needle_bytes: n_needles strings back to back, needle_len[k] bytes each
// (host memory). Returns -1 for a needle list the kernel does not take.
int df_log_scan(const void* pool, uint64_t scan_lo, uint64_t scan_hi,
                const void* body_off, const void* body_len, uint64_t n_rows,
                const void* needle_bytes, const uint32_t* needle_len,
                uint32_t n_needles, uint32_t fold, void* mask,
                uint64_t stream) {
    if (n_needles == 0 || n_rows == 0 || scan_hi <= scan_lo) return 0;
    if (n_needles > LOG_MAX_NEEDLES || (scan_lo & 15)) return -1;
    LogNeedles nd;
    memset(&nd, 0, sizeof(nd));
    const uint8_t* src = (const uint8_t*)needle_bytes;
    for (uint32_t k = 0; k < n_needles; k++) {
        uint32_t L = needle_len[k];
        if (L < 1 || L > LOG_MAX_NEEDLE) return -1;
        memcpy(nd.bytes[k], src, L);
        src += L;
        nd.len[k] = L;
        if (L > nd.maxlen) nd.maxlen = L;
    }
    nd.n = n_needles;
    uint64_t blocks = (scan_hi - scan_lo + LOG_TILE - 1) / LOG_TILE;
    hipLaunchKernelGGL(k_log_scan, dim3((uint32_t)blocks), dim3(BLOCK), 0,
                       STREAM(stream), (const uint8_t*)pool, scan_lo,
                       scan_hi, (const int64_t*)body_off,
                       (const int32_t*)body_len, n_rows, nd, fold,
                       (uint32_t*)mask);
    return (int)hipGetLastError();
}

// table: device memory, 16-byte aligned and padded to a multiple of 16
// bytes: class_of u8[256], next u16[n_states * n_classes] (LogRegex.table()).
// Returns -1 for tables the kernel does not take, and for a pattern that
// matches the empty string without being anchored at both ends: that one
// matches every row and is not the kernel's to answer.
int df_log_regex(const void* pool, uint64_t scan_lo, uint64_t scan_hi,
                 const void* body_off, const void* body_len, uint64_t n_rows,
                 const void* table, uint32_t n_states, uint32_t n_classes,
                 uint32_t flags, void* mask, uint64_t stream) {
    if (n_classes < 1 || n_classes > LOG_RE_MAX_CLASSES || n_states < 2
        || n_states > RE_STATE
        || (uint64_t)n_states * n_classes * 2 > LOG_RE_TABLE_BYTES
        || (scan_lo & 15) || ((uintptr_t)table & 15))
        return -1;
    const uint32_t both = RE_ANCHOR_START | RE_ANCHOR_END;
    if ((flags & RE_NULLABLE) && (flags & both) != both) return -1;
    if (n_rows == 0 || scan_hi <= scan_lo) return 0;
    uint64_t blocks = (scan_hi - scan_lo + LOG_TILE - 1) / LOG_TILE;
    // dynamic LDS: the tables, in the chunks the kernel stages them in
    uint32_t lds = (256 + n_states * n_classes * 2 + 15) / 16 * 16;
    hipLaunchKernelGGL(k_log_regex, dim3((uint32_t)blocks), dim3(BLOCK), lds,
                       STREAM(stream), (const uint8_t*)pool, scan_lo,
                       scan_hi, (const int64_t*)body_off,
                       (const int32_t*)body_len, n_rows, (const uint4*)table,
                       n_states, n_classes, flags, (uint32_t*)mask);
    return (int)hipGetLastError();
}

int df_log_select(const void* time, const void* severity,
                  const void* app_id, const void* mask, uint64_t n_rows,
                  uint32_t severity_max, int64_t t_lo, int64_t t_hi,
                  uint32_t use_app, uint64_t app_key, const void* tkeys,
                  uint32_t app_cap, uint32_t need, void* flags, void* hist,
                  uint64_t interval, uint32_t n_buckets, uint64_t stream) {
    if (n_rows == 0) return 0;
    if (hist && (interval == 0 || n_buckets == 0 || n_buckets > 4096))
        return -1;
    uint32_t blocks = grid_for(n_rows);
    if (blocks > LOG_SELECT_MAX_BLOCKS) blocks = LOG_SELECT_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log_select, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), (const int64_t*)time,
                       (const uint8_t*)severity, (const uint32_t*)app_id,
                       (const uint32_t*)mask, n_rows, severity_max, t_lo,
                       t_hi, use_app, app_key, (const uint64_t*)tkeys,
                       app_cap, need, (uint8_t*)flags,
                       (unsigned long long*)hist, interval, n_buckets);
    return (int)hipGetLastError();
}

// Retention, pass 1, for dropping the `first` oldest of n_rows rows:
// reloc[cap] (i64) and out[2] (u64, device; out[0] is zeroed here on the
// stream) = {packed arena length, cut}. The caller reads out back, pads
// the arena to 16 and allocates the new pool before pass 2.
int df_log_evict_plan(const void* tkeys, uint32_t cap, const void* app_off,
                      const void* app_len, const void* row_boff,
                      const void* row_blen, uint64_t first, uint64_t n_rows,
                      uint64_t pool_len, void* reloc, void* out,
                      uint64_t stream) {
    if (cap == 0 || first == 0 || first > n_rows
        || pool_len >= (1ull << 62))
        return -1;
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long),
                                  STREAM(stream));
    if (e != hipSuccess) return (int)e;
    uint32_t blocks = grid_for(cap);
    if (blocks > LOG_SELECT_MAX_BLOCKS) blocks = LOG_SELECT_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log_evict_plan, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), (const uint64_t*)tkeys,
                       (const int64_t*)app_off, (const int32_t*)app_len, cap,
                       (const int64_t*)row_boff, (const int32_t*)row_blen,
                       first, n_rows, (int64_t)pool_len, (int64_t*)reloc,
                       (unsigned long long*)out);
    return (int)hipGetLastError();
}

// Retention, pass 2: names into new_pool[0, arena), app_off in place, the
// seven row columns from row `first` on into new_* (n_keep rows). The
// suffix old_pool[cut, old_len) -> new_pool[arena, ...) is a plain copy and
// the caller's. Returns -1 for a cut or an arena that is not the shape the
// kernels were written for.
int df_log_evict(const void* old_pool, void* new_pool, uint64_t old_len,
                 uint64_t cut, uint64_t arena, uint64_t new_cap,
                 const void* tkeys, uint32_t cap, void* app_off,
                 const void* app_len, const void* reloc,
                 const void* row_time, const void* row_sev,
                 const void* row_agent, const void* row_type,
                 const void* row_app, const void* row_boff,
                 const void* row_blen,
                 void* new_time, void* new_sev, void* new_agent,
                 void* new_type, void* new_app, void* new_boff,
                 void* new_blen, uint64_t first, uint64_t n_keep,
                 uint64_t stream) {
    if (cap == 0 || first == 0 || cut > old_len || (arena & 15)
        || (n_keep && (cut & 15)) || arena + (old_len - cut) > new_cap
        || old_len >= (1ull << 62))
        return -1;
    LogRows src{(int64_t*)row_time, (uint8_t*)row_sev, (uint32_t*)row_agent,
                (uint16_t*)row_type, (uint32_t*)row_app, (int64_t*)row_boff,
                (int32_t*)row_blen};
    LogRows dst{(int64_t*)new_time, (uint8_t*)new_sev, (uint32_t*)new_agent,
                (uint16_t*)new_type, (uint32_t*)new_app, (int64_t*)new_boff,
                (int32_t*)new_blen};
    uint32_t blocks = grid_for((uint64_t)cap + n_keep);
    if (blocks > LOG_SELECT_MAX_BLOCKS) blocks = LOG_SELECT_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log_evict, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), (const uint8_t*)old_pool,
                       (uint8_t*)new_pool, (int64_t)old_len, (int64_t)cut,
                       (int64_t)arena, (const uint64_t*)tkeys,
                       (int64_t*)app_off, (const int32_t*)app_len,
                       (const int64_t*)reloc, cap, src, dst, first, n_keep);
    return (int)hipGetLastError();
}

uint32_t df_log_pattern_prefix() { return LOG_PAT_PREFIX; }
uint32_t df_log_pattern_lds_slots() { return LOG_PAT_LSLOT; }

// K14: fold the rows with flags[r] != 0 into the pattern table (device
// memory, `cap` slots, a power of two: keys u64 and count u64 zeroed,
// first_row u32 = ROW_NONE, last_row u32 = 0, drops one zeroed u64).
// out_key: nullptr, or u64[n_rows] that gets the key of every flagged row.
// Returns -1 for a table, a pool or a row count the kernel does not take.
int df_log_patterns(const void* pool, uint64_t pool_len,
                    const void* body_off, const void* body_len,
                    const void* flags, uint64_t n_rows, void* keys,
                    uint32_t cap, void* count, void* first_row,
                    void* last_row, void* drops, void* out_key,
                    uint64_t stream) {
    if (cap == 0 || (cap & (cap - 1)) || ((uintptr_t)pool & 15)
        || n_rows >= ROW_NONE)
        return -1;
    if (n_rows == 0) return 0;
    PatTable pt{(uint64_t*)keys, (unsigned long long*)count,
                (uint32_t*)first_row, (uint32_t*)last_row,
                (unsigned long long*)drops, cap - 1};
    uint32_t blocks = grid_for(n_rows);
    if (blocks > LOG_SELECT_MAX_BLOCKS) blocks = LOG_SELECT_MAX_BLOCKS;
    hipLaunchKernelGGL(k_log_patterns, dim3(blocks), dim3(BLOCK), 0,
                       STREAM(stream), (const uint8_t*)pool, pool_len,
                       (const int64_t*)body_off, (const int32_t*)body_len,
                       (const uint8_t*)flags, n_rows, pt,
                       (uint64_t*)out_key);
    return (int)hipGetLastError();
}

}  // extern "C"
