// dfdict — K16: pattern match over a tag dictionary's strings.
//
// DF-SQL `tag LIKE 'pat'` / `tag REGEXP 'pat'` on a SmartEncoding tag does
// not look at rows: the pattern is matched once per distinct string of the
// tag's dictionary domain and the result is a bitmap over dictionary ids.
// The row filter (eval_terms in dfquery.hip, OP_INSET / OP_NOT_INSET) is
// then one bit test per row.
//
// The strings live in a device arena (store/dictionary.py DictArena): the
// entries' bytes back to back, nothing between them, and three columns per
// entry: byte offset (u32), length (u16), dictionary id (u32). The pattern
// is the DFA of query/logregex.py, the same tables k_log_regex (dflog.hip)
// walks: state 0 dead, state 1 start, an entry of `next` carries the target
// state in its low 15 bits and "the target accepts" in bit 15.
//
// Rules: wave = 64 lanes, blocks are multiples of 64 (dftable.h).
#include "dftable.h"

namespace {

constexpr uint32_t DICT_RE_TABLE_BYTES = 32 * 1024;  // n_states*n_classes*2
constexpr uint32_t DICT_RE_MAX_CLASSES = 64;
constexpr uint32_t RE_ACCEPT = 1u << 15;
constexpr uint32_t RE_STATE = RE_ACCEPT - 1;
constexpr uint32_t RE_ANCHOR_START = 1, RE_ANCHOR_END = 2,
                   RE_END_BEFORE_NL = 4, RE_NULLABLE = 8;

// LogRegex.search_py on the n bytes at p: try start positions in turn (only
// position 0 with anchor_start). Without anchor_end the shortest accept
// from a start decides; with it the walk runs to the entry's last byte and
// tests the accept bit there, or one byte earlier when that byte is \n and
// `$` allows it. Reads p[0..n) and nothing else.
DEV bool dict_entry_matches(const uint8_t* __restrict__ p, uint32_t n,
                            const uint8_t* cls, const uint16_t* nxt,
                            uint32_t nc, uint32_t flags) {
    const bool a_start = flags & RE_ANCHOR_START;
    const bool a_end = flags & RE_ANCHOR_END;
    const uint32_t nullable = (flags & RE_NULLABLE) ? 1 : 0;
    // the empty match somewhere inside any string
    if (nullable && !(a_start && a_end)) return true;
    if (n == 0) return nullable;
    const uint32_t q_end = a_start ? 1 : n;
    for (uint32_t q = 0; q < q_end; q++) {
        uint32_t st = 1;
        if (!a_end) {
            for (uint32_t i = q; i < n; i++) {
                uint32_t e = nxt[st * nc + cls[p[i]]];
                if (!e) break;
                if (e & RE_ACCEPT) return true;
                st = e;
            }
            continue;
        }
        uint32_t acc = nullable, acc_before = 0;
        bool alive = true;
        for (uint32_t i = q; i < n; i++) {
            if (i == n - 1) acc_before = acc;
            uint32_t e = nxt[st * nc + cls[p[i]]];
            if (!e) { alive = false; break; }
            st = e & RE_STATE;
            acc = e >> 15;
        }
        if (alive && acc) return true;
        if ((flags & RE_END_BEFORE_NL) && acc_before && p[n - 1] == '\n')
            return true;
    }
    return false;
}

// One lane per entry e in [first, n_entries): set bit id[e] of `words` when
// the entry matches (with `complement`: when it does not). The tables are
// staged once per block as dynamic LDS, 256 + n_states * nc * 2 bytes in
// 16-byte chunks, 33024 at the most: of the CU's 160 KiB that leaves four
// workgroups (16 waves) for the largest pattern and eight (the 32 waves a CU
// holds) for tables under 20 KiB. The walk is one byte load and two
// dependent LDS reads per input byte; those waves are what hides them.
//
// Bounds. Global reads: off[e], len[e], id[e] for e < n_entries, and arena
// bytes [off[e], off[e] + len[e]) only; the neighbours' bytes share cache
// lines with them and are never looked at, so `foo$` cannot see a following
// entry's \n and `bc` cannot match across `..ab|cd..`. Table indices are
// state * nc + class with state < n_states and class < nc by construction
// of the tables (LogRegex asserts it), inside the staged blob. Global
// writes: words[id >> 5] for id < n_bits only; an id outside the bitmap is
// skipped.
__global__ __launch_bounds__(BLOCK)
void k_dict_match(const uint8_t* __restrict__ arena,
                  const uint32_t* __restrict__ off,
                  const uint16_t* __restrict__ len,
                  const uint32_t* __restrict__ id,
                  uint32_t first, uint32_t n_entries,
                  const uint4* __restrict__ blob, uint32_t n_states,
                  uint32_t nc, uint32_t flags, uint32_t complement,
                  uint32_t* __restrict__ words, uint32_t n_bits) {
    extern __shared__ uint4 s_blob4[];      // blob_chunks of them
    const uint32_t blob_chunks = (256 + n_states * nc * 2 + 15) / 16;
    for (uint32_t c = threadIdx.x; c < blob_chunks; c += BLOCK)
        s_blob4[c] = blob[c];
    __syncthreads();

    const uint64_t e = (uint64_t)first + (uint64_t)blockIdx.x * BLOCK
                     + threadIdx.x;
    if (e >= n_entries) return;
    const uint8_t* cls = reinterpret_cast<const uint8_t*>(s_blob4);
    const uint16_t* nxt = reinterpret_cast<const uint16_t*>(s_blob4) + 128;
    const bool hit = dict_entry_matches(arena + off[e], len[e], cls, nxt, nc,
                                        flags);
    if (hit == (complement != 0)) return;
    const uint32_t v = id[e];
    if (v < n_bits) atomicOr(&words[v >> 5], 1u << (v & 31));
}

}  // namespace

extern "C" {

// out[0..1]: table bytes, byte classes k_dict_match was built for
void df_dict_re_limits(uint32_t* out) {
    out[0] = DICT_RE_TABLE_BYTES;
    out[1] = DICT_RE_MAX_CLASSES;
}

// table: device memory, 16-byte aligned and padded to a multiple of 16
// bytes: class_of u8[256], next u16[n_states * n_classes] (LogRegex.table()).
// Returns -1 for tables the kernel does not take.
int df_dict_match(const void* arena, const void* off, const void* len,
                  const void* id, uint32_t first, uint32_t n_entries,
                  const void* table, uint32_t n_states, uint32_t n_classes,
                  uint32_t flags, uint32_t complement, void* words,
                  uint32_t n_bits, uint64_t stream) {
    if (n_classes < 1 || n_classes > DICT_RE_MAX_CLASSES || n_states < 2
        || n_states > RE_STATE
        || (uint64_t)n_states * n_classes * 2 > DICT_RE_TABLE_BYTES
        || ((uintptr_t)table & 15))
        return -1;
    if (first >= n_entries) return 0;
    uint32_t lds = (256 + n_states * n_classes * 2 + 15) / 16 * 16;
    hipLaunchKernelGGL(k_dict_match, dim3(grid_for(n_entries - first)),
                       dim3(BLOCK), lds, STREAM(stream),
                       (const uint8_t*)arena, (const uint32_t*)off,
                       (const uint16_t*)len, (const uint32_t*)id, first,
                       n_entries, (const uint4*)table, n_states, n_classes,
                       flags, complement, (uint32_t*)words, n_bits);
    return (int)hipGetLastError();
}

}  // extern "C"
