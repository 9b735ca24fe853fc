// dfprofile — K9: GPU-resident continuous-profiling store and flame fold.
//
// Replaces the host path of ingest/profile_pipeline.py (per-line split,
// dict intern, one dataclass per row; per-row/per-frame tree walk at query
// time) with the same pattern as the rest of the data plane: parse on the
// GPU, intern into a slot-index dictionary, keep columns in HBM, aggregate
// at query time.
//
// Rules: wave = 64 lanes, blocks are multiples of 64; table rules are in
// dftable.h. Particular to this unit:
//  - stack ids and flame-node ids are slot indices of tables probed from
//    `h & mask`. The claimer alone writes the slot's metadata and nobody
//    reads it before the next launch.
//  - 64-bit hash identity is accepted for stacks and for flame nodes
//    exactly as it is for the SmartEncoding dictionary (dfgpu.hip K3): two
//    different byte strings with one 64-bit hash would share an id.
#include "dftable.h"

namespace {

constexpr uint64_t PROF_STACK_SEED = 0x50524F465354414Bull;  // "PROFSTAK"
constexpr uint64_t PROF_FRAME_SEED = 0x50524F464652414Dull;  // "PROFFRAM"
constexpr uint64_t PROF_ROOT_KEY = 0x524F4F54524F4F54ull;    // "ROOTROOT"

DEV bool is_ws(uint8_t c) {  // bytes.strip(): space \t \n \v \f \r
    return c == 32 || (c >= 9 && c <= 13);
}

struct ProfStacks {
    uint64_t* tkeys;          // [cap]
    uint64_t* stack_off;      // [cap] offset into pool
    uint32_t* stack_len;      // [cap]
    uint32_t* stack_frames;   // [cap] number of ';' + 1
    uint8_t* pool;
    unsigned long long* pool_len;   // device-side bump pointer
    unsigned long long* drops;      // lines lost to a full table
    uint64_t pool_cap;
    uint32_t cap_mask;
};

// one thread per folded line
__global__ void k_prof_ingest(const uint8_t* __restrict__ buf,
                              const uint64_t* __restrict__ line_off,
                              const uint32_t* __restrict__ line_len,
                              const uint32_t* __restrict__ line_msg,
                              uint32_t n_lines,
                              const int64_t* __restrict__ msg_ts,
                              const int64_t* __restrict__ msg_count,
                              const uint32_t* __restrict__ msg_series,
                              const uint8_t* __restrict__ msg_parse,
                              ProfStacks st,
                              int64_t* __restrict__ row_ts,
                              int64_t* __restrict__ row_val,
                              uint32_t* __restrict__ row_stack,
                              uint32_t* __restrict__ row_series,
                              uint64_t base_row) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines) return;
    uint32_t m = line_msg[i];
    const uint8_t* s = buf + line_off[i];
    uint32_t len = line_len[i];
    int64_t value = msg_count[m];
    bool skip = false;
    if (msg_parse[m]) {
        while (len && is_ws(s[len - 1])) len--;
        while (len && is_ws(s[0])) { s++; len--; }
        if (len == 0) {
            skip = true;
        } else {
            // rpartition(b" "): walk the trailing digits back to the last
            // space; anything else before a space means "no count"
            uint32_t p = len;
            uint64_t v = 0, scale = 1;
            while (p > 0 && s[p - 1] >= '0' && s[p - 1] <= '9') {
                v += (uint64_t)(s[p - 1] - '0') * scale;
                scale *= 10;
                p--;
            }
            if (p < len && p > 1 && s[p - 1] == ' ') {
                value = (int64_t)v;
                len = p - 1;
            }
        }
    }
    uint64_t row = base_row + i;
    uint32_t sid = DICT_ID_INVALID;
    if (!skip) {
        uint64_t h = str_hash(s, len, PROF_STACK_SEED);
        bool claimed;
        sid = table_claim(st.tkeys, st.cap_mask, h,
                          (uint32_t)(h & st.cap_mask), &claimed);
        if (sid == DICT_ID_INVALID) {
            atomicAdd(st.drops, 1ull);
        } else if (claimed) {
            uint64_t off = atomicAdd(st.pool_len, (unsigned long long)len);
            uint32_t frames = 1;
            if (off + len <= st.pool_cap) {   // host sizes the pool; belt
                uint8_t* d = st.pool + off;
                for (uint32_t b = 0; b < len; b++) {
                    uint8_t c = s[b];
                    d[b] = c;
                    frames += (c == ';');
                }
                st.stack_len[sid] = len;
            } else {
                st.stack_len[sid] = 0;
                off = 0;
            }
            st.stack_off[sid] = off;
            st.stack_frames[sid] = frames;
        }
    }
    row_ts[row] = msg_ts[m];
    row_val[row] = value;
    row_stack[row] = sid;
    row_series[row] = msg_series[m];
}

// one thread per stored row: filtered per-stack sums + grand total
__global__ void k_prof_stack_sums(const int64_t* __restrict__ row_ts,
                                  const int64_t* __restrict__ row_val,
                                  const uint32_t* __restrict__ row_stack,
                                  const uint32_t* __restrict__ row_series,
                                  uint64_t n_rows,
                                  const uint8_t* __restrict__ series_ok,
                                  uint32_t n_series,
                                  int64_t time_start, int64_t time_end,
                                  uint32_t cap,
                                  unsigned long long* __restrict__ sums,
                                  uint8_t* __restrict__ hit,
                                  unsigned long long* __restrict__ total) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = 0;
    if (i < n_rows) {
        uint32_t sid = row_stack[i];
        uint32_t ser = row_series[i];
        int64_t ts = row_ts[i];
        if (sid < cap && ser < n_series && series_ok[ser] &&
            ts >= time_start && ts <= time_end) {
            v = (unsigned long long)row_val[i];
            atomicAdd(&sums[sid], v);
            hit[sid] = 1;   // same value from every writer
        }
    }
    // one atomic per wave for the single total
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
}

struct FlameNodes {
    uint64_t* nkeys;                 // [ncap] chained path key
    uint64_t* nparent;               // [ncap]
    uint32_t* noff;                  // [ncap] frame name offset in pool
    uint32_t* nlen;                  // [ncap]
    uint32_t* ndepth;                // [ncap] 1 = child of root
    unsigned long long* ntotal;      // [ncap]
    unsigned long long* nself;       // [ncap]
    unsigned long long* drops;       // never counts when sized by the host
    uint32_t ncap_mask;
};

// one thread per selected stack slot: walk its frames, probe-or-insert the
// chained path key of every prefix, add the stack's sum along the path
__global__ void k_flame_fold(const uint8_t* __restrict__ hit,
                             const unsigned long long* __restrict__ sums,
                             const uint64_t* __restrict__ stack_off,
                             const uint32_t* __restrict__ stack_len,
                             const uint8_t* __restrict__ pool,
                             uint32_t cap, FlameNodes nd) {
    uint32_t sid = blockIdx.x * blockDim.x + threadIdx.x;
    if (sid >= cap || !hit[sid]) return;
    unsigned long long sum = sums[sid];
    uint64_t base = stack_off[sid];
    uint32_t len = stack_len[sid];
    const uint8_t* s = pool + base;
    uint64_t h = PROF_ROOT_KEY;
    uint32_t depth = 0;
    uint32_t fs = 0;
    // pos == len closes the last frame (empty frames are real frames)
    for (uint32_t pos = 0; pos <= len; pos++) {
        if (pos < len && s[pos] != ';') continue;
        uint32_t flen = pos - fs;
        uint64_t fh = str_hash(s + fs, flen, PROF_FRAME_SEED);
        uint64_t parent = h;
        h = mix64(parent * 0x9e3779b97f4a7c15ull + fh);
        if (h == EMPTY_KEY) h = 1;
        depth++;
        bool claimed;
        uint32_t slot = table_claim(nd.nkeys, nd.ncap_mask, h,
                                    (uint32_t)(h & nd.ncap_mask), &claimed);
        if (slot == DICT_ID_INVALID) {
            atomicAdd(nd.drops, 1ull);
            return;
        }
        if (claimed) {
            nd.nparent[slot] = parent;
            nd.noff[slot] = (uint32_t)(base + fs);
            nd.nlen[slot] = flen;
            nd.ndepth[slot] = depth;
        }
        atomicAdd(&nd.ntotal[slot], sum);
        if (pos == len) atomicAdd(&nd.nself[slot], sum);
        fs = pos + 1;
    }
}

}  // namespace

extern "C" {

uint64_t df_prof_root_key() { return PROF_ROOT_KEY; }
uint64_t df_prof_stack_seed() { return PROF_STACK_SEED; }

int df_prof_ingest(const void* buf, const void* line_off,
                   const void* line_len, const void* line_msg,
                   uint32_t n_lines,
                   const void* msg_ts, const void* msg_count,
                   const void* msg_series, const void* msg_parse,
                   void* tkeys, uint32_t cap, void* stack_off,
                   void* stack_len, void* stack_frames,
                   void* pool, uint64_t pool_cap, void* pool_len,
                   void* drops,
                   void* row_ts, void* row_val, void* row_stack,
                   void* row_series, uint64_t base_row, uint64_t stream) {
    if (n_lines == 0) return 0;
    ProfStacks st{(uint64_t*)tkeys, (uint64_t*)stack_off,
                  (uint32_t*)stack_len, (uint32_t*)stack_frames,
                  (uint8_t*)pool, (unsigned long long*)pool_len,
                  (unsigned long long*)drops, pool_cap, cap - 1};
    hipLaunchKernelGGL(k_prof_ingest, dim3(grid_for(n_lines)), dim3(BLOCK),
                       0, STREAM(stream),
                       (const uint8_t*)buf, (const uint64_t*)line_off,
                       (const uint32_t*)line_len, (const uint32_t*)line_msg,
                       n_lines, (const int64_t*)msg_ts,
                       (const int64_t*)msg_count,
                       (const uint32_t*)msg_series,
                       (const uint8_t*)msg_parse, st,
                       (int64_t*)row_ts, (int64_t*)row_val,
                       (uint32_t*)row_stack, (uint32_t*)row_series,
                       base_row);
    return (int)hipGetLastError();
}

int df_prof_stack_sums(const void* row_ts, const void* row_val,
                       const void* row_stack, const void* row_series,
                       uint64_t n_rows, const void* series_ok,
                       uint32_t n_series, int64_t time_start,
                       int64_t time_end, uint32_t cap, void* sums,
                       void* hit, void* total, uint64_t stream) {
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(k_prof_stack_sums, dim3(grid_for(n_rows)),
                       dim3(BLOCK), 0, STREAM(stream),
                       (const int64_t*)row_ts, (const int64_t*)row_val,
                       (const uint32_t*)row_stack,
                       (const uint32_t*)row_series, n_rows,
                       (const uint8_t*)series_ok, n_series, time_start,
                       time_end, cap, (unsigned long long*)sums,
                       (uint8_t*)hit, (unsigned long long*)total);
    return (int)hipGetLastError();
}

int df_prof_flame_fold(const void* hit, const void* sums,
                       const void* stack_off, const void* stack_len,
                       const void* pool, uint32_t cap,
                       void* nkeys, void* nparent, void* noff, void* nlen,
                       void* ndepth, void* ntotal, void* nself,
                       void* ndrops, uint32_t ncap, uint64_t stream) {
    if (cap == 0) return 0;
    FlameNodes nd{(uint64_t*)nkeys, (uint64_t*)nparent, (uint32_t*)noff,
                  (uint32_t*)nlen, (uint32_t*)ndepth,
                  (unsigned long long*)ntotal, (unsigned long long*)nself,
                  (unsigned long long*)ndrops, ncap - 1};
    hipLaunchKernelGGL(k_flame_fold, dim3(grid_for(cap)), dim3(BLOCK), 0,
                       STREAM(stream),
                       (const uint8_t*)hit,
                       (const unsigned long long*)sums,
                       (const uint64_t*)stack_off,
                       (const uint32_t*)stack_len, (const uint8_t*)pool,
                       cap, nd);
    return (int)hipGetLastError();
}

}  // extern "C"
