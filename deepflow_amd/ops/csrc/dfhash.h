// Device hash helpers shared by the HIP translation units of libdfgpu.so
// (dfgpu.hip, dfquery.hip, dfprofile.hip, dftrace.hip, dflog.hip, dfflow.hip), which get
// them through dftable.h and dfseg.h. Internal linkage: each unit gets its
// own copy. DEV is defined here and nowhere else.
//
// DF_HOST_BUILD compiles the same text as plain host C++ (no HIP header):
// libdfcpu.so and the stand-alone fuzz program build the ingest decoders
// that way.
#pragma once
#include <stdint.h>

#ifdef DF_HOST_BUILD
#define DEV inline
#else
#include <hip/hip_runtime.h>
#define DEV __device__ __forceinline__
#endif

namespace {

// xxhash64-flavoured string hash (seeded); only needs to be collision-safe
// at 64 bits, not xxh-compatible.
DEV uint64_t str_hash(const uint8_t* s, uint32_t len, uint64_t seed) {
    uint64_t h = seed ^ 0x27d4eb2f165667c5ull ^ (uint64_t)len * 0x9e3779b97f4a7c15ull;
    uint32_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t k;
        __builtin_memcpy(&k, s + i, 8);
        h ^= k * 0xc2b2ae3d27d4eb4full;
        h = (h << 31) | (h >> 33);
        h *= 0x9e3779b185ebca87ull;
    }
    uint64_t tail = 0;
    for (uint32_t j = 0; i + j < len; j++) tail |= (uint64_t)s[i + j] << (8 * j);
    h ^= tail * 0x165667b19e3779f9ull;
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 29; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 32;
    return h ? h : 1ull;  // never return EMPTY_KEY
}

DEV uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// parse 16 lowercase/uppercase hex chars get(0)..get(15) -> u64; false on
// non-hex. One parser for the decoder (ids on the wire) and the trace-tree
// join (pooled parent ids), so both derive the same key from the same text.
template <typename Get>
DEV bool hex_parse64_with(Get get, uint64_t& out) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < 16; i++) {
        uint8_t c = get(i);
        uint8_t d;
        if (c >= '0' && c <= '9') d = c - '0';
        else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
        else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
        else return false;
        v = (v << 4) | d;
    }
    out = v;
    return true;
}

}  // namespace
