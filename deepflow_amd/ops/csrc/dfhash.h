// Device hash helpers shared by the HIP translation units of libdfgpu.so
// (dfgpu.hip, dfprofile.hip). Internal linkage: each unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef DEV
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

}  // namespace
