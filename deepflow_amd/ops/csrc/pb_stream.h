// Protobuf wire primitives of the ingest decoders (l7_decode.h,
// l4_decode.h). One source for the device build (dfgpu.hip) and the host
// build (decode_host.cpp, DF_HOST_BUILD): DEV switches in dfhash.h.
//
// Every reader takes the end of the ENCLOSING message and returns false
// where the malformed-record contract (top of l7_decode.h) ends that
// message; the caller breaks out of its field loop and stores nothing.
#pragma once
#include <stdint.h>
#include "dfhash.h"

namespace {

// Word-buffered byte stream: protobuf parsing is byte-granular and
// sequential per record; buffering an aligned u64 per 8 bytes turns 8
// byte-loads into one dwordx2 load. The base must be 8-byte aligned and
// the allocation behind it must reach the next 8-byte boundary after the
// last record: the word that holds the last byte is loaded whole.
struct ByteStream {
    const uint64_t* w;
    uint64_t cur;
    uint32_t wpos;
    DEV void init(const uint8_t* base) {
        w = (const uint64_t*)base;
        wpos = 0xFFFFFFFFu;
        cur = 0;
    }
    DEV uint8_t get(uint32_t i) {
        uint32_t wp = i >> 3;
        if (wp != wpos) {
            wpos = wp;
            cur = w[wp];
        }
        return (uint8_t)(cur >> ((i & 7) * 8));
    }
};

// false: the message ends inside the varint (its last byte still has the
// continuation bit) or the varint is longer than 10 bytes
DEV bool rd_varint(ByteStream& bs, uint32_t& pos, uint32_t end, uint64_t& v) {
    v = 0;
    for (int sh = 0; sh < 70 && pos < end; sh += 7) {
        uint8_t b = bs.get(pos++);
        v |= (uint64_t)(b & 0x7F) << sh;
        if (!(b & 0x80)) return true;
    }
    return false;
}

// length prefix of a length-delimited field; false when the field runs
// past `end`. Compared in 64 bits against the bytes left, never as
// pos + ln, so no length can wrap.
DEV bool rd_len(ByteStream& bs, uint32_t& pos, uint32_t end, uint32_t& ln) {
    uint64_t v;
    if (!rd_varint(bs, pos, end, v) || v > (uint64_t)(end - pos)) return false;
    ln = (uint32_t)v;
    return true;
}

// skip one field the message has no column for, by its wire type
DEV bool skip_field(ByteStream& bs, uint32_t& pos, uint32_t end, uint32_t wt) {
    switch (wt) {
        case 0: { uint64_t v; return rd_varint(bs, pos, end, v); }
        case 1: if (end - pos < 8) return false; pos += 8; return true;
        case 2: {
            uint32_t ln;
            if (!rd_len(bs, pos, end, ln)) return false;
            pos += ln;
            return true;
        }
        case 5: if (end - pos < 4) return false; pos += 4; return true;
        default: return false;  // groups (3, 4) and the unassigned 6, 7
    }
}

// parse 16 hex chars at pos -> u64; false on non-hex (parser: dfhash.h)
DEV bool hex_parse64(ByteStream& bs, uint32_t pos, uint64_t& out) {
    return hex_parse64_with(
        [&](uint32_t i) -> uint8_t { return bs.get(pos + i); }, out);
}

}  // namespace
