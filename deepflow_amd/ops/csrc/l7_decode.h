// K1: AppProtoLogsData protobuf decode, one record per call. The device
// kernel k_decode_l7 (dfgpu.hip) and df_decode_l7_host (decode_host.cpp)
// both call decode_l7_record; ops/ref.py decode_l7_ref is its Python twin.
//
// MALFORMED-RECORD CONTRACT (also ARCHITECTURE.md, "Ingest decode"). The
// records come off the network; for any byte string:
//  - No byte outside [offs[rid], offs[rid]+lens[rid]) influences row rid.
//    One exception: ByteStream loads the aligned 8-byte word that holds a
//    byte, so the allocation must reach the next 8-byte boundary; the extra
//    bytes are loaded and never looked at.
//  - Every string ref that decode emits lies wholly inside that range.
//  - A length-delimited field whose length runs past the end of its
//    enclosing message is ignored, and parsing of that enclosing message
//    ends. The test is `ln > end - pos` in 64 bits (rd_len); pos + ln is
//    never formed first, so nothing wraps.
//  - These also end parsing of the enclosing message, and nothing is
//    stored for the field:
//      * a varint whose last byte inside the message still has the
//        continuation bit set;
//      * a varint of more than 10 bytes;
//      * a wire type of 3, 4, 6 or 7;
//      * a fixed32 or fixed64 field that does not fit.
//  - Everything decoded before that point in the record stays. A message
//    that ended early is over; its parent goes on with the field after it.
//  - The row always exists, so base_row + rid stays aligned, and
//    attr_cnt[row] is always written.
//  - In every message (AppProtoHead included) a well-formed field of wire
//    type 0, 1, 2 or 5 that has no column is skipped by its wire type.
// Values wider than their column truncate (u8/u32 keep the low bits); a
// field number is the low 32 bits of key >> 3.
#pragma once
#include "l7_layout.h"
#include "pb_stream.h"

namespace {

struct L7Cols {
    uint64_t* u64c;       // [L7_U64_N, stride]
    uint32_t* u32c;       // [L7_U32_N, stride]
    uint8_t* u8c;         // [L7_U8_N, stride]
    uint64_t* strc;       // SCRATCH [L7_STR_N, scratch_stride], row = rid
    uint64_t* attrc;      // SCRATCH [2*L7_MAX_ATTRS, scratch_stride]
    uint8_t* attr_cnt;    // [stride] (segment)
    uint64_t stride;
    uint64_t base_row;
    uint64_t scratch_stride;
};

#define W64(c, v) cols.u64c[(uint64_t)(c) * cols.stride + row] = (v)
#define W32(c, v) cols.u32c[(uint64_t)(c) * cols.stride + row] = (uint32_t)(v)
#define W8(c, v)  cols.u8c[(uint64_t)(c) * cols.stride + row] = (uint8_t)(v)
#define WSTR(c, off, len) cols.strc[(uint64_t)(c) * cols.scratch_stride + rid] = STR_REF_PACK(off, len)

DEV void decode_l7_record(ByteStream& bs, uint32_t pos, uint32_t len,
                          uint32_t rid, const L7Cols& cols) {
    uint64_t row = cols.base_row + rid;
    uint32_t end = pos + len;
    uint32_t n_names = 0, n_vals = 0;

    while (pos < end) {
        uint64_t key;
        if (!rd_varint(bs, pos, end, key)) break;
        uint32_t num = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
        if (wt == 0) {
            uint64_t v;
            if (!rd_varint(bs, pos, end, v)) break;
            switch (num) {
                case 9: W32(L7_U32_REQ_LEN, v); break;
                case 10: W32(L7_U32_RESP_LEN, v); break;
                case 17: W8(L7_U8_DIR_SCORE, v); break;
                case 18: W32(L7_U32_FLAGS, v); break;
                case 19: W32(L7_U32_CAP_REQ_BYTE, v); break;
                case 20: W32(L7_U32_CAP_RESP_BYTE, v); break;
                default: break;
            }
        } else if (wt == 2) {
            uint32_t ln;
            if (!rd_len(bs, pos, end, ln)) break;
            uint32_t sub = pos, send = pos + ln;
            pos = send;
            switch (num) {
                case 1: {  // AppProtoLogsBaseInfo
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 0) {
                            uint64_t v;
                            if (!rd_varint(bs, p2, send, v)) break;
                            switch (n2) {
                                case 1: W64(L7_U64_START_TIME, v); break;
                                case 2: W64(L7_U64_END_TIME, v); break;
                                case 3: W64(L7_U64_FLOW_ID, v); break;
                                case 5: W32(L7_U32_VTAP_ID, v); break;
                                case 6: W8(L7_U8_TAP_TYPE, v); break;
                                case 7: W8(L7_U8_IS_IPV6, v); break;
                                case 8: W8(L7_U8_TAP_SIDE, v); break;
                                case 12: W32(L7_U32_IP4_0, v); break;
                                case 13: W32(L7_U32_IP4_1, v); break;
                                case 16: W32(L7_U32_EPC_0, v); break;
                                case 17: W32(L7_U32_EPC_1, v); break;
                                case 18: W32(L7_U32_PORT_0, v); break;
                                case 19: W32(L7_U32_PORT_1, v); break;
                                case 20: W8(L7_U8_PROTOCOL, v); break;
                                case 23: W32(L7_U32_REQ_TCP_SEQ, v); break;
                                case 24: W32(L7_U32_RESP_TCP_SEQ, v); break;
                                case 25: W32(L7_U32_PID_0, v); break;
                                case 26: W32(L7_U32_PID_1, v); break;
                                case 29: W64(L7_U64_SYSCALL_REQ, v); break;
                                case 30: W64(L7_U64_SYSCALL_RESP, v); break;
                                case 35: W32(L7_U32_GPID_0, v); break;
                                case 36: W32(L7_U32_GPID_1, v); break;
                                case 41: W32(L7_U32_POD_0, v); break;
                                case 42: W32(L7_U32_POD_1, v); break;
                                case 43: W32(L7_U32_BIZ_TYPE, v); break;
                                default: break;
                            }
                        } else if (w2 == 2) {
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            uint32_t s3 = p2, e3 = p2 + l3;
                            p2 = e3;
                            if (n2 == 9) {  // AppProtoHead
                                uint32_t p3 = s3;
                                while (p3 < e3) {
                                    uint64_t k3;
                                    if (!rd_varint(bs, p3, e3, k3)) break;
                                    if ((k3 & 7) == 0) {
                                        uint64_t v;
                                        if (!rd_varint(bs, p3, e3, v)) break;
                                        switch ((uint32_t)(k3 >> 3)) {
                                            case 1: W8(L7_U8_L7_PROTOCOL, v); break;
                                            case 2: W8(L7_U8_MSG_TYPE, v); break;
                                            case 5: W64(L7_U64_RRT, v); break;
                                            default: break;
                                        }
                                    } else {
                                        uint32_t w3 = (uint32_t)(k3 & 7);
                                        if (!skip_field(bs, p3, e3, w3)) break;
                                    }
                                }
                            } else if (n2 == 27) {
                                WSTR(L7_STR_PKNAME_0, s3, l3);
                            } else if (n2 == 28) {
                                WSTR(L7_STR_PKNAME_1, s3, l3);
                            } else if (n2 == 14) {   // ip6_src (16 raw bytes,
                                WSTR(L7_STR_IP6_0, s3, l3);  // pooled)
                            } else if (n2 == 15) {   // ip6_dst
                                WSTR(L7_STR_IP6_1, s3, l3);
                            }
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 11: {  // L7Request
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 2) {
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            switch (n2) {
                                case 1: WSTR(L7_STR_REQ_TYPE, p2, l3); break;
                                case 2: WSTR(L7_STR_DOMAIN, p2, l3); break;
                                case 3: WSTR(L7_STR_RESOURCE, p2, l3); break;
                                case 4: WSTR(L7_STR_ENDPOINT, p2, l3); break;
                                default: break;
                            }
                            p2 += l3;
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 12: {  // L7Response
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 0) {
                            uint64_t v;
                            if (!rd_varint(bs, p2, send, v)) break;
                            if (n2 == 1) W8(L7_U8_STATUS, v);
                            else if (n2 == 2) W32(L7_U32_CODE, v);
                        } else if (w2 == 2) {
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            if (n2 == 3) WSTR(L7_STR_EXCEPTION, p2, l3);
                            else if (n2 == 4) WSTR(L7_STR_RESULT, p2, l3);
                            p2 += l3;
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 13: WSTR(L7_STR_VERSION, sub, ln); break;
                case 14: {  // TraceInfo: hex ids transcode to binary
                    // columns (SmartEncoding: a 32-hex trace id stores as
                    // 16 B of u64s, not 48 B of pool+len); non-hex ids
                    // fall back to the pool columns
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 2) {
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            if (n2 == 1) {
                                uint64_t hi, lo;
                                if (l3 == 32 &&
                                    hex_parse64(bs, p2, hi) &&
                                    hex_parse64(bs, p2 + 16, lo)) {
                                    W64(L7_U64_TRACE_HI, hi);
                                    W64(L7_U64_TRACE_LO, lo);
                                } else {
                                    WSTR(L7_STR_TRACE_ID, p2, l3);
                                }
                            } else if (n2 == 2) {
                                uint64_t sv;
                                if (l3 == 16 && hex_parse64(bs, p2, sv)) {
                                    W64(L7_U64_SPAN_ID_B, sv);
                                } else {
                                    WSTR(L7_STR_SPAN_ID, p2, l3);
                                }
                            } else if (n2 == 3) {
                                WSTR(L7_STR_PARENT_SPAN_ID, p2, l3);
                            }
                            p2 += l3;
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 15: {  // ExtendedInfo
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 0) {
                            uint64_t v;
                            if (!rd_varint(bs, p2, send, v)) break;
                            if (n2 == 3) W32(L7_U32_REQUEST_ID, v);
                        } else if (w2 == 2) {
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            switch (n2) {
                                case 1: WSTR(L7_STR_SERVICE_NAME, p2, l3); break;
                                case 4: WSTR(L7_STR_XREQ_0, p2, l3); break;
                                case 6: WSTR(L7_STR_UA, p2, l3); break;
                                case 7: WSTR(L7_STR_REFERER, p2, l3); break;
                                case 10: WSTR(L7_STR_XREQ_1, p2, l3); break;
                                case 16:
                                    if (n_names < L7_MAX_ATTRS)
                                        cols.attrc[(uint64_t)n_names * cols.scratch_stride + rid] =
                                            STR_REF_PACK(p2, l3);
                                    n_names++;
                                    break;
                                case 17:
                                    if (n_vals < L7_MAX_ATTRS)
                                        cols.attrc[(uint64_t)(L7_MAX_ATTRS + n_vals) * cols.scratch_stride + rid] =
                                            STR_REF_PACK(p2, l3);
                                    n_vals++;
                                    break;
                                default: break;
                            }
                            p2 += l3;
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 21: WSTR(L7_STR_BIZ_CODE, sub, ln); break;
                default: break;
            }
        } else {
            if (!skip_field(bs, pos, end, wt)) break;
        }
    }
    uint32_t na = n_names < n_vals ? n_names : n_vals;
    cols.attr_cnt[row] = (uint8_t)(na > L7_MAX_ATTRS ? L7_MAX_ATTRS : na);
}

}  // namespace
