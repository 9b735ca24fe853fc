// K1b: TaggedFlow (L4 flow log) protobuf decode, one record per call.
// Wire schema: message/flow_log.proto:14-120; columns: l4_layout.h. The
// device kernel k_decode_l4 (dfgpu.hip) and df_decode_l4_host
// (decode_host.cpp) both call decode_l4_record; ops/ref_l4.py
// decode_l4_ref is its Python twin. Malformed records follow the contract
// at the top of l7_decode.h. Only the first Flow field (TaggedFlow field 1)
// of a record is decoded; a column is written only when its field is on
// the wire.
#pragma once
#include "l4_layout.h"
#include "l7_layout.h"  // STR_REF_PACK
#include "pb_stream.h"

namespace {

struct L4Cols {
    uint64_t* u64c;
    uint32_t* u32c;
    uint8_t* u8c;
    uint64_t* strc;   // SCRATCH [L4_STR_N, scratch_stride], row = rid
    uint64_t stride;
    uint64_t base_row;
    uint64_t scratch_stride;
};

#define L4W64(c, v) cols.u64c[(uint64_t)(c) * cols.stride + row] = (v)
#define L4W32(c, v) cols.u32c[(uint64_t)(c) * cols.stride + row] = (uint32_t)(v)
#define L4W8(c, v)  cols.u8c[(uint64_t)(c) * cols.stride + row] = (uint8_t)(v)

DEV void decode_l4_record(ByteStream& bs, uint32_t pos, uint32_t len,
                          uint32_t rid, const L4Cols& cols) {
    uint64_t row = cols.base_row + rid;
    uint32_t end = pos + len;
    // locate flow submessage (TaggedFlow field 1)
    bool found = false;
    while (pos < end) {
        uint64_t key;
        if (!rd_varint(bs, pos, end, key)) break;
        uint32_t num = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
        if (num == 1 && wt == 2) {
            uint32_t ln;
            if (!rd_len(bs, pos, end, ln)) break;
            end = pos + ln;  // narrow to Flow
            found = true;
            break;
        }
        if (!skip_field(bs, pos, end, wt)) break;
    }
    if (!found) return;
    while (pos < end) {
        uint64_t key;
        if (!rd_varint(bs, pos, end, key)) break;
        uint32_t num = (uint32_t)(key >> 3), wt = (uint32_t)(key & 7);
        if (wt == 0) {
            uint64_t v;
            if (!rd_varint(bs, pos, end, v)) break;
            switch (num) {
                case 5: L4W64(L4_U64_FLOW_ID, v); break;
                case 6: L4W64(L4_U64_START_TIME, v); break;
                case 7: L4W64(L4_U64_END_TIME, v); break;
                case 8: L4W64(L4_U64_DURATION, v); break;
                case 10: L4W32(L4_U32_VLAN, v); break;
                case 11: L4W32(L4_U32_ETH_TYPE, v); break;
                case 14: L4W8(L4_U8_CLOSE_TYPE, v); break;
                case 15: L4W8(L4_U8_SIGNAL_SOURCE, v); break;
                case 16: L4W8(L4_U8_IS_ACTIVE_SERVICE, v); break;
                case 18: L4W8(L4_U8_IS_NEW_FLOW, v); break;
                case 19: L4W8(L4_U8_TAP_SIDE, v); break;
                case 25: L4W8(L4_U8_DIRECTION_SCORE, v); break;
                default: break;
            }
        } else if (wt == 2) {
            uint32_t ln;
            if (!rd_len(bs, pos, end, ln)) break;
            uint32_t sub = pos, send = pos + ln;
            pos = send;
            switch (num) {
                case 1: {  // FlowKey
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 0) {
                            uint64_t v;
                            if (!rd_varint(bs, p2, send, v)) break;
                            switch (n2) {
                                case 1: L4W32(L4_U32_VTAP_ID, v); break;
                                case 2: L4W8(L4_U8_TAP_TYPE, v); break;
                                case 4: L4W64(L4_U64_MAC_SRC, v); break;
                                case 5: L4W64(L4_U64_MAC_DST, v); break;
                                case 6: L4W32(L4_U32_IP4_0, v); break;
                                case 7: L4W32(L4_U32_IP4_1, v); break;
                                case 10: L4W32(L4_U32_PORT_SRC, v); break;
                                case 11: L4W32(L4_U32_PORT_DST, v); break;
                                case 12: L4W8(L4_U8_PROTOCOL, v); break;
                                default: break;
                            }
                        } else if (w2 == 2 && (n2 == 8 || n2 == 9)) {
                            // ip6_src/dst: raw 16 bytes into the str pool
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            cols.strc[(uint64_t)(n2 == 8 ? L4_STR_IP6_0
                                                         : L4_STR_IP6_1) *
                                      cols.scratch_stride + rid] =
                                STR_REF_PACK(p2, l3);
                            p2 += l3;
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 24: {  // acl_gids (packed repeated u32): keep first
                    uint32_t p2 = sub;
                    uint64_t v;
                    if (p2 < send && rd_varint(bs, p2, send, v))
                        L4W32(L4_U32_ACL_GID, v);
                    break;
                }
                case 2: case 3: {  // FlowMetricsPeer src/dst
                    bool tx = num == 2;
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 0) {
                            uint64_t v;
                            if (!rd_varint(bs, p2, send, v)) break;
                            switch (n2) {
                                case 1: L4W64(tx ? L4_U64_BYTE_TX : L4_U64_BYTE_RX, v); break;
                                case 2: L4W64(tx ? L4_U64_L3_BYTE_TX : L4_U64_L3_BYTE_RX, v); break;
                                case 3: L4W64(tx ? L4_U64_L4_BYTE_TX : L4_U64_L4_BYTE_RX, v); break;
                                case 4: L4W64(tx ? L4_U64_PACKET_TX : L4_U64_PACKET_RX, v); break;
                                case 5: L4W64(tx ? L4_U64_TOTAL_BYTE_TX : L4_U64_TOTAL_BYTE_RX, v); break;
                                case 6: L4W64(tx ? L4_U64_TOTAL_PACKET_TX : L4_U64_TOTAL_PACKET_RX, v); break;
                                case 9: L4W32(tx ? L4_U32_TCP_FLAGS_SRC : L4_U32_TCP_FLAGS_DST, v); break;
                                case 10: L4W32(tx ? L4_U32_EPC_0 : L4_U32_EPC_1, v); break;
                                case 20: L4W32(tx ? L4_U32_NAT_REAL_IP_0 : L4_U32_NAT_REAL_IP_1, v); break;
                                case 21: L4W32(tx ? L4_U32_NAT_REAL_PORT_0 : L4_U32_NAT_REAL_PORT_1, v); break;
                                case 22: L4W32(tx ? L4_U32_GPID_0 : L4_U32_GPID_1, v); break;
                                default: break;
                            }
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 13: {  // FlowPerfStats
                    uint32_t p2 = sub;
                    while (p2 < send) {
                        uint64_t k2;
                        if (!rd_varint(bs, p2, send, k2)) break;
                        uint32_t n2 = (uint32_t)(k2 >> 3), w2 = (uint32_t)(k2 & 7);
                        if (w2 == 0) {
                            uint64_t v;
                            if (!rd_varint(bs, p2, send, v)) break;
                            if (n2 == 3) L4W8(L4_U8_L4_PROTOCOL, v);
                            else if (n2 == 4) L4W8(L4_U8_L7_PROTOCOL, v);
                        } else if (w2 == 2) {
                            uint32_t l3;
                            if (!rd_len(bs, p2, send, l3)) break;
                            uint32_t s3 = p2, e3 = p2 + l3;
                            p2 = e3;
                            if (n2 == 1) {  // TCPPerfStats
                                uint32_t p3 = s3;
                                while (p3 < e3) {
                                    uint64_t k3;
                                    if (!rd_varint(bs, p3, e3, k3)) break;
                                    uint32_t n3 = (uint32_t)(k3 >> 3), w3 = (uint32_t)(k3 & 7);
                                    if (w3 == 0) {
                                        uint64_t v;
                                        if (!rd_varint(bs, p3, e3, v)) break;
                                        switch (n3) {
                                            case 3: L4W32(L4_U32_SRT_MAX, v); break;
                                            case 4: L4W32(L4_U32_ART_MAX, v); break;
                                            case 5: L4W32(L4_U32_RTT, v); break;
                                            case 8: L4W32(L4_U32_SRT_SUM, v); break;
                                            case 9: L4W32(L4_U32_ART_SUM, v); break;
                                            case 12: L4W32(L4_U32_SRT_COUNT, v); break;
                                            case 13: L4W32(L4_U32_ART_COUNT, v); break;
                                            case 16: L4W32(L4_U32_RETRANS_TOTAL, v); break;
                                            case 17: L4W32(L4_U32_SYN_COUNT, v); break;
                                            case 18: L4W32(L4_U32_SYNACK_COUNT, v); break;
                                            case 19: L4W32(L4_U32_CIT_MAX, v); break;
                                            case 20: L4W32(L4_U32_CIT_SUM, v); break;
                                            case 21: L4W32(L4_U32_CIT_COUNT, v); break;
                                            default: break;
                                        }
                                    } else if (w3 == 2) {
                                        uint32_t l4b;
                                        if (!rd_len(bs, p3, e3, l4b)) break;
                                        uint32_t s4 = p3, e4 = p3 + l4b;
                                        p3 = e4;
                                        if (n3 == 14 || n3 == 15) {  // TcpPerfCountsPeer
                                            bool ptx = n3 == 14;
                                            uint32_t p4 = s4;
                                            while (p4 < e4) {
                                                uint64_t k4;
                                                if (!rd_varint(bs, p4, e4, k4)) break;
                                                if ((k4 & 7) == 0) {
                                                    uint64_t v;
                                                    if (!rd_varint(bs, p4, e4, v)) break;
                                                    uint32_t n4 = (uint32_t)(k4 >> 3);
                                                    if (n4 == 1) L4W32(ptx ? L4_U32_RETRANS_TX : L4_U32_RETRANS_RX, v);
                                                    else if (n4 == 2) L4W32(ptx ? L4_U32_ZERO_WIN_TX : L4_U32_ZERO_WIN_RX, v);
                                                    else if (n4 == 3) L4W32(ptx ? L4_U32_OOO_TX : L4_U32_OOO_RX, v);
                                                } else {
                                                    uint32_t w4 = (uint32_t)(k4 & 7);
                                                    if (!skip_field(bs, p4, e4, w4)) break;
                                                }
                                            }
                                        }
                                    } else {
                                        if (!skip_field(bs, p3, e3, w3)) break;
                                    }
                                }
                            } else if (n2 == 2) {  // L7PerfStats
                                uint32_t p3 = s3;
                                while (p3 < e3) {
                                    uint64_t k3;
                                    if (!rd_varint(bs, p3, e3, k3)) break;
                                    if ((k3 & 7) == 0) {
                                        uint64_t v;
                                        if (!rd_varint(bs, p3, e3, v)) break;
                                        switch ((uint32_t)(k3 >> 3)) {
                                            case 1: L4W32(L4_U32_L7_REQUEST, v); break;
                                            case 2: L4W32(L4_U32_L7_RESPONSE, v); break;
                                            case 3: L4W32(L4_U32_L7_ERR_CLIENT, v); break;
                                            case 4: L4W32(L4_U32_L7_ERR_SERVER, v); break;
                                            case 5: L4W32(L4_U32_L7_ERR_TIMEOUT, v); break;
                                            case 6: L4W32(L4_U32_L7_RRT_COUNT, v); break;
                                            case 7: L4W64(L4_U64_L7_RRT_SUM, v); break;
                                            case 8: L4W32(L4_U32_L7_RRT_MAX, v); break;
                                            default: break;
                                        }
                                    } else {
                                        uint32_t w3 = (uint32_t)(k3 & 7);
                                        if (!skip_field(bs, p3, e3, w3)) break;
                                    }
                                }
                            }
                        } else {
                            if (!skip_field(bs, p2, send, w2)) break;
                        }
                    }
                    break;
                }
                case 26:
                    cols.strc[(uint64_t)L4_STR_REQUEST_DOMAIN * cols.scratch_stride + rid] =
                        STR_REF_PACK(sub, ln);
                    break;
                default: break;
            }
        } else {
            if (!skip_field(bs, pos, end, wt)) break;
        }
    }
}

}  // namespace
