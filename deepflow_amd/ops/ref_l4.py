"""CPU reference for the L4 (TaggedFlow) decode.

Python twin of ops/csrc/l4_decode.h decode_l4_record: the same field ->
column tables walked with ref.pb_fields, so it follows the malformed-record
contract (top of l7_decode.h) and never raises on any byte string. Like the
kernel it writes a column only when its field is on the wire and decodes
only the first Flow of a record. The independent check of both is
tests/ingest_cases.py, whose expectations are known by construction.
"""
from __future__ import annotations

from ..store import l4_schema as L4
from ..store import l7_schema as S
from .ref import pb_fields, rd_varint_ref

M64 = (1 << 64) - 1

_U64 = {c: i for i, c in enumerate(L4.U64_COLS)}
_U32 = {c: i for i, c in enumerate(L4.U32_COLS)}
_U8 = {c: i for i, c in enumerate(L4.U8_COLS)}
_STR = {c: i for i, c in enumerate(L4.STR_COLS)}

# varint field number -> column, per message (flow_log.proto)
_FLOW = {5: "flow_id", 6: "start_time", 7: "end_time", 8: "duration",
         10: "vlan", 11: "eth_type", 14: "close_type", 15: "signal_source",
         16: "is_active_service", 18: "is_new_flow", 19: "tap_side",
         25: "direction_score"}
_FLOW_KEY = {1: "vtap_id", 2: "tap_type", 4: "mac_src", 5: "mac_dst",
             6: "ip4_0", 7: "ip4_1", 10: "client_port", 11: "server_port",
             12: "protocol"}
# FlowMetricsPeer: (src column, dst column)
_PEER = {1: ("byte_tx", "byte_rx"), 2: ("l3_byte_tx", "l3_byte_rx"),
         3: ("l4_byte_tx", "l4_byte_rx"), 4: ("packet_tx", "packet_rx"),
         5: ("total_byte_tx", "total_byte_rx"),
         6: ("total_packet_tx", "total_packet_rx"),
         9: ("tcp_flags_bit_0", "tcp_flags_bit_1"),
         10: ("l3_epc_id_0", "l3_epc_id_1"),
         20: ("nat_real_ip_0", "nat_real_ip_1"),
         21: ("nat_real_port_0", "nat_real_port_1"),
         22: ("gprocess_id_0", "gprocess_id_1")}
_PERF = {3: "l4_protocol", 4: "l7_protocol"}
_TCP = {3: "srt_max", 4: "art_max", 5: "rtt", 8: "srt_sum", 9: "art_sum",
        12: "srt_count", 13: "art_count", 16: "retrans_total",
        17: "syn_count", 18: "synack_count", 19: "cit_max", 20: "cit_sum",
        21: "cit_count"}
# TcpPerfCountsPeer: (tx column, rx column)
_TCP_PEER = {1: ("retrans_tx", "retrans_rx"),
             2: ("zero_win_tx", "zero_win_rx"), 3: ("ooo_tx", "ooo_rx")}
_L7PERF = {1: "l7_request", 2: "l7_response", 3: "l7_err_client",
           4: "l7_err_server", 5: "l7_err_timeout", 6: "l7_rrt_count",
           7: "l7_rrt_sum", 8: "l7_rrt_max"}


def _w(seg, row, col, v):
    if col in _U64:
        v &= M64
        seg.u64[_U64[col], row] = v - (1 << 64) if v >= (1 << 63) else v
    elif col in _U32:
        v &= 0xFFFFFFFF
        seg.u32[_U32[col], row] = v - (1 << 32) if v >= (1 << 31) else v
    else:
        seg.u8[_U8[col], row] = v & 0xFF


def _varints(mv, seg, row, pos, end, table, side=None):
    """Store the mapped varint fields of a message without sub-messages."""
    for num, wt, a, _ in pb_fields(mv, pos, end):
        if wt == 0 and num in table:
            col = table[num]
            _w(seg, row, col if side is None else col[side], a)


def decode_l4_ref(payload: bytes, offs, lens, seg, base_row: int,
                  sstr=None) -> None:
    mv = memoryview(payload)
    if sstr is None:
        import torch
        sstr = torch.zeros((L4.N_STR, len(offs)), dtype=torch.int64)
    for rid in range(len(offs)):
        row = base_row + rid
        pos = int(offs[rid])
        end = pos + int(lens[rid])
        flow = None
        for num, wt, a, ln in pb_fields(mv, pos, end):
            if num == 1 and wt == 2:  # first Flow only
                flow = (a, a + ln)
                break
        if flow is None:
            continue
        for num, wt, a, ln in pb_fields(mv, *flow):
            if wt == 0:
                if num in _FLOW:
                    _w(seg, row, _FLOW[num], a)
            elif num == 1:  # FlowKey
                for n2, w2, a2, l2 in pb_fields(mv, a, a + ln):
                    if w2 == 0:
                        if n2 in _FLOW_KEY:
                            _w(seg, row, _FLOW_KEY[n2], a2)
                    elif n2 in (8, 9):  # ip6_src/dst, raw 16 bytes
                        sstr[_STR["ip6_0" if n2 == 8 else "ip6_1"], rid] = \
                            S.str_ref_pack(a2, l2)
            elif num in (2, 3):  # FlowMetricsPeer src/dst
                _varints(mv, seg, row, a, a + ln, _PEER, side=num - 2)
            elif num == 13:  # FlowPerfStats
                for n2, w2, a2, l2 in pb_fields(mv, a, a + ln):
                    if w2 == 0:
                        if n2 in _PERF:
                            _w(seg, row, _PERF[n2], a2)
                    elif n2 == 1:  # TCPPerfStats
                        for n3, w3, a3, l3 in pb_fields(mv, a2, a2 + l2):
                            if w3 == 0:
                                if n3 in _TCP:
                                    _w(seg, row, _TCP[n3], a3)
                            elif n3 in (14, 15):  # TcpPerfCountsPeer tx/rx
                                _varints(mv, seg, row, a3, a3 + l3,
                                         _TCP_PEER, side=n3 - 14)
                    elif n2 == 2:  # L7PerfStats
                        _varints(mv, seg, row, a2, a2 + l2, _L7PERF)
            elif num == 24:  # acl_gids (packed repeated u32): keep first
                v, _ = rd_varint_ref(mv, a, a + ln)
                if v is not None:
                    _w(seg, row, "acl_gid", v)
            elif num == 26:
                sstr[_STR["request_domain"], rid] = S.str_ref_pack(a, ln)
