"""Hand-built protobuf records with expectations known by construction, for
the ingest kernels (k_decode_l7, k_decode_l4, k_pool_*, k_intern_*), shared
by test_ingest_cases_cpu.py and test_ingest_kernels_gpu.py.

A record is a FIELD TREE: a list of nodes
    (num, 0, int)                 varint field
    (num, 1, int) / (num, 5, int) fixed64 / fixed32 field
    (num, 2, bytes)               string / bytes field
    (num, 2, [nodes])             sub-message
    (num, 2, Packed([ints]))      packed repeated varints
    Raw(bytes)                    malformed bytes that END the enclosing message
    BadLen(num, value, length)    a length-delimited field written with a
                                  length that runs past its enclosing message
`encode` turns the tree into bytes (no schema, any order, unknown fields,
broken bytes). `build` walks the same TREE -- never the bytes, ops/ref.py or
a kernel -- with the field -> column tables below (l7_layout.h /
l4_layout.h and the proto field numbers the decoders name) and applies the
malformed-record contract of ops/csrc/l7_decode.h: at a Raw or BadLen node
the enclosing message ends and its later siblings are lost, everything
before stays, the parent goes on.

A malformed case is a well-formed tree plus ONE named mutation.
"""
import copy
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from deepflow_amd.store import l4_schema as L4
from deepflow_amd.store import l7_schema as S

M64 = (1 << 64) - 1
MAX_ATTRS = S.MAX_ATTRS

# sentinels the buffers are pre-filled with, so an unexpected write shows
SENT64, SENT32, SENT8 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A, 0x5A
# scratch refs: length 0 (so pool/intern treat the column as empty, as a
# zeroed scratch would) but an offset no record produces
SENT_REF = 0x7FFFFFF0 << 16
BASE_ROW = 5            # non-zero base_row
PAD_ROWS = 4            # sentinel rows after the batch
PAYLOAD_LEAD = 3        # bytes before the first record


# ------------------------------------------------------------- the tree

@dataclass
class Raw:
    data: bytes


@dataclass
class BadLen:
    num: int
    value: object       # bytes or subtree, written after the bad length
    length: int


@dataclass
class Packed:
    values: List[int]


def varint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def key(num: int, wt: int) -> bytes:
    return varint((num << 3) | wt)


def encode(nodes) -> bytes:
    out = bytearray()
    bad = []            # (position after the length varint, claimed length)
    for nd in nodes:
        if isinstance(nd, Raw):
            out += nd.data
        elif isinstance(nd, BadLen):
            out += key(nd.num, 2) + varint(nd.length)
            bad.append((len(out), nd.length))
            out += _body(nd.value)
        else:
            num, wt, val = nd
            out += key(num, wt)
            if wt == 0:
                out += varint(val)
            elif wt == 1:
                out += val.to_bytes(8, "little")
            elif wt == 5:
                out += val.to_bytes(4, "little")
            else:
                body = _body(val)
                out += varint(len(body)) + body
    for pos, ln in bad:     # the mutation must be malformed by the contract
        assert ln > len(out) - pos, "BadLen does not leave its message"
    return bytes(out)


def _body(val) -> bytes:
    if isinstance(val, (bytes, bytearray)):
        return bytes(val)
    if isinstance(val, Packed):
        return b"".join(varint(v) for v in val.values)
    return encode(val)


# ------------------------------------------- field -> column tables

@dataclass
class Msg:
    name: str
    varints: Dict[int, str] = field(default_factory=dict)
    strings: Dict[int, str] = field(default_factory=dict)
    subs: Dict[int, "Msg"] = field(default_factory=dict)
    packed: Dict[int, str] = field(default_factory=dict)   # keep first


L7_HEAD = Msg("head", {1: "l7_protocol", 2: "msg_type", 5: "rrt"})
L7_BASE = Msg("base", {
    1: "start_time", 2: "end_time", 3: "flow_id", 5: "vtap_id",
    6: "tap_type", 7: "is_ipv6", 8: "tap_side", 12: "ip4_0", 13: "ip4_1",
    16: "l3_epc_id_0", 17: "l3_epc_id_1", 18: "client_port",
    19: "server_port", 20: "protocol", 23: "req_tcp_seq",
    24: "resp_tcp_seq", 25: "process_id_0", 26: "process_id_1",
    29: "syscall_trace_id_request", 30: "syscall_trace_id_response",
    35: "gprocess_id_0", 36: "gprocess_id_1", 41: "pod_id_0",
    42: "pod_id_1", 43: "biz_type"},
    {14: "ip6_0", 15: "ip6_1", 27: "process_kname_0",
     28: "process_kname_1"}, {9: L7_HEAD})
L7_REQ = Msg("req", {}, {1: "request_type", 2: "request_domain",
                         3: "request_resource", 4: "endpoint"})
L7_RESP = Msg("resp", {1: "response_status", 2: "response_code"},
              {3: "exception_desc", 4: "response_result"})
# trace_id / span_id: hex forms go to the binary columns (_walk)
L7_TRACE = Msg("trace", {}, {1: "trace_id", 2: "span_id",
                             3: "parent_span_id"})
# 16 / 17: attribute names / values (_walk)
L7_EXT = Msg("ext", {3: "request_id"},
             {1: "service_name", 4: "x_request_id_0", 6: "http_user_agent",
              7: "http_referer", 10: "x_request_id_1"})
L7_TOP = Msg("l7", {9: "request_length", 10: "response_length",
                    17: "direction_score", 18: "flags",
                    19: "captured_request_byte",
                    20: "captured_response_byte"},
             {13: "version", 21: "biz_code"},
             {1: L7_BASE, 11: L7_REQ, 12: L7_RESP, 14: L7_TRACE,
              15: L7_EXT})


def _peer(side: int) -> Msg:
    s, d = ("tx", "0") if side == 0 else ("rx", "1")
    return Msg(f"peer{side}", {
        1: f"byte_{s}", 2: f"l3_byte_{s}", 3: f"l4_byte_{s}",
        4: f"packet_{s}", 5: f"total_byte_{s}", 6: f"total_packet_{s}",
        9: f"tcp_flags_bit_{d}", 10: f"l3_epc_id_{d}",
        20: f"nat_real_ip_{d}", 21: f"nat_real_port_{d}",
        22: f"gprocess_id_{d}"})


def _tcp_peer(s: str) -> Msg:
    return Msg(f"tcp_peer_{s}", {1: f"retrans_{s}", 2: f"zero_win_{s}",
                                 3: f"ooo_{s}"})


L4_TCP = Msg("tcp", {3: "srt_max", 4: "art_max", 5: "rtt", 8: "srt_sum",
                     9: "art_sum", 12: "srt_count", 13: "art_count",
                     16: "retrans_total", 17: "syn_count",
                     18: "synack_count", 19: "cit_max", 20: "cit_sum",
                     21: "cit_count"}, {},
             {14: _tcp_peer("tx"), 15: _tcp_peer("rx")})
L4_L7PERF = Msg("l7perf", {1: "l7_request", 2: "l7_response",
                           3: "l7_err_client", 4: "l7_err_server",
                           5: "l7_err_timeout", 6: "l7_rrt_count",
                           7: "l7_rrt_sum", 8: "l7_rrt_max"})
L4_PERF = Msg("perf", {3: "l4_protocol", 4: "l7_protocol"}, {},
              {1: L4_TCP, 2: L4_L7PERF})
L4_KEY = Msg("flow_key", {1: "vtap_id", 2: "tap_type", 4: "mac_src",
                          5: "mac_dst", 6: "ip4_0", 7: "ip4_1",
                          10: "client_port", 11: "server_port",
                          12: "protocol"}, {8: "ip6_0", 9: "ip6_1"})
L4_FLOW = Msg("flow", {5: "flow_id", 6: "start_time", 7: "end_time",
                       8: "duration", 10: "vlan", 11: "eth_type",
                       14: "close_type", 15: "signal_source",
                       16: "is_active_service", 18: "is_new_flow",
                       19: "tap_side", 25: "direction_score"},
              {26: "request_domain"},
              {1: L4_KEY, 2: _peer(0), 3: _peer(1), 13: L4_PERF},
              {24: "acl_gid"})
# TaggedFlow: only the FIRST field 1 is the Flow that gets decoded
L4_TOP = Msg("tagged_flow", {}, {}, {1: L4_FLOW})

SCHEMA = {"l7": S, "l4": L4}
TOP = {"l7": L7_TOP, "l4": L4_TOP}
HEX = b"0123456789abcdefABCDEF"


def col_bits(kind: str, col: str) -> int:
    sch = SCHEMA[kind]
    return 64 if col in sch.U64_COLS else 32 if col in sch.U32_COLS else 8


# ------------------------------------------------------ expectations

@dataclass
class Exp:
    cols: Dict[str, int] = field(default_factory=dict)
    strs: Dict[str, bytes] = field(default_factory=dict)
    names: List[bytes] = field(default_factory=list)
    vals: List[bytes] = field(default_factory=list)

    @property
    def attr_cnt(self) -> int:
        return min(len(self.names), len(self.vals), MAX_ATTRS)

    @property
    def attrs(self):
        return list(zip(self.names, self.vals))[:MAX_ATTRS]


def _is_hex(b: bytes) -> bool:
    return all(c in HEX for c in b)


def _walk(kind: str, nodes, msg: Msg, exp: Exp) -> None:
    for nd in nodes:
        if isinstance(nd, (Raw, BadLen)):
            return                      # the enclosing message ends here
        num, wt, val = nd
        if wt == 0:
            col = msg.varints.get(num)
            if col:
                exp.cols[col] = val & ((1 << col_bits(kind, col)) - 1)
        elif wt == 2:
            if isinstance(val, list):
                if num in msg.subs:
                    _walk(kind, val, msg.subs[num], exp)
                    if msg is L4_TOP:
                        return          # first Flow only
            elif isinstance(val, Packed):
                if num in msg.packed and val.values:
                    exp.cols[msg.packed[num]] = val.values[0] & 0xFFFFFFFF
            elif msg is L7_EXT and num == 16:
                exp.names.append(val)
            elif msg is L7_EXT and num == 17:
                exp.vals.append(val)
            elif msg is L7_TRACE and num == 1 and len(val) == 32 \
                    and _is_hex(val):
                exp.cols["trace_id_hi"] = int(val[:16], 16)
                exp.cols["trace_id_lo"] = int(val[16:], 16)
            elif msg is L7_TRACE and num == 2 and len(val) == 16 \
                    and _is_hex(val):
                exp.cols["span_id_b"] = int(val, 16)
            elif num in msg.strings:
                exp.strs[msg.strings[num]] = val
        # fixed32 / fixed64 fields map to no column


@dataclass
class Case:
    name: str
    kind: str                   # "l7" | "l4"
    tree: list
    malformed: bool = False
    cut: Optional[tuple] = None  # (top-level node index, bytes kept of it)


def build(case: Case):
    """-> (record bytes, Exp)."""
    if case.cut is None:
        exp = Exp()
        _walk(case.kind, case.tree, TOP[case.kind], exp)
        return encode(case.tree), exp
    # record cut short inside top-level node `idx`: that field no longer
    # fits the record, so it is lost with everything after it
    idx, keep = case.cut
    parts = [encode([nd]) for nd in case.tree]
    assert 0 < keep < len(parts[idx])
    exp = Exp()
    _walk(case.kind, case.tree[:idx], TOP[case.kind], exp)
    return b"".join(parts[:idx]) + parts[idx][:keep], exp


# ---------------------------------------------------------- the trees

def full_msg(kind: str, msg: Msg, v: int, how: str = "mixed") -> list:
    """Every mapped field of `msg`, ascending; values differ per variant v.
    how: "mixed" distinct values, "max" every column's maximum, "zero"
    explicit zeros, "big" 10-byte varints (truncate into the column)."""
    nodes = {}
    for num, col in msg.varints.items():
        bits = col_bits(kind, col)
        if how == "max":
            val = (1 << bits) - 1
        elif how == "zero":
            val = 0
        elif how == "big":
            val = (M64 << 20 | (num * 37 + v)) & M64 | (1 << 63)
        else:
            val = (num * 2654435761 + v * 97 + len(msg.name)) \
                % ((1 << (bits - 1)) - 1) + 1
        nodes[num] = (num, 0, val)
    for num, col in msg.strings.items():
        nodes[num] = (num, 2, f"{col}:{v}:{msg.name}".encode())
    for num, sub in msg.subs.items():
        nodes[num] = (num, 2, full_msg(kind, sub, v, how))
    for num in msg.packed:
        nodes[num] = (num, 2, Packed([7 + v, 8, 9]))
    if msg is L7_TRACE:
        nodes[1] = (1, 2, b"%032x" % (0x0123456789abcdef0fedcba987654321 + v))
        nodes[2] = (2, 2, b"%016x" % (0xfeedface12345678 + v))
    out = [nodes[k] for k in sorted(nodes)]
    if msg is L7_EXT:
        for a in range(3):
            out.append((16, 2, b"attr.name.%d" % a))
        for a in range(3):
            out.append((17, 2, b"value-%d-%d" % (a, v)))
    return out


def full(kind: str, v: int, how: str = "mixed") -> list:
    return full_msg(kind, TOP[kind], v, how)


UNKNOWN = [(99, 0, 1234567), (98, 1, 0x1122334455667788),
           (97, 2, b"unknown bytes"), (96, 5, 0xCAFEF00D)]


def sub(tree, *path):
    """The node list of the sub-message reached by field numbers `path`."""
    for num in path:
        tree = next(nd[2] for nd in tree
                    if isinstance(nd, tuple) and nd[0] == num
                    and isinstance(nd[2], list))
    return tree


def with_unknown(kind: str, v: int) -> list:
    """Unknown fields of wire types 0, 1, 2, 5 before the mapped fields of
    EVERY message (in AppProtoHead that puts them before rrt)."""
    def rec(nodes):
        return UNKNOWN + [(n[0], 2, rec(n[2])) if isinstance(n[2], list)
                          else n for n in nodes]
    return rec(full(kind, v))


def reverse_all(nodes) -> list:
    return [(n[0], 2, reverse_all(n[2])) if isinstance(n[2], list) else n
            for n in reversed(nodes)]


def mutate(tree, path, fn) -> list:
    t = copy.deepcopy(tree)
    fn(sub(t, *path))
    return t


def bad_last(nodes, delta=1):
    """Rewrite the message's last field with a length `delta` too long.
    Sub-messages are moved last first, so the field's end is its
    enclosing message's end."""
    num, wt, val = nodes.pop()
    assert wt == 2
    nodes.append(BadLen(num, val, len(_body(val)) + delta))


def to_end(nodes, num):
    i = next(i for i, n in enumerate(nodes)
             if isinstance(n, tuple) and n[0] == num)
    nodes.append(nodes.pop(i))


# L7 message paths by level; L4 by level down to TcpPerfCountsPeer
L7_PATHS = [(), (1,), (1, 9), (15,)]
L4_PATHS = [(), (1,), (1, 1), (1, 13), (1, 13, 1), (1, 13, 1, 14)]
PATHS = {"l7": L7_PATHS, "l4": L4_PATHS}


def _string_cases() -> List[Case]:
    out = []
    for n in (1, 255, 32767, 32768, 65535):
        body = bytes((i * 31 + n) % 251 + 1 for i in range(n))
        t = full("l7", 2)
        # pooled column (http_user_agent) and dictionary column (endpoint)
        e = sub(t, 15)
        e[[x[0] for x in e].index(6)] = (6, 2, body)
        r = sub(t, 11)
        r[[x[0] for x in r].index(4)] = (4, 2, body[::-1])
        out.append(Case(f"l7_str_{n}", "l7", t))
    # pooled total of one row above 65535
    t = full("l7", 3)
    e = sub(t, 15)
    e[[x[0] for x in e].index(6)] = (6, 2, b"U" * 40000)
    e[[x[0] for x in e].index(7)] = (7, 2, b"R" * 30000)
    out.append(Case("l7_row_pool_over_64k", "l7", t))
    return out


def _trace(trace=None, span=None) -> list:
    t = [(1, 2, [(1, 0, 1_700_000_000_000_000_001)])]
    ids = []
    if trace is not None:
        ids.append((1, 2, trace))
    if span is not None:
        ids.append((2, 2, span))
    return t + [(14, 2, ids)]


def _attrs(names, vals) -> list:
    return [(15, 2, [(16, 2, n) for n in names] + [(17, 2, x) for x in vals])]


def well_formed() -> List[Case]:
    c: List[Case] = []
    for kind in ("l7", "l4"):
        c += [
            Case(f"{kind}_empty", kind, []),
            Case(f"{kind}_full_a", kind, full(kind, 0)),
            Case(f"{kind}_full_b", kind, full(kind, 1)),
            Case(f"{kind}_max", kind, full(kind, 0, "max")),
            Case(f"{kind}_varint10_truncates", kind, full(kind, 0, "big")),
            Case(f"{kind}_explicit_zero", kind, full(kind, 0, "zero")),
            Case(f"{kind}_reversed", kind, reverse_all(full(kind, 4))),
            Case(f"{kind}_unknown_fields", kind, with_unknown(kind, 5)),
        ]
        # a field repeated: the last one wins (every message level)
        t = full(kind, 6)
        for p in PATHS[kind][1:]:
            m = sub(t, *p)
            first = next(n for n in m if n[1] == 0)
            m.append((first[0], 0, first[2] + 1))
        c.append(Case(f"{kind}_repeated_last_wins", kind, t))
    c.append(Case("l7_base_only", "l7",
                  [(1, 2, full_msg("l7", L7_BASE, 7))]))
    c.append(Case("l4_flow_only_key", "l4",
                  [(1, 2, [(1, 2, full_msg("l4", L4_KEY, 7))])]))
    # a length-delimited field of length 0: message, string, attribute
    c.append(Case("l7_len0", "l7",
                  [(1, 2, []), (13, 2, b""), (11, 2, [(1, 2, b"")]),
                   (14, 2, [(1, 2, b""), (2, 2, b"")]), (9, 0, 77)]))
    c.append(Case("l4_len0", "l4",
                  [(1, 2, [(1, 2, []), (26, 2, b""), (24, 2, Packed([])),
                           (5, 0, 99)])]))
    hx = b"0123456789abcdef"
    ids = {
        "hex32_lower": (hx + hx[::-1], None),
        "hex32_upper": ((hx + hx[::-1]).upper(), None),
        "nonhex_first_half": (b"0123g56789abcdef" + hx, None),
        "nonhex_second_half": (hx + b"0123456789abcdeg", None),
        "len31": ((hx + hx)[:31], None),
        "len33": (hx + hx + b"0", None),
        "span_hex16": (None, b"00FFeeddCCbbaa99"),
        "span_nonhex16": (None, b"0123456789abcdex"),
        "span_len15": (None, hx[:15]),
    }
    for name, (tr, sp) in ids.items():
        c.append(Case(f"l7_id_{name}", "l7", _trace(tr, sp)))
    nm = [b"k%02d" % i for i in range(MAX_ATTRS + 1)]
    vl = [b"v%02d" % i for i in range(MAX_ATTRS + 1)]
    c += [
        Case("l7_attrs_0", "l7", _attrs([], [])),
        Case("l7_attrs_max", "l7", _attrs(nm[:-1], vl[:-1])),
        Case("l7_attrs_max_plus_1", "l7", _attrs(nm, vl)),
        Case("l7_attrs_more_names", "l7", _attrs(nm[:5], vl[:2])),
        Case("l7_attrs_more_values", "l7", _attrs(nm[:2], vl[:5])),
        Case("l7_attrs_empty_name", "l7", _attrs([b"", b"n1"], [b"x", b"y"])),
        Case("l7_attrs_empty_value", "l7", _attrs([b"n0", b"n1"], [b"", b"y"])),
    ]
    v6a, v6b = bytes(range(1, 17)), bytes(range(0xF0, 0x100))
    c.append(Case("l7_ip6", "l7", [(1, 2, [(7, 0, 1), (14, 2, v6a),
                                           (15, 2, v6b), (5, 0, 9)])]))
    c.append(Case("l4_ip6", "l4", [(1, 2, [(1, 2, [(8, 2, v6a), (9, 2, v6b),
                                                   (1, 0, 9)])])]))
    c += _string_cases()
    # L4: Flow not first in TaggedFlow; a second Flow is not decoded
    c.append(Case("l4_flow_not_first", "l4",
                  UNKNOWN + full("l4", 8) + [(1, 2, full_msg("l4", L4_FLOW, 9))]))
    c.append(Case("l4_acl_gids_empty", "l4",
                  [(1, 2, [(24, 2, Packed([])), (5, 0, 3)])]))
    c.append(Case("l4_acl_gids_several", "l4",
                  [(1, 2, [(24, 2, Packed([300, 2, 1 << 33 | 5])),
                           (5, 0, 3)])]))
    c.append(Case("l4_both_peers", "l4",
                  [(1, 2, [(3, 2, full_msg("l4", _peer(1), 2)),
                           (2, 2, full_msg("l4", _peer(0), 3))])]))
    return c


def malformed() -> List[Case]:
    c: List[Case] = []
    for kind in ("l7", "l4"):
        base = full(kind, 0)
        for lvl, p in enumerate(PATHS[kind]):
            tag = f"{kind}_lvl{lvl}"

            def mid(fn_node, name):
                # the broken bytes go in the middle of message `p`: what
                # follows them in that message is lost
                def fn(m):
                    m.insert(len(m) // 2, fn_node)
                c.append(Case(f"{tag}_{name}", kind, mutate(base, p, fn),
                              True))
            mid(BadLen(97, b"abc", 0x7FFFFFFF), "len_0x7fffffff")
            mid(BadLen(97, b"abc", 0xFFFFFFF0), "len_0xfffffff0")
            mid(Raw(key(5, 0) + b"\xff" * 10 + b"\x01"), "varint_11_bytes")
            mid(Raw(key(99, 3)), "wire_type_3")
            mid(Raw(key(5, 7)), "wire_type_7")
            # at the end of message `p`: 3 bytes where a fixed64 needs 8,
            # 2 where a fixed32 needs 4, a varint whose last byte continues
            for name, raw in (("fixed64_3_left", key(99, 1) + b"\1\2\3"),
                              ("fixed32_2_left", key(99, 5) + b"\1\2"),
                              ("varint_cut", key(5, 0) + b"\xff\xff"),
                              ("key_cut", b"\xf8")):
                c.append(Case(f"{tag}_{name}", kind,
                              mutate(base, p, lambda m, r=raw: m.append(Raw(r))),
                              True))
        # a nested length one byte too long, at each level below the top:
        # chain the enclosing messages last so the field reaches exactly
        # the record's end plus one
        for depth in range(1, len(PATHS[kind][-1]) + 1 if kind == "l4" else 3):
            p = (PATHS["l4"][-1] if kind == "l4" else (1, 9))[:depth]
            t = copy.deepcopy(base)
            for i in range(depth):
                to_end(sub(t, *p[:i]), p[i])
            bad_last(sub(t, *p[:-1]))
            c.append(Case(f"{kind}_len_plus_1_depth{depth}", kind, t, True))
        # ... and a string one byte too long inside a message that is not
        # last: it ends that message only
        if kind == "l7":
            t = mutate(base, (11,), bad_last)
            c.append(Case("l7_req_string_len_plus_1", "l7", t, True))
    # L4: the Flow length longer than the record
    t = [BadLen(1, full_msg("l4", L4_FLOW, 0), 5000)]
    c.append(Case("l4_flow_len_past_record", "l4", t, True))
    # the record cut in the middle of a varint, of a key, and of a string
    base = full("l7", 0)
    idx = {n[0]: i for i, n in enumerate(base)}
    assert len(encode([base[idx[9]]])) >= 4 and len(key(17, 0)) == 2
    c += [
        Case("l7_cut_in_varint", "l7", base, True, (idx[9], 2)),
        Case("l7_cut_in_key", "l7", base, True, (idx[17], 1)),
        Case("l7_cut_in_string", "l7", base, True, (idx[13], 5)),
        Case("l7_cut_in_base", "l7", base, True, (idx[1], 40)),
        Case("l4_cut_in_flow", "l4", full("l4", 0), True, (0, 60)),
    ]
    return c


# ------------------------------------------------------------ batches

BATCH_SIZES = (1, 63, 64, 65, 257)


@dataclass
class Batch:
    kind: str
    names: List[str]
    payload: bytes          # records back to back after PAYLOAD_LEAD bytes
    offs: np.ndarray        # uint32
    lens: np.ndarray        # uint32
    exps: List[Exp]

    @property
    def n(self) -> int:
        return len(self.exps)

    @property
    def stride(self) -> int:    # scratch stride, larger than n
        return self.n + 7


_BUILT: Dict[str, tuple] = {}


def _built(case: Case):
    if case.name not in _BUILT:
        _BUILT[case.name] = build(case)
    return _BUILT[case.name]


def cases(kind: str, include_malformed: bool = True) -> List[Case]:
    out = [x for x in well_formed() if x.kind == kind]
    if include_malformed:
        out += [x for x in malformed() if x.kind == kind]
    return out


def batch(kind: str, n: int, include_malformed: bool = True,
          small_only: bool = False) -> Batch:
    """n records in a fixed shuffled order. Every malformed record is
    followed by a well-formed one whose values differ from its own (the
    full record of another variant), so bleed between records shows."""
    follower = Case(f"{kind}_follower", kind, full(kind, 11))
    units = []
    for x in cases(kind, include_malformed):
        if small_only and len(_built(x)[0]) > 4096:
            continue
        units.append([x, follower] if x.malformed else [x])
    random.Random(20240607).shuffle(units)
    seq: List[Case] = []
    if n == 1:
        seq = [Case(f"{kind}_full_a", kind, full(kind, 0))]
    i = 0
    while len(seq) < n:
        seq += units[i % len(units)]
        i += 1
    seq = seq[:n]
    if seq[-1].malformed:
        seq[-1] = follower
    return make_batch(kind, seq)


def make_batch(kind: str, seq: List[Case]) -> Batch:
    recs = [_built(x) for x in seq]
    lead = PAYLOAD_LEAD
    if (lead + sum(len(r) for r, _ in recs)) % 8 == 0:
        lead += 1       # the total length must not be a multiple of 8
    payload = bytearray(b"\xff" * lead)
    offs, lens = [], []
    for r, _ in recs:
        offs.append(len(payload))
        lens.append(len(r))
        payload += r
    assert len(payload) % 8 != 0
    return Batch(kind, [x.name for x in seq], bytes(payload),
                 np.array(offs, dtype=np.uint32),
                 np.array(lens, dtype=np.uint32), [e for _, e in recs])


# --------------------------------------------- buffers and the checks

def make_segment(kind: str, n: int, device: str = "cpu"):
    """Segment of n + BASE_ROW + PAD_ROWS rows, every fixed column and
    attr_cnt pre-filled with the sentinels."""
    from deepflow_amd.store.segment import L4Segment, L7Segment
    cap = BASE_ROW + n + PAD_ROWS
    seg = (L7Segment if kind == "l7" else L4Segment)(
        cap, device=device, pool_capacity=1 << 16)
    seg.u64.fill_(SENT64)
    seg.u32.fill_(SENT32)
    seg.u8.fill_(SENT8)
    if kind == "l7":
        seg.attr_cnt.fill_(SENT8)
    return seg


def make_scratch(kind: str, b: Batch, device: str = "cpu"):
    sch = SCHEMA[kind]
    sstr = torch.full((sch.N_STR, b.stride), SENT_REF, dtype=torch.int64,
                      device=device)
    sattr = torch.full((2 * MAX_ATTRS, b.stride), SENT_REF,
                       dtype=torch.int64, device=device) \
        if kind == "l7" else None
    return sstr, sattr


def payload_tensor(b: Batch, tail: int = 0, device: str = "cpu"):
    """The payload as a uint8 tensor whose allocation reaches the next
    8-byte boundary (ByteStream's word loads), plus `tail` zero bytes."""
    size = (len(b.payload) + 7) // 8 * 8 + tail
    t = torch.zeros(size, dtype=torch.uint8)
    t[:len(b.payload)] = torch.frombuffer(bytearray(b.payload),
                                          dtype=torch.uint8)
    return t.to(device)


def _signed(v: int, bits: int) -> int:
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def _check_ref(b: Batch, rid: int, ref: int, want: bytes, what: str):
    off, ln = ref >> 16, ref & 0xFFFF
    lo, hi = int(b.offs[rid]), int(b.offs[rid]) + int(b.lens[rid])
    assert lo <= off and off + ln <= hi, \
        f"{what}: ref [{off}, {off + ln}) leaves record [{lo}, {hi})"
    assert ln == min(len(want), 0xFFFF), f"{what}: len {ln}"
    assert b.payload[off:off + ln] == want[:0xFFFF], f"{what}: bytes"


def check_decode(b: Batch, seg, sstr, sattr) -> None:
    """Everything decode writes (CPU tensors) against the expectations:
    fixed columns, scratch refs, attr_cnt, and sentinels everywhere else."""
    sch = SCHEMA[b.kind]
    fams = ((seg.u64, sch.U64_COLS, 64, SENT64), (seg.u32, sch.U32_COLS, 32, SENT32),
            (seg.u8, sch.U8_COLS, 8, SENT8))
    n = b.n
    for t, names, bits, sent in fams:
        a = t.cpu().numpy()
        s = _signed(sent, bits) if bits > 8 else sent
        assert (a[:, :BASE_ROW] == s).all() and \
            (a[:, BASE_ROW + n:] == s).all(), "rows outside the batch written"
        for rid, e in enumerate(b.exps):
            for ci, col in enumerate(names):
                want = e.cols.get(col)
                want = s if want is None else \
                    (_signed(want, bits) if bits > 8 else want)
                got = int(a[ci, BASE_ROW + rid])
                assert got == want, \
                    f"rec {rid} {b.names[rid]}: {col} = {got:#x}, want {want:#x}"
    ss = sstr.cpu().numpy()
    assert (ss[:, n:] == SENT_REF).all(), "scratch columns past n written"
    for rid, e in enumerate(b.exps):
        for ci, col in enumerate(sch.STR_COLS):
            what = f"rec {rid} {b.names[rid]}: {col}"
            if col in e.strs:
                _check_ref(b, rid, int(ss[ci, rid]), e.strs[col], what)
            else:
                assert int(ss[ci, rid]) == SENT_REF, f"{what}: unexpected ref"
    if b.kind != "l7":
        return
    sa = sattr.cpu().numpy()
    assert (sa[:, n:] == SENT_REF).all()
    cnt = seg.attr_cnt.cpu().numpy()
    assert (cnt[:BASE_ROW] == SENT8).all() and (cnt[BASE_ROW + n:] == SENT8).all()
    for rid, e in enumerate(b.exps):
        what = f"rec {rid} {b.names[rid]}"
        assert int(cnt[BASE_ROW + rid]) == e.attr_cnt, f"{what}: attr_cnt"
        for half, lst in ((0, e.names), (1, e.vals)):
            for a in range(MAX_ATTRS):
                r = int(sa[half * MAX_ATTRS + a, rid])
                if a < len(lst):
                    _check_ref(b, rid, r, lst[a], f"{what}: attr {half}/{a}")
                else:
                    assert r == SENT_REF, f"{what}: attr slot {half}/{a}"


def pool_cols(kind: str) -> List[int]:
    return list(S.POOL_COLS) if kind == "l7" else list(range(L4.N_STR))


def expected_pool(b: Batch):
    """Per row: (bytes of the pooled columns in gather order, their
    lengths). A column holds at most 65535 bytes (the ref's length field)."""
    sch = SCHEMA[b.kind]
    rows = []
    for e in b.exps:
        parts = [e.strs.get(sch.STR_COLS[c], b"")[:0xFFFF]
                 for c in pool_cols(b.kind)]
        rows.append((b"".join(parts), [len(p) for p in parts]))
    return rows


def check_pool(b: Batch, row_len, pool, pool_base: int, pool_sent: int,
               str_lens, str_rowref) -> None:
    """pool_lens + pool_gather outputs (CPU tensors) against expectation.
    str_lens holds each length's u16 bit pattern in its int16 column; the
    row ref packs (offset, min(total, 65535))."""
    rows = expected_pool(b)
    rl = row_len.cpu().numpy()
    pl = pool.cpu().numpy()
    sl = str_lens.cpu().numpy().view(np.uint16)
    rr = str_rowref.cpu().numpy()
    pos = pool_base
    assert (pl[:pool_base] == pool_sent).all(), "pool written before base"
    for rid, (data, lens_) in enumerate(rows):
        assert int(rl[rid]) == len(data), f"rec {rid}: row_len"
        assert pl[pos:pos + len(data)].tobytes() == data, \
            f"rec {rid} {b.names[rid]}: pool bytes"
        assert [int(x) for x in sl[:, BASE_ROW + rid]] == lens_, \
            f"rec {rid} {b.names[rid]}: str_lens"
        assert int(rr[BASE_ROW + rid]) == \
            (pos << 16 | min(len(data), 0xFFFF)), f"rec {rid}: str_rowref"
        pos += len(data)
    assert (pl[pos:] == pool_sent).all(), "pool written past the last row"
    assert (sl[:, :BASE_ROW] == 0).all() and \
        (sl[:, BASE_ROW + b.n:] == 0).all(), "str_lens outside the batch"
    assert (rr[:BASE_ROW] == 0).all() and (rr[BASE_ROW + b.n:] == 0).all()


def check_ids(b: Batch, seg, out, by_slot, fill: int = 12345) -> None:
    """Dictionary ids hydrate to the expected strings (compared through
    the slot -> bytes map, never by raw slot id)."""
    assert (out[:, :BASE_ROW] == fill).all()
    assert (out[:, BASE_ROW + b.n:] == fill).all()
    start = seg.attr_start.cpu().numpy()
    pool = seg.attr_pool.cpu().numpy()
    for rid, e in enumerate(b.exps):
        row = BASE_ROW + rid
        for ci, (col, _, dom) in enumerate(S.DID_COLS):
            want = e.strs.get(col, b"")[:0xFFFF]
            got = int(out[ci, row])
            if want:
                assert by_slot[(dom, got)] == want, (rid, col)
            else:
                assert got == -1, (rid, col)
        s, cnt = int(start[row]), e.attr_cnt
        for a, (nm, vl) in enumerate(e.attrs):
            for half, dom, want in ((0, S.DICT_DOM_ATTR_NAME, nm),
                                    (1, S.DICT_DOM_ATTR_VALUE, vl)):
                got = int(pool[s + half * cnt + a])
                if want:
                    assert by_slot[(dom, got)] == want[:0xFFFF], (rid, a)
                else:
                    assert got == -1, (rid, a)
