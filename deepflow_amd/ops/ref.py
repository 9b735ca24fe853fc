"""CPU reference implementations of the HIP kernels.

Used (a) by tests on GPU-less machines, (b) as the numerics oracle the GPU
kernels are compared against (tests/test_gpu_pipeline.py), (c) by the
device='cpu' pipeline (multi-process gloo tests). Semantics mirror
ops/csrc/dfgpu.hip exactly, and for the decoders that holds for malformed
records as well: decode_l7_ref and ref_l4.decode_l4_ref implement the
malformed-record contract written at the top of ops/csrc/l7_decode.h and
never raise on any byte string (tests/test_ingest_cases_cpu.py holds the
twins, the host build of the kernel source and by-construction
expectations to each other). Dictionary/table slot ids may differ from a
concurrent GPU run under hash collisions, so cross-checks compare hydrated
strings, not raw slot ids.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from ..store import l7_schema as S
from ..store.dictionary import str_hash_py, domain_seed

M64 = (1 << 64) - 1
_HEXSET = frozenset(b"0123456789abcdefABCDEF")


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & M64


def hex_parse64_py(raw: bytes):
    """Twin of dfhash.h hex_parse64_with: 16 hex chars -> int, else None."""
    if len(raw) != 16 or not all(c in _HEXSET for c in raw):
        return None
    return int(raw, 16)


# ---------------------------------------------------------------- K1 decode

_U64_IDX = {c: i for i, c in enumerate(S.U64_COLS)}
_U32_IDX = {c: i for i, c in enumerate(S.U32_COLS)}
_U8_IDX = {c: i for i, c in enumerate(S.U8_COLS)}
_STR_IDX = {c: i for i, c in enumerate(S.STR_COLS)}

_BASE_U = {
    1: ("u64", "start_time"), 2: ("u64", "end_time"), 3: ("u64", "flow_id"),
    5: ("u32", "vtap_id"), 6: ("u8", "tap_type"), 7: ("u8", "is_ipv6"),
    8: ("u8", "tap_side"), 12: ("u32", "ip4_0"), 13: ("u32", "ip4_1"),
    16: ("u32", "l3_epc_id_0"), 17: ("u32", "l3_epc_id_1"),
    18: ("u32", "client_port"), 19: ("u32", "server_port"),
    20: ("u8", "protocol"), 23: ("u32", "req_tcp_seq"),
    24: ("u32", "resp_tcp_seq"), 25: ("u32", "process_id_0"),
    26: ("u32", "process_id_1"), 29: ("u64", "syscall_trace_id_request"),
    30: ("u64", "syscall_trace_id_response"), 35: ("u32", "gprocess_id_0"),
    36: ("u32", "gprocess_id_1"), 41: ("u32", "pod_id_0"),
    42: ("u32", "pod_id_1"), 43: ("u32", "biz_type"),
}


def _w(seg, fam, col, row, v):
    t = {"u64": seg.u64, "u32": seg.u32, "u8": seg.u8}[fam]
    idx = {"u64": _U64_IDX, "u32": _U32_IDX, "u8": _U8_IDX}[fam][col]
    if fam == "u64":
        t[idx, row] = v & M64 if v < (1 << 63) else (v & M64) - (1 << 64)
    elif fam == "u32":
        v32 = v & 0xFFFFFFFF
        t[idx, row] = v32 if v32 < (1 << 31) else v32 - (1 << 32)
    else:
        t[idx, row] = v & 0xFF


def rd_varint_ref(mv, pos: int, end: int):
    """Twin of pb_stream.h rd_varint -> (value, pos); value is None where
    the message ends inside the varint or the varint exceeds 10 bytes."""
    v = 0
    for sh in range(0, 70, 7):
        if pos >= end:
            break
        b = mv[pos]
        pos += 1
        v |= (b & 0x7F) << sh
        if not b & 0x80:
            return v & M64, pos
    return None, pos


def pb_fields(mv, pos: int, end: int):
    """Walk one message [pos, end) by the malformed-record contract
    (l7_decode.h): yields (num, 0, value, 0) for a varint field and
    (num, 2, start, length) for a length-delimited one, skips well-formed
    fixed32/fixed64 fields, and stops (never raises) where the contract
    ends the message."""
    while pos < end:
        key, pos = rd_varint_ref(mv, pos, end)
        if key is None:
            return
        num, wt = (key >> 3) & 0xFFFFFFFF, key & 7
        if wt == 0:
            v, pos = rd_varint_ref(mv, pos, end)
            if v is None:
                return
            yield num, 0, v, 0
        elif wt == 2:
            ln, pos = rd_varint_ref(mv, pos, end)
            if ln is None or ln > end - pos:
                return
            yield num, 2, pos, ln
            pos += ln
        elif wt == 1 and end - pos >= 8:
            pos += 8
        elif wt == 5 and end - pos >= 4:
            pos += 4
        else:
            return


_TOP_U = {9: ("u32", "request_length"), 10: ("u32", "response_length"),
          17: ("u8", "direction_score"), 18: ("u32", "flags"),
          19: ("u32", "captured_request_byte"),
          20: ("u32", "captured_response_byte")}
_HEAD_U = {1: ("u8", "l7_protocol"), 2: ("u8", "msg_type"), 5: ("u64", "rrt")}
_BASE_S = {27: "process_kname_0", 28: "process_kname_1", 14: "ip6_0",
           15: "ip6_1"}
_TOP_S = {13: "version", 21: "biz_code"}
# sub-message field -> ({varint field: column}, {string field: column})
_SUB = {
    11: ({}, {1: "request_type", 2: "request_domain", 3: "request_resource",
              4: "endpoint"}),
    12: ({1: ("u8", "response_status"), 2: ("u32", "response_code")},
         {3: "exception_desc", 4: "response_result"}),
    14: ({}, {1: "trace_id", 2: "span_id", 3: "parent_span_id"}),
    15: ({3: ("u32", "request_id")},
         {1: "service_name", 4: "x_request_id_0", 6: "http_user_agent",
          7: "http_referer", 10: "x_request_id_1"}),
}


def decode_l7_ref(payload: bytes, offs, lens, seg, base_row: int,
                  sstr=None, sattr=None) -> None:
    """Python twin of l7_decode.h decode_l7_record, malformed input
    included: it follows the contract written there and never raises."""
    mv = memoryview(payload)
    if sstr is None:
        sstr = torch.zeros((S.N_STR, len(offs)), dtype=torch.int64)
        sattr = torch.zeros((2 * S.MAX_ATTRS, len(offs)), dtype=torch.int64)
    seg._last_sstr, seg._last_sattr = sstr, sattr
    for rid in range(len(offs)):
        row = base_row + rid
        pos = int(offs[rid])
        end = pos + int(lens[rid])
        n_names = n_vals = 0

        def wstr(col, off, ln):
            sstr[_STR_IDX[col], rid] = S.str_ref_pack(off, ln)

        for num, wt, a, ln in pb_fields(mv, pos, end):
            if wt == 0:
                if num in _TOP_U:
                    _w(seg, *_TOP_U[num], row, a)
            elif num == 1:  # AppProtoLogsBaseInfo
                for n2, w2, a2, l2 in pb_fields(mv, a, a + ln):
                    if w2 == 0:
                        if n2 in _BASE_U:
                            _w(seg, *_BASE_U[n2], row, a2)
                    elif n2 == 9:  # AppProtoHead
                        for n3, w3, a3, _ in pb_fields(mv, a2, a2 + l2):
                            if w3 == 0 and n3 in _HEAD_U:
                                _w(seg, *_HEAD_U[n3], row, a3)
                    elif n2 in _BASE_S:
                        wstr(_BASE_S[n2], a2, l2)
            elif num in _SUB:
                umap, smap = _SUB[num]
                for n2, w2, a2, l2 in pb_fields(mv, a, a + ln):
                    if w2 == 0:
                        if n2 in umap:
                            _w(seg, *umap[n2], row, a2)
                    elif num == 15 and n2 == 16:
                        if n_names < S.MAX_ATTRS:
                            sattr[n_names, rid] = S.str_ref_pack(a2, l2)
                        n_names += 1
                    elif num == 15 and n2 == 17:
                        if n_vals < S.MAX_ATTRS:
                            sattr[S.MAX_ATTRS + n_vals, rid] = \
                                S.str_ref_pack(a2, l2)
                        n_vals += 1
                    elif num == 14 and n2 == 1 and l2 == 32 and \
                            hex_parse64_py(bytes(mv[a2:a2 + 16])) is not None \
                            and hex_parse64_py(
                                bytes(mv[a2 + 16:a2 + 32])) is not None:
                        # hex trace/span ids -> binary u64 cols (pool
                        # fallback for non-hex forms)
                        _w(seg, "u64", "trace_id_hi", row,
                           hex_parse64_py(bytes(mv[a2:a2 + 16])))
                        _w(seg, "u64", "trace_id_lo", row,
                           hex_parse64_py(bytes(mv[a2 + 16:a2 + 32])))
                    elif num == 14 and n2 == 2 and l2 == 16 and \
                            hex_parse64_py(bytes(mv[a2:a2 + 16])) is not None:
                        _w(seg, "u64", "span_id_b", row,
                           hex_parse64_py(bytes(mv[a2:a2 + 16])))
                    elif n2 in smap:
                        wstr(smap[n2], a2, l2)
            elif num in _TOP_S:
                wstr(_TOP_S[num], a, ln)
        na = min(n_names, n_vals, S.MAX_ATTRS)
        seg.attr_cnt[row] = na


# ------------------------------------------------------------ K2 kg tables

def kg_build_ref(keys: torch.Tensor, vals: torch.Tensor,
                 tkeys: torch.Tensor, tvals: torch.Tensor) -> None:
    cap_mask = tkeys.numel() - 1
    tk = tkeys.numpy()
    tv = tvals.numpy()
    kk = keys.numpy().view(np.uint64)
    vv = vals.numpy()
    for i in range(len(kk)):
        k = int(kk[i])
        if k == 0:
            continue
        slot = mix64(k) & cap_mask
        for _ in range(cap_mask + 1):
            cur = int(tk[slot]) & M64
            if cur == 0 or cur == k:
                tk[slot] = np.int64(np.uint64(k).astype(np.int64)) \
                    if k < (1 << 63) else np.int64(k - (1 << 64))
                tv[slot] = vv[i]
                break
            slot = (slot + 1) & cap_mask



def intern_ref(payload: bytes, refs: torch.Tensor, ref_rows, domains,
               ref_base_row: int, n: int, tkeys: torch.Tensor,
               out_ids: torch.Tensor, out_base_row: int,
               dictionary=None) -> List[Tuple[int, int, bytes]]:
    """Sequential-deterministic intern; returns new (domain, slot, bytes)."""
    cap_mask = tkeys.numel() - 1
    tk = tkeys.numpy()
    new_entries: List[Tuple[int, int, bytes]] = []
    for ci, (rrow, dom) in enumerate(zip(ref_rows, domains)):
        for i in range(n):
            ref = int(refs[rrow, ref_base_row + i].item()) & M64
            ln = ref & 0xFFFF
            off = ref >> 16
            if ln == 0:
                out_ids[ci, out_base_row + i] = -1  # DICT_ID_INVALID as i32
                continue
            sbytes = payload[off:off + ln]
            h = str_hash_py(bytes(sbytes), domain_seed(dom))
            slot = h & cap_mask
            placed = False
            for _ in range(cap_mask + 1):
                cur = int(tk[slot]) & M64
                if cur == 0:
                    tk[slot] = np.int64(h) if h < (1 << 63) \
                        else np.int64(h - (1 << 64))
                    new_entries.append((dom, slot, bytes(sbytes)))
                    placed = True
                    break
                if cur == h:
                    placed = True
                    break
                slot = (slot + 1) & cap_mask
            v = slot if placed else S.DICT_ID_INVALID
            out_ids[ci, out_base_row + i] = v if v < (1 << 31) else v - (1 << 32)
    if dictionary is not None:
        for dom, slot, sbytes in new_entries:
            dictionary.id_to_str[(dom, slot)] = sbytes
            dictionary.str_to_id[(dom, sbytes)] = slot
            dictionary.pending_sync.append((dom, slot, sbytes))
    return new_entries


def intern_attrs_pool_ref(payload: bytes, sattr, seg, base_row: int, n: int,
                          tkeys, dictionary=None):
    """CPU twin of k_intern_attrs with the variable attr-id pool."""
    new_entries = []
    for i in range(n):
        row = base_row + i
        cnt = int(seg.attr_cnt[row].item())
        start = seg.attr_pool_len
        seg.ensure_attr_pool(2 * cnt)
        seg.attr_start[row] = start
        for a in range(cnt):
            for half, dom in ((0, S.DICT_DOM_ATTR_NAME),
                              (1, S.DICT_DOM_ATTR_VALUE)):
                ref = int(sattr[half * S.MAX_ATTRS + a, i].item()) & M64
                ln = ref & 0xFFFF
                off = ref >> 16
                ident = -1
                if ln:
                    sbytes = payload[off:off + ln]
                    h = str_hash_py(bytes(sbytes), domain_seed(dom))
                    cap_mask = tkeys.numel() - 1
                    tk = tkeys.numpy()
                    slot = h & cap_mask
                    for _ in range(cap_mask + 1):
                        cur = int(tk[slot]) & M64
                        if cur == 0:
                            tk[slot] = np.int64(h) if h < (1 << 63) \
                                else np.int64(h - (1 << 64))
                            new_entries.append((dom, slot, bytes(sbytes)))
                            break
                        if cur == h:
                            break
                        slot = (slot + 1) & cap_mask
                    ident = slot if slot < (1 << 31) else slot - (1 << 32)
                seg.attr_pool[start + half * cnt + a] = ident
        seg.attr_pool_len += 2 * cnt
    if dictionary is not None:
        for dom, slot, sbytes in new_entries:
            dictionary.id_to_str[(dom, slot)] = sbytes
            dictionary.str_to_id[(dom, sbytes)] = slot
            dictionary.pending_sync.append((dom, slot, sbytes))
    return new_entries


# -------------------------------------------------------------- K4 pool

def pool_lens_ref(sstr, pool_cols, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.int32)
    for i in range(n):
        total = 0
        for c in pool_cols:
            total += int(sstr[c, i].item()) & 0xFFFF
        out[i] = total
    return out


def pool_gather_ref(payload: bytes, seg, pool_cols, base_row: int, n: int,
                    row_start: torch.Tensor, pool_base: int, sstr) -> None:
    pool = seg.pool.numpy()
    for i in range(n):
        dst0 = pool_base + int(row_start[i].item())
        dst = dst0
        for ci, c in enumerate(pool_cols):
            r = int(sstr[c, i].item()) & M64
            ln = r & 0xFFFF
            off = r >> 16
            pool[dst:dst + ln] = np.frombuffer(payload[off:off + ln],
                                               dtype=np.uint8)
            # u16 bit pattern in the int16 column (l7_schema.py, str_lens)
            seg.str_lens[ci, base_row + i] = ln - (1 << 16) \
                if ln >= (1 << 15) else ln
            dst += ln
        seg.str_rowref[base_row + i] = S.str_ref_pack(dst0, dst - dst0)


# -------------------------------------------------------------- K5 agg

AGG_NVALS = 7  # req, resp, err_c, err_s, rrt_sum, rrt_cnt, rrt_max


