"""Tensor-level wrappers over the HIP C API (libdfgpu.so).

Every function takes torch tensors already resident on the GPU, launches
asynchronously on the current torch CUDA stream, and raises on HIP errors.
There is deliberately NO eager/PyTorch fallback here: on a GPU box these are
the only code paths (see ops/ref.py for the CPU reference used by tests and
by the device='cpu' pipeline).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import native


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def decode_l7(payload: torch.Tensor, offs: torch.Tensor, lens: torch.Tensor,
              seg, base_row: int, scratch_str: torch.Tensor,
              scratch_attr: torch.Tensor) -> None:
    """k_decode_l7. Contract on `payload`: its base is 8-byte aligned and
    the allocation behind it reaches the next 8-byte boundary after the
    last record -- the kernel loads the aligned 8-byte word that holds a
    byte (ByteStream, pb_stream.h), so up to 7 bytes past the tensor's
    nominal end are loaded and never looked at. The caching allocator
    rounds every block to 512 bytes, which satisfies this for a whole
    tensor; a view that ends inside a larger allocation does too.
    Malformed records: contract at the top of csrc/l7_decode.h."""
    assert payload.data_ptr() % 8 == 0, "payload must be 8-byte aligned"
    n = offs.numel()
    lib = native.gpu()
    native.check(lib.df_decode_l7(
        payload.data_ptr(), offs.data_ptr(), lens.data_ptr(), n,
        seg.u64.data_ptr(), seg.u32.data_ptr(), seg.u8.data_ptr(),
        scratch_str.data_ptr(), scratch_attr.data_ptr(),
        seg.attr_cnt.data_ptr(),
        seg.capacity, base_row, scratch_str.shape[1], _stream()),
        "df_decode_l7")


def decode_l4(payload: torch.Tensor, offs: torch.Tensor, lens: torch.Tensor,
              seg, base_row: int, scratch_str: torch.Tensor) -> None:
    """k_decode_l4. Same contract on `payload` as decode_l7: 8-byte aligned
    base, allocation reaching the next 8-byte boundary."""
    assert payload.data_ptr() % 8 == 0, "payload must be 8-byte aligned"
    n = offs.numel()
    lib = native.gpu()
    native.check(lib.df_decode_l4(
        payload.data_ptr(), offs.data_ptr(), lens.data_ptr(), n,
        seg.u64.data_ptr(), seg.u32.data_ptr(), seg.u8.data_ptr(),
        scratch_str.data_ptr(), seg.capacity, base_row,
        scratch_str.shape[1], _stream()), "df_decode_l4")


def rollup_family(seg, base_row: int, n: int, time_base_s: int, tables,
                  stream: int = 0) -> None:
    """ONE fused launch updates every table of a family (k_rollup_l4/l7
    iterate the per-table key specs over a single pass of the row)."""
    lib = native.gpu()
    src = tables[0].td.source
    fn = lib.df_rollup_l4 if src == "l4" else lib.df_rollup_l7
    specs = b"".join(t.spec_bytes() for t in tables)
    ptrs = np.array([x for t in tables
                     for x in (t.tkeys.data_ptr(), t.traw.data_ptr(),
                               t.tvals.data_ptr(), t.drops.data_ptr())],
                    dtype=np.uint64)
    caps = np.array([t.capacity for t in tables], dtype=np.uint32)
    native.check(fn(
        seg.u64.data_ptr(), seg.u32.data_ptr(), seg.u8.data_ptr(),
        seg.capacity, base_row, n, time_base_s, specs, len(tables),
        ptrs.ctypes.data, caps.ctypes.data,
        stream or _stream()), "df_rollup_family")


def rollup_insert(kws: torch.Tensor, vals: torch.Tensor, ops: torch.Tensor,
                  table, stream: int = 0) -> None:
    lib = native.gpu()
    native.check(lib.df_rollup_insert(
        kws.data_ptr(), vals.data_ptr(), ops.data_ptr(),
        kws.shape[0], kws.shape[1], vals.shape[1],
        table.tkeys.data_ptr(), table.traw.data_ptr(),
        table.tvals.data_ptr(), table.capacity, table.drops.data_ptr(),
        stream or _stream()), "df_rollup_insert")


def rollup_drain(table, out_keys: torch.Tensor, out_vals: torch.Tensor,
                 hdr: torch.Tensor, stream: int = 0) -> None:
    """Pack the table's occupied slots into out_keys [cap, nw] / out_vals
    [cap, nv] and reset the table, all on the stream. hdr: i64[2], zeroed
    by the caller; receives (rows written, drops). No host sync."""
    lib = native.gpu()
    native.check(lib.df_rollup_drain(
        table.tkeys.data_ptr(), table.traw.data_ptr(),
        table.tvals.data_ptr(), table.drops.data_ptr(),
        table.capacity, table.nw, table.nv,
        out_keys.data_ptr(), out_vals.data_ptr(), hdr.data_ptr(),
        stream or _stream()), "df_rollup_drain")


def sort_u64(data: torch.Tensor) -> None:
    """In-place rocPRIM radix sort of a device int64 tensor (values
    treated as u64)."""
    lib = native.gpu()
    n = data.numel()
    if n == 0:
        return
    alt = torch.empty_like(data)
    nbytes = ctypes.c_uint64(0)
    native.check(lib.df_sort_u64(data.data_ptr(), alt.data_ptr(), n, None,
                                 ctypes.byref(nbytes), _stream()),
                 "df_sort_u64(size)")
    temp = torch.empty(int(nbytes.value), dtype=torch.uint8,
                       device=data.device)
    native.check(lib.df_sort_u64(data.data_ptr(), alt.data_ptr(), n,
                                 temp.data_ptr(), ctypes.byref(nbytes),
                                 _stream()), "df_sort_u64")


def gather_records(payload: torch.Tensor, offs: torch.Tensor,
                   lens: torch.Tensor, sel: torch.Tensor,
                   dst_off: torch.Tensor, out: torch.Tensor) -> None:
    """Pack selected records contiguously (shard-routing all-to-all)."""
    lib = native.gpu()
    native.check(lib.df_gather_records(
        payload.data_ptr(), offs.data_ptr(), lens.data_ptr(),
        sel.data_ptr(), dst_off.data_ptr(), sel.numel(), out.data_ptr(),
        _stream()), "df_gather_records")


def kg_build(keys: torch.Tensor, vals: torch.Tensor, tkeys: torch.Tensor,
             tvals: torch.Tensor) -> None:
    lib = native.gpu()
    native.check(lib.df_kg_build(
        keys.data_ptr(), vals.data_ptr(), keys.numel(),
        tkeys.data_ptr(), tvals.data_ptr(), tkeys.numel(), _stream()),
        "df_kg_build")


def intern_many(payload: torch.Tensor, refs: torch.Tensor,
                ref_rows: torch.Tensor, domains: torch.Tensor,
                ref_base_row: int, n: int,
                tkeys: torch.Tensor, emit: torch.Tensor,
                emit_ctr: torch.Tensor, out_ids: torch.Tensor,
                out_base_row: int) -> None:
    C = domains.numel()
    lib = native.gpu()
    native.check(lib.df_intern_many(
        payload.data_ptr(), refs.data_ptr(), ref_rows.data_ptr(),
        domains.data_ptr(), C, n, refs.shape[1], ref_base_row,
        tkeys.data_ptr(), tkeys.numel(),
        emit.data_ptr(), emit_ctr.data_ptr(), emit.shape[0],
        out_ids.data_ptr(), out_ids.shape[1], out_base_row, _stream()),
        "df_intern_many")


def intern_attrs(payload: torch.Tensor, seg, base_row: int, n: int,
                 tkeys: torch.Tensor, emit: torch.Tensor,
                 emit_ctr: torch.Tensor, scratch_attr: torch.Tensor,
                 attr_start: torch.Tensor) -> None:
    lib = native.gpu()
    native.check(lib.df_intern_attrs(
        payload.data_ptr(), scratch_attr.data_ptr(), seg.attr_cnt.data_ptr(),
        n, seg.capacity, base_row, scratch_attr.shape[1],
        tkeys.data_ptr(), tkeys.numel(),
        emit.data_ptr(), emit_ctr.data_ptr(), emit.shape[0],
        attr_start.data_ptr(), seg.attr_pool.data_ptr(), _stream()),
        "df_intern_attrs")


def pool_lens(scratch_str: torch.Tensor, pool_cols: torch.Tensor, n: int,
              row_len: torch.Tensor) -> None:
    lib = native.gpu()
    native.check(lib.df_pool_lens(
        scratch_str.data_ptr(), pool_cols.data_ptr(), pool_cols.numel(), n,
        scratch_str.shape[1], 0, row_len.data_ptr(), _stream()),
        "df_pool_lens")


def pool_gather(payload: torch.Tensor, seg, pool_cols: torch.Tensor,
                base_row: int, n: int, row_start: torch.Tensor,
                pool: torch.Tensor, pool_base: int,
                scratch_str: torch.Tensor) -> None:
    lib = native.gpu()
    native.check(lib.df_pool_gather(
        payload.data_ptr(), scratch_str.data_ptr(), pool_cols.data_ptr(),
        pool_cols.numel(), n, scratch_str.shape[1], 0, row_start.data_ptr(),
        pool.data_ptr(), pool_base,
        seg.str_rowref.data_ptr(), seg.str_lens.data_ptr(),
        seg.capacity, base_row, _stream()),
        "df_pool_gather")


class SegViewC(ctypes.Structure):
    """Host mirror of dfseg.h's SegView, member for member
    (tests/test_query_kernels_gpu.py holds it against df_seg_view_size /
    df_seg_view_offsets)."""
    _fields_ = [(m, ctypes.c_void_p) for m in
                ("u64c", "u32c", "u8c", "didc", "kg_tk", "kg_tv")] + \
               [("kg_mask", ctypes.c_uint32)] + \
               [(m, ctypes.c_void_p) for m in
                ("attr_pool", "attr_start", "attr_cnt", "str_rowref",
                 "str_lens", "pool")] + \
               [("stride", ctypes.c_uint64), ("n_rows", ctypes.c_uint64)]


def seg_view(seg, kg=None) -> SegViewC:
    """The segment, and the KnowledgeGraph table of the query-time join, as
    every entry point that reads one takes it. A tensor the segment does
    not have stays null. The library reads the struct during the call, so
    it only has to live that long."""
    def ptr(attr):
        t = getattr(seg, attr, None)
        return t.data_ptr() if t is not None else None
    v = SegViewC(u64c=ptr("u64"), u32c=ptr("u32"), u8c=ptr("u8"),
                 didc=ptr("did"), attr_pool=ptr("attr_pool"),
                 attr_start=ptr("attr_start"), attr_cnt=ptr("attr_cnt"),
                 str_rowref=ptr("str_rowref"), str_lens=ptr("str_lens"),
                 pool=ptr("pool"), stride=seg.capacity, n_rows=seg.n_rows)
    if kg is not None:
        v.kg_tk, v.kg_tv = kg.tkeys.data_ptr(), kg.tvals.data_ptr()
        v.kg_mask = max(kg.tkeys.numel() - 1, 0)
    return v


def query_agg(seg, spec_bytes: bytes, base_row: int, n: int,
              gkeys: torch.Tensor, graw: torch.Tensor,
              gvals: torch.Tensor, kg=None, *,
              overflow: torch.Tensor) -> None:
    """overflow: u32[1] device counter (caller zeroes it): rows whose group
    found no free slot in the group table. They are left out of every
    reported group, so a non-zero count means 'rerun with a larger
    table'."""
    lib = native.gpu()
    native.check(lib.df_query_agg(
        ctypes.byref(seg_view(seg, kg)), spec_bytes, n, base_row,
        gkeys.data_ptr(), graw.data_ptr(), gvals.data_ptr(), gkeys.numel(),
        overflow.data_ptr(), _stream()), "df_query_agg")


def query_uniq(seg, spec_bytes: bytes, uniq_bytes: bytes, base_row: int,
               n: int, gkeys: torch.Tensor, graw: torch.Tensor,
               guniq: torch.Tensor, pkeys: torch.Tensor, kg=None, *,
               overflow: torch.Tensor, use_filter: bool = True) -> None:
    """K15 distinct counts of rows [base_row, base_row + n) into
    guniq[cap, QMAX_UNIQ] (u64, caller zeroes it), slot-aligned with the
    gkeys/graw group table of query_agg. pkeys: the query-scoped table of
    seen (group, value tuple) pair hashes, u64[power of two], zeroed once
    and shared by every segment's launch. overflow: u32[2] device counters
    (caller zeroes them): [0] pairs whose group found no slot, [1] pairs
    that found no slot in pkeys; non-zero means 'rerun with fresh, larger
    tables'."""
    from ..query.spec import QMAX_KEYS, QMAX_UNIQ
    lib = native.gpu()
    assert base_row + n <= seg.capacity
    cap = gkeys.numel()
    assert graw.numel() == cap * QMAX_KEYS and overflow.numel() >= 2
    assert guniq.numel() == cap * QMAX_UNIQ
    native.check(lib.df_query_uniq(
        ctypes.byref(seg_view(seg, kg)), spec_bytes, uniq_bytes,
        n, base_row, gkeys.data_ptr(), graw.data_ptr(), gkeys.numel(),
        guniq.data_ptr(), pkeys.data_ptr(), pkeys.numel(),
        overflow.data_ptr(), 1 if use_filter else 0, _stream()),
        "df_query_uniq")


def qpart_agg(seg, spec_bytes: bytes, base_row: int, n: int,
              counts: torch.Tensor, cursors: torch.Tensor,
              row_scratch: torch.Tensor,
              gkeys: torch.Tensor, graw: torch.Tensor,
              gvals: torch.Tensor, kg=None, *,
              overflow: torch.Tensor) -> None:
    """Radix-partitioned group-by (high key cardinality): bucket rows by
    8 hash bits, aggregate one bucket per workgroup set — each block's
    LDS table then holds every key it sees (no per-row global atomics).
    counts/cursors: u32[256] (counts zeroed); row_scratch:
    u64[n * (n_keys+n_aggs)] payload staging; overflow: as in query_agg."""
    lib = native.gpu()
    native.check(lib.df_qpart_agg(
        ctypes.byref(seg_view(seg, kg)), spec_bytes, n, base_row,
        counts.data_ptr(), cursors.data_ptr(), row_scratch.data_ptr(),
        gkeys.data_ptr(), graw.data_ptr(), gvals.data_ptr(),
        gkeys.numel(), overflow.data_ptr(), _stream()), "df_qpart_agg")


def query_select(seg, spec_bytes: bytes, base_row: int, n: int,
                 out_rows: torch.Tensor, out_ctr: torch.Tensor,
                 kg=None) -> None:
    lib = native.gpu()
    native.check(lib.df_query_select(
        ctypes.byref(seg_view(seg, kg)), spec_bytes, n, base_row,
        out_rows.data_ptr(), out_ctr.data_ptr(), out_rows.numel(), _stream()),
        "df_query_select")


# ----------------------------------------------------------------------
# K16: LIKE / REGEXP on dictionary tags (dfdict.hip). `arena` is a
# store.dictionary.DictArena on the GPU.
# ----------------------------------------------------------------------

def query_set_ops():
    """(OP_INSET, OP_NOT_INSET) as eval_terms was built with."""
    out = (ctypes.c_uint32 * 2)()
    native.gpu().df_query_set_ops(out)
    return int(out[0]), int(out[1])


def dict_re_limits():
    """(table bytes, byte classes) k_dict_match was built for;
    query/logregex.py carries the same two."""
    out = (ctypes.c_uint32 * 2)()
    native.gpu().df_dict_re_limits(out)
    return int(out[0]), int(out[1])


def dict_regex_table(rx, device) -> torch.Tensor:
    """rx's tables on `device`, padded to the 16-byte chunks the kernel
    stages them in."""
    table = rx.table()
    blob = np.zeros((table.nbytes + 15) & ~15, dtype=np.uint8)
    blob[:table.nbytes] = table
    return torch.from_numpy(blob).to(device)


def dict_match(arena, rx, words: torch.Tensor, n_bits: int, *,
               first: int = 0, n_entries: int = None,
               complement: bool = False,
               table: torch.Tensor = None) -> None:
    """Set bit id of `words` (u32 bitmap of n_bits bits, caller zeroes it)
    for every arena entry in [first, n_entries) that rx (a
    query.logregex.LogRegex) matches, or with `complement` for every entry
    it does not match. Ids outside the bitmap are skipped."""
    n_entries = arena.n if n_entries is None else n_entries
    assert 0 <= first and n_entries <= arena.n
    assert words.dtype == torch.int32 and n_bits <= words.numel() * 32
    if table is None:
        table = dict_regex_table(rx, words.device)
    native.check(native.gpu().df_dict_match(
        arena.data.data_ptr(), arena.off.data_ptr(), arena.lens.data_ptr(),
        arena.ids.data_ptr(), first, n_entries, table.data_ptr(),
        rx.n_states, rx.n_classes, rx.flags, 1 if complement else 0,
        words.data_ptr(), n_bits, _stream()), "df_dict_match")


# ----------------------------------------------------------------------
# K9: profile store ingest + flame fold (dfprofile.hip). `st` is a
# store.profile_store.GpuProfileStore (owns every tensor named here).
# ----------------------------------------------------------------------

def prof_ingest(buf: torch.Tensor, line_off: torch.Tensor,
                line_len: torch.Tensor, line_msg: torch.Tensor,
                msg_ts: torch.Tensor, msg_count: torch.Tensor,
                msg_series: torch.Tensor, msg_parse: torch.Tensor,
                st, base_row: int) -> None:
    lib = native.gpu()
    native.check(lib.df_prof_ingest(
        buf.data_ptr(), line_off.data_ptr(), line_len.data_ptr(),
        line_msg.data_ptr(), line_off.numel(),
        msg_ts.data_ptr(), msg_count.data_ptr(), msg_series.data_ptr(),
        msg_parse.data_ptr(),
        st.tkeys.data_ptr(), st.tkeys.numel(), st.stack_off.data_ptr(),
        st.stack_len.data_ptr(), st.stack_frames.data_ptr(),
        st.pool.data_ptr(), st.pool.numel(), st.pool_len.data_ptr(),
        st.drops.data_ptr(),
        st.row_ts.data_ptr(), st.row_val.data_ptr(),
        st.row_stack.data_ptr(), st.row_series.data_ptr(), base_row,
        _stream()), "df_prof_ingest")


def prof_stack_sums(st, n_rows: int, series_ok: torch.Tensor,
                    time_start: int, time_end: int, sums: torch.Tensor,
                    hit: torch.Tensor, total: torch.Tensor) -> None:
    lib = native.gpu()
    native.check(lib.df_prof_stack_sums(
        st.row_ts.data_ptr(), st.row_val.data_ptr(),
        st.row_stack.data_ptr(), st.row_series.data_ptr(), n_rows,
        series_ok.data_ptr(), series_ok.numel(), time_start, time_end,
        sums.numel(), sums.data_ptr(), hit.data_ptr(), total.data_ptr(),
        _stream()), "df_prof_stack_sums")


def prof_flame_fold(st, hit: torch.Tensor, sums: torch.Tensor,
                    nkeys: torch.Tensor, nparent: torch.Tensor,
                    noff: torch.Tensor, nlen: torch.Tensor,
                    ndepth: torch.Tensor, ntotal: torch.Tensor,
                    nself: torch.Tensor, ndrops: torch.Tensor) -> None:
    lib = native.gpu()
    native.check(lib.df_prof_flame_fold(
        hit.data_ptr(), sums.data_ptr(), st.stack_off.data_ptr(),
        st.stack_len.data_ptr(), st.pool.data_ptr(), sums.numel(),
        nkeys.data_ptr(), nparent.data_ptr(), noff.data_ptr(),
        nlen.data_ptr(), ndepth.data_ptr(), ntotal.data_ptr(),
        nself.data_ptr(), ndrops.data_ptr(), nkeys.numel(), _stream()),
        "df_prof_flame_fold")


# ----------------------------------------------------------------------
# K10: trace-tree assembly + service trace map (dftrace.hip). `ws` is a
# query.tracemap._GpuWorkspace (owns every tensor named here; ws.flat_ptrs
# is a host u64 array of the flat-column pointers in TraceFlat order).
# ----------------------------------------------------------------------

def trace_extract(seg, base_row: int, time_start: int, time_end: int,
                  ws) -> None:
    lib = native.gpu()
    native.check(lib.df_trace_extract(
        ctypes.byref(seg_view(seg)), base_row, time_start, time_end,
        ws.flat_ptrs.ctypes.data, ws.idx_keys.data_ptr(),
        ws.idx_rows.data_ptr(), ws.drops.data_ptr(), ws.idx_cap,
        _stream()), "df_trace_extract")


def trace_link(ws) -> None:
    lib = native.gpu()
    native.check(lib.df_trace_link(
        ws.flat_ptrs.ctypes.data, ws.idx_keys.data_ptr(),
        ws.idx_rows.data_ptr(), ws.idx_cap, ws.n, ws.parent.data_ptr(),
        ws.kind.data_ptr(), _stream()), "df_trace_link")


def trace_depth(ws) -> None:
    lib = native.gpu()
    native.check(lib.df_trace_depth(
        ws.tkey.data_ptr(), ws.parent.data_ptr(), ws.n,
        ws.depth.data_ptr(), _stream()), "df_trace_depth")


def trace_fold(ws) -> None:
    lib = native.gpu()
    native.check(lib.df_trace_fold(
        ws.flat_ptrs.ctypes.data, ws.parent.data_ptr(), ws.kind.data_ptr(),
        ws.depth.data_ptr(), ws.n, ws.tkeys.data_ptr(), ws.tvals.data_ptr(),
        ws.tkeys.numel(), ws.ekeys.data_ptr(), ws.evals.data_ptr(),
        ws.ekeys.numel(), ws.drops.data_ptr(), _stream()), "df_trace_fold")


# ----------------------------------------------------------------------
# K12: flow groups (dfflow.hip). `ws` is a query.flowgroups._FlowWorkspace
# (owns every tensor named here; ws.flat_ptrs is a host u64 array of the
# flat-column pointers in FlowFlat order).
# ----------------------------------------------------------------------

def flow_extract(seg, base_row: int, time_start: int, time_end: int,
                 ws) -> None:
    lib = native.gpu()
    native.check(lib.df_flow_extract(
        ctypes.byref(seg_view(seg)), base_row, time_start, time_end,
        ws.flat_ptrs.ctypes.data,
        ws.idx_keys.data_ptr(), ws.idx_rows.data_ptr(),
        ws.drops.data_ptr(), ws.idx_cap, _stream()), "df_flow_extract")


def flow_index(ws) -> None:
    """Index inserts from flat columns already in `ws` (what flow_extract
    does per segment row); for callers that filled the columns themselves."""
    lib = native.gpu()
    native.check(lib.df_flow_index(
        ws.flat_ptrs.ctypes.data, ws.idx_keys.data_ptr(),
        ws.idx_rows.data_ptr(), ws.drops.data_ptr(), ws.idx_cap, ws.n,
        _stream()), "df_flow_index")


def flow_union(ws) -> None:
    lib = native.gpu()
    native.check(lib.df_flow_union(
        ws.flat_ptrs.ctypes.data, ws.idx_keys.data_ptr(),
        ws.idx_rows.data_ptr(), ws.idx_cap, ws.n, ws.label.data_ptr(),
        ws.via.data_ptr(), _stream()), "df_flow_union")


def flow_flatten(ws) -> None:
    lib = native.gpu()
    native.check(lib.df_flow_flatten(
        ws.label.data_ptr(), ws.n, ws.group.data_ptr(), _stream()),
        "df_flow_flatten")


def flow_fold(ws) -> None:
    lib = native.gpu()
    native.check(lib.df_flow_fold(
        ws.flat_ptrs.ctypes.data, ws.group.data_ptr(), ws.via.data_ptr(),
        ws.n, ws.gvals.data_ptr(), _stream()), "df_flow_fold")


# ----------------------------------------------------------------------
# K11: application-log store + substring search (dflog.hip). `st` is a
# store.log_store.GpuLogStore (owns every tensor named here).
# ----------------------------------------------------------------------

def log_ingest(st, base: int, line_off: torch.Tensor, line_len: torch.Tensor,
               now: int, agent_id: int, log_type: int, base_row: int,
               pre_app_len: torch.Tensor = None,
               pre_time: torch.Tensor = None,
               pre_sev: torch.Tensor = None) -> None:
    """Parse (or, with pre_*, take as parsed) the lines of the batch that
    already sits in st.pool at `base`; line_off is relative to it."""
    lib = native.gpu()
    pre = [t.data_ptr() if t is not None else 0
           for t in (pre_app_len, pre_time, pre_sev)]
    native.check(lib.df_log_ingest(
        st.pool.data_ptr(), base, line_off.data_ptr(), line_len.data_ptr(),
        line_off.numel(), pre[0], pre[1], pre[2], now, agent_id, log_type,
        st.tkeys.data_ptr(), st.tkeys.numel(), st.app_off.data_ptr(),
        st.app_len.data_ptr(), st.drops.data_ptr(),
        st.row_time.data_ptr(), st.row_sev.data_ptr(),
        st.row_agent.data_ptr(), st.row_type.data_ptr(),
        st.row_app.data_ptr(), st.row_boff.data_ptr(),
        st.row_blen.data_ptr(), base_row, _stream()), "df_log_ingest")


def log_scan(st, needles, fold: bool, mask: torch.Tensor) -> None:
    """OR bit k into mask[row] for every row whose body holds needles[k]
    (bytes, 1..128 each, at most 8; already folded when fold is set)."""
    if not needles:
        return
    lib = native.gpu()
    lens = np.array([len(x) for x in needles], dtype=np.uint32)
    native.check(lib.df_log_scan(
        st.pool.data_ptr(), 0, st.pool_len, st.row_boff.data_ptr(),
        st.row_blen.data_ptr(), st.n_rows, b"".join(needles),
        lens.ctypes.data, len(needles), 1 if fold else 0, mask.data_ptr(),
        _stream()), "df_log_scan")


LOG_RE_BIT = 1 << 8        # the mask bit k_log_regex sets; needles: 0..7


def log_re_limits():
    """(table bytes, pattern bytes, byte classes) k_log_regex was built
    for; query/logregex.py carries the same three."""
    out = (ctypes.c_uint32 * 3)()
    native.gpu().df_log_re_limits(out)
    return tuple(int(x) for x in out)


def log_regex_table(st, rx) -> torch.Tensor:
    """rx's tables on st's device, padded to the 16-byte chunks the kernel
    stages them in."""
    table = rx.table()
    blob = np.zeros((table.nbytes + 15) & ~15, dtype=np.uint8)
    blob[:table.nbytes] = table
    return torch.from_numpy(blob).to(st.pool.device)


def log_regex(st, rx, mask: torch.Tensor,
              table: torch.Tensor = None) -> None:
    """OR LOG_RE_BIT into mask[row] for every row whose body holds a
    non-empty match of rx (a query.logregex.LogRegex). Without `table`
    (log_regex_table) the tables are uploaded here, once per query."""
    if table is None:
        table = log_regex_table(st, rx)
    native.check(native.gpu().df_log_regex(
        st.pool.data_ptr(), 0, st.pool_len, st.row_boff.data_ptr(),
        st.row_blen.data_ptr(), st.n_rows, table.data_ptr(), rx.n_states,
        rx.n_classes, rx.flags, mask.data_ptr(), _stream()), "df_log_regex")


def log_select(st, mask: torch.Tensor, need: int, severity_max: int,
               t_lo: int, t_hi: int, app_key, flags: torch.Tensor,
               hist: torch.Tensor = None, interval: int = 1,
               n_buckets: int = 0) -> None:
    lib = native.gpu()
    native.check(lib.df_log_select(
        st.row_time.data_ptr(), st.row_sev.data_ptr(),
        st.row_app.data_ptr(), mask.data_ptr(), st.n_rows, severity_max,
        t_lo, t_hi, 0 if app_key is None else 1, app_key or 0,
        st.tkeys.data_ptr(), st.tkeys.numel(), need, flags.data_ptr(),
        hist.data_ptr() if hist is not None else 0, interval, n_buckets,
        _stream()), "df_log_select")


class LogPatternTable:
    """Query-scoped table of k_log_patterns: slot = pattern."""

    def __init__(self, device, cap: int):
        self.cap = cap
        self.keys = torch.zeros(cap, dtype=torch.int64, device=device)
        self.count = torch.zeros(cap, dtype=torch.int64, device=device)
        # u32 words: ROW_NONE until a row takes them with atomicMin
        self.first_row = torch.full((cap,), -1, dtype=torch.int32,
                                    device=device)
        # atomicMax; valid where count != 0
        self.last_row = torch.zeros(cap, dtype=torch.int32, device=device)
        self.drops = torch.zeros(1, dtype=torch.int64, device=device)

    def reset(self) -> None:
        self.keys.zero_()
        self.count.zero_()
        self.first_row.fill_(-1)
        self.last_row.zero_()
        self.drops.zero_()


def log_patterns(st, flags: torch.Tensor, cap: int,
                 out_key: torch.Tensor = None,
                 table: LogPatternTable = None) -> LogPatternTable:
    """Group the rows of st with flags[row] != 0 (u8 per row) by the
    template of their body (query/logpattern.py) into a table of `cap`
    slots, a power of two: a fresh one, or `table` (reset by the caller).
    One launch; nothing comes to the host.
    out_key (i64 per row, tests): gets the key of every flagged row."""
    n = st.n_rows
    assert flags.dtype == torch.uint8 and flags.numel() >= n
    assert out_key is None or \
        (out_key.dtype == torch.int64 and out_key.numel() >= n)
    # the kernel loads aligned 16-byte chunks that start below pool_len
    assert st.pool_len <= st.pool.numel() and st.pool.numel() % 16 == 0
    t = table if table is not None else LogPatternTable(st.pool.device, cap)
    assert t.cap == cap
    native.check(native.gpu().df_log_patterns(
        st.pool.data_ptr(), st.pool_len, st.row_boff.data_ptr(),
        st.row_blen.data_ptr(), flags.data_ptr(), n, t.keys.data_ptr(), cap,
        t.count.data_ptr(), t.first_row.data_ptr(), t.last_row.data_ptr(),
        t.drops.data_ptr(), out_key.data_ptr() if out_key is not None else 0,
        _stream()), "df_log_patterns")
    return t


def log_evict(st, first: int):
    """Drop the `first` oldest rows of st (0 < first <= st.n_rows) by
    compacting it out of place into fresh row columns and a fresh pool
    (k_log_evict_plan, k_log_evict, one D2D copy of the pool's suffix; the
    layout is described in dflog.hip). One host read: the arena length and
    the cut. Replaces st's pool, row columns, pool_len and n_rows and
    rewrites app_off; tkeys, app_len and drops stay. What the host keys by
    row index (OTLP extras, dense app ids) is the caller's to fix.
    -> (cut, arena): bytes dropped from the front of the old pool, bytes of
    relocated app names at the front of the new one."""
    n = st.n_rows
    if not 0 < first <= n:
        raise ValueError("first must be in 1..n_rows")
    lib = native.gpu()
    dev = st.pool.device
    cap = st.tkeys.numel()
    reloc = torch.empty(cap, dtype=torch.int64, device=dev)
    out = torch.empty(2, dtype=torch.int64, device=dev)
    native.check(lib.df_log_evict_plan(
        st.tkeys.data_ptr(), cap, st.app_off.data_ptr(),
        st.app_len.data_ptr(), st.row_boff.data_ptr(),
        st.row_blen.data_ptr(), first, n, st.pool_len, reloc.data_ptr(),
        out.data_ptr(), _stream()), "df_log_evict_plan")
    packed, cut = out.tolist()
    arena = (packed + 15) & ~15
    assert 0 <= cut <= st.pool_len
    keep = n - first
    tail = st.pool_len - cut
    new_len = arena + tail
    # the arena can outgrow the cut by 16 bytes at the most (dflog.hip)
    new_cap = max(st.pool.numel(), (new_len + 15) & ~15)
    pool = torch.empty(new_cap, dtype=torch.uint8, device=dev)
    assert pool.data_ptr() % 16 == 0
    pool[:arena].zero_()
    old_cols = [getattr(st, name) for name, _ in st._COLS]
    new_cols = [torch.empty_like(c) for c in old_cols]
    native.check(lib.df_log_evict(
        st.pool.data_ptr(), pool.data_ptr(), st.pool_len, cut, arena,
        new_cap, st.tkeys.data_ptr(), cap, st.app_off.data_ptr(),
        st.app_len.data_ptr(), reloc.data_ptr(),
        *[c.data_ptr() for c in old_cols],
        *[c.data_ptr() for c in new_cols], first, keep, _stream()),
        "df_log_evict")
    if tail:
        pool[arena:new_len] = st.pool[cut:st.pool_len]
    for (name, _), c in zip(st._COLS, new_cols):
        setattr(st, name, c)
    st.pool = pool
    st.pool_len = new_len
    st.n_rows = keep
    return cut, arena
