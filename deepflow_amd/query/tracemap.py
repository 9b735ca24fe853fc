"""Bulk trace assembly over a time window (K10): every span linked to its
parent, per-trace summaries, and the service -> service edge table.

`DistributedTracer.assemble()` builds one tree for one trace id; this module
answers the window-wide questions ("which services call which, as seen by
traces") in one pass. Reference counterparts: libs/tracetree (the tree
rows), querier tracemap (the generator), flow_log tracetree_writer.

Semantics, shared by the host twin below and ops/csrc/dftrace.hip:

* global row = position in scan order (`SegmentSet.scan_list()` order,
  then row order inside a segment);
* a row takes part when start_time lies in [time_start, time_end] and its
  trace key (SRC_TRACE128 idx 0) is non-zero;
* three first-row-wins indexes per query: (trace, span key),
  (trace, syscall_trace_id_response), (trace, req_tcp_seq | tap_side == 1);
* parent = parent-span key in the span index (kind 1), else
  syscall_trace_id_request in the syscall index (kind 2), else, unless
  tap_side == 1, req_tcp_seq in the tcp index (kind 3); a candidate equal
  to the row itself is rejected at each step; never across traces;
* depth = hops to a parentless row, at most MAX_TRACE_HOPS, else -1
  ("unrooted": cycles and over-deep chains).

The parent key applies the decoder's span-id rule to the pooled
parent_span_id text (16 hex chars -> the parsed value, anything else -> the
pooled-string hash), so it equals the span key of the span that carries the
same text. Hex case is therefore not significant here, while `assemble()`
compares the hydrated (lower-case) strings.

device 'cpu' runs the host twin (the oracle); anything else runs the HIP
kernels. There is no fallback between the two.
"""
from __future__ import annotations

import contextlib
from typing import Dict, List, Optional

import numpy as np
import torch

from ..store import l7_schema as S
from ..wire.const_enums import STATUS_CLIENT_ERROR, STATUS_SERVER_ERROR
from .spec import SRC_TRACE128, STR_FILTER_SEED
from .tags import L7_TAGS

MAX_TRACE_HOPS = 4096  # twin: dftrace.hip MAX_TRACE_HOPS
U64MAX = (1 << 64) - 1
M32 = 0xFFFFFFFF

LINK_NONE, LINK_SPAN, LINK_SYSCALL, LINK_TCP = 0, 1, 2, 3
# value words of the per-trace and per-edge tables (twin: dftrace.hip enums)
(TV_SPANS, TV_ROOTS, TV_UNROOTED, TV_MAX_DEPTH, TV_ERRORS, TV_START_MIN,
 TV_END_MAX, TV_ROOT_ROW, TV_FIRST_ROW, TV_N) = range(10)
(EV_CALLS, EV_SPAN, EV_SYSCALL, EV_TCP, EV_ERRORS, EV_DUR_NS,
 EV_N) = range(7)
_TV_MIN_WORDS = [TV_START_MIN, TV_ROOT_ROW, TV_FIRST_ROW]

_U64 = {c: i for i, c in enumerate(S.U64_COLS)}
_U32 = {c: i for i, c in enumerate(S.U32_COLS)}
_U8 = {c: i for i, c in enumerate(S.U8_COLS)}
_DID_SERVICE = [c[0] for c in S.DID_COLS].index("service_name")


def _pow2_at_least(n: int) -> int:
    return 1 << max(int(n) - 1, 1).bit_length()


def pool_strings(seg, n: int, idx: int):
    """(row, bytes) of every non-empty string in pool column `idx` among
    the first n rows of a host segment (twin: dfseg.h seg_pool_str)."""
    lens = seg.str_lens[:, :n].numpy().view(np.uint16)
    hit = np.nonzero(lens[idx])[0]
    if len(hit) == 0:
        return
    rowref = seg.str_rowref[:n].numpy().view(np.uint64)
    pool = seg.pool.numpy().tobytes()
    before = lens[:idx].astype(np.int64).sum(axis=0)
    for i in hit:
        off = (int(rowref[i]) >> 16) + int(before[i])
        yield i, pool[off:off + int(lens[idx, i])]


def _parent_keys_np(seg, n: int) -> np.ndarray:
    from ..ops.ref import hex_parse64_py
    from ..store.dictionary import str_hash_py
    out = np.zeros(n, dtype=np.uint64)
    for i, raw in pool_strings(seg, n, S.POOL_POS["parent_span_id"]):
        v = hex_parse64_py(raw)
        out[i] = str_hash_py(raw, STR_FILTER_SEED) if v is None else v
    return out


@contextlib.contextmanager
def _timed_launches(kernel_ms: Optional[Dict[str, float]]):
    """Yields mark(name), to be called after each group of launches. With a
    dict, the milliseconds since the previous mark land under `name` (one
    event pair per mark); with None, marks cost nothing."""
    marks = []

    def mark(name):
        if kernel_ms is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((name, ev))

    mark("start")
    yield mark
    if kernel_ms is not None:
        torch.cuda.synchronize()
        for (_, a), (name, b) in zip(marks, marks[1:]):
            kernel_ms[name] = a.elapsed_time(b)


class _Flat:
    """Host flat columns over global rows (the GPU path's TraceFlat)."""

    def __init__(self, segs, tb: int, lo: int, hi: int):
        from .executor import _src_np
        cols = {k: [] for k in ("tkey", "skey", "pkey", "sreq", "sresp",
                                "start", "end", "tcp", "svc", "tap",
                                "status")}
        for seg in segs:
            n = seg.n_rows
            if n == 0:
                continue
            u64 = lambda c: seg.u64[_U64[c], :n].numpy().view(np.uint64)
            cols["tkey"].append(_src_np(seg, SRC_TRACE128, 0, 0, tb, n))
            cols["skey"].append(_src_np(seg, SRC_TRACE128, 1, 0, tb, n))
            cols["pkey"].append(_parent_keys_np(seg, n))
            cols["sreq"].append(u64("syscall_trace_id_request"))
            cols["sresp"].append(u64("syscall_trace_id_response"))
            cols["start"].append(u64("start_time"))
            cols["end"].append(u64("end_time"))
            cols["tcp"].append(seg.u32[_U32["req_tcp_seq"], :n].numpy()
                               .view(np.uint32))
            cols["svc"].append(seg.did[_DID_SERVICE, :n].numpy()
                               .view(np.uint32))
            cols["tap"].append(seg.u8[_U8["tap_side"], :n].numpy())
            cols["status"].append(seg.u8[_U8["response_status"], :n].numpy())
        dts = dict(tcp=np.uint32, svc=np.uint32, tap=np.uint8,
                   status=np.uint8)
        for k, parts in cols.items():
            setattr(self, k, np.concatenate(parts) if parts else
                    np.zeros(0, dtype=dts.get(k, np.uint64)))
        part = (self.start >= np.uint64(lo)) & (self.start <= np.uint64(hi)) \
            & (self.tkey != 0)
        self.tkey = np.where(part, self.tkey, np.uint64(0))
        self.n = int(self.tkey.shape[0])


def _host_link(f: _Flat):
    """-> (rows, parent, kind, depth); the last three over all global rows."""
    rows = np.nonzero(f.tkey)[0]
    tkey, skey, sresp = f.tkey.tolist(), f.skey.tolist(), f.sresp.tolist()
    tcp, tap = f.tcp.tolist(), f.tap.tolist()
    pkey, sreq = f.pkey.tolist(), f.sreq.tolist()
    rows_l = rows.tolist()
    span_ix: Dict[tuple, int] = {}
    sys_ix: Dict[tuple, int] = {}
    tcp_ix: Dict[tuple, int] = {}
    for g in rows_l:                       # ascending: the first row wins
        t = tkey[g]
        if skey[g]:
            span_ix.setdefault((t, skey[g]), g)
        if sresp[g]:
            sys_ix.setdefault((t, sresp[g]), g)
        if tcp[g] and tap[g] == 1:
            tcp_ix.setdefault((t, tcp[g]), g)
    parent = np.full(f.n, -1, dtype=np.int64)
    kind = np.zeros(f.n, dtype=np.uint8)
    for g in rows_l:
        t = tkey[g]
        steps = [(LINK_SPAN, span_ix, pkey[g]), (LINK_SYSCALL, sys_ix, sreq[g])]
        if tap[g] != 1:
            steps.append((LINK_TCP, tcp_ix, tcp[g]))
        for k, ix, v in steps:
            c = ix.get((t, v)) if v else None
            if c is not None and c != g:
                parent[g], kind[g] = c, k
                break
    # depth: hops to a parentless row, exact under the MAX_TRACE_HOPS bound
    # (a row's depth is its parent's + 1 while that stays within the bound)
    UNK = -2
    par = parent.tolist()
    depth = [UNK] * f.n
    for g in rows_l:
        if depth[g] != UNK:
            continue
        path, cur, over = [], g, False
        while depth[cur] == UNK:
            path.append(cur)
            if len(path) > MAX_TRACE_HOPS + 1:
                over = True
                break
            if par[cur] < 0:
                break
            cur = par[cur]
        if over:
            depth[g] = -1       # MAX_TRACE_HOPS hops made, still no root
            continue
        p = par[path[-1]]
        d = 0 if p < 0 else \
            (depth[p] + 1 if 0 <= depth[p] < MAX_TRACE_HOPS else -1)
        depth[path[-1]] = d
        for node in reversed(path[:-1]):
            d = d + 1 if 0 <= d < MAX_TRACE_HOPS else -1
            depth[node] = d
    depth_a = np.array(depth, dtype=np.int64)
    depth_a[depth_a == UNK] = 0
    return rows, parent, kind, depth_a.astype(np.int32)


def _host_fold(f: _Flat, rows, parent, kind, depth):
    traces: Dict[int, List[int]] = {}
    edges: Dict[tuple, List[int]] = {}
    errs = (STATUS_SERVER_ERROR, STATUS_CLIENT_ERROR)
    for g in rows.tolist():
        tv = traces.get(int(f.tkey[g]))
        if tv is None:
            tv = [0] * TV_N
            for w in _TV_MIN_WORDS:
                tv[w] = U64MAX
            traces[int(f.tkey[g])] = tv
        p, d = int(parent[g]), int(depth[g])
        err = int(f.status[g]) in errs
        start, end = int(f.start[g]), int(f.end[g])
        tv[TV_SPANS] += 1
        if d < 0:
            tv[TV_UNROOTED] += 1
        else:
            tv[TV_MAX_DEPTH] = max(tv[TV_MAX_DEPTH], d)
        if p < 0:
            tv[TV_ROOTS] += 1
            tv[TV_ROOT_ROW] = min(tv[TV_ROOT_ROW], g)
        tv[TV_ERRORS] += err
        tv[TV_START_MIN] = min(tv[TV_START_MIN], start)
        tv[TV_END_MAX] = max(tv[TV_END_MAX], end)
        tv[TV_FIRST_ROW] = min(tv[TV_FIRST_ROW], g)
        if p < 0:
            continue
        ev = edges.setdefault((int(f.svc[p]), int(f.svc[g])), [0] * EV_N)
        k = int(kind[g])
        ev[EV_CALLS] += 1
        ev[EV_SPAN] += k == LINK_SPAN
        ev[EV_SYSCALL] += k == LINK_SYSCALL
        ev[EV_TCP] += k == LINK_TCP
        ev[EV_ERRORS] += err
        ev[EV_DUR_NS] += max(end - start, 0)
    tk = np.array(list(traces.keys()), dtype=np.uint64)
    tv = np.array(list(traces.values()), dtype=np.uint64).reshape(-1, TV_N)
    esvc = np.array(list(edges.keys()), dtype=np.int64).reshape(-1, 2)
    ev = np.array(list(edges.values()), dtype=np.uint64).reshape(-1, EV_N)
    return tk, tv, esvc, ev


class _GpuWorkspace:
    """Query-scoped device buffers: flat columns over `n` global rows, the
    three join indexes, and the trace/edge tables. Every table holds a
    power of two >= 2n slots (n bounds the participating rows)."""

    def __init__(self, n: int, dev):
        self.n = n
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        z = lambda shape: torch.zeros(shape, dtype=torch.int64, device=dev)
        i64, i32, u8 = torch.int64, torch.int32, torch.uint8
        self.tkey, self.pkey, self.sreq = e(n, i64), e(n, i64), e(n, i64)
        self.start, self.end = e(n, i64), e(n, i64)
        self.tcp, self.svc = e(n, i32), e(n, i32)
        self.tap, self.status = e(n, u8), e(n, u8)
        self.flat_ptrs = np.array(
            [t.data_ptr() for t in (self.tkey, self.pkey, self.sreq,
                                    self.start, self.end, self.tcp,
                                    self.svc, self.tap, self.status)],
            dtype=np.uint64)
        cap = _pow2_at_least(max(2 * n, 64))
        self.idx_cap = cap
        self.idx_keys = z(3 * cap)
        self.idx_rows = torch.full((3 * cap,), -1, dtype=i32, device=dev)
        self.drops = z(1)
        self.parent, self.kind, self.depth = e(n, i32), e(n, u8), e(n, i32)
        self.tkeys, self.tvals = z(cap), z((cap, TV_N))
        self.tvals[:, _TV_MIN_WORDS] = -1          # atomicMin words
        self.ekeys, self.evals = z(cap), z((cap, EV_N))


class TraceMapper:
    def __init__(self, engine):
        self.engine = engine
        # when set, the GPU path records per-kernel milliseconds here
        # (benchmarks/trace_map.py); costs one event pair per launch
        self.kernel_ms: Optional[Dict[str, float]] = None

    # ------------------------------------------------------------ plumbing
    def _on_gpu(self) -> bool:
        return not str(self.engine.device).startswith("cpu")

    def _window(self, time_start, time_end):
        lo = 0 if time_start is None else max(int(time_start), 0)
        hi = U64MAX if time_end is None else min(int(time_end), U64MAX)
        return lo, hi

    def _scan(self, lo: int, hi: int):
        pipe = self.engine.pipe
        if hasattr(pipe, "sync_stats"):
            pipe.sync_stats()
        tr = None if (lo == 0 and hi == U64MAX) else (lo, hi)
        segs = [s for s in pipe.segments.scan_list(time_range=tr)
                if s.n_rows]
        bases = np.cumsum([0] + [s.n_rows for s in segs])
        if int(bases[-1]) >= M32:
            raise ValueError("trace map window exceeds 2^32-1 rows")
        return segs, bases

    def _gpu_run(self, segs, bases, lo: int, hi: int, fold: bool):
        from ..ops import gpu_ops
        dev = segs[0].u64.device
        ws = _GpuWorkspace(int(bases[-1]), dev)
        with _timed_launches(self.kernel_ms) as mark:
            for seg, base in zip(segs, bases):
                gpu_ops.trace_extract(seg, int(base), lo, hi, ws)
            mark("extract")
            gpu_ops.trace_link(ws)
            mark("link")
            gpu_ops.trace_depth(ws)
            mark("depth")
            if fold:
                gpu_ops.trace_fold(ws)
                mark("fold")
        return ws

    def _trace_ids(self, segs, bases, rows: np.ndarray) -> List[str]:
        """Hex/pooled trace id of each global row: the binary columns are
        gathered per segment in bulk; pooled fallbacks go through the
        engine's row fetch."""
        out: List[str] = [""] * len(rows)
        si = np.searchsorted(bases, rows, side="right") - 1
        hi_i, lo_i = _U64["trace_id_hi"], _U64["trace_id_lo"]
        for s in np.unique(si).tolist():
            seg = segs[s]
            pos = np.nonzero(si == s)[0]
            local = rows[pos] - int(bases[s])
            lt = torch.from_numpy(local.astype(np.int64)).to(seg.u64.device)
            hl = torch.stack([seg.u64[hi_i].index_select(0, lt),
                              seg.u64[lo_i].index_select(0, lt)]) \
                .cpu().numpy().view(np.uint64)
            for j, p in enumerate(pos.tolist()):
                h, l = int(hl[0, j]), int(hl[1, j])
                out[p] = f"{h:016x}{l:016x}" if (h | l) else \
                    self.engine._fetch(seg, int(local[j]), "trace_id",
                                       L7_TAGS, S.STR_COLS)
        return out

    # -------------------------------------------------------------- public
    def link_spans(self, time_start=None, time_end=None) -> Dict:
        """Arrays over participating rows in global-row order: row,
        trace_key, parent_row (-1 = none), link_kind, depth (-1 =
        unrooted)."""
        lo, hi = self._window(time_start, time_end)
        with self.engine.lock:
            try:
                segs, bases = self._scan(lo, hi)
                if not segs:
                    return {"row": np.zeros(0, np.int64),
                            "trace_key": np.zeros(0, np.uint64),
                            "parent_row": np.zeros(0, np.int64),
                            "link_kind": np.zeros(0, np.uint8),
                            "depth": np.zeros(0, np.int32), "drops": 0}
                if self._on_gpu():
                    ws = self._gpu_run(segs, bases, lo, hi, fold=False)
                    rows = torch.nonzero(ws.tkey).view(-1)
                    packed = torch.stack([
                        rows, ws.tkey[rows], ws.parent[rows].to(torch.int64),
                        ws.kind[rows].to(torch.int64),
                        ws.depth[rows].to(torch.int64)]).cpu().numpy()
                    return {"row": packed[0],
                            "trace_key": packed[1].view(np.uint64),
                            "parent_row": packed[2],
                            "link_kind": packed[3].astype(np.uint8),
                            "depth": packed[4].astype(np.int32),
                            "drops": int(ws.drops.item())}
                f = _Flat(segs, self.engine.pipe.time_base_s, lo, hi)
                rows, parent, kind, depth = _host_link(f)
                return {"row": rows.astype(np.int64),
                        "trace_key": f.tkey[rows], "parent_row": parent[rows],
                        "link_kind": kind[rows], "depth": depth[rows],
                        "drops": 0}
            finally:
                self.engine.pipe.segments.release_scratch()

    def trace_map(self, time_start=None, time_end=None) -> Dict:
        lo, hi = self._window(time_start, time_end)
        with self.engine.lock:
            try:
                segs, bases = self._scan(lo, hi)
                if not segs:
                    return {"traces": [], "edges": [], "trace_count": 0,
                            "span_count": 0, "drops": 0}
                if self._on_gpu():
                    tab = self._gpu_tables(segs, bases, lo, hi)
                else:
                    tab = self._host_tables(segs, lo, hi)
                return self._finish(segs, bases, *tab)
            finally:
                self.engine.pipe.segments.release_scratch()

    # ------------------------------------------------------------- tables
    def _host_tables(self, segs, lo, hi):
        f = _Flat(segs, self.engine.pipe.time_base_s, lo, hi)
        rows, parent, kind, depth = _host_link(f)
        tk, tv, esvc, ev = _host_fold(f, rows, parent, kind, depth)
        root = self._root_rows(tv)
        rinfo = np.stack([f.svc[root].astype(np.uint64), f.start[root],
                          f.end[root]], axis=1) if len(root) else \
            np.zeros((0, 3), np.uint64)
        return tk, tv, root, rinfo, esvc, ev, 0

    @staticmethod
    def _root_rows(tv: np.ndarray) -> np.ndarray:
        # the lowest root, or the lowest row of a trace that has none
        return np.where(tv[:, TV_ROOTS] > 0, tv[:, TV_ROOT_ROW],
                        tv[:, TV_FIRST_ROW]).astype(np.int64)

    def _gpu_tables(self, segs, bases, lo, hi):
        return self._read_gpu_tables(
            self._gpu_run(segs, bases, lo, hi, fold=True))

    @staticmethod
    def _read_gpu_tables(ws: _GpuWorkspace):
        # one compaction + one D2H per table
        tsel = torch.nonzero(ws.tkeys).view(-1)
        tv_d = ws.tvals[tsel]
        root_d = torch.where(tv_d[:, TV_ROOTS] > 0, tv_d[:, TV_ROOT_ROW],
                             tv_d[:, TV_FIRST_ROW])
        tpack = torch.cat([
            ws.tkeys[tsel].view(-1, 1), tv_d, root_d.view(-1, 1),
            (ws.svc[root_d].to(torch.int64) & M32).view(-1, 1),
            ws.start[root_d].view(-1, 1), ws.end[root_d].view(-1, 1)],
            dim=1).cpu().numpy().view(np.uint64)
        esel = torch.nonzero(ws.ekeys).view(-1)
        epack = torch.cat([ws.ekeys[esel].view(-1, 1), ws.evals[esel]],
                          dim=1).cpu().numpy().view(np.uint64)
        drops = int(ws.drops.item())
        tk, tv = tpack[:, 0], tpack[:, 1:1 + TV_N]
        root = tpack[:, 1 + TV_N].astype(np.int64)
        rinfo = tpack[:, 2 + TV_N:]
        # edge key = ((parent id + 1) << 32 | (child id + 1)) + 1, halves
        # wrapping at 32 bits (dftrace.hip edge_key)
        k = epack[:, 0] - np.uint64(1)
        esvc = np.stack([((k >> np.uint64(32)).astype(np.int64) - 1) & M32,
                         ((k & np.uint64(M32)).astype(np.int64) - 1) & M32],
                        axis=1)
        return tk, tv, root, rinfo, esvc, epack[:, 1:], drops

    def _finish(self, segs, bases, tk, tv, root, rinfo, esvc, ev,
                drops: int) -> Dict:
        hyd = self.engine._hydrator(L7_TAGS["service_name"].hydrate)
        svc_name = lambda i: hyd(int(i)) or ""
        ids = self._trace_ids(segs, bases, root)
        traces = []
        for i, tid in enumerate(ids):
            v = tv[i].tolist()
            rstart, rend = int(rinfo[i, 1]), int(rinfo[i, 2])
            traces.append({
                "trace_id": tid,
                "time": rstart // 10**9,
                "start_time": v[TV_START_MIN],
                "end_time": v[TV_END_MAX],
                "span_count": v[TV_SPANS],
                "root_count": v[TV_ROOTS],
                "unrooted": v[TV_UNROOTED],
                "max_depth": v[TV_MAX_DEPTH],
                "error_count": v[TV_ERRORS],
                "root_service": svc_name(rinfo[i, 0]),
                "duration_us": max(rend - rstart, 0) // 1000,
            })
        traces.sort(key=lambda t: (t["start_time"], t["trace_id"]))
        edges = []
        for (p, c), v in zip(esvc.tolist(), ev.tolist()):
            edges.append({
                "parent_service": svc_name(p),
                "child_service": svc_name(c),
                "calls": v[EV_CALLS],
                "calls_span": v[EV_SPAN],
                "calls_syscall": v[EV_SYSCALL],
                "calls_tcp": v[EV_TCP],
                "errors": v[EV_ERRORS],
                "duration_ns_sum": v[EV_DUR_NS],
            })
        edges.sort(key=lambda e: (e["parent_service"], e["child_service"]))
        return {"traces": traces, "edges": edges,
                "trace_count": len(traces),
                "span_count": sum(t["span_count"] for t in traces),
                "drops": drops}
