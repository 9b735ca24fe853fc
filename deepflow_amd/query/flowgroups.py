"""Flow groups over a time window (K12): every span, with or without a
trace id, put into the group of spans it shares a join key with.

K10 (tracemap.py) links spans inside one trace id. eBPF and packet spans
carry none; they are tied to each other and to instrumented spans by
syscall trace ids, tcp sequence numbers and x-request-ids. This module
partitions ALL spans of a window by those keys, summarises each group, and
returns the group a given id belongs to. Reference counterpart: the
tracing app that `server/querier/tempo` calls out to (not in the reference
tree); the oracle is the host twin below.

Semantics, shared by the host twin and ops/csrc/dfflow.hip:

* global row, scan order, the window test (start_time in
  [time_start, time_end]) and the 2^32-1 row cap are those of tracemap.py;
* every row in the window takes part, whether or not it has a trace id;
* a participating row emits up to six join keys in four key spaces; a zero
  or empty value emits nothing:
  - REL_TRACE: the K10 trace key (SRC_TRACE128 idx 0);
  - REL_SYSCALL: syscall_trace_id_request and syscall_trace_id_response,
    two keys in one space (a request id matches another row's request or
    response id);
  - REL_TCP: req_tcp_seq | resp_tcp_seq << 32, emitted when req_tcp_seq is
    non-zero. The pair, not the request sequence alone: 32-bit sequence
    numbers collide across a large window, and two taps on one session see
    both numbers;
  - REL_XREQ: the pooled-string hash (seed STR_FILTER_SEED) of
    x_request_id_0 and of x_request_id_1, two keys in one space (a
    gateway's outgoing id meets the next hop's incoming id);
* two rows are related when they emit an equal key in the same space; a
  group is a connected component of that relation, and its id is its
  lowest global row, which makes the result unique;
* one first-row-wins index over (space, key); each row is united with the
  index row of each of its keys. `via` bit r of a row is set when some key
  of space r has an index row other than the row itself;
* the result is the full transitive closure inside the window. The
  reference app bounds its expansion by an iteration count instead; there
  is no such bound here. On the GPU equal 64-bit mixes of different
  (space, key) pairs would share an index slot, the identity K10 accepts.

Per-group words (GV_*): spans, spans with a trace key, errors (the K10
status rule), min start, max end, lowest row with a trace key (all-ones if
none), and per space the number of rows with that `via` bit.

device 'cpu' runs the host twin (the oracle): a plain union-find over
dictionaries, linking to the minimum root. Anything else runs the HIP
kernels. There is no fallback between the two.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from ..store import l7_schema as S
from ..wire.const_enums import STATUS_CLIENT_ERROR, STATUS_SERVER_ERROR
from .spec import SRC_TRACE128, STR_FILTER_SEED
from .tags import L7_TAGS
from .tracemap import (M32, U64MAX, TraceMapper, _pow2_at_least,
                       _timed_launches, pool_strings)

# key spaces (twin: dfflow.hip REL_*); bit r of `via` = space r
REL_TRACE, REL_SYSCALL, REL_TCP, REL_XREQ, REL_N = range(5)
# per-group value words (twin: dfflow.hip GV_*)
(GV_SPANS, GV_TRACED, GV_ERRORS, GV_START_MIN, GV_END_MAX,
 GV_FIRST_TRACED_ROW, GV_VIA_TRACE, GV_VIA_SYSCALL, GV_VIA_TCP, GV_VIA_XREQ,
 GV_N) = range(11)
_GV_MIN_WORDS = [GV_START_MIN, GV_FIRST_TRACED_ROW]
KEYS_PER_ROW = 6        # twin: dfflow.hip FLOW_KEYS_PER_ROW
MAX_IDX_CAP = 1 << 31   # the index capacity is a 32-bit power of two

# key columns of the flat table in emit order, with their spaces
_KEY_COLS = (("tkey", REL_TRACE), ("sreq", REL_SYSCALL),
             ("sresp", REL_SYSCALL), ("tcp", REL_TCP), ("x0", REL_XREQ),
             ("x1", REL_XREQ))
# flat columns in FlowFlat order (dfflow.hip)
_FLAT_COLS = ("part", "tkey", "sreq", "sresp", "tcp", "x0", "x1", "start",
              "end", "status")

# what flow_trace returns per span: the columns fetch_spans selects, plus
# the two x-request-ids
SPAN_COLS = ("trace_id", "span_id", "parent_span_id", "request_resource",
             "service_name", "start_time", "end_time", "response_status",
             "syscall_trace_id_request", "syscall_trace_id_response",
             "req_tcp_seq", "resp_tcp_seq", "tap_side", "flow_id",
             "x_request_id_0", "x_request_id_1")

_U64 = {c: i for i, c in enumerate(S.U64_COLS)}
_U32 = {c: i for i, c in enumerate(S.U32_COLS)}
_U8 = {c: i for i, c in enumerate(S.U8_COLS)}


def trace_key_of(trace_id: str) -> int:
    """The stored trace key of a trace-id literal (sql.py's tracebin
    rule)."""
    from ..ops.ref import mix64
    from ..store.dictionary import str_hash_py
    if len(trace_id) == 32 and \
            all(c in "0123456789abcdefABCDEF" for c in trace_id):
        v = int(trace_id, 16)
        if v:
            return mix64(v >> 64) ^ (v & U64MAX)
    return str_hash_py(trace_id.encode(), STR_FILTER_SEED)


def xreq_key_of(x_request_id: str) -> int:
    from ..store.dictionary import str_hash_py
    return str_hash_py(x_request_id.encode(), STR_FILTER_SEED)


def _pool_hash_np(seg, n: int, idx: int) -> np.ndarray:
    """Pooled-string hash of pool column `idx`, 0 where it is empty."""
    from ..store.dictionary import str_hash_py
    out = np.zeros(n, dtype=np.uint64)
    for i, raw in pool_strings(seg, n, idx):
        out[i] = str_hash_py(raw, STR_FILTER_SEED)
    return out


class _Flat:
    """Host flat columns over global rows (the GPU path's FlowFlat). Key
    columns are zero on rows that take no part."""

    def __init__(self, segs, tb: int, lo: int, hi: int):
        from .executor import _src_np
        cols = {k: [] for k in _FLAT_COLS[1:]}
        for seg in segs:
            n = seg.n_rows
            if n == 0:
                continue
            u64 = lambda c: seg.u64[_U64[c], :n].numpy().view(np.uint64)
            u32 = lambda c: seg.u32[_U32[c], :n].numpy().view(np.uint32) \
                .astype(np.uint64)
            cols["tkey"].append(_src_np(seg, SRC_TRACE128, 0, 0, tb, n))
            cols["sreq"].append(u64("syscall_trace_id_request"))
            cols["sresp"].append(u64("syscall_trace_id_response"))
            req, resp = u32("req_tcp_seq"), u32("resp_tcp_seq")
            cols["tcp"].append(np.where(
                req != 0, req | (resp << np.uint64(32)), np.uint64(0)))
            cols["x0"].append(_pool_hash_np(
                seg, n, S.POOL_POS["x_request_id_0"]))
            cols["x1"].append(_pool_hash_np(
                seg, n, S.POOL_POS["x_request_id_1"]))
            cols["start"].append(u64("start_time"))
            cols["end"].append(u64("end_time"))
            cols["status"].append(seg.u8[_U8["response_status"], :n].numpy())
        for k, parts in cols.items():
            setattr(self, k, np.concatenate(parts) if parts else
                    np.zeros(0, np.uint8 if k == "status" else np.uint64))
        self.part = ((self.start >= np.uint64(lo)) &
                     (self.start <= np.uint64(hi))).astype(np.uint8)
        for k, _ in _KEY_COLS:
            setattr(self, k, np.where(self.part != 0, getattr(self, k),
                                      np.uint64(0)))
        self.n = int(self.part.shape[0])


def _host_union(f):
    """-> (rows, group, via); the last two over all global rows. A row
    outside the window is its own group."""
    rows = np.nonzero(f.part)[0]
    rows_l = rows.tolist()
    keys = [(getattr(f, c).tolist(), rel) for c, rel in _KEY_COLS]
    index: Dict[tuple, int] = {}
    for g in rows_l:                       # ascending: the first row wins
        for col, rel in keys:
            if col[g]:
                index.setdefault((rel, col[g]), g)
    label = list(range(f.n))

    def find(x):
        while label[x] != x:
            label[x] = label[label[x]]     # halving
            x = label[x]
        return x

    via = np.zeros(f.n, dtype=np.uint8)
    for g in rows_l:
        v = 0
        for col, rel in keys:
            if not col[g]:
                continue
            rep = index[(rel, col[g])]
            if rep == g:
                continue
            v |= 1 << rel
            a, b = find(g), find(rep)
            if a != b:                     # the lower root stays a root
                label[max(a, b)] = min(a, b)
        via[g] = v
    group = np.array([find(g) for g in range(f.n)], dtype=np.int64) \
        if f.n else np.zeros(0, np.int64)
    return rows, group, via


def _host_fold(f, rows, group, via):
    """-> (group ids ascending, [groups, GV_N] words)."""
    errs = (STATUS_SERVER_ERROR, STATUS_CLIENT_ERROR)
    out: Dict[int, List[int]] = {}
    for g in rows.tolist():
        gv = out.get(int(group[g]))
        if gv is None:
            gv = [0] * GV_N
            for w in _GV_MIN_WORDS:
                gv[w] = U64MAX
            out[int(group[g])] = gv
        gv[GV_SPANS] += 1
        if int(f.tkey[g]):
            gv[GV_TRACED] += 1
            gv[GV_FIRST_TRACED_ROW] = min(gv[GV_FIRST_TRACED_ROW], g)
        gv[GV_ERRORS] += int(f.status[g]) in errs
        gv[GV_START_MIN] = min(gv[GV_START_MIN], int(f.start[g]))
        gv[GV_END_MAX] = max(gv[GV_END_MAX], int(f.end[g]))
        for r in range(REL_N):
            gv[GV_VIA_TRACE + r] += (int(via[g]) >> r) & 1
    gid = np.array(sorted(out), dtype=np.int64)
    gv = np.array([out[g] for g in gid.tolist()], dtype=np.uint64) \
        .reshape(-1, GV_N)
    return gid, gv


class _FlowWorkspace:
    """Query-scoped device buffers: flat columns over `n` global rows, the
    one join index, the union-find labels and the group table. The index
    holds a power of two >= 12n slots: a row emits at most six keys, so the
    load factor stays at or below one half."""

    def __init__(self, n: int, dev):
        self.n = n
        cap = _pow2_at_least(max(2 * KEYS_PER_ROW * n, 64))
        if cap > MAX_IDX_CAP:
            raise ValueError("flow-group window needs a join index of more "
                             "than 2^31 slots")
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        z = lambda shape: torch.zeros(shape, dtype=torch.int64, device=dev)
        i64, i32, u8 = torch.int64, torch.int32, torch.uint8
        for c in _FLAT_COLS:
            setattr(self, c, e(n, u8 if c in ("part", "status") else i64))
        self.flat_ptrs = np.array(
            [getattr(self, c).data_ptr() for c in _FLAT_COLS],
            dtype=np.uint64)
        self.idx_cap = cap
        self.idx_keys = z(cap)
        self.idx_rows = torch.full((cap,), -1, dtype=i32, device=dev)
        self.drops = z(1)
        self.label = torch.arange(n, dtype=i32, device=dev)
        self.via = torch.zeros(n, dtype=u8, device=dev)
        self.group = e(n, i32)
        self.gvals = z((n, GV_N))
        self.gvals[:, _GV_MIN_WORDS] = -1          # atomicMin words


def _empty_links() -> Dict:
    return {"row": np.zeros(0, np.int64), "group": np.zeros(0, np.int64),
            "via": np.zeros(0, np.uint8), "drops": 0}


class FlowGrouper:
    def __init__(self, engine):
        self.engine = engine
        self._tm = TraceMapper(engine)     # window, scan and id hydration
        # when set, the GPU path records per-kernel milliseconds here
        # (benchmarks/flow_groups.py); costs one event pair per launch
        self.kernel_ms: Optional[Dict[str, float]] = None

    # ------------------------------------------------------------ plumbing
    def _gpu_run(self, segs, bases, lo: int, hi: int, fold: bool):
        from ..ops import gpu_ops
        dev = segs[0].u64.device
        ws = _FlowWorkspace(int(bases[-1]), dev)
        with _timed_launches(self.kernel_ms) as mark:
            for seg, base in zip(segs, bases):
                gpu_ops.flow_extract(seg, int(base), lo, hi, ws)
            mark("extract")
            gpu_ops.flow_union(ws)
            mark("union")
            gpu_ops.flow_flatten(ws)
            mark("flatten")
            if fold:
                gpu_ops.flow_fold(ws)
                mark("fold")
        return ws

    def _host_flat(self, segs, lo, hi) -> _Flat:
        return _Flat(segs, self.engine.pipe.time_base_s, lo, hi)

    # -------------------------------------------------------------- public
    def link_groups(self, time_start=None, time_end=None) -> Dict:
        """Arrays over participating rows in global-row order: row, group
        (the lowest row of the row's group), via (bit r = joined through
        key space r), and the index overflow count `drops`."""
        lo, hi = self._tm._window(time_start, time_end)
        with self.engine.lock:
            try:
                segs, bases = self._tm._scan(lo, hi)
                if not segs:
                    return _empty_links()
                if self._tm._on_gpu():
                    ws = self._gpu_run(segs, bases, lo, hi, fold=False)
                    rows = torch.nonzero(ws.part).view(-1)
                    packed = torch.stack([
                        rows, ws.group[rows].to(torch.int64) & M32,
                        ws.via[rows].to(torch.int64)]).cpu().numpy()
                    return {"row": packed[0], "group": packed[1],
                            "via": packed[2].astype(np.uint8),
                            "drops": int(ws.drops.item())}
                f = self._host_flat(segs, lo, hi)
                rows, group, via = _host_union(f)
                return {"row": rows.astype(np.int64), "group": group[rows],
                        "via": via[rows], "drops": 0}
            finally:
                self.engine.pipe.segments.release_scratch()

    def flow_groups(self, time_start=None, time_end=None,
                    min_spans: int = 2) -> Dict:
        """One summary per group of at least `min_spans` spans, sorted by
        (start_time, group_row); group_count and span_count cover the
        groups returned."""
        lo, hi = self._tm._window(time_start, time_end)
        min_spans = max(int(min_spans), 1)
        with self.engine.lock:
            try:
                segs, bases = self._tm._scan(lo, hi)
                if not segs:
                    return {"groups": [], "group_count": 0, "span_count": 0,
                            "drops": 0}
                if self._tm._on_gpu():
                    ws = self._gpu_run(segs, bases, lo, hi, fold=True)
                    gid, gv, drops = self._read_gpu_table(ws, min_spans)
                else:
                    f = self._host_flat(segs, lo, hi)
                    rows, group, via = _host_union(f)
                    gid, gv = _host_fold(f, rows, group, via)
                    keep = gv[:, GV_SPANS] >= np.uint64(min_spans)
                    gid, gv, drops = gid[keep], gv[keep], 0
                return self._finish(segs, bases, gid, gv, drops)
            finally:
                self.engine.pipe.segments.release_scratch()

    def flow_trace(self, time_start=None, time_end=None, *,
                   trace_id: Optional[str] = None,
                   syscall_trace_id: Optional[int] = None,
                   x_request_id: Optional[str] = None,
                   limit: int = 10000) -> Dict:
        """The group of the lowest participating row that emits the seed
        key: its spans in row order, at most `limit` of them."""
        seeds = [(k, v) for k, v in (("trace", trace_id),
                                     ("syscall", syscall_trace_id),
                                     ("xreq", x_request_id))
                 if v is not None]
        if len(seeds) != 1:
            raise ValueError("flow_trace takes exactly one of trace_id, "
                             "syscall_trace_id, x_request_id")
        kind, val = seeds[0]
        if kind == "trace":
            cols, key = ("tkey",), trace_key_of(str(val)) if val else 0
        elif kind == "syscall":
            cols, key = ("sreq", "sresp"), int(val) & U64MAX
        else:
            cols, key = ("x0", "x1"), xreq_key_of(str(val)) if val else 0
        empty = {"group_row": None, "span_count": 0, "truncated": False,
                 "spans": []}
        lo, hi = self._tm._window(time_start, time_end)
        limit = max(int(limit), 0)
        with self.engine.lock:
            try:
                segs, bases = self._tm._scan(lo, hi)
                if not segs or key == 0:
                    return empty
                if self._tm._on_gpu():
                    ws = self._gpu_run(segs, bases, lo, hi, fold=False)
                    part = ws.part != 0
                    k = torch.tensor(key - (1 << 64) if key >> 63 else key,
                                     dtype=torch.int64, device=ws.part.device)
                    hit = torch.zeros_like(part)
                    for c in cols:
                        hit |= getattr(ws, c) == k
                    hit = torch.nonzero(hit & part).view(-1)
                    if hit.numel() == 0:
                        return empty
                    grp = ws.group[hit[0]]
                    members = torch.nonzero((ws.group == grp) & part) \
                        .view(-1).cpu().numpy()
                    grp = int(grp.item()) & M32
                else:
                    f = self._host_flat(segs, lo, hi)
                    rows, group, _ = _host_union(f)
                    hit = np.zeros(f.n, dtype=bool)
                    for c in cols:
                        hit |= getattr(f, c) == np.uint64(key)
                    hit = np.nonzero(hit & (f.part != 0))[0]
                    if len(hit) == 0:
                        return empty
                    grp = int(group[hit[0]])
                    members = rows[group[rows] == grp]
                spans = [self._fetch_span(segs, bases, int(g))
                         for g in members[:limit].tolist()]
                return {"group_row": grp, "span_count": int(len(members)),
                        "truncated": len(members) > limit, "spans": spans}
            finally:
                self.engine.pipe.segments.release_scratch()

    # ------------------------------------------------------------- tables
    def _fetch_span(self, segs, bases, g: int) -> Dict:
        si = int(np.searchsorted(bases, g, side="right")) - 1
        local = g - int(bases[si])
        return {c: self.engine._fetch(segs[si], local, c, L7_TAGS,
                                      S.STR_COLS) for c in SPAN_COLS}

    @staticmethod
    def _read_gpu_table(ws: _FlowWorkspace, min_spans: int = 1):
        # one compaction + one D2H; group ids are rows, so ascending
        sel = torch.nonzero(ws.gvals[:, GV_SPANS] >= min_spans).view(-1)
        pack = torch.cat([sel.view(-1, 1), ws.gvals[sel]], dim=1) \
            .cpu().numpy()
        return pack[:, 0], pack[:, 1:].view(np.uint64), \
            int(ws.drops.item())

    def _finish(self, segs, bases, gid, gv, drops: int) -> Dict:
        first = gv[:, GV_FIRST_TRACED_ROW]
        traced = np.nonzero(first != np.uint64(U64MAX))[0]
        ids = self._tm._trace_ids(segs, bases,
                                  first[traced].astype(np.int64))
        tid = dict(zip(traced.tolist(), ids))
        groups = []
        for i, g in enumerate(gid.tolist()):
            v = gv[i].tolist()
            groups.append({
                "group_row": g,
                "span_count": v[GV_SPANS],
                "traced_spans": v[GV_TRACED],
                "error_count": v[GV_ERRORS],
                "start_time": v[GV_START_MIN],
                "end_time": v[GV_END_MAX],
                "via_trace": v[GV_VIA_TRACE],
                "via_syscall": v[GV_VIA_SYSCALL],
                "via_tcp": v[GV_VIA_TCP],
                "via_xreq": v[GV_VIA_XREQ],
                "trace_id": tid.get(i, ""),
            })
        groups.sort(key=lambda t: (t["start_time"], t["group_row"]))
        return {"groups": groups, "group_count": len(groups),
                "span_count": sum(t["span_count"] for t in groups),
                "drops": drops}
