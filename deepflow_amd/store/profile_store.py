"""GPU-resident continuous-profiling store (K9).

Same shape as the rest of the data plane: folded-stack lines are parsed by
a HIP kernel, each stack is interned into a slot-index dictionary whose
bytes live in a device pool, rows are four HBM columns, and a flame query
is two kernels (per-stack sums, then a fold of the selected stacks into a
per-query node table). The host store in ingest/profile_pipeline.py stays
the default and is the oracle for this one.

Host work: per *message* at ingest (series interning), per *tree node* at
query time. Nothing on the host is per line, per row or per frame x row.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

SERIES_FIELDS = ("event_type", "pid", "tid", "pod_id", "process_name",
                 "app_service", "profile_language_type")

_WS = np.zeros(256, dtype=bool)
_WS[[9, 10, 11, 12, 13, 32]] = True      # what bytes.strip() strips

STACK_ID_INVALID = 0xFFFFFFFF
POOL_LIMIT = 1 << 32                     # node frame offsets are u32


def split_lines(buf: np.ndarray, msg_start: np.ndarray,
                folded: np.ndarray
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Vectorised line splitter over a batch of concatenated blobs.

    buf is the u8 concatenation, message k owns
    buf[msg_start[k]:msg_start[k+1]], folded[k] says whether it is in a
    collapsed ("stack count" lines) format. Returns (line_off u64,
    line_len u32, line_msg u32, parse u8[n_msg]) with exactly the lines
    ProfilePipeline.ingest_profile would add, in its order:

    - a folded blob that holds a newline, or a space inside its stripped
      text, is cut at \\n, \\r and \\r\\n as bytes.splitlines() does, every
      line is stripped of ASCII whitespace and empty lines are skipped
      (parse[k] = 1: the kernel looks for a trailing count);
    - any other non-empty folded blob, and every non-folded blob (even an
      empty one), is a single unstripped line (parse[k] = 0).
    """
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    msg_start = np.asarray(msg_start, dtype=np.int64)
    folded = np.asarray(folded, dtype=bool)
    starts, ends = msg_start[:-1], msg_start[1:]
    n = int(buf.shape[0])
    # every byte of interest is <= 32: one cheap compare over the buffer,
    # everything after it works on the (few) candidates or on the lines
    C = np.flatnonzero(buf <= 32)
    cb = buf[C]
    W = C[_WS[cb]]                      # whitespace positions, sorted
    NL = C[cb == 10]
    SP = C[cb == 32]
    if W.size:
        # [run_lo, run_hi) of the whitespace run each W belongs to
        cut = np.flatnonzero(np.diff(W) != 1) + 1
        head = np.concatenate(([0], cut))
        size = np.diff(np.concatenate((head, [W.size])))
        run_lo = np.repeat(W[head], size)
        run_hi = run_lo + np.repeat(size, size)

    def trim(s, e):
        """[s, e) -> the same ranges without ASCII whitespace at either
        end; an all-blank or empty range comes back with first >= last."""
        if not W.size:
            return s, e
        i = np.minimum(np.searchsorted(W, s), W.size - 1)
        first = np.where(W[i] == s, run_hi[i], s)
        j = np.minimum(np.searchsorted(W, e - 1), W.size - 1)
        last = np.where((e > s) & (W[j] == e - 1), run_lo[j], e)
        return first, last

    first, last = trim(starts, ends)
    has_nl = np.searchsorted(NL, ends) > np.searchsorted(NL, starts)
    inner_sp = (first < last) & (np.searchsorted(SP, last)
                                 > np.searchsorted(SP, first))
    parse = folded & (has_nl | inner_sp)
    raw = ~parse & (~folded | (ends > starts))

    # parse-mode lines: one candidate per message start and per break,
    # ending at the next break or at the message end, then trimmed
    pm = np.flatnonzero(parse)
    B = C[(cb == 10) | (cb == 13)]
    mB = np.searchsorted(ends, B, side="right")     # message of a break
    keep = parse[mB] if B.size else np.zeros(0, dtype=bool)
    B, mB = B[keep], mB[keep]
    s = np.concatenate((starts[pm], B + 1))
    l_msg = np.concatenate((pm, mB))
    e = ends[l_msg]
    if B.size:
        nb = np.searchsorted(B, s)
        e = np.minimum(e, B[np.minimum(nb, B.size - 1)]
                       + (nb >= B.size) * n)
    l_off, l_end = trim(s, e)
    keep = l_off < l_end
    l_off, l_len, l_msg = l_off[keep], (l_end - l_off)[keep], l_msg[keep]

    r = np.flatnonzero(raw)
    l_off = np.concatenate((l_off, starts[r]))
    l_len = np.concatenate((l_len, ends[r] - starts[r]))
    l_msg = np.concatenate((l_msg, r))
    order = np.argsort(l_msg * (n + 1) + l_off, kind="stable")
    l_off, l_len, l_msg = l_off[order], l_len[order], l_msg[order]
    return (l_off.astype(np.uint64), l_len.astype(np.uint32),
            l_msg.astype(np.uint32), parse.astype(np.uint8))


def _pow2_at_least(x: int) -> int:
    return 1 << max(int(x) - 1, 0).bit_length()


class GpuProfileStore:
    """Row columns + stack dictionary + stack byte pool in HBM."""

    def __init__(self, device: str = "cuda", stack_capacity: int = 1 << 20,
                 row_capacity: int = 1 << 16,
                 pool_capacity: int = 1 << 20):
        import torch
        if stack_capacity < 1 or stack_capacity & (stack_capacity - 1):
            raise ValueError("stack_capacity must be a power of two")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GpuProfileStore needs a GPU device")
        from ..ops import native
        self._root_key = int(native.gpu().df_prof_root_key())
        dev = self.device
        self.stack_capacity = stack_capacity
        # stack dictionary: id == slot index; EMPTY_KEY = 0
        self.tkeys = torch.zeros(stack_capacity, dtype=torch.int64,
                                 device=dev)
        self.stack_off = torch.zeros(stack_capacity, dtype=torch.int64,
                                     device=dev)
        self.stack_len = torch.zeros(stack_capacity, dtype=torch.int32,
                                     device=dev)
        self.stack_frames = torch.zeros(stack_capacity, dtype=torch.int32,
                                        device=dev)
        self.pool = torch.zeros(max(pool_capacity, 16), dtype=torch.uint8,
                                device=dev)
        self.pool_len = torch.zeros(1, dtype=torch.int64, device=dev)
        self.drops = torch.zeros(1, dtype=torch.int64, device=dev)
        self._pool_upper = 0     # host upper bound on pool_len
        self._alloc_rows(max(row_capacity, 1))
        self.n_rows = 0
        # host-side series table, interned once per message
        self._series_id: Dict[tuple, int] = {}
        self._series: List[tuple] = []
        self._series_rows = np.zeros(0, dtype=np.int64)

    # ------------------------------------------------------------ storage
    def _alloc_rows(self, cap: int) -> None:
        import torch
        dev = self.device
        self.row_capacity = cap
        self.row_ts = torch.empty(cap, dtype=torch.int64, device=dev)
        self.row_val = torch.empty(cap, dtype=torch.int64, device=dev)
        self.row_stack = torch.empty(cap, dtype=torch.int32, device=dev)
        self.row_series = torch.empty(cap, dtype=torch.int32, device=dev)

    def _reserve_rows(self, need: int) -> None:
        if need <= self.row_capacity:
            return
        cap = self.row_capacity
        while cap < need:
            cap *= 2
        old = (self.row_ts, self.row_val, self.row_stack, self.row_series)
        self._alloc_rows(cap)
        n = self.n_rows
        for dst, src in zip((self.row_ts, self.row_val, self.row_stack,
                             self.row_series), old):
            dst[:n] = src[:n]

    def _reserve_pool(self, batch_bytes: int) -> None:
        import torch
        if self._pool_upper + batch_bytes <= self.pool.numel():
            return
        # the bound drifts up by every batch's bytes; tighten it with the
        # device's own counter before paying for a bigger pool
        self._pool_upper = int(self.pool_len.item())
        need = self._pool_upper + batch_bytes
        cap = self.pool.numel()
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        if cap > POOL_LIMIT:
            raise MemoryError("profile stack pool would exceed 4 GiB")
        pool = torch.zeros(cap, dtype=torch.uint8, device=self.device)
        pool[:self._pool_upper] = self.pool[:self._pool_upper]
        self.pool = pool

    def _intern_series(self, key: tuple) -> int:
        i = self._series_id.get(key)
        if i is None:
            i = len(self._series)
            self._series_id[key] = i
            self._series.append(key)
        return i

    # ------------------------------------------------------------- ingest
    def ingest_batch(self, blobs: Sequence[bytes],
                     metas: Sequence[Dict]) -> int:
        """One H2D copy + one k_prof_ingest launch for a batch of Profile
        messages. blobs[k] is the (decompressed) data of message k;
        metas[k] = {"ts", "count", "folded", "series"} where series is the
        SERIES_FIELDS tuple. Returns the number of rows appended."""
        import torch
        from ..ops import gpu_ops
        n_msg = len(blobs)
        if n_msg == 0:
            return 0
        msg_start = np.zeros(n_msg + 1, dtype=np.int64)
        np.cumsum([len(b) for b in blobs], out=msg_start[1:])
        buf = np.frombuffer(b"".join(blobs), dtype=np.uint8)
        folded = np.fromiter((m["folded"] for m in metas), dtype=bool,
                             count=n_msg)
        line_off, line_len, line_msg, parse = split_lines(
            buf, msg_start, folded)
        n_lines = int(line_off.shape[0])
        msg_series = np.fromiter(
            (self._intern_series(m["series"]) for m in metas),
            dtype=np.uint32, count=n_msg)
        if self._series_rows.shape[0] < len(self._series):
            self._series_rows = np.concatenate((
                self._series_rows,
                np.zeros(len(self._series) - self._series_rows.shape[0],
                         dtype=np.int64)))
        if n_lines == 0:
            return 0
        np.add.at(self._series_rows, msg_series[line_msg], 1)
        msg_ts = np.fromiter((m["ts"] for m in metas), dtype=np.int64,
                             count=n_msg)
        msg_count = np.fromiter((m["count"] for m in metas),
                                dtype=np.int64, count=n_msg)

        # one staging buffer, 16-byte aligned sections, one H2D copy
        parts = (line_off, msg_ts, msg_count, line_len, line_msg,
                 msg_series, parse, buf)
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += (a.nbytes + 15) & ~15
        stage = np.zeros(max(total, 16), dtype=np.uint8)
        for a, o in zip(parts, offs):
            stage[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        dstage = torch.from_numpy(stage).to(self.device)

        def sect(k, dtype):
            return dstage[offs[k]:offs[k] + parts[k].nbytes].view(dtype)

        self._reserve_rows(self.n_rows + n_lines)
        self._reserve_pool(int(buf.shape[0]))
        gpu_ops.prof_ingest(
            sect(7, torch.uint8), sect(0, torch.int64),
            sect(3, torch.int32), sect(4, torch.int32),
            sect(1, torch.int64), sect(2, torch.int64),
            sect(5, torch.int32), sect(6, torch.uint8),
            self, self.n_rows)
        self._pool_upper += int(buf.shape[0])
        self.n_rows += n_lines
        return n_lines

    # -------------------------------------------------------------- query
    def _series_mask(self, event_type: Optional[int],
                     process_name: Optional[str]) -> np.ndarray:
        ok = np.ones(len(self._series), dtype=np.uint8)
        for i, s in enumerate(self._series):
            if event_type is not None and s[0] != event_type:
                ok[i] = 0
            elif process_name is not None and s[4] != process_name:
                ok[i] = 0
        return ok

    def flame(self, event_type: Optional[int] = None,
              process_name: Optional[str] = None,
              time_start: int = 0, time_end: int = 1 << 62) -> Dict:
        """Same dict shape as build_flame; children ordered by
        (-value, name). Frames whose bytes differ stay separate nodes even
        if they decode (utf-8, "replace") to the same text."""
        import torch
        from ..ops import gpu_ops
        root = {"name": "root", "value": 0, "self": 0, "children": []}
        if self.n_rows == 0 or not self._series:
            return root
        dev = self.device
        lim = (1 << 63) - 1
        t0 = max(-lim - 1, min(lim, int(time_start)))
        t1 = max(-lim - 1, min(lim, int(time_end)))
        ok = torch.from_numpy(
            self._series_mask(event_type, process_name)).to(dev)
        cap = self.stack_capacity
        sums = torch.zeros(cap, dtype=torch.int64, device=dev)
        hit = torch.zeros(cap, dtype=torch.uint8, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        gpu_ops.prof_stack_sums(self, self.n_rows, ok, t0, t1, sums, hit,
                                total)
        # exact upper bound on tree nodes: frames of the selected stacks
        bound = int((self.stack_frames.to(torch.int64)
                     * hit.to(torch.int64)).sum().item())
        if bound == 0:
            return root
        ncap = max(_pow2_at_least(2 * bound), 64)
        nkeys = torch.zeros(ncap, dtype=torch.int64, device=dev)
        nparent = torch.zeros(ncap, dtype=torch.int64, device=dev)
        noff = torch.zeros(ncap, dtype=torch.int32, device=dev)
        nlen = torch.zeros(ncap, dtype=torch.int32, device=dev)
        ndepth = torch.zeros(ncap, dtype=torch.int32, device=dev)
        ntotal = torch.zeros(ncap, dtype=torch.int64, device=dev)
        nself = torch.zeros(ncap, dtype=torch.int64, device=dev)
        ndrops = torch.zeros(1, dtype=torch.int64, device=dev)
        gpu_ops.prof_flame_fold(self, hit, sums, nkeys, nparent, noff, nlen,
                                ndepth, ntotal, nself, ndrops)
        # compact occupied slots, pack frame names, one D2H copy
        idx = torch.nonzero(nkeys).reshape(-1)
        m = int(idx.numel())
        lens = nlen[idx].to(torch.int64)
        ends = torch.cumsum(lens, 0)
        name_bytes = int(ends[-1].item())
        names = torch.zeros(max(name_bytes, 1), dtype=torch.uint8,
                            device=dev)
        gpu_ops.gather_records(self.pool, noff, nlen,
                               idx.to(torch.int32), ends - lens, names)
        packed = torch.cat([
            torch.stack([nkeys[idx], nparent[idx], ntotal[idx], nself[idx],
                         ends, ndepth[idx].to(torch.int64)]).reshape(-1),
            ndrops, total]).view(torch.uint8)
        host = torch.cat([packed, names]).cpu().numpy()
        cols = host[:6 * m * 8].view(np.int64).reshape(6, m)
        n_drops, grand = (int(x) for x in
                          host[6 * m * 8:6 * m * 8 + 16].view(np.int64))
        if n_drops:
            raise RuntimeError(
                f"flame node table overflowed ({n_drops} stacks dropped)")
        blob = host[6 * m * 8 + 16:].tobytes()
        return self._link(cols, blob, grand)

    def _link(self, cols: np.ndarray, blob: bytes, grand: int) -> Dict:
        """Children -> parents by key; host work is per tree node."""
        keys = cols[0].view(np.uint64).tolist()
        parents = cols[1].view(np.uint64).tolist()
        totals, selfs, ends = (cols[i].tolist() for i in (2, 3, 4))
        root = {"name": "root", "value": grand, "self": 0, "children": []}
        by_key = {self._root_key: root}
        # a big tree is hundreds of thousands of small dicts: keep the
        # cycle collector from rescanning them all while they are built
        import gc
        was_on = gc.isenabled()
        gc.disable()
        try:
            start = 0
            for k, v, s, e in zip(keys, totals, selfs, ends):
                by_key[k] = {
                    "name": blob[start:e].decode("utf-8", "replace"),
                    "value": v, "self": s, "children": []}
                start = e
            for k, p in zip(keys, parents):
                by_key[p]["children"].append(by_key[k])
            for node in by_key.values():
                kids = node["children"]
                if len(kids) > 1:
                    kids.sort(key=lambda c: (-c["value"], c["name"]))
        finally:
            if was_on:
                gc.enable()
        return root

    def processes(self) -> List[str]:
        return sorted({s[4] for s, n in zip(self._series, self._series_rows)
                       if n > 0})

    # ------------------------------------------------------- introspection
    @property
    def n_stacks(self) -> int:
        import torch
        return int(torch.count_nonzero(self.tkeys).item())

    @property
    def stack_drops(self) -> int:
        return int(self.drops.item())

    def stored_bytes(self) -> int:
        return self.n_rows * 24 + int(self.pool_len.item())

    def _materialise(self):
        """(rows, id_to_loc) as the host store keeps them. D2H of every
        column and the whole pool: for tests and debugging only. Rows whose
        stack was dropped by a full table are left out; location ids are
        dense, in first-seen order."""
        from ..ingest.profile_pipeline import ProfileRow
        n = self.n_rows
        ts = self.row_ts[:n].cpu().numpy()
        val = self.row_val[:n].cpu().numpy()
        sid = self.row_stack[:n].cpu().numpy().view(np.uint32)
        ser = self.row_series[:n].cpu().numpy()
        off = self.stack_off.cpu().numpy()
        ln = self.stack_len.cpu().numpy()
        pool = self.pool[:int(self.pool_len.item())].cpu().numpy()
        dense: Dict[int, int] = {}
        id_to_loc: List[bytes] = []
        rows = []
        for t, v, s, r in zip(ts.tolist(), val.tolist(), sid.tolist(),
                              ser.tolist()):
            if s == STACK_ID_INVALID:
                continue
            lid = dense.get(s)
            if lid is None:
                lid = dense[s] = len(id_to_loc)
                id_to_loc.append(
                    pool[off[s]:off[s] + ln[s]].tobytes())
            rows.append(ProfileRow(
                timestamp=t, location_id=lid, value=v,
                **dict(zip(SERIES_FIELDS, self._series[r]))))
        return rows, id_to_loc

    @property
    def rows(self):
        return self._materialise()[0]

    @property
    def id_to_loc(self) -> List[bytes]:
        return self._materialise()[1]

