"""GPU-resident application-log store with substring (K11) and regex
(K13) search.

The pool is the raw payload: every batch's bytes are appended to a growable
HBM byte pool unchanged, a HIP kernel parses one line per thread into row
columns that point back into the pool, and a query is a flat scan of the
pool (k_log_scan), a per-row filter (k_log_select), one compaction, one
gather and one D2H copy. A regex is compiled on the host to a DFA
(query/logregex.py) and walked from every pool position by k_log_regex,
between the scan and the select. patterns() (K14) groups the selected rows
by the template of their body with one more kernel, k_log_patterns, and
brings only the top groups' newest rows to the host. The host store in
ingest/applog_pipeline.py stays the default and is the oracle for this one.

Host work: per *batch* at ingest (vectorised line split), per *hit* at
query time. OTLP rows keep their extra keys (trace_id, attr.*, ...) in a
host map; that path is already per record in Python.

Known divergences from the host path:
- non-ASCII Unicode whitespace at line edges is not stripped (bytes 9-13,
  28-31 and 32 are, which is all str.strip() removes in ASCII);
- timestamps of 19 or more digits fall back to free-form;
- non-ASCII digits are not digits;
- substring search is on bytes, which equals str search for valid UTF-8
  only (needles are at most 128 bytes, at most 8 per query);
- regex search is Python `re` on the pool's bytes (the host store's
  body.encode("utf-8", "replace") for valid UTF-8 only, as above) for a
  subset of its syntax (query/logregex.py lists it): one pattern of at
  most 256 bytes per query, whose DFA fits 32 KiB; no backreferences,
  look-around or \\b, and no
  required-literal prefilter or index, so a pattern such as `e.*zzz` walks
  from every `e` to the end of its row. The host store refuses exactly the
  patterns this one refuses;
- patterns() (K14, query/logpattern.py) takes the template from the pool's
  bytes, not from a str: equal to the host store's
  body.encode("utf-8", "replace") for valid UTF-8 only. Only the first 512
  bytes of a body count on either store. Patterns are told apart by a
  64-bit key here and by the symbol tuple on the host: two templates with
  one key would be counted as one. The query-scoped table has max_patterns
  slots (a power of two, default 65536); a pattern that finds it full
  loses all of its rows to dropped_rows, which the host store never does,
  and has probed every slot to find that out, so the table is to be sized
  above the number of patterns expected;
- severity is stored as a u8, the pool is limited to 4 GiB, and a row
  whose app name found the app table full reads back with
  app_service "" and app_id -1 (`drops` counts them);
- retention by bytes exists here only. max_pool_bytes bounds pool_len (the
  payload bytes as they arrived, headers and line breaks included, plus
  the names of apps whose first row is gone), not the bodies: before a
  batch of nb bytes is appended and would pass the limit, the oldest rows
  go until pool_len <= min(floor(max_pool_bytes * keep_fraction),
  max_pool_bytes - nb). The cut falls on a row boundary rounded down to 16
  bytes and the room is judged with an upper bound for the names, so a few
  more rows than strictly needed may go. A batch larger than the limit is
  a ValueError; ingest_rows makes room per run of equal (agent_id,
  log_type), so such a run fails after the runs before it were stored.

Retention (evict_rows, evict_before, max_rows, as on the host store, and
max_pool_bytes) drops oldest-inserted rows by compacting the store on the
device into a fresh pool and fresh columns (k_log_evict in dflog.hip).
Apps are never dropped; the name of an app whose claiming row is gone moves
to an arena at the front of the new pool, below the first body, where the
scans attribute bytes to no row.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..ingest.applog_pipeline import (check_regex, check_retention,
                                      fold_ascii, hist_buckets,
                                      norm_needles, rows_to_evict)
from .dictionary import str_hash_py

APP_ID_INVALID = 0xFFFFFFFF
POOL_LIMIT = 1 << 32                 # k_gather_records offsets are u32
MAX_NEEDLE_BYTES = 128
CORE_KEYS = ("time", "agent_id", "log_type", "severity", "app_service",
             "app_id", "body")

_WS = np.zeros(256, dtype=bool)
_WS[[9, 10, 11, 12, 13, 28, 29, 30, 31, 32]] = True   # ASCII str.strip()


def split_log_lines(buf: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(line_off i64, line_len i32) of the lines AppLogPipeline.ingest_lines
    would keep, in its order: buf is cut at \\n, \\r and \\r\\n as
    bytes.splitlines() does, every line is stripped of the ASCII bytes
    str.strip() removes (9-13, 28-31, 32) and empty lines are skipped."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    n = int(buf.shape[0])
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32)
    # every byte of interest is <= 32: one compare over the buffer, the
    # rest works on the (few) candidates or on the lines
    C = np.flatnonzero(buf <= 32)
    cb = buf[C]
    W = C[_WS[cb]]                          # whitespace positions, sorted
    B = C[(cb == 10) | (cb == 13)]          # line breaks
    # \r\n leaves an empty line between the two bytes; it is dropped below
    s = np.concatenate(([0], B + 1))
    e = np.concatenate((B, [n]))
    if W.size:
        # [run_lo, run_hi) of the whitespace run each W belongs to
        cut = np.flatnonzero(np.diff(W) != 1) + 1
        head = np.concatenate(([0], cut))
        size = np.diff(np.concatenate((head, [W.size])))
        run_lo = np.repeat(W[head], size)
        run_hi = run_lo + np.repeat(size, size)
        i = np.minimum(np.searchsorted(W, s), W.size - 1)
        first = np.where(W[i] == s, run_hi[i], s)
        j = np.minimum(np.searchsorted(W, e - 1), W.size - 1)
        last = np.where((e > s) & (W[j] == e - 1), run_lo[j], e)
    else:
        first, last = s, e
    keep = first < last
    return (first[keep].astype(np.int64),
            (last - first)[keep].astype(np.int32))


def _pad16(x: int) -> int:
    return (int(x) + 15) & ~15


class GpuLogStore:
    """Row columns + app dictionary + raw payload pool in HBM."""

    def __init__(self, device: str = "cuda", row_capacity: int = 1 << 16,
                 pool_capacity: int = 1 << 22, app_capacity: int = 1 << 12,
                 max_rows: Optional[int] = None,
                 max_pool_bytes: Optional[int] = None,
                 keep_fraction: float = 0.5):
        import torch
        if app_capacity < 1 or app_capacity & (app_capacity - 1):
            raise ValueError("app_capacity must be a power of two")
        check_retention(max_rows, keep_fraction)
        if max_pool_bytes is not None:
            if max_pool_bytes < 1:
                raise ValueError("max_pool_bytes must be >= 1")
            if max_pool_bytes > POOL_LIMIT:
                raise ValueError("max_pool_bytes is at most 4 GiB")
            pool_capacity = min(pool_capacity, max_pool_bytes)
        self.max_rows = max_rows
        self.max_pool_bytes = max_pool_bytes
        self.keep_fraction = keep_fraction
        self.evicted_rows = 0
        self.evictions = 0
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("GpuLogStore needs a GPU device")
        from ..ops import native
        lib = native.gpu()
        self._app_seed = int(lib.df_log_app_seed())
        dev = self.device
        # app dictionary: id == slot index; EMPTY_KEY = 0. The claimer
        # records where its own token lies in the pool: no byte copy.
        self.app_capacity = app_capacity
        self.tkeys = torch.zeros(app_capacity, dtype=torch.int64, device=dev)
        self.app_off = torch.zeros(app_capacity, dtype=torch.int64,
                                   device=dev)
        self.app_len = torch.zeros(app_capacity, dtype=torch.int32,
                                   device=dev)
        self.drops = torch.zeros(1, dtype=torch.int64, device=dev)
        # the scan kernel loads 16 bytes at a time: the capacity stays a
        # multiple of 16 and the base is the allocator's (>= 256-aligned)
        self.pool = torch.zeros(max(_pad16(pool_capacity), 16),
                                dtype=torch.uint8, device=dev)
        assert self.pool.data_ptr() % 16 == 0
        self.pool_len = 0
        self._alloc_rows(max(row_capacity, 1))
        self.n_rows = 0
        self._log_types: List[str] = []
        self._log_type_id: Dict[str, int] = {}
        self._extras: Dict[int, Dict] = {}      # row index -> extra keys
        # slot -> dense first-seen app id, extended lazily at query time
        self._dense: Dict[int, int] = {}
        self._dense_rows = 0

    # ------------------------------------------------------------ storage
    _COLS = (("row_time", "int64"), ("row_sev", "uint8"),
             ("row_agent", "int32"), ("row_type", "int16"),
             ("row_app", "int32"), ("row_boff", "int64"),
             ("row_blen", "int32"))

    def _alloc_rows(self, cap: int) -> None:
        import torch
        self.row_capacity = cap
        for name, dt in self._COLS:
            setattr(self, name, torch.empty(cap, dtype=getattr(torch, dt),
                                            device=self.device))

    def _reserve_rows(self, need: int) -> None:
        if need <= self.row_capacity:
            return
        cap = self.row_capacity
        while cap < need:
            cap *= 2
        old = [getattr(self, name) for name, _ in self._COLS]
        self._alloc_rows(cap)
        n = self.n_rows
        for (name, _), src in zip(self._COLS, old):
            getattr(self, name)[:n] = src[:n]

    def _reserve_pool(self, batch_bytes: int) -> None:
        import torch
        need = self.pool_len + batch_bytes
        cap = self.pool.numel()
        if need <= cap:
            return
        while cap < need:
            cap *= 2
        if self.max_pool_bytes is not None:
            # _make_room saw to it that need <= max_pool_bytes
            cap = min(cap, _pad16(self.max_pool_bytes))
            assert need <= cap
        if cap > POOL_LIMIT:
            raise MemoryError("log pool would exceed 4 GiB")
        pool = torch.zeros(cap, dtype=torch.uint8, device=self.device)
        pool[:self.pool_len] = self.pool[:self.pool_len]
        assert pool.data_ptr() % 16 == 0
        self.pool = pool

    def _log_type(self, s: str) -> int:
        i = self._log_type_id.get(s)
        if i is None:
            i = len(self._log_types)
            if i >= 1 << 16:
                raise ValueError("too many distinct log types")
            self._log_type_id[s] = i
            self._log_types.append(s)
        return i

    # ------------------------------------------------------------- ingest
    def _ingest(self, buf: np.ndarray, line_off: np.ndarray,
                line_len: np.ndarray, now: int, agent_id: int,
                log_type: str, pre=None, extras=None) -> int:
        """One H2D copy, one D2D append of the payload to the pool, one
        k_log_ingest launch. With max_pool_bytes set, room is made first
        (_make_room). extras: {line index: extra keys}, recorded under the
        row indices the lines get."""
        import torch
        from ..ops import gpu_ops
        n_lines = int(line_off.shape[0])
        if n_lines == 0:
            return 0
        self._make_room(int(buf.shape[0]))
        for k, extra in (extras or {}).items():
            self._extras[self.n_rows + k] = extra
        parts = [line_off, line_len, buf]
        if pre is not None:
            parts += list(pre)
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += _pad16(a.nbytes)
        stage = np.zeros(max(total, 16), dtype=np.uint8)
        for a, o in zip(parts, offs):
            stage[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
        dstage = torch.from_numpy(stage).to(self.device)

        def sect(k, dtype):
            return dstage[offs[k]:offs[k] + parts[k].nbytes].view(dtype)

        nb = int(buf.shape[0])
        self._reserve_rows(self.n_rows + n_lines)
        self._reserve_pool(nb)
        base = self.pool_len
        self.pool[base:base + nb] = sect(2, torch.uint8)
        kw = {}
        if pre is not None:
            kw = {"pre_app_len": sect(3, torch.int32),
                  "pre_time": sect(4, torch.int64),
                  "pre_sev": sect(5, torch.uint8)}
        gpu_ops.log_ingest(self, base, sect(0, torch.int64),
                           sect(1, torch.int32), int(now),
                           int(agent_id) & 0xFFFFFFFF,
                           self._log_type(log_type), self.n_rows, **kw)
        self.pool_len += nb
        self.n_rows += n_lines
        return n_lines

    def ingest_lines(self, payload: bytes, agent_id: int = 0,
                     log_type: str = "system", now: int = 0) -> int:
        buf = np.frombuffer(bytes(payload), dtype=np.uint8)
        line_off, line_len = split_log_lines(buf)
        n = self._ingest(buf, line_off, line_len, now, agent_id, log_type)
        self._apply_row_rule()
        return n

    def ingest_rows(self, rows: List[Dict]) -> int:
        """Pre-parsed rows (OTLP). Rows are grouped into runs of equal
        (agent_id, log_type), one kernel launch per run; a batch from one
        exporter is one run."""
        n = 0
        i = 0
        while i < len(rows):
            key = (rows[i].get("agent_id", 0), rows[i].get("log_type", ""))
            j = i
            while j < len(rows) and \
                    (rows[j].get("agent_id", 0),
                     rows[j].get("log_type", "")) == key:
                j += 1
            n += self._ingest_row_run(rows[i:j], key[0], key[1])
            i = j
        self._apply_row_rule()
        return n

    def _ingest_row_run(self, rows: List[Dict], agent_id: int,
                        log_type: str) -> int:
        m = len(rows)
        chunks: List[bytes] = []
        app_len = np.zeros(m, dtype=np.int32)
        line_len = np.zeros(m, dtype=np.int32)
        times = np.zeros(m, dtype=np.int64)
        sevs = np.zeros(m, dtype=np.uint8)
        extras: Dict[int, Dict] = {}
        for k, r in enumerate(rows):
            app = str(r.get("app_service", "")).encode("utf-8", "replace")
            body = str(r["body"]).encode("utf-8", "replace")
            chunks.append(app)
            chunks.append(body)
            app_len[k] = len(app)
            line_len[k] = len(app) + len(body)
            times[k] = r["time"]
            sevs[k] = min(max(int(r["severity"]), 0), 255)
            extra = {key: v for key, v in r.items() if key not in CORE_KEYS}
            if extra:
                extras[k] = extra
        line_off = np.zeros(m, dtype=np.int64)
        np.cumsum(line_len[:-1], out=line_off[1:])
        buf = np.frombuffer(b"".join(chunks), dtype=np.uint8)
        return self._ingest(buf, line_off, line_len, 0, agent_id, log_type,
                            pre=(app_len, times, sevs), extras=extras)

    # ---------------------------------------------------------- retention
    def evict_rows(self, n: int) -> int:
        """Drop the min(n, n_rows) oldest-inserted rows; -> how many went.
        A device-side compaction into a fresh pool and fresh row columns
        (gpu_ops.log_evict): peak memory is old pool plus new pool. Apps are
        never forgotten: an app whose rows are all gone keeps its slot, its
        name (moved to the front of the new pool) and its app_id."""
        from ..ops import gpu_ops
        first = min(int(n), self.n_rows)
        if first <= 0:
            return 0
        # dense ids are first-seen order over *all* rows ever stored: bring
        # them up to date while the rows are still there
        self._dense_ids()
        gpu_ops.log_evict(self, first)
        self._extras = {r - first: e for r, e in self._extras.items()
                        if r >= first}
        self._dense_rows = self.n_rows
        self.evicted_rows += first
        self.evictions += 1
        return first

    def evict_before(self, t: int) -> int:
        """Drop the longest insertion-order prefix in which every row has
        time < t (times are not monotone in row index: the cut is the first
        row with time >= t, wherever older rows lie after it). The index is
        found on the device; one scalar goes to the host."""
        import torch
        n = self.n_rows
        if n == 0:
            return 0
        lim = (1 << 63) - 1
        t = max(-lim - 1, min(lim, int(t)))
        idx = torch.arange(n, device=self.device)
        first = torch.where(self.row_time[:n] >= t, idx,
                            torch.full_like(idx, n)).min()
        return self.evict_rows(int(first.item()))

    def _apply_row_rule(self) -> None:
        self.evict_rows(rows_to_evict(self.n_rows, self.max_rows,
                                      self.keep_fraction))

    def _make_room(self, nb: int) -> None:
        """The byte rule, before a batch of nb bytes is appended: when the
        pool would pass max_pool_bytes, evict the fewest oldest rows that
        bring pool_len down to min(floor(max_pool_bytes * keep_fraction),
        max_pool_bytes - nb). `first` is chosen on the device (one scalar
        to the host) from the non-decreasing cuts the rows would give, with
        the padded sum of all live app names as an upper bound for the
        arena; when no row set meets the target, everything goes."""
        import torch
        limit = self.max_pool_bytes
        if limit is None:
            return
        if nb > limit:
            raise ValueError(f"a batch of {nb} bytes does not fit "
                             f"max_pool_bytes={limit}")
        if self.pool_len + nb <= limit:
            return
        n = self.n_rows
        if n:
            target = min(int(limit * self.keep_fraction), limit - nb)
            live = self.tkeys != 0
            arena = (torch.sum(self.app_len.to(torch.int64) * live) + 15) \
                & ~15
            # new pool_len = arena + pool_len - cut(first) <= target
            need = arena + (self.pool_len - target)
            cuts = (self.row_boff[:n] + self.row_blen[:n]) & ~15
            # lines end in increasing order, so cuts is sorted; the last row
            # stands for "everything": its cut is the whole pool
            cuts[n - 1] = self.pool_len
            first = torch.clamp(torch.searchsorted(cuts, need.reshape(1)),
                                max=n - 1) + 1
            self.evict_rows(int(first.item()))
        if self.pool_len + nb > limit:
            raise MemoryError("the app names alone leave no room for the "
                              "batch under max_pool_bytes")

    # -------------------------------------------------------------- query
    def _dense_ids(self) -> Dict[int, int]:
        """slot -> dense app id in first-seen row order, as the host
        interner numbers them. Incremental: only rows added since the last
        call are looked at, on the device."""
        import torch
        lo, n = self._dense_rows, self.n_rows
        if lo < n:
            ids = self.row_app[lo:n].to(torch.int64) & 0xFFFFFFFF
            uniq, inv = torch.unique(ids, return_inverse=True)
            first = torch.full((uniq.numel(),), n, dtype=torch.int64,
                               device=self.device)
            first.scatter_reduce_(
                0, inv, torch.arange(n - lo, device=self.device),
                reduce="amin")
            host = torch.stack([uniq, first]).cpu().numpy()
            for k in np.argsort(host[1], kind="stable"):
                slot = int(host[0, k])
                if slot != APP_ID_INVALID and slot not in self._dense:
                    self._dense[slot] = len(self._dense)
            self._dense_rows = n
        return self._dense

    def _flags(self, substr, severity_max, time_start, time_end,
               app_service, case_insensitive, hist=None, interval=1,
               n_buckets=0, regex=None):
        """Scan + regex + select -> u8 flag per row (None: nothing can
        match)."""
        import torch
        from ..ops import gpu_ops
        rx = check_regex(regex, case_insensitive)
        needles = norm_needles(substr)
        if case_insensitive:
            needles = [fold_ascii(s) for s in needles]
        needles_b = [s.encode("utf-8") for s in needles]
        for s in needles_b:
            if len(s) > MAX_NEEDLE_BYTES:
                raise ValueError(
                    f"needles are at most {MAX_NEEDLE_BYTES} bytes")
        if self.n_rows == 0 or severity_max < 0:
            return None
        lim = (1 << 63) - 1
        t_lo = -lim - 1 if time_start is None else \
            max(-lim - 1, min(lim, int(time_start)))
        t_hi = lim if time_end is None else \
            max(-lim - 1, min(lim, int(time_end)))
        app_key = None
        if app_service is not None:
            app_key = str_hash_py(app_service.encode("utf-8"),
                                  self._app_seed)
        n = self.n_rows
        # query-scoped workspace: one u32 of needle bits and one flag per row
        mask = torch.zeros(n, dtype=torch.int32, device=self.device)
        flags = torch.empty(n, dtype=torch.uint8, device=self.device)
        gpu_ops.log_scan(self, needles_b, case_insensitive, mask)
        need = (1 << len(needles_b)) - 1
        # a pattern that matches the empty string somewhere in every body
        # constrains nothing; k_log_regex finds non-empty matches only
        if rx is not None and not rx.matches_everything:
            need |= gpu_ops.LOG_RE_BIT
            gpu_ops.log_regex(self, rx, mask)
            if rx.nullable:             # ^$, ^a*$: the empty bodies too
                mask |= (self.row_blen[:n] == 0).to(torch.int32) \
                    * gpu_ops.LOG_RE_BIT
        gpu_ops.log_select(self, mask, need,
                           min(int(severity_max), 255), t_lo, t_hi, app_key,
                           flags, hist, interval, n_buckets)
        return flags

    def search(self, substr: Union[str, Sequence[str]] = "",
               severity_max: int = 7, limit: int = 100, *,
               time_start: Optional[int] = None,
               time_end: Optional[int] = None,
               app_service: Optional[str] = None,
               case_insensitive: bool = False,
               regex: Optional[str] = None) -> List[Dict]:
        import torch
        flags = self._flags(substr, severity_max, time_start, time_end,
                            app_service, case_insensitive, regex=regex)
        if flags is None or limit <= 0:
            return []
        idx = torch.nonzero(flags).reshape(-1)
        if idx.numel() > limit:
            idx = idx[idx.numel() - limit:]
        return self._hydrate(torch.flip(idx, [0]))

    def _hydrate(self, idx) -> List[Dict]:
        """Rows idx (device i64) -> dicts: one gather of bodies and app
        names, one D2H copy, then per-hit work on the host."""
        import torch
        from ..ops import gpu_ops
        m = int(idx.numel())
        if m == 0:
            return []
        dev = self.device
        app = self.row_app[idx].to(torch.int64) & 0xFFFFFFFF
        valid = app < self.app_capacity
        slot = torch.where(valid, app, torch.zeros_like(app))
        offs = torch.cat([self.row_boff[idx], self.app_off[slot]])
        lens = torch.cat([self.row_blen[idx].to(torch.int64),
                          torch.where(valid,
                                      self.app_len[slot].to(torch.int64),
                                      torch.zeros_like(app))])
        ends = torch.cumsum(lens, 0)
        # u32 offsets for k_gather_records (the pool is at most 4 GiB)
        offs32 = torch.where(offs >= 1 << 31, offs - (1 << 32),
                             offs).to(torch.int32)
        blob = torch.zeros(max(int(ends[-1].item()), 1), dtype=torch.uint8,
                           device=dev)
        gpu_ops.gather_records(
            self.pool, offs32, lens.to(torch.int32),
            torch.arange(2 * m, dtype=torch.int32, device=dev),
            ends - lens, blob)
        cols = torch.stack([
            idx, self.row_time[idx], self.row_sev[idx].to(torch.int64),
            self.row_agent[idx].to(torch.int64) & 0xFFFFFFFF,
            self.row_type[idx].to(torch.int64) & 0xFFFF, app,
            ends[:m], ends[m:]]).reshape(-1)
        host = torch.cat([cols.view(torch.uint8), blob]).cpu().numpy()
        c = host[:8 * m * 8].view(np.int64).reshape(8, m)
        data = host[8 * m * 8:].tobytes()
        dense = self._dense_ids()
        out = []
        b0 = 0
        a0 = int(c[6, m - 1])
        for k in range(m):
            b1, a1 = int(c[6, k]), int(c[7, k])
            row = {
                "time": int(c[1, k]),
                "agent_id": int(c[3, k]),
                "log_type": self._log_types[int(c[4, k])],
                "severity": int(c[2, k]),
                "app_service": data[a0:a1].decode("utf-8", "replace"),
                "app_id": dense.get(int(c[5, k]), -1),
                "body": data[b0:b1].decode("utf-8", "replace"),
            }
            extra = self._extras.get(int(c[0, k]))
            if extra:
                row.update(extra)
            out.append(row)
            b0, a0 = b1, a1
        return out

    def histogram(self, interval: int, time_start: int, time_end: int,
                  substr: Union[str, Sequence[str]] = "",
                  severity_max: int = 7, *,
                  app_service: Optional[str] = None,
                  case_insensitive: bool = False,
                  regex: Optional[str] = None) -> List[Dict]:
        import torch
        check_regex(regex, case_insensitive)
        n_buckets = hist_buckets(interval, time_start, time_end)
        if n_buckets == 0:
            norm_needles(substr)
            return []
        hist = torch.zeros(n_buckets * 8, dtype=torch.int64,
                           device=self.device)
        flags = self._flags(substr, severity_max, time_start, time_end,
                            app_service, case_insensitive, hist=hist,
                            interval=int(interval), n_buckets=n_buckets,
                            regex=regex)
        if flags is None:
            return []
        cells = torch.nonzero(hist).reshape(-1)
        host = torch.stack([cells, hist[cells]]).cpu().numpy()
        return [{"time": int(time_start) + (cell // 8) * int(interval),
                 "severity": cell % 8, "count": cnt}
                for cell, cnt in zip(host[0].tolist(), host[1].tolist())]

    def patterns(self, substr: Union[str, Sequence[str]] = "",
                 severity_max: int = 7, limit: int = 20, *,
                 time_start: Optional[int] = None,
                 time_end: Optional[int] = None,
                 app_service: Optional[str] = None,
                 case_insensitive: bool = False,
                 regex: Optional[str] = None,
                 max_patterns: int = 1 << 16) -> Dict:
        """AppLogPipeline.patterns on this store: the flags of search(), one
        k_log_patterns launch into a query-scoped table of max_patterns
        slots, the top `limit` slots chosen on the device, their newest
        rows hydrated. Three scalars and `limit` rows come to the host."""
        import torch
        from ..ops import gpu_ops
        from ..query.logpattern import (check_max_patterns, render,
                                        template_symbols)
        check_regex(regex, case_insensitive)
        check_max_patterns(max_patterns)
        flags = self._flags(substr, severity_max, time_start, time_end,
                            app_service, case_insensitive, regex=regex)
        if flags is None:
            return {"matched": 0, "distinct": 0, "dropped_rows": 0,
                    "patterns": []}
        t = gpu_ops.log_patterns(self, flags, max_patterns)
        slots = torch.nonzero(t.count).reshape(-1)
        distinct = int(slots.numel())
        cnt = t.count[slots]
        first = t.first_row[slots].to(torch.int64) & 0xFFFFFFFF
        # count descending, ties by the lowest first row: two stable sorts.
        # A row has one pattern, so first rows are distinct and the order
        # does not depend on which slot a pattern landed in.
        order = torch.argsort(first, stable=True)
        order = order[torch.argsort(cnt[order], descending=True,
                                    stable=True)]
        top = order[:min(max(int(limit), 0), distinct)]
        last = t.last_row[slots[top]].to(torch.int64) & 0xFFFFFFFF
        host = torch.cat([flags.sum(dtype=torch.int64).reshape(1), t.drops,
                          cnt[top]]).cpu().tolist()
        out = []
        for n, row in zip(host[2:], self._hydrate(last)):
            sym = template_symbols(row["body"].encode("utf-8", "replace"))
            out.append({"pattern": render(sym), "count": n, "sample": row})
        return {"matched": host[0], "distinct": distinct,
                "dropped_rows": host[1], "patterns": out}

    # ------------------------------------------------------- introspection
    @property
    def app_drops(self) -> int:
        return int(self.drops.item())

    @property
    def n_apps(self) -> int:
        import torch
        return int(torch.count_nonzero(self.tkeys).item())

    def stored_bytes(self) -> int:
        return self.n_rows * 31 + self.pool_len

    def _materialise(self) -> List[Dict]:
        """Every row as the host store keeps it, oldest first. D2H of all
        columns and the whole pool."""
        n = self.n_rows
        if n == 0:
            return []
        boff = self.row_boff[:n].cpu().numpy()
        # k_log_scan finds a hit's row by binary search over body_off
        assert bool(np.all(boff[1:] >= boff[:-1])), \
            "body_off must be non-decreasing in row index"
        blen = self.row_blen[:n].cpu().numpy()
        ts = self.row_time[:n].cpu().numpy().tolist()
        sev = self.row_sev[:n].cpu().numpy().tolist()
        agent = self.row_agent[:n].cpu().numpy().view(np.uint32).tolist()
        ltype = self.row_type[:n].cpu().numpy().view(np.uint16).tolist()
        app = self.row_app[:n].cpu().numpy().view(np.uint32).tolist()
        a_off = self.app_off.cpu().numpy()
        a_len = self.app_len.cpu().numpy()
        pool = self.pool[:self.pool_len].cpu().numpy().tobytes()
        dense = self._dense_ids()
        names: Dict[int, str] = {}
        out = []
        for r in range(n):
            slot = app[r]
            if slot == APP_ID_INVALID:
                name = ""
            else:
                name = names.get(slot)
                if name is None:
                    name = names[slot] = pool[
                        a_off[slot]:a_off[slot] + a_len[slot]].decode(
                            "utf-8", "replace")
            row = {
                "time": ts[r],
                "agent_id": agent[r],
                "log_type": self._log_types[ltype[r]],
                "severity": sev[r],
                "app_service": name,
                "app_id": dense.get(slot, -1),
                "body": pool[boff[r]:boff[r] + blen[r]].decode(
                    "utf-8", "replace"),
            }
            extra = self._extras.get(r)
            if extra:
                row.update(extra)
            out.append(row)
        return out

    @property
    def rows(self) -> List[Dict]:
        return self._materialise()
