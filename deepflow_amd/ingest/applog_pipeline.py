"""Application log ingest (agent logs / syslog / OTLP logs -> queryable
rows with dict-encoded fields). Reference: server/ingester/app_log.

Wire: MSG_APPLICATION_LOG / MSG_SYSLOG / MSG_AGENT_LOG frames carrying
line-oriented or record payloads; OTLP logs arrive via the OTLP route.

device="cpu" (default): one dict per line on the host; this store is also
the oracle for the GPU one. device="cuda": store/log_store.py::GpuLogStore
keeps the payload bytes and the row columns in HBM and answers search() and
histogram() with HIP kernels (K11). Both take an optional regex (K13):
query/logregex.py validates it identically for either store; the host
store then matches with Python's `re` on bytes, the GPU store walks the
compiled DFA in k_log_regex. patterns() (K14) groups the matching rows by
the template of their body (query/logpattern.py, one definition for both
stores); the GPU store hashes the templates in k_log_patterns.

Retention: both stores drop oldest-inserted rows, by hand (evict_rows,
evict_before) or past max_rows; the GPU store also bounds its pool in bytes
and compacts itself on the device (k_log_evict). The host store stays the
exact oracle: fed the same calls, both hold the same rows.
"""
from __future__ import annotations

import time
from typing import Dict, List, Optional, Sequence, Union

from ..utils.stats import Counter

SEVERITIES = {"debug": 7, "info": 6, "warn": 4, "warning": 4, "error": 3,
              "fatal": 2, "critical": 2}

MAX_NEEDLES = 8
MAX_HIST_BUCKETS = 4096

_FOLD = {c: c + 32 for c in range(ord("A"), ord("Z") + 1)}


def fold_ascii(s: str) -> str:
    """Lower-case A-Z only (what the scan kernel does on bytes)."""
    return s.translate(_FOLD)


def norm_needles(substr: Union[str, Sequence[str]]) -> List[str]:
    """search()'s substr argument -> the non-empty needles (an empty
    needle matches every row, so it constrains nothing)."""
    needles = [substr] if isinstance(substr, str) else list(substr)
    if len(needles) > MAX_NEEDLES:
        raise ValueError(f"at most {MAX_NEEDLES} needles")
    for s in needles:
        if not isinstance(s, str):
            raise TypeError("needles are str")
    return [s for s in needles if s]


def check_regex(regex, case_insensitive: bool):
    """search()'s regex argument -> a compiled query.logregex.LogRegex, or
    None when it constrains nothing. Raises for what either store would
    refuse; both stores call it before anything else."""
    from ..query.logregex import check_log_regex
    return check_log_regex(regex, case_insensitive)


def hist_buckets(interval: int, time_start: int, time_end: int) -> int:
    if interval < 1:
        raise ValueError("interval must be >= 1")
    if time_end < time_start:
        return 0
    n = (time_end - time_start) // interval + 1
    if n > MAX_HIST_BUCKETS:
        raise ValueError(f"window holds {n} buckets "
                         f"(max {MAX_HIST_BUCKETS})")
    return n


def check_retention(max_rows, keep_fraction) -> None:
    if max_rows is not None and max_rows < 1:
        raise ValueError("max_rows must be >= 1")
    if not 0 < keep_fraction <= 1:
        raise ValueError("keep_fraction must be in (0, 1]")


def rows_to_evict(n_rows: int, max_rows, keep_fraction: float) -> int:
    """The row rule, applied by either store after a batch is appended:
    past max_rows, the oldest rows go until max(1, floor(max_rows *
    keep_fraction)) are left."""
    if max_rows is None or n_rows <= max_rows:
        return 0
    return n_rows - max(1, int(max_rows * keep_fraction))


def _body_bytes(r: Dict) -> int:
    return len(str(r.get("body", "")).encode("utf-8", "replace"))


class AppLogPipeline:
    """max_rows / keep_fraction: retention by row count, identical on both
    stores (rows_to_evict); both None-default limits mean an unbounded
    store. Other keywords go to the GPU store (store/log_store.py), which
    alone knows max_pool_bytes."""

    def __init__(self, counter: Optional[Counter] = None,
                 device: str = "cpu", *, max_rows: Optional[int] = None,
                 keep_fraction: float = 0.5, **store_kw):
        self.device = device
        self.gpu = not str(device).startswith("cpu")
        self._rows: List[Dict] = []
        # SmartEncoding for repetitive fields; never shrunk, so an app
        # whose rows were all evicted keeps its id
        self.app_interner: Dict[str, int] = {}
        self.counter = counter or Counter("ingester.app_log")
        check_retention(max_rows, keep_fraction)
        self.max_rows = max_rows
        self.keep_fraction = keep_fraction
        self._evicted_rows = 0
        self._evictions = 0
        if self.gpu:
            from ..store.log_store import GpuLogStore
            self.store = GpuLogStore(device=device, max_rows=max_rows,
                                     keep_fraction=keep_fraction, **store_kw)
        elif store_kw:
            raise TypeError(f"unexpected arguments for the host store: "
                            f"{sorted(store_kw)}")

    @property
    def rows(self) -> List[Dict]:
        """Every stored row, oldest first. On the GPU store this is a full
        materialisation (D2H of all columns and the pool): fine for the SQL
        table and for tests, not something to call per request."""
        return self.store.rows if self.gpu else self._rows

    @rows.setter
    def rows(self, value: List[Dict]) -> None:
        if self.gpu:
            raise AttributeError("rows of the GPU store are read-only")
        self._rows = value

    @property
    def n_rows(self) -> int:
        return self.store.n_rows if self.gpu else len(self._rows)

    # ---------------------------------------------------------- retention
    @property
    def evicted_rows(self) -> int:
        return self.store.evicted_rows if self.gpu else self._evicted_rows

    @property
    def evictions(self) -> int:
        return self.store.evictions if self.gpu else self._evictions

    def _host_evict(self, n: int) -> int:
        n = min(int(n), len(self._rows))
        if n <= 0:
            return 0
        del self._rows[:n]
        self._evicted_rows += n
        self._evictions += 1
        return n

    def _counted(self, fn, *args):
        """Run a store call that may evict; what it evicted goes to the
        counter as logs_evicted."""
        before = self.evicted_rows
        try:
            return fn(*args)
        finally:
            gone = self.evicted_rows - before
            if gone:
                self.counter.add("logs_evicted", gone)

    def evict_rows(self, n: int) -> int:
        """Drop the min(n, n_rows) oldest-inserted rows; -> how many went
        (n <= 0: none). Apps keep their ids."""
        return self._counted(
            self.store.evict_rows if self.gpu else self._host_evict, n)

    def evict_before(self, t: int) -> int:
        """Drop the longest insertion-order prefix in which every row has
        time < t: rows are in arrival order, not time order, and the cut
        is the first row with time >= t even when older rows follow it."""
        if self.gpu:
            return self._counted(self.store.evict_before, t)
        first = next((i for i, r in enumerate(self._rows)
                      if r["time"] >= t), len(self._rows))
        return self._counted(self._host_evict, first)

    def _host_row_rule(self) -> None:
        self._host_evict(rows_to_evict(len(self._rows), self.max_rows,
                                       self.keep_fraction))

    def stats(self) -> Dict:
        """Rows, retention counters, stored bytes (GPU store: row columns
        plus pool; host store: UTF-8 bytes of the bodies, counted per call)
        and the limits."""
        out = {
            "rows": self.n_rows,
            "evicted_rows": self.evicted_rows,
            "evictions": self.evictions,
            "stored_bytes": self.store.stored_bytes() if self.gpu
            else sum(_body_bytes(r) for r in self._rows),
            "max_rows": self.max_rows,
            "max_pool_bytes": self.store.max_pool_bytes if self.gpu
            else None,
            "keep_fraction": self.keep_fraction,
        }
        if self.gpu:
            out["pool_bytes"] = self.store.pool_len
        return out

    def _intern(self, s: str) -> int:
        i = self.app_interner.get(s)
        if i is None:
            i = len(self.app_interner)
            self.app_interner[s] = i
        return i

    def ingest_lines(self, payload: bytes, agent_id: int = 0,
                     log_type: str = "system",
                     now: Optional[int] = None) -> int:
        """Line format: '<ts> <severity> <app> <body...>' with graceful
        fallback for free-form lines, which get the time `now` (None: the
        wall clock)."""
        if self.gpu:
            n = self._counted(
                lambda: self.store.ingest_lines(
                    payload, agent_id=agent_id, log_type=log_type,
                    now=int(time.time()) if now is None else now))
            self.counter.add("logs_in", n)
            return n
        n = 0
        for line in payload.splitlines():
            line = line.decode("utf-8", "replace").strip()
            if not line:
                continue
            parts = line.split(" ", 3)
            ts = int(time.time()) if now is None else now
            sev = 6
            app = ""
            body = line
            if len(parts) >= 4 and parts[0].isdigit():
                ts = int(parts[0])
                sev = SEVERITIES.get(parts[1].lower(), 6)
                app = parts[2]
                body = parts[3]
            self._rows.append({
                "time": ts,
                "agent_id": agent_id,
                "log_type": log_type,
                "severity": sev,
                "app_service": app,
                "app_id": self._intern(app),
                "body": body,
            })
            n += 1
        self.counter.add("logs_in", n)
        self._counted(self._host_row_rule)
        return n

    def ingest_rows(self, rows: List[Dict]) -> int:
        """Append pre-converted rows (OTLP logs path)."""
        if self.gpu:
            n = self._counted(self.store.ingest_rows, rows)
            self.counter.add("logs_in", n)
            return n
        for r in rows:
            app = r.get("app_service", "")
            r.setdefault("app_id", self._intern(app))
            self._rows.append(r)
        self.counter.add("logs_in", len(rows))
        self._counted(self._host_row_rule)
        return len(rows)

    # -------------------------------------------------------------- query
    def _matcher(self, substr, severity_max, time_start, time_end,
                 app_service, case_insensitive, rx=None):
        needles = norm_needles(substr)
        if case_insensitive:
            needles = [fold_ascii(s) for s in needles]

        def match(r: Dict) -> bool:
            if r["severity"] > severity_max:
                return False
            if time_start is not None and r["time"] < time_start:
                return False
            if time_end is not None and r["time"] > time_end:
                return False
            if app_service is not None and \
                    r.get("app_service", "") != app_service:
                return False
            if needles:
                body = fold_ascii(r["body"]) if case_insensitive \
                    else r["body"]
                for s in needles:
                    if s not in body:
                        return False
            if rx is not None and not rx.host.search(
                    r["body"].encode("utf-8", "replace")):
                return False
            return True
        return match

    def search(self, substr: Union[str, Sequence[str]] = "",
               severity_max: int = 7, limit: int = 100, *,
               time_start: Optional[int] = None,
               time_end: Optional[int] = None,
               app_service: Optional[str] = None,
               case_insensitive: bool = False,
               regex: Optional[str] = None) -> List[Dict]:
        """Newest-inserted first, cut at `limit`. substr: one needle or up
        to 8, all of which must occur in the body; time_start/time_end are
        inclusive bounds on `time`; app_service is an exact match;
        case_insensitive folds ASCII A-Z only, on both sides.

        regex: at most one pattern, ANDed with the needles and every other
        filter; None and "" constrain nothing. A row matches when
        re.search(regex.encode("utf-8"), body.encode("utf-8", "replace"))
        does: Python `re` on bytes, so \\d \\w \\s are ASCII, `.` is any
        byte but \\n, and case_insensitive (re.IGNORECASE) folds A-Z only.
        The supported subset (query/logregex.py): literals, escapes, `.`,
        classes, groups, `|`, * + ? {m,n} (lazy or not), ^ or \\A first and
        $ or \\Z last in the top-level sequence. Backreferences,
        look-around, \\b, inline flags, anchors elsewhere, patterns over
        256 bytes and patterns whose DFA exceeds 32 KiB raise ValueError
        on either store, also on an empty one. Cost on the GPU store: a
        pattern such as `e.*zzz` walks from every `e` to the end of its
        row, O(hits x body length); there is no literal prefilter."""
        rx = check_regex(regex, case_insensitive)
        if self.gpu:
            return self.store.search(
                substr, severity_max, limit, time_start=time_start,
                time_end=time_end, app_service=app_service,
                case_insensitive=case_insensitive, regex=regex)
        match = self._matcher(substr, severity_max, time_start, time_end,
                              app_service, case_insensitive, rx)
        out: List[Dict] = []
        if limit <= 0:
            return out
        for r in reversed(self._rows):
            if match(r):
                out.append(r)
                if len(out) >= limit:
                    break
        return out

    def histogram(self, interval: int, time_start: int, time_end: int,
                  substr: Union[str, Sequence[str]] = "",
                  severity_max: int = 7, *,
                  app_service: Optional[str] = None,
                  case_insensitive: bool = False,
                  regex: Optional[str] = None) -> List[Dict]:
        """Log volume per (time bucket, severity) over [time_start,
        time_end] for the rows search() would match: [{"time":
        bucket_start, "severity": s, "count": c}, ...] sorted by (time,
        severity), nonzero counts only. Severity is clamped to 0..7."""
        rx = check_regex(regex, case_insensitive)
        n_buckets = hist_buckets(interval, time_start, time_end)
        if self.gpu:
            return self.store.histogram(
                interval, time_start, time_end, substr, severity_max,
                app_service=app_service, case_insensitive=case_insensitive,
                regex=regex)
        match = self._matcher(substr, severity_max, time_start, time_end,
                              app_service, case_insensitive, rx)
        counts: Dict[tuple, int] = {}
        if n_buckets:
            for r in self._rows:
                if match(r):
                    b = time_start + \
                        (r["time"] - time_start) // interval * interval
                    key = (b, min(max(r["severity"], 0), 7))
                    counts[key] = counts.get(key, 0) + 1
        return [{"time": t, "severity": s, "count": c}
                for (t, s), c in sorted(counts.items())]

    def patterns(self, substr: Union[str, Sequence[str]] = "",
                 severity_max: int = 7, limit: int = 20, *,
                 time_start: Optional[int] = None,
                 time_end: Optional[int] = None,
                 app_service: Optional[str] = None,
                 case_insensitive: bool = False,
                 regex: Optional[str] = None,
                 max_patterns: int = 1 << 16) -> Dict:
        """The rows search() would match, grouped by the template of their
        body (query/logpattern.py: tokens that hold a digit become `<*>`,
        over the first 512 bytes of the body as UTF-8). The filters mean
        what they mean for search(); case_insensitive touches them only,
        never the template. ->

            {"matched": rows that passed the filters,
             "distinct": patterns found,
             "dropped_rows": matched rows whose pattern found the table full,
             "patterns": [{"pattern": text, "count": n, "sample": row}, ...]}

        `patterns` is sorted by count, largest first, ties by the oldest
        first occurrence, and cut at `limit`. `sample` is the
        newest-inserted matching row of the pattern, as search() returns
        it. max_patterns, a power of two, is the size of the GPU store's
        query-scoped table: a pattern that finds it full loses all of its
        rows to dropped_rows, every reported count stays exact. The host
        store validates it and never drops."""
        from ..query.logpattern import (check_max_patterns, render,
                                        template_symbols)
        rx = check_regex(regex, case_insensitive)
        check_max_patterns(max_patterns)
        if self.gpu:
            return self.store.patterns(
                substr, severity_max, limit, time_start=time_start,
                time_end=time_end, app_service=app_service,
                case_insensitive=case_insensitive, regex=regex,
                max_patterns=max_patterns)
        match = self._matcher(substr, severity_max, time_start, time_end,
                              app_service, case_insensitive, rx)
        # symbols -> [count, first row index, newest row]; by the symbol
        # tuple, not the rendered text: a body may hold a literal "<*>"
        groups: Dict[tuple, list] = {}
        matched = 0
        for i, r in enumerate(self._rows):
            if not match(r):
                continue
            matched += 1
            sym = template_symbols(r["body"].encode("utf-8", "replace"))
            g = groups.get(sym)
            if g is None:
                groups[sym] = [1, i, r]
            else:
                g[0] += 1
                g[2] = r
        top = sorted(groups.items(), key=lambda kv: (-kv[1][0], kv[1][1]))
        return {"matched": matched, "distinct": len(groups),
                "dropped_rows": 0,
                "patterns": [{"pattern": render(sym), "count": g[0],
                              "sample": g[2]}
                             for sym, g in top[:max(int(limit), 0)]]}


class LogApp:
    """HTTP surface: log search and the log-volume histogram. Works on
    either store."""

    def __init__(self, pipeline: AppLogPipeline):
        self.pipe = pipeline

    def register(self, app) -> None:
        from fastapi import HTTPException, Query

        def guarded(fn, *args, **kw):
            try:
                return fn(*args, **kw)
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))

        @app.get("/v1/logs/search")
        def logs_search(q: List[str] = Query(default=[]),
                        severity_max: int = 7,
                        time_start: Optional[int] = None,
                        time_end: Optional[int] = None,
                        app_service: Optional[str] = None,
                        case_insensitive: bool = False,
                        limit: int = 100,
                        re: Optional[str] = None):
            return guarded(self.pipe.search, q, severity_max, limit,
                           time_start=time_start, time_end=time_end,
                           app_service=app_service,
                           case_insensitive=case_insensitive, regex=re)

        @app.get("/v1/logs/patterns")
        def logs_patterns(q: List[str] = Query(default=[]),
                          severity_max: int = 7,
                          time_start: Optional[int] = None,
                          time_end: Optional[int] = None,
                          app_service: Optional[str] = None,
                          case_insensitive: bool = False,
                          limit: int = 20,
                          re: Optional[str] = None,
                          max_patterns: int = 1 << 16):
            return guarded(self.pipe.patterns, q, severity_max, limit,
                           time_start=time_start, time_end=time_end,
                           app_service=app_service,
                           case_insensitive=case_insensitive, regex=re,
                           max_patterns=max_patterns)

        @app.get("/v1/logs/stats")
        def logs_stats():
            return self.pipe.stats()

        @app.get("/v1/logs/histogram")
        def logs_histogram(interval: int, time_start: int, time_end: int,
                           q: List[str] = Query(default=[]),
                           severity_max: int = 7,
                           app_service: Optional[str] = None,
                           case_insensitive: bool = False,
                           re: Optional[str] = None):
            return guarded(self.pipe.histogram, interval, time_start,
                           time_end, q, severity_max,
                           app_service=app_service,
                           case_insensitive=case_insensitive, regex=re)
