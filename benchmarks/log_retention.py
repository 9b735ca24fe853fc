"""Bounded vs unbounded GPU application-log store: what retention costs.

Uses the corpus generator and the timing method of log_search.py (host
wall clock around device-synchronised regions, one untimed warm-up per
shape, median of --repeats runs with the spread). Ingests the same payloads,
several times the byte budget, through AppLogPipeline(device="cuda",
max_pool_bytes=budget) and through an unbounded AppLogPipeline(device=
"cuda"), alternating the two in every repetition. The unbounded store is
the parent commit's code path and is the baseline.

Reported: ingest rate of both; per-eviction time, bytes moved per eviction
(new pool + new row columns written) and the copy rate that makes, next to
a torch D2D copy of the same size timed in the same run; and one
rare-literal search() and one histogram() on the bounded store after its
last eviction against the same queries on an unbounded store holding the
same rows. Evictions are timed in a pass of their own, because timing one
needs two device synchronises that the ingest-rate pass must not pay.

Writes one JSON document (default profiles/log_retention.json).

    python benchmarks/log_retention.py [--lines 2000000 ...]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from log_search import RARE, T0, gen_corpus, med, sync, time_call  # noqa: E402

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402

ROW_BYTES = 31          # the seven row columns, as stored_bytes() counts


def ingest_all(pipe, payloads):
    sync()
    t0 = time.perf_counter()
    for p in payloads:
        pipe.ingest_lines(p, agent_id=1, now=T0)
    sync()
    return time.perf_counter() - t0


def time_ingest_pair(payloads, n_lines, budget, keep, repeats):
    """Lines per second of an unbounded and a bounded store, alternated."""
    rates = {"unbounded": [], "bounded": []}
    evictions = 0
    for rep in range(repeats + 1):          # rep 0 is the warm-up
        for name in ("unbounded", "bounded"):
            kw = {"max_pool_bytes": budget, "keep_fraction": keep} \
                if name == "bounded" else {}
            pipe = AppLogPipeline(device="cuda", **kw)
            dt = ingest_all(pipe, payloads)
            if rep:
                rates[name].append(n_lines / dt)
            if name == "bounded":
                evictions = pipe.evictions
                assert pipe.store.pool_len <= budget
            pipe = None
    return {k: med(v) for k, v in rates.items()}, evictions


def time_evictions(payloads, budget, keep):
    """One bounded ingest with every eviction timed on its own.
    -> (pipeline, [per-eviction dicts])."""
    pipe = AppLogPipeline(device="cuda", max_pool_bytes=budget,
                          keep_fraction=keep)
    st = pipe.store
    inner = st.evict_rows
    log = []

    def timed(n):
        if min(int(n), st.n_rows) <= 0:
            return inner(n)
        before = st.pool_len
        sync()
        t0 = time.perf_counter()
        gone = inner(n)
        sync()
        ms = (time.perf_counter() - t0) * 1e3
        log.append({"ms": ms, "rows_dropped": gone,
                    "rows_kept": st.n_rows, "pool_before": before,
                    "pool_after": st.pool_len,
                    "bytes_moved": st.pool_len + st.n_rows * ROW_BYTES})
        return gone

    st.evict_rows = timed
    for p in payloads:
        pipe.ingest_lines(p, agent_id=1, now=T0)
    sync()
    st.evict_rows = inner
    return pipe, log


def time_d2d(n_bytes, repeats):
    src = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    _, ms = time_call(lambda: dst.copy_(src), repeats)
    return ms


def no_app_id(rows):
    # dense app ids are first-seen order over every row a store ever held
    return [{k: v for k, v in r.items() if k != "app_id"} for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--lines-per-payload", type=int, default=50_000)
    ap.add_argument("--apps", type=int, default=40)
    ap.add_argument("--rare", type=int, default=200)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--budget-divisor", type=float, default=5.0,
                    help="the byte budget is the corpus size over this")
    ap.add_argument("--keep-fraction", type=float, default=0.5)
    ap.add_argument("--out", default="profiles/log_retention.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "log_retention.py measures on a GPU"

    payloads, n_bytes = gen_corpus(a)
    budget = int(n_bytes / a.budget_divisor)
    assert max(len(p) for p in payloads) <= budget // 2

    ingest, evictions = time_ingest_pair(payloads, a.lines, budget,
                                         a.keep_fraction, a.repeats)
    bounded, ev = time_evictions(payloads, budget, a.keep_fraction)
    assert len(ev) == evictions >= 2
    moved = [e["bytes_moved"] for e in ev]
    ev_ms = [e["ms"] for e in ev]
    typical = int(statistics.median(moved))
    d2d_ms = time_d2d(typical, max(a.repeats, 5))
    ev_gbps = [e["bytes_moved"] / (e["ms"] * 1e-3) / 1e9 for e in ev]

    # an unbounded store that holds exactly the surviving rows
    lines = [ln for p in payloads for ln in p.split(b"\n") if ln]
    tail = lines[len(lines) - bounded.n_rows:]
    same = AppLogPipeline(device="cuda")
    for i in range(0, len(tail), a.lines_per_payload):
        same.ingest_lines(b"\n".join(tail[i:i + a.lines_per_payload])
                          + b"\n", agent_id=1, now=T0)
    assert same.n_rows == bounded.n_rows

    n_sec = a.lines // 64 + 1
    interval = max(1, -(-n_sec // 512))
    hargs = (interval, T0, T0 + n_sec - 1)
    queries = {}
    for name, fn in (
            ("search_rare", lambda p: p.search(RARE, limit=a.limit)),
            ("histogram", lambda p: p.histogram(*hargs))):
        bw, b_ms = time_call(lambda: fn(bounded), a.repeats)
        sw, s_ms = time_call(lambda: fn(same), a.repeats)
        if name == "search_rare":
            bw, sw = no_app_id(bw), no_app_id(sw)
        queries[name] = {
            "results": len(bw), "results_equal": bw == sw,
            "bounded_after_eviction_ms": b_ms, "unbounded_same_rows_ms": s_ms,
            "bounded_over_unbounded": b_ms["median"] / s_ms["median"]}

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per shape; median of N runs; bounded and "
                  "unbounded ingest alternate within every repetition; "
                  "evictions are timed in a separate pass (two extra "
                  "synchronises each); baseline = unbounded GPU store",
        "shapes": {"lines": a.lines, "payloads": len(payloads),
                   "payload_bytes": n_bytes, "apps": a.apps,
                   "seed": a.seed, "max_pool_bytes": budget,
                   "keep_fraction": a.keep_fraction,
                   "ingested_over_budget": n_bytes / budget},
        "ingest_lines_per_s": {
            **ingest, "bounded_over_unbounded":
            ingest["bounded"]["median"] / ingest["unbounded"]["median"]},
        "evictions": {
            "count": len(ev), "ms": med(ev_ms),
            "bytes_moved": med(moved),
            "gb_per_s": med(ev_gbps),
            "rows_dropped": med([e["rows_dropped"] for e in ev]),
            "bytes_moved_per_byte_ingested": sum(moved) / n_bytes,
            "torch_d2d_same_size": {
                "bytes": typical, "ms": d2d_ms,
                "gb_per_s": typical / (d2d_ms["median"] * 1e-3) / 1e9},
            "eviction_over_d2d_copy":
            statistics.median(ev_ms) / d2d_ms["median"],
        },
        "rows_after": bounded.n_rows,
        "pool_bytes_after": bounded.store.pool_len,
        "queries_after_last_eviction": queries,
    }
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
