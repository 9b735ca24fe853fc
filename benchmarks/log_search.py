"""Host vs GPU application-log store: ingest rate and search time (K11).

Generates a deterministic corpus with the splitmix64 generator, feeds the
same payloads to AppLogPipeline() and AppLogPipeline(device="cuda") and runs
the same queries on both. Writes one JSON document (default
profiles/log_search.json).

Timing method: host wall clock (perf_counter) around work that ends in a
device synchronise; every timed shape is run once untimed first (warm-up);
each figure is the median of --repeats runs (the spread is reported too).
"end to end" is AppLogPipeline.search()/histogram() as a caller sees it
(scan, select, compaction, gather, D2H, hydration of `limit` rows);
"kernels" is k_log_scan + k_log_select alone, between two device
synchronises, on a preallocated workspace. The baseline is the host
store's search() on the same rows, which is the parent commit's code path
(the histogram baseline is the host twin added with this store).

    python benchmarks/log_search.py [--lines 2000000 ...]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from deepflow_amd.gen.rng import SplitMix64
from deepflow_amd.ingest.applog_pipeline import AppLogPipeline, fold_ascii
from deepflow_amd.ops import gpu_ops

PEAK_HBM_GBPS = 8000.0          # MI355X HBM3E, vendor figure
T0 = 1_700_000_000
WORDS = ("request served handler timeout retry connect upstream cache miss "
         "hit user session token expired refresh queue depth worker spawn "
         "exit flush commit rollback begin select insert update delete index "
         "shard replica leader follower vote term heartbeat lease renew "
         "socket closed reset peer dial listen accept bytes latency ms").split()
SEVS = ("debug", "info", "info", "info", "WARN", "warning", "error", "Fatal")
RARE = "rare-needle-7f3a"


def gen_corpus(a):
    """-> list of payloads of --lines-per-payload lines each, 60-200 bytes
    per line, --apps apps; RARE is planted in --rare lines."""
    rng = SplitMix64(a.seed)
    rare_at = {rng.below(a.lines) for _ in range(a.rare)}
    payloads, cur, n_bytes = [], [], 0
    for i in range(a.lines):
        head = "%d %s app-%02d " % (T0 + i // 64, SEVS[rng.below(len(SEVS))],
                                    rng.below(a.apps))
        want = 60 + rng.below(141)
        parts, ln = [], len(head)
        if i in rare_at:
            parts.append(RARE)
            ln += len(RARE) + 1
        while ln < want:
            r = rng.next()
            w = WORDS[r % len(WORDS)]
            if (r >> 32) % 5 == 0:
                w = "%s=%d" % (w, (r >> 40) % 100000)
            elif (r >> 32) % 17 == 0:
                w = w.capitalize()
            parts.append(w)
            ln += len(w) + 1
        cur.append(head + " ".join(parts))
        if len(cur) == a.lines_per_payload or i == a.lines - 1:
            p = ("\n".join(cur) + "\n").encode()
            n_bytes += len(p)
            payloads.append(p)
            cur = []
    return payloads, n_bytes


def sync():
    torch.cuda.synchronize()


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "runs": len(xs)}


def time_ingest(device, payloads, n_lines, repeats):
    rates, pipe = [], None
    for rep in range(repeats + 1):          # rep 0 is the warm-up
        pipe = None
        pipe = AppLogPipeline(device=device)
        sync()
        t0 = time.perf_counter()
        for p in payloads:
            pipe.ingest_lines(p, agent_id=1, now=T0)
        sync()
        if rep:
            rates.append(n_lines / (time.perf_counter() - t0))
    return pipe, med(rates)


def time_call(fn, repeats):
    out = fn()                              # warm-up
    sync()
    ms = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, med(ms)


def time_kernels(store, needles, fold, repeats, hist_args=None):
    """k_log_scan and k_log_select alone on a preallocated workspace."""
    dev = store.device
    n = store.n_rows
    mask = torch.zeros(n, dtype=torch.int32, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    hist = interval = None
    n_buckets = 0
    if hist_args:
        interval, n_buckets = hist_args
        hist = torch.zeros(n_buckets * 8, dtype=torch.int64, device=dev)
    need = (1 << len(needles)) - 1
    lim = (1 << 63) - 1
    scan_ms, select_ms = [], []
    for rep in range(repeats + 1):
        mask.zero_()
        sync()
        t0 = time.perf_counter()
        gpu_ops.log_scan(store, needles, fold, mask)
        sync()
        t1 = time.perf_counter()
        gpu_ops.log_select(store, mask, need, 7, T0 if hist_args else -lim,
                           lim, None, flags, hist, interval or 1, n_buckets)
        sync()
        t2 = time.perf_counter()
        if rep:
            scan_ms.append((t1 - t0) * 1e3)
            select_ms.append((t2 - t1) * 1e3)
    out = {"scan_ms": med(scan_ms), "select_ms": med(select_ms),
           "rows_flagged": int(flags.sum().item())}
    if needles:
        gbps = store.pool_len / (out["scan_ms"]["median"] * 1e-3) / 1e9
        out["scan_gb_per_s"] = gbps
        out["scan_share_of_peak_hbm"] = gbps / PEAK_HBM_GBPS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--lines-per-payload", type=int, default=50_000)
    ap.add_argument("--apps", type=int, default=40)
    ap.add_argument("--rare", type=int, default=25)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--limit", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--host-ingest-repeats", type=int, default=1)
    ap.add_argument("--out", default="profiles/log_search.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "log_search.py measures on a GPU"

    payloads, n_bytes = gen_corpus(a)
    host, h_ingest = time_ingest("cpu", payloads, a.lines,
                                 a.host_ingest_repeats)
    gpu, g_ingest = time_ingest("cuda", payloads, a.lines, a.repeats)
    assert gpu.n_rows == host.n_rows == a.lines
    assert gpu.store.app_drops == 0

    n_sec = a.lines // 64 + 1
    interval = max(1, -(-n_sec // 512))
    queries = {
        "rare": {"substr": RARE},
        "dense": {"substr": "e"},
        "and3": {"substr": ["timeout", "retry", "cache"]},
        "case_insensitive": {"substr": "HEARTBEAT",
                             "case_insensitive": True},
    }
    search = {}
    for name, kw in queries.items():
        hw, h_ms = time_call(lambda: host.search(limit=a.limit, **kw),
                             a.host_repeats)
        gw, g_ms = time_call(lambda: gpu.search(limit=a.limit, **kw),
                             a.repeats)
        sub = kw["substr"]
        needles = [sub] if isinstance(sub, str) else list(sub)
        fold = kw.get("case_insensitive", False)
        if fold:
            needles = [fold_ascii(s) for s in needles]
        k = time_kernels(gpu.store, [s.encode() for s in needles], fold,
                         a.repeats)
        search[name] = {
            "query": kw, "limit": a.limit, "hits_returned": len(gw),
            "results_equal": hw == gw, "host_ms": h_ms,
            "gpu_end_to_end_ms": g_ms, "gpu_kernels": k,
            "speedup_end_to_end": h_ms["median"] / g_ms["median"],
            "speedup_kernels": h_ms["median"]
            / (k["scan_ms"]["median"] + k["select_ms"]["median"])}
    hargs = (interval, T0, T0 + n_sec - 1)
    hw, h_ms = time_call(lambda: host.histogram(*hargs), a.host_repeats)
    gw, g_ms = time_call(lambda: gpu.histogram(*hargs), a.repeats)
    n_buckets = (n_sec - 1) // interval + 1
    k = time_kernels(gpu.store, [], False, a.repeats,
                     hist_args=(interval, n_buckets))
    search["histogram"] = {
        "interval": interval, "buckets": n_buckets, "cells": len(gw),
        "results_equal": hw == gw, "host_ms": h_ms,
        "gpu_end_to_end_ms": g_ms, "gpu_kernels": k,
        "speedup_end_to_end": h_ms["median"] / g_ms["median"]}

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per shape; median of N runs; end to end "
                  "= AppLogPipeline.search()/histogram(); kernels = "
                  "k_log_scan + k_log_select alone; baseline = host "
                  "store on the same rows",
        "shapes": {"lines": a.lines, "payloads": len(payloads),
                   "payload_bytes": n_bytes,
                   "mean_line_bytes": n_bytes / a.lines, "apps": a.apps,
                   "rare_lines": a.rare, "seed": a.seed,
                   "pool_bytes": gpu.store.pool_len},
        "peak_hbm_gb_per_s_assumed": PEAK_HBM_GBPS,
        "ingest_lines_per_s": {"host": h_ingest, "gpu": g_ingest,
                               "gpu_over_host": g_ingest["median"]
                               / h_ingest["median"]},
        "search": search,
        "gpu_store_bytes": gpu.store.stored_bytes(),
    }
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
