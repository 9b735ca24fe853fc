"""Log patterns over the application-log store, host vs GPU (K14).

Same corpus, same timing method as benchmarks/log_search.py (imported from
there): perf_counter around work that ends in a device synchronise, one
untimed warm-up per GPU shape, the median of --repeats runs. The host store
needs seconds to tens of seconds per call (a Python loop over every byte
of every matching body) and has nothing to warm up: it is timed
--host-repeats times without a warm-up run. Writes one JSON document (default
profiles/log_patterns.json).

  kernels      k_log_patterns alone over all rows (every flag set, table
               preallocated and reset outside the timed region), and in the
               same run k_log_scan with one needle over the same pool: the
               project's measured bandwidth-bound pass over these bytes.
               `patterns_over_scan_kernel` is the figure of merit; GB/s is
               pool bytes over kernel time for both.
  end_to_end   AppLogPipeline.patterns(limit=20) on either store:
               unfiltered, with the rare literal as a needle, and with
               timeout=\\d+ as the regex. On the GPU store that is scan,
               regex, select, k_log_patterns, the top-k selection, the
               hydration of 20 rows and the rendering.

    python benchmarks/log_patterns.py [--lines 2000000 ...]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from log_search import (PEAK_HBM_GBPS, RARE, T0, gen_corpus, med,  # noqa: E402
                        sync, time_call, time_kernels)

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.ops import gpu_ops  # noqa: E402

QUERIES = {
    "unfiltered": {},
    "rare_needle": {"substr": RARE},
    "regex_digits": {"regex": r"timeout=\d+"},
}


def time_patterns_kernel(store, cap, repeats):
    """k_log_patterns alone: every row selected, the table preallocated."""
    n = store.n_rows
    flags = torch.ones(n, dtype=torch.uint8, device=store.device)
    table = gpu_ops.LogPatternTable(store.device, cap)
    ms = []
    for rep in range(repeats + 1):              # rep 0 is the warm-up
        table.reset()
        sync()
        t0 = time.perf_counter()
        gpu_ops.log_patterns(store, flags, cap, table=table)
        sync()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
    body_bytes = int(store.row_blen[:n].sum().item())
    out = {"patterns_ms": med(ms),
           "rows": n,
           "distinct": int(torch.count_nonzero(table.count).item()),
           "rows_counted": int(table.count.sum().item()),
           "dropped_rows": int(table.drops.item()),
           "body_bytes": body_bytes}
    sec = out["patterns_ms"]["median"] * 1e-3
    out["patterns_gb_per_s"] = store.pool_len / sec / 1e9
    out["patterns_body_gb_per_s"] = body_bytes / sec / 1e9
    out["patterns_share_of_peak_hbm"] = \
        out["patterns_gb_per_s"] / PEAK_HBM_GBPS
    return out


def time_host(fn, repeats):
    ms, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, med(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--lines-per-payload", type=int, default=50_000)
    ap.add_argument("--apps", type=int, default=40)
    ap.add_argument("--rare", type=int, default=25)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--limit", type=int, default=20)
    # the generator strings random words together: nearly every line is a
    # template of its own, so the table is sized for --lines of them
    ap.add_argument("--max-patterns", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default="profiles/log_patterns.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "log_patterns.py measures on a GPU"

    payloads, n_bytes = gen_corpus(a)
    host, gpu = AppLogPipeline(), AppLogPipeline(device="cuda")
    for p in payloads:
        host.ingest_lines(p, agent_id=1, now=T0)
        gpu.ingest_lines(p, agent_id=1, now=T0)
    assert gpu.n_rows == host.n_rows == a.lines
    store = gpu.store

    kern = time_patterns_kernel(store, a.max_patterns, a.repeats)
    kern["scan_kernel"] = time_kernels(store, [RARE.encode()], False,
                                       a.repeats)
    ratio = kern["patterns_ms"]["median"] \
        / kern["scan_kernel"]["scan_ms"]["median"]

    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per GPU shape; median of N runs; host "
                  "store timed without warm-up (pure Python, tens of "
                  "seconds a call); kernels = k_log_patterns alone over "
                  "all rows on a preallocated table, and k_log_scan with "
                  "one needle over the same pool in the same run; end to "
                  "end = AppLogPipeline.patterns(limit)",
        "shapes": {"lines": a.lines, "payloads": len(payloads),
                   "payload_bytes": n_bytes,
                   "mean_line_bytes": n_bytes / a.lines, "apps": a.apps,
                   "rare_lines": a.rare, "seed": a.seed,
                   "pool_bytes": store.pool_len,
                   "max_patterns": a.max_patterns},
        "peak_hbm_gb_per_s_assumed": PEAK_HBM_GBPS,
        "matched": kern["rows_counted"] + kern["dropped_rows"],
        "distinct": kern["distinct"],
        "kernels": kern,
        "patterns_over_scan_kernel": ratio,
        "pool_read": "one lane per row, aligned 16-byte loads from the "
                     "pool; no LDS staging",
    }

    # the GPU store first, and the document written once before the host
    # store's minutes begin
    e2e = {}
    for name, kw in QUERIES.items():
        kw = dict(kw, limit=a.limit, max_patterns=a.max_patterns)
        gw, g_ms = time_call(lambda: gpu.patterns(**kw), a.repeats)
        e2e[name] = {
            "query": kw, "matched": gw["matched"],
            "distinct": gw["distinct"], "dropped_rows": gw["dropped_rows"],
            "top": [{"pattern": p["pattern"], "count": p["count"]}
                    for p in gw["patterns"][:3]],
            "gpu_end_to_end_ms": g_ms, "_gpu_result": gw}
    out["end_to_end"] = {k: {x: y for x, y in v.items() if x[0] != "_"}
                         for k, v in e2e.items()}
    path.write_text(json.dumps(out, indent=1) + "\n")
    for name, q in e2e.items():
        gw = q.pop("_gpu_result")
        hw, h_ms = time_host(lambda: host.patterns(**q["query"]),
                             a.host_repeats)
        q.update({
            "results_equal": gw == hw, "host_ms": h_ms,
            "speedup_end_to_end":
            h_ms["median"] / q["gpu_end_to_end_ms"]["median"],
            "gpu_slower_than_host":
            h_ms["median"] < q["gpu_end_to_end_ms"]["median"]})
        del hw
    out["end_to_end"] = e2e
    out["all_results_equal"] = all(q["results_equal"] for q in e2e.values())
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
