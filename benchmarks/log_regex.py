"""Regex search over the application-log store, host vs GPU (K13).

Same corpus, same timing method as benchmarks/log_search.py (imported from
there): perf_counter around work that ends in a device synchronise, one
untimed warm-up per shape, the median of --repeats runs. Writes one JSON
document (default profiles/log_regex.json).

Per pattern:
  host_ms            AppLogPipeline().search(regex=..., limit) on the host
                     store: Python `re` per row, newest first, stopping at
                     `limit` hits (so a dense pattern ends early);
  gpu_end_to_end_ms  the same call on the GPU store (compile or cache hit,
                     table upload, k_log_regex, k_log_select, compaction,
                     gather, D2H, hydration of `limit` rows);
  count_all          histogram(regex=...) over the whole time range, one
                     bucket: both stores must look at every row;
  regex_kernel       k_log_regex alone on a preallocated mask with the
                     tables already uploaded, and GB/s over the pool.
The literal pattern also runs as a `substr`, and k_log_scan is timed for it
in the same run: `regex_over_scan_kernel` is the figure of merit.

    python benchmarks/log_regex.py [--lines 2000000 ...]
"""
import argparse
import json
import re
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
from deepflow_amd.query.logregex import compile_log_regex  # noqa: E402

PATTERNS = {
    "literal": {"regex": re.escape(RARE)},
    "digits": {"regex": r"timeout=\d+"},
    "alt_dotstar": {"regex": r"(retry|rollback) .*lease"},
    "anchored": {"regex": r"^request"},
    "case_insensitive": {"regex": r"HEARTBEAT (lease|vote)",
                         "case_insensitive": True},
}


def time_regex_kernel(store, rx, repeats):
    """k_log_regex alone: tables uploaded and mask allocated beforehand."""
    mask = torch.zeros(store.n_rows, dtype=torch.int32, device=store.device)
    table = gpu_ops.log_regex_table(store, rx)
    ms = []
    for rep in range(repeats + 1):              # rep 0 is the warm-up
        mask.zero_()
        sync()
        t0 = time.perf_counter()
        gpu_ops.log_regex(store, rx, mask, table)
        sync()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = {"regex_ms": med(ms),
           "rows_marked": int((mask & gpu_ops.LOG_RE_BIT).ne(0).sum().item())}
    gbps = store.pool_len / (out["regex_ms"]["median"] * 1e-3) / 1e9
    out["regex_gb_per_s"] = gbps
    out["regex_share_of_peak_hbm"] = gbps / PEAK_HBM_GBPS
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
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default="profiles/log_regex.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "log_regex.py measures on a GPU"

    payloads, n_bytes = gen_corpus(a)
    host, gpu = AppLogPipeline(), AppLogPipeline(device="cuda")
    for p in payloads:
        host.ingest_lines(p, agent_id=1, now=T0)
        gpu.ingest_lines(p, agent_id=1, now=T0)
    assert gpu.n_rows == host.n_rows == a.lines
    store = gpu.store
    hargs = (a.lines, T0, T0 + a.lines // 64)   # one bucket: count them all

    def measure(kw):
        hw, h_ms = time_call(lambda: host.search(limit=a.limit, **kw),
                             a.host_repeats)
        gw, g_ms = time_call(lambda: gpu.search(limit=a.limit, **kw),
                             a.repeats)
        hc, hc_ms = time_call(lambda: host.histogram(*hargs, **kw),
                              a.host_repeats)
        gc, gc_ms = time_call(lambda: gpu.histogram(*hargs, **kw),
                              a.repeats)
        return {
            "query": kw, "limit": a.limit, "hits_returned": len(gw),
            "rows_matching": sum(d["count"] for d in gc),
            "results_equal": hw == gw and hc == gc,
            "host_ms": h_ms, "gpu_end_to_end_ms": g_ms,
            "speedup_end_to_end": h_ms["median"] / g_ms["median"],
            "count_all": {"host_ms": hc_ms, "gpu_end_to_end_ms": gc_ms,
                          "speedup_end_to_end":
                          hc_ms["median"] / gc_ms["median"]}}

    out_p = {}
    for name, kw in PATTERNS.items():
        rx = compile_log_regex(kw["regex"], kw.get("case_insensitive", False))
        r = measure(kw)
        r["dfa"] = {"states": rx.n_states, "classes": rx.n_classes,
                    "table_bytes": int(rx.next.nbytes)}
        r["regex_kernel"] = time_regex_kernel(store, rx, a.repeats)
        r["gpu_slower_than_host"] = {
            "search": r["speedup_end_to_end"] < 1.0,
            "count_all": r["count_all"]["speedup_end_to_end"] < 1.0}
        out_p[name] = r

    # the same literal as a substr, and k_log_scan for it in the same run
    sub = measure({"substr": RARE})
    sub["scan_kernel"] = time_kernels(store, [RARE.encode()], False,
                                      a.repeats)
    lit = out_p["literal"]
    assert lit["rows_matching"] == sub["rows_matching"]
    ratio = lit["regex_kernel"]["regex_ms"]["median"] \
        / sub["scan_kernel"]["scan_ms"]["median"]

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per shape; median of N runs; end to end "
                  "= AppLogPipeline.search(regex=)/histogram(regex=); "
                  "regex_kernel = k_log_regex alone, tables uploaded "
                  "beforehand; baseline = host store (Python re per row) "
                  "on the same rows",
        "shapes": {"lines": a.lines, "payloads": len(payloads),
                   "payload_bytes": n_bytes,
                   "mean_line_bytes": n_bytes / a.lines, "apps": a.apps,
                   "rare_lines": a.rare, "seed": a.seed,
                   "pool_bytes": store.pool_len},
        "peak_hbm_gb_per_s_assumed": PEAK_HBM_GBPS,
        "patterns": out_p,
        "literal_as_substr": sub,
        "regex_over_scan_kernel": ratio,
        "all_results_equal": all(p["results_equal"] for p in out_p.values())
        and sub["results_equal"],
    }
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
