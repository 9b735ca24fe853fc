"""Distinct counts in DF-SQL (K15): k_query_uniq against k_query_agg, the
LDS filter on and off, and Uniq() against the GROUP BY route it replaces.

Same timing method as benchmarks/log_patterns.py: perf_counter around work
that ends in a device synchronise, one untimed warm-up per shape, the
median of --repeats runs with min and max. Within one repeat the kernels
under comparison run one after the other on the same rows, so they share
whatever else the machine is doing. Writes one JSON document (default
profiles/query_uniq.json).

  kernels      one segment of --rows generated spans, grouped by
               l7_protocol, no filter. k_query_agg with one Count, then
               k_query_uniq with and without its block-local LDS filter,
               every table preallocated and reset outside the timed region.
               Shapes: (a) Uniq(ip4_0), --ips distinct values; (b)
               Uniq(trace_id), every row its own value, with the pair table
               the executor would try first and with one twice as large;
               (c) both items in one launch. `uniq_over_agg_kernel` is the
               figure of merit.
  end_to_end   QueryEngine: SELECT l7_protocol, Uniq(ip4_0) ... against
               SELECT l7_protocol, ip4_0, Count(*) ... GROUP BY both plus
               the per-key count on the host, in the same run; the results
               must be equal. Uniq(trace_id) runs alone: the old route
               would pull one group per trace to the host (--old-trace-route
               tries it once).

    python benchmarks/query_uniq.py [--rows 4000000 ...]
"""
import argparse
import ctypes as ct
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from deepflow_amd.gen import SpanGenConfig  # noqa: E402
from deepflow_amd.ingest import L7IngestPipeline  # noqa: E402
from deepflow_amd.ops import gpu_ops, native  # noqa: E402
from deepflow_amd.query import QueryEngine  # noqa: E402
from deepflow_amd.query import executor as EX  # noqa: E402
from deepflow_amd.query import spec as Q  # noqa: E402
from deepflow_amd.query.sql import parse_sql  # noqa: E402
from deepflow_amd.query.tags import L7_METRICS, L7_TAGS  # noqa: E402
from deepflow_amd.store.kg import KnowledgeGraphTable, default_platform  # noqa: E402


def sync():
    torch.cuda.synchronize()


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "runs": len(xs)}


def load(rows, ips, seed):
    cfg = SpanGenConfig(n=rows, seed=seed, tag_cardinality=100_000,
                        n_ips=ips, n_services=256, n_resources=4096)
    kg = KnowledgeGraphTable(capacity_pow2=1 << 14, device="cuda")
    kg.update(default_platform(cfg))
    seg_rows = 1 << max(rows - 1, 1).bit_length()
    pipe = L7IngestPipeline(device="cuda", segment_rows=seg_rows, kg=kg,
                            dict_capacity=1 << 23,
                            time_base_s=cfg.base_time_ns // 10**9)
    lib = native.cpu()
    c = native.span_cfg_c(cfg)
    done, batch = 0, 1_000_000
    while done < rows:
        n = min(batch, rows - done)
        need = int(lib.df_gen_spans_parallel(ct.byref(c), done, n, None, 0,
                                             None, None))
        buf = np.zeros(need, dtype=np.uint8)
        offs = np.zeros(n, dtype=np.uint32)
        lens = np.zeros(n, dtype=np.uint32)
        lib.df_gen_spans_parallel(ct.byref(c), done, n,
                                  buf.ctypes.data_as(ct.c_void_p), need,
                                  offs.ctypes.data_as(ct.c_void_p),
                                  lens.ctypes.data_as(ct.c_void_p))
        pipe.ingest(buf, offs, lens)
        done += n
    sync()
    return pipe


def first_try_pcap(rows, n_uniq):
    want = 2 * max(rows, 1) * n_uniq
    return min(1 << (want - 1).bit_length(), EX.UNIQ_PAIR_CAP_FIRST_MAX)


def time_kernels(eng, seg, uniq_sql, pcap, repeats):
    """k_query_agg (one Count) and k_query_uniq (filter on, filter off) on
    the same rows, key and filter, alternating inside each repeat."""
    def plan_of(sql):
        return parse_sql(sql, dictionary=eng.pipe.dict,
                         time_base_s=eng.pipe.time_base_s, tags=L7_TAGS,
                         metrics=L7_METRICS)
    aplan = plan_of("SELECT l7_protocol, Count(*) AS c FROM l7_flow_log "
                    "GROUP BY l7_protocol")
    uplan = plan_of(uniq_sql)
    aspec, uspec, ubytes = aplan.to_bytes(), uplan.to_bytes(), \
        uplan.uniq_to_bytes()
    dev, cap, n, kg = seg.u64.device, EX.GROUP_CAP, seg.n_rows, eng.pipe.kg
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
    gkeys, graw, gvals = z(cap), z(cap, Q.QMAX_KEYS), z(cap, Q.QMAX_AGGS)
    guniq, pkeys = z(cap, Q.QMAX_UNIQ), z(pcap)
    ovf = torch.zeros(2, dtype=torch.int32, device=dev)

    def reset():
        for t in (gkeys, graw, gvals, guniq, pkeys, ovf):
            t.zero_()
        sync()

    def run_agg():
        gpu_ops.query_agg(seg, aspec, 0, n, gkeys, graw, gvals, kg=kg,
                          overflow=ovf)

    def run_uniq(use_filter):
        gpu_ops.query_uniq(seg, uspec, ubytes, 0, n, gkeys, graw, guniq,
                           pkeys, kg=kg, overflow=ovf, use_filter=use_filter)

    runs = {"agg": run_agg, "uniq_filter": lambda: run_uniq(True),
            "uniq_nofilter": lambda: run_uniq(False)}
    ms = {k: [] for k in runs}
    counts = {}
    for rep in range(repeats + 1):              # rep 0 is the warm-up
        for name, fn in runs.items():
            reset()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            if name != "agg":
                assert ovf.tolist() == [0, 0], (name, ovf.tolist())
                counts[name] = guniq.sum(0).tolist()[:len(uplan.uniqs)]
    assert counts["uniq_filter"] == counts["uniq_nofilter"]
    pairs = int((pkeys != 0).sum().item())
    out = {k + "_ms": med(v) for k, v in ms.items()}
    out.update({
        "sql": uniq_sql, "rows": n, "pair_slots": pcap, "pairs": pairs,
        "pair_table_load": pairs / pcap,
        "distinct_per_item_all_groups": counts["uniq_filter"],
        "uniq_filter_rows_per_s":
        n / (out["uniq_filter_ms"]["median"] * 1e-3),
        "uniq_nofilter_rows_per_s":
        n / (out["uniq_nofilter_ms"]["median"] * 1e-3),
        "agg_rows_per_s": n / (out["agg_ms"]["median"] * 1e-3),
        "uniq_over_agg_kernel":
        out["uniq_filter_ms"]["median"] / out["agg_ms"]["median"],
        "nofilter_over_agg_kernel":
        out["uniq_nofilter_ms"]["median"] / out["agg_ms"]["median"],
        "filter_over_nofilter":
        out["uniq_filter_ms"]["median"] / out["uniq_nofilter_ms"]["median"]})
    return out


def time_call(fn, repeats):
    out = fn()                                  # warm-up
    sync()
    ms = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, med(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--ips", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--old-trace-route", action="store_true")
    ap.add_argument("--out", default="profiles/query_uniq.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "query_uniq.py measures on a GPU"

    pipe = load(a.rows, a.ips, a.seed)
    eng = QueryEngine(pipe, device="cuda")
    segs = [s for s in pipe.segments.scan_list() if s.n_rows]
    assert len(segs) == 1 and segs[0].n_rows == a.rows
    seg = segs[0]

    one, two = first_try_pcap(a.rows, 1), first_try_pcap(a.rows, 2)
    q = "SELECT l7_protocol, {} FROM l7_flow_log GROUP BY l7_protocol"
    shapes = {
        "a_ip4_0": (q.format("Uniq(ip4_0) AS u"), one),
        "b_trace_id": (q.format("Uniq(trace_id) AS u"), one),
        "b_trace_id_table_x2": (q.format("Uniq(trace_id) AS u"), 2 * one),
        "c_two_items": (q.format("Uniq(ip4_0) AS u, Uniq(trace_id) AS t"),
                        two),
    }
    kernels = {name: time_kernels(eng, seg, sql, pcap, a.repeats)
               for name, (sql, pcap) in shapes.items()}

    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per shape; median of N runs with min "
                  "and max; per repeat k_query_agg (one Count), "
                  "k_query_uniq with and without the LDS filter run one "
                  "after the other on the same segment, key and filter, "
                  "tables preallocated and reset outside the timed region; "
                  "end to end = QueryEngine.query",
        "shapes": {"rows": a.rows, "ips": a.ips, "seed": a.seed,
                   "segments": 1, "group_key": "l7_protocol",
                   "group_slots": EX.GROUP_CAP},
        "kernels": kernels,
        "uniq_over_agg_kernel": {k: v["uniq_over_agg_kernel"]
                                 for k, v in kernels.items()},
    }
    path.write_text(json.dumps(out, indent=1) + "\n")

    # ---- end to end: Uniq() against GROUP BY (key, value) + host count
    new_sql = q.format("Uniq(ip4_0) AS u")
    old_sql = ("SELECT l7_protocol, ip4_0, Count(*) AS c FROM l7_flow_log "
               "GROUP BY l7_protocol, ip4_0")

    def old_route():
        per = {}
        for proto, _ip, _c in eng.query(old_sql)["values"]:
            per[proto] = per.get(proto, 0) + 1
        return per

    new_r, new_ms = time_call(lambda: eng.query(new_sql), a.repeats)
    old_r, old_ms = time_call(old_route, a.repeats)
    new_d = {row[0]: row[1] for row in new_r["values"]}
    tr_sql = q.format("Uniq(trace_id) AS u")
    tr_r, tr_ms = time_call(lambda: eng.query(tr_sql), a.repeats)
    e2e = {
        "ip4_0": {"uniq_sql": new_sql, "group_by_sql": old_sql,
                  "uniq_ms": new_ms, "group_by_plus_host_ms": old_ms,
                  "results_equal": new_d == old_r, "result": new_d,
                  "speedup": old_ms["median"] / new_ms["median"]},
        "trace_id": {"uniq_sql": tr_sql, "uniq_ms": tr_ms,
                     "result": {r[0]: r[1] for r in tr_r["values"]},
                     "group_by_route": "not measured: one group per trace "
                     f"({a.rows} groups, above the first-try group table of "
                     f"{EX.GROUP_CAP} slots) pulled to the host"},
    }
    if a.old_trace_route:
        try:
            t0 = time.perf_counter()
            n = len(eng.query("SELECT l7_protocol, trace_id, Count(*) AS c "
                              "FROM l7_flow_log GROUP BY l7_protocol, "
                              "trace_id")["values"])
            e2e["trace_id"]["group_by_route"] = {
                "groups": n, "one_run_ms": (time.perf_counter() - t0) * 1e3}
        except RuntimeError as e:
            e2e["trace_id"]["group_by_route"] = f"failed: {e}"
    out["end_to_end"] = e2e
    out["all_results_equal"] = e2e["ip4_0"]["results_equal"]
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
