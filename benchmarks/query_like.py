"""LIKE / REGEXP on dictionary tags in DF-SQL (K16): the dictionary walk,
the set-membership term in k_query_agg, and the whole query.

Same timing method as benchmarks/query_uniq.py: perf_counter around work
that ends in a device synchronise, one untimed warm-up per shape, the median
of --repeats runs with min and max, everything in one run. Writes one JSON
document (default profiles/query_like.json).

  dict_match   k_dict_match over the request_resource arena (--resources
               distinct paths with numeric ids) for three patterns, bitmap
               zeroed and tables uploaded outside the timed region; ms and
               GB/s over the arena's bytes. `host_re_ms` is the Python `re`
               loop over the same entries, the route the kernel replaces;
               the two id sets must be equal.
  agg          k_query_agg grouped by l7_protocol with one OP_INSET term on
               request_resource against the same kernel with one OP_EQ term
               on the same column, alternating inside each repeat.
               `inset_over_eq_kernel` is the figure of merit.
  end_to_end   QueryEngine.query of a grouped Count with a LIKE filter: the
               first query builds the arena (host walk of the dictionary and
               the upload), later ones find it warm.

    python benchmarks/query_like.py [--rows 4000000 --resources 1000000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from deepflow_amd.gen import SpanGenConfig  # noqa: E402
from deepflow_amd.ops import gpu_ops  # noqa: E402
from deepflow_amd.query import QueryEngine  # noqa: E402
from deepflow_amd.query import executor as EX  # noqa: E402
from deepflow_amd.query import spec as Q  # noqa: E402
from deepflow_amd.query.logregex import compile_log_regex  # noqa: E402
from deepflow_amd.query.sql import like_to_regex, parse_sql  # noqa: E402
from deepflow_amd.query.tags import L7_METRICS, L7_TAGS  # noqa: E402


def sync():
    torch.cuda.synchronize()


def med(xs):
    import statistics
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "runs": len(xs)}


def load(rows, resources, seed):
    """One segment of `rows` generated spans over `resources` paths."""
    import ctypes as ct
    from deepflow_amd.ingest import L7IngestPipeline
    from deepflow_amd.ops import native
    from deepflow_amd.store.kg import KnowledgeGraphTable, default_platform
    cfg = SpanGenConfig(n=rows, seed=seed, tag_cardinality=1000, n_ips=1024,
                        n_services=256, n_resources=resources)
    kg = KnowledgeGraphTable(capacity_pow2=1 << 14, device="cuda")
    kg.update(default_platform(cfg))
    pipe = L7IngestPipeline(device="cuda",
                            segment_rows=1 << max(rows - 1, 1).bit_length(),
                            kg=kg, dict_capacity=1 << 22,
                            time_base_s=cfg.base_time_ns // 10**9)
    lib, c = native.cpu(), native.span_cfg_c(cfg)
    done, batch = 0, 500_000          # below the dictionary's emit buffer
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


def time_dict_match(pipe, dom, patterns, repeats):
    d = pipe.dict
    arena = d.arena(dom, torch.device("cuda", torch.cuda.current_device()))
    entries = [(i, s) for (dm, i), s in d.id_to_str.items() if dm == dom]
    assert len(entries) == arena.n
    nbits = d.capacity
    words = torch.zeros(nbits // 32, dtype=torch.int32, device="cuda")
    out = {}
    for name, (kind, pat) in patterns.items():
        regex = like_to_regex(pat)[0] if kind == "like" else pat
        rx = compile_log_regex(regex)
        table = gpu_ops.dict_regex_table(rx, words.device)
        gpu_ms, host_ms = [], []
        for rep in range(repeats + 1):          # rep 0 is the warm-up
            words.zero_()
            sync()
            t0 = time.perf_counter()
            gpu_ops.dict_match(arena, rx, words, nbits, table=table)
            sync()
            if rep:
                gpu_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            search = rx.host.search
            host_ids = [i for i, s in entries if search(s)]
            if rep:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        bits = np.unpackbits(words.cpu().numpy().view(np.uint8),
                             bitorder="little")
        g = med(gpu_ms)
        out[name] = {
            "kind": kind, "pattern": pat, "regex": regex,
            "dfa_states": rx.n_states, "dfa_classes": rx.n_classes,
            "table_bytes": int(rx.table().nbytes), "matches": len(host_ids),
            "ids_equal": set(np.nonzero(bits)[0].tolist()) == set(host_ids),
            "k_dict_match_ms": g, "host_re_ms": med(host_ms),
            "arena_GBps": arena.nbytes / (g["median"] * 1e-3) / 1e9,
            "entries_per_s": arena.n / (g["median"] * 1e-3),
            "host_over_kernel": med(host_ms)["median"] / g["median"]}
    return {"entries": arena.n, "arena_bytes": arena.nbytes,
            "mean_entry_bytes": arena.nbytes / max(arena.n, 1),
            "bitmap_bytes": nbits // 8, "patterns": out}


def time_agg(eng, seg, like_sql, eq_sql, repeats):
    def plan_of(sql):
        return parse_sql(sql, dictionary=eng.pipe.dict,
                         time_base_s=eng.pipe.time_base_s, tags=L7_TAGS,
                         metrics=L7_METRICS)
    lplan, eplan = plan_of(like_sql), plan_of(eq_sql)
    assert [t.op for t in lplan.terms] == [Q.OP_INSET]
    assert [t.op for t in eplan.terms] == [Q.OP_EQ]
    dev, cap, n, kg = seg.u64.device, EX.GROUP_CAP, seg.n_rows, eng.pipe.kg
    specs = {"inset": EX._spec_bytes(lplan, dev), "eq": eplan.to_bytes()}
    z = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
    gkeys, graw, gvals = z(cap), z(cap, Q.QMAX_KEYS), z(cap, Q.QMAX_AGGS)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    ms = {k: [] for k in specs}
    hits = {}
    for rep in range(repeats + 1):
        for name, spec in specs.items():
            for t in (gkeys, graw, gvals, ovf):
                t.zero_()
            sync()
            t0 = time.perf_counter()
            gpu_ops.query_agg(seg, spec, 0, n, gkeys, graw, gvals, kg=kg,
                              overflow=ovf)
            sync()
            if rep:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            hits[name] = int(gvals[:, 0].sum().item())
    out = {k + "_ms": med(v) for k, v in ms.items()}
    out.update({"inset_sql": like_sql, "eq_sql": eq_sql, "rows": n,
                "rows_passing": hits,
                "inset_over_eq_kernel":
                out["inset_ms"]["median"] / out["eq_ms"]["median"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--resources", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/query_like.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "query_like.py measures on a GPU"

    pipe = load(a.rows, a.resources, a.seed)
    eng = QueryEngine(pipe, device="cuda")
    eng.query("SELECT Count(*) AS c FROM l7_flow_log")   # lands the harvest
    segs = [s for s in pipe.segments.scan_list() if s.n_rows]
    assert len(segs) == 1 and segs[0].n_rows == a.rows
    dom = int(L7_TAGS["request_resource"].hydrate.split(":")[1])
    some = next(s for (d, _), s in pipe.dict.id_to_str.items() if d == dom)

    patterns = {"a_like_api": ("like", "*/api/*"),
                "b_regexp_user": ("regexp", "^/user/[0-9]+$"),
                "c_rare_infix": ("like", "%/r/4242_%")}
    q = ("SELECT l7_protocol, Count(*) AS c FROM l7_flow_log WHERE {} "
         "GROUP BY l7_protocol")
    like_sql = q.format("request_resource LIKE '%/r/4242_%'")
    eq_sql = q.format(f"request_resource = '{some.decode()}'")

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per shape; median of N runs with min and "
                  "max; kernels under comparison alternate inside each "
                  "repeat; tables and bitmaps prepared outside the timed "
                  "region; end to end = QueryEngine.query",
        "shapes": {"rows": a.rows, "resources": a.resources, "seed": a.seed,
                   "segments": 1, "dict_entries": pipe.dict.n_entries(),
                   "dict_capacity": pipe.dict.capacity},
        "dict_match": time_dict_match(pipe, dom, patterns, a.repeats),
        "agg": time_agg(eng, segs[0], like_sql, eq_sql, a.repeats),
    }

    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")

    # ---- end to end: first query (arena cold) and later ones (warm)
    cold, warm = [], []
    want = None
    for rep in range(a.repeats):
        pipe.dict._arenas.clear()               # forget the device arena
        torch.cuda.empty_cache()
        sync()
        t0 = time.perf_counter()
        r = eng.query(like_sql)
        sync()
        cold.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        r2 = eng.query(like_sql)
        sync()
        warm.append((time.perf_counter() - t0) * 1e3)
        assert r == r2 and (want is None or r == want)
        want = r
    eq_ms = []
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        eng.query(eq_sql)
        sync()
        if rep:
            eq_ms.append((time.perf_counter() - t0) * 1e3)
    out["end_to_end"] = {"sql": like_sql, "result": want["values"],
                         "first_query_arena_cold_ms": med(cold),
                         "second_query_arena_warm_ms": med(warm),
                         "eq_query_ms": med(eq_ms), "eq_sql": eq_sql}
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
