"""Distributed query execution across GPU shards.

Span/flow streams are hash-sharded by agent across ranks (one rank per
GPU); queries run shard-local and merge on collectives (RCCL over xGMI on
cuda, gloo on cpu) — the reference's "each analyzer independent, merge at
query time" model with the scatter of ClickHouse sub-queries
replaced by an all-gather of partials.

Aggregate queries exchange (hydrated key tuple, RAW agg vector): dict IDs
are shard-local so keys hydrate before the exchange, while avg stays split
as (sum, count) so cross-shard merging is exact. 1s rollup tables merge the
same way via merge_metric_rows (the time-bucket reduce step).
"""
from __future__ import annotations

import json
from typing import Dict, List

import torch
import torch.distributed as dist

from ..query import spec as Q


def _gather_variable_u8(t: torch.Tensor, device: str) -> List[torch.Tensor]:
    n = torch.tensor([t.numel()], dtype=torch.int64, device=device)
    world = dist.get_world_size()
    sizes = [torch.zeros(1, dtype=torch.int64, device=device)
             for _ in range(world)]
    dist.all_gather(sizes, n)
    max_n = max(int(s.item()) for s in sizes)
    pad = torch.zeros(max_n, dtype=torch.uint8, device=device)
    if t.numel():
        pad[: t.numel()] = t
    out = [torch.zeros(max_n, dtype=torch.uint8, device=device)
           for _ in range(world)]
    dist.all_gather(out, pad)
    return [o[: int(s.item())] for o, s in zip(out, sizes)]


def exchange_json(obj, device: str = "cpu") -> List:
    """all_gather a JSON-serializable object from every rank (byte-tensor
    transport: works on gloo and nccl/RCCL)."""
    blob = json.dumps(obj).encode()
    t = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
    parts = _gather_variable_u8(t, device)
    return [json.loads(bytes(p.cpu().numpy()).decode()) for p in parts]


def _merge_qrow(a, b):
    """Merge two per-group quantile rows (histograms sum by bucket,
    apdex counts sum elementwise)."""
    if a is None:
        return b
    if b is None:
        return a
    out = []
    for x, y in zip(a, b):
        if x is None:
            out.append(y)
        elif y is None:
            out.append(x)
        elif "apdex" in x:
            out.append({"apdex": [i + j
                                  for i, j in zip(x["apdex"], y["apdex"])]})
        else:
            h = {int(k): v for k, v in x["hist"].items()}
            for k, v in y["hist"].items():
                h[int(k)] = h.get(int(k), 0) + v
            out.append({"hist": h})
    return out


def merge_agg_partials(parts: List[Dict]) -> Dict:
    """Merge per-rank {key_rows, aggs, agg_ops[, qhist][, uniq]} by agg
    op. Uniq counts pass through for a group that one part holds alone;
    distinct counts do not add and value ids are shard-local, so a group
    that arrives from two parts with Uniq data is an error."""
    agg_ops = next((p["agg_ops"] for p in parts if p["aggs"]), [])
    merged: Dict[tuple, list] = {}
    keys_of: Dict[tuple, list] = {}
    qof: Dict[tuple, list] = {}
    uof: Dict[tuple, list] = {}
    for p in parts:
        qh = p.get("qhist")
        un = p.get("uniq")
        for i, (key, agg) in enumerate(zip(p["key_rows"], p["aggs"])):
            k = tuple(tuple(x) if isinstance(x, list) else x for x in key)
            if qh is not None:
                qof[k] = _merge_qrow(qof.get(k), qh[i])
            if un is not None:
                if k in uof:
                    raise ValueError(
                        f"Uniq does not merge across shards: group "
                        f"{list(key)!r} has rows on more than one shard")
                uof[k] = un[i]
            acc = merged.get(k)
            if acc is None:
                merged[k] = list(agg)
                keys_of[k] = key
                continue
            for ai, op in enumerate(agg_ops):
                if op in (Q.AGGOP_COUNT, Q.AGGOP_SUM):
                    acc[ai] += agg[ai]
                elif op == Q.AGGOP_MIN:
                    acc[ai] = min(acc[ai], agg[ai])
                else:
                    acc[ai] = max(acc[ai], agg[ai])
    out = {"key_rows": [keys_of[k] for k in merged],
           "aggs": list(merged.values())}
    if qof:
        out["qdata"] = [qof.get(k) for k in merged]
    if uof:
        out["uniq"] = [uof.get(k) for k in merged]
    return out


def merge_metric_rows(parts: List[List[Dict]], max_fields=("rrt_max",
                                                           "rtt_max")) -> List[Dict]:
    """Merge per-rank 1s rollup rows: sum additive fields, max the maxima —
    the time-bucket reduce across shards."""
    merged: Dict[tuple, Dict] = {}
    for rows in parts:
        for r in rows:
            key = tuple(sorted((k, v) for k, v in r.items()
                               if isinstance(v, str) or
                               k in ("time", "vtap_id", "l7_protocol",
                                     "response_status", "server_port",
                                     "l3_epc_id", "protocol")))
            acc = merged.get(key)
            if acc is None:
                merged[key] = dict(r)
                continue
            for k, v in r.items():
                if isinstance(v, str) or k in ("time", "vtap_id",
                                               "l7_protocol",
                                               "response_status",
                                               "server_port", "l3_epc_id",
                                               "protocol"):
                    continue
                if k in max_fields:
                    acc[k] = max(acc[k], v)
                else:
                    acc[k] = acc[k] + v
    return sorted(merged.values(),
                  key=lambda r: (r.get("time", 0), r.get("vtap_id", 0)))


class DistQueryEngine:
    """SPMD distributed querier: every rank calls query() with the same SQL
    and gets the merged global result."""

    def __init__(self, engine, device: str = "cpu"):
        self.engine = engine
        self.device = device

    def query(self, sql: str) -> Dict:
        import re
        if sql.strip().lower().startswith("with"):
            # resolve each CTE through the DISTRIBUTED path (globally
            # correct aggregates), then run the outer query on the
            # merged rows — identical on every rank, so no exchange
            from ..query.engine import split_with, _result_rows
            ctes, main = split_with(sql)
            env = {}
            for name, inner in ctes:
                env[name] = self.query(inner)
            m = re.search(r"\bfrom\s+`?(\w+)`?", main, re.IGNORECASE)
            table = m.group(1).lower() if m else ""
            if table in env:
                return self.engine._run_rows(main,
                                             _result_rows(env[table]),
                                             time_base_s=0)
            raise ValueError("distributed WITH: the outer query must "
                             "select FROM one of its CTEs")
        m = re.search(r"\bslimit\s+(\d+)", sql, re.IGNORECASE)
        if m:  # series-limited queries take the topN pushdown path
            return self.query_topn(sql, int(m.group(1)))
        partial = self.engine.query_partial(sql)
        parts = exchange_json(partial, self.device)
        if partial["kind"] == "rows":
            # row-table / select / show results: concatenate + dedup
            first = parts[0]["result"]
            cols = first["columns"]
            seen = []
            seen_set = set()
            for p in parts:
                for row in p["result"]["values"]:
                    kt = tuple(tuple(x) if isinstance(x, list) else x
                               for x in row)
                    if kt not in seen_set:
                        seen_set.add(kt)
                        seen.append(row)
            return {"columns": cols, "values": seen}
        merged = merge_agg_partials([p for p in parts])
        return self.engine.finalize_groups(sql, merged["key_rows"],
                                           merged["aggs"],
                                           qdata=merged.get("qdata"),
                                           uniq=merged.get("uniq"))

    # ---------------------------------------------------- topN pushdown
    # Exchange O(world x K) groups instead of every group: each rank sends
    # its local top candidates (ranked by the first aggregate — the
    # SLIMIT/ORDER-BY-agg metric), the candidate set is unioned, then a
    # second exchange ships each rank's aggregates for candidates it did
    # not already send, making the merged totals exact for every
    # candidate. A key can only miss the candidate set if it is outside
    # the top `margin` on EVERY shard; margin = 4K + 64 makes that
    # practically impossible for real skew (and the full-exchange path
    # remains available below the `pushdown_threshold`).
    pushdown_threshold = 10000

    def query_topn(self, sql: str, k: int) -> Dict:
        partial = self.engine.query_partial(sql)
        if partial["kind"] != "agg":
            return self.query(sql)
        key_rows, aggs = partial["key_rows"], partial["aggs"]
        if len(aggs) <= self.pushdown_threshold:
            parts = exchange_json(partial, self.device)
            merged = merge_agg_partials(parts)
            return self.engine.finalize_groups(sql, merged["key_rows"],
                                               merged["aggs"],
                                               uniq=merged.get("uniq"))
        margin = 4 * k + 64

        def tup(key):
            return tuple(tuple(x) if isinstance(x, list) else x
                         for x in key)

        order = sorted(range(len(aggs)),
                       key=lambda i: -(aggs[i][0] or 0))
        top_idx = order[:margin]
        sent = {tup(key_rows[i]) for i in top_idx}
        phase1 = {"key_rows": [key_rows[i] for i in top_idx],
                  "aggs": [aggs[i] for i in top_idx],
                  "agg_ops": partial["agg_ops"]}
        uniq = partial.get("uniq")
        if uniq is not None:
            phase1["uniq"] = [uniq[i] for i in top_idx]
        parts = exchange_json(phase1, self.device)
        candidates = set()
        for p in parts:
            for key in p["key_rows"]:
                candidates.add(tup(key))
        local = {tup(kr): (kr, a, i)
                 for i, (kr, a) in enumerate(zip(key_rows, aggs))}
        delta_keys = [c for c in candidates if c in local and c not in sent]
        phase2 = {"key_rows": [local[c][0] for c in delta_keys],
                  "aggs": [local[c][1] for c in delta_keys],
                  "agg_ops": partial["agg_ops"]}
        if uniq is not None:
            phase2["uniq"] = [uniq[local[c][2]] for c in delta_keys]
        parts2 = exchange_json(phase2, self.device)
        merged = merge_agg_partials(parts + parts2)
        return self.engine.finalize_groups(sql, merged["key_rows"],
                                           merged["aggs"],
                                           uniq=merged.get("uniq"))
