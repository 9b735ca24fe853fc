"""Hand-built cases, the pair hash and a brute-force reference for the K15
distinct-count aggregates (Uniq / UniqExact), shared by test_uniq_cpu.py
and test_uniq_gpu.py.

`ref_uniq` is a per-row pure-Python loop over the semantics documented at
k_query_uniq in ops/csrc/dfquery.hip; it shares no code with
query/executor.py (it reads rows through query_cases.ref_value /
ref_match). `pair_hash` rebuilds the documented formula, the way
query_cases.group_hash rebuilds the group hash.
"""
from typing import Dict, List, Optional

import numpy as np

import query_cases as QC
from deepflow_amd.ops.ref import mix64
from deepflow_amd.query import spec as Q
from deepflow_amd.query.spec import Agg, Key, Plan, Term, Uniq
from deepflow_amd.store import l7_schema as S

M64 = QC.M64
U64, U32, U8 = QC.U64, QC.U32, QC.U8

# twins of dfquery.hip UNIQ_SEED / UNIQ_ITEM_MUL / UNIQ_FILTER_SLOTS /
# UNIQ_FILTER_SHIFT (test_uniq_gpu.py compares them with df_uniq_consts)
UNIQ_SEED = 0x13198A2E03707344
UNIQ_ITEM_MUL = 0x9E3779B97F4A7C15
FILTER_SLOTS = 4096
FILTER_SHIFT = 32

_INV1 = pow(0xBF58476D1CE4E5B9, -1, 1 << 64)
_INV2 = pow(0x94D049BB133111EB, -1, 1 << 64)


def unmix64(z: int) -> int:
    """Inverse of ops.ref.mix64."""
    z &= M64
    z ^= (z >> 31) ^ (z >> 62)
    z = (z * _INV2) & M64
    z ^= (z >> 27) ^ (z >> 54)
    z = (z * _INV1) & M64
    z ^= (z >> 30) ^ (z >> 60)
    return z & M64


def item_salt(u: int) -> int:
    return UNIQ_SEED ^ (((u + 1) * UNIQ_ITEM_MUL) & M64)


def pair_hash(group_key: tuple, u: int, values: tuple) -> int:
    """vh = UNIQ_SEED ^ ((u + 1) * 0x9E37...); vh = mix64(vh ^ value_j ^
    (j << 56)) per argument; pair = mix64(group_hash ^ vh), 0 -> 1."""
    vh = item_salt(u)
    for j, v in enumerate(values):
        vh = mix64(vh ^ (v & M64) ^ (j << 56))
    return mix64(QC.group_hash(group_key) ^ vh) or 1


def filter_index(pair: int) -> int:
    return (pair >> FILTER_SHIFT) & (FILTER_SLOTS - 1)


def zero_pair_value(group_key: tuple = (), u: int = 0) -> int:
    """The single-argument value whose pair hash is 0 before the 0 -> 1
    mapping: mix64(x) == 0 only for x == 0, so vh must equal the group
    hash."""
    return unmix64(QC.group_hash(group_key)) ^ item_salt(u)


def values_sharing_filter_slot(seed: int = 5, group_key: tuple = ()):
    """Two u64 values (item 0, one argument) whose pair hashes differ but
    map to one filter slot."""
    rng = np.random.default_rng(seed)
    first: Dict[int, int] = {}
    while True:
        v = int(rng.integers(1, 1 << 62))
        p = pair_hash(group_key, 0, (v,))
        other = first.setdefault(filter_index(p), v)
        if other != v and pair_hash(group_key, 0, (other,)) != p:
            return other, v


# ------------------------------------------------------------- reference

def ref_uniq(plan: Plan, segs, kg=None, ranges=None) -> Dict[tuple, List[set]]:
    """{raw key tuple: [set of value tuples per Uniq item]} over rows
    [base, base + n) of each segment (default: all n_rows)."""
    out: Dict[tuple, List[set]] = {}
    for si, seg in enumerate(segs):
        base, n = ranges[si] if ranges else (0, seg.n_rows)
        c = QC._Cols(seg)
        for row in range(base, base + n):
            if not QC.ref_match(c, row, plan, kg):
                continue
            key = tuple(QC.ref_value(c, row, k.family, k.idx, k.bucket,
                                     plan.time_base_s, kg)
                        for k in plan.keys)
            sets = out.get(key)
            if sets is None:
                sets = out[key] = [set() for _ in plan.uniqs]
            for ui, item in enumerate(plan.uniqs):
                sets[ui].add(tuple(
                    QC.ref_value(c, row, fam, idx, 0, plan.time_base_s, kg)
                    for fam, idx in item.cols))
    return out


def ref_counts(plan: Plan, segs, kg=None, ranges=None) -> Dict[tuple, List[int]]:
    return {k: [len(s) for s in v]
            for k, v in ref_uniq(plan, segs, kg, ranges).items()}


def engine_counts(groups) -> Dict[tuple, List[int]]:
    """executor output -> {key: uniq counts}."""
    return {tuple(g["key"]): list(g["uniq"]) for g in groups}


# ----------------------------------------------------------------- plans

def uplan(uniqs, keys=(), terms=(), extra_aggs=()) -> Plan:
    """A plan the way the parser builds it: the extra aggregates, then one
    AGGOP_COUNT placeholder per Uniq item."""
    items = [Uniq(list(cols)) for cols in uniqs]
    p = QC.plan(terms, keys, list(extra_aggs) + [QC.COUNT] * len(items))
    p.uniqs = items
    return p


RRT = (Q.SRC_U64, U64["rrt"])
FLOW = (Q.SRC_U64, U64["flow_id"])
IP0 = (Q.SRC_U32, U32["ip4_0"])
STATUS = (Q.SRC_U8, U8["response_status"])
DID2 = (Q.SRC_DID, 2)
K_PROTO = Key(Q.SRC_U8, U8["l7_protocol"])
K_FLOW = Key(Q.SRC_U64, U64["flow_id"])


def shape_case(n: int) -> QC.Case:
    """n rows, 2 groups, at most 7 distinct values."""
    rng = np.random.default_rng(n)
    seg = QC.new_segment(n)
    vals = np.array([0, 1, 5, 1 << 40, M64, 1 << 63, 77], dtype=np.uint64)
    QC.set_u64(seg, "rrt", vals[rng.integers(0, 7, n)])
    QC.set_u8(seg, "l7_protocol", rng.choice([20, 21], n))
    QC.set_u8(seg, "response_status", rng.integers(0, 4, n))
    return QC.Case(f"shape_{n}", uplan([[RRT]], [K_PROTO]), [seg])


def no_match_plan() -> Plan:
    return uplan([[RRT]], [K_PROTO], [Term(Q.SRC_U8, U8["response_status"],
                                           Q.OP_EQ, 99)])


def one_value_case() -> QC.Case:
    seg = QC.new_segment(1500)
    QC.set_u64(seg, "rrt", np.full(1500, 42, dtype=np.uint64))
    return QC.Case("one_value", uplan([[RRT]]), [seg],
                   extra={"want": {(): [1]}})


def all_distinct_case(n: int = 5000) -> QC.Case:
    """More distinct values than the filter has slots."""
    assert n > FILTER_SLOTS
    rng = np.random.default_rng(50)
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", rng.permutation(
        np.arange(10**6, 10**6 + n, dtype=np.uint64)))
    return QC.Case("all_distinct", uplan([[RRT]]), [seg],
                   extra={"want": {(): [n]}})


def eviction_case() -> QC.Case:
    a, b = values_sharing_filter_slot()
    pa, pb = pair_hash((), 0, (a,)), pair_hash((), 0, (b,))
    assert pa != pb and filter_index(pa) == filter_index(pb)
    n = 2000
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", np.where(np.arange(n) % 2 == 0, a, b)
               .astype(np.uint64))
    return QC.Case("eviction", uplan([[RRT]]), [seg],
                   extra={"want": {(): [2]}})


def group_in_pair_case() -> QC.Case:
    n = 600
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", np.full(n, 9, dtype=np.uint64))
    QC.set_u8(seg, "l7_protocol", np.where(np.arange(n) % 3 == 0, 20, 21))
    return QC.Case("group_in_pair", uplan([[RRT]], [K_PROTO]), [seg],
                   extra={"want": {(20,): [1], (21,): [1]}})


def two_items_case() -> QC.Case:
    """5 in column A and 5 in column B are different pairs."""
    n = 300
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", np.where(np.arange(n) % 2 == 0, 5, 6))
    QC.set_u64(seg, "flow_id", np.array([5, 6, 7], dtype=np.uint64)[
        np.arange(n) % 3])
    return QC.Case("two_items", uplan([[RRT], [FLOW]]), [seg],
                   extra={"want": {(): [2, 3]}})


def tuple_order_case() -> QC.Case:
    seg = QC.new_segment(4)
    QC.set_u64(seg, "rrt", [1, 2, 1, 2])
    QC.set_u64(seg, "flow_id", [2, 1, 2, 1])
    return QC.Case("tuple_order", uplan([[RRT, FLOW]]), [seg],
                   extra={"want": {(): [2]}})


def multi_arg_case() -> QC.Case:
    """Uniq(a, b), Uniq(a), Uniq(b) and a four-argument item on random
    data, 3 groups."""
    n = 2500
    rng = np.random.default_rng(25)
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", rng.integers(0, 40, n))
    QC.set_u32(seg, "ip4_0", 0x0A000000 + rng.integers(0, 30, n))
    QC.set_u8(seg, "response_status", rng.integers(0, 5, n))
    QC.set_did(seg, 2, rng.integers(0, 6, n))
    QC.set_u8(seg, "l7_protocol", rng.choice([20, 21, 40], n))
    p = uplan([[RRT, IP0], [RRT], [IP0], [RRT, IP0, STATUS, DID2]],
              [K_PROTO])
    return QC.Case("multi_arg", p, [seg])


def zero_pair_case() -> QC.Case:
    z = zero_pair_value()
    assert mix64(QC.group_hash(()) ^ mix64(item_salt(0) ^ z)) == 0
    assert pair_hash((), 0, (z,)) == 1
    n = 400
    rng = np.random.default_rng(4)
    others = np.arange(1000, 1050, dtype=np.uint64)
    col = np.concatenate([np.full(5, z, dtype=np.uint64), others,
                          others[rng.integers(0, 50, n - 55)]])
    assert col.dtype == np.uint64 and int(col[0]) == z
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", rng.permutation(col))
    return QC.Case("zero_pair", uplan([[RRT]]), [seg],
                   extra={"want": {(): [51]}})


def family_plans() -> Dict[str, Plan]:
    """name -> plan over query_cases.sources_case(); names ending in _nokg
    run with kg=None. request_domain is dictionary-encoded in this store
    (SRC_DID); the pooled-string family is exercised through
    http_user_agent, which has empty strings on every 4th row."""
    ua = (Q.SRC_STR_HASH, S.POOL_POS["http_user_agent"])
    return {
        "u64": uplan([[FLOW]], [K_PROTO]),
        "u32": uplan([[(Q.SRC_U32, U32["server_port"])]], [K_PROTO]),
        "u8": uplan([[STATUS]], [K_PROTO]),
        "did_minus_one": uplan([[DID2]], [K_PROTO]),
        "str_hash": uplan([[ua]], [K_PROTO]),
        "trace128_trace": uplan([[(Q.SRC_TRACE128, 0)]], [K_PROTO]),
        "trace128_span": uplan([[(Q.SRC_TRACE128, 1)]]),
        "kg_pod": uplan([[(Q.SRC_KG, 0)], [(Q.SRC_KG, S.N_KG + 10)]],
                        [K_PROTO]),
        "kg_pod_nokg": uplan([[(Q.SRC_KG, 0)]], [K_PROTO]),
        "time_bucket_key": uplan([[STATUS], [ua, DID2]],
                                 [Key(Q.SRC_TIME_BUCKET, 0, 60)]),
        "time_bucket_arg": uplan([[(Q.SRC_TIME_BUCKET, 0)]], [K_PROTO]),
        "filtered_mixed": uplan(
            [[STATUS, DID2]], [K_PROTO],
            [Term(Q.SRC_U32, U32["server_port"], Q.OP_NE, 65535),
             Term(Q.SRC_U8, U8["response_status"], Q.OP_EQ, 1, group=1),
             Term(Q.SRC_U8, U8["response_status"], Q.OP_EQ, 3, group=1)],
            extra_aggs=[QC.COUNT, Agg(Q.AGGOP_MAX, Q.SRC_U64, U64["rrt"])]),
    }


def window_segment():
    """700 rows, capacity 1024; every row carries its own value, so any
    row outside the launched window would raise the count."""
    seg = QC.new_segment(700, capacity=1024)
    QC.set_u64(seg, "rrt", np.arange(700, dtype=np.uint64) // 2)
    QC.set_u8(seg, "l7_protocol", np.where(np.arange(700) % 2 == 0, 20, 21))
    return seg


WINDOWS = [(0, 700), (0, 1), (699, 1), (255, 2), (100, 257), (256, 444)]


def two_segment_case() -> QC.Case:
    """Values 0..59 in the first segment, 40..99 in the second: 100
    distinct over both, not 120."""
    rng = np.random.default_rng(2)
    segs = []
    for n, cap, lo in ((900, 1024, 0), (300, 300, 40)):
        seg = QC.new_segment(n, capacity=cap)
        QC.set_u64(seg, "rrt", (lo + rng.integers(0, 60, n))
                   .astype(np.uint64))
        QC.set_u64(seg, "flow_id", rng.integers(0, 3, n))
        segs.append(seg)
    return QC.Case("two_segments", uplan([[RRT]], [K_FLOW]), segs)


def pair_overflow_case() -> QC.Case:
    """200 distinct pairs for a 64-slot pair table."""
    n = 1000
    rng = np.random.default_rng(64)
    vals = np.arange(7000, 7200, dtype=np.uint64)
    seg = QC.new_segment(n)
    QC.set_u64(seg, "rrt", np.concatenate(
        [vals, vals[rng.integers(0, 200, n - 200)]]))
    return QC.Case("pair_overflow", uplan([[RRT]]), [seg])


def group_overflow_case() -> QC.Case:
    """16 groups for a 4-slot group table."""
    n = 640
    rng = np.random.default_rng(16)
    seg = QC.new_segment(n)
    QC.set_u64(seg, "flow_id", (100 + np.arange(n) % 16).astype(np.uint64))
    QC.set_u64(seg, "rrt", rng.integers(0, 10, n))
    return QC.Case("group_overflow", uplan([[RRT]], [K_FLOW]), [seg])


def cpu_cases() -> List[QC.Case]:
    """Every whole-segment case (the CPU engine has no row window)."""
    out = [shape_case(1), shape_case(257), shape_case(3000),
           one_value_case(), all_distinct_case(), eviction_case(),
           group_in_pair_case(), two_items_case(), tuple_order_case(),
           multi_arg_case(), zero_pair_case(), two_segment_case(),
           pair_overflow_case(), group_overflow_case()]
    src = QC.sources_case()
    for name, p in family_plans().items():
        out.append(QC.Case("fam_" + name, p, src.segs,
                           None if name.endswith("_nokg") else src.kg))
    return out


# ------------------------------------------------ generated data and SQL

def gen_cfg(seed: int = 15, n: int = 1500):
    from deepflow_amd.gen import SpanGenConfig
    return SpanGenConfig(n=n, seed=seed, tag_cardinality=60, n_attrs=2,
                         n_ips=48, n_services=5, n_resources=12)


def l7_engine(device: str, l4: bool = False):
    """QueryEngine over 3000 generated spans in 2 segments: two batches
    from one tag universe, so values recur across the segments (and, with
    l4, over 400 generated flows)."""
    from deepflow_amd.gen.spans import gen_span_payload
    from deepflow_amd.ingest import L7IngestPipeline
    from deepflow_amd.query import QueryEngine
    from deepflow_amd.store.kg import KnowledgeGraphTable, default_platform
    cfg = gen_cfg()
    kg = KnowledgeGraphTable(capacity_pow2=1 << 12, device=device)
    kg.update(default_platform(cfg))
    pipe = L7IngestPipeline(device=device, segment_rows=1 << 11, kg=kg,
                            dict_capacity=1 << 14,
                            time_base_s=cfg.base_time_ns // 10**9)
    pipe.ingest_frame_payload(gen_span_payload(cfg))
    pipe.ingest_frame_payload(gen_span_payload(gen_cfg(seed=16)))
    l4p = None
    if l4:
        from deepflow_amd.gen import FlowGenConfig
        from deepflow_amd.gen.flows import gen_flow_payload
        from deepflow_amd.ingest.l4_pipeline import L4IngestPipeline
        fcfg = FlowGenConfig(n=400, seed=31, n_ips=32, n_epcs=4)
        l4p = L4IngestPipeline(device=device, segment_rows=1 << 9,
                               kg=KnowledgeGraphTable(capacity_pow2=1 << 10,
                                                      device=device),
                               time_base_s=fcfg.base_time_ns // 10**9)
        l4p.ingest_frame_payload(gen_flow_payload(fcfg))
    return QueryEngine(pipe, device=device, l4_pipeline=l4p)


WHERE = "WHERE response_status != 4"
MIXED_SQL = (
    "SELECT l7_protocol, Count(*) AS c, Uniq(ip4_0) AS clients, "
    "UniqExact(trace_id) AS traces, Avg(response_duration) "
    f"FROM l7_flow_log {WHERE} GROUP BY l7_protocol "
    "HAVING clients > 1 ORDER BY traces DESC LIMIT 3")
SINGLE_SQL = (
    "SELECT Count(*) AS c, Uniq(ip4_0) AS clients, "
    "UniqExact(trace_id) AS traces, Avg(response_duration) AS a "
    f"FROM l7_flow_log {WHERE}")
UNIQ_ONLY_SQL = "SELECT Uniq(ip4_0, server_port) AS pairs FROM l7_flow_log"
ROWS_SQL = ("SELECT l7_protocol, ip4_0, trace_id, server_port, "
            f"response_duration FROM l7_flow_log {WHERE} LIMIT 100000")
L4_SQL = ("SELECT protocol, Count(*) AS c, Uniq(ip4_0, ip4_1) AS peers, "
          "Uniq(server_port) AS ports FROM l4_flow_log GROUP BY protocol")
L4_ROWS_SQL = ("SELECT protocol, ip4_0, ip4_1, server_port "
               "FROM l4_flow_log LIMIT 100000")
# agreement GPU vs CPU vs ref_uniq on the executor level
AGREE_SQL = [
    MIXED_SQL, SINGLE_SQL, UNIQ_ONLY_SQL,
    "SELECT request_domain, Uniq(trace_id) AS t, Uniq(ip4_0, ip4_1) AS p, "
    "Uniq(endpoint) AS e, Uniq(pod_id_0) AS pods, Max(response_duration) "
    "AS m FROM l7_flow_log GROUP BY request_domain",
    "SELECT time(60), Uniq(span_id) AS s, Uniq(http_user_agent) AS ua "
    "FROM l7_flow_log GROUP BY time(60)",
]


def host_mixed(rows: List[list]) -> Dict:
    """Per l7_protocol: (count, distinct ip4_0, distinct trace_id, avg
    duration) from SELECT rows (columns of ROWS_SQL)."""
    acc: Dict = {}
    for proto, ip, trace, _port, dur in rows:
        a = acc.setdefault(proto, [0, set(), set(), 0])
        a[0] += 1
        a[1].add(ip)
        a[2].add(trace)
        a[3] += dur
    return {k: (a[0], len(a[1]), len(a[2]), a[3] / a[0])
            for k, a in acc.items()}


def check_mixed_sql(eng, row_eng, key: str) -> None:
    """MIXED_SQL grouped by `key` on `eng` against a host computation from
    `row_eng`'s SELECT rows."""
    host = host_mixed(row_eng.query(
        ROWS_SQL.replace("l7_protocol", key))["values"])
    sql = MIXED_SQL.replace("l7_protocol", key)
    r = eng.query(sql)
    assert r["columns"] == [key, "c", "clients", "traces",
                            "avg(response_duration)"]
    kept = sorted((h[2] for h in host.values() if h[1] > 1), reverse=True)
    assert len(r["values"]) == min(3, len(kept))
    if key != "l7_protocol":
        assert len(kept) > 3 and len(set(kept)) == len(kept)
    for k, c, clients, traces, avg in r["values"]:
        assert (c, clients, traces) == host[k][:3]
        assert abs(avg - host[k][3]) < 1e-9
        assert clients > 1
    assert [row[3] for row in r["values"]] == kept[:3]
    # every group, through the form without HAVING / ORDER BY / LIMIT
    full = eng.query(sql.split(" HAVING")[0])
    assert {row[0]: tuple(row[1:4]) for row in full["values"]} == \
        {k: h[:3] for k, h in host.items()}


def plan_for(eng, sql: str) -> Plan:
    from deepflow_amd.query.sql import parse_sql
    from deepflow_amd.query.tags import L7_TAGS, L7_METRICS
    return parse_sql(sql, dictionary=eng.pipe.dict,
                     time_base_s=eng.pipe.time_base_s, tags=L7_TAGS,
                     metrics=L7_METRICS, name_maps=eng.name_maps)
