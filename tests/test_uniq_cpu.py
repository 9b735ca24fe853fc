"""K15 Uniq / UniqExact on the CPU engine: the parser, the executor against
the brute-force reference of uniq_cases.py, SQL through QueryEngine, the
distributed merge and derived rows. Everything is integer and compared
exactly, as dicts."""
import ctypes as ct

import pytest

import query_cases as QC
import uniq_cases as UC
from deepflow_amd.query import spec as Q
from deepflow_amd.query.executor import execute_agg_cpu
from deepflow_amd.query.sql import SqlError, parse_sql


# ---------------------------------------------------------------- hashing

def test_unmix64_inverts_mix64():
    from deepflow_amd.ops.ref import mix64
    for z in (0, 1, 5, UC.M64, 1 << 63, UC.UNIQ_SEED, 0x243F6A8885A308D3):
        assert UC.unmix64(mix64(z)) == z
        assert mix64(UC.unmix64(z)) == z


def test_pair_hash_properties():
    assert Q.UNIQ_SEED == UC.UNIQ_SEED
    assert UC.pair_hash((), 0, (5,)) != UC.pair_hash((), 1, (5,))
    assert UC.pair_hash((1,), 0, (5,)) != UC.pair_hash((2,), 0, (5,))
    assert UC.pair_hash((), 0, (1, 2)) != UC.pair_hash((), 0, (2, 1))
    assert UC.pair_hash((), 0, (UC.zero_pair_value(),)) == 1
    a, b = UC.values_sharing_filter_slot()
    assert a != b
    assert UC.filter_index(UC.pair_hash((), 0, (a,))) == \
        UC.filter_index(UC.pair_hash((), 0, (b,)))


# ----------------------------------------------------------------- parser

def test_uniq_spec_layout():
    # QUniqCol {u8, u16} = 4 bytes; QUniq = 4 cols + n_args = 20 bytes;
    # UniqSpec = 4 items + n_uniq (test_uniq_gpu.py compares the total
    # with the library's sizeof)
    assert ct.sizeof(Q.QUniqColC) == 4
    assert ct.sizeof(Q.QUniqC) == 4 * Q.QMAX_UNIQ_ARGS + 4
    assert ct.sizeof(Q.UniqSpecC) == 20 * Q.QMAX_UNIQ + 4
    p = UC.uplan([[UC.RRT, UC.IP0], [UC.STATUS]])
    c = Q.UniqSpecC.from_buffer_copy(p.uniq_to_bytes())
    assert c.n_uniq == 2
    assert (c.items[0].n_args, c.items[1].n_args) == (2, 1)
    assert (c.items[0].cols[1].family, c.items[0].cols[1].idx) == UC.IP0
    assert (c.items[1].cols[0].family, c.items[1].cols[0].idx) == UC.STATUS


@pytest.mark.parametrize("func", ["Uniq", "UniqExact", "uniq", "UNIQEXACT",
                                  "uniqExact"])
def test_parse_spellings_and_alias(func):
    p = parse_sql(f"SELECT {func}(ip4_0) AS clients, {func}(trace_id) "
                  f"FROM l7_flow_log")
    assert p.agg_names == ["clients", f"{func.lower()}(trace_id)"]
    assert [m["op"] for m in p.agg_meta] == ["uniq", "uniq"]
    assert [m["uniq"] for m in p.agg_meta] == [0, 1]
    assert p.uniqs[0].cols == [UC.IP0]
    assert p.uniqs[1].cols == [(Q.SRC_TRACE128, 0)]
    assert p.agg_meta[0]["cols"] == [UC.IP0]
    # one AGGOP_COUNT placeholder per item, no keys: a single group
    assert [(a.op, a.family) for a in p.aggs] == \
        [(Q.AGGOP_COUNT, Q.SRC_CONST0)] * 2
    assert not p.select_rows and p.keys == []


def test_parse_one_to_four_arguments():
    names = ["ip4_0", "server_port", "l7_protocol", "request_domain"]
    for k in range(1, 5):
        p = parse_sql(f"SELECT Uniq({', '.join(names[:k])}) AS u "
                      f"FROM l7_flow_log GROUP BY response_status")
        assert len(p.uniqs) == 1 and len(p.uniqs[0].cols) == k
        assert p.agg_names == ["u"]
    p = parse_sql("SELECT Uniq(ip4_0,server_port) FROM l7_flow_log")
    assert p.agg_names == ["uniq(ip4_0, server_port)"]
    assert p.uniqs[0].cols == [UC.IP0, (Q.SRC_U32, UC.U32["server_port"])]


def test_parse_every_family():
    p = parse_sql("SELECT Uniq(response_duration, ip4_0, l7_protocol, "
                  "request_domain) AS a, Uniq(pod_id_0, http_user_agent, "
                  "span_id, time) AS b FROM l7_flow_log")
    fams = [[f for f, _ in it.cols] for it in p.uniqs]
    assert fams == [[Q.SRC_U64, Q.SRC_U32, Q.SRC_U8, Q.SRC_DID],
                    [Q.SRC_KG, Q.SRC_STR_HASH, Q.SRC_TRACE128,
                     Q.SRC_TIME_BUCKET]]


def test_parse_mixes_with_other_aggregates():
    p = parse_sql("SELECT l7_protocol, Count(*) AS c, Uniq(ip4_0) AS u, "
                  "Avg(response_duration) AS a, Percentile(response_duration"
                  ", 90) AS p, UniqExact(trace_id) AS t FROM l7_flow_log "
                  "GROUP BY l7_protocol HAVING u > 1 ORDER BY t DESC "
                  "SLIMIT 5 LIMIT 3")
    assert [m["op"] for m in p.agg_meta] == \
        ["count", "uniq", "avg", "percentile", "uniq"]
    # count, uniq placeholder, sum + count, percentile placeholder, uniq
    assert len(p.aggs) == 6
    assert p.having == [("u", ">", 1.0)] and p.order_by == [("t", True)]
    assert (p.slimit, p.limit) == (5, 3)


@pytest.mark.parametrize("sql, says", [
    ("SELECT Uniq(attribute.foo) FROM l7_flow_log", "attribute"),
    ("SELECT Uniq(ip4_0, attribute.foo) FROM l7_flow_log", "attribute"),
    ("SELECT Uniq(*) FROM l7_flow_log", "*"),
    ("SELECT UniqExact() FROM l7_flow_log", "none"),
    ("SELECT Uniq(ip4_0, ip4_1, server_port, l7_protocol, vtap_id) "
     "FROM l7_flow_log", "at most 4 arguments"),
    ("SELECT Uniq(ip4_0) AS a, Uniq(ip4_1) AS b, Uniq(server_port) AS c, "
     "Uniq(l7_protocol) AS d, Uniq(vtap_id) AS e FROM l7_flow_log",
     "at most 4 Uniq"),
    ("SELECT Uniq(no_such_tag) FROM l7_flow_log", "unknown tag"),
    ("SELECT Uniq(ip4_0 ip4_1) FROM l7_flow_log", "expected"),
    ("SELECT Uniq(ip4_0, 5) FROM l7_flow_log", "expected"),
])
def test_parse_refusals(sql, says):
    with pytest.raises(SqlError) as e:
        parse_sql(sql)
    assert says in str(e.value)


def test_existing_plans_unchanged():
    """Every query_cases plan and a sample of SQL without Uniq still plan
    to the same bytes: no Uniq items, QuerySpec size as before."""
    size = ct.sizeof(Q.QuerySpecC)
    assert size == 472
    for case in QC.cpu_agg_cases():
        assert case.plan.uniqs == []
        assert len(case.plan.to_bytes()) == size
    for sql in ("SELECT Count(*) AS cnt FROM l7_flow_log",
                "SELECT request_domain, Count(*) AS c, Avg(response_duration)"
                " AS a, Percentile(response_duration, 90) AS p "
                "FROM l7_flow_log WHERE server_port IN (80, 443) "
                "GROUP BY request_domain ORDER BY c DESC LIMIT 5"):
        p = parse_sql(sql)
        assert p.uniqs == [] and len(p.to_bytes()) == size
        assert all(m["op"] != "uniq" for m in p.agg_meta)
    empty = Q.UniqSpecC.from_buffer_copy(parse_sql(
        "SELECT Count(*) FROM l7_flow_log").uniq_to_bytes())
    assert empty.n_uniq == 0


# --------------------------------------------------------------- executor

@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in UC.cpu_cases()}


@pytest.mark.parametrize("name", [c.name for c in UC.cpu_cases()])
def test_cpu_executor_matches_reference(cases, name):
    case = cases[name]
    want = UC.ref_counts(case.plan, case.segs, case.kg)
    if "want" in case.extra:
        assert want == case.extra["want"]
    groups = execute_agg_cpu(case.plan, case.segs, kg=case.kg)
    assert UC.engine_counts(groups) == want
    # the placeholders are row counts: the other aggregates are untouched
    assert {tuple(g["key"]): g["agg"] for g in groups} == \
        QC.ref_agg(case.plan, case.segs, case.kg)


def test_cpu_no_match_and_no_uniq(cases):
    seg = cases["shape_3000"].segs
    assert execute_agg_cpu(UC.no_match_plan(), seg) == []
    plain = QC.plan([], [UC.K_PROTO], [QC.COUNT])
    assert all("uniq" not in g for g in execute_agg_cpu(plain, seg))


def test_multi_arg_bounds(cases):
    case = cases["multi_arg"]
    for key, (ab, a, b, abcd) in UC.ref_counts(case.plan, case.segs).items():
        rows = QC.ref_agg(case.plan, case.segs)[key][0]
        assert max(a, b) <= ab <= abcd <= rows
        assert ab > max(a, b)          # the data does have more tuples


# -------------------------------------------------------------------- SQL

@pytest.fixture(scope="module")
def eng():
    return UC.l7_engine("cpu", l4=True)


def test_engine_data_shape(eng):
    segs = [s for s in eng.pipe.segments.scan_list() if s.n_rows]
    assert len(segs) == 2 and sum(s.n_rows for s in segs) == 3000


@pytest.mark.parametrize("sql", UC.AGREE_SQL)
def test_cpu_engine_matches_reference(eng, sql):
    plan = UC.plan_for(eng, sql)
    segs = eng.pipe.segments.scan_list()
    groups = execute_agg_cpu(plan, segs, kg=eng.pipe.kg)
    assert UC.engine_counts(groups) == \
        UC.ref_counts(plan, segs, eng.pipe.kg)


@pytest.mark.parametrize("key", ["l7_protocol", "request_domain"])
def test_mixed_sql(eng, key):
    """The issue's query (the generator emits one l7_protocol, so the same
    text also runs grouped by request_domain, where HAVING, ORDER BY and
    LIMIT have groups to act on)."""
    UC.check_mixed_sql(eng, eng, key)


def test_single_group_sql(eng):
    rows = eng.query(UC.ROWS_SQL)["values"]
    r = eng.query(UC.SINGLE_SQL)
    assert r["columns"] == ["c", "clients", "traces", "a"]
    assert len(r["values"]) == 1
    c, clients, traces, _ = r["values"][0]
    assert c == len(rows)
    assert clients == len({x[1] for x in rows})
    assert traces == len({x[2] for x in rows})


def test_uniq_only_sql(eng):
    rows = eng.query("SELECT ip4_0, server_port FROM l7_flow_log "
                     "LIMIT 100000")["values"]
    assert eng.query(UC.UNIQ_ONLY_SQL) == \
        {"columns": ["pairs"], "values": [[len({tuple(x) for x in rows})]]}


def test_slimit_on_alias(eng):
    r = eng.query("SELECT l7_protocol, Uniq(ip4_0) AS clients "
                  "FROM l7_flow_log GROUP BY l7_protocol SLIMIT 2")
    full = eng.query("SELECT l7_protocol, Uniq(ip4_0) AS clients "
                     "FROM l7_flow_log GROUP BY l7_protocol")
    top = sorted((row[1] for row in full["values"]), reverse=True)[:2]
    assert sorted((row[1] for row in r["values"]), reverse=True) == top


def test_l4_sql(eng):
    rows = eng.query(UC.L4_ROWS_SQL)["values"]
    assert len(rows) == 400
    want = {}
    for proto, ip0, ip1, port in rows:
        a = want.setdefault(proto, [0, set(), set()])
        a[0] += 1
        a[1].add((ip0, ip1))
        a[2].add(port)
    r = eng.query(UC.L4_SQL)
    assert r["columns"] == ["protocol", "c", "peers", "ports"]
    assert {row[0]: row[1:] for row in r["values"]} == \
        {k: [a[0], len(a[1]), len(a[2])] for k, a in want.items()}


def test_derived_rows(eng):
    inner = ("SELECT l7_protocol, ip4_0, Count(*) AS c FROM l7_flow_log "
             "GROUP BY l7_protocol, ip4_0")
    rows = eng.query(inner)["values"]
    r = eng.query(f"WITH t AS ({inner}) SELECT Uniq(ip4_0) AS ips, "
                  f"Uniq(l7_protocol, ip4_0) AS pairs, Sum(c) AS n FROM t")
    assert r["values"] == [[len({x[1] for x in rows}), len(rows), 3000]]
    per = eng.query(f"SELECT l7_protocol, Uniq(ip4_0) AS ips FROM ({inner}) "
                    f"t GROUP BY l7_protocol")
    want = {}
    for proto, ip, _ in rows:
        want.setdefault(proto, set()).add(ip)
    assert {x[0]: x[1] for x in per["values"]} == \
        {k: len(v) for k, v in want.items()}
    # and it equals the direct distinct count per group
    direct = eng.query("SELECT l7_protocol, Uniq(ip4_0) AS ips "
                       "FROM l7_flow_log GROUP BY l7_protocol")
    assert sorted(map(tuple, direct["values"])) == \
        sorted(map(tuple, per["values"]))


# ------------------------------------------------------------ distributed

def test_merge_agg_partials_uniq():
    from deepflow_amd.parallel.dist_query import merge_agg_partials
    ops = [Q.AGGOP_COUNT, Q.AGGOP_COUNT]
    a = {"key_rows": [["x"], ["y"]], "aggs": [[3, 3], [1, 1]],
         "agg_ops": ops, "uniq": [[2], [1]]}
    b = {"key_rows": [["z"]], "aggs": [[5, 5]], "agg_ops": ops,
         "uniq": [[4]]}
    m = merge_agg_partials([a, b])
    assert dict(zip((k[0] for k in m["key_rows"]), m["uniq"])) == \
        {"x": [2], "y": [1], "z": [4]}
    assert dict(zip((k[0] for k in m["key_rows"]), m["aggs"])) == \
        {"x": [3, 3], "y": [1, 1], "z": [5, 5]}
    c = {"key_rows": [["y"]], "aggs": [[2, 2]], "agg_ops": ops,
         "uniq": [[2]]}
    with pytest.raises(ValueError, match="Uniq does not merge across "
                                         "shards"):
        merge_agg_partials([a, c])
    # without Uniq data the same shapes still add
    for p in (a, c):
        del p["uniq"]
    m = merge_agg_partials([a, c])
    assert "uniq" not in m
    assert dict(zip((k[0] for k in m["key_rows"]), m["aggs"]))["y"] == [3, 3]


def test_world1_dist_engine(eng, tmp_path):
    import torch.distributed as dist
    from deepflow_amd.parallel.dist_query import DistQueryEngine
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        deng = DistQueryEngine(eng, device="cpu")
        for sql in (UC.MIXED_SQL, UC.SINGLE_SQL, UC.UNIQ_ONLY_SQL, UC.L4_SQL,
                    "SELECT l7_protocol, Uniq(ip4_0) AS clients FROM "
                    "l7_flow_log GROUP BY l7_protocol SLIMIT 2"):
            assert deng.query(sql) == eng.query(sql), sql
        part = eng.query_partial(UC.MIXED_SQL)
        assert part["kind"] == "agg"
        assert len(part["uniq"]) == len(part["key_rows"])
        assert all(len(u) == 2 for u in part["uniq"])
    finally:
        dist.destroy_process_group()
