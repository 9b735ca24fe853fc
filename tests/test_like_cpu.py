"""DF-SQL LIKE / REGEXP on dictionary tags (K16) without a GPU: the LIKE
translation, the parser, the id-set semantics through the CPU executor
against the string-level reference of like_cases.py, SQL through
QueryEngine, and the device arena's bookkeeping on a CPU device. Every
comparison is of exact integers or exact sets."""
import re
from collections import Counter

import numpy as np
import pytest

import like_cases as LC
import query_cases as QC
import uniq_cases as UC
from deepflow_amd.query import executor as EX
from deepflow_amd.query import spec as Q
from deepflow_amd.query.logregex import compile_log_regex
from deepflow_amd.query.sql import SqlError, like_to_regex, parse_sql
from deepflow_amd.query.tags import L4_METRICS, L4_TAGS

SEL = "SELECT Count(*) AS c FROM l7_flow_log WHERE "


# ------------------------------------------------------------ translation

@pytest.mark.parametrize("pattern,regex,literal", LC.LIKE_TABLE)
def test_like_translation_table(pattern, regex, literal):
    assert like_to_regex(pattern) == (regex, literal)
    compile_log_regex(regex)                    # inside the DFA subset


@pytest.mark.parametrize("pattern,value,want", LC.LIKE_VALUES)
def test_like_translation_meaning(pattern, value, want):
    regex, _ = like_to_regex(pattern)
    assert (re.fullmatch(regex.encode(), value) is not None) == want
    assert LC.like_match(pattern, value) == want
    assert compile_log_regex(regex).search_py(value) == want


# ----------------------------------------------------------------- parser

@pytest.fixture(scope="module")
def hand():
    return LC.hand_dictionary(), LC.hand_segment()


@pytest.mark.parametrize("text,kind,op", [
    ("request_resource LIKE 'x%'", "like", Q.OP_INSET),
    ("request_resource NOT LIKE 'x%'", "like", Q.OP_NOT_INSET),
    ("request_resource REGEXP '^x'", "regexp", Q.OP_INSET),
    ("request_resource NOT REGEXP '^x'", "regexp", Q.OP_NOT_INSET),
    ("request_resource not  like 'x%'", "like", Q.OP_NOT_INSET),
    ("request_resource rEgExP '^x'", "regexp", Q.OP_INSET),
    ("`request_resource` Like 'x%'", "like", Q.OP_INSET),
    ("app_service LIKE 'x%'", "like", Q.OP_INSET),
])
def test_parse_operators(hand, text, kind, op):
    plan = parse_sql(SEL + text, dictionary=hand[0])
    (t,) = plan.terms
    (ps,) = plan.sets
    assert (t.family, t.op, t.v0, t.group) == (Q.SRC_DID, op, 0, 0)
    assert ps.kind == kind and not ps.complement
    assert ps.dictionary is hand[0]
    assert ps.domain == (5 if text.startswith("app_service") else LC.DOM_RES)


def test_parse_empty_match_swaps_op(hand):
    """A pattern that matches b'' is stored as the ids that do not match."""
    for text, op in [("LIKE '%'", Q.OP_NOT_INSET),
                     ("NOT LIKE '%'", Q.OP_INSET),
                     ("REGEXP 'a*'", Q.OP_NOT_INSET),
                     ("NOT REGEXP '^$'", Q.OP_INSET)]:
        plan = parse_sql(SEL + "request_resource " + text,
                         dictionary=hand[0])
        assert plan.terms[0].op == op and plan.sets[0].complement, text


def test_parse_or_clause_and_in(hand):
    plan = parse_sql(
        SEL + "(request_resource LIKE '/user/%' OR request_domain NOT "
        "REGEXP 'com$' OR response_code = 500) AND request_domain IN "
        "('example.com', 'nope') AND request_resource LIKE '%s'",
        dictionary=hand[0])
    assert [(t.family, t.op, t.group) for t in plan.terms] == [
        (Q.SRC_DID, Q.OP_INSET, 1), (Q.SRC_DID, Q.OP_NOT_INSET, 1),
        (Q.SRC_U32, Q.OP_EQ, 1), (Q.SRC_DID, Q.OP_EQ, 2),
        (Q.SRC_CONST0, Q.OP_EQ, 2), (Q.SRC_DID, Q.OP_INSET, 0)]
    assert [t.v0 for t in plan.terms if t.op in Q.SET_OPS] == [0, 1, 2]
    assert [ps.pattern for ps in plan.sets] == ["/user/%", "com$", "%s"]


@pytest.mark.parametrize("like,eq", [
    ("request_resource LIKE '/health'", "request_resource = '/health'"),
    ("request_resource NOT LIKE '/health'", "request_resource != '/health'"),
    ("request_resource LIKE 'unknown'", "request_resource = 'unknown'"),
    ("request_resource NOT LIKE 'unknown'", "request_resource != 'unknown'"),
    ("(request_resource LIKE 'unknown' OR request_resource LIKE 'a\\_b')",
     "(request_resource = 'unknown' OR request_resource = 'a_b')"),
])
def test_wildcard_free_like_is_equality(hand, like, eq):
    a = parse_sql(SEL + like, dictionary=hand[0])
    b = parse_sql(SEL + eq, dictionary=hand[0])
    assert a.terms == b.terms and a.impossible == b.impossible
    assert a.sets == [] and not a.has_sets()


@pytest.mark.parametrize("text,says", [
    ("http_user_agent LIKE 'curl%'", "http_user_agent"),       # strhash
    ("x_request_id_0 REGEXP '^a'", "x_request_id_0"),
    ("trace_id LIKE 'ab%'", "trace_id"),                       # tracebin
    ("ip6_0 LIKE 'fe80%'", "ip6_0"),                           # ip6str
    ("attribute.foo LIKE 'a%'", "attribute.foo"),
    ("response_code LIKE '5%'", "response_code"),              # numeric
    ("l7_protocol REGEXP 'HTTP'", "l7_protocol"),
    ("time LIKE '1%'", "time"),
    ("request_resource LIKE 5", "string"),
    ("request_resource NOT REGEXP 12", "string"),
    ("request_resource REGEXP 'a\\b'", r"\b"),
    ("request_resource REGEXP '(a)\\1'", "backreference"),
    ("request_resource REGEXP '(?i)a'", "inline flags"),
    ("request_resource REGEXP '" + "(a|b)" * 60 + "'", "too complex"),
    ("request_resource REGEXP '(a'", "invalid pattern"),
])
def test_parse_refusals(hand, text, says):
    with pytest.raises(SqlError) as e:
        parse_sql(SEL + text, dictionary=hand[0])
    assert says in str(e.value)


def test_l4_and_missing_dictionary_are_refused(hand):
    with pytest.raises(SqlError) as e:
        parse_sql("SELECT Count(*) FROM l4_flow_log WHERE ip6_0 LIKE 'a%'",
                  tags=L4_TAGS, metrics=L4_METRICS)
    assert "ip6_0" in str(e.value)
    with pytest.raises(SqlError) as e:
        parse_sql("SELECT Count(*) FROM l4_flow_log WHERE protocol LIKE '6%'",
                  tags=L4_TAGS, metrics=L4_METRICS)
    assert "protocol" in str(e.value)
    # ids are shard-local: without the shard's dictionary a pattern term
    # must not compile to "impossible"
    with pytest.raises(SqlError) as e:
        parse_sql(SEL + "request_resource LIKE 'a%'", dictionary=None)
    assert "dictionary" in str(e.value)


def test_kgname_id_limit():
    with pytest.raises(SqlError) as e:
        parse_sql(SEL + "pod_name_0 LIKE 'a%'",
                  name_maps={"pod": {1: "a", Q.SET_MAX_BITS: "b"}})
    assert "pod_name_0" in str(e.value)
    plan = parse_sql(SEL + "pod_name_0 LIKE 'a%'",
                     name_maps={"pod": {1: "a", Q.SET_MAX_BITS - 1: "ab"}})
    assert plan.terms[0].family == Q.SRC_KG


def test_unbound_plan_does_not_serialise(hand):
    plan = parse_sql(SEL + "request_resource LIKE 'x%'", dictionary=hand[0])
    with pytest.raises(RuntimeError):
        plan.to_bytes()
    spec = plan.to_bytes(sets=[(0x7F0000001000, 1024)])
    c = Q.QuerySpecC.from_buffer_copy(spec)
    assert (c.terms[0].v0, c.terms[0].v1) == (0x7F0000001000, 1024)
    # plans without set terms serialise as before
    plain = parse_sql(SEL + "request_resource = '/health'",
                      dictionary=hand[0])
    assert len(plain.to_bytes()) == len(spec) == \
        len(bytes(memoryview(Q.QuerySpecC())))


def test_plan_needed_reports_set_columns(hand):
    from deepflow_amd.query.engine import _plan_needed
    plan = parse_sql(SEL + "request_resource LIKE 'x%' AND pod_name_0 "
                     "LIKE 'p%'", dictionary=hand[0],
                     name_maps={"pod": {1: "p1"}})
    need = _plan_needed(plan)
    assert LC.DID_RES in need[Q.SRC_DID]
    assert plan.terms[1].idx in need[Q.SRC_KG]


# ------------------------------------------------------- bitmap semantics

@pytest.mark.parametrize("where,cnf", LC.HAND_WHERE,
                         ids=[w for w, _ in LC.HAND_WHERE])
def test_cpu_executor_matches_string_reference(hand, where, cnf):
    d, seg = hand
    plan = parse_sql("SELECT start_time FROM l7_flow_log WHERE " + where +
                     " LIMIT 100000", dictionary=d)
    got = EX.execute(plan, [seg], "cpu")
    want = LC.hand_ref_rows(seg, cnf)
    assert {r for _, r in got} == want and len(got) == len(want)
    agg = parse_sql(SEL + where, dictionary=d)
    groups = EX.execute(agg, [seg], "cpu")
    assert groups == ([{"key": [], "agg": [len(want)]}] if want else [])


def test_reference_covers_the_edges(hand):
    """The cases mean something: empty rows exist and the four empty-value
    cases select different row sets."""
    _, seg = hand
    n = seg.n_rows
    empty = {r for r in range(n)
             if LC.hand_values(seg, r)["request_resource"] is None}
    assert 0 < len(empty) < n
    by = {w: LC.hand_ref_rows(seg, c) for w, c in LC.HAND_WHERE[:6]}
    R = LC.R
    assert by[f"{R} LIKE '%'"] == set(range(n))
    assert by[f"{R} NOT LIKE '%'"] == set()
    assert by[f"{R} LIKE 'x%'"] and not by[f"{R} LIKE 'x%'"] & empty
    assert empty < by[f"{R} NOT LIKE 'x%'"] < set(range(n))
    assert by[f"{R} LIKE '%nothing-like-this%'"] == set()
    assert by[f"{R} LIKE '%_%'"] == set(range(n)) - empty


def test_host_bitmap_is_python_re(hand):
    d, _ = hand
    plan = parse_sql(SEL + "request_resource REGEXP '^/user/[0-9]+$'",
                     dictionary=d)
    (words, nbits), = EX.bind_sets(plan, "cpu")[0]
    assert nbits == LC.HAND_CAPACITY and words.dtype == np.uint32
    got = {i for i in range(nbits) if (int(words[i >> 5]) >> (i & 31)) & 1}
    assert got == {31}
    assert EX.bind_sets(plan, "cpu")[0][0][0] is words      # built once


# ------------------------------------------------------------------ arena

def _arena_strings(a):
    data = a.data[:a.nbytes].numpy().tobytes()
    off = a.off[:a.n].numpy().view(np.uint32).tolist()
    ln = a.lens[:a.n].numpy().view(np.uint16).tolist()
    ids = a.ids[:a.n].numpy().view(np.uint32).tolist()
    assert off == [sum(ln[:i]) for i in range(a.n)]      # back to back
    return {i: data[o:o + n] for i, o, n in zip(ids, off, ln)}


def test_arena_catches_up_incrementally():
    d = LC.hand_dictionary()
    a = d.arena(LC.DOM_RES, "cpu")
    assert _arena_strings(a) == LC.RES_STRINGS
    assert (a.uploads, a.h2d_copies) == (1, 2)
    assert d.arena(LC.DOM_RES, "cpu") is a
    assert (a.uploads, a.h2d_copies) == (1, 2)           # nothing new: O(1)
    # new entries by every road: harvest writes the maps directly,
    # import_entries merges, a checkpoint restore update()s
    d.id_to_str[(LC.DOM_RES, 7)] = b"/new/7"
    d.import_entries([(LC.DOM_RES, 8, b"/new/8"), (LC.DOM_DOMAIN, 9, b"dom"),
                      (LC.DOM_RES, 3, b"ignored: id 3 is taken")])
    d.id_to_str.update({(LC.DOM_RES, 500 + i): b"/bulk/%d" % i
                        for i in range(400)})
    want = dict(LC.RES_STRINGS)
    want.update({7: b"/new/7", 8: b"/new/8"})
    want.update({500 + i: b"/bulk/%d" % i for i in range(400)})
    b = d.arena(LC.DOM_DOMAIN, "cpu")                    # another domain
    assert _arena_strings(b) == {**LC.DOMAIN_STRINGS, 9: b"dom"}
    assert (a.uploads, a.n) == (1, len(LC.RES_STRINGS))  # a not touched yet
    assert d.arena(LC.DOM_RES, "cpu") is a
    assert _arena_strings(a) == want
    assert (a.uploads, a.h2d_copies) == (2, 4)           # grew by doubling
    assert a.off.numel() >= a.n and a.off.numel() & (a.off.numel() - 1) == 0
    d.arena(LC.DOM_RES, "cpu")
    assert (a.uploads, a.h2d_copies) == (2, 4)


# ----------------------------------------------------------------- engine

@pytest.fixture(scope="module")
def eng():
    e = UC.l7_engine("cpu")
    e.name_maps = {"pod": LC.pod_names(e)}
    return e


def _rows(eng, cols):
    res = eng.query(f"SELECT {', '.join(cols)} FROM l7_flow_log "
                    "LIMIT 100000")
    assert res["columns"] == cols and len(res["values"]) == 3000
    return res["values"]


def _b(s):
    return None if s is None else s.encode()


def test_engine_grouped_count(eng):
    rows = _rows(eng, ["request_domain", "request_resource"])
    want = Counter(d for d, r in rows
                   if LC.like_match("%/r/0000_", _b(r) or b""))
    assert want and sum(want.values()) < 3000
    got = eng.query(LC.ENGINE_SQL[0])
    assert {d: c for d, c in got["values"]} == dict(want)


def test_engine_not_like_and_or(eng):
    rows = _rows(eng, ["request_resource", "service_name",
                       "response_status"])
    want = sum(1 for r, s, st in rows
               if (LC.like_match("%3", _b(r) or b"") or
                   LC.like_match("svc-__4", _b(s) or b""))
               and st != "Client Error")
    assert 0 < want < 3000
    assert eng.query(LC.ENGINE_SQL[5])["values"] == [[want]]
    keep = Counter(r for r, _, _ in rows
                   if not LC.like_match("*1", _b(r) or b""))
    got = eng.query(LC.ENGINE_SQL[1])
    assert {r[0]: r[1] for r in got["values"]} == dict(keep)


def test_engine_uniq(eng):
    rows = _rows(eng, ["request_domain", "ip4_0"])
    hit = [ip for d, ip in rows if re.search(rb"^svc-00[12]", _b(d) or b"")]
    assert 0 < len(hit) < 3000
    assert eng.query(LC.ENGINE_SQL[2])["values"] == \
        [[len(hit), len(set(hit))]]


def test_engine_percentile_equals_in_list(eng):
    names = sorted({r for (r,) in _rows(eng, ["request_resource"])
                    if r and r.endswith("1")})
    assert names
    in_list = ", ".join(f"'{n}'" for n in names)
    want = eng.query(LC.ENGINE_SQL[4].replace(
        "request_resource LIKE '%1'", f"request_resource IN ({in_list})"))
    got = eng.query(LC.ENGINE_SQL[4])
    assert LC.sorted_result(got) == LC.sorted_result(want)
    assert got["values"] and all(r[1] is not None for r in got["values"])


def test_engine_select_rows(eng):
    cols = ["request_domain", "request_resource", "response_code"]
    want = [r for r in _rows(eng, cols)
            if re.search(rb"r/0+[2-5]$", _b(r[1]) or b"") and
            LC.like_match("svc-00_.example.com", _b(r[0]) or b"")]
    got = eng.query(LC.ENGINE_SQL[6])
    assert got["columns"] == cols and 0 < len(want) < 3000
    assert sorted(got["values"]) == sorted(want)


def test_engine_kgname(eng):
    names = eng.name_maps["pod"]
    assert any(n.startswith("pod-1") for n in names.values())
    res = eng.query("SELECT pod_id_0, Count(*) AS c FROM l7_flow_log "
                    "GROUP BY pod_id_0")
    by_id = {pid: c for pid, c in res["values"]}
    unnamed = [p for p in by_id if p not in names]
    assert unnamed and 10 in unnamed             # pod_names leaves them out
    want = {names[p]: c for p, c in by_id.items()
            if p in names and names[p].startswith("pod-1")}
    got = eng.query(LC.ENGINE_SQL[7])
    assert {n: c for n, c in got["values"]} == want and want
    # an id without a name (and id 0, no KG hit) behaves as '':
    # NOT LIKE 'pod-%' keeps exactly those rows
    assert eng.query(LC.ENGINE_SQL[8])["values"] == \
        [[sum(by_id[p] for p in unnamed)]]


def test_engine_everything_and_nothing(eng):
    assert eng.query(LC.ENGINE_SQL[9])["values"] == [[3000]]
    assert eng.query(LC.ENGINE_SQL[10])["values"] == [[3000]]
    assert eng.query("SELECT Count(*) AS c FROM l7_flow_log WHERE "
                     "request_resource LIKE '%nothing%'")["values"] == []


def test_engine_cte_over_raw_rows(eng):
    inner = eng.query("SELECT request_domain, Count(*) AS c FROM "
                      "l7_flow_log GROUP BY request_domain")
    want = [r for r in inner["values"]
            if LC.like_match("svc-00_.%", _b(r[0]) or b"") and
            not re.search(rb"svc-00[03]", _b(r[0]) or b"")]
    got = eng.query(LC.ENGINE_SQL[11])
    assert got["columns"] == ["request_domain", "c"]
    assert sorted(got["values"]) == sorted(want) and 0 < len(want) < 5


def test_world1_dist_engine(eng, tmp_path):
    import torch.distributed as dist
    from deepflow_amd.parallel.dist_query import DistQueryEngine
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        deng = DistQueryEngine(eng, device="cpu")
        for sql in (LC.ENGINE_SQL[0], LC.ENGINE_SQL[2], LC.ENGINE_SQL[11]):
            assert LC.sorted_result(deng.query(sql)) == \
                LC.sorted_result(eng.query(sql)), sql
    finally:
        dist.destroy_process_group()
