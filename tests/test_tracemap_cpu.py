"""Bulk trace assembly (query/tracemap.py host twin) against the unchanged
per-trace `DistributedTracer.assemble()` and against hand-written
expectations, on a span set that spans several 256-row segments.

The cpu engine's SELECT returns rows in store order (checked below), so
assemble()'s first-wins dictionaries see the same order as the global row
index and the duplicate-key cases take part in the cross-check.
"""
import os
import sys

import numpy as np
import pytest
from fastapi.testclient import TestClient

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracemap_cases as C  # noqa: E402

from deepflow_amd.ingest import L7IngestPipeline  # noqa: E402
from deepflow_amd.query import QueryEngine  # noqa: E402
from deepflow_amd.query.http_api import build_app  # noqa: E402
from deepflow_amd.query.tracemap import MAX_TRACE_HOPS, TraceMapper  # noqa: E402
from deepflow_amd.query.tracing import DistributedTracer  # noqa: E402


@pytest.fixture(scope="module")
def env():
    spans = C.build_spans()
    pipe = L7IngestPipeline(device="cpu", segment_rows=1 << 8,
                            dict_capacity=1 << 12)
    for payload in C.payloads_of(spans):
        pipe.ingest_frame_payload(payload)
    engine = QueryEngine(pipe, device="cpu")
    engine.trace_tree_rows = lambda: tracer.tree_rows
    tracer = DistributedTracer(engine)
    mapper = TraceMapper(engine)
    links = mapper.link_spans()
    tmap = mapper.trace_map()
    # reference: the per-trace path, once per trace id
    asm, asm_rows = {}, {}
    for t in C.trace_ids_of(spans):
        asm[t] = tracer.assemble(t)
        asm_rows[t] = tracer.tree_rows[-1]
    tracer.tree_rows.clear()
    return dict(spans=spans, pipe=pipe, engine=engine, tracer=tracer,
                mapper=mapper, links=links, tmap=tmap, asm=asm,
                asm_rows=asm_rows)


def _by_row(links):
    return {int(r): i for i, r in enumerate(links["row"])}


def _link(env, trace, sid, nth=0):
    """(parent span dict or None, kind, depth) of the nth span of `trace`
    with span id `sid`, via the global row = payload index identity."""
    rows = [g for g, s in enumerate(env["spans"])
            if s["trace_info"]["trace_id"] == trace and
            s["trace_info"]["span_id"] == sid]
    i = _by_row(env["links"])[rows[nth]]
    p = int(env["links"]["parent_row"][i])
    return (env["spans"][p] if p >= 0 else None,
            int(env["links"]["link_kind"][i]), int(env["links"]["depth"][i]))


def test_shape_of_the_set(env):
    spans = env["spans"]
    assert 1400 <= len(spans) <= 1700 and len(spans) % 64
    assert len(env["pipe"].segments.segments) >= 5
    n_traced = sum(1 for s in spans if s["trace_info"]["trace_id"])
    assert len(env["links"]["row"]) == n_traced == env["tmap"]["span_count"]
    assert env["tmap"]["drops"] == 0
    # rows without a trace id never take part
    rows = set(env["links"]["row"].tolist())
    assert all((g in rows) == bool(s["trace_info"]["trace_id"])
               for g, s in enumerate(spans))
    assert np.all(np.diff(env["links"]["row"]) > 0)


def test_select_returns_store_order(env):
    r = env["engine"].query(
        "SELECT span_id, start_time FROM l7_flow_log "
        f"WHERE trace_id = '{C.T_FAN}' LIMIT 10000")
    want = [[s["trace_info"]["span_id"], s["base"]["start_time"]]
            for s in env["spans"] if s["trace_info"]["trace_id"] == C.T_FAN]
    assert r["values"] == want


def test_links_match_assemble_for_every_trace(env):
    """parent span, roots, span_count, max_depth, root_service and
    duration_us of the bulk path equal assemble()'s, trace by trace."""
    spans, links = env["spans"], env["links"]
    by_row = _by_row(links)
    summaries = {t["trace_id"]: t for t in env["tmap"]["traces"]}
    assert len(summaries) == env["tmap"]["trace_count"] == len(env["asm"])
    for tid, a in env["asm"].items():
        rows = [g for g, s in enumerate(spans)
                if s["trace_info"]["trace_id"] == tid]
        assert a["span_count"] == len(rows), tid
        # assemble()'s node i is the trace's i-th row in store order
        for node, g in zip(a["spans"], rows):
            assert (node["span_id"] or "") == \
                spans[g]["trace_info"]["span_id"]
            p = int(links["parent_row"][by_row[g]])
            want = None if node["parent_index"] is None \
                else rows[node["parent_index"]]
            assert (p if p >= 0 else None) == want, (tid, g)
        s = summaries[tid]
        assert s["span_count"] == a["span_count"]
        assert s["root_count"] == len(a["roots"])
        row = env["asm_rows"][tid]
        assert row["trace_id"] == tid
        for k in ("time", "span_count", "max_depth", "root_service",
                  "duration_us"):
            assert s[k] == row[k], (tid, k)


def test_edges_match_assemble(env):
    want = {}
    for a in env["asm"].values():
        for n in a["spans"]:
            if n["parent_index"] is None:
                continue
            k = (a["spans"][n["parent_index"]]["service"] or "",
                 n["service"] or "")
            e = want.setdefault(k, [0, 0, 0])
            e[0] += 1
            e[1] += n["status"] in ("Server Error", "Client Error")
            e[2] += n["duration_ns"]
    got = {(e["parent_service"], e["child_service"]):
           [e["calls"], e["errors"], e["duration_ns_sum"]]
           for e in env["tmap"]["edges"]}
    assert got == want
    assert sum(e[1] for e in want.values()) > 0
    for e in env["tmap"]["edges"]:
        assert e["calls"] == e["calls_span"] + e["calls_syscall"] + \
            e["calls_tcp"]
    keys = [(e["parent_service"], e["child_service"])
            for e in env["tmap"]["edges"]]
    assert keys == sorted(keys)
    # spans without a service name are a legal edge end
    assert any(p == "" for p, _ in keys) and any(c == "" for _, c in keys)
    totals = [sum(e[k] for e in env["tmap"]["edges"])
              for k in ("calls_span", "calls_syscall", "calls_tcp")]
    assert all(totals)


def test_hand_written_cases(env):
    sid = lambda s: s["trace_info"]["span_id"]
    # chain 48 deep
    assert _link(env, C.T_CHAIN, C.hx(0x1000)) == (None, 0, 0)
    p, k, d = _link(env, C.T_CHAIN, C.hx(0x1000 + 47))
    assert (sid(p), k, d) == (C.hx(0x1000 + 46), 1, 47)
    # 300 children below a non-hex (pooled, hashed) span id
    p, k, d = _link(env, C.T_FAN, C.hx(0x2000 + 299))
    assert (sid(p), k, d) == ("s-root", 1, 1)
    # duplicated span id: the lowest row wins, the copy hangs below it
    first = next(s for s in env["spans"]
                 if s["trace_info"]["trace_id"] == C.T_DUP)
    assert _link(env, C.T_DUP, C.hx(0xD1), 0) == (None, 0, 0)
    assert _link(env, C.T_DUP, C.hx(0xD1), 1)[0] is first
    assert _link(env, C.T_DUP, C.hx(0xD2))[0] is first
    # same ids in two traces: links stay inside the trace
    for t in (C.T_TWIN_A, C.T_TWIN_B):
        for child in (C.hx(0xAB), "same-text-id", C.hx(0xAC)):
            p, k, _ = _link(env, t, child)
            assert p["trace_info"]["trace_id"] == t and k == 1
    # own parent: rejected; the syscall rule or nothing takes over
    p, k, d = _link(env, C.T_SELF, C.hx(0x5E1))
    assert (sid(p), k, d) == (C.hx(0x5E0), 2, 1)
    assert _link(env, C.T_SELF, C.hx(0x5E2)) == (None, 0, 0)
    # cycle: linked, but nothing reaches a root
    for s_, par in ((0xC1, 0xC2), (0xC2, 0xC1), (0xC3, 0xC1)):
        p, k, d = _link(env, C.T_CYCLE, C.hx(s_))
        assert (sid(p), k, d) == (C.hx(par), 1, -1)
    # dangling parents are roots
    assert _link(env, C.T_ORPHAN, "o-lost") == (None, 0, 0)
    assert _link(env, C.T_ORPHAN, C.hx(0x0F)) == (None, 0, 0)
    assert sid(_link(env, C.T_ORPHAN, "o-kid")[0]) == "o-root"
    # tcp rule and tap_side
    p, k, d = _link(env, C.T_TCP, C.hx(0x7C1))
    assert (sid(p), k, d) == (C.hx(0x7C0), 3, 1)
    for s_ in (0x7C0, 0x7C2, 0x7C3, 0x7C4):
        assert _link(env, C.T_TCP, C.hx(s_)) == (None, 0, 0)
    # priority
    assert [_link(env, C.T_PRIO, C.hx(s_))[1]
            for s_ in (0x9D, 0x9E, 0x9F)] == [1, 2, 3]
    assert sid(_link(env, C.T_PRIO, C.hx(0x9E))[0]) == C.hx(0x9B)
    assert sid(_link(env, C.T_PRIO, C.hx(0x9F))[0]) == C.hx(0x9C)
    # 16 non-hex characters hash on both sides
    assert sid(_link(env, C.T_ZZ, C.hx(0x22))[0]) == "zzzzzzzzzzzzzzzz"

    summ = {t["trace_id"]: t for t in env["tmap"]["traces"]}
    cyc = summ[C.T_CYCLE]
    assert (cyc["span_count"], cyc["root_count"], cyc["unrooted"],
            cyc["max_depth"]) == (3, 0, 3, 0)
    assert (cyc["root_service"], cyc["duration_us"]) == ("cart", 3000)
    assert summ[C.T_ORPHAN]["root_count"] == 3
    assert summ[C.T_SINGLE]["span_count"] == 1
    assert summ[C.T_CHAIN]["max_depth"] == 47
    assert summ[C.T_CHAIN]["error_count"] == 7
    assert summ[C.T_FAN]["error_count"] == 6
    assert summ[C.T_SYS]["max_depth"] == 2 and summ[C.T_SYS]["root_count"] == 2
    order = [(t["start_time"], t["trace_id"]) for t in env["tmap"]["traces"]]
    assert order == sorted(order)


def test_window_makes_the_child_a_root(env):
    m = env["mapper"]
    full = {t["trace_id"]: t for t in env["tmap"]["traces"]}[C.T_WINDOW]
    assert (full["span_count"], full["root_count"], full["max_depth"],
            full["root_service"]) == (3, 1, 2, "front")
    win = {t["trace_id"]: t
           for t in m.trace_map(time_start=C.WINDOW_LO)["traces"]}[C.T_WINDOW]
    assert (win["span_count"], win["root_count"], win["max_depth"],
            win["root_service"]) == (2, 1, 1, "cart")
    # both bounds inclusive: a window of one instant holds that span only
    t_one = C.T_SINGLE_START
    one = m.trace_map(time_start=t_one, time_end=t_one)
    assert [t["trace_id"] for t in one["traces"]] == [C.T_SINGLE]
    assert m.trace_map(time_end=C.T0 - 20_000 * C.MS)["trace_count"] == 0


def test_depth_bound_is_exact():
    """A chain of MAX_TRACE_HOPS + 2 rows: the deepest rooted row sits at
    exactly MAX_TRACE_HOPS, the one below it is unrooted."""
    from deepflow_amd.query import tracemap as TM
    n = MAX_TRACE_HOPS + 2

    class F:
        pass
    f = F()
    f.n = n
    f.tkey = np.full(n, 5, np.uint64)
    f.skey = np.arange(1, n + 1, dtype=np.uint64)
    f.pkey = np.arange(0, n, dtype=np.uint64)
    z = np.zeros(n, np.uint64)
    f.sreq, f.sresp = z, z
    f.tcp, f.tap = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    rows, parent, kind, depth = TM._host_link(f)
    assert parent.tolist() == [-1] + list(range(n - 1))
    assert depth[:-1].tolist() == list(range(MAX_TRACE_HOPS + 1))
    assert depth[-1] == -1


def test_build_trace_trees_upserts(env):
    tr = env["tracer"]
    tr.tree_rows.clear()
    # a row left by the per-trace path is replaced, not duplicated
    tr.assemble(C.T_CHAIN)
    assert len(tr.tree_rows) == 1
    for _ in range(2):
        info = tr.build_trace_trees()
        r = env["engine"].query(
            "SELECT trace_id, span_count, max_depth FROM trace_tree "
            "LIMIT 10000")
        got = sorted(map(tuple, r["values"]))
        want = sorted((t["trace_id"], t["span_count"], t["max_depth"])
                      for t in env["tmap"]["traces"])
        assert got == want
        assert info["rows"] == len(want) == info["traces"]
    assert (C.T_CHAIN, 48, 47) in got
    tr.tree_rows.clear()


def test_routes(env):
    client = TestClient(build_app(env["engine"], tracing=env["tracer"]))
    body = client.get("/v1/tracing/map").json()
    assert body == env["tmap"]
    win = client.get("/v1/tracing/map",
                     params={"time_start": C.WINDOW_LO}).json()
    assert win["span_count"] == env["tmap"]["span_count"] - 1
    built = client.post("/v1/tracing/trees/build").json()
    assert built["traces"] == env["tmap"]["trace_count"]
    # the parameterised route still serves real ids
    one = client.get(f"/v1/tracing/{C.T_PRIO}").json()
    assert one["span_count"] == 6 and one["trace_id"] == C.T_PRIO
    env["tracer"].tree_rows.clear()
