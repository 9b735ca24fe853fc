"""Flow groups (query/flowgroups.py host twin) against an independent
brute-force component search over the span dicts and against hand-written
expectations, on a span set that spans several 256-row segments. The
global row of a span is its payload index, so every comparison is exact.
"""
import os
import re
import sys
from pathlib import Path

import numpy as np
import pytest
from fastapi.testclient import TestClient

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgroup_cases as C  # noqa: E402
import tracemap_cases as TC  # noqa: E402

from deepflow_amd.ingest import L7IngestPipeline  # noqa: E402
from deepflow_amd.query import QueryEngine  # noqa: E402
from deepflow_amd.query import flowgroups as FG  # noqa: E402
from deepflow_amd.query.http_api import build_app  # noqa: E402
from deepflow_amd.query.tracemap import TraceMapper  # noqa: E402
from deepflow_amd.query.tracing import DistributedTracer  # noqa: E402
from deepflow_amd.store import l7_schema as S  # noqa: E402

SYS, TCP, XREQ, TRACE = (1 << FG.REL_SYSCALL, 1 << FG.REL_TCP,
                         1 << FG.REL_XREQ, 1 << FG.REL_TRACE)
SPACE_BIT = {"trace": TRACE, "syscall": SYS, "tcp": TCP, "xreq": XREQ}


def _engine(spans):
    pipe = L7IngestPipeline(device="cpu", segment_rows=1 << 8,
                            dict_capacity=1 << 12)
    for payload in C.payloads_of(spans):
        pipe.ingest_frame_payload(payload)
    return QueryEngine(pipe, device="cpu")


@pytest.fixture(scope="module")
def env():
    spans = C.build_spans()
    engine = _engine(spans)
    grouper = FG.FlowGrouper(engine)
    return dict(spans=spans, engine=engine, grouper=grouper,
                tracer=DistributedTracer(engine),
                links=grouper.link_groups(),
                groups=grouper.flow_groups(min_spans=1))


def brute_force(spans, lo=None, hi=None):
    """-> {row: (group, via)} for the rows in the window: a breadth-first
    search over "emits an equal key in the same space", nothing shared
    with the module under test."""
    rows = [g for g, s in enumerate(spans)
            if (lo is None or s["base"]["start_time"] >= lo) and
            (hi is None or s["base"]["start_time"] <= hi)]
    by_key = {}
    for g in rows:
        for k in C.keys_of(spans[g]):
            by_key.setdefault(k, []).append(g)
    group = {}
    for g in rows:
        if g in group:
            continue
        seen, todo = {g}, [g]
        while todo:
            cur = todo.pop()
            for k in C.keys_of(spans[cur]):
                for other in by_key[k]:
                    if other not in seen:
                        seen.add(other)
                        todo.append(other)
        for m in seen:
            group[m] = min(seen)
    out = {}
    for g in rows:
        via = 0
        for k in C.keys_of(spans[g]):
            if by_key[k][0] != g:           # ascending: [0] is the first row
                via |= SPACE_BIT[k[0]]
        out[g] = (group[g], via)
    return out


def _members(env, tag):
    """Tags of the spans grouped with `tag`, and the group row."""
    links, spans = env["links"], env["spans"]
    at = {int(r): i for i, r in enumerate(links["row"])}
    grp = int(links["group"][at[C.row_of(spans, tag)]])
    rows = links["row"][links["group"] == grp]
    return {spans[g]["trace_info"]["span_id"] for g in rows.tolist()}, grp


def _via(env, tag):
    links = env["links"]
    at = {int(r): i for i, r in enumerate(links["row"])}
    return int(links["via"][at[C.row_of(env["spans"], tag)]])


def _summary(env, tag):
    grp = _members(env, tag)[1]
    return {g["group_row"]: g for g in env["groups"]["groups"]}[grp]


def test_shape_of_the_set(env):
    spans, links = env["spans"], env["links"]
    assert 1400 <= len(spans) <= 1700 and len(spans) % 64
    assert len(env["engine"].pipe.segments.segments) >= 5
    # every row takes part, trace id or not
    assert links["row"].tolist() == list(range(len(spans)))
    assert sum(1 for s in spans if not s["trace_info"]["trace_id"]) > 600
    assert links["drops"] == 0 and env["groups"]["drops"] == 0
    assert links["row"].dtype == np.int64 and \
        links["group"].dtype == np.int64 and links["via"].dtype == np.uint8
    assert env["groups"]["span_count"] == len(spans)
    assert np.all(links["group"] <= links["row"])
    # groups interleave and cross segments
    _, grp = _members(env, "chain-0")
    rows = links["row"][links["group"] == grp]
    assert rows.max() - rows.min() > 3 * 256


@pytest.mark.parametrize("window", [
    {}, dict(lo=C.WINDOW_LO), dict(lo=C.T0 + 20 * C.MS, hi=C.T0 + 400 * C.MS)])
def test_host_twin_equals_brute_force(env, window):
    want = brute_force(env["spans"], **window)
    got = env["grouper"].link_groups(window.get("lo"), window.get("hi"))
    assert got["row"].tolist() == sorted(want)
    assert got["group"].tolist() == [want[g][0] for g in sorted(want)]
    assert got["via"].tolist() == [want[g][1] for g in sorted(want)]
    assert len(set(got["group"].tolist())) > 40


def test_summaries_equal_brute_force(env):
    spans = env["spans"]
    want = {}
    for g, (grp, via) in brute_force(spans).items():
        w = want.setdefault(grp, dict(
            group_row=grp, span_count=0, traced_spans=0, error_count=0,
            start_time=1 << 64, end_time=0, via_trace=0, via_syscall=0,
            via_tcp=0, via_xreq=0, trace_id=None))
        s = spans[g]
        w["span_count"] += 1
        if s["trace_info"]["trace_id"]:
            w["traced_spans"] += 1
            if w["trace_id"] is None:       # rows ascend: the first traced
                w["trace_id"] = s["trace_info"]["trace_id"]
        w["error_count"] += s["resp"]["status"] in (3, 4)
        w["start_time"] = min(w["start_time"], s["base"]["start_time"])
        w["end_time"] = max(w["end_time"], s["base"]["end_time"])
        for name, bit in SPACE_BIT.items():
            w["via_" + name] += bool(via & bit)
    for w in want.values():
        w["trace_id"] = w["trace_id"] or ""
    want = sorted(want.values(),
                  key=lambda w: (w["start_time"], w["group_row"]))
    assert env["groups"]["groups"] == want
    assert env["groups"]["group_count"] == len(want)
    # the default drops groups of one span
    two = env["grouper"].flow_groups()
    assert two["groups"] == [w for w in want if w["span_count"] >= 2]
    assert two["span_count"] == sum(w["span_count"] for w in want
                                    if w["span_count"] >= 2)
    assert 0 < two["group_count"] < len(want)


def test_hand_written_cases(env):
    # pure syscall chain: request = request, request = response
    tags, _ = _members(env, "sys-a")
    assert tags == {"sys-a", "sys-b", "sys-c", "sys-d"}
    assert [_via(env, t) for t in ("sys-a", "sys-b", "sys-c", "sys-d")] == \
        [0, SYS, SYS, SYS]
    s = _summary(env, "sys-a")
    assert (s["span_count"], s["traced_spans"], s["error_count"],
            s["via_syscall"], s["trace_id"]) == (4, 0, 1, 3, "")
    assert s["group_row"] == C.row_of(env["spans"], "sys-a")
    assert (s["start_time"], s["end_time"]) == (C.T0 + 1 * C.MS,
                                                C.T0 + 9 * C.MS)
    # two traces bridged by one span without a trace id
    tags, _ = _members(env, "br-ebpf")
    assert tags == {"br-a1", "br-a2", "br-ebpf", "br-b1", "br-b2"}
    s = _summary(env, "br-ebpf")
    assert (s["span_count"], s["traced_spans"], s["error_count"]) == (5, 4, 1)
    assert (s["via_trace"], s["via_syscall"], s["via_tcp"],
            s["via_xreq"]) == (2, 2, 0, 0)
    assert s["trace_id"] == C.T_BRIDGE_A
    assert _via(env, "br-b1") == SYS and _via(env, "br-b2") == TRACE
    # a trace on its own
    tags, _ = _members(env, "plain-2")
    assert tags == {f"plain-{i}" for i in range(4)}
    assert _summary(env, "plain-0")["trace_id"] == C.T_PLAIN
    assert _summary(env, "plain-0")["via_trace"] == 3
    # x-request-id: out -> in, and the same text twice
    assert _members(env, "xhop-gw")[0] == {"xhop-gw", "xhop-next"}
    assert (_via(env, "xhop-gw"), _via(env, "xhop-next")) == (0, XREQ)
    assert _members(env, "xsame-2")[0] == {"xsame-1", "xsame-2"}
    assert _summary(env, "xsame-1")["via_xreq"] == 1
    # tcp pair
    assert _members(env, "tcp-tap1")[0] == {"tcp-tap1", "tcp-tap2"}
    assert _via(env, "tcp-tap2") == TCP
    for t in ("tcp-other-resp", "tcp-zero-req-1", "tcp-zero-req-2"):
        assert _members(env, t)[0] == {t} and _via(env, t) == 0
    # one value in two key spaces
    assert _members(env, "cross-sys")[0] == {"cross-sys"}
    assert _members(env, "cross-tcp")[0] == {"cross-tcp"}
    # chain and star
    tags, grp = _members(env, "chain-117")
    assert tags == {f"chain-{i}" for i in range(C.CHAIN_LEN)}
    assert grp == C.row_of(env["spans"], "chain-0")
    s = _summary(env, "chain-0")
    assert (s["span_count"], s["via_syscall"], s["error_count"]) == \
        (C.CHAIN_LEN, C.CHAIN_LEN - 1, 5)
    tags, grp = _members(env, "star-200")
    assert tags == {f"star-{i}" for i in range(C.STAR_LEN)}
    assert grp == C.row_of(env["spans"], "star-0")
    assert _summary(env, "star-0")["via_xreq"] == C.STAR_LEN - 1
    # singletons
    for t in ("single-bare", "single-keys", "single-instant"):
        assert _members(env, t) == ({t}, C.row_of(env["spans"], t))
        assert _via(env, t) == 0
    assert _summary(env, "single-keys")["traced_spans"] == 1
    # the window case, unwindowed: one group through `win-out`
    assert _members(env, "win-lone")[0] == \
        {"win-out", "win-in-1", "win-in-2", "win-lone"}
    assert _summary(env, "win-out")["trace_id"] == C.T_WINDOW
    order = [(g["start_time"], g["group_row"])
             for g in env["groups"]["groups"]]
    assert order == sorted(order)


def test_window_variants(env):
    gr, spans = env["grouper"], env["spans"]
    win = gr.link_groups(time_start=C.WINDOW_LO)
    assert C.row_of(spans, "win-out") not in win["row"].tolist()
    assert len(win["row"]) == len(spans) - 1
    at = {int(r): i for i, r in enumerate(win["row"])}
    # the partner outside the window no longer ties the three together
    for t in ("win-in-1", "win-in-2", "win-lone"):
        g = C.row_of(spans, t)
        assert int(win["group"][at[g]]) == g and int(win["via"][at[g]]) == 0
    # both bounds inclusive: a window of one instant holds that span only
    one = gr.flow_groups(C.SINGLE_START, C.SINGLE_START, min_spans=1)
    assert [g["group_row"] for g in one["groups"]] == \
        [C.row_of(spans, "single-instant")]
    assert gr.flow_groups(time_end=C.T0 - 20_000 * C.MS, min_spans=1) == \
        {"groups": [], "group_count": 0, "span_count": 0, "drops": 0}
    assert len(gr.link_groups(time_end=C.T0 - 20_000 * C.MS)["row"]) == 0


def test_refines_k10_trace_partition():
    """On the K10 case set, over the rows that have a trace id: every
    trace lies inside one group, and every group holds one trace, except
    that T_SYS and T_TCP share a group. The 25 rows without a trace id
    carry syscall id 777 (T_SYS) and the tcp pair (5000, 0) (T_TCP); no
    other key of that set crosses traces."""
    spans = TC.build_spans()
    engine = _engine(spans)
    k10 = TraceMapper(engine).link_spans()
    links = FG.FlowGrouper(engine).link_groups()
    assert links["row"].tolist() == list(range(len(spans)))
    group = links["group"][k10["row"]]              # traced rows only
    traces_of, groups_of = {}, {}
    for g, k in zip(group.tolist(), k10["trace_key"].tolist()):
        traces_of.setdefault(g, set()).add(k)
        groups_of.setdefault(k, set()).add(g)
    assert all(len(v) == 1 for v in groups_of.values())
    merged = [v for v in traces_of.values() if len(v) > 1]
    assert merged == [{FG.trace_key_of(TC.T_SYS), FG.trace_key_of(TC.T_TCP)}]
    assert len(traces_of) == len(groups_of) - 1
    # the rows without a trace id sit in that group too
    untraced = [g for g, s in enumerate(spans)
                if not s["trace_info"]["trace_id"]]
    assert len(untraced) == 25
    shared = next(g for g, v in traces_of.items() if len(v) > 1)
    assert set(links["group"][untraced].tolist()) == {shared}


def test_flow_trace_seeds(env):
    tr, spans = env["tracer"], env["spans"]
    sid = lambda r: [s["span_id"] for s in r["spans"]]
    r = tr.flow_trace(trace_id=C.T_BRIDGE_B)
    assert sid(r) == ["br-a1", "br-a2", "br-ebpf", "br-b1", "br-b2"]
    assert (r["group_row"], r["span_count"], r["truncated"]) == \
        (C.row_of(spans, "br-a1"), 5, False)
    assert list(r["spans"][0]) == list(FG.SPAN_COLS)
    b1 = r["spans"][3]
    assert (b1["trace_id"], b1["syscall_trace_id_request"],
            b1["service_name"], b1["start_time"]) == \
        (C.T_BRIDGE_B, 202, "pay", C.T0 + 8 * C.MS)
    assert tr.flow_trace(trace_id=C.T_BRIDGE_A) == r
    # a syscall id matches the request or the response column
    r = tr.flow_trace(syscall_trace_id=102)
    assert sid(r) == ["sys-a", "sys-b", "sys-c", "sys-d"]
    assert sid(tr.flow_trace(syscall_trace_id=202)) == \
        ["br-a1", "br-a2", "br-ebpf", "br-b1", "br-b2"]
    r = tr.flow_trace(x_request_id=C.X_HOP)
    assert sid(r) == ["xhop-gw", "xhop-next"]
    assert (r["spans"][0]["x_request_id_1"],
            r["spans"][1]["x_request_id_0"]) == (C.X_HOP, C.X_HOP)
    # tcp values are no syscall ids
    assert sid(tr.flow_trace(syscall_trace_id=5000)) == ["cross-sys"]
    # the window applies to the seed and to the group
    assert tr.flow_trace(C.WINDOW_LO, trace_id=C.T_WINDOW)["span_count"] == 1
    assert tr.flow_trace(trace_id=C.T_WINDOW)["span_count"] == 4


def test_flow_trace_errors_and_limit(env):
    tr = env["tracer"]
    with pytest.raises(ValueError):
        tr.flow_trace(trace_id=C.T_PLAIN, syscall_trace_id=101)
    with pytest.raises(ValueError):
        tr.flow_trace()
    empty = {"group_row": None, "span_count": 0, "truncated": False,
             "spans": []}
    assert tr.flow_trace(trace_id="no-such-trace") == empty
    assert tr.flow_trace(syscall_trace_id=987654321) == empty
    assert tr.flow_trace(x_request_id="nobody") == empty
    assert tr.flow_trace(C.T0 + 10_000 * C.MS, x_request_id=C.X_HOP) == empty
    r = tr.flow_trace(x_request_id="star-request-id", limit=3)
    assert (r["span_count"], r["truncated"]) == (C.STAR_LEN, True)
    assert [s["span_id"] for s in r["spans"]] == \
        ["star-0", "star-1", "star-2"]
    assert not tr.flow_trace(x_request_id="star-request-id")["truncated"]


def test_routes(env):
    client = TestClient(build_app(env["engine"], tracing=env["tracer"]))
    body = client.get("/v1/tracing/groups", params={"min_spans": 1}).json()
    assert body == env["groups"]
    assert client.get("/v1/tracing/groups").json() == \
        env["grouper"].flow_groups()
    win = client.get("/v1/tracing/groups",
                     params={"time_start": C.WINDOW_LO, "min_spans": 1})
    assert win.json()["span_count"] == len(env["spans"]) - 1
    # /flow is its own route, not a trace id of the parameterised one
    flow = client.get("/v1/tracing/flow",
                      params={"syscall_trace_id": 102}).json()
    assert flow == env["tracer"].flow_trace(syscall_trace_id=102)
    assert "roots" not in flow and flow["span_count"] == 4
    flow = client.get("/v1/tracing/flow",
                      params={"x_request_id": C.X_SAME, "limit": 1}).json()
    assert (flow["span_count"], flow["truncated"], len(flow["spans"])) == \
        (2, True, 1)
    assert client.get("/v1/tracing/flow").status_code == 400
    assert client.get("/v1/tracing/flow", params={
        "trace_id": C.T_PLAIN, "x_request_id": C.X_HOP}).status_code == 400
    # the parameterised route still serves real ids
    one = client.get(f"/v1/tracing/{C.T_PLAIN}").json()
    assert one["span_count"] == 4 and one["trace_id"] == C.T_PLAIN
    env["tracer"].tree_rows.clear()


def test_pool_positions_match_header():
    hdr = (Path(FG.__file__).resolve().parent.parent / "ops" / "csrc" /
           "l7_layout.h").read_text()
    defs = dict(re.findall(r"#define L7_POOL_(\w+) (\d+)", hdr))
    assert int(defs["X_REQUEST_ID_0"]) == S.POOL_POS["x_request_id_0"]
    assert int(defs["X_REQUEST_ID_1"]) == S.POOL_POS["x_request_id_1"]
    assert int(defs["TRACE_ID"]) == S.POOL_POS["trace_id"]
