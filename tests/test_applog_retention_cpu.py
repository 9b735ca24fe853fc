"""Retention on the host application-log store, the oracle for the GPU
store's: evict_rows, evict_before, the row rule, and the HTTP surface."""
import copy
import os
import sys

import pytest
from fastapi.testclient import TestClient

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402
import applog_retention_cases as R  # noqa: E402

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402


@pytest.fixture(scope="module")
def parse_rows():
    return R.host_of(C.PARSE_CALLS).rows        # shared, never changed


@pytest.mark.parametrize("n, gone", [
    (0, 0), (1, 1), (R.N_PARSE - 1, R.N_PARSE - 1), (R.N_PARSE, R.N_PARSE),
    (R.N_PARSE + 5, R.N_PARSE), (-3, 0)])
def test_evict_rows_edge_values(parse_rows, n, gone):
    pipe = R.host_of(C.PARSE_CALLS)
    assert pipe.n_rows == R.N_PARSE
    assert pipe.evict_rows(n) == gone
    assert pipe.rows == parse_rows[gone:]
    assert pipe.n_rows == R.N_PARSE - gone
    assert pipe.evicted_rows == gone
    assert pipe.evictions == (1 if gone else 0)
    assert pipe.counter.snapshot().get("logs_evicted", 0) == gone
    # the interner is never shrunk
    assert len(pipe.app_interner) == len({r["app_service"]
                                          for r in parse_rows})


@pytest.mark.parametrize("t, gone", R.BEFORE_CASES)
def test_evict_before_non_monotone_times(t, gone):
    pipe = R.host_of(R.BEFORE_CALLS)
    assert [r["time"] for r in pipe.rows] == R.BEFORE_TIMES
    assert pipe.evict_before(t) == gone
    assert [r["time"] for r in pipe.rows] == R.BEFORE_TIMES[gone:]


def test_evict_before_leaves_older_rows_behind_the_cut():
    pipe = R.host_of(R.BEFORE_CALLS)
    assert pipe.evict_before(13) == 3
    # rows older than t after the first row that is not: they stay
    assert [r["time"] for r in pipe.rows if r["time"] < 13] == [5, 7]


def test_row_rule_against_a_list_model():
    pipe = AppLogPipeline(max_rows=R.MAX_ROWS, keep_fraction=R.KEEP)
    unbounded = AppLogPipeline()
    sizes, seen = [], []
    for call in R.ROW_RULE_CALLS:
        sizes += C.feed(pipe, [call])
        C.feed(unbounded, [call])
        want_n, want_gone = R.row_rule_model(sizes)[-1]
        seen.append((pipe.n_rows, pipe.evicted_rows))
        assert seen[-1] == (want_n, want_gone)
        # the survivors are the newest rows of the unbounded store
        assert pipe.rows == unbounded.rows[unbounded.n_rows - want_n:]
    assert 12 in sizes and max(sizes) > R.MAX_ROWS     # one oversized batch
    assert (8, 0) in seen                   # exactly at the limit: kept
    gone = [g for _, g in R.row_rule_model(sizes)]
    assert pipe.evictions == len(set(gone) - {0}) == 4


def test_keep_fraction_one_and_tiny():
    pipe = AppLogPipeline(max_rows=4, keep_fraction=1.0)
    C.feed(pipe, [R._batch(0, 6, 1)])
    assert pipe.n_rows == 4 and pipe.evicted_rows == 2
    pipe = AppLogPipeline(max_rows=4, keep_fraction=0.01)   # floor -> 0 -> 1
    C.feed(pipe, [R._batch(0, 6, 1)])
    assert pipe.n_rows == 1 and pipe.rows[0]["body"] == "batch 0 line 5"


def test_app_id_survives_the_eviction_of_all_its_rows():
    pipe = AppLogPipeline()
    pipe.ingest_lines(b"1 info gone-app a\n2 info other b", now=C.NOW)
    gone_id = pipe.rows[0]["app_id"]
    assert pipe.evict_rows(2) == 2 and pipe.rows == []
    pipe.ingest_lines(b"3 info new-app c\n4 info gone-app d", now=C.NOW)
    assert [r["app_id"] for r in pipe.rows] == [2, gone_id]


@pytest.mark.parametrize("first", R.PARSE_FIRSTS)
def test_queries_after_eviction_equal_a_fresh_store(parse_rows, first):
    pipe = R.host_of(C.PARSE_CALLS)
    pipe.evict_rows(first)
    fresh = AppLogPipeline()
    fresh.ingest_rows(copy.deepcopy(parse_rows[first:]))
    # a fresh store numbers its apps from 0: app_id must differ, so it is
    # left out; the rows were given their ids by the first store
    assert fresh.rows == parse_rows[first:]
    for kw in R.PARSE_QUERIES:
        assert pipe.search(limit=1000, **kw) == \
            fresh.search(limit=1000, **kw)
    assert pipe.histogram(*R.PARSE_HIST) == fresh.histogram(*R.PARSE_HIST)
    assert pipe.histogram(*R.PARSE_HIST, regex="o") == \
        fresh.histogram(*R.PARSE_HIST, regex="o")


def test_argument_validation():
    for kw in ({"keep_fraction": 0}, {"keep_fraction": 1.5},
               {"keep_fraction": -0.1}, {"max_rows": 0}, {"max_rows": -1}):
        with pytest.raises(ValueError):
            AppLogPipeline(**kw)
    # the host store knows no byte budget
    with pytest.raises(TypeError):
        AppLogPipeline(max_pool_bytes=1 << 20)
    with pytest.raises(ValueError):
        DeepflowServer(device="cpu", log_max_pool_bytes=1 << 20)
    with pytest.raises(ValueError):
        DeepflowServer(device="cpu", log_retain_s=0)
    # defaults: no limit, nothing evicted
    pipe = R.host_of(C.PARSE_CALLS)
    assert pipe.max_rows is None and pipe.evicted_rows == 0


def _frame(lines):
    return framing.encode_frame(
        framing.FrameHeader(msg_type=framing.MSG_APPLICATION_LOG,
                            agent_id=6), lines)


def test_stats_and_debug_store_over_http():
    srv = DeepflowServer(device="cpu", tcp_port=0, segment_rows=1 << 10,
                         dict_capacity=1 << 12, log_max_rows=4)
    client = TestClient(srv.app)
    before = client.get("/v1/debug/store").json()
    assert before["log_rows"] == 0 and before["log_evicted_rows"] == 0
    assert "log_pool_bytes" not in before           # host store
    assert {"l7_rows", "l7_evicted_rows", "l4_rows"} <= set(before)
    lines = b"\n".join(b"%d info app body %d" % (C.T0 + i, i)
                       for i in range(6))
    assert srv.receiver.handle_frame(_frame(lines))
    dbg = client.get("/v1/debug/store").json()
    assert dbg["log_rows"] == 2 and dbg["log_evicted_rows"] == 4
    stats = client.get("/v1/logs/stats").json()
    assert stats == {"rows": 2, "evicted_rows": 4, "evictions": 1,
                     "stored_bytes": len("body 4") + len("body 5"),
                     "max_rows": 4, "max_pool_bytes": None,
                     "keep_fraction": 0.5}
    assert [r["body"] for r in client.get("/v1/logs/search").json()] == \
        ["body 5", "body 4"]


def test_log_retain_s_evicts_from_the_ingest_handler(monkeypatch):
    import time as real_time
    srv = DeepflowServer(device="cpu", tcp_port=0, segment_rows=1 << 10,
                         dict_capacity=1 << 12, log_retain_s=100)
    clock = [2_000_000_000.0]
    monkeypatch.setattr(real_time, "time", lambda: clock[0])
    now = int(clock[0])
    old = b"%d info app old row\n%d info app kept row" % (now - 500, now - 5)
    assert srv.receiver.handle_frame(_frame(old))
    assert [r["body"] for r in srv.applogs.rows] == ["kept row"]
    # within the same second nothing is checked again
    assert srv.receiver.handle_frame(_frame(b"%d info app late old row"
                                            % (now - 900)))
    assert srv.applogs.n_rows == 2
    clock[0] += 1.5
    assert srv.receiver.handle_frame(_frame(b"%d info app fresh" % now))
    # the prefix rule: "kept row" stops the cut, the old row behind it stays
    assert [r["body"] for r in srv.applogs.rows] == \
        ["kept row", "late old row", "fresh"]
    assert srv.applogs.evicted_rows == 1
