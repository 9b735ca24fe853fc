"""GPU application-log store (K11, ops/csrc/dflog.hip) against the host
AppLogPipeline fed the same calls with the same `now` (-m gpu). Every
comparison is exact."""
import os
import sys
import types

import pytest
import torch
from fastapi.testclient import TestClient

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402

from deepflow_amd.ingest import applog_pipeline  # noqa: E402
from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.ops import native  # noqa: E402
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402


def gpu_of(calls, **kw):
    assert torch.cuda.is_available()
    pipe = AppLogPipeline(device="cuda", **kw)
    counts = C.feed(pipe, calls)
    return pipe, counts


def same_search(host, gpu, substr="", **kw):
    kw.setdefault("limit", 1000)
    want = host.search(substr, **kw)
    got = gpu.search(substr, **kw)
    assert got == want
    return got


# ------------------------------------------------------------------ parse
@pytest.fixture(scope="module")
def parse_host():
    return C.host_of(C.PARSE_CALLS)


def test_parse_rows_equal(parse_host):
    gpu, counts = gpu_of(C.PARSE_CALLS)
    assert counts == C.feed(AppLogPipeline(), C.PARSE_CALLS)
    assert gpu.n_rows == parse_host.n_rows == len(parse_host.rows)
    rows = gpu.rows
    want_rows = C.as_gpu(parse_host.rows)
    assert want_rows != parse_host.rows
    for got, want in zip(rows, want_rows):
        assert got == want
    assert len(rows) == len(want_rows)
    assert gpu.store.app_drops == 0
    # the cases the kernel must tell apart, by what the host made of them
    by_body = {r["body"]: r for r in rows}
    assert by_body["only two spaces"]["time"] == C.NOW
    assert by_body["app double space"]["app_service"] == "warn"
    assert by_body["body after an empty app"]["app_service"] == ""
    assert by_body["eighteen digits"]["time"] == 123456789012345678
    assert by_body[C.NINETEEN]["time"] == C.NOW
    assert by_body["1700000203 info app"]["severity"] == 6
    assert by_body[""]["trace_id"] == ""            # OTLP row, empty body
    assert by_body["otlp body one"]["attr.k"] == "v"
    assert [by_body["word %d" % i]["severity"] for i in range(8)] == \
        [7, 6, 4, 4, 3, 2, 2, 6]
    # search hydrates the same dicts, extras included
    assert gpu.search() == C.as_gpu(parse_host.search())
    assert len(same_search(parse_host, gpu, "otlp body")) == 2
    # a needle longer than every body
    same_search(parse_host, gpu, "x" * 100)


def test_growth_reallocates_rows_and_pool(parse_host):
    gpu, _ = gpu_of(C.PARSE_CALLS, row_capacity=4, pool_capacity=64)
    assert gpu.store.row_capacity > 4 and gpu.store.pool.numel() > 64
    assert gpu.store.pool.numel() % 16 == 0
    assert gpu.rows == C.as_gpu(parse_host.rows)
    same_search(parse_host, gpu, "ot")


def test_app_ids_are_home_slots():
    """An app id is the slot the probe starts at, `hash & (cap - 1)`, when
    that slot is free. cap = 4 is the smallest power of two with room for
    three distinct home slots."""
    from deepflow_amd.store.dictionary import str_hash_py
    seed, cap = int(native.gpu().df_log_app_seed()), 4
    apps, homes = [], []
    for i in range(64):
        a = b"app%d" % i
        home = str_hash_py(a, seed) & (cap - 1)
        if home not in homes:
            apps.append(a)
            homes.append(home)
        if len(apps) == 3:
            break
    assert len(set(homes)) == len(apps) == 3
    data = b"\n".join(b"%d info %s body" % (i + 1, a)
                      for i, a in enumerate(apps))
    gpu, _ = gpu_of([("lines", data, 0, "s")], app_capacity=cap)
    assert gpu.store.app_drops == 0
    assert gpu.store.row_app[:3].tolist() == homes
    assert [r["app_service"] for r in gpu.rows] == [a.decode() for a in apps]


def test_full_app_table_counts_drops():
    calls = [
        ("lines", b"1 info a1 one\n2 info a2 two\n3 info a1 three", 0, "s"),
        ("lines", b"4 info a3 four\n5 info a2 five\n6 info a4 six\n"
                  b"7 info a5 seven", 0, "s"),
    ]
    host = C.host_of(calls)
    gpu, _ = gpu_of(calls, app_capacity=2)
    assert gpu.store.app_drops == 3
    rows = gpu.rows
    assert len(rows) == 7
    for got, want in zip(rows, host.rows):
        if want["app_service"] in ("a1", "a2"):
            assert got == want
        else:
            assert got == dict(want, app_service="", app_id=-1)
    same_search(host, gpu, app_service="a2")
    assert gpu.search(app_service="a3") == []


# ------------------------------------------------------------------- scan
@pytest.fixture(scope="module")
def scan_pair():
    host = C.host_of(C.SCAN_CALLS)      # computed once, shared, unchanged
    gpu, _ = gpu_of(C.SCAN_CALLS)
    assert gpu.rows == host.rows
    return host, gpu


@pytest.mark.parametrize("k", range(len(C.SCAN_QUERIES)))
def test_scan(scan_pair, k):
    host, gpu = scan_pair
    substr, ci = C.SCAN_QUERIES[k]
    same_search(host, gpu, substr, case_insensitive=ci)


def test_scan_hit_counts(scan_pair):
    # the oracle itself: these cases only mean something with these counts
    host, _ = scan_pair
    n = [len(host.search(q, limit=1000, case_insensitive=ci))
         for q, ci in C.SCAN_QUERIES]
    assert n == [1, 1, 1, 5, 1, 0, 0, 0, 1, 1, 2, 2, 1, 1, 2,
                 len(host.rows), 1, 0]


def test_needle_limits(scan_pair):
    _, gpu = scan_pair
    with pytest.raises(ValueError):
        gpu.search("x" * 129)
    with pytest.raises(ValueError):
        gpu.search(["x"] * 9)


def test_scan_across_tile_edges():
    tile = int(native.gpu().df_log_tile_bytes())
    payload, starts = C.tile_payload(tile)
    assert starts[0] + len(C.EDGE_NEEDLE) > tile > starts[0]
    assert starts[1] % tile == 0 and len(payload) > 2 * tile
    calls = [("lines", payload, 3, "system")]
    host = C.host_of(calls)
    gpu, _ = gpu_of(calls)
    # alone in its query the straddling needle is the longest one, so its
    # hit starts exactly maxlen-1 bytes before the edge
    hit = same_search(host, gpu, [C.EDGE_NEEDLE])
    assert len(hit) == 1
    assert len(same_search(host, gpu, [C.ON_EDGE_NEEDLE])) == 1
    assert same_search(host, gpu, [C.EDGE_NEEDLE, C.ON_EDGE_NEEDLE]) == []
    assert len(same_search(host, gpu, ["E-STRADDLE", "."])) == 1
    # dense needle: (nearly) every row of every tile
    assert len(same_search(host, gpu, ".", limit=10000)) == host.n_rows
    same_search(host, gpu, ".", limit=7, app_service="tile1")
    assert gpu.histogram(3, C.T0, C.T0 + 7, "..") == \
        host.histogram(3, C.T0, C.T0 + 7, "..")


def test_empty_store():
    gpu = AppLogPipeline(device="cuda")
    assert gpu.search() == [] and gpu.search("x") == []
    assert gpu.histogram(1, 0, 10) == [] and gpu.rows == []
    assert gpu.ingest_lines(b"\n \r\n", now=C.NOW) == 0
    assert gpu.ingest_rows([]) == 0 and gpu.n_rows == 0


# ----------------------------------------------------------------- select
@pytest.mark.parametrize("k", range(len(C.SELECT_FILTERS)))
def test_select_filters(scan_pair, k):
    host, gpu = scan_pair
    kw = dict(C.SELECT_FILTERS[k])
    same_search(host, gpu, kw.pop("substr", ""), **kw)


def test_select_window_is_inclusive(scan_pair):
    host, gpu = scan_pair
    got = same_search(host, gpu, time_start=C.T0 + 3, time_end=C.T0 + 7)
    assert {r["time"] for r in got} >= {C.T0 + 3, C.T0 + 7}
    assert same_search(host, gpu, app_service="never-ingested") == []


def test_limit_and_order(scan_pair):
    host, gpu = scan_pair
    hits = len(host.search("e", limit=1000))
    assert hits > 3
    for limit in (0, 1, hits - 1, hits, hits + 1):
        got = same_search(host, gpu, "e", limit=limit)
        assert len(got) == min(limit, hits)
    assert same_search(host, gpu) == list(reversed(host.rows))


# -------------------------------------------------------------- histogram
def test_histogram_lds_and_global_paths(scan_pair):
    host, gpu = scan_pair
    lds_buckets = int(native.gpu().df_log_hist_lds_buckets())
    assert 4 <= lds_buckets < 4096
    # 4 buckets: pre-aggregated in LDS; rows sit on T0 and on T0+7
    want = host.histogram(2, C.T0, C.T0 + 7)
    assert gpu.histogram(2, C.T0, C.T0 + 7) == want
    assert {C.T0, C.T0 + 6} <= {d["time"] for d in want}
    # 4096 buckets: straight to global atomics
    assert gpu.histogram(1, C.T0, C.T0 + 4095) == \
        host.histogram(1, C.T0, C.T0 + 4095)
    # rows exactly on time_start and on time_end
    want = host.histogram(1, C.T0 + 3, C.T0 + 7)
    assert gpu.histogram(1, C.T0 + 3, C.T0 + 7) == want
    assert {C.T0 + 3, C.T0 + 7} <= {d["time"] for d in want}
    # with every filter
    kw = dict(severity_max=4, app_service="beta", case_insensitive=True)
    assert gpu.histogram(4, C.T0, C.T0 + 7, ["E", "t"], **kw) == \
        host.histogram(4, C.T0, C.T0 + 7, ["E", "t"], **kw) != []
    assert gpu.histogram(1, C.T0 + 5, C.T0 + 4) == []
    with pytest.raises(ValueError):
        gpu.histogram(0, C.T0, C.T0 + 7)
    with pytest.raises(ValueError):
        gpu.histogram(1, C.T0, C.T0 + 4096)


# ----------------------------------------------------------------- server
def test_server_gpu_logs(monkeypatch):
    # one wall clock for the free-form line on both servers
    monkeypatch.setattr(applog_pipeline, "time",
                        types.SimpleNamespace(time=lambda: C.NOW))
    lines = b"\n".join([
        b"1700000100 ERROR checkout failed to connect to db",
        b"1700000101 info checkout request ok",
        b"free form line",
    ])
    frame = framing.encode_frame(
        framing.FrameHeader(msg_type=framing.MSG_APPLICATION_LOG,
                            agent_id=6), lines)
    out = {}
    for dev in ("cpu", "cuda"):
        srv = DeepflowServer(device=dev, tcp_port=0, segment_rows=1 << 10,
                             dict_capacity=1 << 12, gpu_logs=True)
        assert srv.applogs.gpu == (dev == "cuda")
        assert srv.receiver.handle_frame(frame)
        client = TestClient(srv.app)
        out[dev] = (
            srv.engine.query(
                "SELECT severity, Count(*) AS c FROM application_log "
                "GROUP BY severity"),
            srv.applogs.search(severity_max=3),
            client.get("/v1/logs/search", params={
                "q": ["CONNECT", "db"], "case_insensitive": "true"}).json(),
            client.get("/v1/logs/search").json(),
            client.get("/v1/logs/histogram", params={
                "interval": 60, "time_start": 1700000100,
                "time_end": C.NOW}).json(),
        )
    assert out["cuda"] == out["cpu"]
    sql, errs, hits, everything, hist = out["cuda"]
    assert sum(v[1] for v in sql["values"]) == 3
    assert len(errs) == 1 and len(hits) == 1 and len(everything) == 3
    assert sum(d["count"] for d in hist) == 3
