"""Regex search on the GPU application-log store (K13, k_log_regex in
ops/csrc/dflog.hip) against the host AppLogPipeline fed the same calls
(-m gpu). Every comparison is exact; the host matches with Python's `re`."""
import os
import sys
import types

import pytest
import torch
from fastapi.testclient import TestClient

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402
import applog_regex_cases as R  # noqa: E402

from deepflow_amd.ingest import applog_pipeline  # noqa: E402
from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.ops import gpu_ops, native  # noqa: E402
from deepflow_amd.query import logregex  # noqa: E402
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402


def gpu_of(calls, **kw):
    assert torch.cuda.is_available()
    pipe = AppLogPipeline(device="cuda", **kw)
    C.feed(pipe, calls)
    return pipe


def same_search(host, gpu, regex, substr="", **kw):
    kw.setdefault("limit", 1000)
    want = host.search(substr, regex=regex, **kw)
    got = gpu.search(substr, regex=regex, **kw)
    assert got == want
    return got


# ------------------------------------------------------- SCAN_CALLS corpus
@pytest.fixture(scope="module")
def scan_pair():
    host = C.host_of(C.SCAN_CALLS)      # computed once, shared, unchanged
    gpu = gpu_of(C.SCAN_CALLS)
    assert gpu.rows == host.rows
    return host, gpu


@pytest.mark.parametrize("k", range(len(R.SCAN_REGEX)))
def test_scan_regex(scan_pair, k):
    host, gpu = scan_pair
    pat, ci, hits = R.SCAN_REGEX[k]
    got = same_search(host, gpu, pat, case_insensitive=ci)
    # the oracle itself: the case only means something with this count
    assert len(got) == hits
    assert got == R.re_rows(host.rows, pat, ci)


@pytest.mark.parametrize("k", range(len(R.SCAN_COMBINED)))
def test_scan_regex_with_needles_and_filters(scan_pair, k):
    host, gpu = scan_pair
    pat, kw = R.SCAN_COMBINED[k]
    kw = dict(kw)
    same_search(host, gpu, pat, kw.pop("substr", ""), **kw)


def test_combined_cases_mean_something(scan_pair):
    host, _ = scan_pair
    n = []
    for pat, kw in R.SCAN_COMBINED:
        kw = dict(kw)
        kw.setdefault("limit", 1000)
        n.append(len(host.search(kw.pop("substr", ""), regex=pat, **kw)))
    assert n == [1, 2, 1, 1, 4, 11, 6, 9, 2, 1, 0, 3, 0, 2, 0, 1, 1]


def test_histogram_with_regex(scan_pair):
    host, gpu = scan_pair
    for pat, ci in ((r"t[eh]", False), (r"NEEDLE|POOL", True),
                    (r"^$", False), (r".*", False), (r"tail$", False)):
        want = host.histogram(2, C.T0, C.T0 + 7, regex=pat,
                              case_insensitive=ci)
        assert gpu.histogram(2, C.T0, C.T0 + 7, regex=pat,
                             case_insensitive=ci) == want
    kw = dict(severity_max=4, app_service="beta", case_insensitive=True)
    assert gpu.histogram(4, C.T0, C.T0 + 7, ["E", "t"], regex="T.*N", **kw) \
        == host.histogram(4, C.T0, C.T0 + 7, ["E", "t"], regex="T.*N",
                          **kw) != []


def test_empty_and_none_constrain_nothing(scan_pair):
    host, gpu = scan_pair
    for rx in ("", None):
        assert same_search(host, gpu, rx) == gpu.search(limit=1000)
        assert same_search(host, gpu, rx, "e") == gpu.search("e", limit=1000)


# ------------------------------------------------------ PARSE_CALLS corpus
@pytest.fixture(scope="module")
def parse_pair():
    host = C.host_of(C.PARSE_CALLS)
    # the one parse divergence of these cases changes a body: compare with
    # a host store that holds what the GPU store holds
    twin = AppLogPipeline()
    twin.rows = C.as_gpu(host.rows)
    gpu = gpu_of(C.PARSE_CALLS)
    assert gpu.rows == twin.rows
    return twin, gpu


@pytest.mark.parametrize("k", range(len(R.PARSE_REGEX)))
def test_parse_regex(parse_pair, k):
    host, gpu = parse_pair
    pat, ci = R.PARSE_REGEX[k]
    same_search(host, gpu, pat, case_insensitive=ci)


def test_empty_bodies_and_the_body_off_tie(parse_pair):
    host, gpu = parse_pair
    # the tie itself: an empty body, then a row whose body starts there
    boff = gpu.store.row_boff[:gpu.n_rows].tolist()
    blen = gpu.store.row_blen[:gpu.n_rows].tolist()
    empty = blen.index(0)
    assert boff[empty] == boff[empty + 1] and blen[empty + 1] > 0
    for pat in (r"^$", r"^\Z", r"^a*$"):
        got = same_search(host, gpu, pat)
        assert [r["body"] for r in got] == [""]
        assert got[0]["time"] == C.T0 + 401
    # nullable and not anchored at both ends: every row
    for pat in (r".*", r"a*", r"^", r"$", r"x?$", r"^a*"):
        assert len(same_search(host, gpu, pat)) == host.n_rows
    # the row after the tie gets its own matches, the empty row none
    for pat in (r"^no app", r"^no app, otlp body two$", r"two$", r"^n"):
        got = same_search(host, gpu, pat)
        assert [r["time"] for r in got] == [C.T0 + 402]
    assert [r["body"] for r in same_search(host, gpu, r"^.")] == \
        [r["body"] for r in reversed(host.rows) if r["body"]]


def test_growth_reallocates_rows_and_pool(parse_pair):
    host, _ = parse_pair
    gpu = gpu_of(C.PARSE_CALLS, row_capacity=4, pool_capacity=64)
    assert gpu.store.row_capacity > 4 and gpu.store.pool.numel() > 64
    for pat, ci in R.PARSE_REGEX:
        same_search(host, gpu, pat, case_insensitive=ci)


# -------------------------------------------------------------- tile edges
@pytest.fixture(scope="module")
def tile_pair():
    lib = native.gpu()
    tile = int(lib.df_log_tile_bytes())
    overhang = int(lib.df_log_re_overhang())
    assert overhang % 16 == 0 and 0 < overhang < tile
    payload, at = R.regex_tile_payload(tile, overhang)
    calls = [("lines", payload, 3, "system")]
    host = C.host_of(calls)
    gpu = gpu_of(calls)
    assert gpu.store.pool_len == len(payload)
    return host, gpu, tile, overhang, at, payload


def test_match_starts_around_a_tile_edge(tile_pair):
    host, gpu, tile, _, at, payload = tile_pair
    assert at["edge1"] == tile - 1 and at["onedge"] == 2 * tile
    # starts 1 byte before the first edge
    assert len(same_search(host, gpu, r"EDGE1-[A-Z]+ ok$")) == 1
    assert len(same_search(host, gpu, r"E?DGE1-MATCH")) == 1
    # starts exactly on the second edge
    assert len(same_search(host, gpu, r"ONEDGE-\w+")) == 1
    assert len(same_search(host, gpu, r"\.ONEDGE")) == 1
    assert len(same_search(host, gpu, r"(EDGE1|ONEDGE)-MATCH")) == 2
    assert same_search(host, gpu, r"EDGE1-MATCH", "ONEDGE") == []


def test_walk_continues_past_the_staged_bytes(tile_pair):
    host, gpu, tile, overhang, at, payload = tile_pair
    # START lies in the third tile, END beyond that tile's overhang
    end = payload.index(R.END.encode())
    assert at["long"] < 3 * tile and end > 3 * tile + overhang
    for pat in (R.START + ".*" + R.END, R.START + "=+" + R.END + " ok$",
                r"^\.+" + R.START + "=*" + R.END, R.START + r"[^\n]+K"):
        assert len(same_search(host, gpu, pat)) == 1
    # the same walk on the last row of the pool: no END, and the walk stops
    # at the row's end, which is the pool's length, not its capacity
    assert at["last"] < 4 * tile
    assert len(payload) > 4 * tile + overhang
    assert gpu.store.pool.numel() > gpu.store.pool_len
    assert same_search(host, gpu, R.START + "=+[^=]") \
        == same_search(host, gpu, R.START + ".*" + R.END)
    assert same_search(host, gpu, "last.*" + R.END) == []
    assert same_search(host, gpu, "=+x") == []
    # ... and reaches it when the pattern asks for the end
    last = same_search(host, gpu, R.START + "=+$")
    assert [r["body"] for r in last] == [host.rows[-1]["body"]]
    assert same_search(host, gpu, r"^\.+" + R.START + "=+$") == last
    assert len(same_search(host, gpu, R.START + "=+")) == 2


def test_dense_pattern_hits_every_row_of_every_tile(tile_pair):
    host, gpu, tile, _, _, payload = tile_pair
    assert len(payload) > 3 * tile
    assert len(same_search(host, gpu, r"\.", limit=10000)) == host.n_rows
    assert len(same_search(host, gpu, r"^\.+", limit=10000)) == host.n_rows
    same_search(host, gpu, r"\.", limit=7, app_service="tile1")
    assert gpu.histogram(3, C.T0, C.T0 + 7, regex=r"\.\.$") == \
        host.histogram(3, C.T0, C.T0 + 7, regex=r"\.\.$") != []


# ------------------------------------------------------- limits and errors
def test_limits_are_the_python_constants():
    assert gpu_ops.log_re_limits() == (
        logregex.MAX_TABLE_BYTES, logregex.MAX_PATTERN_BYTES,
        logregex.MAX_CLASSES)
    assert gpu_ops.LOG_RE_BIT == 1 << 8


@pytest.mark.parametrize("k", range(len(R.REFUSED)))
def test_refused_on_the_gpu_store(scan_pair, k):
    pat, _ = R.REFUSED[k]
    _, gpu = scan_pair
    empty = AppLogPipeline(device="cuda")
    for pipe in (gpu, empty):
        with pytest.raises(ValueError):
            pipe.search(regex=pat)
        with pytest.raises(ValueError):
            pipe.store.search(regex=pat)
        with pytest.raises(ValueError):
            pipe.histogram(1, C.T0, C.T0 + 7, regex=pat)
        with pytest.raises(ValueError):
            pipe.store.histogram(1, C.T0 + 7, C.T0, regex=pat)


def test_non_str_is_a_type_error(scan_pair):
    _, gpu = scan_pair
    with pytest.raises(TypeError):
        gpu.search(regex=b"a")
    with pytest.raises(TypeError):
        gpu.store.search(regex=5)


def test_a_large_dfa_fills_the_lds_table(scan_pair):
    """A pattern whose tables come close to the 32 KiB the kernel stages."""
    host, gpu = scan_pair
    pat = r"(k\dk ){7}k7k|pool-e[a-z]{2}|(a|b)*a(a|b){9}!"
    rx = logregex.compile_log_regex(pat)
    assert rx.next.nbytes > logregex.MAX_TABLE_BYTES // 2
    assert len(same_search(host, gpu, pat)) == 2


# ------------------------------------------------------------------ server
def test_server_gpu_logs_regex(monkeypatch):
    monkeypatch.setattr(applog_pipeline, "time",
                        types.SimpleNamespace(time=lambda: C.NOW))
    lines = b"\n".join([
        b"1700000100 ERROR checkout failed to connect to db status=503",
        b"1700000101 info checkout request ok status=200",
        b"1700000102 warn checkout Dial tcp refused status=502",
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
        bad = client.get("/v1/logs/search", params={"re": "("})
        assert bad.status_code == 400
        assert client.get("/v1/logs/histogram", params={
            "interval": 60, "time_start": 1700000100, "time_end": C.NOW,
            "re": r"a\1"}).status_code == 400
        out[dev] = (
            client.get("/v1/logs/search", params={
                "re": r"STATUS=5\d\d$", "q": "ED",
                "case_insensitive": "true"}).json(),
            client.get("/v1/logs/search", params={
                "re": r"(connect|dial) .*refused"}).json(),
            client.get("/v1/logs/search", params={"re": r"^free"}).json(),
            client.get("/v1/logs/histogram", params={
                "interval": 60, "time_start": 1700000100,
                "time_end": C.NOW, "q": "status",
                "re": r"=\d+$"}).json(),
        )
    assert out["cuda"] == out["cpu"]
    both, none, free, hist = out["cuda"]
    assert len(both) == 2 and none == [] and len(free) == 1
    assert sum(d["count"] for d in hist) == 3
