"""Log patterns on the GPU application-log store (K14, k_log_patterns in
ops/csrc/dflog.hip) against query/logpattern.py row by row and against the
host AppLogPipeline fed the same calls (-m gpu). Every comparison is exact."""
import os
import sys
import types

import pytest
import torch
from fastapi.testclient import TestClient

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402
import applog_pattern_cases as P  # noqa: E402

from deepflow_amd.ingest import applog_pipeline  # noqa: E402
from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.ops import gpu_ops, native  # noqa: E402
from deepflow_amd.query import logpattern as L  # noqa: E402
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402

SENTINEL = 0x5A5A5A5A5A5A5A5A


def gpu_of(calls, **kw):
    assert torch.cuda.is_available()
    pipe = AppLogPipeline(device="cuda", **kw)
    C.feed(pipe, calls)
    return pipe


def signed(k):
    return k - (1 << 64) if k >= 1 << 63 else k


def test_constants_are_the_python_ones():
    lib = native.gpu()
    assert int(lib.df_log_pattern_prefix()) == L.PATTERN_PREFIX
    slots = int(lib.df_log_pattern_lds_slots())
    assert slots >= 2 and slots & (slots - 1) == 0


# ---------------------------------------------------------------- row keys
def check_row_keys(store, bodies):
    """Run the kernel with out_key over `store`, whose row r holds
    bodies[r], with every third row unselected: each selected row gets
    template_key(body), the others keep the sentinel, and the table's
    counts are those of the selected rows."""
    n = store.n_rows
    assert n == len(bodies)
    flags = torch.tensor([0 if r % 3 == 1 else 1 for r in range(n)],
                         dtype=torch.uint8, device=store.device)
    out = torch.full((max(n, 1),), SENTINEL, dtype=torch.int64,
                     device=store.device)
    t = gpu_ops.log_patterns(store, flags, 1 << 10, out_key=out)
    got = out[:n].tolist()
    want = {}
    for r, b in enumerate(bodies):
        if r % 3 == 1:
            assert got[r] == SENTINEL, r
            continue
        key = L.template_key(b)
        assert got[r] == signed(key), (r, b)
        w = want.setdefault(key, [0, r, r])
        w[0] += 1
        w[2] = r
    assert int(t.drops.item()) == 0
    keys = t.keys.tolist()
    count = t.count.tolist()
    first = t.first_row.tolist()
    last = t.last_row.tolist()
    table = {k & ((1 << 64) - 1): [count[s], first[s], last[s]]
             for s, k in enumerate(keys) if k}
    assert table == want
    assert all(c == 0 and f == -1 for k, c, f in zip(keys, count, first)
               if not k)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 0])
def test_row_keys_lines(n):
    src = P.LINE_BODIES
    call, bodies = P.lines_call([src[i % len(src)] for i in range(n)])
    gpu = gpu_of([call] if n else [])
    check_row_keys(gpu.store, bodies)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 0])
def test_row_keys_rows(n):
    src = P.TEXT_BODIES
    texts = [src[(i * 7) % len(src)] for i in range(n)]
    gpu = gpu_of([P.rows_call(texts)] if n else [])
    check_row_keys(gpu.store, [t.encode() for t in texts])


@pytest.mark.parametrize("rem", [0, 1, 15])
def test_last_row_ends_the_pool(rem):
    call, bodies = P.lines_call(P.LINE_BODIES, pad_to=(rem, 16))
    payload = call[1]
    assert len(payload) % 16 == rem and payload.endswith(bodies[-1])
    # a pool with no room to spare: its capacity is pool_len rounded up
    gpu = gpu_of([call], pool_capacity=len(payload))
    st = gpu.store
    assert st.pool_len == len(payload)
    assert st.pool.numel() == (len(payload) + 15) // 16 * 16
    n = st.n_rows
    assert int(st.row_boff[n - 1]) + int(st.row_blen[n - 1]) == st.pool_len
    check_row_keys(st, bodies)


# -------------------------------------------------------------- whole query
def same_patterns(host, gpu, **kw):
    want = host.patterns(**kw)
    got = gpu.patterns(**kw)
    assert got == want, kw
    assert gpu.store.patterns(**kw) == want
    return got


@pytest.fixture(scope="module")
def pattern_pair():
    host = C.host_of(P.PATTERN_CALLS)       # computed once, shared, unchanged
    gpu = gpu_of(P.PATTERN_CALLS)
    assert gpu.rows == host.rows
    return host, gpu


@pytest.fixture(scope="module")
def scan_pair():
    host = C.host_of(C.SCAN_CALLS)
    gpu = gpu_of(C.SCAN_CALLS)
    assert gpu.rows == host.rows
    return host, gpu


@pytest.mark.parametrize("k", range(len(P.PATTERN_QUERIES)))
def test_pattern_corpus(pattern_pair, k):
    host, gpu = pattern_pair
    kw = P.PATTERN_QUERIES[k]
    if kw.get("max_patterns") == 1:         # that one drops on the GPU
        kw = {"max_patterns": 1 << 8}
    same_patterns(host, gpu, **kw)


def test_limits_and_nothing_selected(pattern_pair):
    host, gpu = pattern_pair
    full = same_patterns(host, gpu, limit=1000)
    assert full["matched"] == host.n_rows
    assert len(full["patterns"]) == full["distinct"] > 20
    assert same_patterns(host, gpu, limit=1)["patterns"] == \
        full["patterns"][:1]
    none = same_patterns(host, gpu, substr="no such text anywhere")
    assert none == {"matched": 0, "distinct": 0, "dropped_rows": 0,
                    "patterns": []}
    assert AppLogPipeline(device="cuda").patterns() == none
    # the same answer twice, and whatever the table's size
    assert gpu.patterns(limit=1000) == full
    assert gpu.patterns(limit=1000, max_patterns=1 << 7) == full


def test_scan_corpus_every_filter(scan_pair):
    host, gpu = scan_pair
    matched = set()
    for kw in P.scan_queries():
        matched.add(same_patterns(host, gpu, **kw)["matched"])
    assert len(matched) > 5


@pytest.mark.parametrize("k", range(len(P.BAD_ARGS)))
def test_value_errors_full_and_empty(pattern_pair, k):
    kw, word = P.BAD_ARGS[k]
    for pipe in (pattern_pair[1], AppLogPipeline(device="cuda")):
        with pytest.raises(ValueError, match=word):
            pipe.patterns(**kw)
        with pytest.raises(ValueError, match=word):
            pipe.store.patterns(**kw)


# -------------------------------------------------------------- skew, spill
def test_skew_counts_are_exact_across_blocks():
    calls = P.skew_calls()
    host = C.host_of(calls)
    gpu = gpu_of(calls)
    assert gpu.n_rows == host.n_rows > 5000     # 20 blocks of 256 rows
    got = same_patterns(host, gpu)
    assert got["patterns"][0]["count"] == 5000
    assert got["patterns"][0]["pattern"] == "request <*> took <*>"
    assert got["distinct"] == 3
    same_patterns(host, gpu, substr="cold")
    same_patterns(host, gpu, regex=r"took 9\dms$", time_start=P.T0 + 10)


def test_spill_past_the_lds_table():
    slots = int(native.gpu().df_log_pattern_lds_slots())
    calls, d = P.spill_calls(slots)
    assert d > 2 * slots
    host = C.host_of(calls)
    gpu = gpu_of(calls)
    got = same_patterns(host, gpu, limit=10 ** 6)
    assert got["distinct"] == d == len(got["patterns"])
    assert got["matched"] == host.n_rows == sum(
        p["count"] for p in got["patterns"])
    assert {p["count"] for p in got["patterns"]} == {2, 3}
    same_patterns(host, gpu, limit=7)
    # a global table barely larger than the number of patterns
    cap = 1 << d.bit_length()
    assert same_patterns(host, gpu, limit=10 ** 6, max_patterns=cap) == got


# ---------------------------------------------------------------- overflow
@pytest.mark.parametrize("cap", [2, 1])
def test_overflow_drops_whole_patterns(cap):
    host = C.host_of(P.OVERFLOW_CALLS)
    gpu = gpu_of(P.OVERFLOW_CALLS)
    want = {p["pattern"]: p for p in host.patterns(limit=100)["patterns"]}
    assert len(want) == 5
    got = gpu.patterns(limit=100, max_patterns=cap)
    assert got["matched"] == len(P.OVERFLOW_LINES)
    assert 1 <= got["distinct"] <= cap
    assert len(got["patterns"]) == got["distinct"]
    assert got["dropped_rows"] > 0
    assert got["dropped_rows"] == \
        got["matched"] - sum(p["count"] for p in got["patterns"])
    for p in got["patterns"]:
        assert p == want[p["pattern"]]
    # with room for all five nothing is dropped
    assert gpu.patterns(limit=100, max_patterns=8) == host.patterns(limit=100)


# --------------------------------------------------------- after retention
def test_after_retention_with_a_full_app_table():
    host = C.host_of(P.RETENTION_CALLS)
    gpu = gpu_of(P.RETENTION_CALLS, app_capacity=1)
    assert gpu.store.n_apps == 1 and gpu.store.app_drops == 0
    assert host.evict_rows(3) == gpu.evict_rows(3) == 3
    st = gpu.store
    # the app's name moved to the arena at the front of the new pool and
    # every body was rebased behind it
    assert int(st.app_off[0]) == 0
    assert int(st.row_boff[0]) >= 16
    assert gpu.rows == host.rows
    for kw in ({}, {"limit": 1}, {"app_service": "solo"},
               {"substr": "solo"}, {"regex": r"^job \d"},
               {"severity_max": 4}, {"time_start": 6, "time_end": 10}):
        same_patterns(host, gpu, **kw)
    got = gpu.patterns()
    assert got["patterns"][0]["pattern"] == "job <*> finished in <*>"
    assert got["patterns"][0]["count"] == 4
    # ... and with the byte rule doing the evicting
    lines = [b"%d info solo job %d took %dms" % (i, i, i * 7) if i % 3
             else b"%d warn solo queue is full" % i for i in range(1, 120)]
    calls = [("lines", b"\n".join(lines[k:k + 10]), 1, "system")
             for k in range(0, len(lines), 10)]
    gpu = gpu_of(calls, app_capacity=1, max_pool_bytes=1500)
    assert gpu.evictions > 0 and 0 < gpu.n_rows < len(lines)
    twin = AppLogPipeline()
    twin.rows = gpu.rows
    for kw in ({}, {"substr": "job"}, {"limit": 1}):
        same_patterns(twin, gpu, **kw)


# ------------------------------------------------------------------ server
def test_server_gpu_logs_patterns(monkeypatch):
    monkeypatch.setattr(applog_pipeline, "time",
                        types.SimpleNamespace(time=lambda: C.NOW))
    lines = b"\n".join([
        b"1700000100 ERROR checkout failed to connect to db status=503",
        b"1700000101 info checkout request ok status=200",
        b"1700000102 warn checkout Dial tcp refused status=502",
        b"1700000103 info checkout request ok status=201",
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
        for bad in ({"max_patterns": 3}, {"re": "("}):
            assert client.get("/v1/logs/patterns",
                              params=bad).status_code == 400
        out[dev] = (
            client.get("/v1/logs/patterns").json(),
            client.get("/v1/logs/patterns", params={
                "q": "STATUS", "re": r"=\d+$", "case_insensitive": "true",
                "limit": 1, "max_patterns": 16}).json(),
            client.get("/v1/logs/patterns", params={
                "app_service": "checkout", "severity_max": 4}).json(),
        )
    assert out["cuda"] == out["cpu"]
    every, top, sev = out["cuda"]
    assert every["matched"] == 5 and every["distinct"] == 4
    assert top["patterns"] == [{
        "pattern": "request ok status=<*>", "count": 2,
        "sample": every["patterns"][0]["sample"]}]
    assert top["matched"] == 4 and sev["matched"] == 2
