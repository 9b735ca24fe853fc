"""Host side of the application-log store (K11): the numpy line splitter,
the new search filters, the histogram and the two HTTP endpoints. No GPU."""
import os
import sys

import numpy as np
import pytest
from fastapi.testclient import TestClient

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402

from deepflow_amd.ingest.applog_pipeline import (AppLogPipeline,  # noqa: E402
                                                 fold_ascii)
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.store.log_store import split_log_lines  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402


def lines_ref(payload: bytes):
    """What ingest_lines keeps, computed its way (latin-1 keeps every byte
    a single char, so only the ASCII whitespace is stripped)."""
    out = []
    for line in payload.splitlines():
        line = line.decode("latin-1").strip(
            "\t\n\v\f\r\x1c\x1d\x1e\x1f ").encode("latin-1")
        if line:
            out.append(line)
    return out


@pytest.mark.parametrize("payload", [
    b"",
    b"\n\n \n\t\r\n",                             # blank lines only
    b"a b\r\nc d\r\n",
    b"one\rtwo\r\rthree",                         # \r alone
    b"tail ws \x1c\x1d\x1e\x1f\nnext\x1f",        # bytes 28-31
    b"no newline at all",
    b"  lead and trail  \n\x0b\x0cx\x0b\n",
    b"\r\n\r\n x \r\n",
    b"\x85 not ascii ws \xa0\n\x00nul stays\x00",
    b"x",
    b"\n",
] + [c[1] for c in C.PARSE_CALLS + C.SCAN_CALLS if c[0] == "lines"])
def test_split_log_lines(payload):
    off, ln = split_log_lines(np.frombuffer(payload, dtype=np.uint8))
    assert off.dtype == np.int64 and ln.dtype == np.int32
    got = [payload[o:o + n] for o, n in zip(off.tolist(), ln.tolist())]
    assert got == lines_ref(payload)


def test_split_matches_ingest_lines():
    for call in C.PARSE_CALLS + C.SCAN_CALLS:
        if call[0] != "lines":
            continue
        p = AppLogPipeline()
        n = p.ingest_lines(call[1], now=C.NOW)
        off, _ = split_log_lines(np.frombuffer(call[1], dtype=np.uint8))
        assert n == off.shape[0] == p.n_rows


@pytest.fixture(scope="module")
def host():
    return C.host_of(C.SCAN_CALLS)


def bodies(rows):
    return [r["body"] for r in rows]


def test_defaults_match_the_old_call(host):
    # the parent's search(), verbatim
    def old(substr="", severity_max=7, limit=100):
        out = []
        for r in reversed(host.rows):
            if r["severity"] <= severity_max and \
                    (not substr or substr in r["body"]):
                out.append(r)
                if len(out) >= limit:
                    break
        return out
    assert host.search() == old()
    assert host.search("needle") == old("needle")
    assert host.search("e", 4, 3) == old("e", 4, 3)
    assert host.search(severity_max=3) == old(severity_max=3)
    assert host.search(limit=0) == []


def test_now_is_applied_to_free_form_lines():
    p = AppLogPipeline()
    p.ingest_lines(b"free\n1700000001 info a b", now=42)
    assert [r["time"] for r in p.rows] == [42, 1700000001]


def test_search_filters(host):
    n = len(host.rows)
    assert len(host.search(limit=1000)) == n
    assert bodies(host.search("needle-end")) == ["text then needle-end"]
    assert bodies(host.search(["pre", "post"])) == [
        "pre %s# post" % C.N128[:-1], "pre %s post" % C.N128]
    assert bodies(host.search(C.AND8)) == [
        "all eight " + " ".join(C.AND8)]
    assert host.search(["", "hello"]) == host.search("hello")
    with pytest.raises(ValueError):
        host.search(["x"] * 9)
    got = host.search(time_start=C.T0 + 3, time_end=C.T0 + 7, limit=1000)
    assert got and all(C.T0 + 3 <= r["time"] <= C.T0 + 7 for r in got)
    assert {r["time"] for r in got} >= {C.T0 + 3, C.T0 + 7}
    got = host.search(app_service="beta", limit=1000)
    assert len(got) == 4 and all(r["app_service"] == "beta" for r in got)
    assert host.search(app_service="never-ingested") == []
    assert [r["time"] for r in host.search(app_service="")] == [C.NOW]
    # newest first, cut at limit
    allrows = host.search(limit=1000)
    assert allrows == list(reversed(host.rows))
    assert host.search(limit=3) == allrows[:3]


def test_case_insensitive_folds_ascii_only(host):
    assert fold_ascii("AZaz[@É") == "azaz[@É"
    assert host.search("NEEDLE-start") == []
    assert len(host.search("NEEDLE-start", case_insensitive=True)) == 2
    assert bodies(host.search("mIxEdÉcAsE", case_insensitive=True)) == [
        "MiXeDÉCase body"]
    assert bodies(host.search("mixedécase", case_insensitive=True)) == [
        "lower mixedécase body"]


def test_histogram(host):
    full = host.histogram(2, C.T0, C.T0 + 7)
    assert full == sorted(full, key=lambda d: (d["time"], d["severity"]))
    assert sum(d["count"] for d in full) == len(host.rows) - 1   # not NOW
    assert all(d["count"] > 0 and (d["time"] - C.T0) % 2 == 0 for d in full)
    want = {}
    for r in host.rows:
        if C.T0 <= r["time"] <= C.T0 + 7:
            k = (C.T0 + (r["time"] - C.T0) // 2 * 2, r["severity"])
            want[k] = want.get(k, 0) + 1
    assert {(d["time"], d["severity"]): d["count"] for d in full} == want
    # rows exactly on both ends of a narrower window
    edge = host.histogram(1, C.T0 + 3, C.T0 + 7)
    assert {d["time"] for d in edge} >= {C.T0 + 3, C.T0 + 7}
    # same filters as search
    beta = host.histogram(4, C.T0, C.T0 + 7, "e", 4, app_service="beta",
                          case_insensitive=True)
    assert sum(d["count"] for d in beta) == len(host.search(
        "e", 4, 1000, time_start=C.T0, time_end=C.T0 + 7,
        app_service="beta", case_insensitive=True))
    assert len(host.histogram(1, C.T0, C.T0 + 4095)) > 0      # 4096 buckets
    assert host.histogram(1, C.T0 + 5, C.T0 + 4) == []
    with pytest.raises(ValueError):
        host.histogram(0, C.T0, C.T0 + 7)
    with pytest.raises(ValueError):
        host.histogram(1, C.T0, C.T0 + 4096)                  # 4097 buckets


def test_histogram_clamps_severity():
    p = AppLogPipeline()
    p.ingest_rows([{"time": 5, "severity": 11, "body": "x"},
                   {"time": 5, "severity": -2, "body": "y"}])
    assert p.histogram(10, 0, 9, severity_max=99) == [
        {"time": 0, "severity": 0, "count": 1},
        {"time": 0, "severity": 7, "count": 1}]


def test_endpoints_on_a_cpu_server():
    srv = DeepflowServer(device="cpu", tcp_port=0, segment_rows=1 << 10,
                         dict_capacity=1 << 12, gpu_logs=True)  # ignored
    assert not srv.applogs.gpu
    for call in C.SCAN_CALLS:
        assert srv.receiver.handle_frame(framing.encode_frame(
            framing.FrameHeader(msg_type=framing.MSG_APPLICATION_LOG,
                                agent_id=call[2]), call[1]))
    pipe = srv.applogs
    client = TestClient(srv.app)
    r = client.get("/v1/logs/search")
    assert r.status_code == 200 and r.json() == pipe.search()
    r = client.get("/v1/logs/search", params={
        "q": ["pre", "POST"], "case_insensitive": "true", "limit": 1})
    assert r.json() == pipe.search(["pre", "POST"], limit=1,
                                   case_insensitive=True)
    assert len(r.json()) == 1
    r = client.get("/v1/logs/search", params={
        "severity_max": 3, "time_start": C.T0 + 1, "time_end": C.T0 + 7,
        "app_service": "beta"})
    assert r.json() == pipe.search(severity_max=3, time_start=C.T0 + 1,
                                   time_end=C.T0 + 7, app_service="beta")
    assert len(r.json()) == 3
    r = client.get("/v1/logs/histogram", params={
        "interval": 2, "time_start": C.T0, "time_end": C.T0 + 7, "q": "e"})
    assert r.status_code == 200
    assert r.json() == pipe.histogram(2, C.T0, C.T0 + 7, "e") != []
    r = client.get("/v1/logs/histogram", params={
        "interval": 0, "time_start": C.T0, "time_end": C.T0 + 7})
    assert r.status_code == 400
    r = client.get("/v1/logs/search", params={"q": ["x"] * 9})
    assert r.status_code == 400
