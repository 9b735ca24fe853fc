"""Regex search over application logs (K13), host side: the pattern
compiler of query/logregex.py against Python's `re`, what it refuses, and
the host pipeline and HTTP surface with the new `regex` / `re` parameter.
No GPU."""
import os
import re
import sys
import time

import numpy as np
import pytest
from fastapi.testclient import TestClient

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402
import applog_regex_cases as R  # noqa: E402

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.query import logregex  # noqa: E402
from deepflow_amd.query.logregex import compile_log_regex  # noqa: E402
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "deepflow_amd", "ops", "csrc", "dflog.hip")


# --------------------------------------------------------------- compiler
@pytest.mark.parametrize("ci", [False, True])
def test_compiler_matches_re(ci):
    assert len(R.PATTERNS) >= 40 and len(R.BODIES) > 1600
    for pat in R.PATTERNS:
        rx = compile_log_regex(pat, ci)
        host = re.compile(pat.encode("utf-8"), R.host_flags(ci))
        wrong = [s for s in R.BODIES
                 if rx.search_py(s) != bool(host.search(s))]
        assert not wrong, (pat, ci, wrong[:5])
        assert rx.host.pattern == host.pattern
        assert rx.host.flags == host.flags


def test_tables_have_the_documented_shape():
    rx = compile_log_regex(R.PATTERNS[-1])
    assert rx.class_of.dtype == np.uint8 and rx.class_of.shape == (256,)
    assert rx.next.dtype == np.uint16
    assert rx.next.shape == (rx.n_states * rx.n_classes,)
    assert rx.accept.shape == (rx.n_states,) and not rx.accept[0]
    assert 8 <= rx.n_classes <= logregex.MAX_CLASSES
    assert rx.next.nbytes <= logregex.MAX_TABLE_BYTES
    # the dead state stays dead; every target is a state
    assert not rx.next[:rx.n_classes].any()
    assert int(rx.next.max()) < rx.n_states
    # table(): class_of, then next with the target's accept bit on top
    t = rx.table()
    assert t.dtype == np.uint8 and t.nbytes == 256 + rx.next.nbytes
    assert (t[:256] == rx.class_of).all()
    packed = t[256:].view(np.uint16)
    assert ((packed & 0x7fff) == rx.next).all()
    assert ((packed >> 15).astype(bool) == rx.accept[rx.next]).all()
    flags = {p: compile_log_regex(p) for p in
             ("a", "^a", "a$", r"a\Z", "^a*$", "a*", r"^\Z")}
    assert [(f.anchor_start, f.anchor_end, f.end_before_newline, f.nullable,
             f.matches_everything) for f in flags.values()] == [
        (False, False, False, False, False),
        (True, False, False, False, False),
        (False, True, True, False, False),
        (False, True, False, False, False),
        (True, True, True, True, False),
        (False, False, False, True, True),
        (True, True, False, True, False)]


def test_case_folding_is_baked_into_the_sets():
    rx = compile_log_regex("[^a]Z", True)
    assert not rx.search_py(b"az") and not rx.search_py(b"AZ")
    assert rx.search_py(b"bz") and rx.search_py(b"\xc9Z")
    # A-Z only: 0xC9/0xE9 (Latin-1 E-acute) are different bytes
    assert not compile_log_regex(r"\xe9", True).search_py(b"\xc9")


def test_cache_returns_the_same_object():
    a = compile_log_regex(r"timeout=\d+", False)
    assert compile_log_regex(r"timeout=\d+", False) is a
    assert compile_log_regex(r"timeout=\d+", True) is not a


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("k", range(len(R.REFUSED)))
def test_refused(k):
    pat, names = R.REFUSED[k]
    t0 = time.perf_counter()
    with pytest.raises(ValueError) as e:
        compile_log_regex(pat)
    assert time.perf_counter() - t0 < 1.0       # the blow-ups fail fast
    assert names in str(e.value)
    with pytest.raises(ValueError):
        compile_log_regex(pat, True)


def test_non_str_is_a_type_error():
    for bad in (b"a", 5, ["a"], re.compile("a")):
        with pytest.raises(TypeError):
            compile_log_regex(bad)
        with pytest.raises(TypeError):
            AppLogPipeline().search(regex=bad)


def test_limits_match_the_kernel_source():
    text = open(CSRC).read()
    for name, want in (("LOG_RE_TABLE_BYTES", logregex.MAX_TABLE_BYTES),
                       ("LOG_RE_MAX_PATTERN", logregex.MAX_PATTERN_BYTES),
                       ("LOG_RE_MAX_CLASSES", logregex.MAX_CLASSES)):
        m = re.search(r"constexpr uint32_t %s = ([^;]+);" % name, text)
        assert m, name
        assert eval(m.group(1), {"__builtins__": {}}) == want
    for name, want in (("RE_ANCHOR_START", logregex.FLAG_ANCHOR_START),
                       ("RE_ANCHOR_END", logregex.FLAG_ANCHOR_END),
                       ("RE_END_BEFORE_NL", logregex.FLAG_END_BEFORE_NL),
                       ("RE_NULLABLE", logregex.FLAG_NULLABLE)):
        m = re.search(r"\b%s = (\d+)[,;]" % name, text)
        assert m and int(m.group(1)) == want, name


# ----------------------------------------------------------- host pipeline
@pytest.fixture(scope="module")
def host():
    return C.host_of(C.SCAN_CALLS)


@pytest.mark.parametrize("k", range(len(R.SCAN_REGEX)))
def test_host_search_is_re_over_rows(host, k):
    pat, ci, hits = R.SCAN_REGEX[k]
    got = host.search(regex=pat, case_insensitive=ci, limit=1000)
    assert got == R.re_rows(host.rows, pat, ci)
    assert len(got) == hits


@pytest.mark.parametrize("k", range(len(R.SCAN_COMBINED)))
def test_host_regex_combines_with_every_filter(host, k):
    pat, kw = R.SCAN_COMBINED[k]
    kw = dict(kw)
    limit = kw.pop("limit", 1000)
    plain = host.search(limit=1000, **kw)
    want = [r for r in plain
            if r in R.re_rows(host.rows, pat,
                              kw.get("case_insensitive", False))]
    assert host.search(regex=pat, limit=limit, **kw) == want[:limit]


def test_host_histogram_counts_the_same_rows(host):
    for pat, ci in ((r"t[eh]", False), (r"NEEDLE|POOL", True), (r"^$", False),
                    (r".*", False)):
        rows = host.search(regex=pat, case_insensitive=ci, limit=1000,
                           time_start=C.T0, time_end=C.T0 + 7)
        hist = host.histogram(2, C.T0, C.T0 + 7, regex=pat,
                              case_insensitive=ci)
        assert sum(d["count"] for d in hist) == len(rows)
    assert host.histogram(2, C.T0, C.T0 + 7, "e", 4, app_service="beta",
                          regex=r"t.*n") == \
        host.histogram(2, C.T0, C.T0 + 7, ["e", "t"], 4, app_service="beta",
                       regex=r"t.*n") != []


def test_empty_and_none_constrain_nothing(host):
    for kw in ({}, {"substr": "e", "severity_max": 4}):
        want = host.search(limit=1000, **kw)
        assert host.search(regex="", limit=1000, **kw) == want
        assert host.search(regex=None, limit=1000, **kw) == want
    assert host.histogram(2, C.T0, C.T0 + 7, regex="") == \
        host.histogram(2, C.T0, C.T0 + 7, regex=None) == \
        host.histogram(2, C.T0, C.T0 + 7)


def test_bad_pattern_raises_on_an_empty_store():
    empty = AppLogPipeline()
    for pat, _ in R.REFUSED[:8]:
        with pytest.raises(ValueError):
            empty.search(regex=pat)
        with pytest.raises(ValueError):
            empty.histogram(1, 0, 10, regex=pat)
        with pytest.raises(ValueError):         # also with an empty window
            empty.histogram(1, 10, 0, regex=pat)
    assert empty.search(regex="a") == []


def test_endpoints_take_re_on_a_cpu_server():
    srv = DeepflowServer(device="cpu", tcp_port=0, segment_rows=1 << 10,
                         dict_capacity=1 << 12)
    for call in C.SCAN_CALLS:
        assert srv.receiver.handle_frame(framing.encode_frame(
            framing.FrameHeader(msg_type=framing.MSG_APPLICATION_LOG,
                                agent_id=call[2]), call[1]))
    pipe = srv.applogs
    client = TestClient(srv.app)
    r = client.get("/v1/logs/search", params={
        "re": r"NEEDLE-(start|end)", "q": "text", "case_insensitive": "true"})
    assert r.status_code == 200
    assert r.json() == pipe.search("text", regex=r"NEEDLE-(start|end)",
                                   case_insensitive=True)
    assert len(r.json()) == 3
    r = client.get("/v1/logs/histogram", params={
        "interval": 2, "time_start": C.T0, "time_end": C.T0 + 7,
        "re": r"t[eh]"})
    assert r.status_code == 200
    assert r.json() == pipe.histogram(2, C.T0, C.T0 + 7, regex=r"t[eh]") != []
    assert client.get("/v1/logs/search",
                      params={"re": ""}).json() == pipe.search()
    for bad in ("(", r"(a)\1", r"\bx", "^a|b"):
        assert client.get("/v1/logs/search",
                          params={"re": bad}).status_code == 400
        assert client.get("/v1/logs/histogram", params={
            "interval": 2, "time_start": C.T0, "time_end": C.T0 + 7,
            "re": bad}).status_code == 400
