"""ProfilePipeline.flame()/processes() dispatch, the time-window HTTP
parameters and the vectorised line splitter of the GPU profile store (pure
numpy; no GPU needed)."""
import numpy as np
from fastapi.testclient import TestClient

from deepflow_amd.ingest.profile_pipeline import (ProfilePipeline,
                                                  ProfileStore, build_flame)
from deepflow_amd.server import DeepflowServer
from deepflow_amd.store.profile_store import split_lines
from deepflow_amd.wire import pb, metric, framing


def mk_profile(stacks, process="svc-a", event_type=1, ts=1000000):
    data = "\n".join(f"{s} {c}" for s, c in stacks).encode()
    return {
        "name": "app", "units": "samples", "format": "folded",
        "data": data, "timestamp": ts, "event_type": event_type,
        "pid": 42, "process_name": process, "spy_name": "ebpf",
        "count": 1,
    }


def _fed_pipeline(**kw):
    pipe = ProfilePipeline(**kw)
    msgs = [
        mk_profile([("main;work;io", 5), ("main;work;spin", 3),
                    ("main;idle", 2)], process="pa", event_type=1, ts=100),
        mk_profile([("main;work;io", 4), ("other", 9)], process="pb",
                   event_type=2, ts=200),
        mk_profile([("main;gc", 6)], process="pa", event_type=2, ts=300),
    ]
    payload = framing.pack_records(
        [pb.encode(m, metric.PROFILE) for m in msgs])
    assert pipe.ingest_payload(payload) == 3
    return pipe


def test_default_store_is_host_store():
    assert type(ProfilePipeline().store) is ProfileStore
    assert type(ProfilePipeline(device="cpu").store) is ProfileStore
    assert type(ProfilePipeline(device="cpu",
                                stack_capacity=1 << 4).store) is ProfileStore


def test_flame_and_processes_dispatch_to_host_path():
    pipe = _fed_pipeline()
    st = pipe.store
    assert pipe.processes() == sorted({r.process_name for r in st.rows})
    assert pipe.processes() == ["pa", "pb"]
    assert pipe.n_rows == len(st.rows) == 6
    for kw in ({}, {"event_type": 2}, {"process_name": "pa"},
               {"event_type": 2, "process_name": "pa"},
               {"time_start": 200, "time_end": 300},
               {"process_name": "nobody"}):
        assert pipe.flame(**kw) == build_flame(st.rows, st.id_to_loc, **kw)
    assert pipe.flame()["value"] == 29
    assert pipe.flame(process_name="nobody") == {
        "name": "root", "value": 0, "self": 0, "children": []}


def _cpu_server():
    srv = DeepflowServer(device="cpu", tcp_port=0, segment_rows=1 << 9,
                         dict_capacity=1 << 10)
    msgs = [mk_profile([("a;b", 7)], process="px", ts=100),
            mk_profile([("a;c", 5)], process="py", ts=200),
            mk_profile([("a;b", 3)], process="px", ts=300)]
    payload = framing.pack_records(
        [pb.encode(m, metric.PROFILE) for m in msgs])
    frame = framing.encode_frame(
        framing.FrameHeader(msg_type=framing.MSG_PROFILE), payload)
    assert srv.receiver.handle_frame(frame)
    return srv


def test_http_time_window_is_inclusive():
    srv = _cpu_server()
    assert type(srv.profiles.store) is ProfileStore
    client = TestClient(srv.app)

    def value(**params):
        return client.get("/v1/profile/flame", params=params).json()["value"]

    assert value() == 15
    assert value(time_start=100, time_end=300) == 15
    assert value(time_start=100, time_end=200) == 12
    assert value(time_start=200, time_end=200) == 5
    assert value(time_start=101, time_end=299) == 5
    assert value(time_start=201) == 3
    assert value(time_end=99) == 0
    assert value(process_name="px", time_start=300, time_end=300) == 3


def test_http_processes_and_mcp_unchanged():
    srv = _cpu_server()
    client = TestClient(srv.app)
    assert client.get("/v1/profile/processes").json() == ["px", "py"]
    tree = client.get("/v1/profile/flame",
                      params={"process_name": "px"}).json()
    assert tree["value"] == 10
    assert tree["children"][0]["name"] == "a"
    r = srv.mcp.handle({"jsonrpc": "2.0", "id": 1, "method": "tools/call",
                        "params": {"name": "profile_analysis",
                                   "arguments": {"process_name": "px"}}})
    text = r["result"]["content"][0]["text"]
    assert text.splitlines() == ["total samples: 10", "10 (100.0%)  a;b"]


# ---------------------------------------------------------------- splitter

def _host_lines(blobs, folded):
    """(offset, length, message) of every stack-bearing line, following
    ProfilePipeline.ingest_profile: splitlines() + strip() + skip-empty for
    collapsed blobs; one verbatim line otherwise."""
    out, base = [], 0
    parse = []
    for k, (data, fo) in enumerate(zip(blobs, folded)):
        if fo and (b"\n" in data or b" " in data.strip()):
            parse.append(1)
            pos = 0
            for raw in data.splitlines(keepends=True):
                line = raw.strip()
                if line:
                    lead = len(raw) - len(raw.lstrip())
                    out.append((base + pos + lead, len(line), k))
                pos += len(raw)
        else:
            parse.append(0)
            if data or not fo:
                out.append((base, len(data), k))
        base += len(data)
    return out, parse


def _split(blobs, folded=None):
    folded = [True] * len(blobs) if folded is None else folded
    buf = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    starts = np.zeros(len(blobs) + 1, dtype=np.int64)
    starts[1:] = np.cumsum([len(b) for b in blobs])
    off, ln, msg, parse = split_lines(buf, starts, np.array(folded))
    assert off.dtype == np.uint64 and ln.dtype == np.uint32
    assert msg.dtype == np.uint32 and parse.dtype == np.uint8
    return (list(zip(off.tolist(), ln.tolist(), msg.tolist())),
            parse.tolist())


def _check(blobs, folded=None):
    fo = [True] * len(blobs) if folded is None else folded
    got = _split(blobs, fo)
    want = _host_lines(blobs, fo)
    assert got == want
    return got[0]


def test_splitter_line_terminators():
    lines = _check([b"a;b 1\nc;d 2\r\ne;f 3\rg;h 4"])
    assert len(lines) == 4
    assert lines[2] == (13, 5, 0)


def test_splitter_blank_lines_and_tabs():
    lines = _check([b"\n\n  \n\ta;b 1\t\n\r\n \t x\ty 2 \n\n\r"])
    assert [ln for _, ln, _ in lines] == [5, 5]


def test_splitter_blob_without_newline():
    assert _check([b"a;b 7"]) == [(0, 5, 0)]
    assert _check([b"  a;b 7\t"]) == [(2, 5, 0)]
    # no newline and no inner space: the blob is one verbatim stack
    assert _split([b" a;b\t"]) == ([(0, 5, 0)], [0])
    assert _check([b"a\rb"]) == [(0, 3, 0)]
    assert _check([b" 5"]) == [(0, 2, 0)]


def test_splitter_empty_blob_between_two():
    lines = _check([b"a 1\nb 2", b"", b"c 3\n"])
    assert lines == [(0, 3, 0), (4, 3, 0), (7, 3, 2)]
    # a \r that ends one blob and a \n that starts the next stay apart
    _check([b"a 1\r", b"\nb 2", b"", b"", b"c"])
    _check([b"", b"", b"x y 1"])
    assert _check([b"", b""]) == []
    assert _check([b"   ", b"\n"]) == [(0, 3, 0)]


def test_splitter_non_folded_blob_is_one_line():
    blobs = [b"a 1\nb 2", b"p q\nr s 9\n", b"", b"c 3"]
    lines = _check(blobs, [True, False, False, True])
    assert lines == [(0, 3, 0), (4, 3, 0), (7, 10, 1), (17, 0, 2),
                     (17, 3, 3)]


def test_splitter_matches_host_on_seeded_noise():
    rng = np.random.default_rng(7)
    alphabet = np.frombuffer(b"ab;1 \t\n\r", dtype=np.uint8)
    for _ in range(200):
        blobs = [alphabet[rng.integers(0, len(alphabet),
                                       rng.integers(0, 24))].tobytes()
                 for _ in range(rng.integers(1, 5))]
        folded = (rng.random(len(blobs)) < 0.8).tolist()
        _check(blobs, folded)
