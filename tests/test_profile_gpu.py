"""GPU profile store + flame fold (K9) against the host ProfilePipeline and
build_flame fed the same messages. Every comparison is exact."""
import dataclasses

import numpy as np
import pytest
from fastapi.testclient import TestClient

from deepflow_amd.ingest.profile_pipeline import (ProfilePipeline,
                                                  ProfileStore, build_flame)
from deepflow_amd.wire import pb, metric, framing

pytestmark = pytest.mark.gpu


def msg(data, process="svc-a", event_type=1, ts=1_000_000, count=1,
        fmt="folded", **extra):
    d = {"name": "app", "units": "samples", "format": fmt, "data": data,
         "timestamp": ts, "event_type": event_type, "pid": 42,
         "process_name": process, "spy_name": "ebpf", "count": count}
    d.update(extra)
    return d


def payload_of(msgs):
    return framing.pack_records([pb.encode(m, metric.PROFILE) for m in msgs])


def both(payloads, **gpu_kw):
    host = ProfilePipeline()
    gpu = ProfilePipeline(device="cuda", **gpu_kw)
    for p in payloads:
        assert host.ingest_payload(p) == gpu.ingest_payload(p)
    return host, gpu


def row_tuples(store):
    locs = store.id_to_loc
    out = []
    for r in store.rows:
        t = dataclasses.asdict(r)
        t["location_id"] = locs[r.location_id]
        out.append(tuple(t.items()))
    return out


def canon(node):
    kids = sorted((canon(c) for c in node["children"]),
                  key=lambda c: (-c["value"], c["name"]))
    for a, b in zip(kids, kids[1:]):
        assert (a["value"], a["name"]) != (b["value"], b["name"])
    return {"name": node["name"], "value": node["value"],
            "self": node["self"], "children": kids}


def assert_same_flame(host, gpu, **kw):
    want = canon(build_flame(host.store.rows, host.store.id_to_loc, **kw))
    got = gpu.flame(**kw)
    assert got == want      # GPU side is already in canonical order
    return got


# 40 distinct stacks, depths 1..5, shared prefixes
STACKS = [";".join(["main", f"mod{i % 3}", f"fn{i % 8}", "deep"][:i % 5]
                   + [f"leaf{i}"])
          for i in range(40)]


def base_payload():
    def lines(lo, hi):
        out = []
        for j in range(lo, hi):
            s = STACKS[(j * 7) % 40]
            # every 11th line has no count: the message's count applies
            out.append(s if j % 11 == 0 else f"{s} {(j * 5) % 13 + 1}")
        return "\n".join(out).encode()
    return payload_of([
        msg(lines(0, 120), process="pa", event_type=1, ts=1_000_000,
            count=3),
        msg(lines(120, 220), process="pb", event_type=2, ts=2_000_000,
            count=5),
        msg(lines(220, 300), process="pa", event_type=2, ts=3_000_000,
            count=2)])


@pytest.fixture(scope="module")
def base_pair():
    return both([base_payload()])


def test_rows_and_dictionary_match_host(base_pair):
    host, gpu = base_pair
    assert len(set(STACKS)) == 40
    assert gpu.store.n_rows == len(host.store.rows) == 300
    assert gpu.n_rows == 300
    assert gpu.store.n_stacks == len(host.store.id_to_loc) == 40
    assert gpu.store.stack_drops == 0
    assert row_tuples(gpu.store) == row_tuples(host.store)
    assert gpu.store.id_to_loc == host.store.id_to_loc
    assert gpu.processes() == host.processes() == ["pa", "pb"]
    assert gpu.store.stored_bytes() == 300 * 24 + sum(
        len(s) for s in host.store.id_to_loc)


def _zstd(raw):
    from deepflow_amd.ops import native
    lib = native.cpu()
    src = np.frombuffer(raw, dtype=np.uint8)
    dst = np.zeros(1024, dtype=np.uint8)
    n = lib.df_zstd_compress(src.ctypes.data, len(raw), dst.ctypes.data,
                             1024, 3)
    return dst[:n].tobytes()


EDGE_LINES = [b"a;b 7", b"a;b", b"a b;c 12", b"a;b x9", b" 5", b"5",
              b" \t a;c 4 \t ", b"big;count 1099511627776", b"a;b  8",
              b"x 0012", b"solo"]


def test_line_parsing_edge_cases():
    msgs = [msg(b"\n".join(EDGE_LINES) + b"\n", count=21, ts=10)]
    # the same cases as single-line blobs without a newline
    msgs += [msg(line, count=30 + i, ts=100 + i)
             for i, line in enumerate(EDGE_LINES)]
    msgs.append(msg(b"p q\nr s 9\n 1 ", fmt="pprof", count=17, ts=500))
    msgs.append(msg(b"", fmt="pprof", count=2, ts=501))
    msgs.append(msg(b"", count=2, ts=502))
    msgs.append(msg(_zstd(b"x;y;z 11\nx;y 2"), ts=600, data_compressed=1))
    host, gpu = both([payload_of(msgs)])
    got = row_tuples(gpu.store)
    assert got == row_tuples(host.store)
    by = [(dict(t)["location_id"], dict(t)["value"]) for t in got]
    assert by[:len(EDGE_LINES)] == [
        (b"a;b", 7), (b"a;b", 21), (b"a b;c", 12), (b"a;b x9", 21),
        (b"5", 21), (b"5", 21), (b"a;c", 4), (b"big;count", 1 << 40),
        (b"a;b ", 8), (b"x", 12), (b"solo", 21)]
    assert (b" 5", 34) in by            # verbatim single blob
    assert (b"p q\nr s 9\n 1 ", 17) in by
    assert (b"", 2) in by
    assert by[-2:] == [(b"x;y;z", 11), (b"x;y", 2)]
    assert_same_flame(host, gpu)


def test_hash_and_copy_boundaries():
    lens = [1, 7, 8, 9, 15, 16, 17, 64]
    stacks = []
    for n in lens:
        s = (f"f{n};" + "abcdefghijklmnopqrstuvwxyz;" * 3)[:n].encode()
        assert len(s) == n
        stacks.append(s)
    stacks += ["héllo;wörld;日本語".encode(), "日;本;語;é".encode()]
    data, offs = b"q 1\n", []
    for i, s in enumerate(stacks):
        if len(data) % 8 == 0:
            data += b" "
        offs.append(len(data))
        data += s + b" " + str(i + 2).encode() + b"\n"
    assert all(o % 8 for o in offs)
    host, gpu = both([payload_of([msg(b"pad"), msg(data)])])
    assert gpu.store.id_to_loc == host.store.id_to_loc
    assert gpu.store.id_to_loc[2:] == stacks
    assert row_tuples(gpu.store) == row_tuples(host.store)
    assert_same_flame(host, gpu)


@pytest.fixture(scope="module")
def flame_pair():
    deep = ";".join(f"d{k}" for k in range(128))
    extra = "\n".join(["a;;b 3", ";a 4", "a; 5", f"{deep} 6",
                       "single 7"]).encode()
    return both([base_payload(),
                 payload_of([msg(extra, process="pc", event_type=3,
                                 ts=4_000_000)])])


@pytest.mark.parametrize("kw", [
    {}, {"event_type": 2}, {"process_name": "pa"},
    {"event_type": 2, "process_name": "pa"},
    {"time_start": 2_000_000, "time_end": 3_000_000},
    {"time_start": 4_000_000, "time_end": 4_000_000},
    {"process_name": "nobody"}, {"event_type": 1, "process_name": "pb"},
    {"time_start": 3_000_001, "time_end": 3_999_999},
], ids=str)
def test_flame_equals_host(flame_pair, kw):
    host, gpu = flame_pair
    got = assert_same_flame(host, gpu, **kw)
    if kw in ({"process_name": "nobody"},
              {"event_type": 1, "process_name": "pb"},
              {"time_start": 3_000_001, "time_end": 3_999_999}):
        assert got == {"name": "root", "value": 0, "self": 0,
                       "children": []}
    else:
        assert got["value"] > 0 and got["children"]


def test_flame_empty_frames_and_depth(flame_pair):
    _, gpu = flame_pair
    tree = gpu.flame(event_type=3)
    kids = {c["name"]: c for c in tree["children"]}
    assert sorted(kids) == ["", "a", "d0", "single"]
    assert kids[""]["children"][0]["name"] == "a"           # ";a"
    a = {c["name"]: c for c in kids["a"]["children"]}
    assert a[""]["value"] == 8 and a[""]["self"] == 5       # "a;" + "a;;b"
    assert a[""]["children"][0] == {"name": "b", "value": 3, "self": 3,
                                    "children": []}
    node, depth = kids["d0"], 1
    while node["children"]:
        assert node["self"] == 0 and node["value"] == 6
        node, depth = node["children"][0], depth + 1
    assert depth == 128 and node["name"] == "d127" and node["self"] == 6


def test_shared_prefix_under_contention():
    lines = [f"p0;p1;p2;leaf{i} {i + 1}" for i in range(512)] * 4
    host, gpu = both([payload_of([msg("\n".join(lines).encode())])])
    tree = assert_same_flame(host, gpu)
    total = 4 * 512 * 513 // 2
    node = tree
    for name in ("p0", "p1", "p2"):
        assert node["value"] == total and len(node["children"]) == 1
        node = node["children"][0]
        assert node["name"] == name and node["self"] == 0
    assert node["value"] == total
    assert {c["name"]: (c["value"], c["self"]) for c in node["children"]} \
        == {f"leaf{i}": (4 * (i + 1), 4 * (i + 1)) for i in range(512)}
    assert gpu.store.n_stacks == 512


def test_stack_ids_are_home_slots():
    """A stack id is the slot the probe starts at, `hash & (cap - 1)`, when
    that slot is free. cap = 4 is the smallest power of two with room for
    three distinct home slots."""
    import ctypes
    from deepflow_amd.ops import native
    from deepflow_amd.store.dictionary import str_hash_py
    seed_fn = native.gpu().df_prof_stack_seed
    seed_fn.restype, seed_fn.argtypes = ctypes.c_uint64, []
    seed, cap = int(seed_fn()), 4
    stacks, homes = [], []
    for i in range(64):
        s = b"frame%d" % i
        home = str_hash_py(s, seed) & (cap - 1)
        if home not in homes:
            stacks.append(s)
            homes.append(home)
        if len(stacks) == 3:
            break
    assert len(set(homes)) == len(stacks) == 3
    gpu = ProfilePipeline(device="cuda", stack_capacity=cap)
    data = b"\n".join(s + b" 1" for s in stacks)
    gpu.ingest_payload(payload_of([msg(data)]))
    st = gpu.store
    assert st.n_rows == 3 and st.stack_drops == 0
    assert st.row_stack[:3].tolist() == homes
    assert st.id_to_loc == stacks


def test_full_stack_table_is_bounded():
    value = {f"s{i};t".encode(): i + 1 for i in range(12)}
    data = b"\n".join(k + b" " + str(v).encode() for k, v in value.items())
    gpu = ProfilePipeline(device="cuda", stack_capacity=8)
    gpu.ingest_payload(payload_of([msg(data)]))
    st = gpu.store
    assert st.n_rows == 12
    assert st.n_stacks == 8
    assert st.stack_drops == 4
    kept = st.id_to_loc
    assert len(kept) == 8 and set(kept) <= set(value)
    assert len(st.rows) == 8
    assert gpu.flame()["value"] == sum(value[k] for k in kept)


def test_growth_of_rows_and_pool():
    from deepflow_amd.store.profile_store import GpuProfileStore
    host = ProfilePipeline()
    gpu = ProfilePipeline(device="cuda", stack_capacity=1 << 10)
    gpu.store = GpuProfileStore(device="cuda", stack_capacity=1 << 10,
                                row_capacity=64, pool_capacity=256)
    for b in range(5):
        lines = [f"batch{b % 3};frame_number_{(j * 3) % 70};"
                 f"a_rather_long_leaf_name_{b}_{j % 50} {j + 1}"
                 for j in range(100)]
        p = payload_of([msg("\n".join(lines).encode(), ts=1000 + b,
                            process=f"p{b % 2}")])
        host.ingest_payload(p)
        gpu.ingest_payload(p)
    assert gpu.store.row_capacity >= 500 > 64
    assert gpu.store.pool.numel() > 256
    assert gpu.store.n_rows == 500
    assert gpu.store.n_stacks == len(host.store.id_to_loc)
    assert row_tuples(gpu.store) == row_tuples(host.store)
    assert_same_flame(host, gpu)
    assert_same_flame(host, gpu, process_name="p1", time_start=1001,
                      time_end=1003)


def test_server_wiring():
    from deepflow_amd.server import DeepflowServer
    from deepflow_amd.store.profile_store import GpuProfileStore
    srv = DeepflowServer(device="cuda", tcp_port=0, segment_rows=1 << 9,
                         dict_capacity=1 << 10, gpu_profiles=True)
    assert type(srv.profiles.store) is GpuProfileStore
    payload = payload_of([msg(b"a;b 7\na;c 2", process="px", ts=50),
                          msg(b"a;b 1", process="py", ts=60)])
    frame = framing.encode_frame(
        framing.FrameHeader(msg_type=framing.MSG_PROFILE), payload)
    assert srv.receiver.handle_frame(frame)
    client = TestClient(srv.app)
    assert client.get("/v1/profile/processes").json() == ["px", "py"]
    tree = client.get("/v1/profile/flame",
                      params={"process_name": "px"}).json()
    assert tree == {"name": "root", "value": 9, "self": 0, "children": [
        {"name": "a", "value": 9, "self": 0, "children": [
            {"name": "b", "value": 7, "self": 7, "children": []},
            {"name": "c", "value": 2, "self": 2, "children": []}]}]}
    assert client.get("/v1/profile/flame",
                      params={"time_start": 60,
                              "time_end": 60}).json()["value"] == 1
    r = srv.mcp.handle({"jsonrpc": "2.0", "id": 1, "method": "tools/call",
                        "params": {"name": "profile_analysis",
                                   "arguments": {}}})
    assert r["result"]["content"][0]["text"].splitlines()[0] \
        == "total samples: 10"
    # the GPU profilers add samples one verbatim stack at a time
    srv.profiles._add(70, b"gpu;kern", 5, dict(
        event_type=9, pid=1, tid=0, pod_id=0, process_name="pz",
        app_service="gpu", profile_language_type="roctracer"))
    assert srv.profiles.flame(process_name="pz")["value"] == 5
    default = DeepflowServer(device="cuda", tcp_port=0,
                             segment_rows=1 << 9, dict_capacity=1 << 10)
    assert type(default.profiles.store) is ProfileStore
