"""K10 kernels (ops/csrc/dftrace.hip) against the host twin on identical
ingested data (-m gpu). Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracemap_cases as C  # noqa: E402

from deepflow_amd.ingest import L7IngestPipeline  # noqa: E402
from deepflow_amd.query import QueryEngine  # noqa: E402
from deepflow_amd.query import tracemap as TM  # noqa: E402
from deepflow_amd.query.tracing import DistributedTracer  # noqa: E402

LINK_KEYS = ("row", "trace_key", "parent_row", "link_kind", "depth")


def _mappers(demote: bool):
    assert torch.cuda.is_available()
    payloads = C.payloads_of(C.build_spans())
    out = {}
    for dev in ("cpu", "cuda"):
        p = L7IngestPipeline(device=dev, segment_rows=1 << 8,
                             dict_capacity=1 << 12)
        for payload in payloads:
            p.ingest_frame_payload(payload)
        if demote:
            assert p.segments.demote_oldest()
        out[dev] = TM.TraceMapper(QueryEngine(p, device=dev))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def mappers():
    return _mappers(demote=False)


@pytest.fixture(scope="module")
def host_ref(mappers):
    # computed once, shared, never modified
    return mappers["cpu"].link_spans(), mappers["cpu"].trace_map()


def assert_same_links(a, b):
    for k in LINK_KEYS:
        assert a[k].dtype == b[k].dtype, k
        assert np.array_equal(a[k], b[k]), k
    assert b["drops"] == 0


def test_max_hops_constant_is_shared():
    from deepflow_amd.ops import native
    assert native.gpu().df_trace_max_hops() == TM.MAX_TRACE_HOPS


def test_link_spans_equal_host(mappers, host_ref):
    got = mappers["cuda"].link_spans()
    assert len(got["row"]) > 1400 and len(got["row"]) % 64
    assert_same_links(host_ref[0], got)
    assert set(got["link_kind"].tolist()) == {0, 1, 2, 3}
    assert (got["depth"] == -1).sum() == 3 and got["depth"].max() == 47


def test_trace_map_equal_host(mappers, host_ref):
    got = mappers["cuda"].trace_map()
    assert got["drops"] == 0
    assert got == host_ref[1]
    assert got["trace_count"] > 60 and len(got["edges"]) > 30


@pytest.mark.parametrize("window", [
    dict(time_start=C.WINDOW_LO),
    dict(time_start=C.T0 + 20 * C.MS, time_end=C.T0 + 400 * C.MS),
    dict(time_start=C.T_SINGLE_START, time_end=C.T_SINGLE_START),
    dict(time_end=C.T0 - 20_000 * C.MS),
])
def test_window_equal_host(mappers, window):
    want = mappers["cpu"].trace_map(**window)
    got = mappers["cuda"].trace_map(**window)
    assert got == want
    assert_same_links(mappers["cpu"].link_spans(**window),
                      mappers["cuda"].link_spans(**window))
    if window == dict(time_start=C.WINDOW_LO):
        t = {x["trace_id"]: x for x in got["traces"]}[C.T_WINDOW]
        assert (t["span_count"], t["root_count"], t["root_service"]) == \
            (2, 1, "cart")


def test_cold_tier_equal_host(host_ref):
    """One segment arrives through materialize(); links cross from it into
    the hot segments."""
    m = _mappers(demote=True)
    for dev in ("cpu", "cuda"):
        assert len(m[dev].engine.pipe.segments.cold) == 1
    got = m["cuda"].link_spans()
    assert_same_links(host_ref[0], got)
    assert m["cuda"].trace_map() == host_ref[1]
    assert not getattr(m["cuda"].engine.pipe.segments, "_scratch", [])


def test_build_trace_trees_on_gpu(mappers, host_ref):
    eng = mappers["cuda"].engine
    tracer = DistributedTracer(eng)
    eng.trace_tree_rows = lambda: tracer.tree_rows
    tracer.build_trace_trees()
    tracer.build_trace_trees()
    r = eng.query("SELECT trace_id, span_count, max_depth FROM trace_tree "
                  "LIMIT 10000")
    want = sorted((t["trace_id"], t["span_count"], t["max_depth"])
                  for t in host_ref[1]["traces"])
    assert sorted(map(tuple, r["values"])) == want


def _ws_from_flat(f, parent=None, kind=None, depth=None):
    """Device workspace holding the host flat columns `f` (kernel-level
    tests: no segments involved)."""
    ws = TM._GpuWorkspace(f.n, torch.device("cuda"))
    i64 = lambda a: torch.from_numpy(a.astype(np.uint64).view(np.int64))
    ws.tkey.copy_(i64(f.tkey))
    ws.start.copy_(i64(f.start))
    ws.end.copy_(i64(f.end))
    ws.svc.copy_(torch.from_numpy(f.svc.astype(np.uint32).view(np.int32)))
    ws.status.copy_(torch.from_numpy(f.status))
    if parent is not None:
        ws.parent.copy_(torch.from_numpy(parent.astype(np.int32)))
        ws.kind.copy_(torch.from_numpy(kind))
        ws.depth.copy_(torch.from_numpy(depth))
    return ws


class _F:
    pass


def test_depth_bound_on_device():
    """Chain of MAX_TRACE_HOPS + 2 rows plus a 2-cycle: depth
    MAX_TRACE_HOPS is still rooted, one more hop is not."""
    from deepflow_amd.ops import gpu_ops
    n = TM.MAX_TRACE_HOPS + 4
    parent = np.arange(-1, n - 1, dtype=np.int64)
    parent[n - 2], parent[n - 1] = n - 1, n - 2
    f = _F()
    f.n = n
    f.tkey = np.full(n, 9, np.uint64)
    f.tkey[5] = 0                       # a row that takes no part: skipped
    f.start = f.end = np.zeros(n, np.uint64)
    f.svc, f.status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    ws = _ws_from_flat(f, parent, np.zeros(n, np.uint8),
                       np.full(n, 77, np.int32))
    gpu_ops.trace_depth(ws)
    torch.cuda.synchronize()
    got = ws.depth.cpu().numpy()
    want = np.arange(n, dtype=np.int32)
    want[TM.MAX_TRACE_HOPS + 1:] = -1
    want[5] = 77
    assert np.array_equal(got, want)


def test_fold_many_edges_many_blocks():
    """More distinct edges in one block than its LDS table holds (the rest
    go straight to the global table), several blocks, a ragged tail, and
    the (0, 0) and (invalid, invalid) service pairs."""
    from deepflow_amd.ops import gpu_ops
    rng = np.random.default_rng(10)
    n = 3 * 4096 + 77
    f = _F()
    f.n = n
    f.tkey = rng.integers(1, 400, n).astype(np.uint64)
    f.tkey[rng.random(n) < 0.05] = 0
    f.start = rng.integers(1, 1 << 40, n).astype(np.uint64)
    f.end = (f.start.astype(np.int64) +
             rng.integers(-5, 1 << 20, n)).astype(np.uint64)
    svc = rng.integers(0, 48, n).astype(np.uint32)
    svc[rng.random(n) < 0.1] = 0xFFFFFFFF
    f.svc = svc
    f.status = rng.integers(0, 6, n).astype(np.uint8)
    rows = np.nonzero(f.tkey)[0]
    # any participating earlier row serves as a parent here: the fold only
    # reads the link arrays
    parent = np.full(n, -1, np.int64)
    pick = rows[(rng.random(len(rows)) * np.arange(len(rows))).astype(int)]
    linked = rng.random(len(rows)) < 0.8
    linked[0] = False
    parent[rows[linked]] = pick[linked]
    kind = np.zeros(n, np.uint8)
    kind[rows[linked]] = rng.integers(1, 4, int(linked.sum()))
    depth = rng.integers(-1, 60, n).astype(np.int32)
    depth[parent < 0] = 0
    ws = _ws_from_flat(f, parent, kind, depth)
    gpu_ops.trace_fold(ws)
    torch.cuda.synchronize()
    tk, tv, root, rinfo, esvc, ev, drops = TM.TraceMapper._read_gpu_tables(ws)
    wtk, wtv, wesvc, wev = TM._host_fold(f, rows, parent, kind, depth)
    assert drops == 0
    assert len(wesvc) > 2000
    o, wo = np.argsort(tk), np.argsort(wtk)
    assert np.array_equal(tk[o], wtk[wo])
    assert np.array_equal(tv[o], wtv[wo])
    got_e = {tuple(k): v for k, v in zip(esvc.tolist(), ev.tolist())}
    want_e = {tuple(k): v for k, v in zip(wesvc.tolist(), wev.tolist())}
    assert got_e == want_e
    assert (0, 0) in got_e and (0xFFFFFFFF, 0xFFFFFFFF) in got_e


def test_undersized_tables_count_drops():
    """Bounded probing: a table smaller than its key set loses rows to
    `drops` and terminates; nothing waits for a free slot."""
    from deepflow_amd.ops import gpu_ops
    n = 1000
    f = _F()
    f.n = n
    f.tkey = np.arange(1, n + 1, dtype=np.uint64)     # every row a trace
    f.start = f.end = np.ones(n, np.uint64)
    f.svc, f.status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    ws = _ws_from_flat(f, np.full(n, -1, np.int64), np.zeros(n, np.uint8),
                       np.zeros(n, np.int32))
    ws.tkeys = ws.tkeys[:64].contiguous()
    ws.tvals = ws.tvals[:64].contiguous()
    gpu_ops.trace_fold(ws)
    torch.cuda.synchronize()
    assert int((ws.tkeys != 0).sum()) == 64
    assert int(ws.drops.item()) == n - 64
    assert int(ws.tvals[:, TM.TV_SPANS].sum()) == 64
