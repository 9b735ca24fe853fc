"""K12 kernels (ops/csrc/dfflow.hip) against the host twin on identical
ingested data, and kernel by kernel from flat arrays (-m gpu). Every
comparison is exact: a group id is the lowest row of its group."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowgroup_cases as C  # noqa: E402

from deepflow_amd.ingest import L7IngestPipeline  # noqa: E402
from deepflow_amd.query import QueryEngine  # noqa: E402
from deepflow_amd.query import flowgroups as FG  # noqa: E402

LINK_KEYS = ("row", "group", "via")
N_BIG = 3 * 4096 + 77       # several blocks and a ragged tail


def _groupers(demote: bool):
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
        out[dev] = FG.FlowGrouper(QueryEngine(p, device=dev))
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def groupers():
    return _groupers(demote=False)


@pytest.fixture(scope="module")
def host_ref(groupers):
    # computed once, shared, never modified
    return (groupers["cpu"].link_groups(),
            groupers["cpu"].flow_groups(min_spans=1))


def assert_same_links(a, b):
    for k in LINK_KEYS:
        assert a[k].dtype == b[k].dtype, k
        assert np.array_equal(a[k], b[k]), k
    assert b["drops"] == 0


def test_constants_are_shared():
    from deepflow_amd.ops import native
    lib = native.gpu()
    assert lib.df_flow_gv_n() == FG.GV_N
    assert lib.df_flow_rel_n() == FG.REL_N
    assert lib.df_flow_keys_per_row() == FG.KEYS_PER_ROW == len(FG._KEY_COLS)


def test_link_groups_equal_host(groupers, host_ref):
    got = groupers["cuda"].link_groups()
    assert len(got["row"]) > 1400 and len(got["row"]) % 64
    assert_same_links(host_ref[0], got)
    assert set(got["via"].tolist()) >= {0, 1, 2, 4, 8}
    sizes = np.bincount(got["group"])
    assert sizes.max() == C.STAR_LEN and (sizes == C.CHAIN_LEN).sum() == 1


def test_flow_groups_equal_host(groupers, host_ref):
    got = groupers["cuda"].flow_groups(min_spans=1)
    assert got["drops"] == 0
    assert got == host_ref[1]
    assert got["group_count"] > 100
    assert groupers["cuda"].flow_groups() == groupers["cpu"].flow_groups()


@pytest.mark.parametrize("window", [
    dict(time_start=C.WINDOW_LO),
    dict(time_start=C.T0 + 20 * C.MS, time_end=C.T0 + 400 * C.MS),
    dict(time_start=C.SINGLE_START, time_end=C.SINGLE_START),
    dict(time_end=C.T0 - 20_000 * C.MS),
])
def test_window_equal_host(groupers, window):
    want = groupers["cpu"].flow_groups(min_spans=1, **window)
    got = groupers["cuda"].flow_groups(min_spans=1, **window)
    assert got == want
    assert_same_links(groupers["cpu"].link_groups(**window),
                      groupers["cuda"].link_groups(**window))
    if window == dict(time_start=C.SINGLE_START, time_end=C.SINGLE_START):
        assert got["span_count"] == 1


def test_cold_tier_equal_host(host_ref):
    """One segment arrives through materialize(); groups cross from it
    into the hot segments."""
    m = _groupers(demote=True)
    for dev in ("cpu", "cuda"):
        assert len(m[dev].engine.pipe.segments.cold) == 1
    assert_same_links(host_ref[0], m["cuda"].link_groups())
    assert m["cuda"].flow_groups(min_spans=1) == host_ref[1]
    assert not getattr(m["cuda"].engine.pipe.segments, "_scratch", [])


def test_flow_trace_equal_host(groupers):
    for seed in (dict(trace_id=C.T_BRIDGE_B), dict(syscall_trace_id=102),
                 dict(x_request_id=C.X_HOP), dict(x_request_id="nobody"),
                 dict(x_request_id="star-request-id", limit=2)):
        want = groupers["cpu"].flow_trace(**seed)
        assert groupers["cuda"].flow_trace(**seed) == want
    assert want["span_count"] == C.STAR_LEN and want["truncated"]


# ------------------------------------------------ kernels from flat arrays
class _F:
    """Host flat columns (flowgroups._Flat's fields), all-zero keys."""

    def __init__(self, n):
        self.n = n
        self.part = np.ones(n, np.uint8)
        for c, _ in FG._KEY_COLS:
            setattr(self, c, np.zeros(n, np.uint64))
        self.start = np.ones(n, np.uint64)
        self.end = np.ones(n, np.uint64)
        self.status = np.zeros(n, np.uint8)


def _ws_from_flat(f):
    ws = FG._FlowWorkspace(f.n, torch.device("cuda"))
    for c in FG._FLAT_COLS:
        a = getattr(f, c)
        t = torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64))
        getattr(ws, c).copy_(t)
    return ws


def _union_on_device(ws):
    from deepflow_amd.ops import gpu_ops
    gpu_ops.flow_index(ws)
    gpu_ops.flow_union(ws)
    gpu_ops.flow_flatten(ws)
    torch.cuda.synchronize()
    return (ws.group.cpu().numpy().astype(np.int64) & 0xFFFFFFFF,
            ws.via.cpu().numpy())


def _check_against_host(f):
    rows, want_group, want_via = FG._host_union(f)
    ws = _ws_from_flat(f)
    group, via = _union_on_device(ws)
    assert int(ws.drops.item()) == 0
    assert np.array_equal(group, want_group)
    assert np.array_equal(via, want_via)
    # a group id is the lowest row of its group
    first = np.full(f.n, f.n, np.int64)
    np.minimum.at(first, group, np.arange(f.n))
    assert np.array_equal(first[group], group)
    return ws, rows, group, via


def test_chain_of_many_blocks():
    """Row i shares a key with row i + 1 only: one group, the deepest
    walks, every hook at a different root."""
    f = _F(N_BIG)
    i = np.arange(N_BIG, dtype=np.uint64)
    f.sresp = i + np.uint64(1000)                   # row i answers ...
    f.sreq = i + np.uint64(999)
    f.sreq[0] = 0
    _, _, group, via = _check_against_host(f)
    assert not group.any()
    assert via[0] == 0 and (via[1:] == 1 << FG.REL_SYSCALL).all()


def test_star_of_many_blocks():
    """Every row on one key: every thread hooks below one root."""
    f = _F(N_BIG)
    f.x1[:] = 0xABCDEF
    f.part[0] = 0                                   # the root is row 1
    _, _, group, via = _check_against_host(f)
    assert group[0] == 0 and (group[1:] == 1).all()
    assert (via[2:] == 1 << FG.REL_XREQ).all() and via[1] == 0


def test_random_keys_equal_host():
    rng = np.random.default_rng(12)
    f = _F(N_BIG)
    n = N_BIG

    def draw(pool, p):
        v = rng.integers(1, pool, n).astype(np.uint64)
        v[rng.random(n) >= p] = 0
        return v
    f.tkey = draw(n // 6, 0.4)
    f.sreq, f.sresp = draw(2 * n, 0.3), draw(2 * n, 0.3)
    f.tcp = draw(1 << 40, 0.1)
    # one value in every space: spaces must stay apart
    f.tcp[::97] = 5
    f.sreq[1::97] = 5
    f.x0, f.x1 = draw(3 * n, 0.2), draw(3 * n, 0.2)
    f.part[rng.random(n) < 0.05] = 0               # keys stay: ignored
    _, rows, group, via = _check_against_host(f)
    sizes = np.bincount(group[rows])
    assert (sizes > 0).sum() > 500 and sizes.max() > 20
    assert set(via[rows].tolist()) >= {0, 1, 2, 4, 8, 3}
    out = f.part == 0
    assert np.array_equal(group[out], np.nonzero(out)[0])
    assert not via[out].any()


def test_fold_equal_host():
    from deepflow_amd.ops import gpu_ops
    rng = np.random.default_rng(13)
    n = N_BIG
    f = _F(n)
    f.part[rng.random(n) < 0.05] = 0
    f.tkey = rng.integers(0, 3, n).astype(np.uint64)
    f.start = rng.integers(1, 1 << 40, n).astype(np.uint64)
    f.end = (f.start.astype(np.int64) +
             rng.integers(-5, 1 << 20, n)).astype(np.uint64)
    f.status = rng.integers(0, 6, n).astype(np.uint8)
    # the fold only reads the arrays: any row serves as a group id. A few
    # hundred groups of ~30 rows, one of ~2000, one at the last row
    group = rng.integers(0, 400, n).astype(np.int64)
    group[rng.random(n) < 0.15] = 7
    group[-1] = n - 1
    via = rng.integers(0, 16, n).astype(np.uint8)
    rows = np.nonzero(f.part)[0]
    ws = _ws_from_flat(f)
    ws.group.copy_(torch.from_numpy(group.astype(np.int32)))
    ws.via.copy_(torch.from_numpy(via))
    gpu_ops.flow_fold(ws)
    torch.cuda.synchronize()
    gid, gv, drops = FG.FlowGrouper._read_gpu_table(ws)
    want_gid, want_gv = FG._host_fold(f, rows, group, via)
    assert drops == 0 and len(want_gid) > 300
    assert gv.dtype == want_gv.dtype
    assert np.array_equal(gid, want_gid)
    assert np.array_equal(gv, want_gv)
    some_untraced = want_gv[:, FG.GV_FIRST_TRACED_ROW] == FG.U64MAX
    assert want_gv[:, FG.GV_SPANS].max() > 1500 and not some_untraced.all()


def test_undersized_index_counts_drops():
    """Bounded probing: an index smaller than its key set loses keys to
    `drops` and every launch terminates. Rows may then miss partners, but
    a row is only ever grouped with rows that share its key, below it."""
    n = 1000
    f = _F(n)
    g = np.arange(n, dtype=np.uint64)
    f.tkey = g // np.uint64(4) + np.uint64(1)       # shared by four rows
    f.sreq = g + np.uint64(10_000)                  # shared by nobody
    ws = _ws_from_flat(f)
    ws.idx_keys = ws.idx_keys[:64].contiguous()
    ws.idx_rows = ws.idx_rows[:64].contiguous()
    ws.idx_cap = 64
    group, via = _union_on_device(ws)
    assert int((ws.idx_keys != 0).sum()) == 64
    assert int(ws.drops.item()) > 0
    rows = np.arange(n)
    assert (group <= rows).all()
    assert np.array_equal(group // 4, rows // 4)
    assert (group != rows).any()
