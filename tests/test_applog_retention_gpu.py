"""Retention on the GPU application-log store (k_log_evict_plan and
k_log_evict in ops/csrc/dflog.hip) against the host AppLogPipeline fed the
same calls and the same evictions (-m gpu). Every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import applog_cases as C  # noqa: E402
import applog_retention_cases as R  # noqa: E402

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline  # noqa: E402
from deepflow_amd.ops import gpu_ops, native  # noqa: E402
from deepflow_amd.server import DeepflowServer  # noqa: E402
from deepflow_amd.store.dictionary import str_hash_py  # noqa: E402
from deepflow_amd.store.log_store import GpuLogStore, _pad16  # noqa: E402
from deepflow_amd.wire import framing  # noqa: E402


def gpu_of(calls, **kw):
    assert torch.cuda.is_available()
    pipe = AppLogPipeline(device="cuda", **kw)
    C.feed(pipe, calls)
    return pipe


def pair_of(calls, **kw):
    return R.host_of(calls), gpu_of(calls, **kw)


def same_search(host, gpu, substr="", **kw):
    kw.setdefault("limit", 10000)
    want = host.search(substr, **kw)
    assert gpu.search(substr, **kw) == want
    return want


def check_layout(store):
    """What the three scan kernels rely on."""
    n = store.n_rows
    assert store.pool.numel() % 16 == 0 and store.pool.data_ptr() % 16 == 0
    assert store.pool_len <= store.pool.numel()
    boff = store.row_boff[:n].cpu().numpy()
    blen = store.row_blen[:n].cpu().numpy()
    assert bool(np.all(boff[1:] >= boff[:-1]))
    assert bool(np.all(boff >= 0))
    assert bool(np.all(boff + blen <= store.pool_len))


# --------------------------------------------- 1. cut positions vs the host
@pytest.mark.parametrize("first", R.PARSE_FIRSTS)
def test_cut_positions_equal_the_host(first):
    host, gpu = pair_of(C.PARSE_CALLS)
    assert gpu.n_rows == R.N_PARSE
    assert gpu.evict_rows(first) == host.evict_rows(first) == first
    assert R.check_parse_pair(host, gpu) > 8
    check_layout(gpu.store)
    # OTLP extras stay on their rows
    by_body = {r["body"]: r for r in gpu.rows}
    if first <= 6:
        assert by_body["otlp body one"]["attr.k"] == "v"
        assert by_body["otlp body one"]["trace_id"] == "ab" * 16
    if first <= 9:
        assert by_body["another agent"]["attr.n"] == 5
        assert "attr.k" not in by_body["another agent"]
    assert all("attr.k" not in r for r in gpu.rows
               if r["body"] != "otlp body one")
    assert gpu.store.evictions == 1 and gpu.store.app_drops == 0
    assert gpu.counter.snapshot()["logs_evicted"] == first


# ------------------------------------------------------ 2. name relocation
def _colliding_apps(cap):
    """Two app names with the same home slot in a table of `cap`, and a
    third elsewhere."""
    seed = int(native.gpu().df_log_app_seed())
    home = {}
    for i in range(64):
        a = "app%d" % i
        home.setdefault(str_hash_py(a.encode(), seed) & (cap - 1),
                        []).append(a)
    pair = next(v for v in home.values() if len(v) >= 2)
    return pair[0], pair[1], seed


def test_name_of_an_evicted_claimer_moves_and_moves_again():
    cap = 4
    solo, other, seed = _colliding_apps(cap)
    calls = R.relocation_calls(solo, other)
    host, gpu = pair_of(calls, app_capacity=cap)
    st = gpu.store
    assert gpu.rows == host.rows and st.app_drops == 0
    slot = int(st.row_app[0])
    assert slot == str_hash_py(solo.encode(), seed) & (cap - 1)
    # `other` has the same home and came second: it was probed past it
    assert str_hash_py(other.encode(), seed) & (cap - 1) == slot
    assert int(st.row_app[1]) != slot
    others = [3, 2, 2]          # rows of `other` left after each eviction
    for step in range(3):               # from the pool, then from the arena
        assert gpu.evict_rows(1) == host.evict_rows(1) == 1
        rows = gpu.rows
        assert rows == host.rows
        assert rows[-1]["app_service"] == solo
        assert rows[-1]["app_id"] == 0
        assert int(st.row_app[st.n_rows - 1]) == slot   # ids are slots
        # the name lies in the arena, below the first body
        assert int(st.app_off[slot]) + len(solo) <= int(st.row_boff[0])
        check_layout(st)
        # hydration through search(), and the app filter
        assert gpu.search(limit=1)[0]["app_service"] == solo
        assert len(same_search(host, gpu, app_service=solo)) == 1
        assert len(same_search(host, gpu, app_service=other)) \
            == others[step]
        # the arena's bytes belong to no row: only the body that really
        # says the name matches it
        hit = same_search(host, gpu, solo)
        assert [r["time"] for r in hit] == [5]
        assert len(same_search(host, gpu, regex=solo)) == 1
        assert len(same_search(host, gpu, regex="^" + solo)) == 0
    assert st.n_apps == 3


def test_full_app_table_reads_back_unchanged_after_eviction():
    host, gpu = pair_of(R.FULL_TABLE_CALLS, app_capacity=2)
    assert gpu.store.app_drops == 3
    for n in (2, 1):
        assert gpu.evict_rows(n) == host.evict_rows(n) == n
        assert gpu.store.app_drops == 3
        got = gpu.rows
        assert len(got) == len(host.rows)
        for g, w in zip(got, host.rows):
            if w["app_service"] in ("a1", "a2"):
                assert g == w
            else:
                assert g == dict(w, app_service="", app_id=-1)
        same_search(host, gpu, app_service="a2")
        assert gpu.search(app_service="a3") == []
    assert {r["app_service"] for r in gpu.rows} == {"", "a2"}


# ------------------------------------------- 3. cut boundary and alignment
def test_cut_boundary_and_alignment():
    host, gpu = pair_of(R.CUT_CALLS)
    st = gpu.store
    end0 = int(st.row_boff[0]) + int(st.row_blen[0])
    assert end0 == R.CUT_END0 and end0 % 16 >= 3    # the cut gets rounded
    for needle in R.CUT_SPANNING:
        assert same_search(host, gpu, needle) == []
    assert gpu.evict_rows(1) == host.evict_rows(1) == 1
    check_layout(st)
    # the evicted body's last bytes are still in the pool, in front of the
    # first kept body, and still belong to no row
    lo = int(st.row_boff[0])
    head = bytes(st.pool[:lo].cpu().numpy())
    assert head.endswith(b"END\n1700000002 info appb ")
    for needle in R.CUT_SPANNING:
        assert same_search(host, gpu, needle) == []
    assert same_search(host, gpu, regex=r"END\s17") == []
    # the very start of the first kept body
    assert [r["time"] for r in same_search(host, gpu, R.CUT_HEAD)] == \
        [1700000002]
    assert len(same_search(host, gpu, regex="^" + R.CUT_HEAD)) == 1
    # the other row that says TAILEND is still found
    assert [r["app_service"] for r in same_search(host, gpu, "TAILEND")] \
        == ["appc"]
    assert gpu.rows == host.rows


# -------------------------------------------------------- 4. tile boundaries
def test_evictions_that_move_rows_across_tile_edges():
    lib = native.gpu()
    tile = int(lib.df_log_tile_bytes())
    overhang = int(lib.df_log_re_overhang())
    payload, plan = R.retention_tile_payload(tile, overhang)
    calls = [("lines", payload, 3, "system")]
    host, gpu = pair_of(calls)
    st = gpu.store
    assert gpu.n_rows == plan["rows"] and st.pool_len == len(payload)
    assert st.pool_len > 2 * tile
    walk = R.START + "=+" + R.END

    def start_of(row):      # pool offset of START in a planted long line
        return int(st.row_boff[row]) + 5

    def check(long_rows):
        check_layout(st)
        assert len(same_search(host, gpu, regex=walk)) == long_rows
        assert len(same_search(host, gpu, regex=walk + "$")) == long_rows
        assert len(same_search(host, gpu, regex=r"^\.+" + R.START)) \
            == long_rows
        assert len(same_search(host, gpu, R.START)) == long_rows
        assert len(same_search(host, gpu, R.END)) == long_rows
        # dense: every row of every tile, the ones on the new edges too
        assert len(same_search(host, gpu, ".")) == host.n_rows
        assert len(same_search(host, gpu, regex=r"\.")) == host.n_rows
        same_search(host, gpu, ".", limit=7, app_service="tile1")
        assert gpu.histogram(3, C.T0, C.T0 + 7, "..", regex=r"\.\.$") == \
            host.histogram(3, C.T0, C.T0 + 7, "..", regex=r"\.\.$") != []

    check(2)
    # 1: the first kept body starts mid-tile
    kept = int(st.row_boff[plan["first1"]])
    assert kept == plan["kept1_body"] and tile // 4 < kept < 3 * tile // 4
    n1 = plan["first1"]
    assert gpu.evict_rows(n1) == host.evict_rows(n1) == n1
    a = start_of(plan["row_a"] - n1)
    # long line A now starts below the first edge of the new pool and ends
    # beyond the bytes that tile's block stages
    assert tile - 210 < a < tile
    assert a + len(R.START) + overhang + 200 > tile + overhang
    check(2)
    # 2: the first kept body (A's) starts within 128 bytes of that edge
    n2 = plan["first2"]
    assert tile - 128 <= int(st.row_boff[n2]) < tile
    assert gpu.evict_rows(n2) == host.evict_rows(n2) == n2
    assert start_of(0) < 128                # A leads the new pool
    b = start_of(plan["row_b"] - n1 - n2)
    assert tile - 210 < b < tile
    check(2)
    assert gpu.rows == host.rows
    assert st.evictions == 2 and st.evicted_rows == n1 + n2


# ---------------------------------------------------- 5. ingest after evict
def test_ingest_and_eviction_interleaved_with_growth():
    host = AppLogPipeline()
    gpu = AppLogPipeline(device="cuda", row_capacity=4, pool_capacity=64)
    steps = [("feed", C.PARSE_CALLS[0]), ("evict", 3),
             ("feed", C.PARSE_CALLS[1]), ("evict", 5),
             ("feed", C.PARSE_CALLS[2]), ("evict", 1),
             ("feed", C.PARSE_CALLS[1])]
    for kind, arg in steps:
        if kind == "feed":
            assert C.feed(gpu, [arg]) == C.feed(host, [arg])
        else:
            assert gpu.evict_rows(arg) == host.evict_rows(arg) == arg
        R.check_parse_pair(host, gpu)
        check_layout(gpu.store)
    assert gpu.store.row_capacity > 4 and gpu.store.pool.numel() > 64
    assert gpu.n_rows == 2 + 13 - 1 + 4
    # extras were re-keyed with the rows they belong to
    assert [r.get("attr.n") for r in gpu.rows[:2]] == [5, None]
    assert gpu.rows[-4]["attr.k"] == "v"


# ------------------------------------------------------------- 6. row rule
def test_row_rule_equals_the_host():
    kw = {"max_rows": R.MAX_ROWS, "keep_fraction": R.KEEP}
    host = AppLogPipeline(**kw)
    gpu = AppLogPipeline(device="cuda", **kw)
    sizes = []
    for call in R.ROW_RULE_CALLS:
        sizes += C.feed(host, [call])
        C.feed(gpu, [call])
        assert (gpu.n_rows, gpu.evicted_rows) == \
            (host.n_rows, host.evicted_rows) == R.row_rule_model(sizes)[-1]
        assert gpu.rows == host.rows
        same_search(host, gpu, limit=3)
    assert gpu.evictions == host.evictions == 4
    assert gpu.counter.snapshot()["logs_evicted"] == gpu.evicted_rows


# ------------------------------------------------------------ 7. byte rule
def test_byte_rule_keeps_the_pool_under_its_budget():
    budget = R.BYTE_BUDGET
    gpu = AppLogPipeline(device="cuda", max_pool_bytes=budget,
                         pool_capacity=256, row_capacity=16)
    host = AppLogPipeline()                 # unbounded
    st = gpu.store
    for p in R.byte_rule_payloads():
        n_before, gone_before = gpu.n_rows, gpu.evicted_rows
        evictions = st.evictions
        host.ingest_lines(p, agent_id=2, now=C.NOW)
        gpu.ingest_lines(p, agent_id=2, now=C.NOW)
        assert st.pool_len <= budget
        assert st.pool.numel() <= _pad16(budget)
        check_layout(st)
        assert gpu.n_rows + gpu.evicted_rows == host.n_rows
        assert gpu.rows == host.rows[host.n_rows - gpu.n_rows:]
        if st.evictions > evictions:
            # room is made before the batch goes in: of the rows that were
            # there, at least one survived
            assert st.evictions == evictions + 1
            assert 0 < gpu.evicted_rows - gone_before < n_before
            # down to keep_fraction of the budget, then the batch
            assert st.pool_len <= int(budget * 0.5) + len(p)
    assert st.evictions >= 2
    assert st.app_drops == 0 and st.n_apps == 6
    same_search(host, gpu, "payload 23")
    assert gpu.search("payload 0 ") == []           # long gone
    # a batch that cannot fit: refused, nothing changes
    rows = gpu.rows
    state = (st.n_rows, st.pool_len, st.evictions)
    with pytest.raises(ValueError):
        gpu.ingest_lines(b"1 info big " + b"y" * budget, now=C.NOW)
    assert (st.n_rows, st.pool_len, st.evictions) == state
    assert gpu.rows == rows
    stats = gpu.stats()
    assert stats["max_pool_bytes"] == budget
    assert stats["pool_bytes"] == st.pool_len


def test_byte_rule_arguments():
    with pytest.raises(ValueError):
        GpuLogStore(max_pool_bytes=(1 << 32) + 1)
    with pytest.raises(ValueError):
        GpuLogStore(max_pool_bytes=0)
    with pytest.raises(ValueError):
        GpuLogStore(keep_fraction=0.0)
    st = GpuLogStore(max_pool_bytes=100)
    assert st.pool.numel() == _pad16(100)


def test_server_ingests_past_its_byte_budget():
    srv = DeepflowServer(device="cuda", tcp_port=0, segment_rows=1 << 10,
                         dict_capacity=1 << 12, gpu_logs=True,
                         log_max_pool_bytes=R.BYTE_BUDGET)
    total = 0
    for p in R.byte_rule_payloads():
        frame = framing.encode_frame(
            framing.FrameHeader(msg_type=framing.MSG_APPLICATION_LOG,
                                agent_id=6), p)
        assert srv.receiver.handle_frame(frame)
        total += len(p.splitlines())
    from fastapi.testclient import TestClient
    dbg = TestClient(srv.app).get("/v1/debug/store").json()
    assert dbg["log_rows"] + dbg["log_evicted_rows"] == total
    assert 0 < dbg["log_pool_bytes"] <= R.BYTE_BUDGET
    assert dbg["log_evicted_rows"] > 0


# ---------------------------------------------------------- 8. evict_before
@pytest.mark.parametrize("t, gone", R.BEFORE_CASES)
def test_evict_before_equals_the_host(t, gone):
    host, gpu = pair_of(R.BEFORE_CALLS)
    assert gpu.evict_before(t) == host.evict_before(t) == gone
    assert gpu.rows == host.rows
    assert [r["time"] for r in gpu.rows] == R.BEFORE_TIMES[gone:]
    assert gpu.evict_before(t) == 0         # nothing more to take


# -------------------------------------------------- 9. gpu_ops.log_evict
def test_log_evict_of_every_row_leaves_the_arena_only():
    host, gpu = pair_of(C.SCAN_CALLS)
    st = gpu.store
    n = st.n_rows
    names = sorted({r["app_service"] for r in host.rows})
    st._dense_ids()                         # host-side state is the caller's
    for bad in (0, n + 1, -1):
        with pytest.raises(ValueError):
            gpu_ops.log_evict(st, bad)
    cut, arena = gpu_ops.log_evict(st, n)
    st._dense_rows = 0
    assert cut > 0 and st.n_rows == 0
    packed = sum(len(a.encode()) for a in names)
    assert arena == _pad16(packed) and st.pool_len == arena
    check_layout(st)
    # every name is in the arena, at its slot's offset
    pool = bytes(st.pool[:arena].cpu().numpy())
    live = torch.nonzero(st.tkeys).reshape(-1).tolist()
    got = sorted(pool[int(st.app_off[s]):int(st.app_off[s])
                      + int(st.app_len[s])].decode() for s in live)
    assert got == names
    assert gpu.search() == [] and gpu.search("alpha") == []
    assert gpu.rows == []
    # ingest and search go on; apps keep the ids they had
    ids = {r["app_service"]: r["app_id"] for r in host.rows}
    C.feed(gpu, C.SCAN_CALLS[1:])
    fresh = R.host_of(C.SCAN_CALLS[1:])
    want = [dict(r, app_id=ids[r["app_service"]]) for r in fresh.rows]
    assert gpu.rows == want
    assert gpu.search("pool-end") == [want[-1]]
    assert gpu.search("alpha") == []        # the arena says it, no body does
    assert gpu.search(regex="^alpha") == []
    check_layout(st)
