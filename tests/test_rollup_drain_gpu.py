"""GPU interval flush: k_rollup_drain directly at the wave64 edges of its
ballot compaction, and the queue-a-drain / settle state machine of
RollupTable and RollupFamily against never-flushed and CPU pipelines.
Requires an MI355X (run with -m gpu)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deepflow_amd.gen import SpanGenConfig
from deepflow_amd.gen.spans import gen_span_payload
from deepflow_amd.ingest import L7IngestPipeline
from deepflow_amd.store.kg import KnowledgeGraphTable, default_platform
from deepflow_amd.store.metrics import (APP_OPS, RU_MAX_KEYS, RollupFamily,
                                        RollupTable, TableDef)

# 2 keys + the time word: nw = 3; app aggregation: nv = 7
TD = TableDef("t.drain", "doc", 1, ("vtap_id", "x"), "app", 0)
APP_TABLES = ("application.1s", "application.1m", "application_map.1s",
              "application_map.1m")


def _table(cap):
    assert torch.cuda.is_available(), "GPU required"
    return RollupTable(TD, 0, device="cuda", capacity_pow2=cap)


def _fill(t, g):
    """g distinct keys, each with its own values, through rollup_insert."""
    if g == 0:
        return
    from deepflow_amd.ops import gpu_ops
    i = np.arange(g, dtype=np.int64)
    kws = np.stack((i % 5, i + 1, 1000 + 7 * i), axis=1)
    vals = np.stack([i * (v + 1) + v for v in range(t.nv)], axis=1)
    gpu_ops.rollup_insert(torch.from_numpy(kws).cuda(),
                          torch.from_numpy(vals).cuda(),
                          torch.tensor(APP_OPS, dtype=torch.uint8,
                                       device="cuda"), t)


def _sorted(keys, vals):
    order = np.lexsort(keys.T[::-1])
    return keys[order], vals[order]


def _assert_pristine(t):
    assert int(torch.count_nonzero(t.tkeys)) == 0
    assert int(torch.count_nonzero(t.tvals)) == 0
    assert t.traw.shape[1] == RU_MAX_KEYS
    assert bool((t.traw == -1).all())
    assert int(t.drops.item()) == 0


@pytest.mark.parametrize("g", [0, 1, 63, 64, 65, 700])
def test_drain_kernel_packs_and_resets(g):
    from deepflow_amd.ops import gpu_ops
    t = _table(1 << 10)
    _fill(t, g)
    want_k, want_v = _sorted(*t._harvest_np())
    assert want_k.shape[0] == g  # distinct keys, nothing dropped
    out_k = torch.full((t.capacity, t.nw), -7, dtype=torch.int64,
                       device="cuda")
    out_v = torch.full((t.capacity, t.nv), -7, dtype=torch.int64,
                       device="cuda")
    hdr = torch.zeros(2, dtype=torch.int64, device="cuda")
    gpu_ops.rollup_drain(t, out_k, out_v, hdr)
    hdr = hdr.cpu()
    assert int(hdr[0]) == g and int(hdr[1]) == 0
    got_k, got_v = _sorted(out_k[:g].cpu().numpy().view(np.uint64),
                           out_v[:g].cpu().numpy().view(np.uint64))
    assert np.array_equal(got_k, want_k)
    assert np.array_equal(got_v, want_v)
    # nothing written past the packed rows
    assert bool((out_k[g:] == -7).all()) and bool((out_v[g:] == -7).all())
    _assert_pristine(t)


def test_drain_rejects_bad_shapes():
    from deepflow_amd.ops import native
    lib = native.gpu()
    t = _table(1 << 6)
    args = (t.tkeys.data_ptr(), t.traw.data_ptr(), t.tvals.data_ptr(),
            t.drops.data_ptr())
    tail = (t._out_keys.data_ptr(), t._out_vals.data_ptr(),
            t._hdr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert lib.df_rollup_drain(*args, 48, t.nw, t.nv, *tail) != 0
    assert lib.df_rollup_drain(*args, 0, t.nw, t.nv, *tail) != 0
    assert lib.df_rollup_drain(*args, 64, RU_MAX_KEYS + 1, t.nv, *tail) != 0
    torch.cuda.synchronize()
    _assert_pristine(t)


def test_saturated_table_drains_its_drop_counter():
    t = _table(1 << 6)
    _fill(t, 200)
    drops = int(t.drops.item())
    assert drops > 0
    live = t._harvest_np()[0].shape[0]
    assert t.flush_live() == 0
    t.settle()
    assert t._hdr.cpu().tolist() == [live, drops]
    assert t.drop_count() == drops
    assert len(t.archive) == 1 and t.archive[0][0].shape[0] == live
    _assert_pristine(t)
    # nothing live, nothing dropped since: an empty drain
    t.flush_live()
    t.settle()
    assert t._hdr.cpu().tolist() == [0, 0]
    assert len(t.archive) == 1
    assert t.drop_count() == drops


def test_insert_right_behind_flush_lands_in_the_reset_table():
    """Stream order: the drain sits between the two inserts, so the first
    value is archived, the second is live, and a read merges them."""
    fam = RollupFamily([TD], 0, device="cuda")
    t = fam.get(TD.name)
    key = (3, 9, 42)
    t.insert([key], [[5, 0, 0, 0, 0, 0, 0]])
    fam.flush()
    t.insert([key], [[7, 0, 0, 0, 0, 0, 0]])
    rows = t.rows()
    assert len(rows) == 1 and rows[0]["request"] == 12
    assert rows[0]["vtap_id"] == 9 and rows[0]["x"] == 42
    lk, lv = t._harvest_np()
    assert lk.shape[0] == 1 and lk[0].tolist() == list(key)
    assert int(lv[0, 0]) == 7
    assert len(t.archive) == 1 and int(t.archive[0][1][0, 0]) == 5


# ------------------------------------------------------------- pipelines
CFG = SpanGenConfig(n=2000, seed=77, tag_cardinality=500, n_attrs=4,
                    n_ips=256, n_services=16, n_resources=100,
                    ip6_rate_pct=15)


def _pipe(device, flush_every=None):
    kg = KnowledgeGraphTable(capacity_pow2=1 << 12, device=device)
    kg.update(default_platform(CFG))
    p = L7IngestPipeline(device=device, segment_rows=1 << 14, kg=kg,
                         dict_capacity=1 << 14,
                         time_base_s=CFG.base_time_ns // 10**9)
    if flush_every is not None:
        p.rollups.FLUSH_EVERY_ROWS = flush_every
    return p


@pytest.fixture(scope="module")
def batches():
    import dataclasses
    return [gen_span_payload(dataclasses.replace(CFG, seed=CFG.seed + i))
            for i in range(3)]


@pytest.fixture(scope="module")
def cpu_rows(batches):
    """Rows of the CPU pipeline over all three batches (computed once)."""
    c = _pipe("cpu")
    for b in batches:
        c.ingest_frame_payload(b)
    return {name: c.rollups.get(name).rows() for name in APP_TABLES}


def test_flush_mid_ingest_reads_like_no_flush_and_like_cpu(batches, cpu_rows):
    a = _pipe("cuda", flush_every=3000)  # fires at the end of batch 2
    b = _pipe("cuda")
    for payload in batches:
        a.ingest_frame_payload(payload)  # batch 3 runs behind the drain
        b.ingest_frame_payload(payload)
    assert a.rollups._rows_since_flush == CFG.n
    assert b.rollups._rows_since_flush == 3 * CFG.n
    for name in APP_TABLES:
        ra = a.rollups.get(name).rows()
        assert ra == b.rollups.get(name).rows(), name
        assert ra == cpu_rows[name], name
    assert len(a.metrics.archive) == 1 and len(b.metrics.archive) == 0
    assert sum(r["request"] for r in cpu_rows["application.1s"]) == 3 * CFG.n


def test_every_read_path_settles(batches):
    """Each read below is the first thing to touch its pipeline after the
    ingest that queued the drain: no explicit settle anywhere."""
    live = ("application.1s", "application_map.1s")
    # drop_count: the counter moved from the device into dropped_total
    a = _pipe("cuda", flush_every=3000)
    a.ingest_frame_payload(batches[0])
    drops0 = {n: a.rollups.get(n).drop_count() for n in live}
    a.ingest_frame_payload(batches[1])   # triggers the flush
    for n in live:
        assert a.rollups.get(n).drop_count() == drops0[n], n
    # state_dict: the drained groups are in the archive, the table is empty
    b = _pipe("cuda", flush_every=3000)
    b.ingest_frame_payload(batches[0])
    b.ingest_frame_payload(batches[1])
    sd = b.rollups.state_dict()
    for n in live:
        (keys, vals), = sd[n]["archive"]
        assert keys.shape[0] > 0
        assert int(vals[:, 0].sum()) == 2 * CFG.n, n  # one request a span
        assert int(torch.count_nonzero(sd[n]["tkeys"])) == 0, n
    # load_state_dict into a fresh pipeline reads back what was saved
    c = _pipe("cuda")
    c.rollups.load_state_dict(sd)
    # ... and so does one that has a drain of other rows queued
    d = _pipe("cuda", flush_every=3000)
    d.ingest_frame_payload(batches[2])
    d.ingest_frame_payload(batches[2])
    d.rollups.load_state_dict(sd)
    for n in APP_TABLES:
        want = b.rollups.get(n).rows()
        assert want == a.rollups.get(n).rows(), n
        assert want == c.rollups.get(n).rows(), n
        assert want == d.rollups.get(n).rows(), n
