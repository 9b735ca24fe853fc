"""Interval flush on the CPU path: the archive/settle state machine that
the GPU path shares, with the plain-dict tables as the oracle."""
import dataclasses

import pytest

from deepflow_amd.gen import SpanGenConfig
from deepflow_amd.gen.spans import gen_span_payload
from deepflow_amd.ingest import L7IngestPipeline
from deepflow_amd.store.metrics import RollupFamily, RollupTable, TableDef

CFG = SpanGenConfig(n=1000, seed=77, tag_cardinality=500, n_attrs=4,
                    n_ips=256, n_services=16, n_resources=100)
APP_TABLES = ("application.1s", "application.1m", "application_map.1s",
              "application_map.1m")
TD = TableDef("t.drain", "doc", 1, ("vtap_id", "x"), "app", 0)


def _pipe():
    return L7IngestPipeline(device="cpu", segment_rows=1 << 14,
                            dict_capacity=1 << 14,
                            time_base_s=CFG.base_time_ns // 10**9)


@pytest.fixture(scope="module")
def pipes():
    """a: flush threshold 1500 (fires after batch 2, batch 3 follows);
    b: never flushed. Same three batches."""
    a, b = _pipe(), _pipe()
    a.rollups.FLUSH_EVERY_ROWS = 1500
    for i in range(3):
        payload = gen_span_payload(dataclasses.replace(CFG,
                                                       seed=CFG.seed + i))
        a.ingest_frame_payload(payload)
        b.ingest_frame_payload(payload)
    return a, b


def test_flush_mid_ingest_reads_like_no_flush(pipes):
    a, b = pipes
    assert a.rollups._rows_since_flush == CFG.n
    assert len(a.metrics.archive) == 1 and len(b.metrics.archive) == 0
    assert len(a.metrics.table) < len(b.metrics.table)
    for name in APP_TABLES:
        ra = a.rollups.get(name).rows()
        assert ra == b.rollups.get(name).rows(), name
    assert sum(r["request"] for r in a.metrics.rows()) == 3 * CFG.n


def test_double_flush_then_read(pipes):
    shared, b = pipes
    want = {name: b.rollups.get(name).rows() for name in APP_TABLES}
    a = _pipe()                  # a copy: the shared pipelines stay as built
    a.rollups.load_state_dict(shared.rollups.state_dict())
    assert len(a.metrics.archive) == 1 and a.metrics.table
    a.rollups.flush()
    assert len(a.metrics.archive) == 2 and not a.metrics.table
    a.rollups.flush()            # nothing live: no empty chunk
    assert len(a.metrics.archive) == 2
    for name in APP_TABLES:
        assert a.rollups.get(name).rows() == want[name], name


def test_settle_is_a_noop_on_the_cpu():
    fam = RollupFamily([TD], 0, device="cpu")
    t = fam.get(TD.name)
    key = (3, 9, 42)
    t.insert([key], [[5, 0, 0, 0, 0, 0, 0]])
    assert t.settle() is None and fam.settle() is None
    assert t.flush_live() == 1   # the CPU flush still reports its groups
    assert t.settle() is None and fam.settle() is None
    t.insert([key], [[7, 0, 0, 0, 0, 0, 0]])
    rows = t.rows()
    assert len(rows) == 1 and rows[0]["request"] == 12
    assert t.table == {key: [7, 0, 0, 0, 0, 0, 0]}
    assert t.drop_count() == 0
    lone = RollupTable(TD, 0, device="cpu")
    assert lone.settle() is None and lone.flush_live() == 0


def test_archive_compacts_past_eight_chunks():
    t = RollupTable(TD, 0, device="cpu")
    for i in range(10):
        t.insert([(0, 1, i % 3)], [[1, 0, 0, 0, 0, 0, i]])
        t.flush_live()
    # the ninth chunk folds all nine into one merged chunk, the tenth
    # lands next to it
    assert len(t.archive) == 2
    rows = t.rows()
    assert [r["request"] for r in rows] == [4, 3, 3]
    assert [r["rrt_max"] for r in rows] == [9, 7, 8]
