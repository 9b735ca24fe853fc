"""CPU query engine vs the brute-force reference on the hand-built cases of
query_cases.py (the GPU twins are in test_query_kernels_gpu.py). Every
comparison is exact: the engine, the kernels and the reference all implement
the same u64 accumulators."""
import numpy as np
import pytest

import query_cases as QC
from deepflow_amd.ops.ref import mix64
from deepflow_amd.query import spec as Q
from deepflow_amd.query.executor import execute_agg_cpu, execute_select_cpu

AGG_CASES = QC.cpu_agg_cases()


def engine_agg(plan, segs, kg=None):
    out = {}
    for g in execute_agg_cpu(plan, segs, kg=kg):
        key = tuple(g["key"])
        assert key not in out
        out[key] = g["agg"]
    return out


def test_mix64_np_matches_scalar():
    rng = np.random.default_rng(1)
    z = rng.integers(0, 1 << 64, 500, dtype=np.uint64)
    z[:4] = [0, 1, (1 << 64) - 1, 1 << 63]
    assert QC.mix64_np(z).tolist() == [mix64(int(v)) for v in z]
    keys = z[:50]
    assert QC.group_hash_np(keys).tolist() == \
        [QC.group_hash((int(k),)) for k in keys]


@pytest.mark.parametrize("case", AGG_CASES, ids=lambda c: c.name)
def test_agg_engine_equals_reference(case):
    want = QC.ref_agg(case.plan, case.segs, case.kg)
    assert engine_agg(case.plan, case.segs, case.kg) == want
    if "want" in case.extra:           # hand-computed expectation
        assert want == case.extra["want"]
    if not case.name.startswith("cnf_dead"):
        assert want, "case selects nothing"


def test_dead_or_group_selects_nothing():
    plan = QC.cnf_plans()["dead_group"]
    assert QC.ref_agg(plan, [QC.cnf_segment()]) == {}


def test_source_cases_reach_their_edges():
    """The source case really holds the edge it is named after."""
    src = QC.sources_case()
    plans = QC.source_plans()
    ref = lambda name, kg=src.kg: QC.ref_agg(plans[name], src.segs, kg)
    assert (QC.M32,) in ref("attr_val_slot2") and len(ref("attr_val_slot2")) > 1
    assert list(ref("attr_val_slot9")) == [(QC.M32,)]
    assert (QC.M32,) in ref("did_minus_one")
    assert (0,) in ref("kg_side0_pod") and len(ref("kg_side0_pod")) > 2
    assert list(ref("kg_pod_nokg", None)) == [(0,)]
    assert (0,) in ref("str_hash_user_agent")          # zero-length string
    assert (0,) in ref("trace128_trace")               # both fallbacks empty
    assert (0,) in ref("trace128_span")
    assert (0,) in ref("time_bucket_60")               # before the time base
    aggs = ref("keyless_eight_aggs")[()]
    # COUNT, SUM, MIN incl. 0, MAX incl. 2^64-1, MAX and MIN of all zeros
    assert aggs[0] == 1000 and aggs[2] == 0 and aggs[3] == QC.M64
    assert aggs[4] == 0 and aggs[5] == 0
    assert len(ref("four_keys_eight_aggs")) > 8


@pytest.mark.parametrize("family", list(QC.FILTER_FAMILIES),
                         ids=["u64", "u32", "u8", "did"])
def test_filter_matrix_engine_equals_reference(family):
    seg = QC.filter_segment()
    nonempty = 0
    for term in QC.filter_terms(family):
        sel = QC.plan([term])
        want = QC.ref_select(sel, seg)
        got = execute_select_cpu(sel, [seg], limit=10**9)
        assert {r for _, r in got} == want and len(got) == len(want), term
        cnt = engine_agg(QC.plan([term], [], [QC.COUNT]), [seg])
        assert cnt == ({(): [len(want)]} if want else {}), term
        if term.op == Q.OP_BETWEEN and term.v0 > term.v1:
            assert not want, term
        nonempty += bool(want)
    assert nonempty > 30


def test_select_engine_equals_reference():
    seg = QC.select_segment()
    plan = QC.select_plan()
    want = QC.ref_select(plan, seg)
    assert 100 < len(want) < 400
    got = execute_select_cpu(plan, [seg, seg], limit=10**9)
    assert got == [(si, r) for si in (0, 1) for r in sorted(want)]
