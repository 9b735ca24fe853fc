"""K15 k_query_uniq called directly (gpu_ops.query_uniq) on the hand-built
cases of uniq_cases.py against its brute-force reference, then the GPU
executor and engine against the CPU ones. The table sizes, base_row and n
are chosen by the test; every comparison is of exact integers, as dicts
(slot order is undefined)."""
import ctypes as ct

import numpy as np
import pytest
import torch

import query_cases as QC
import uniq_cases as UC
from deepflow_amd.query import executor as EX
from deepflow_amd.query import spec as Q

pytestmark = pytest.mark.gpu

GUARD = -7


def new_tables(cap=1024, pcap=1 << 14):
    """Fresh group table, counters and pair table; one guard word sits
    behind the pair words."""
    z = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    pbuf = torch.full((pcap + 1,), GUARD, dtype=torch.int64, device="cuda")
    pbuf[:pcap] = 0
    return {"gkeys": z(cap), "graw": z(cap, Q.QMAX_KEYS),
            "guniq": z(cap, Q.QMAX_UNIQ), "pbuf": pbuf, "pcap": pcap,
            "overflow": torch.zeros(2, dtype=torch.int32, device="cuda")}


def run_uniq(seg, plan, t, base_row=0, n=None, kg=None, use_filter=True):
    from deepflow_amd.ops import gpu_ops
    n = seg.n_rows - base_row if n is None else n
    gpu_ops.query_uniq(seg, plan.to_bytes(), plan.uniq_to_bytes(), base_row,
                       n, t["gkeys"], t["graw"], t["guniq"],
                       t["pbuf"][:t["pcap"]], kg=kg, overflow=t["overflow"],
                       use_filter=use_filter)
    torch.cuda.synchronize()
    assert int(t["pbuf"][t["pcap"]].item()) == GUARD
    return t


def lost(t):
    return [int(x) & 0xFFFFFFFF for x in t["overflow"].tolist()]


def uniq_dict(t, plan):
    live = t["gkeys"] != 0
    # no count outside a live group slot, none in an unused item column
    assert int(t["guniq"][~live].abs().sum().item()) == 0
    assert int(t["guniq"][:, len(plan.uniqs):].abs().sum().item()) == 0
    raw = t["graw"][live].cpu().numpy().view(np.uint64)[:, :len(plan.keys)]
    cnt = t["guniq"][live].cpu()[:, :len(plan.uniqs)]
    out = {}
    for k, v in zip(raw.tolist(), cnt.tolist()):
        assert tuple(k) not in out, "one group in two slots"
        out[tuple(k)] = v
    # every claimed pair was counted exactly once
    pairs = int((t["pbuf"][:t["pcap"]] != 0).sum().item())
    assert pairs == int(t["guniq"].sum().item()) + lost(t)[0]
    return out


def uniq(case_or_segs, plan, kg=None, ranges=None, use_filter=True, **kw):
    t = new_tables(**kw)
    for si, seg in enumerate(case_or_segs):
        base, n = ranges[si] if ranges else (0, seg.n_rows)
        run_uniq(seg, plan, t, base, n, kg=kg, use_filter=use_filter)
    assert lost(t) == [0, 0]
    return uniq_dict(t, plan)


# ------------------------------------------------------------ the library

def test_uniq_spec_size_matches():
    from deepflow_amd.ops import native
    assert ct.sizeof(Q.UniqSpecC) == native.gpu().df_uniq_spec_size()


def test_constants_match():
    from deepflow_amd.ops import native
    seed, mul = ct.c_uint64(), ct.c_uint64()
    slots, shift = ct.c_uint32(), ct.c_uint32()
    native.gpu().df_uniq_consts(ct.byref(seed), ct.byref(mul),
                                ct.byref(slots), ct.byref(shift))
    assert (seed.value, mul.value, slots.value, shift.value) == \
        (UC.UNIQ_SEED, UC.UNIQ_ITEM_MUL, UC.FILTER_SLOTS, UC.FILTER_SHIFT)
    assert Q.UNIQ_SEED == UC.UNIQ_SEED


# ------------------------------------------------------ kernel-level cases

@pytest.fixture(scope="module")
def cases():
    """name -> (case, device segments, device kg, reference counts)."""
    out = {}
    dev = {}
    for c in UC.cpu_cases():
        for s in c.segs:
            if id(s) not in dev:
                dev[id(s)] = QC.to_device(s)
        out[c.name] = (c, [dev[id(s)] for s in c.segs],
                       QC.kg_to_device(c.kg),
                       UC.ref_counts(c.plan, c.segs, c.kg))
    return out


@pytest.mark.parametrize("use_filter", [True, False],
                         ids=["filter", "nofilter"])
@pytest.mark.parametrize("name", [c.name for c in UC.cpu_cases()])
def test_kernel_matches_reference(cases, name, use_filter):
    case, dsegs, dkg, want = cases[name]
    if "want" in case.extra:
        assert want == case.extra["want"]
    assert uniq(dsegs, case.plan, kg=dkg, use_filter=use_filter) == want


@pytest.mark.parametrize("n", [1, 257, 3000])
def test_no_row_matches(cases, n):
    _, dsegs, _, _ = cases[f"shape_{n}"]
    t = new_tables()
    run_uniq(dsegs[0], UC.no_match_plan(), t)
    assert lost(t) == [0, 0]
    for name in ("gkeys", "graw", "guniq"):
        assert int(t[name].abs().sum().item()) == 0
    assert int(t["pbuf"][:t["pcap"]].abs().sum().item()) == 0


def test_multi_arg_bounds(cases):
    case, dsegs, _, want = cases["multi_arg"]
    got = uniq(dsegs, case.plan)
    rows = QC.ref_agg(case.plan, case.segs)
    assert got == want
    for key, (ab, a, b, abcd) in got.items():
        assert max(a, b) <= ab <= abcd <= rows[key][0]


def test_zero_pair_hash_claims_slot_of_one(cases):
    """The pair whose hash is 0 is stored as 1."""
    case, dsegs, _, _ = cases["zero_pair"]
    t = new_tables()
    run_uniq(dsegs[0], case.plan, t)
    pk = t["pbuf"][:t["pcap"]]
    assert int((pk == 1).sum().item()) == 1
    assert uniq_dict(t, case.plan) == {(): [51]}


@pytest.mark.parametrize("base_row, n", UC.WINDOWS)
def test_row_window(base_row, n):
    seg = UC.window_segment()
    plan = UC.uplan([[UC.RRT]], [UC.K_PROTO])
    want = UC.ref_counts(plan, [seg], ranges=[(base_row, n)])
    assert sum(v[0] for v in want.values()) == n
    assert uniq([QC.to_device(seg)], plan, ranges=[(base_row, n)]) == want


def test_two_launches_share_the_pair_table(cases):
    case, dsegs, _, want = cases["two_segments"]
    assert dsegs[0].capacity > dsegs[0].n_rows
    each = [UC.ref_counts(case.plan, [s]) for s in case.segs]
    got = uniq(dsegs, case.plan)
    assert got == want
    # values present in both segments count once: the whole is less than
    # the sum of the parts, for every group
    for key, (c,) in got.items():
        assert c < each[0][key][0] + each[1][key][0]
    # a second pass over the same rows into the same tables adds nothing
    t = new_tables()
    for _ in range(2):
        for s in dsegs:
            run_uniq(s, case.plan, t)
    assert uniq_dict(t, case.plan) == want


@pytest.mark.parametrize("use_filter", [True, False],
                         ids=["filter", "nofilter"])
def test_pair_table_too_small(cases, use_filter):
    case, dsegs, _, want = cases["pair_overflow"]
    assert want == {(): [200]}
    t = new_tables(pcap=64)
    run_uniq(dsegs[0], case.plan, t, use_filter=use_filter)   # checks guard
    group_lost, pair_lost = lost(t)
    assert group_lost == 0 and pair_lost > 0
    total = int(t["guniq"].sum().item())
    assert total <= 64
    assert total == int((t["pbuf"][:64] != 0).sum().item())
    # what did land is a set of true pairs
    truth = {UC.pair_hash((), 0, (v,)) for v in range(7000, 7200)}
    got = set(t["pbuf"][:64].cpu().numpy().view(np.uint64).tolist()) - {0}
    assert got <= truth


def test_group_table_too_small(cases):
    case, dsegs, _, want = cases["group_overflow"]
    assert len(want) == 16
    t = new_tables(cap=4)
    run_uniq(dsegs[0], case.plan, t)
    group_lost, pair_lost = lost(t)
    assert group_lost > 0 and pair_lost == 0
    got = uniq_dict(t, case.plan)    # asserts: no count off a live slot
    assert len(got) == 4
    # a live group holds every one of its pairs; the others' are reported
    assert all(want[k] == v for k, v in got.items())
    assert group_lost == sum(v[0] for k, v in want.items() if k not in got)


@pytest.mark.parametrize("order", ["agg_first", "uniq_first"])
def test_slot_alignment_with_query_agg(cases, order):
    """gvals and guniq rows of one slot describe the same raw key."""
    from deepflow_amd.ops import gpu_ops
    case, dsegs, _, want = cases["multi_arg"]
    plan = case.plan
    counts = QC.ref_agg(plan, case.segs)
    t = new_tables()
    gvals = torch.zeros((1024, Q.QMAX_AGGS), dtype=torch.int64,
                        device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")

    def agg():
        gpu_ops.query_agg(dsegs[0], plan.to_bytes(), 0, dsegs[0].n_rows,
                          t["gkeys"], t["graw"], gvals, overflow=ovf)
        torch.cuda.synchronize()
    if order == "agg_first":
        agg()
        keys_before = t["gkeys"].clone()
        run_uniq(dsegs[0], plan, t)
        assert torch.equal(keys_before, t["gkeys"])   # no new group slot
    else:
        run_uniq(dsegs[0], plan, t)
        agg()
    assert int(ovf.item()) == 0 and lost(t) == [0, 0]
    live = torch.nonzero(t["gkeys"] != 0).flatten().tolist()
    assert len(live) == len(want)
    for slot in live:
        key = (int(t["graw"][slot, 0].item()),)
        assert int(t["gkeys"][slot].item()) & UC.M64 == QC.group_hash(key)
        assert gvals[slot, :len(plan.aggs)].tolist() == counts[key]
        assert t["guniq"][slot].tolist() == want[key]


def test_bad_launch_arguments_are_refused(cases):
    """Sizes the kernel would index out of bounds with never launch."""
    from deepflow_amd.ops import gpu_ops
    case, dsegs, _, _ = cases["shape_257"]
    t = new_tables()
    bad = bytearray(case.plan.uniq_to_bytes())
    bad[-4:] = (Q.QMAX_UNIQ + 1).to_bytes(4, "little")
    with pytest.raises(RuntimeError):
        gpu_ops.query_uniq(dsegs[0], case.plan.to_bytes(), bytes(bad), 0,
                           257, t["gkeys"], t["graw"], t["guniq"],
                           t["pbuf"][:t["pcap"]], overflow=t["overflow"])
    with pytest.raises(RuntimeError):      # pair table not a power of two
        gpu_ops.query_uniq(dsegs[0], case.plan.to_bytes(),
                           case.plan.uniq_to_bytes(), 0, 257, t["gkeys"],
                           t["graw"], t["guniq"], t["pbuf"][:100],
                           overflow=t["overflow"])
    torch.cuda.synchronize()
    assert int(t["guniq"].sum().item()) == 0


# ---------------------------------------------------------------- executor

@pytest.mark.parametrize("name", ["shape_3000", "all_distinct", "multi_arg",
                                  "two_segments", "fam_kg_pod",
                                  "fam_filtered_mixed", "fam_time_bucket_key"])
def test_executor_matches_reference(cases, name):
    case, dsegs, dkg, want = cases[name]
    groups = EX.execute_agg_gpu(case.plan, dsegs, kg=dkg)
    assert UC.engine_counts(groups) == want
    assert {tuple(g["key"]): g["agg"] for g in groups} == \
        QC.ref_agg(case.plan, case.segs, case.kg)
    cpu = EX.execute_agg_cpu(case.plan, case.segs, kg=case.kg)
    assert UC.engine_counts(cpu) == want


def test_executor_without_uniq_is_unchanged(cases):
    case, dsegs, _, _ = cases["shape_3000"]
    plain = QC.plan([], [UC.K_PROTO], [QC.COUNT])
    groups = EX.execute_agg_gpu(plain, dsegs)
    assert groups and all(set(g) == {"key", "agg"} for g in groups)


@pytest.mark.parametrize("name", ["all_distinct", "multi_arg",
                                  "two_segments"])
def test_pair_table_growth(cases, name, monkeypatch):
    case, dsegs, dkg, want = cases[name]
    monkeypatch.setattr(EX, "UNIQ_PAIR_CAP_FIRST_MAX", 64)
    assert sum(sum(v) for v in want.values()) > 64
    groups = EX.execute_agg_gpu(case.plan, dsegs, kg=dkg)
    assert UC.engine_counts(groups) == want


def test_pair_table_limit_raises(cases, monkeypatch):
    case, dsegs, _, _ = cases["pair_overflow"]
    monkeypatch.setattr(EX, "UNIQ_PAIR_CAP_FIRST_MAX", 16)
    monkeypatch.setattr(EX, "UNIQ_PAIR_CAP_MAX", 64)
    with pytest.raises(RuntimeError, match="pair table limit"):
        EX.execute_agg_gpu(case.plan, dsegs)


def test_group_table_growth_with_uniq(cases, monkeypatch):
    case, dsegs, _, want = cases["group_overflow"]
    monkeypatch.setattr(EX, "GROUP_CAP", 4)
    groups = EX.execute_agg_gpu(case.plan, dsegs)
    assert UC.engine_counts(groups) == want


# ------------------------------------------------------------------ engine

@pytest.fixture(scope="module")
def engines():
    out = {dev: UC.l7_engine(dev, l4=True) for dev in ("cpu", "cuda")}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("sql", UC.AGREE_SQL)
def test_gpu_cpu_reference_agree(engines, sql):
    cpu, gpu = engines["cpu"], engines["cuda"]
    plan = UC.plan_for(cpu, sql)
    csegs = cpu.pipe.segments.scan_list()
    assert len([s for s in csegs if s.n_rows]) == 2
    want = UC.ref_counts(plan, csegs, cpu.pipe.kg)
    assert UC.engine_counts(
        EX.execute_agg_cpu(plan, csegs, kg=cpu.pipe.kg)) == want
    # the GPU store numbers its dictionary ids itself: its reference is
    # computed from a host copy of its own segments
    gplan = UC.plan_for(gpu, sql)
    gsegs = gpu.pipe.segments.scan_list()
    want_g = UC.ref_counts(gplan, [QC.to_device(s, "cpu") for s in gsegs],
                           gpu.pipe.kg)
    got = EX.execute_agg_gpu(gplan, gsegs, kg=gpu.pipe.kg)
    assert UC.engine_counts(got) == want_g
    assert sorted(want_g.values()) == sorted(want.values())


def test_engine_growth(engines, monkeypatch):
    sql = UC.AGREE_SQL[3]
    want = engines["cpu"].query(sql)
    monkeypatch.setattr(EX, "UNIQ_PAIR_CAP_FIRST_MAX", 64)
    assert engines["cuda"].query(sql) == want


@pytest.mark.parametrize("key", ["l7_protocol", "request_domain"])
def test_mixed_sql(engines, key):
    UC.check_mixed_sql(engines["cuda"], engines["cpu"], key)


@pytest.mark.parametrize("sql", [
    UC.MIXED_SQL, UC.SINGLE_SQL, UC.UNIQ_ONLY_SQL, UC.L4_SQL,
    "SELECT l7_protocol, Uniq(ip4_0) AS clients FROM l7_flow_log "
    "GROUP BY l7_protocol SLIMIT 2",
    "WITH t AS (SELECT request_domain, ip4_0, Count(*) AS c FROM l7_flow_log "
    "GROUP BY request_domain, ip4_0) SELECT request_domain, Uniq(ip4_0) AS "
    "ips, Sum(c) AS n FROM t GROUP BY request_domain",
] + UC.AGREE_SQL[3:])
def test_engine_sql_matches_cpu(engines, sql):
    want = engines["cpu"].query(sql)
    assert want["values"]
    assert engines["cuda"].query(sql) == want


def test_world1_dist_engine(engines, tmp_path):
    import torch.distributed as dist
    from deepflow_amd.parallel.dist_query import DistQueryEngine
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        deng = DistQueryEngine(engines["cuda"], device="cpu")
        for sql in (UC.MIXED_SQL, UC.SINGLE_SQL, UC.L4_SQL):
            assert deng.query(sql) == engines["cpu"].query(sql), sql
    finally:
        dist.destroy_process_group()
