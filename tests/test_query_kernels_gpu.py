"""K7 query kernels called directly (gpu_ops.query_agg / qpart_agg /
query_select) on the hand-built cases of query_cases.py, against its
brute-force reference. The group-table size, base_row, n and the kernel
taken are chosen by the test. Everything is integer: every comparison is
exact, as sets/dicts (slot and emit order are undefined).

Below them: what the four query entry points (the three and
gpu_ops.query_uniq) share across the C ABI. The SegView mirror against the
library's layout, the spec checks that come before any launch, and the one
group hash of every path."""
import ctypes as ct

import numpy as np
import pytest
import torch

import query_cases as QC
import uniq_cases as UC
from deepflow_amd.ops.ref import mix64
from deepflow_amd.query import spec as Q

pytestmark = pytest.mark.gpu

KERNELS = ["direct", "qpart"]


def run_agg(kernel, seg, plan, base_row=0, n=None, cap=1024, kg=None,
            table=None):
    """One launch into a `cap`-slot group table (or an existing `table`).
    -> (gkeys, graw, gvals, overflow) device tensors."""
    from deepflow_amd.ops import gpu_ops
    n = seg.n_rows - base_row if n is None else n
    if table is None:
        gkeys = torch.zeros(cap, dtype=torch.int64, device="cuda")
        graw = torch.zeros((cap, Q.QMAX_KEYS), dtype=torch.int64,
                           device="cuda")
        gvals = torch.zeros((cap, Q.QMAX_AGGS), dtype=torch.int64,
                            device="cuda")
        for ai, a in enumerate(plan.aggs):
            if a.op == Q.AGGOP_MIN:
                gvals[:, ai] = -1
        overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
        table = (gkeys, graw, gvals, overflow)
    gkeys, graw, gvals, overflow = table
    spec = plan.to_bytes()
    if kernel == "direct":
        gpu_ops.query_agg(seg, spec, base_row, n, gkeys, graw, gvals,
                          kg=kg, overflow=overflow)
    else:
        w = len(plan.keys) + len(plan.aggs)
        counts = torch.zeros(256, dtype=torch.int32, device="cuda")
        cursors = torch.zeros(256, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(max(n * w, 1), dtype=torch.int64,
                              device="cuda")
        gpu_ops.qpart_agg(seg, spec, base_row, n, counts, cursors, scratch,
                          gkeys, graw, gvals, kg=kg, overflow=overflow)
    torch.cuda.synchronize()
    return table


def table_dict(table, plan):
    gkeys, graw, gvals, _ = table
    live = gkeys != 0
    raw = graw[live].cpu().numpy().view(np.uint64)[:, :len(plan.keys)]
    vals = gvals[live].cpu().numpy().view(np.uint64)[:, :len(plan.aggs)]
    out = {}
    for k, v in zip(raw.tolist(), vals.tolist()):
        assert tuple(k) not in out, "one group in two slots"
        out[tuple(k)] = v
    return out


def lost_rows(table) -> int:
    return int(table[3].item()) & 0xFFFFFFFF


def agg(kernel, seg, plan, **kw):
    table = run_agg(kernel, seg, plan, **kw)
    assert lost_rows(table) == 0
    return table_dict(table, plan)


def run_select(seg, plan, base_row, n, out_cap, kg=None):
    from deepflow_amd.ops import gpu_ops
    # one guard element past out_cap: the kernel must never write it
    buf = torch.full((out_cap + 1,), -7, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu_ops.query_select(seg, plan.to_bytes(), base_row, n, buf[:out_cap],
                         ctr, kg=kg)
    torch.cuda.synchronize()
    assert int(buf[out_cap].item()) == -7
    return int(ctr.item()), buf[:out_cap].cpu().tolist()


# ------------------------------------------------------------- filters

@pytest.fixture(scope="module")
def filter_seg():
    seg = QC.filter_segment()
    return seg, QC.to_device(seg)


@pytest.mark.parametrize("family", list(QC.FILTER_FAMILIES),
                         ids=["u64", "u32", "u8", "did"])
def test_filter_matrix(filter_seg, family):
    seg, dseg = filter_seg
    n = seg.n_rows
    for term in QC.filter_terms(family):
        want = QC.ref_select(QC.plan([term]), seg)
        cnt, rows = run_select(dseg, QC.plan([term]), 0, n, n)
        assert cnt == len(want), term
        assert set(rows[:cnt]) == want and len(set(rows[:cnt])) == cnt, term
        got = agg("direct", dseg, QC.plan([term], [], [QC.COUNT]), cap=64)
        assert got == ({(): [len(want)]} if want else {}), term


# ----------------------------------------------------------------- CNF

@pytest.fixture(scope="module")
def cnf_seg():
    seg = QC.cnf_segment()
    return seg, QC.to_device(seg)


@pytest.mark.parametrize("name", list(QC.cnf_plans()))
def test_cnf(cnf_seg, name):
    seg, dseg = cnf_seg
    plan = QC.cnf_plans()[name]
    want = QC.ref_agg(plan, [seg])
    assert bool(want) == (name != "dead_group")
    assert agg("direct", dseg, plan) == want
    assert agg("qpart", dseg, plan) == want
    sel = QC.plan(plan.terms)
    cnt, rows = run_select(dseg, sel, 0, seg.n_rows, seg.n_rows)
    assert set(rows[:cnt]) == QC.ref_select(sel, seg)
    assert cnt == sum(v[0] for v in want.values())


# ------------------------------------------------------ source families

@pytest.fixture(scope="module")
def sources():
    case = QC.sources_case()
    return case, QC.to_device(case.segs[0]), QC.kg_to_device(case.kg)


@pytest.mark.parametrize("name", list(QC.source_plans()))
def test_source_families(sources, name):
    case, dseg, dkg = sources
    plan = QC.source_plans()[name]
    nokg = name.endswith("_nokg")
    want = QC.ref_agg(plan, case.segs, None if nokg else case.kg)
    assert want
    assert agg("direct", dseg, plan, kg=None if nokg else dkg) == want
    if plan.keys:
        assert agg("qpart", dseg, plan, kg=None if nokg else dkg) == want


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", [QC.sum_wrap_case, QC.hash_zero_case,
                                  QC.lds_spill_case],
                         ids=["sum_wrap", "hash_zero", "lds_spill"])
def test_small_cases(case, kernel):
    """SUM wraps at 2^64; the key hashing to 0 keeps its group; a 40-key
    LDS probe chain spills past the 16-probe limit into the global table."""
    case = case()
    want = QC.ref_agg(case.plan, case.segs)
    if "want" in case.extra:
        assert want == case.extra["want"]
    if case.name == "hash_zero":
        assert (QC.HASH_ZERO_KEY,) in want
    if case.name == "lds_spill":
        assert all((int(k),) in want for k in case.extra["chain"])
    assert agg(kernel, QC.to_device(case.segs[0]), case.plan) == want


def test_more_keys_than_lds_slots_in_one_partition_block():
    """>= 9600 keys in ONE radix bucket: each of its 16 blocks sees >= 600
    distinct keys for a 512-slot LDS table."""
    keys = QC.keys_with_hash_bits(9600, 40, 8, seed=40, batch=1 << 20)
    assert len(keys) == 9600
    assert len(set(((QC.group_hash_np(keys) >> np.uint64(40)) &
                    np.uint64(255)).tolist())) == 1
    rng = np.random.default_rng(41)
    col = rng.permutation(np.concatenate([keys, keys[::3]]))
    n = len(col)
    seg = QC.new_segment(n)
    QC.set_u64(seg, "flow_id", col)
    QC.set_u64(seg, "rrt", rng.integers(0, 1 << 40, n))
    case = QC.Case("one_bucket", QC._agg_plan_u64_key(), [seg])
    want = QC.ref_agg(case.plan, [seg])
    assert len(want) == 9600 and {v[0] for v in want.values()} == {1, 2}
    dseg = QC.to_device(seg)
    assert agg("qpart", dseg, case.plan, cap=1 << 15) == want
    assert agg("direct", dseg, case.plan, cap=1 << 15) == want


# ------------------------------------------------------------- geometry

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("base_row,n", [(0, 1), (0, 255), (0, 256),
                                        (0, 257), (1, 1), (1, 256),
                                        (300, 257), (300, 399)])
def test_launch_geometry(kernel, base_row, n):
    base = QC.geometry_segment()
    assert base_row + n < base.n_rows
    seg = QC.geometry_poison(base, base_row, n)
    plan = QC._agg_plan_u64_key()
    want = QC.ref_agg(plan, [seg], ranges=[(base_row, n)])
    assert want == QC.ref_agg(plan, [base], ranges=[(base_row, n)])
    assert want != QC.ref_agg(plan, [seg], ranges=[(0, seg.n_rows)])
    got = agg(kernel, QC.to_device(seg), plan, base_row=base_row, n=n)
    assert got == want


@pytest.mark.parametrize("kernel", KERNELS)
def test_segments_share_one_group_table(kernel):
    """Successive launches into one table: MIN is not re-initialised."""
    case = QC.multi_segment_case()
    want = QC.ref_agg(case.plan, case.segs)
    table = None
    for seg in case.segs:
        table = run_agg(kernel, QC.to_device(seg), case.plan, table=table)
    assert lost_rows(table) == 0
    assert table_dict(table, case.plan) == want


def as_dict(groups):
    return {tuple(g["key"]): g["agg"] for g in groups}


def test_execute_agg_gpu_multi_segment():
    from deepflow_amd.query.executor import execute_agg_gpu
    case = QC.multi_segment_case()
    want = QC.ref_agg(case.plan, case.segs)
    got = execute_agg_gpu(case.plan, [QC.to_device(s) for s in case.segs])
    assert len(got) == len(want) and as_dict(got) == want


def test_grid_stride_second_iteration():
    """n = 4096*256 + 257: the grid is capped at 4096 blocks, so the last
    257 rows are only reached by a second grid-stride iteration."""
    from deepflow_amd.store.segment import L7Segment
    n = 4096 * 256 + 257
    rng = np.random.default_rng(4096)
    key = rng.integers(0, 1000, n).astype(np.uint32)
    val = rng.integers(0, 1 << 40, n).astype(np.uint64)
    status = rng.integers(0, 4, n).astype(np.uint8)
    # the tail rows alone hold three keys and the extreme values
    key[-257:] = 2000 + np.arange(257) % 3
    val[-1], val[-2] = 0, (1 << 64) - 1
    status[-257:] = 1
    seg = L7Segment(n, "cuda", pool_capacity=64)
    seg.n_rows = n
    kc, vc, sc = (QC.U32["server_port"], QC.U64["rrt"],
                  QC.U8["response_status"])
    seg.u32[kc] = QC.u32_t(key).cuda()
    seg.u64[vc] = QC.u64_t(val).cuda()
    seg.u8[sc] = torch.from_numpy(status).cuda()
    plan = QC.plan([QC.Term(Q.SRC_U8, sc, Q.OP_NE, 0)],
                   [QC.Key(Q.SRC_U32, kc)],
                   [QC.COUNT, QC.Agg(Q.AGGOP_SUM, Q.SRC_U64, vc),
                    QC.Agg(Q.AGGOP_MIN, Q.SRC_U64, vc),
                    QC.Agg(Q.AGGOP_MAX, Q.SRC_U64, vc)])
    m = status != 0
    uniq, inv = np.unique(key[m], return_inverse=True)
    cnt = np.bincount(inv, minlength=len(uniq)).astype(np.uint64)
    s = np.zeros(len(uniq), dtype=np.uint64)
    np.add.at(s, inv, val[m])                     # uint64: wraps at 2^64
    mn = np.full(len(uniq), (1 << 64) - 1, dtype=np.uint64)
    np.minimum.at(mn, inv, val[m])
    mx = np.zeros(len(uniq), dtype=np.uint64)
    np.maximum.at(mx, inv, val[m])
    want = {(int(k),): [int(a), int(b), int(c), int(d)]
            for k, a, b, c, d in zip(uniq, cnt, s, mn, mx)}
    assert len(want) == 1003 and want[(2000,)][0] == 86
    assert agg("direct", seg, plan, cap=4096) == want
    assert agg("qpart", seg, plan, cap=4096) == want


# --------------------------------------------------------------- select

@pytest.mark.parametrize("base_row,n", [(0, 700), (1, 256), (300, 257)])
def test_select_capacity_and_ranges(base_row, n):
    seg = QC.select_segment()
    dseg = QC.to_device(seg)
    plan = QC.select_plan()
    want = QC.ref_select(plan, seg, base_row, n)
    assert len(want) > 40
    # room to spare: exactly the reference set
    cnt, rows = run_select(dseg, plan, base_row, n, len(want) + 5)
    assert cnt == len(want) and set(rows[:cnt]) == want
    assert rows[cnt:] == [-7] * 5
    # too small: the counter is still the true match count, and every id
    # written is a distinct matching row
    cap = len(want) // 3
    cnt, rows = run_select(dseg, plan, base_row, n, cap)
    assert cnt == len(want)
    assert len(set(rows)) == cap and set(rows) <= want


# ------------------------------------------------- group-table overflow

@pytest.mark.parametrize("kernel", KERNELS)
def test_full_group_table_reports_instead_of_merging(kernel):
    """200 keys, 64 slots: each reported group is exact, and the rows of
    the groups left out are counted."""
    case = QC.overflow_case()
    seg = case.segs[0]
    want = QC.ref_agg(case.plan, [seg])
    assert len(want) == 200
    table = run_agg(kernel, QC.to_device(seg), case.plan, cap=64)
    got = table_dict(table, case.plan)
    assert len(got) == 64
    for key, aggs in got.items():
        assert aggs == want[key], key
    reported = sum(v[0] for v in got.values())
    assert lost_rows(table) == seg.n_rows - reported > 0


def test_full_group_table_counts_rows_without_a_count_aggregate():
    """No COUNT in the spec: the row tally comes from the per-slot row
    counter instead."""
    case = QC.overflow_case()
    seg = case.segs[0]
    rrt = QC.U64["rrt"]
    plan = QC.plan([], case.plan.keys,
                   [QC.Agg(Q.AGGOP_MAX, Q.SRC_U64, rrt),
                    QC.Agg(Q.AGGOP_SUM, Q.SRC_U64, rrt)])
    want = QC.ref_agg(plan, [seg])
    rows_of = {k: v[0] for k, v in QC.ref_agg(case.plan, [seg]).items()}
    for kernel in KERNELS:
        table = run_agg(kernel, QC.to_device(seg), plan, cap=64)
        got = table_dict(table, plan)
        assert len(got) == 64
        assert all(got[k] == want[k] for k in got)
        assert lost_rows(table) == seg.n_rows - sum(rows_of[k] for k in got)


def test_execute_agg_gpu_grows_the_group_table(monkeypatch):
    from deepflow_amd.query import executor as ex
    case = QC.overflow_case()
    want = QC.ref_agg(case.plan, case.segs)
    monkeypatch.setattr(ex, "GROUP_CAP", 64)
    dsegs = [QC.to_device(s) for s in case.segs]
    got = ex.execute_agg_gpu(case.plan, dsegs)
    assert len(got) == 200 and as_dict(got) == want
    # and at the growth limit the error names the group count limit
    monkeypatch.setattr(ex, "GROUP_CAP_MAX", 64)
    with pytest.raises(RuntimeError, match="more than 64 groups"):
        ex.execute_agg_gpu(case.plan, dsegs)


# ------------------------------------------------- the segment view ABI

def test_seg_view_mirror_matches_the_library():
    """sizeof and every member offset of gpu_ops.SegViewC are the
    library's SegView's. No kernel runs."""
    from deepflow_amd.ops import gpu_ops, native
    lib = native.gpu()
    mirror = gpu_ops.SegViewC
    names = [name for name, _ in mirror._fields_]
    # room to spare behind the mirror's members: a member the library has
    # and the mirror lacks lands on a guard word instead of past the array
    guard = 0xFFFFFFFF
    offs = (ct.c_uint32 * (len(names) + 8))(*[guard] * (len(names) + 8))
    lib.df_seg_view_offsets(offs)
    assert ct.sizeof(mirror) == lib.df_seg_view_size()
    assert list(offs[:len(names)]) == [getattr(mirror, n).offset
                                       for n in names]
    assert list(offs[len(names):]) == [guard] * 8


# ------------------------------------------- spec checks before a launch

ENTRIES = ["agg", "qpart", "uniq", "select"]
UNTOUCHED = 5
HIP_INVALID_VALUE = r"HIP error 1 in "      # not 9, invalid configuration


def call_entry(entry, seg, spec, uspec, n, cap):
    """One call of a query entry point with `cap`-slot tables.
    -> every device tensor it could write, each filled with UNTOUCHED."""
    from deepflow_amd.ops import gpu_ops

    def t(*shape, dtype=torch.int64):
        return torch.full(shape, UNTOUCHED, dtype=dtype, device="cuda")
    gkeys, graw, gvals = t(cap), t(cap, Q.QMAX_KEYS), t(cap, Q.QMAX_AGGS)
    ovf = t(2, dtype=torch.int32)
    if entry == "agg":
        out = [gkeys, graw, gvals, ovf]
        gpu_ops.query_agg(seg, spec, 0, n, gkeys, graw, gvals, overflow=ovf)
    elif entry == "qpart":
        counts, cursors = t(256, dtype=torch.int32), t(256, dtype=torch.int32)
        scratch = t(64)
        out = [gkeys, graw, gvals, ovf, counts, cursors, scratch]
        gpu_ops.qpart_agg(seg, spec, 0, n, counts, cursors, scratch, gkeys,
                          graw, gvals, overflow=ovf)
    elif entry == "uniq":
        guniq, pkeys = t(cap, Q.QMAX_UNIQ), t(1024)
        out = [gkeys, graw, guniq, pkeys, ovf]
        gpu_ops.query_uniq(seg, spec, uspec, 0, n, gkeys, graw, guniq, pkeys,
                           overflow=ovf)
    else:
        rows, ctr = t(16), t(1, dtype=torch.int32)
        out = [rows, ctr]
        gpu_ops.query_select(seg, spec, 0, n, rows, ctr)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_specs_are_refused_before_any_launch(entry):
    """n = 0 throughout, so a check that is missing cannot put a malformed
    spec in front of a kernel: it shows as a call that does not raise."""
    dseg = QC.to_device(QC.geometry_segment())
    plan = UC.uplan([[UC.RRT]], [UC.K_PROTO])
    spec, uspec = plan.to_bytes(), plan.uniq_to_bytes()
    # well-formed and empty: a clean return, nothing written
    for buf in call_entry(entry, dseg, spec, uspec, 0, 1024):
        assert bool((buf == UNTOUCHED).all())

    def with_count(field, value):
        bad = bytearray(spec)
        off = getattr(Q.QuerySpecC, field).offset
        bad[off:off + 4] = value.to_bytes(4, "little")
        return bytes(bad)
    bad_calls = [(with_count("n_terms", Q.QMAX_TERMS + 1), 1024),
                 (with_count("n_keys", Q.QMAX_KEYS + 1), 1024),
                 (with_count("n_aggs", Q.QMAX_AGGS + 1), 1024)]
    if entry != "select":           # the one entry point without a table
        bad_calls.append((spec, 768))
    for bad_spec, cap in bad_calls:
        with pytest.raises(RuntimeError, match=HIP_INVALID_VALUE):
            call_entry(entry, dseg, bad_spec, uspec, 0, cap)


# ------------------------------------------------ one hash on every path

def hash_paths_case():
    """Two segments of 300 rows (one full block and a partial one) over 40
    tuples of QMAX_KEYS keys. One tuple is hash_zero_case's key completed
    to four so that its hash is still 0 before the 0 -> 1 rule: the last
    key is a u64 column, set to undo what the three before it left."""
    rng = np.random.default_rng(1615)
    keys = [QC.Key(Q.SRC_U64, QC.U64["flow_id"]),
            QC.Key(Q.SRC_U32, QC.U32["server_port"]),
            QC.Key(Q.SRC_U8, QC.U8["l7_protocol"]),
            QC.Key(Q.SRC_U64, QC.U64["syscall_trace_id_request"])]
    assert len(keys) == Q.QMAX_KEYS
    tuples = {(int(rng.integers(1, 1 << 62)), int(rng.integers(0, 1 << 16)),
               int(rng.integers(0, 4)), int(rng.integers(0, 1 << 62)))
              for _ in range(39)}
    h = QC.HASH_SEED
    for k, v in enumerate((QC.HASH_ZERO_KEY, 443, 2)):
        h = mix64(h ^ v ^ (k << 56))
    zero = (QC.HASH_ZERO_KEY, 443, 2, h ^ (3 << 56))
    assert QC.group_hash(zero) == 1 and len(tuples | {zero}) == 40
    tuples = np.array(sorted(tuples | {zero}), dtype=np.uint64)
    rrt = QC.U64["rrt"]
    plan = UC.uplan([[UC.RRT]], keys,
                    extra_aggs=[QC.COUNT, QC.Agg(Q.AGGOP_SUM, Q.SRC_U64, rrt),
                                QC.Agg(Q.AGGOP_MIN, Q.SRC_U64, rrt),
                                QC.Agg(Q.AGGOP_MAX, Q.SRC_U64, rrt)])
    segs = []
    for _ in range(2):
        # every tuple at least once per segment, the rest at random
        pick = tuples[np.concatenate([rng.permutation(40),
                                      rng.integers(0, 40, 260)])]
        seg = QC.new_segment(300)
        QC.set_u64(seg, "flow_id", pick[:, 0])
        QC.set_u32(seg, "server_port", pick[:, 1])
        QC.set_u8(seg, "l7_protocol", pick[:, 2])
        QC.set_u64(seg, "syscall_trace_id_request", pick[:, 3])
        QC.set_u64(seg, "rrt", rng.integers(1, 12, 300))
        segs.append(seg)
    return plan, segs, zero


def test_every_path_names_a_group_by_one_hash():
    """Segment A through query_agg, segment B through qpart_agg, both
    through query_uniq, all into one 1024-slot table. A path that hashed a
    tuple differently would give it a second slot, or count its distinct
    values against another group's."""
    from deepflow_amd.ops import gpu_ops
    from deepflow_amd.query.executor import execute_agg_cpu
    plan, segs, zero = hash_paths_case()
    want = {tuple(g["key"]): (g["agg"], g["uniq"])
            for g in execute_agg_cpu(plan, segs)}
    assert len(want) == 40 and zero in want
    dsegs = [QC.to_device(s) for s in segs]
    table = run_agg("direct", dsegs[0], plan, cap=1024)
    table = run_agg("qpart", dsegs[1], plan, table=table)
    gkeys, graw, gvals, overflow = table
    guniq = torch.zeros((1024, Q.QMAX_UNIQ), dtype=torch.int64,
                        device="cuda")
    pkeys = torch.zeros(1 << 12, dtype=torch.int64, device="cuda")
    lost = torch.zeros(2, dtype=torch.int32, device="cuda")
    for dseg in dsegs:
        gpu_ops.query_uniq(dseg, plan.to_bytes(), plan.uniq_to_bytes(), 0,
                           dseg.n_rows, gkeys, graw, guniq, pkeys,
                           overflow=lost)
    torch.cuda.synchronize()
    assert lost_rows(table) == 0 and lost.tolist() == [0, 0]
    live = torch.nonzero(gkeys != 0).flatten().tolist()
    assert len(live) == 40          # every tuple owns exactly one slot
    assert int(guniq[gkeys == 0].abs().sum().item()) == 0
    raw = graw.cpu().numpy().view(np.uint64)
    vals = gvals.cpu().numpy().view(np.uint64)
    seen = set()
    for slot in live:
        key = tuple(raw[slot].tolist())
        seen.add(key)
        assert int(gkeys[slot].item()) & QC.M64 == QC.group_hash(key)
        aggs, uniq = want[key]
        assert vals[slot, :len(plan.aggs)].tolist() == aggs, key
        assert guniq[slot, :len(plan.uniqs)].tolist() == uniq, key
    assert seen == set(want)
