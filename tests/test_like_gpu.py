"""DF-SQL LIKE / REGEXP on dictionary tags (K16) on the GPU: k_dict_match
called directly against Python `re` per entry, the arena's catch-up through
the real ingest pipeline, OP_INSET / OP_NOT_INSET in eval_terms through the
four query entry points against the brute-force reference of like_cases.py,
and the GPU engine against the CPU engine. Every comparison is of exact
integers or exact sets."""
import numpy as np
import pytest
import torch

import like_cases as LC
import query_cases as QC
import uniq_cases as UC
from deepflow_amd.query import executor as EX
from deepflow_amd.query import logregex
from deepflow_amd.query import spec as Q
from deepflow_amd.query.logregex import compile_log_regex
from deepflow_amd.store.dictionary import DictArena

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
GUARD_BYTES = 64


# ------------------------------------------------------ constants, sizes

def test_set_ops_and_spec_size_match_the_library():
    from deepflow_amd.ops import gpu_ops, native
    assert gpu_ops.query_set_ops() == (Q.OP_INSET, Q.OP_NOT_INSET)
    import ctypes as ct
    sizes = [ct.c_uint32() for _ in range(4)]
    native.gpu().df_spec_sizes(*[ct.byref(s) for s in sizes])
    assert sizes[0].value == ct.sizeof(Q.QTermC) == 24
    assert sizes[3].value == ct.sizeof(Q.QuerySpecC)
    assert gpu_ops.dict_re_limits() == (logregex.MAX_TABLE_BYTES,
                                        logregex.MAX_CLASSES)


# ------------------------------------------------- k_dict_match, directly

def _arena(entries):
    """A device arena of the entries in order, with a guard run of bytes
    behind the last entry."""
    a = DictArena("cuda")
    a.pending = list(entries)
    a.upload()
    used = a.nbytes
    data = torch.full((used + GUARD_BYTES,), 0x5A, dtype=torch.uint8,
                      device="cuda")
    data[:used].copy_(a.data[:used])
    a.data = data
    return a


def _run_match(a, rx, first=0, n_entries=None, complement=False,
               words=None):
    """-> the bitmap tensor, with one guard word on each side."""
    from deepflow_amd.ops import gpu_ops
    n_words = LC.MATCH_CAPACITY // 32
    if words is None:
        words = torch.zeros(n_words + 2, dtype=torch.int32, device="cuda")
        words[0] = GUARD
        words[-1] = GUARD
    gpu_ops.dict_match(a, rx, words[1:-1], LC.MATCH_CAPACITY, first=first,
                       n_entries=n_entries, complement=complement)
    torch.cuda.synchronize()
    return words


def _ids(words) -> set:
    w = words.cpu().numpy().view(np.uint32)
    assert int(w[0]) == GUARD and int(w[-1]) == GUARD
    bits = np.unpackbits(w[1:-1].view(np.uint8), bitorder="little")
    return set(np.nonzero(bits)[0].tolist())


@pytest.fixture(scope="module")
def arenas():
    out = {}
    for n in LC.MATCH_SIZES:
        entries = LC.match_entries(n)
        out[n] = (entries, _arena(entries))
    return out


@pytest.mark.parametrize("n", LC.MATCH_SIZES)
def test_dict_match_equals_re(arenas, n):
    entries, a = arenas[n]
    assert a.n == n
    for pat in LC.MATCH_PATTERNS:
        rx = compile_log_regex(pat)
        want = {i for i, s in entries if rx.host.search(s)}
        assert _ids(_run_match(a, rx)) == want, pat
        rest = {i for i, _ in entries} - want
        assert _ids(_run_match(a, rx, complement=True)) == rest, pat
    tail = a.data[a.nbytes:].cpu()
    assert tail.numel() == GUARD_BYTES and bool((tail == 0x5A).all())


def test_dict_match_cases_mean_something(arenas):
    """What the special entries are there for, spelled out."""
    entries, a = arenas[1000]
    by = {p: _ids(_run_match(a, compile_log_regex(p)))
          for p in LC.MATCH_PATTERNS}
    top = LC.MATCH_CAPACITY - 1
    assert 0 in by["foo$"] and 72 in by["foo$"]   # `foo`, `foo\n`
    assert by["bc"] == {73}                       # not across ..ab|cd..
    assert {64, 70, 71} <= by["Z"] and by["Z"] == by["Z$"]
    assert top in by["line$"] and top not in by[r"line\Z"]
    assert by["^$"] == {74}                       # `\n` alone
    assert by["a*"] == {i for i, _ in entries}    # nullable: everything
    assert by[r"\A[\s\S]\Z"] == {65, 74}
    assert 71 in by["q{40}Z"]                     # the 4096-byte entry
    assert {i for i, _ in entries} >= {0, 31, 32, 63, 64, top}


@pytest.mark.parametrize("k", [1, 64, 300, 999])
def test_dict_match_in_two_ranges(arenas, k):
    entries, a = arenas[1000]
    for pat in ("/api/", "^/user/[0-9]+$", "foo$"):
        rx = compile_log_regex(pat)
        one = _ids(_run_match(a, rx))
        words = _run_match(a, rx, first=0, n_entries=k)
        assert _ids(words) == {i for i, s in entries[:k]
                               if rx.host.search(s)}
        words = _run_match(a, rx, first=k, words=words)
        assert _ids(words) == one, (pat, k)


def test_dict_match_skips_ids_outside_the_bitmap():
    from deepflow_amd.ops import gpu_ops
    a = _arena([(5, b"aa"), (95, b"ab"), (96, b"ac"), (LC.INVALID, b"ad")])
    words = torch.zeros(5, dtype=torch.int32, device="cuda")
    words[0] = GUARD
    words[4] = GUARD
    gpu_ops.dict_match(a, compile_log_regex("^a"), words[1:4], 96)
    torch.cuda.synchronize()
    w = words.cpu().numpy().view(np.uint32).tolist()
    assert w == [GUARD, 1 << 5, 0, 1 << 31, GUARD]


# ---------------------------------------------------------- arena catch-up

def _span_pipe(device):
    from deepflow_amd.ingest import L7IngestPipeline
    cfg = UC.gen_cfg(n=300)
    return L7IngestPipeline(device=device, segment_rows=1 << 10,
                            dict_capacity=1 << 12,
                            time_base_s=cfg.base_time_ns // 10**9)


def test_arena_catch_up_through_the_pipeline():
    from deepflow_amd.gen import SpanGenConfig
    from deepflow_amd.gen.spans import gen_span_payload
    from deepflow_amd.query import QueryEngine
    engines = {d: QueryEngine(_span_pipe(d), device=d)
               for d in ("cpu", "cuda")}
    sql = ("SELECT request_resource, Count(*) AS c FROM l7_flow_log WHERE "
           "request_resource LIKE '%/r/000__' GROUP BY request_resource")

    def ingest(cfg):
        for e in engines.values():
            e.pipe.ingest_frame_payload(gen_span_payload(cfg))

    def both():
        got = LC.sorted_result(engines["cuda"].query(sql))
        assert got == LC.sorted_result(engines["cpu"].query(sql))
        return got

    ingest(UC.gen_cfg(n=300))
    first = both()
    (arena,) = engines["cuda"].pipe.dict._arenas[LC.DOM_RES].values()
    seen = (arena.n, arena.uploads, arena.h2d_copies)
    assert arena.n == 12 and seen[1:] == (1, 2) and len(first[1]) == 12
    # more resources, harvested by the pipeline in small batches
    for seed in (21, 22, 23):
        ingest(SpanGenConfig(n=100, seed=seed, tag_cardinality=60,
                             n_attrs=2, n_ips=48, n_services=5,
                             n_resources=60))
    second = both()
    assert len(second[1]) > len(first[1])
    assert arena.n > seen[0]
    assert (arena.uploads, arena.h2d_copies) == (2, 4)   # one catch-up
    launches = EX.SET_STATS["dict_match"]
    assert both() == second
    assert (arena.uploads, arena.h2d_copies) == (2, 4)   # nothing new
    assert EX.SET_STATS["dict_match"] == launches + 1


# ------------------------------------------------- eval_terms, set terms

@pytest.fixture(scope="module")
def set_data():
    words = torch.from_numpy(LC.set_words().view(np.int32)).cuda()
    segs = {n: LC.set_segment(n) for n in (257, 1025)}
    return words, {n: (s, QC.to_device(s)) for n, s in segs.items()}


def _spec(plan, words):
    return plan.to_bytes(sets=[(words.data_ptr(), LC.SET_BITS)])


def _counts(seg, rows, plan):
    c = QC._Cols(seg)
    out = {}
    for r in rows:
        k = tuple(QC.ref_value(c, r, key.family, key.idx, key.bucket, 0,
                               None) for key in plan.keys)
        out[k] = out.get(k, 0) + 1
    return {k: [v] for k, v in out.items()}


@pytest.mark.parametrize("n,base_row,rows", [(257, 0, 257), (257, 37, 220),
                                             (1025, 0, 1025),
                                             (1025, 129, 801)])
@pytest.mark.parametrize("name", list(LC.set_plans()))
def test_eval_terms_set_ops(set_data, name, n, base_row, rows):
    from deepflow_amd.ops import gpu_ops
    words, segs = set_data
    seg, dseg = segs[n]
    plan = LC.set_plans()[name]
    spec = _spec(plan, words)
    want_rows = LC.set_ref_rows(plan, seg, base_row, rows)
    assert 0 < len(want_rows) < rows
    want = _counts(seg, want_rows, plan)
    cap = 64

    def table():
        return (torch.zeros(cap, dtype=torch.int64, device="cuda"),
                torch.zeros((cap, Q.QMAX_KEYS), dtype=torch.int64,
                            device="cuda"),
                torch.zeros((cap, Q.QMAX_AGGS), dtype=torch.int64,
                            device="cuda"),
                torch.zeros(2, dtype=torch.int32, device="cuda"))

    def as_dict(gkeys, graw, gvals):
        live = gkeys != 0
        raw = graw[live].cpu().numpy().view(np.uint64)[:, :len(plan.keys)]
        vals = gvals[live].cpu().numpy().view(np.uint64)[:, :1]
        return {tuple(k): v for k, v in zip(raw.tolist(), vals.tolist())}

    # k_query_agg
    gkeys, graw, gvals, ovf = table()
    gpu_ops.query_agg(dseg, spec, base_row, rows, gkeys, graw, gvals,
                      overflow=ovf[:1])
    torch.cuda.synchronize()
    assert as_dict(gkeys, graw, gvals) == want and int(ovf[0]) == 0
    # the partitioned group-by
    pk, pr, pv, povf = table()
    counts = torch.zeros(256, dtype=torch.int32, device="cuda")
    cursors = torch.zeros(256, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(rows * 2, dtype=torch.int64, device="cuda")
    gpu_ops.qpart_agg(dseg, spec, base_row, rows, counts, cursors, scratch,
                      pk, pr, pv, overflow=povf[:1])
    torch.cuda.synchronize()
    assert as_dict(pk, pr, pv) == want and int(povf[0]) == 0
    # k_query_uniq: distinct rrt per group, into k_query_agg's table
    uplan = UC.uplan([[UC.RRT]], plan.keys, plan.terms)
    guniq = torch.zeros((cap, Q.QMAX_UNIQ), dtype=torch.int64,
                        device="cuda")
    pkeys = torch.zeros(4096, dtype=torch.int64, device="cuda")
    uovf = torch.zeros(2, dtype=torch.int32, device="cuda")
    gpu_ops.query_uniq(dseg, _spec(uplan, words), uplan.uniq_to_bytes(),
                       base_row, rows, gkeys, graw, guniq, pkeys,
                       overflow=uovf)
    torch.cuda.synchronize()
    c = QC._Cols(seg)
    distinct = {}
    for r in want_rows:
        k = (int(c.u8[QC.U8["response_status"], r]),)
        distinct.setdefault(k, set()).add(int(c.u64[QC.U64["rrt"], r]))
    live = gkeys != 0
    got_u = {tuple(k): int(u) for k, u in zip(
        graw[live].cpu().numpy().view(np.uint64)[:, :1].tolist(),
        guniq[live].cpu()[:, 0].tolist())}
    assert got_u == {k: len(v) for k, v in distinct.items()}
    assert uovf.cpu().tolist() == [0, 0]
    # k_query_select
    buf = torch.full((rows + 1,), -7, dtype=torch.int64, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu_ops.query_select(dseg, spec, base_row, rows, buf[:rows], ctr)
    torch.cuda.synchronize()
    cnt = int(ctr.item())
    assert cnt == len(want_rows) and int(buf[rows].item()) == -7
    assert sorted(buf[:cnt].cpu().tolist()) == want_rows


def test_set_edge_ids_one_by_one(set_data):
    """bits-1 is a member, bits and DICT_ID_INVALID are not, although the
    word behind `bits` has its bit set."""
    from deepflow_amd.ops import gpu_ops
    words, _ = set_data
    ids = [LC.SET_BITS - 1, LC.SET_BITS, LC.INVALID, 1, 0, 95, 96]
    seg = QC.new_segment(len(ids))
    QC.set_did(seg, LC.DID_RES, np.array(ids, dtype=np.uint32))
    dseg = QC.to_device(seg)
    for op, want in ((Q.OP_INSET, [0, 4]), (Q.OP_NOT_INSET, [1, 2, 3, 5, 6])):
        plan = QC.plan([Q.Term(Q.SRC_DID, LC.DID_RES, op, 0)])
        buf = torch.zeros(len(ids), dtype=torch.int64, device="cuda")
        ctr = torch.zeros(1, dtype=torch.int32, device="cuda")
        gpu_ops.query_select(dseg, _spec(plan, words), 0, len(ids), buf, ctr)
        torch.cuda.synchronize()
        assert sorted(buf[:int(ctr.item())].cpu().tolist()) == want


# ------------------------------------------------- hand-built, end to end

@pytest.mark.parametrize("where,cnf", LC.HAND_WHERE,
                         ids=[w for w, _ in LC.HAND_WHERE])
def test_gpu_executor_matches_string_reference(where, cnf):
    from deepflow_amd.query.sql import parse_sql
    d, seg = LC.hand_dictionary(), LC.hand_segment()
    dseg = QC.to_device(seg)
    want = LC.hand_ref_rows(seg, cnf)
    plan = parse_sql("SELECT start_time FROM l7_flow_log WHERE " + where +
                     " LIMIT 100000", dictionary=d)
    got = EX.execute(plan, [dseg], "cuda")
    assert {r for _, r in got} == want and len(got) == len(want)
    agg = parse_sql("SELECT Count(*) AS c FROM l7_flow_log WHERE " + where,
                    dictionary=d)
    groups = EX.execute(agg, [dseg], "cuda")
    assert groups == ([{"key": [], "agg": [len(want)]}] if want else [])


# ----------------------------------------------------------------- engines

@pytest.fixture(scope="module")
def engines():
    out = {dev: UC.l7_engine(dev) for dev in ("cpu", "cuda")}
    for e in out.values():
        e.name_maps = {"pod": LC.pod_names(e)}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("sql", LC.ENGINE_SQL)
def test_gpu_engine_equals_cpu_engine(engines, sql):
    want = engines["cpu"].query(sql)
    assert want["values"]
    assert LC.sorted_result(engines["cuda"].query(sql)) == \
        LC.sorted_result(want)


def test_query_without_patterns_is_unchanged(engines):
    before = dict(EX.SET_STATS)
    sql = ("SELECT request_domain, Count(*) AS c FROM l7_flow_log WHERE "
           "request_resource = '/api/v1/r/00003' GROUP BY request_domain")
    want = engines["cpu"].query(sql)
    assert want["values"]
    assert LC.sorted_result(engines["cuda"].query(sql)) == \
        LC.sorted_result(want)
    # a wildcard-free LIKE is that same query: no bitmap, no launch
    like = sql.replace("= '/api", "LIKE '/api")
    assert LC.sorted_result(engines["cuda"].query(like)) == \
        LC.sorted_result(want)
    assert EX.SET_STATS == before
    engines["cuda"].query(LC.ENGINE_SQL[0])
    assert EX.SET_STATS["bitmaps"] == before["bitmaps"] + 1
    assert EX.SET_STATS["dict_match"] == before["dict_match"] + 1


def test_world1_dist_engine(engines, tmp_path):
    import torch.distributed as dist
    from deepflow_amd.parallel.dist_query import DistQueryEngine
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg",
                            rank=0, world_size=1)
    try:
        deng = DistQueryEngine(engines["cuda"], device="cpu")
        # (no Percentile here: across shards it merges as histograms)
        for sql in (LC.ENGINE_SQL[0], LC.ENGINE_SQL[2], LC.ENGINE_SQL[5],
                    LC.ENGINE_SQL[7]):
            assert LC.sorted_result(deng.query(sql)) == \
                LC.sorted_result(engines["cpu"].query(sql)), sql
    finally:
        dist.destroy_process_group()


def test_cold_segment(engines):
    """Last in the module: it demotes the GPU engine's oldest segment."""
    eng = engines["cuda"]
    sqls = [LC.ENGINE_SQL[0], LC.ENGINE_SQL[3], LC.ENGINE_SQL[6]]
    want = [LC.sorted_result(eng.query(s)) for s in sqls]
    assert eng.pipe.segments.demote_oldest()
    assert len(eng.pipe.segments.cold) == 1
    assert [LC.sorted_result(eng.query(s)) for s in sqls] == want
    assert want == [LC.sorted_result(engines["cpu"].query(s)) for s in sqls]
