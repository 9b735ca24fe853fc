"""Hand-built segments, plans and a brute-force reference for the K7 query
kernels, shared by test_query_cases_cpu.py and test_query_kernels_gpu.py.

Nothing here goes through the generator, the ingest pipeline or SQL: a case
is an `L7Segment` filled from numpy with a fixed seed plus a `Plan` built
from Term/Key/Agg directly, so every source family, filter op and launch
shape is reachable on purpose.

`ref_agg` / `ref_select` are a per-row pure-Python loop written from the
semantics documented in ops/csrc/dfquery.hip (src_value, eval_terms, the u64
accumulators). They share no code with query/executor.py.
"""
import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from deepflow_amd.ops.ref import mix64
from deepflow_amd.query import spec as Q
from deepflow_amd.query.spec import Agg, Key, Plan, Term
from deepflow_amd.store import l7_schema as S
from deepflow_amd.store.dictionary import str_hash_py
from deepflow_amd.store.kg import KgInfo, KnowledgeGraphTable
from deepflow_amd.store.segment import L7Segment

M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
HASH_SEED = 0x243F6A8885A308D3      # dfquery.hip GROUP_HASH_SEED
HASH_ZERO_KEY = HASH_SEED           # mix64(seed ^ key) == mix64(0) == 0

U64 = {c: i for i, c in enumerate(S.U64_COLS)}
U32 = {c: i for i, c in enumerate(S.U32_COLS)}
U8 = {c: i for i, c in enumerate(S.U8_COLS)}
T0_S = 1_700_000_000                # time base used by the cases


# ------------------------------------------------------------- hashing

def mix64_np(z: np.ndarray) -> np.ndarray:
    """Vectorised ops.ref.mix64 (uint64 arithmetic wraps)."""
    z = z.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def group_hash_np(keys: np.ndarray) -> np.ndarray:
    """Group hash of single-u64-key rows, as the kernels compute it."""
    h = mix64_np(keys.astype(np.uint64) ^ np.uint64(HASH_SEED))
    h[h == 0] = 1
    return h


def group_hash(key: tuple) -> int:
    h = HASH_SEED
    for k, v in enumerate(key):
        h = mix64(h ^ v ^ (k << 56))
    return h or 1


def keys_with_hash_bits(count: int, shift: int, width: int, seed: int,
                        batch: int = 1 << 16) -> np.ndarray:
    """`count` distinct u64 keys whose group hash agrees on the `width`
    bits at `shift` (which value they agree on is left to the search)."""
    rng = np.random.default_rng(seed)
    mask = np.uint64((1 << width) - 1)
    found: List[np.ndarray] = []
    want = None
    have = 0
    while have < count:
        k = rng.integers(1, 1 << 62, size=batch, dtype=np.uint64)
        bits = (group_hash_np(k) >> np.uint64(shift)) & mask
        if want is None:
            want = bits[0]
        hit = np.unique(k[bits == want])
        found.append(hit)
        have = len(np.unique(np.concatenate(found)))
    return np.unique(np.concatenate(found))[:count]


# ------------------------------------------------------------- segments

def u64_t(a) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64))


def u32_t(a) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, dtype=np.uint32).view(np.int32))


def new_segment(n: int, capacity: Optional[int] = None,
                pool_capacity: int = 1 << 15) -> L7Segment:
    seg = L7Segment(capacity or n, "cpu", pool_capacity=pool_capacity)
    seg.n_rows = n
    return seg


def set_u64(seg, col: str, vals) -> None:
    seg.u64[U64[col], :len(vals)] = u64_t(vals)


def set_u32(seg, col: str, vals) -> None:
    seg.u32[U32[col], :len(vals)] = u32_t(vals)


def set_u8(seg, col: str, vals) -> None:
    seg.u8[U8[col], :len(vals)] = torch.from_numpy(
        np.asarray(vals, dtype=np.uint8))


def set_did(seg, idx: int, vals) -> None:
    seg.did[idx, :len(vals)] = u32_t(vals)


def set_strings(seg, rows: List[Dict[int, bytes]]) -> None:
    """rows[i] maps pool column -> bytes (absent = zero length). Row blocks
    are laid out back to back in pool-column order, as K4 writes them."""
    off = 8                                  # not at the pool's very start
    pool = seg.pool.numpy()
    for i, cols in enumerate(rows):
        total = 0
        for c in range(S.N_POOL):
            b = cols.get(c, b"")
            seg.str_lens[c, i] = len(b)
            pool[off + total: off + total + len(b)] = np.frombuffer(
                b, dtype=np.uint8)
            total += len(b)
        seg.str_rowref[i] = S.str_ref_pack(off, total)
        off += total
    assert off <= seg.pool.numel()
    seg.pool_len = off


def set_attrs(seg, rows: List[List[tuple]]) -> None:
    """rows[i] = [(name_id, value_id), ...]: name ids first, then value ids,
    in the row's attr-pool block."""
    off = 3
    for i, pairs in enumerate(rows):
        c = len(pairs)
        seg.attr_start[i] = off
        seg.attr_cnt[i] = c
        for a, (nm, vl) in enumerate(pairs):
            seg.attr_pool[off + a] = nm
            seg.attr_pool[off + c + a] = vl
        off += 2 * c
    assert off <= seg.attr_pool.numel()
    seg.attr_pool_len = off


_TENSORS = ("u64", "u32", "u8", "did", "str_rowref", "str_lens",
            "attr_start", "attr_pool", "attr_cnt", "pool")


def to_device(seg, device: str = "cuda"):
    out = copy.copy(seg)
    out.device = device
    for name in _TENSORS:
        setattr(out, name, getattr(seg, name).to(device))
    return out


def kg_to_device(kg, device: str = "cuda"):
    if kg is None:
        return None
    out = KnowledgeGraphTable(capacity_pow2=kg.capacity, device=device)
    out.update(dict(kg.host))
    return out


# ------------------------------------------------------------ reference

class _Cols:
    def __init__(self, seg):
        self.u64 = seg.u64.numpy().view(np.uint64)
        self.u32 = seg.u32.numpy().view(np.uint32)
        self.u8 = seg.u8.numpy()
        self.did = seg.did.numpy().view(np.uint32)
        self.attr_start = seg.attr_start.numpy()
        self.attr_cnt = seg.attr_cnt.numpy()
        self.attr_pool = seg.attr_pool.numpy().view(np.uint32)
        self.rowref = seg.str_rowref.numpy().view(np.uint64)
        self.lens = seg.str_lens.numpy().view(np.uint16)
        self.pool = seg.pool.numpy().tobytes()


def _pool_hash(c: _Cols, row: int, idx: int) -> int:
    ln = int(c.lens[idx, row])
    if ln == 0:
        return 0
    off = int(c.rowref[row]) >> 16
    for j in range(idx):
        off += int(c.lens[j, row])
    return str_hash_py(c.pool[off:off + ln], Q.STR_FILTER_SEED)


def ref_value(c: _Cols, row: int, family: int, idx: int, bucket: int,
              time_base_s: int, kg) -> int:
    if family == Q.SRC_U64:
        return int(c.u64[idx, row])
    if family == Q.SRC_U32:
        return int(c.u32[idx, row])
    if family == Q.SRC_U8:
        return int(c.u8[idx, row])
    if family == Q.SRC_DID:
        return int(c.did[idx, row])
    if family == Q.SRC_KG:
        if kg is None:
            return 0
        side, j = divmod(idx, S.N_KG)
        info = kg.host.get((int(c.u32[3 + side, row]),
                            int(c.u32[1 + side, row])))
        return 0 if info is None else info.as_list()[j] & M32
    if family == Q.SRC_ATTR_VAL:
        cnt = int(c.attr_cnt[row])
        if idx >= cnt:
            return M32
        return int(c.attr_pool[int(c.attr_start[row]) + cnt + idx])
    if family == Q.SRC_TIME_BUCKET:
        t_s = int(c.u64[U64["start_time"], row]) // 10**9
        rel = t_s - time_base_s if t_s > time_base_s else 0
        return (rel // bucket) * bucket if bucket else rel
    if family == Q.SRC_STR_HASH:
        return _pool_hash(c, row, idx)
    if family == Q.SRC_TRACE128:
        if idx == 0:
            hi = int(c.u64[U64["trace_id_hi"], row])
            lo = int(c.u64[U64["trace_id_lo"], row])
            if hi | lo:
                return mix64(hi) ^ lo
            return _pool_hash(c, row, S.POOL_POS["trace_id"])
        sv = int(c.u64[U64["span_id_b"], row])
        return sv if sv else _pool_hash(c, row, S.POOL_POS["span_id"])
    return 0                                   # SRC_CONST0 and unknown


def _term_ok(c: _Cols, row: int, t: Term, time_base_s: int, kg) -> bool:
    v0, v1 = t.v0 & M64, t.v1 & M64
    if t.family == Q.SRC_ATTR_MATCH:
        cnt = int(c.attr_cnt[row])
        st = int(c.attr_start[row])
        ok = any(int(c.attr_pool[st + a]) == (v0 & M32) and
                 int(c.attr_pool[st + cnt + a]) == (v1 & M32)
                 for a in range(cnt))
        return not ok if t.op == Q.OP_NE else ok
    v = ref_value(c, row, t.family, t.idx, 0, time_base_s, kg)
    if t.op == Q.OP_EQ:
        return v == v0
    if t.op == Q.OP_NE:
        return v != v0
    if t.op == Q.OP_LT:
        return v < v0
    if t.op == Q.OP_LE:
        return v <= v0
    if t.op == Q.OP_GT:
        return v > v0
    if t.op == Q.OP_GE:
        return v >= v0
    if t.op == Q.OP_BETWEEN:
        return v0 <= v <= v1
    return True


def ref_match(c: _Cols, row: int, plan: Plan, kg) -> bool:
    """CNF: group-0 terms AND; every other present group needs one hit."""
    need, have = set(), set()
    for t in plan.terms:
        ok = _term_ok(c, row, t, plan.time_base_s, kg)
        if t.group == 0:
            if not ok:
                return False
        else:
            need.add(t.group)
            if ok:
                have.add(t.group)
    return need == have


def ref_agg(plan: Plan, segs, kg=None, ranges=None) -> Dict[tuple, List[int]]:
    """{raw key tuple: [aggregate, ...]} over rows [base, base + n) of each
    segment (default: all n_rows)."""
    out: Dict[tuple, List[int]] = {}
    for si, seg in enumerate(segs):
        base, n = ranges[si] if ranges else (0, seg.n_rows)
        c = _Cols(seg)
        for row in range(base, base + n):
            if not ref_match(c, row, plan, kg):
                continue
            key = tuple(ref_value(c, row, k.family, k.idx, k.bucket,
                                  plan.time_base_s, kg) for k in plan.keys)
            acc = out.get(key)
            if acc is None:
                acc = out[key] = [M64 if a.op == Q.AGGOP_MIN else 0
                                  for a in plan.aggs]
            for ai, a in enumerate(plan.aggs):
                if a.op == Q.AGGOP_COUNT:
                    acc[ai] = (acc[ai] + 1) & M64
                    continue
                v = ref_value(c, row, a.family, a.idx, 0, plan.time_base_s,
                              kg)
                if a.op == Q.AGGOP_SUM:
                    acc[ai] = (acc[ai] + v) & M64
                elif a.op == Q.AGGOP_MIN:
                    acc[ai] = min(acc[ai], v)
                else:
                    acc[ai] = max(acc[ai], v)
    return out


def ref_select(plan: Plan, seg, base_row: int = 0, n: Optional[int] = None,
               kg=None) -> set:
    n = seg.n_rows - base_row if n is None else n
    c = _Cols(seg)
    return {row for row in range(base_row, base_row + n)
            if ref_match(c, row, plan, kg)}


# ----------------------------------------------------------------- cases

@dataclass
class Case:
    name: str
    plan: Plan
    segs: list
    kg: object = None
    extra: dict = field(default_factory=dict)


def plan(terms=(), keys=(), aggs=(), time_base_s=T0_S) -> Plan:
    return Plan(terms=list(terms), keys=list(keys), aggs=list(aggs),
                time_base_s=time_base_s)


COUNT = Agg(Q.AGGOP_COUNT)
ALL_OPS = [Q.OP_EQ, Q.OP_NE, Q.OP_LT, Q.OP_LE, Q.OP_GT, Q.OP_GE]

# ---- filter matrix: 600 rows (not a multiple of the 256-thread block)
FILTER_ROWS = 600
# family -> (column index, pivot, type max)
FILTER_FAMILIES = {
    Q.SRC_U64: (U64["rrt"], 1000, M64),
    Q.SRC_U32: (U32["response_code"], 1000, M32),
    Q.SRC_U8: (U8["response_status"], 100, 0xFF),
    Q.SRC_DID: (2, 1000, M32),             # 0xFFFFFFFF is a stored -1
}


def filter_values(family: int) -> List[int]:
    _, p, mx = FILTER_FAMILIES[family]
    vals = [0, 1, p - 1, p, p + 1, mx - 1, mx]
    if family == Q.SRC_U64:
        vals += [(1 << 63) - 1, 1 << 63, (1 << 63) + 1]
    return vals


def filter_segment() -> L7Segment:
    rng = np.random.default_rng(600)
    seg = new_segment(FILTER_ROWS)
    for fam, (col, _, _) in FILTER_FAMILIES.items():
        vals = np.array(filter_values(fam), dtype=np.uint64)
        pick = vals[rng.integers(0, len(vals), FILTER_ROWS)]
        if fam == Q.SRC_U64:
            seg.u64[col, :FILTER_ROWS] = u64_t(pick)
        elif fam == Q.SRC_U32:
            seg.u32[col, :FILTER_ROWS] = u32_t(pick.astype(np.uint32))
        elif fam == Q.SRC_U8:
            seg.u8[col, :FILTER_ROWS] = torch.from_numpy(
                pick.astype(np.uint8))
        else:
            seg.did[col, :FILTER_ROWS] = u32_t(pick.astype(np.uint32))
    return seg


def filter_terms(family: int) -> List[Term]:
    """Every op x every edge value, plus the BETWEEN pairs."""
    col, p, mx = FILTER_FAMILIES[family]
    terms = [Term(family, col, op, v0)
             for op in ALL_OPS for v0 in filter_values(family)]
    pairs = [(p, p), (p + 1, p - 1), (p - 1, p + 1), (0, mx), (1, mx - 1),
             (0, 0), (mx, mx)]
    if family == Q.SRC_U64:
        pairs += [(1 << 63, M64), (1, 1 << 63), ((1 << 63) + 1, (1 << 63) - 1)]
    terms += [Term(family, col, Q.OP_BETWEEN, a, b) for a, b in pairs]
    return terms


# ---- CNF and attribute matching
ATTR_NAME, ATTR_VAL = 7, 70


def cnf_segment() -> L7Segment:
    n = 600
    rng = np.random.default_rng(16)
    seg = new_segment(n)
    set_u64(seg, "rrt", rng.integers(0, 50, n))
    set_u64(seg, "flow_id", rng.integers(0, 4, n))
    set_u32(seg, "response_code", rng.choice([200, 404, 500, 503], n))
    set_u32(seg, "server_port", rng.choice([80, 443, 8080], n))
    set_u8(seg, "response_status", rng.integers(0, 5, n))
    set_u8(seg, "l7_protocol", rng.choice([20, 21, 40], n))
    set_did(seg, 1, rng.integers(0, 6, n))
    attrs = []
    for i in range(n):
        cnt = (0, 1, 8)[i % 3]
        pairs = [(int(rng.integers(5, 9)), int(rng.integers(68, 72)))
                 for _ in range(cnt)]
        attrs.append(pairs)
    set_attrs(seg, attrs)
    return seg


def cnf_plans() -> Dict[str, Plan]:
    rc, port = U32["response_code"], U32["server_port"]
    st, proto = U8["response_status"], U8["l7_protocol"]
    sixteen = [
        Term(Q.SRC_U64, U64["rrt"], Q.OP_LT, 45),
        Term(Q.SRC_U64, U64["rrt"], Q.OP_GE, 2),
        Term(Q.SRC_U8, st, Q.OP_NE, 4),
        Term(Q.SRC_DID, 1, Q.OP_LE, 4),
        Term(Q.SRC_U32, rc, Q.OP_EQ, 200, group=1),
        Term(Q.SRC_U32, rc, Q.OP_EQ, 500, group=1),
        Term(Q.SRC_U32, rc, Q.OP_EQ, 503, group=1),
        Term(Q.SRC_U32, port, Q.OP_EQ, 80, group=2),
        Term(Q.SRC_U32, port, Q.OP_GT, 1000, group=2),
        Term(Q.SRC_U8, proto, Q.OP_EQ, 20, group=3),
        Term(Q.SRC_U8, proto, Q.OP_EQ, 40, group=3),
        Term(Q.SRC_U64, U64["flow_id"], Q.OP_BETWEEN, 1, 2, group=3),
        Term(Q.SRC_U64, U64["flow_id"], Q.OP_GE, 0),
        Term(Q.SRC_U8, st, Q.OP_LE, 3),
        Term(Q.SRC_U32, rc, Q.OP_NE, 404),
        Term(Q.SRC_DID, 1, Q.OP_GE, 0),
    ]
    assert len(sixteen) == Q.QMAX_TERMS
    match_eq = Term(Q.SRC_ATTR_MATCH, 0, Q.OP_EQ, ATTR_NAME, ATTR_VAL)
    match_ne = Term(Q.SRC_ATTR_MATCH, 0, Q.OP_NE, ATTR_NAME, ATTR_VAL)
    in_group = lambda t, g: Term(t.family, t.idx, t.op, t.v0, t.v1, group=g)
    keys = [Key(Q.SRC_U8, st)]
    return {
        "sixteen_terms": plan(sixteen, keys, [COUNT]),
        # group 2 can never hit: the whole result is empty
        "dead_group": plan([Term(Q.SRC_U8, st, Q.OP_LE, 3),
                            Term(Q.SRC_U32, rc, Q.OP_EQ, 200, group=1),
                            Term(Q.SRC_U32, rc, Q.OP_EQ, 500, group=1),
                            Term(Q.SRC_U32, port, Q.OP_EQ, 81, group=2),
                            Term(Q.SRC_CONST0, 0, Q.OP_EQ, 1, group=2)],
                           keys, [COUNT]),
        "attr_eq_and": plan([match_eq], keys, [COUNT]),
        "attr_ne_and": plan([match_ne], keys, [COUNT]),
        "attr_eq_or": plan([in_group(match_eq, 1),
                            Term(Q.SRC_U32, rc, Q.OP_EQ, 503, group=1)],
                           keys, [COUNT]),
        "attr_ne_or": plan([in_group(match_ne, 2),
                            Term(Q.SRC_U32, rc, Q.OP_EQ, 503, group=2),
                            Term(Q.SRC_U8, st, Q.OP_GE, 1, group=1)],
                           keys, [COUNT]),
    }


# ---- source families: ~1000 rows, <= 64 groups per plan
def sources_case() -> Case:
    n = 1000
    rng = np.random.default_rng(1000)
    seg = new_segment(n)
    # start_time: a third of the rows lie before the time base
    t_s = T0_S + rng.integers(-120, 600, n)
    set_u64(seg, "start_time", t_s.astype(np.uint64) * np.uint64(10**9) +
            rng.integers(0, 10**9, n).astype(np.uint64))
    # MIN/MAX/SUM operands: rrt has 0 and 2^64-1; end_time is all zero
    rrt = rng.integers(0, 1 << 40, n).astype(np.uint64)
    rrt[rng.integers(0, n, 40)] = 0
    rrt[rng.integers(0, n, 40)] = M64
    set_u64(seg, "rrt", rrt)
    set_u64(seg, "flow_id", rng.integers(0, 1 << 50, n))
    set_u32(seg, "response_length", rng.integers(0, 1 << 32, n))
    set_u32(seg, "server_port", rng.choice([80, 443, 8080, 65535], n))
    set_u8(seg, "response_status", rng.integers(0, 5, n))
    set_u8(seg, "l7_protocol", rng.choice([20, 21, 40], n))
    did = rng.integers(0, 5, n).astype(np.int64)
    did[rng.integers(0, n, 200)] = -1
    set_did(seg, 2, did.astype(np.uint32))
    # KG join keys: 8 known (epc, ip) pairs, the rest miss
    ips = 0x0A000000 + rng.integers(0, 12, n)
    set_u32(seg, "ip4_0", ips)
    set_u32(seg, "ip4_1", 0x0A000000 + rng.integers(0, 12, n))
    set_u32(seg, "l3_epc_id_0", 1 + (ips % 2))
    set_u32(seg, "l3_epc_id_1", np.ones(n))
    kg = KnowledgeGraphTable(capacity_pow2=64, device="cpu")
    kg.update({(1 + (ip % 2), ip): KgInfo(pod_id=100 + ip % 8,
                                          service_id=1 + ip % 3,
                                          az_id=7)
               for ip in range(0x0A000000, 0x0A000008)})
    # binary ids: a third zero (string fallback), a third of those with an
    # empty string too
    hi = rng.integers(1, 6, n).astype(np.uint64)
    lo = rng.integers(1, 4, n).astype(np.uint64)
    span = rng.integers(1, 9, n).astype(np.uint64)
    strings = []
    tpos, spos = S.POOL_POS["trace_id"], S.POOL_POS["span_id"]
    epos, upos = S.POOL_POS["exception_desc"], S.POOL_POS["http_user_agent"]
    for i in range(n):
        cols = {}
        if i % 3 == 0:
            hi[i] = lo[i] = 0
            span[i] = 0
            if i % 9:
                cols[tpos] = b"trace-%d" % (i % 5)
                cols[spos] = b"sp%d" % (i % 4)
        elif i % 3 == 1:
            hi[i] = 0                           # hi == 0, lo != 0: binary
            cols[tpos] = b"ignored-%d" % i
        if i % 4:                               # zero length on every 4th
            cols[upos] = (b"agent/%d " % (i % 6)) * (1 + i % 3)
        if i % 5 == 0:                          # shifts the later columns
            cols[epos] = b"E" * (i % 13)
        strings.append(cols)
    set_u64(seg, "trace_id_hi", hi)
    set_u64(seg, "trace_id_lo", lo)
    set_u64(seg, "span_id_b", span)
    set_strings(seg, strings)
    set_attrs(seg, [[(int(rng.integers(5, 9)), int(rng.integers(68, 72)))
                     for _ in range((0, 1, 3, 8)[i % 4])]
                    for i in range(n)])
    return Case("sources", plan(), [seg], kg)


def source_plans() -> Dict[str, Plan]:
    """name -> plan; names ending in _nokg run with kg=None."""
    rrt, zero = U64["rrt"], U64["end_time"]
    aggs4 = [COUNT, Agg(Q.AGGOP_SUM, Q.SRC_U32, U32["response_length"]),
             Agg(Q.AGGOP_MIN, Q.SRC_U64, rrt),
             Agg(Q.AGGOP_MAX, Q.SRC_U64, rrt)]
    aggs8 = aggs4 + [Agg(Q.AGGOP_MAX, Q.SRC_U64, zero),
                     Agg(Q.AGGOP_MIN, Q.SRC_U64, zero),
                     Agg(Q.AGGOP_SUM, Q.SRC_U64, U64["flow_id"]),
                     Agg(Q.AGGOP_MAX, Q.SRC_ATTR_VAL, 2)]
    one = lambda k: plan([], [k], aggs4)
    return {
        "attr_val_slot0": one(Key(Q.SRC_ATTR_VAL, 0)),
        "attr_val_slot2": one(Key(Q.SRC_ATTR_VAL, 2)),   # idx >= cnt often
        "attr_val_slot9": one(Key(Q.SRC_ATTR_VAL, 9)),   # idx >= cnt always
        "did_minus_one": one(Key(Q.SRC_DID, 2)),
        "kg_side0_pod": one(Key(Q.SRC_KG, 0)),
        "kg_side1_service": one(Key(Q.SRC_KG, S.N_KG + 10)),
        "kg_pod_nokg": one(Key(Q.SRC_KG, 0)),
        "str_hash_user_agent": one(Key(Q.SRC_STR_HASH,
                                       S.POOL_POS["http_user_agent"])),
        "trace128_trace": one(Key(Q.SRC_TRACE128, 0)),
        "trace128_span": one(Key(Q.SRC_TRACE128, 1)),
        "time_bucket_60": one(Key(Q.SRC_TIME_BUCKET, 0, 60)),
        "time_bucket_1": plan([Term(Q.SRC_TIME_BUCKET, 0, Q.OP_LT, 50)],
                              [Key(Q.SRC_TIME_BUCKET, 0, 1)], aggs4),
        "time_bucket_0": plan([Term(Q.SRC_TIME_BUCKET, 0, Q.OP_LT, 50)],
                              [Key(Q.SRC_TIME_BUCKET, 0, 0)], aggs4),
        "str_hash_filter": plan(
            [Term(Q.SRC_STR_HASH, S.POOL_POS["http_user_agent"], Q.OP_EQ,
                  str_hash_py(b"agent/1 agent/1 ", Q.STR_FILTER_SEED))],
            [Key(Q.SRC_U8, U8["response_status"])], aggs4),
        "str_hash_empty_filter": plan(
            [Term(Q.SRC_STR_HASH, S.POOL_POS["http_user_agent"], Q.OP_EQ,
                  0)], [Key(Q.SRC_U8, U8["response_status"])], aggs4),
        "four_keys_eight_aggs": plan(
            [Term(Q.SRC_U32, U32["server_port"], Q.OP_NE, 65535),
             Term(Q.SRC_DID, 2, Q.OP_LE, 1)],
            [Key(Q.SRC_U8, U8["l7_protocol"]), Key(Q.SRC_DID, 2),
             Key(Q.SRC_KG, S.N_KG + 10), Key(Q.SRC_TIME_BUCKET, 0, 300)],
            aggs8),
        "keyless_eight_aggs": plan([], [], aggs8),
    }


def sum_wrap_case() -> Case:
    """2^63 + 2^63 == 0 in a u64 accumulator; a second group stays below."""
    seg = new_segment(5)
    set_u64(seg, "flow_id", [1, 1, 2, 2, 2])
    set_u64(seg, "rrt", [1 << 63, 1 << 63, M64, 1, 5])
    p = plan([], [Key(Q.SRC_U64, U64["flow_id"])],
             [Agg(Q.AGGOP_SUM, Q.SRC_U64, U64["rrt"]), COUNT])
    return Case("sum_wrap", p, [seg],
                extra={"want": {(1,): [0, 2], (2,): [5, 3]}})


def _agg_plan_u64_key() -> Plan:
    rrt = U64["rrt"]
    return plan([], [Key(Q.SRC_U64, U64["flow_id"])],
                [COUNT, Agg(Q.AGGOP_SUM, Q.SRC_U64, rrt),
                 Agg(Q.AGGOP_MIN, Q.SRC_U64, rrt),
                 Agg(Q.AGGOP_MAX, Q.SRC_U64, rrt)])


def hash_zero_case() -> Case:
    n = 700
    rng = np.random.default_rng(243)
    seg = new_segment(n)
    keys = np.array([HASH_ZERO_KEY, 0, 1, 5, M64, 1 << 63], dtype=np.uint64)
    set_u64(seg, "flow_id", keys[rng.integers(0, len(keys), n)])
    set_u64(seg, "rrt", rng.integers(1, 1 << 30, n))
    assert group_hash((HASH_ZERO_KEY,)) == 1 and mix64(0) == 0
    return Case("hash_zero", _agg_plan_u64_key(), [seg])


def lds_spill_case() -> Case:
    """40 keys whose group hash shares its low 9 bits (one LDS probe chain
    of 40 > the 16-probe limit) round-robin in block 0; later blocks hold
    subsets that fit, so LDS and global paths feed the same groups."""
    n = 1024
    rng = np.random.default_rng(512)
    chain = keys_with_hash_bits(40, 0, 9, seed=9)
    assert len(set((group_hash_np(chain) & np.uint64(511)).tolist())) == 1
    ordinary = np.arange(1000, 1030, dtype=np.uint64)
    col = np.empty(n, dtype=np.uint64)
    col[:256] = chain[np.arange(256) % 40]
    col[256:512] = np.where(np.arange(256) % 2 == 0,
                            chain[np.arange(256) % 10],
                            ordinary[np.arange(256) % 30])
    col[512:768] = np.where(np.arange(256) % 2 == 0,
                            chain[30 + np.arange(256) % 10],
                            ordinary[np.arange(256) % 30])
    col[768:] = np.concatenate([chain, ordinary])[rng.integers(0, 70, 256)]
    seg = new_segment(n)
    set_u64(seg, "flow_id", col)
    set_u64(seg, "rrt", rng.integers(0, 1 << 40, n))
    return Case("lds_spill", _agg_plan_u64_key(), [seg],
                extra={"chain": chain})


def multi_segment_case() -> Case:
    """Three segments of different sizes and capacities sharing keys."""
    rng = np.random.default_rng(3)
    segs = []
    for n, cap, lo in ((257, 300, 0), (1, 4, 3), (900, 1024, 2)):
        seg = new_segment(n, capacity=cap)
        set_u64(seg, "flow_id", rng.integers(lo, lo + 6, n))
        # MIN must survive later launches: the smallest values sit in the
        # first segment, larger ones follow
        set_u64(seg, "rrt", rng.integers(1 + 1000 * len(segs),
                                         1 << (20 + 10 * len(segs)), n))
        segs.append(seg)
    return Case("multi_segment", _agg_plan_u64_key(), segs)


def geometry_segment() -> L7Segment:
    """700 rows; see geometry_fill: rows outside the launched range carry
    values that would change every aggregate."""
    rng = np.random.default_rng(700)
    seg = new_segment(700)
    set_u64(seg, "flow_id", rng.integers(0, 5, 700))
    set_u64(seg, "rrt", rng.integers(1000, 2000, 700))
    return seg


def geometry_poison(seg, base_row: int, n: int) -> L7Segment:
    """Copy of seg whose rows outside [base_row, base_row + n) hold rrt 0
    (breaks MIN), then 2^63 (breaks MAX and SUM); COUNT breaks either way."""
    out = copy.copy(seg)
    out.u64 = seg.u64.clone()
    rrt = out.u64[U64["rrt"]]
    outside = torch.ones(seg.capacity, dtype=torch.bool)
    outside[base_row:base_row + n] = False
    idx = torch.nonzero(outside).flatten()
    rrt[idx[0::2]] = 0
    rrt[idx[1::2]] = -(1 << 63)
    return out


def overflow_case() -> Case:
    """200 distinct keys for a 64-slot group table."""
    n = 1000
    rng = np.random.default_rng(64)
    seg = new_segment(n)
    keys = rng.permutation(np.arange(5000, 5200, dtype=np.uint64))
    col = np.concatenate([keys, keys[rng.integers(0, 200, n - 200)]])
    set_u64(seg, "flow_id", col)
    set_u64(seg, "rrt", rng.integers(1, 1 << 30, n))
    return Case("overflow", _agg_plan_u64_key(), [seg])


def select_segment() -> L7Segment:
    rng = np.random.default_rng(77)
    seg = new_segment(700)
    set_u8(seg, "response_status", rng.integers(0, 4, 700))
    set_u32(seg, "response_code", rng.choice([200, 500], 700))
    return seg


def select_plan() -> Plan:
    return plan([Term(Q.SRC_U8, U8["response_status"], Q.OP_GE, 1),
                 Term(Q.SRC_U32, U32["response_code"], Q.OP_EQ, 500)])


def cpu_agg_cases() -> List[Case]:
    """Every aggregate case small enough for the CPU engine's row loop."""
    out = [sum_wrap_case(), hash_zero_case(), lds_spill_case(),
           multi_segment_case(), overflow_case()]
    src = sources_case()
    for name, p in source_plans().items():
        out.append(Case("src_" + name, p, src.segs,
                        None if name.endswith("_nokg") else src.kg))
    cnf = cnf_segment()
    for name, p in cnf_plans().items():
        out.append(Case("cnf_" + name, p, [cnf]))
    return out
