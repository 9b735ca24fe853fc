"""QuerySpec ABI — ctypes mirror of dfquery.hip's QTerm/QKey/QAgg/QuerySpec.

tests/test_query_spec.py validates sizeof against df_spec_sizes() so the two
sides cannot drift silently.
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field
from typing import List, Optional

QMAX_TERMS = 16
QMAX_KEYS = 4
QMAX_AGGS = 8
# K15 distinct counts: a second POD next to QuerySpec (which must not grow)
QMAX_UNIQ = 4
QMAX_UNIQ_ARGS = 4

# source families (dfquery.hip enum)
SRC_U64 = 0
SRC_U32 = 1
SRC_U8 = 2
SRC_DID = 3
SRC_KG = 4
SRC_ATTR_VAL = 5
SRC_TIME_BUCKET = 6
SRC_CONST0 = 7
SRC_STR_HASH = 8
SRC_ATTR_MATCH = 9  # filter-only: attr name_id == v0 AND value_id == v1
# binary-transcoded OTel ids: idx 0 = trace_id (mix64(hi)^lo), 1 = span_id;
# zero binary cols fall back to the pooled-string hash (non-hex ids)
SRC_TRACE128 = 10

# seed for pooled-string filter hashing (twin: dfseg.h STR_FILTER_SEED)
STR_FILTER_SEED = 0x5157A15E5EED

# seed of the Uniq pair hash (twin: dfquery.hip UNIQ_SEED; the formula is in
# k_query_uniq's comment)
UNIQ_SEED = 0x13198A2E03707344
# families src_value reads for a Uniq argument (SRC_ATTR_VAL is per-slot,
# not per-name, and SRC_ATTR_MATCH is a filter)
UNIQ_FAMILIES = frozenset((SRC_U64, SRC_U32, SRC_U8, SRC_DID, SRC_KG,
                           SRC_STR_HASH, SRC_TRACE128, SRC_TIME_BUCKET))

OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_BETWEEN = range(7)
# K16 set membership (LIKE / REGEXP on dictionary tags): in the kernel spec
# v0 is the device address of a u32 bitmap and v1 its length in bits; in a
# Plan, until it is bound, v0 indexes Plan.sets. A value outside the bitmap
# (DICT_ID_INVALID among them) is not a member.
OP_INSET, OP_NOT_INSET = 7, 8
SET_OPS = (OP_INSET, OP_NOT_INSET)
# the largest id a host-built (kgname) set may hold: bitmaps stay <= 8 MiB
SET_MAX_BITS = 1 << 26
AGGOP_COUNT, AGGOP_SUM, AGGOP_MIN, AGGOP_MAX = range(4)

OP_BY_NAME = {"=": OP_EQ, "==": OP_EQ, "!=": OP_NE, "<>": OP_NE, "<": OP_LT,
              "<=": OP_LE, ">": OP_GT, ">=": OP_GE}


class QTermC(ct.Structure):
    _fields_ = [("family", ct.c_uint8), ("op", ct.c_uint8),
                ("idx", ct.c_uint16), ("group", ct.c_uint8),
                ("v0", ct.c_uint64), ("v1", ct.c_uint64)]


class QKeyC(ct.Structure):
    _fields_ = [("family", ct.c_uint8), ("idx", ct.c_uint16),
                ("bucket", ct.c_uint32)]


class QAggC(ct.Structure):
    _fields_ = [("op", ct.c_uint8), ("family", ct.c_uint8),
                ("idx", ct.c_uint16)]


class QuerySpecC(ct.Structure):
    _fields_ = [("terms", QTermC * QMAX_TERMS),
                ("keys", QKeyC * QMAX_KEYS),
                ("aggs", QAggC * QMAX_AGGS),
                ("n_terms", ct.c_uint32), ("n_keys", ct.c_uint32),
                ("n_aggs", ct.c_uint32),
                ("time_base_s", ct.c_uint64)]


class QUniqColC(ct.Structure):
    _fields_ = [("family", ct.c_uint8), ("idx", ct.c_uint16)]


class QUniqC(ct.Structure):
    _fields_ = [("cols", QUniqColC * QMAX_UNIQ_ARGS),
                ("n_args", ct.c_uint32)]


class UniqSpecC(ct.Structure):
    _fields_ = [("items", QUniqC * QMAX_UNIQ), ("n_uniq", ct.c_uint32)]


@dataclass
class Term:
    family: int
    idx: int
    op: int
    v0: int
    v1: int = 0
    group: int = 0  # 0 = AND; >=1 = member of that OR-clause


@dataclass
class Key:
    family: int
    idx: int
    bucket: int = 0  # seconds per bucket for SRC_TIME_BUCKET


@dataclass
class Agg:
    op: int
    family: int = SRC_CONST0
    idx: int = 0


@dataclass
class Uniq:
    """One Uniq/UniqExact item: the (family, idx) columns of its value
    tuple, in argument order."""
    cols: List[tuple] = field(default_factory=list)


@dataclass(eq=False)
class PatternSet:
    """Host description of one id set behind an OP_INSET / OP_NOT_INSET
    term: the ids of a dictionary domain (or of a name map) whose string
    matches a pattern, or, with `complement`, whose string does not. The
    executor turns it into a bitmap on the plan's device before the first
    launch (executor.bind_sets)."""
    kind: str                       # 'like' | 'regexp'
    pattern: str                    # as written in the query
    regex: str                      # what is evaluated (LIKE: translated)
    rx: object                      # logregex.LogRegex: DFA + host `re`
    complement: bool = False
    domain: Optional[int] = None    # dict:<domain> tags
    dictionary: object = None       # the shard's TagDictionary
    name_map: Optional[dict] = None  # kgname tags: id -> display name

    def host_matches(self, value: bytes) -> bool:
        """Python `re` on one string: the oracle of the DFA walk."""
        if self.kind == "like":
            return self.rx.host.fullmatch(value) is not None
        return self.rx.host.search(value) is not None

    def __deepcopy__(self, memo):
        return self                 # never copy a dictionary with a plan


@dataclass
class Plan:
    table: str = "l7_flow_log"
    terms: List[Term] = field(default_factory=list)
    keys: List[Key] = field(default_factory=list)
    aggs: List[Agg] = field(default_factory=list)
    time_base_s: int = 0
    # host-side metadata (not part of the kernel spec)
    key_names: List[str] = field(default_factory=list)
    agg_names: List[str] = field(default_factory=list)
    key_meta: List[dict] = field(default_factory=list)  # hydration info
    agg_meta: List[dict] = field(default_factory=list)
    order_by: Optional[List] = None
    having: Optional[List] = None  # [(column, op, number)] post-agg
    limit: Optional[int] = None
    slimit: Optional[int] = None
    select_rows: bool = False  # non-aggregated SELECT
    select_cols: List[str] = field(default_factory=list)
    impossible: bool = False   # filter references unknown dict string
    # distinct-count items; each also owns an AGGOP_COUNT placeholder in
    # `aggs` (as percentile does) so agg_meta walks stay aligned
    uniqs: List[Uniq] = field(default_factory=list)
    # K16: the id sets of OP_INSET / OP_NOT_INSET terms (Term.v0 indexes
    # this list), and what the executor bound them to, per device:
    # {device: (bitmaps, [(address, bits), ...])}. The bitmaps live as long
    # as the plan does, which is longer than any launch of its query.
    sets: List[PatternSet] = field(default_factory=list)
    bound: dict = field(default_factory=dict)

    def has_sets(self) -> bool:
        return any(t.op in SET_OPS for t in self.terms)

    def to_bytes(self, sets=None) -> bytes:
        """The kernel spec. `sets`: [(device address, bits)] per entry of
        self.sets; a plan with set terms does not serialise without it (an
        index must never travel as if it were a pointer)."""
        c = QuerySpecC()
        assert len(self.terms) <= QMAX_TERMS
        assert len(self.keys) <= QMAX_KEYS
        assert len(self.aggs) <= QMAX_AGGS
        for i, t in enumerate(self.terms):
            v0, v1 = t.v0, t.v1
            if t.op in SET_OPS:
                if sets is None:
                    raise RuntimeError(
                        "plan has LIKE/REGEXP set terms that are not bound "
                        "to device bitmaps (executor.bind_sets)")
                v0, v1 = sets[t.v0]
            c.terms[i] = QTermC(family=t.family, op=t.op, idx=t.idx,
                                group=getattr(t, "group", 0),
                                v0=v0 & (2**64 - 1), v1=v1 & (2**64 - 1))
        for i, k in enumerate(self.keys):
            c.keys[i] = QKeyC(family=k.family, idx=k.idx, bucket=k.bucket)
        for i, a in enumerate(self.aggs):
            c.aggs[i] = QAggC(op=a.op, family=a.family, idx=a.idx)
        c.n_terms, c.n_keys, c.n_aggs = (len(self.terms), len(self.keys),
                                         len(self.aggs))
        c.time_base_s = self.time_base_s
        return bytes(memoryview(c))

    def uniq_to_bytes(self) -> bytes:
        c = UniqSpecC()
        assert len(self.uniqs) <= QMAX_UNIQ
        for u, item in enumerate(self.uniqs):
            assert 1 <= len(item.cols) <= QMAX_UNIQ_ARGS
            for j, (family, idx) in enumerate(item.cols):
                c.items[u].cols[j] = QUniqColC(family=family, idx=idx)
            c.items[u].n_args = len(item.cols)
        c.n_uniq = len(self.uniqs)
        return bytes(memoryview(c))
