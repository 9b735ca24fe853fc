"""Shared cases and brute-force references for DF-SQL LIKE / REGEXP on
dictionary tags (K16): test_like_cpu.py and test_like_gpu.py.

The references here work on strings: `like_match` is a wildcard matcher
written from the operator's definition (it uses no regex), REGEXP is
Python's `re.search`. They share no code with query/sql.py's translation,
the DFA compiler, the executor's bitmaps or the kernels.
"""
import re
from typing import Dict, List, Optional

import numpy as np

import query_cases as QC
from deepflow_amd.query import spec as Q
from deepflow_amd.query.spec import Key, Plan, Term
from deepflow_amd.store import l7_schema as S
from deepflow_amd.store.dictionary import TagDictionary

INVALID = S.DICT_ID_INVALID

# ------------------------------------------------- LIKE -> regex, by hand
# (LIKE pattern, the regex it must become, the literal it equals or None)
ANY, ONE = r"[\s\S]*", r"[\s\S]"
LIKE_TABLE = [
    ("%", r"\A" + ANY + r"\Z", None),
    ("*", r"\A" + ANY + r"\Z", None),
    ("_", r"\A" + ONE + r"\Z", None),
    ("a%b*c_d", r"\Aa" + ANY + "b" + ANY + "c" + ONE + r"d\Z", None),
    (r"100\%", r"\A100\%\Z", "100%"),
    (r"a\*b", r"\Aa\*b\Z", "a*b"),
    (r"a\_b", r"\Aa_b\Z", "a_b"),
    (r"a\\b", r"\Aa\\b\Z", "a\\b"),
    (r"\%%", r"\A\%" + ANY + r"\Z", None),
    ("a.b+c(d[e", r"\Aa\.b\+c\(d\[e\Z", "a.b+c(d[e"),
    ("x.%", r"\Ax\." + ANY + r"\Z", None),
    ("", r"\A\Z", ""),
    ("a\nb%", "\\Aa\\\nb" + ANY + r"\Z", None),
    ("/api/v1/*", r"\A\/api\/v1\/" + ANY + r"\Z", None),
]
# (LIKE pattern, value, matches) for the translated regex under `re`
LIKE_VALUES = [
    ("%", b"", True), ("%", b"a\nb", True), ("_", b"\n", True),
    ("_", b"", False), ("_", b"ab", False),
    ("a%b*c_d", b"abcxd", True), ("a%b*c_d", b"a\nb\n\nc\nd", True),
    ("a%b*c_d", b"abcd", False),
    (r"100\%", b"100%", True), (r"100\%", b"1000", False),
    (r"a\*b", b"a*b", True), (r"a\*b", b"axb", False),
    (r"a\_b", b"a_b", True), (r"a\_b", b"axb", False),
    (r"a\\b", b"a\\b", True),
    ("a.b+c(d[e", b"a.b+c(d[e", True), ("a.b+c(d[e", b"axb+c(d[e", False),
    ("x.%", b"x.y", True), ("x.%", b"xzy", False),
    ("", b"", True), ("", b"a", False),
    ("a\nb%", b"a\nb\n", True), ("a\nb%", b"a b", False),
    ("A%", b"abc", False),                      # case-sensitive
    ("%c", b"abc\n", False),                    # anchored: \Z is not $
]


def like_match(pattern: str, value: bytes) -> bool:
    """LIKE by definition: % and * any run of bytes, _ one byte, backslash
    makes the next character literal; the whole value must match."""
    toks = []                                   # 'any' | 'one' | bytes
    i = 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\" and i + 1 < len(pattern):
            i += 1
            toks.append(pattern[i].encode())
        elif c in "%*":
            toks.append("any")
        elif c == "_":
            toks.append("one")
        else:
            toks.append(c.encode())
        i += 1
    # positions of `value` reachable after each token
    reach = {0}
    for t in toks:
        nxt = set()
        for p in reach:
            if t == "any":
                nxt.update(range(p, len(value) + 1))
            elif t == "one":
                if p < len(value):
                    nxt.add(p + 1)
            elif value[p:p + len(t)] == t:
                nxt.add(p + len(t))
        reach = nxt
    return len(value) in reach


def atom_ok(op: str, pattern: str, value: Optional[bytes]) -> bool:
    """One condition on one hydrated value; None (no value) is ''."""
    v = b"" if value is None else value
    if op == "=":
        return value is not None and v == pattern.encode()
    if op == "like":
        return like_match(pattern, v)
    if op == "not like":
        return not like_match(pattern, v)
    hit = re.search(pattern.encode(), v) is not None
    return hit if op == "regexp" else not hit


def cnf_ok(cnf, values: Dict[str, Optional[bytes]]) -> bool:
    """cnf: list of clauses (ANDed), each a list of (tag, op, pattern)
    atoms (ORed)."""
    return all(any(atom_ok(op, pat, values[tag]) for tag, op, pat in clause)
               for clause in cnf)


# ------------------------------------------- hand-built dictionary + rows
DOM_RES, DID_RES = 2, 2            # request_resource: domain 2, did col 2
DOM_DOMAIN, DID_DOMAIN = 1, 1      # request_domain
assert S.DID_COLS[DID_RES][:1] == ("request_resource",) and \
    S.DID_COLS[DID_RES][2] == DOM_RES
assert S.DID_COLS[DID_DOMAIN][2] == DOM_DOMAIN

RES_STRINGS = {3: b"/api/v1/users", 4: b"/api/v1/orders/17", 31: b"/user/12",
               32: b"/user/ab", 33: b"x/api/v1/", 64: b"xylophone",
               100: b"a\nb", 1023: b"/health"}
DOMAIN_STRINGS = {1: b"a.svc.cluster.local", 2: b"example.com",
                  40: b"checkout-7.example.com"}
HAND_CAPACITY = 1 << 10


def hand_dictionary() -> TagDictionary:
    d = TagDictionary(HAND_CAPACITY, device="cpu")
    for dom, strings in ((DOM_RES, RES_STRINGS),
                         (DOM_DOMAIN, DOMAIN_STRINGS)):
        for i, s in strings.items():
            d.id_to_str[(dom, i)] = s
            d.str_to_id[(dom, s)] = i
    return d


def hand_segment(n: int = 300):
    """Rows over every string above plus rows without a value."""
    rng = np.random.default_rng(n)
    seg = QC.new_segment(n)
    res = np.array(list(RES_STRINGS) + [INVALID, INVALID], dtype=np.uint32)
    dom = np.array(list(DOMAIN_STRINGS) + [INVALID], dtype=np.uint32)
    QC.set_did(seg, DID_RES, res[rng.integers(0, len(res), n)])
    QC.set_did(seg, DID_DOMAIN, dom[rng.integers(0, len(dom), n)])
    QC.set_u64(seg, "rrt", rng.integers(0, 50, n))
    return seg


def hand_values(seg, row: int) -> Dict[str, Optional[bytes]]:
    did = seg.did.numpy().view(np.uint32)
    return {"request_resource": RES_STRINGS.get(int(did[DID_RES, row])),
            "request_domain": DOMAIN_STRINGS.get(int(did[DID_DOMAIN, row]))}


def hand_ref_rows(seg, cnf) -> set:
    return {r for r in range(seg.n_rows) if cnf_ok(cnf, hand_values(seg, r))}


R, D = "request_resource", "request_domain"
# (WHERE text, the same condition for the reference)
HAND_WHERE = [
    # rows without a value behave as ''
    (f"{R} LIKE '%'", [[(R, "like", "%")]]),
    (f"{R} LIKE 'x%'", [[(R, "like", "x%")]]),
    (f"{R} NOT LIKE 'x%'", [[(R, "not like", "x%")]]),
    (f"{R} NOT LIKE '%'", [[(R, "not like", "%")]]),
    # no entry, every entry
    (f"{R} LIKE '%nothing-like-this%'", [[(R, "like", "%nothing-like-this%")]]),
    (f"{R} LIKE '%_%'", [[(R, "like", "%_%")]]),
    (f"{R} REGEXP '[a-z]'", [[(R, "regexp", "[a-z]")]]),
    # the operators
    (f"{R} LIKE '*/api/v1/*'", [[(R, "like", "*/api/v1/*")]]),
    (f"{R} LIKE '/user/__'", [[(R, "like", "/user/__")]]),
    (f"{R} LIKE 'a_b'", [[(R, "like", "a_b")]]),
    (f"{R} REGEXP '^/user/[0-9]+$'", [[(R, "regexp", "^/user/[0-9]+$")]]),
    (f"{R} NOT REGEXP '^/user/[0-9]+$'",
     [[(R, "not regexp", "^/user/[0-9]+$")]]),
    (f"{R} REGEXP '^$'", [[(R, "regexp", "^$")]]),
    (f"{R} NOT REGEXP 'a*'", [[(R, "not regexp", "a*")]]),
    (f"{D} NOT LIKE '*.svc.cluster.local'",
     [[(D, "not like", "*.svc.cluster.local")]]),
    (f"{D} LIKE 'checkout-*'", [[(D, "like", "checkout-*")]]),
    # combined
    (f"{R} LIKE '/api/%' AND {D} = 'example.com'",
     [[(R, "like", "/api/%")], [(D, "=", "example.com")]]),
    (f"({R} LIKE '/user/%' OR {R} LIKE 'x%')",
     [[(R, "like", "/user/%"), (R, "like", "x%")]]),
    (f"({R} NOT LIKE '/%' OR {D} REGEXP 'example') AND {D} NOT LIKE 'a%'",
     [[(R, "not like", "/%"), (D, "regexp", "example")],
      [(D, "not like", "a%")]]),
    (f"{D} IN ('example.com', 'a.svc.cluster.local') AND "
     f"{R} not  like '%s'",
     [[(D, "=", "example.com"), (D, "=", "a.svc.cluster.local")],
      [(R, "not like", "%s")]]),
]


# --------------------------------------- dictionaries for k_dict_match
MATCH_SIZES = [1, 63, 64, 65, 256, 257, 1000]
MATCH_CAPACITY = 1 << 12
LONG = b"q" * 4095 + b"Z"


def match_entries(n: int) -> List[tuple]:
    """n (id, bytes) entries, the special ones first. Order is arena
    order: `foo` is followed by an entry that starts with \\n, `..ab` by
    `cd..`."""
    special = [
        (0, b"foo"), (31, b"\nbar"),
        (32, b"xxab"), (63, b"cdxx"),
        (64, b"only-at-the-end-Z"),
        (MATCH_CAPACITY - 1, b"line\n"),
        (65, b"a"), (66, b"ab"), (67, b"/user/7"), (68, b"/user/12"),
        (69, b"/user/123"), (70, b"/u" * 127 + b"Z"), (71, LONG),
        (72, b"foo\n"), (73, b"bc"), (74, b"\n"),
    ]
    assert [len(s) for _, s in special[6:13]] == [1, 2, 7, 8, 9, 255, 4096]
    out = special[:n]
    for i in range(len(out), n):
        kind = i % 3
        s = (b"/api/v1/r/%05d" % i if kind == 0 else
             b"/user/%d" % i if kind == 1 else b"/user/x%d/foo" % i)
        out.append((100 + i, s))
    assert len({i for i, _ in out}) == n
    return out


# regexes for the direct kernel test (compile_log_regex takes them all)
MATCH_PATTERNS = [
    "foo$", "bc", "Z", "Z$", "line$", r"line\Z", "^/user/[0-9]+$", "/api/",
    "^$", "a*", r"\A[\s\S]*\Z", r"\A[\s\S]\Z", r"\Aa[\s\S]*\Z", "^foo",
    r"\A[\s\S]*\/r\/0000[\s\S]\Z", "(ab|cd)x*$", "q{40}Z", "x[0-9]+/foo$",
]


# -------------------------------------------- eval_terms with set terms
SET_BITS = 77                      # not a multiple of 32: a partial word


def set_words() -> np.ndarray:
    """A 77-bit set in 3 words. Bits 77..95 of the last word are all ones:
    an id at or past `bits` must read as 'not a member' whatever the
    memory behind it says."""
    rng = np.random.default_rng(77)
    bits = rng.integers(0, 2, SET_BITS).astype(bool)
    bits[[0, 31, 32, 63, 64, SET_BITS - 1]] = True
    bits[[1, 33, 65]] = False
    words = np.zeros(3, dtype=np.uint32)
    for i in np.nonzero(bits)[0]:
        words[i >> 5] |= np.uint32(1 << (i & 31))
    words[2] |= np.uint32(0xFFFFFFFF << (SET_BITS & 31) & 0xFFFFFFFF)
    return words


def set_members() -> set:
    w = set_words()
    return {i for i in range(SET_BITS) if (int(w[i >> 5]) >> (i & 31)) & 1}


def set_segment(n: int):
    rng = np.random.default_rng(n)
    seg = QC.new_segment(n, capacity=n + 200)
    ids = np.array([0, 1, 31, 32, 33, 63, 64, 65, SET_BITS - 2, SET_BITS - 1,
                    SET_BITS, SET_BITS + 1, 95, 96, 1 << 20, INVALID],
                   dtype=np.uint32)
    QC.set_did(seg, DID_RES, ids[rng.integers(0, len(ids), n)])
    QC.set_u32(seg, "response_code", ids[rng.integers(0, len(ids), n)])
    QC.set_u64(seg, "rrt", rng.integers(0, 50, n))
    QC.set_u8(seg, "response_status", rng.integers(0, 4, n))
    return seg


def set_plans() -> Dict[str, Plan]:
    """Every plan refers to set 0 (set_words())."""
    rc = QC.U32["response_code"]
    keys = [Key(Q.SRC_U8, QC.U8["response_status"])]
    inset = Term(Q.SRC_DID, DID_RES, Q.OP_INSET, 0)
    notin = Term(Q.SRC_DID, DID_RES, Q.OP_NOT_INSET, 0)
    low = Term(Q.SRC_U64, QC.U64["rrt"], Q.OP_LT, 10)
    g = lambda t, k: Term(t.family, t.idx, t.op, t.v0, t.v1, group=k)
    return {
        "inset": QC.plan([inset], keys, [QC.COUNT]),
        "not_inset": QC.plan([notin], keys, [QC.COUNT]),
        "inset_u32": QC.plan([Term(Q.SRC_U32, rc, Q.OP_INSET, 0)], keys,
                             [QC.COUNT]),
        "inset_and": QC.plan([inset, low], keys, [QC.COUNT]),
        "inset_or": QC.plan([g(inset, 1), g(low, 1)], keys, [QC.COUNT]),
        "two_groups": QC.plan([g(notin, 1), g(low, 1),
                               g(Term(Q.SRC_U32, rc, Q.OP_NOT_INSET, 0), 2),
                               g(inset, 2)], keys, [QC.COUNT]),
    }


def _set_term_ok(c, row: int, t: Term, members: set) -> bool:
    if t.op in (Q.OP_INSET, Q.OP_NOT_INSET):
        v = QC.ref_value(c, row, t.family, t.idx, 0, 0, None)
        return (v in members) == (t.op == Q.OP_INSET)
    return QC._term_ok(c, row, t, 0, None)


def set_ref_rows(plan: Plan, seg, base_row: int, n: int) -> List[int]:
    """Rows of [base_row, base_row + n) the plan's CNF lets through."""
    c = QC._Cols(seg)
    members = set_members()
    out = []
    for row in range(base_row, base_row + n):
        need, have, ok = set(), set(), True
        for t in plan.terms:
            hit = _set_term_ok(c, row, t, members)
            if t.group == 0:
                ok = ok and hit
            else:
                need.add(t.group)
                if hit:
                    have.add(t.group)
        if ok and need == have:
            out.append(row)
    return out


# ---------------------------------------------- SQL over generated spans
# (uniq_cases.l7_engine: domains svc-00N.example.com, resources
# /api/v1/r/000NN, services svc-00N)
ENGINE_SQL = [
    "SELECT request_domain, Count(*) AS c FROM l7_flow_log "
    "WHERE request_resource LIKE '%/r/0000_' GROUP BY request_domain",
    "SELECT request_resource, Count(*) AS c, Avg(response_duration) AS a "
    "FROM l7_flow_log WHERE request_resource NOT LIKE '*1' "
    "GROUP BY request_resource",
    "SELECT Count(*) AS c, Uniq(ip4_0) AS u FROM l7_flow_log "
    "WHERE request_domain REGEXP '^svc-00[12]'",
    "SELECT l7_protocol, Uniq(request_resource) AS u FROM l7_flow_log "
    "WHERE request_domain NOT REGEXP '[34]\\.example' GROUP BY l7_protocol",
    "SELECT service_name, Percentile(response_duration, 50) AS p "
    "FROM l7_flow_log WHERE request_resource LIKE '%1' "
    "GROUP BY service_name",
    "SELECT Count(*) AS c FROM l7_flow_log WHERE (request_resource LIKE "
    "'%3' OR app_service LIKE 'svc-__4') AND response_status != 4",
    "SELECT request_domain, request_resource, response_code FROM "
    "l7_flow_log WHERE request_resource REGEXP 'r/0+[2-5]$' AND "
    "request_domain LIKE 'svc-00_.example.com' LIMIT 100000",
    "SELECT pod_name_0, Count(*) AS c FROM l7_flow_log "
    "WHERE pod_name_0 LIKE 'pod-1%' GROUP BY pod_name_0",
    "SELECT Count(*) AS c FROM l7_flow_log WHERE pod_name_0 NOT LIKE 'pod-%'",
    "SELECT Count(*) AS c FROM l7_flow_log WHERE request_resource LIKE '%'",
    "SELECT Count(*) AS c FROM l7_flow_log "
    "WHERE request_resource NOT LIKE '%nothing%'",
    "WITH t AS (SELECT request_domain, Count(*) AS c FROM l7_flow_log "
    "GROUP BY request_domain) SELECT request_domain, c FROM t "
    "WHERE request_domain LIKE 'svc-00_.%' AND request_domain NOT REGEXP "
    "'svc-00[03]'",
]


def pod_names(eng) -> Dict[int, str]:
    """A name map for the pod ids in the engine's KnowledgeGraph, except
    every fifth: those have no name and must behave as ''."""
    ids = {info.pod_id for info in eng.pipe.kg.host.values()}
    return {int(i): "pod-%d" % i for i in ids if i % 5}


def sorted_result(res) -> tuple:
    return (res["columns"],
            sorted(res["values"], key=lambda r: [str(x) for x in r]))
