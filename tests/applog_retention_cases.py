"""Shared inputs for the log-retention tests: the same calls, evictions
included, are fed to the host AppLogPipeline (the oracle) and to the GPU
store. Imports applog_cases read-only."""
import applog_cases as C

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline

T0, NOW = C.T0, C.NOW


def host_of(calls, **kw):
    pipe = AppLogPipeline(**kw)
    C.feed(pipe, calls)
    return pipe


# ------------------------------------------------------------ PARSE_CALLS
N_PARSE = 6 + len(C.OTLP_ROWS) + len(C.PARSE_LINES) - 6      # 23 rows
# rows 6..9 are the OTLP run, row 7 is the empty body that ties on body_off:
# cuts just before (6), inside (7, 8) and just after (10) the run
PARSE_FIRSTS = [1, 6, 7, 8, 10, N_PARSE - 1, N_PARSE]
# app "" is first seen on row 1 ("free form line"), after "checkout"
EMPTY_APP_ID = 1


def as_gpu(rows):
    """applog_cases.as_gpu for any subset of PARSE_CALLS' rows (the id of
    app "" is a constant here, its first row may be gone)."""
    return [dict(r, time=NOW, severity=6, app_service="",
                 app_id=EMPTY_APP_ID, body=C.NINETEEN)
            if r["body"] == "nineteen digits" else r for r in rows]


# search() keywords; none tells the 19-digit row's two readings apart
PARSE_QUERIES = [
    {},
    {"substr": "otlp body"},                            # substring
    {"substr": "WORD", "case_insensitive": True},       # case-insensitive
    {"app_service": "otel-svc"},
    {"app_service": "sev-app", "severity_max": 4},
    {"regex": r"bod[yi] (one|two)"},                    # unanchored
    {"regex": r"^word \d$"},                            # anchored
    {"regex": r"^$"},                                   # the empty body
]
# the window leaves out NOW, where the GPU store puts the 19-digit row
PARSE_HIST = (100, T0, T0 + 499)


def check_parse_pair(host, gpu):
    """Everything the GPU store answers equals the host's (PARSE_CALLS
    corpus, any eviction state). -> number of comparisons made."""
    assert gpu.n_rows == host.n_rows
    assert gpu.evicted_rows == host.evicted_rows
    assert gpu.rows == as_gpu(host.rows)
    for kw in PARSE_QUERIES:
        assert gpu.search(limit=1000, **kw) == \
            as_gpu(host.search(limit=1000, **kw)), kw
    assert gpu.search(limit=3) == as_gpu(host.search(limit=3))
    assert gpu.histogram(*PARSE_HIST) == host.histogram(*PARSE_HIST)
    assert gpu.histogram(*PARSE_HIST, regex=r"o") == \
        host.histogram(*PARSE_HIST, regex=r"o")
    return len(PARSE_QUERIES) + 4


# ----------------------------------------------------------- evict_before
# times are not monotone in row index
BEFORE_TIMES = [10, 12, 11, 30, 5, 31, 7]
BEFORE_CALLS = [("lines", b"\n".join(
    b"%d info app%d body %d" % (t, i % 3, i)
    for i, t in enumerate(BEFORE_TIMES)), 1, "system")]
# (t, rows evicted): the prefix stops at the first row with time >= t
BEFORE_CASES = [
    (5, 0), (10, 0),            # below or equal to row 0's time: nothing
    (11, 1),                    # row 1 (12) stops it; row 2 (11) is not older
    (13, 3),                    # rows 4 (5) and 6 (7) are older and stay
    (31, 5), (32, 7), (1 << 70, 7), (-(1 << 70), 0),
]

# --------------------------------------------------------------- row rule
MAX_ROWS, KEEP = 8, 0.5         # keeps floor(8 * 0.5) = 4 rows


def _batch(k, n, agent):
    return ("lines", b"\n".join(
        b"%d warn app%d batch %d line %d" % (T0 + k, (k + i) % 5, k, i)
        for i in range(n)), agent, "system")


# sizes: up to the limit exactly (8, no eviction), past it, one batch
# larger than max_rows on its own, an OTLP batch, single rows
ROW_RULE_CALLS = [_batch(0, 3, 1), _batch(1, 5, 1), _batch(2, 1, 2),
                  _batch(3, 12, 2), ("rows", C.OTLP_ROWS), _batch(4, 1, 3),
                  _batch(5, 4, 3), _batch(6, 2, 3)]


def row_rule_model(sizes, max_rows=MAX_ROWS, keep=KEEP):
    """(n_rows, evicted_rows) after every batch, from the rule's wording."""
    n = gone = 0
    out = []
    for s in sizes:
        n += s
        if n > max_rows:
            left = max(1, int(max_rows * keep))
            gone += n - left
            n = left
        out.append((n, gone))
    return out


# -------------------------------------------------------- name relocation
def relocation_calls(solo, other):
    """Row 0 alone claims app `solo` (its own batch, so the claim comes
    first); `other` arrives later. One body really contains the name."""
    s, o = solo.encode(), other.encode()
    return [
        ("lines", b"1 info %s the first line" % s, 1, "system"),
        ("lines", b"\n".join([
            b"2 info %s second" % o,
            b"3 warn third-app third",
            b"4 info %s fourth" % o,
            b"5 info %s a body that says %s itself" % (o, s),
            b"6 error %s the last line" % s]), 1, "system"),
    ]


FULL_TABLE_CALLS = [
    ("lines", b"1 info a1 one\n2 info a2 two\n3 info a1 three", 0, "s"),
    ("lines", b"4 info a3 four\n5 info a2 five\n6 info a4 six\n"
              b"7 info a5 seven", 0, "s"),
]

# ----------------------------------------------------------- cut boundary
# one payload into an empty store: pool offset == payload offset
CUT_LINES = [
    b"1700000001 info appa first body TAILEND",
    b"1700000002 info appb HEADSTART of the second body",
    b"1700000003 warn appa third body",
    b"1700000004 info appc fourth body TAILEND",
]
CUT_PAYLOAD = b"\n".join(CUT_LINES)
CUT_END0 = len(CUT_LINES[0])            # end of the first body
# the cut is rounded down: the last bytes of the evicted body stay in the
# pool, below the first kept body
assert CUT_END0 % 16 >= 3
CUT_CALLS = [("lines", CUT_PAYLOAD, 1, "system")]
# end of the evicted body + the next line's header (+ the kept body's head)
CUT_SPANNING = ["END\n1700000002 info", "END\n1700000002 info appb HEAD",
                "appb HEADSTART"]
CUT_HEAD = "HEADSTART"


# ------------------------------------------------------------------- tile
ARENA = 16                      # "tile0" "tile1" "tile2", padded
START, END = "WALK-START", "WALK-END"


def retention_tile_payload(tile, overhang):
    """About three tiles of lines for an empty store and two evictions of
    it, planned so that after each one a line START =...= END, longer than
    the regex kernel's staged overhang, starts just below a tile edge *of
    the new pool* and ends past that tile's overhang:
      eviction 1 drops `first1` rows; the first kept body started mid-tile;
      eviction 2 drops `first2` more; the first kept body (long line A)
        started within 128 bytes of the edge A straddled.
    New offsets follow from new = old - cut + ARENA, cut = the end of the
    last evicted line rounded down to 16.
    -> (payload, plan dict)."""
    out = bytearray()
    ends = []                   # end offset of every line's body
    n = 0

    def prefix():
        nonlocal n
        n += 1
        return b"%d info tile%d " % (T0 + n % 8, n % 3)

    def line(text):
        out.extend(text)
        ends.append(len(out))
        out.extend(b"\n")

    def filler():
        line(prefix() + b"." * 90)

    def plant(text, pos):
        """text at offset pos, five dots into its body."""
        while pos - len(out) > 400:
            filler()
        adj, pre = prefix(), prefix()
        d = pos - len(out) - len(adj) - 1 - len(pre) - 5
        assert d >= 1, d
        line(adj + b"." * d)
        at = len(ends)          # row index of the planted line
        line(pre + b"....." + text)
        assert bytes(out[pos:pos + len(text)]) == text
        return at

    long = START.encode() + b"=" * (overhang + 200) + END.encode()
    while len(out) < tile // 2:
        filler()
    first1 = len(ends)
    cut1 = ends[-1] & ~15
    # pool 1 offset = old - shift1
    shift1 = cut1 - ARENA
    row_a = plant(long, tile - 90 + shift1)
    first2 = row_a - first1
    cut2 = (ends[row_a - 1] - shift1) & ~15
    shift2 = cut2 - ARENA       # pool 2 offset = pool 1 offset - shift2
    row_b = plant(long, tile - 90 + shift2 + shift1)
    while len(out) < 3 * tile - 150:
        filler()
    payload = bytes(out[:-1])
    plan = {"first1": first1, "first2": first2, "row_a": row_a,
            "row_b": row_b, "rows": len(ends),
            # old offset of the first kept body of eviction 1
            "kept1_body": ends[first1 - 1] + 1 + 22}
    assert tile // 4 < plan["kept1_body"] % tile < 3 * tile // 4
    assert first1 >= 3 and 2 * tile < len(payload) < 3 * tile
    return payload, plan


# -------------------------------------------------------------- byte rule
BYTE_BUDGET = 4100              # not a multiple of 16


def byte_rule_payloads():
    """24 payloads of 8..18 lines, 45-70 bytes a line: the largest is under
    half the budget, the sum several times the budget."""
    out = []
    row = 0
    for k in range(24):
        lines = []
        for i in range(8 + (k * 5) % 15):
            lines.append(b"%d info svc-%d payload %d row %d %s"
                         % (T0 + row % 50, (k + i) % 6, k, row,
                            b"x" * (row % 23)))
            row += 1
        out.append(b"\n".join(lines) + b"\n")
    assert max(len(p) for p in out) < BYTE_BUDGET // 2
    assert sum(len(p) for p in out) > 3 * BYTE_BUDGET
    return out
