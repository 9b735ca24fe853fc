"""Shared inputs for the log-pattern tests (K14) and a deliberately naive
oracle: re.split plus a dict, written from the issue's wording and without
a look at deepflow_amd/query/logpattern.py. Imports applog_cases read-only."""
import re

import applog_cases as C

T0, NOW = C.T0, C.NOW

PREFIX = 512
WILD, TRUNC = 0x100, 0x101
DELIMS = bytes(range(0x21)) + b"\"'(),;:=[]{}|"
_SPLIT = re.compile(b"([" + re.escape(DELIMS) + b"])")
_M = (1 << 64) - 1


# ----------------------------------------------------------------- oracle
def naive_symbols(body: bytes):
    out = []
    for k, piece in enumerate(_SPLIT.split(body[:PREFIX])):
        if k % 2:                               # the delimiter itself
            out.append(piece[0])
        elif any(48 <= c <= 57 for c in piece):
            out.append(WILD)
        else:
            out.extend(piece)
    if len(body) > PREFIX:
        out.append(TRUNC)
    return tuple(out)


def naive_key(body: bytes) -> int:
    h = 0xCBF29CE484222325
    for s in naive_symbols(body):
        h = ((h ^ s) * 0x100000001B3) & _M
    h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & _M
    h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & _M
    h ^= h >> 31
    return h or 1


def naive_render(body: bytes) -> str:
    out, run = "", b""
    for s in naive_symbols(body) + (None,):
        if s is not None and s < 256:
            run += bytes([s])
            continue
        out += run.decode("utf-8", "replace")
        run = b""
        if s is not None:
            out += "<*>" if s == WILD else "<...>"
    return out


def naive_patterns(host, **kw):
    """What patterns(**kw) must return on the host store, from search():
    the matching rows oldest first, grouped in a dict."""
    kw = dict(kw)
    limit = kw.pop("limit", 20)
    kw.pop("max_patterns", None)
    rows = list(reversed(host.search(kw.pop("substr", ""), limit=10 ** 9,
                                     **kw)))
    groups = {}
    for i, r in enumerate(rows):
        sym = naive_symbols(r["body"].encode("utf-8", "replace"))
        g = groups.setdefault(sym, {"count": 0, "first": i})
        g["count"] += 1
        g["sample"] = r
    order = sorted(groups.values(), key=lambda g: (-g["count"], g["first"]))
    return {"matched": len(rows), "distinct": len(groups), "dropped_rows": 0,
            "patterns": [
                {"pattern": naive_render(
                    g["sample"]["body"].encode("utf-8", "replace")),
                 "count": g["count"], "sample": g["sample"]}
                for g in order[:max(limit, 0)]]}


# ------------------------------------------------------------ edge bodies
def _long(n):
    b = (b"alpha beta=7 gamma/delta " * 100)[:n]
    return b[:-1] + b"x" if b[-1:] == b" " else b


_PAD = b"ab " * 168                             # 504 bytes, digit-free
# a token that straddles byte 512; its only digit lies after the cap
STRADDLE = _PAD + b"x" * 12 + b"9zz tail"
# a token with digits that ends exactly at byte 512, then more
ENDS_AT_CAP = _PAD + b"endtok12" + b" after 3"
# ... and a body that ends there too
ENDS_AT_CAP_EXACT = _PAD + b"endtok12"
# the last byte inside the cap and the first byte outside it are digits
DIGIT_AT_511 = _PAD + b"xxxxxxx7" + b"yy"
DIGIT_AT_512 = _PAD + b"xxxxxxxx" + b"7y"
assert len(_PAD) == 504 and len(ENDS_AT_CAP_EXACT) == 512
assert STRADDLE.index(b"9") > 512 and DIGIT_AT_511[511:513] == b"7y"
assert DIGIT_AT_512[512:513] == b"7"

# valid UTF-8, so they survive str: usable as OTLP bodies as well.
# (body, rendered template): the expectation is written by hand
EDGE_TEXT = [
    (b"", ""),
    (b" ", " "),
    (b",;:=", ",;:="),
    (b"()[]{}|\"'", "()[]{}|\"'"),
    (b"token", "token"),
    (b"5xx", "<*>"),
    (b"xx5", "<*>"),
    (b"x5x", "<*>"),
    (b"7", "<*>"),
    (b"ends with digit 7", "ends with digit <*>"),
    (b"10.0.0.1:8080", "<*>:<*>"),
    (b"k=v a=1 b=two c=3x", "k=v a=<*> b=two c=<*>"),
    (b"literal <*> here", "literal <*> here"),
    (b"literal <*> 5", "literal <*> <*>"),
    (b"a\x00b", "a\x00b"),
    (b"a\x001 \x002", "a\x00<*> \x00<*>"),
    (b"line1\nline two\n9", "<*>\nline two\n<*>"),
    ("café 日本 1é x".encode(), "café 日本 <*> x"),
    (b"\x7f! x.y-z/w_v <t>", "\x7f! x.y-z/w_v <t>"),
    (b"tab\tsep\x1fx1", "tab\tsep\x1f<*>"),
    (_long(511), None), (_long(512), None), (_long(513), None),
    (_long(2000), None),
    (STRADDLE, (_PAD + b"x" * 8).decode() + "<...>"),
    (ENDS_AT_CAP, _PAD.decode() + "<*><...>"),
    (ENDS_AT_CAP_EXACT, _PAD.decode() + "<*>"),
    (DIGIT_AT_511, _PAD.decode() + "<*><...>"),
    (DIGIT_AT_512, (_PAD + b"x" * 8).decode() + "<...>"),
]
# not valid UTF-8: bytes 0x80..0xFF are literals, never digits or delimiters
EDGE_RAW = [
    (b"\x80\xff\xfe raw 1\xff", "\ufffd\ufffd\ufffd raw <*>"),
    (bytes(range(0x80, 0x100)), None),
    (b"\xb0\xb9=\xa0", "\ufffd\ufffd=\ufffd"),      # 0x30 | 0x80 is no digit
]
EDGE_BODIES = [b for b, _ in EDGE_TEXT + EDGE_RAW]


def line_safe(body: bytes) -> bool:
    """Can the body be fed as the tail of one '<ts> <sev> <app> ' line and
    come back unchanged (no line break, nothing for strip() at its end)?"""
    ws = b"\t\n\x0b\x0c\r\x1c\x1d\x1e\x1f "
    return bool(body) and b"\n" not in body and b"\r" not in body \
        and body[-1] not in ws


LINE_BODIES = [b for b in EDGE_BODIES if line_safe(b)]
TEXT_BODIES = [b.decode() for b, _ in EDGE_TEXT]        # for ingest_rows


def lines_call(bodies, agent=3, pad_to=None):
    """One ingest_lines call with one line per body and no trailing line
    break, so the last body ends the payload. pad_to=(m, 16): dots are
    appended to the last body until len(payload) % 16 == m.
    -> (call, bodies as stored)."""
    bodies = list(bodies)

    def build():
        return b"\n".join(b"%d info app%d %s" % (T0 + i % 8, i % 3, b)
                          for i, b in enumerate(bodies))
    if pad_to is not None:
        while len(build()) % pad_to[1] != pad_to[0]:
            bodies[-1] += b"."
    return ("lines", build(), agent, "system"), bodies


def rows_call(texts):
    return ("rows", [
        {"time": T0 + 10 + i % 5, "agent_id": 9, "log_type": "otlp",
         "severity": 2 + i % 6, "severity_text": "", "trace_id": "%032x" % i,
         "span_id": "", "app_service": "otel-%d" % (i % 2), "body": t,
         "attr.i": i}
        for i, t in enumerate(texts)])


# -------------------------------------------------------- template corpus
def _template_lines():
    out = []
    for i in range(60):
        k = i % 6
        body = [
            "request id=%d served in %dms" % (i * 7919, i % 13),
            "connect to 10.0.%d.%d:5432 failed" % (i % 7, i),
            "cache miss",
            "worker spawn" if i < 30 else "worker exit",
            "user u%d logged in (session=%x)" % (i, i * 2654435761 % 2 ** 32),
            "Timeout after %d retries" % i if i % 12 == 5
            else "literal <*> after %d retries" % i,
        ][k]
        out.append("%d %s svc-%d %s" % (T0 + i // 4,
                                        ("info", "warn", "error")[i % 3],
                                        i % 4, body))
    return out


TEMPLATE_LINES = _template_lines()
# two line batches around an OTLP batch that holds every text edge body
PATTERN_CALLS = [
    ("lines", "\n".join(TEMPLATE_LINES[:35]).encode() + b"\n", 1, "system"),
    rows_call(TEXT_BODIES),
    ("lines", "\n".join(TEMPLATE_LINES[35:]).encode(), 2, "syslog"),
]

# patterns() keywords over PATTERN_CALLS
PATTERN_QUERIES = [
    {},
    {"limit": 1},
    {"limit": 3},
    {"limit": 1000},
    {"limit": 0},
    {"limit": -5},
    {"substr": "worker"},
    {"substr": "TIMEOUT", "case_insensitive": True},
    {"substr": ["after", "retries"]},
    {"regex": r"id=\d+"},
    {"regex": r"^(cache|worker) "},
    {"regex": r"LOGGED IN", "case_insensitive": True},
    {"severity_max": 3},
    {"time_start": T0 + 5, "time_end": T0 + 11},
    {"app_service": "svc-2"},
    {"app_service": "otel-1"},
    {"substr": "e", "regex": r"\d", "severity_max": 4, "time_start": T0 + 2,
     "time_end": T0 + 13, "app_service": "svc-1", "case_insensitive": True},
    {"substr": "no such text anywhere"},
    {"app_service": "never-ingested"},
    {"severity_max": -1},
    {"max_patterns": 1},            # the host store never drops
]

# every filter set the scan and regex tests use on SCAN_CALLS
def scan_queries():
    import applog_regex_cases as R
    out = [{"substr": s, "case_insensitive": ci} for s, ci in C.SCAN_QUERIES]
    out += [dict(f) for f in C.SELECT_FILTERS]
    out += [{"regex": p, "case_insensitive": ci} for p, ci, _ in R.SCAN_REGEX]
    out += [dict(kw, regex=p) for p, kw in R.SCAN_COMBINED]
    return out


# (keywords, what the message names); ValueError on either store, full or
# empty
BAD_ARGS = [
    ({"max_patterns": 0}, "max_patterns"),
    ({"max_patterns": 3}, "max_patterns"),
    ({"max_patterns": -4}, "max_patterns"),
    ({"max_patterns": 1.5}, "max_patterns"),
    ({"regex": "("}, "invalid"),
    ({"regex": r"(a)\1"}, "backreference"),
    ({"substr": ["a"] * 9}, "needles"),
]


# ------------------------------------------------------------ skew, spill
def skew_calls(n_hot=5000):
    """n_hot rows of one template, a few others strewn among them."""
    lines = []
    for i in range(n_hot):
        lines.append(b"%d info hot request %d took %dms" % (T0 + i % 50, i,
                                                            i % 97))
        if i % 701 == 0:
            lines.append(b"%d warn cold cache miss" % (T0 + i % 50))
        if i % 1303 == 5:
            lines.append(b"%d error cold disk /dev/sd%d full" % (T0, i % 4))
    return [("lines", b"\n".join(lines[:3000]), 1, "system"),
            ("lines", b"\n".join(lines[3000:]), 1, "system")]


def _letters(i):
    s = ""
    for _ in range(3):
        s += "abcdefghijklmnopqrstuvwxyz"[i % 26]
        i //= 26
    return s


def spill_calls(lds_slots):
    """2 * lds_slots + 3 digit-free templates, cycled so that any 256
    consecutive rows hold 256 different ones; template t occurs 2 + (t % 3
    == 0) times. -> (calls, number of templates)."""
    d = 2 * lds_slots + 3
    assert d <= 26 ** 3
    lines = [b"%d info app tmpl-%s happened" % (T0 + i % 9,
                                                _letters(i % d).encode())
             for i in range(2 * d)]
    lines += [b"%d info app tmpl-%s happened" % (T0, _letters(t).encode())
              for t in range(0, d, 3)]
    return [("lines", b"\n".join(lines), 1, "system")], d


OVERFLOW_LINES = [
    b"1 info a alpha %d" % 1, b"2 info a beta", b"3 info a alpha 22",
    b"4 info a gamma x=1", b"5 info a delta", b"6 info a alpha 333",
    b"7 info a epsilon", b"8 info a beta", b"9 info a gamma x=77",
]
OVERFLOW_CALLS = [("lines", b"\n".join(OVERFLOW_LINES), 1, "system")]

# ------------------------------------------------------- after retention
# one app only: with app_capacity=1 the app table is full and every row
# still reads back as on the host. Row 0 claims the app and is evicted.
RETENTION_CALLS = [
    ("lines", b"1 info solo the first line 1", 1, "system"),
    ("lines", b"\n".join(
        [b"%d info solo job %d finished in %ds" % (2 + i, i, i * 3)
         for i in range(6)]
        + [b"9 warn solo solo says hello", b"10 info solo job x finished",
           b"11 error solo the first line 2"]), 1, "system"),
]
