"""Shared patterns and corpora for the log-regex tests (K13). The oracle is
always Python's `re` on bytes, directly or through the host AppLogPipeline.
Imports applog_cases read-only."""
import itertools
import re

import applog_cases as C

# ---------------------------------------------------------------- compiler
# supported patterns; each is tried with and without IGNORECASE
PATTERNS = [
    r"a", r"ab", r"a*", r"a+b", r"a?b", r"a{2}", r"a{2,}", r"a{1,3}b",
    r"a{0}b", r"a+?b", r"a*?b", r"a??b", r"a{1,2}?1",      # every quantifier
    r"(a|b)+1", r"((a|b)a)*b", r"(?:ab|ba)+", r"(a*)*b",    # nested groups
    r"(?P<x>a)b", r"(a|ab)(1|b1)?A", r"x(a|aa)+by", r"ab|ba|1",
    r"[^a]", r"[^a\n]b", r"[A-Z]", r"[a-b]1", r"[^A-B]a",   # classes
    r"\d", r"\D", r"\w+", r"\W", r"\s", r"\S\s", r"[\d\s]a", r"[^\w]",
    r".", r"a.b", r".*", r"a.*b", r"\n.", r"\.",            # . against \n
    r"^a", r"^", r"\Aab", r"a$", r"a\Z", r"$", r"\Z", r"\n$", r"\n\Z",
    r"[^\n]$", r"^$", r"^\Z", r"^a*$", r"^a*\Z", r"^(a|b)*$", r"^a.*1$",
    r"\xc3", r"é", r"\x41",
    # splits all 256 bytes into classes: four quarters, then \d \w \s and .
    r"[\x00-\x3f]a|[\x40-\x7f]b|[\x80-\xbf]1|[\xc0-\xff]\d|\w\s.",
]


def _words(alphabet, max_len):
    return [b"".join(t) for n in range(max_len + 1)
            for t in itertools.product(alphabet, repeat=n)]


# every byte string of length 0..4 over {a, b, A, 1, \n, 0xC3} and every
# string of length 0..6 over {a, b}
BODIES = _words([b"a", b"b", b"A", b"1", b"\n", b"\xc3"], 4) \
    + _words([b"a", b"b"], 6)

# (pattern, what the message must name); all raise ValueError
REFUSED = [
    (r"(a)\1", "backreference"),
    (r"(?P<x>a)(?P=x)", "backreference"),
    (r"a(?=b)", "look-around"),
    (r"a(?!b)", "look-around"),
    (r"(?<=a)b", "look-around"),
    (r"\bfoo", r"\b"),
    (r"foo\B", r"\B"),
    (r"^a|b", "anchor"),
    (r"a$b", "anchor"),
    (r"(^a)", "anchor"),
    (r"a(b$)", "anchor"),
    (r"(?i)a", "inline flags"),
    (r"(?i:a)b", "inline flags"),
    (r"(a)(?(1)b|c)", "conditional"),
    (r"(a", "invalid"),
    (r"a)", "invalid"),
    (r"[a", "invalid"),
    (r"*a", "invalid"),
    ("\\u00e9", "invalid"),                # no \\u escape in a bytes pattern
    ("\ud800", "not valid as bytes"),       # a lone surrogate
    (r"(a|b)*a(a|b){30}", "too complex"),   # 2^30 DFA states
    (r"((a{99}){99}){99}", "too complex"),  # NFA blow-up before any DFA
    ("a" * 257, "too complex"),             # over the pattern length
    # U+0080..U+00BF are C2 80..C2 BF in UTF-8: 65 distinct literal bytes
    ("".join(chr(c) for c in range(0x80, 0xc0)), "too complex"),
]


def host_flags(ci):
    return re.IGNORECASE if ci else 0


def re_rows(rows, pattern, ci=False):
    """The oracle spelled out: rows (oldest first) whose body matches,
    newest first, as search() returns them."""
    rx = re.compile(pattern.encode("utf-8"), host_flags(ci))
    return [r for r in reversed(rows)
            if rx.search(r["body"].encode("utf-8", "replace"))]


# --------------------------------------------------- SCAN_CALLS corpus
# (regex, case_insensitive, hits the oracle must report)
SCAN_REGEX = [
    (r"needle-sta[r-t]+", False, 1),            # at a body's start
    (r"needle-e.d$", False, 1),                 # at a body's end
    (r"pool-e\w+", False, 1),                   # the last bytes of the pool
    (r"pool-end$", False, 1),
    (r"pool-end.", False, 0),                   # nothing after the pool
    (r"tail\s+\d+", False, 0),                  # would span two lines
    (r"tail$", False, 1),
    (r"^info", False, 0),                       # header tokens are no body
    (r"^alpha", False, 0),
    (r"alpha", False, 0),
    (r"x(a|aa)+by", False, 1),
    (r"^x(a|aa)+by$", False, 1),
    (r"xa{4}by", False, 0),
    (r"^pre [a-j]{128} post$", False, 1),
    (r"^pre [a-j]+# post", False, 1),
    (r"NEEDLE-start", False, 0),
    (r"NEEDLE-start", True, 2),
    (r"mixed.+case", True, 2),
    (r"mIxEdÉcAsE", True, 1),                   # the É row: A-Z folds only
    (r"mixedécase", True, 1),
    (r"[A-Z]{2}", False, 0),                    # "MiXeDÉCase": "ÉC" is not
    (r"^[a-z -]+$", False, 8),
    (r"k\dk k\dk k\dk k[^3]k", False, 2),
    (r"y", False, 5),
    (r"^y", False, 1),
    (r"(text|form) .*(end|inside)$", False, 2),
    (r"no such (text|pattern) anywhere", False, 0),
]

# (regex, search() keywords): the regex ANDed with everything else
SCAN_COMBINED = [
    (r"k\dk", {"substr": C.AND8}),              # all 8 needles and the regex
    (r"k\dk$", {"substr": C.AND8[:3] + C.AND8[4:]}),
    (r"k7k$", {"substr": C.AND8}),
    (r"^all", {"substr": C.AND8, "case_insensitive": True}),
    (r"e", {"severity_max": 3}),
    (r"e", {"time_start": C.T0 + 2}),
    (r"e", {"time_end": C.T0 + 3}),
    (r"e", {"time_start": C.T0 + 3, "time_end": C.T0 + 7}),
    (r"t[eh]", {"app_service": "beta"}),
    (r"\w", {"app_service": ""}),
    (r"e", {"app_service": "never-ingested"}),
    (r"E.*T", {"substr": "e", "severity_max": 4, "time_start": C.T0 + 1,
               "time_end": C.T0 + 7, "app_service": "beta",
               "case_insensitive": True}),
    (r"e", {"severity_max": -1}),
    (r"e", {"limit": 2}),
    (r"e", {"limit": 0}),
    (r".*", {"substr": "hello"}),               # matches every body
    (r"", {"substr": "hello"}),
]

# --------------------------------------------------- PARSE_CALLS corpus
# (regex, case_insensitive); the empty-body OTLP row ties on body_off with
# the row after it ("no app, otlp body two")
PARSE_REGEX = [
    (r"^$", False), (r"^\Z", False), (r"^a*$", False), (r".*", False),
    (r"a*", False), (r"^", False), (r"$", False), (r"x?$", False),
    (r"^no app", False), (r"^no app, otlp body two$", False),
    (r"otlp body (one|two)$", False), (r"^otlp", False), (r"two", False),
    (r"^.$", False), (r"^[^o]", False), (r"\d{18}", False),
    (r"^OTLP BODY", True), (r"digits$", False), (r"^another agent$", False),
]


# ------------------------------------------------------------------- tile
START, END = "WALK-START", "WALK-END"


def regex_tile_payload(tile, overhang):
    """A bit over four tiles of lines for an empty store (pool offset ==
    payload offset), built like applog_cases.tile_payload. Planted:
      EDGE1 starts 1 byte before the first tile edge;
      ONEDGE starts exactly on the second edge;
      START, more than `overhang` filler bytes, END: starts 100 bytes
        before the third edge and ends beyond that tile's overhang;
      the last line holds START 100 bytes before the fourth edge and a
        filler as long, but no END, and ends the pool.
    -> (payload, {name: offset})."""
    out = bytearray()
    n = 0
    at = {}

    def prefix():
        nonlocal n
        n += 1
        return b"%d info tile%d " % (C.T0 + n % 8, n % 3)

    def filler_until(pos):
        while pos - len(out) > 260:
            out.extend(prefix() + b"." * 90 + b"\n")

    def plant(name, text, pos):
        filler_until(pos)
        pre = prefix()
        k = pos - len(out) - len(pre)
        assert k >= 1, (name, k)
        out.extend(pre + b"." * k + text + b" ok\n")
        at[name] = pos
        assert bytes(out[pos:pos + len(text)]) == text

    long = START.encode() + b"=" * (overhang + 200)
    plant("edge1", b"EDGE1-MATCH", tile - 1)
    plant("onedge", b"ONEDGE-MATCH", 2 * tile)
    plant("long", long + END.encode(), 3 * tile - 100)
    plant("last", long, 4 * tile - 100)
    payload = bytes(out[:-len(b" ok\n")])
    for name, edge in (("long", 3 * tile), ("last", 4 * tile)):
        assert at[name] < edge and at[name] + len(long) > edge + overhang
    assert payload.endswith(b"=" * 200) and len(payload) > 4 * tile
    return payload, at
