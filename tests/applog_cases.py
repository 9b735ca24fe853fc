"""Shared inputs for the application-log tests (K11): the same calls are
fed to the host AppLogPipeline (the oracle) and to the GPU store."""
import copy

from deepflow_amd.ingest.applog_pipeline import AppLogPipeline

NOW = 1_700_000_500          # the `now` of every ingest_lines call
T0 = 1_700_000_000


def feed(pipe, calls):
    """calls: ("lines", payload, agent_id, log_type) | ("rows", [dict])."""
    counts = []
    for call in calls:
        if call[0] == "lines":
            counts.append(pipe.ingest_lines(call[1], agent_id=call[2],
                                            log_type=call[3], now=NOW))
        else:
            counts.append(pipe.ingest_rows(copy.deepcopy(call[1])))
    return counts


def host_of(calls):
    pipe = AppLogPipeline()
    feed(pipe, calls)
    return pipe


# ------------------------------------------------------------------ parse
SEVERITY_WORDS = ["DeBuG", "INFO", "Warn", "WARNING", "eRRoR", "Fatal",
                  "CRITICAL", "notice"]

PARSE_LINES = [
    b"1700000100 ERROR checkout failed to connect to db",     # full line
    b"free form line",
    b"only two spaces",                                       # free-form
    b"1700000200  warn app double space",                     # empty token
    b"1700000201 info  body after an empty app",
    b"123456789012345678 info app eighteen digits",
    b"1234567890123456789 info app nineteen digits",          # free-form
    b"12a info app token zero is not a number",
    b"  \t 1700000202 info padded stripped line \x1c\x1f ",
    # stripping removes the trailing space: two spaces left, free-form
    b"1700000203 info app ",
    b"1700000204 info app \xff\xfe invalid utf-8 \xc3",
] + [b"%d %s sev-app word %d" % (T0 + 300 + i, w.encode(), i)
     for i, w in enumerate(SEVERITY_WORDS)]

OTLP_ROWS = [
    {"time": T0 + 400, "agent_id": 9, "log_type": "otlp", "severity": 3,
     "severity_text": "ERROR", "app_service": "otel-svc",
     "trace_id": "ab" * 16, "span_id": "cd" * 8,
     "body": "otlp body one", "attr.k": "v"},
    # empty body right after an app: body_off ties with the next row
    {"time": T0 + 401, "agent_id": 9, "log_type": "otlp", "severity": 6,
     "severity_text": "", "app_service": "otel-svc", "trace_id": "",
     "span_id": "", "body": ""},
    {"time": T0 + 402, "agent_id": 9, "log_type": "otlp", "severity": 7,
     "severity_text": "DEBUG", "app_service": "", "trace_id": "",
     "span_id": "", "body": "no app, otlp body two"},
    {"time": T0 + 403, "agent_id": 4, "log_type": "otlp", "severity": 2,
     "severity_text": "FATAL", "app_service": "checkout", "trace_id": "",
     "span_id": "", "body": "another agent", "attr.n": 5},
]

NINETEEN = "1234567890123456789 info app nineteen digits"


def as_gpu(rows):
    """Host rows -> what the GPU store holds: its one documented parse
    divergence in these cases is the 19-digit timestamp, which the kernel
    treats as a free-form line (app "" already has its id by then)."""
    empty_id = next(r["app_id"] for r in rows if r["app_service"] == "")
    return [dict(r, time=NOW, severity=6, app_service="", app_id=empty_id,
                 body=NINETEEN)
            if r["body"] == "nineteen digits" else r for r in rows]


# three batches; the OTLP batch sits between two line batches
PARSE_CALLS = [
    ("lines", b"\r\n".join(PARSE_LINES[:6]) + b"\r\n", 6, "system"),
    ("rows", OTLP_ROWS),
    ("lines", b"\n\n".join(PARSE_LINES[6:]), 7, "syslog"),
]

# ------------------------------------------------------------------- scan
N128 = ("abcdefghij" * 13)[:128]
AND8 = ["k%dk" % i for i in range(8)]

SCAN_LINES = [
    "%d info alpha needle-start then text" % (T0 + 0),
    "%d error beta text then needle-end" % (T0 + 1),
    "%d warn gamma xaaaby" % (T0 + 2),
    "%d info zeta-only hello" % (T0 + 3),
    "%d debug alpha ends with tail" % (T0 + 4),
    "%d info beta y marks the spot" % (T0 + 5),
    "%d fatal alpha pre %s post" % (T0 + 6, N128),
    "%d info alpha pre %s# post" % (T0 + 7, N128[:-1]),
    "%d error beta all eight %s" % (T0 + 7, " ".join(AND8)),
    "%d error beta one short %s" % (T0 + 7, " ".join(AND8[:3] + AND8[4:])),
    "%d warn gamma MiXeDÉCase body" % (T0 + 3),
    "%d warn gamma lower mixedécase body" % (T0 + 3),
    "free form text with Needle-Start inside",
    "%d info alpha the very last bytes are pool-end" % (T0 + 2),
]

# two batches, no trailing newline: "pool-end" ends the pool
SCAN_CALLS = [
    ("lines", "\n".join(SCAN_LINES[:7]).encode() + b"\n", 1, "system"),
    ("lines", "\n".join(SCAN_LINES[7:]).encode(), 2, "syslog"),
]

# (substr, case_insensitive); the comment says what the case is for
SCAN_QUERIES = [
    ("needle-start", False),            # body start
    ("needle-end", False),              # body end
    ("pool-end", False),                # last bytes of the pool
    ("y", False),                       # length 1
    (N128, False),                      # length 128; one near miss
    ("zeta-only", False),               # an app name: prefixes only
    ("info", False),                    # a severity word: prefixes only
    ("tail\n%d" % (T0 + 5), False),     # spans two lines
    ("aab", False),                     # restart after a partial match
    (AND8, False),                      # one row lacks exactly one needle
    (AND8[:3] + AND8[4:], False),
    ("NEEDLE-start", True),
    ("mIxEdÉcAsE", True),          # ASCII folds, the E-acute does not
    ("mixedécase", True),
    (["mixed", "BODY"], True),
    ("", False),                        # empty needle: every row
    (["", "hello"], False),
    ("no such text anywhere", False),
]


# ------------------------------------------------------------------- tile
EDGE_NEEDLE = "EDGE-STRADDLE-NEEDLE"        # 20 bytes
ON_EDGE_NEEDLE = "ON-EDGE"


def tile_payload(tile):
    """About three tiles of lines for an empty store (pool offset ==
    payload offset). One EDGE_NEEDLE starts len-1 bytes before the first
    tile edge and ends after it; one ON_EDGE_NEEDLE starts exactly on the
    second edge. -> (payload, [start of each planted needle])."""
    out = bytearray()
    n = 0

    def prefix():
        nonlocal n
        n += 1
        return b"%d info tile%d " % (T0 + n % 8, n % 3)

    def plant(needle, at):
        while True:
            pre = prefix()
            k = at - len(out) - len(pre)
            if 1 <= k < 200:
                out.extend(pre + b"." * k + needle.encode() + b" ok\n")
                return
            assert k > 0
            out.extend(pre + b"." * 90 + b"\n")

    a = tile - (len(EDGE_NEEDLE) - 1)
    plant(EDGE_NEEDLE, a)
    plant(ON_EDGE_NEEDLE, 2 * tile)
    while len(out) < 3 * tile - 150:
        out.extend(prefix() + b"." * 90 + b"\n")
    payload = bytes(out)
    assert payload[a:a + len(EDGE_NEEDLE)] == EDGE_NEEDLE.encode()
    assert payload[2 * tile:2 * tile + 7] == ON_EDGE_NEEDLE.encode()
    return payload, [a, 2 * tile]


# ----------------------------------------------------------------- select
# filters over SCAN_CALLS' rows; times T0..T0+7 plus NOW for the free-form
SELECT_FILTERS = [
    {"severity_max": 3},
    {"time_start": T0 + 2},
    {"time_end": T0 + 3},
    {"time_start": T0 + 3, "time_end": T0 + 7},     # rows on both ends
    {"app_service": "beta"},
    {"app_service": ""},                            # the free-form row
    {"app_service": "never-ingested"},
    {"substr": "e", "severity_max": 4, "time_start": T0 + 1,
     "time_end": T0 + 7, "app_service": "beta", "case_insensitive": True},
    {"severity_max": -1},
]
