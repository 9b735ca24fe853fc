"""Hand-built span set shared by test_flowgroup_cpu.py and
test_flowgroup_gpu.py: every case the flow-group join can get wrong, mixed
into one payload whose rows interleave the groups (so groups cross segment
boundaries at segment_rows = 256).

Every span carries a unique `tag` in its span_id, so a test finds a span's
global row (= payload index) by name. Key values are kept apart between
the cases; the ranges are noted next to each.
"""
import random

from deepflow_amd.wire import pb, flow_log, framing

T0 = 1_700_000_000_000_000_000
MS = 1_000_000
SERVICES = ["front", "cart", "pay", "stock", "mail", "auth", "db", ""]


def hx(n: int, width: int = 16) -> str:
    return f"{n:0{width}x}"


def span(tag, trace="", svc="front", t0=T0, dur=5 * MS, sreq=0, sresp=0,
         tcp=0, rtcp=0, x0="", x1="", status=0, tap=0):
    return {
        "base": {
            "start_time": t0, "end_time": t0 + dur, "flow_id": 7,
            "vtap_id": 1, "tap_side": tap,
            "head": {"proto": 20, "msg_type": 2, "rrt": dur // 1000},
            "ip_src": 0x0A000001, "ip_dst": 0x0A000002,
            "l3_epc_id_src": 1, "l3_epc_id_dst": 1,
            "port_src": 40000, "port_dst": 8080, "protocol": 6,
            "req_tcp_seq": tcp, "resp_tcp_seq": rtcp,
            "syscall_trace_id_request": sreq,
            "syscall_trace_id_response": sresp,
        },
        "req": {"req_type": "GET", "domain": "svc", "resource": "/r",
                "endpoint": "/r"},
        "resp": {"status": status, "code": 200},
        "trace_info": {"trace_id": trace, "span_id": tag},
        "ext_info": {"service_name": svc, "x_request_id_0": x0,
                     "x_request_id_1": x1},
    }


# trace ids used by name in the tests
T_BRIDGE_A = hx(0xB41D6EA, 32)
T_BRIDGE_B = "bridge-b-not-hex"                # pooled trace id
T_PLAIN = hx(0x91A1, 32)
T_WINDOW = hx(0x3141, 32)
X_HOP = "req-7f3a-hop"
X_SAME = "req-same-text"
CHAIN_LEN = 230
STAR_LEN = 320
SINGLE_START = T0 + 33 * MS + 1                # no other span starts here
WINDOW_LO = T0                                 # `win-out` starts before


def build_spans():
    """-> list of span dicts in payload (= global row) order."""
    groups = []

    # pure syscall chain, no trace ids (ids 100-199): request = request,
    # then request = response
    groups.append([
        span("sys-a", sreq=101, t0=T0 + 1 * MS, svc="front"),
        span("sys-b", sreq=101, sresp=102, t0=T0 + 2 * MS, svc="cart"),
        span("sys-c", sreq=102, t0=T0 + 3 * MS, svc="db", status=3),
        span("sys-d", sresp=101, t0=T0 + 4 * MS, svc="mail"),
    ])

    # two trace ids bridged by one eBPF span through syscall ids (200-299)
    groups.append([
        span("br-a1", T_BRIDGE_A, t0=T0 + 5 * MS, svc="front"),
        span("br-a2", T_BRIDGE_A, sresp=201, t0=T0 + 6 * MS, svc="cart"),
        span("br-ebpf", sreq=201, sresp=202, t0=T0 + 7 * MS, svc="",
             status=4),
        span("br-b1", T_BRIDGE_B, sreq=202, t0=T0 + 8 * MS, svc="pay"),
        span("br-b2", T_BRIDGE_B, t0=T0 + 9 * MS, svc="db"),
    ])

    # a trace on its own: the K10 relation alone
    groups.append([span(f"plain-{i}", T_PLAIN, t0=T0 + (10 + i) * MS,
                        svc=SERVICES[i % 5]) for i in range(4)])

    # x-request-id: a gateway's outgoing id is the next hop's incoming id
    groups.append([
        span("xhop-gw", x1=X_HOP, t0=T0 + 14 * MS, svc="front"),
        span("xhop-next", x0=X_HOP, t0=T0 + 15 * MS, svc="cart"),
    ])
    # the same text in x_request_id_0 of two rows
    groups.append([
        span("xsame-1", x0=X_SAME, t0=T0 + 16 * MS, svc="pay"),
        span("xsame-2", x0=X_SAME, t0=T0 + 17 * MS, svc="stock"),
    ])

    # tcp pair (sequence numbers 7000-7999): two taps on one session join;
    # the same request sequence with another response sequence does not;
    # req_tcp_seq == 0 emits nothing, whatever resp_tcp_seq holds
    groups.append([
        span("tcp-tap1", tcp=7001, rtcp=7101, tap=1, t0=T0 + 18 * MS),
        span("tcp-tap2", tcp=7001, rtcp=7101, tap=0, t0=T0 + 19 * MS),
        span("tcp-other-resp", tcp=7001, rtcp=7999, t0=T0 + 20 * MS),
        span("tcp-zero-req-1", tcp=0, rtcp=7101, t0=T0 + 21 * MS),
        span("tcp-zero-req-2", tcp=0, rtcp=7101, t0=T0 + 22 * MS),
    ])

    # one value in two key spaces: syscall id 5000, tcp pair value 5000
    # (resp_tcp_seq 0 makes the pair equal the request sequence)
    groups.append([
        span("cross-sys", sreq=5000, t0=T0 + 23 * MS),
        span("cross-tcp", tcp=5000, rtcp=0, t0=T0 + 24 * MS),
    ])

    # a chain: row i shares a key only with row i + 1 (ids 10000-10999)
    groups.append([span(f"chain-{i}", sreq=10000 + i if i else 0,
                        sresp=10001 + i if i < CHAIN_LEN - 1 else 0,
                        t0=T0 + 25 * MS + i, svc=SERVICES[i % 7],
                        status=3 if i % 50 == 0 else 0)
                   for i in range(CHAIN_LEN)])

    # a star: every row on one key
    groups.append([span(f"star-{i}", x0="star-request-id",
                        t0=T0 + 26 * MS + i, svc=SERVICES[i % 6])
                   for i in range(STAR_LEN)])

    # singletons: no key at all; keys nobody shares; one at its own instant
    groups.append([
        span("single-bare", t0=T0 + 27 * MS),
        span("single-keys", hx(0x51261E, 32), sreq=301, sresp=302, tcp=7300,
             rtcp=7301, x0="only-me", x1="only-me-out", t0=T0 + 28 * MS),
        span("single-instant", sreq=303, t0=SINGLE_START),
    ])

    # window case: `win-out` starts before WINDOW_LO and is the only link
    # between `win-in-1` and `win-in-2` (ids 400-499); `win-lone`'s only
    # partner lies outside
    groups.append([
        span("win-out", T_WINDOW, sresp=401, x1="win-x", t0=T0 - 10_000 * MS,
             dur=20_000 * MS),
        span("win-in-1", T_WINDOW, t0=T0 + 36 * MS, svc="cart"),
        span("win-in-2", sreq=401, t0=T0 + 37 * MS, svc="db"),
        span("win-lone", x0="win-x", t0=T0 + 38 * MS, svc="mail"),
    ])

    # filler: small groups, each a mix of the four relations (syscall ids
    # from 1 << 20, tcp from 1 << 21, trace ids 0xF000000 + t)
    rng = random.Random(20261020)
    n_fill = 0
    t = 0
    while n_fill < 900:
        size = rng.choice([1, 2, 3, 5, 9, 17])
        tid = [hx(0xF000000 + t, 32), f"filler-trace-{t}", ""][t % 3]
        g = []
        for i in range(size):
            kw = dict(svc=rng.choice(SERVICES), t0=T0 + (100 + n_fill) * MS,
                      dur=rng.randrange(1, 50) * MS,
                      status=rng.choice([0, 0, 0, 0, 3, 4]))
            how = rng.randrange(4) if i else 0
            if how == 0 and tid:
                kw["trace"] = tid
            elif i:
                j = rng.randrange(i)              # partner: an earlier span
                b, e = g[j]["base"], g[j]["ext_info"]
                if how <= 1:                      # syscall, either side
                    side = rng.choice(["syscall_trace_id_request",
                                       "syscall_trace_id_response"])
                    b[side] = b[side] or (1 << 20) + (t << 6) + j
                    kw[rng.choice(["sreq", "sresp"])] = b[side]
                elif how == 2:                    # tcp pair
                    if not b["req_tcp_seq"]:
                        b["req_tcp_seq"] = (1 << 21) + n_fill
                        b["resp_tcp_seq"] = rng.choice([0, 77 + n_fill])
                    kw["tcp"], kw["rtcp"] = b["req_tcp_seq"], \
                        b["resp_tcp_seq"]
                else:                             # x-request-id, out -> in
                    e["x_request_id_1"] = e["x_request_id_1"] or \
                        f"fill-{t}-{j}"
                    kw["x0"] = e["x_request_id_1"]
            g.append(span(f"fill-{t}-{i}", **kw))
            n_fill += 1
        groups.append(g)
        t += 1

    # interleave the groups, keeping each group's own order
    rng = random.Random(7)
    cursors = [0] * len(groups)
    weights = [len(g) for g in groups]
    out = []
    while any(w for w in weights):
        gi = rng.choices(range(len(groups)), weights=weights)[0]
        out.append(groups[gi][cursors[gi]])
        cursors[gi] += 1
        weights[gi] -= 1
    # a row count that is no multiple of the wave or the block
    while len(out) % 64 in (0, 1):
        out.append(span(f"pad-{len(out)}", t0=T0 + 2000 * MS))
    return out


def payloads_of(spans, chunk: int = 97):
    """One frame payload per `chunk` spans: a batch has to fit the tail
    segment, and 97-row batches leave every 256-row segment part-filled."""
    return [framing.pack_records(
        [pb.encode(s, flow_log.APP_PROTO_LOGS_DATA)
         for s in spans[i:i + chunk]]) for i in range(0, len(spans), chunk)]


def row_of(spans, tag: str) -> int:
    return next(g for g, s in enumerate(spans)
                if s["trace_info"]["span_id"] == tag)


def keys_of(s):
    """The (space, key) pairs a span emits, from its dict alone: what the
    brute-force search in the tests joins on."""
    b, e = s["base"], s["ext_info"]
    out = set()
    if s["trace_info"]["trace_id"]:
        out.add(("trace", s["trace_info"]["trace_id"]))
    for k in ("syscall_trace_id_request", "syscall_trace_id_response"):
        if b[k]:
            out.add(("syscall", b[k]))
    if b["req_tcp_seq"]:
        out.add(("tcp", (b["req_tcp_seq"], b["resp_tcp_seq"])))
    for k in ("x_request_id_0", "x_request_id_1"):
        if e[k]:
            out.add(("xreq", e[k]))
    return out
