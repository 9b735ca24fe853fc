"""Hand-built span set shared by test_tracemap_cpu.py and
test_tracemap_gpu.py: every case the bulk trace join can get wrong, mixed
into one payload whose rows interleave the traces (so links cross segment
boundaries at segment_rows = 256)."""
import random

from deepflow_amd.wire import pb, flow_log, framing

T0 = 1_700_000_000_000_000_000
MS = 1_000_000
SERVICES = ["front", "cart", "pay", "stock", "mail", "auth", "db", ""]


def hx(n: int, width: int = 16) -> str:
    return f"{n:0{width}x}"


def span(trace, sid, parent="", tap=0, svc="front", t0=T0, dur=5 * MS,
         sreq=0, sresp=0, tcp=0, status=0):
    return {
        "base": {
            "start_time": t0, "end_time": t0 + dur, "flow_id": 7,
            "vtap_id": 1, "tap_side": tap,
            "head": {"proto": 20, "msg_type": 2, "rrt": dur // 1000},
            "ip_src": 0x0A000001, "ip_dst": 0x0A000002,
            "l3_epc_id_src": 1, "l3_epc_id_dst": 1,
            "port_src": 40000, "port_dst": 8080, "protocol": 6,
            "req_tcp_seq": tcp,
            "syscall_trace_id_request": sreq,
            "syscall_trace_id_response": sresp,
        },
        "req": {"req_type": "GET", "domain": "svc", "resource": "/r",
                "endpoint": "/r"},
        "resp": {"status": status, "code": 200},
        "trace_info": {"trace_id": trace, "span_id": sid,
                       "parent_span_id": parent},
        "ext_info": {"service_name": svc},
    }


# trace ids used by name in the tests
T_CHAIN = hx(0xC4A1, 32)
T_FAN = "trace-fanout"                        # non-hex: pooled trace id
T_DUP = hx(0xD0D0, 32)
T_TWIN_A = hx(0x7A, 32)
T_TWIN_B = "7b-not-hex-7b-not-hex-7b-not-hex"  # 32 chars, not hex
T_SELF = hx(0x5E1F, 32)
T_CYCLE = hx(0xC1C1E, 32)
T_ORPHAN = "trace-orphan"
T_SYS = hx(0x5115, 32)
T_TCP = hx(0x7C9, 32)
T_PRIO = hx(0x9410, 32)
T_SINGLE = hx(0x51261E, 32)
T_ZZ = hx(0x2222, 32)
T_WINDOW = hx(0x3141, 32)
T_SINGLE_START = T0 + 33 * MS + 1              # no other span starts here
WINDOW_LO = T0                                # T_WINDOW's root starts before


def build_spans():
    """-> list of span dicts in payload (= global row) order."""
    groups = []

    # a chain 48 deep, 16-hex ids (binary span ids, hex parents)
    groups.append([span(T_CHAIN, hx(0x1000 + i),
                        hx(0x1000 + i - 1) if i else "",
                        svc=SERVICES[i % 5], t0=T0 + i * MS,
                        status=3 if i % 7 == 0 else 0)
                   for i in range(48)])

    # one parent with 300 children; the parent id is non-hex (pooled span
    # id, hashed parent), the trace id is non-hex too
    fan = [span(T_FAN, "s-root", tap=1, svc="front", dur=900 * MS)]
    fan += [span(T_FAN, hx(0x2000 + i), "s-root", svc=SERVICES[i % 7],
                 t0=T0 + (i + 1) * MS, status=4 if i % 50 == 0 else 0)
            for i in range(300)]
    groups.append(fan)

    # duplicated span id inside one trace: the lowest row wins, and the
    # second copy (whose parent is that id) hangs below the first
    groups.append([
        span(T_DUP, hx(0xD1), svc="auth", t0=T0 + 1 * MS),
        span(T_DUP, hx(0xD1), hx(0xD1), svc="db", t0=T0 + 2 * MS),
        span(T_DUP, hx(0xD2), hx(0xD1), svc="pay", t0=T0 + 3 * MS),
    ])

    # the same span ids in two traces: no link may cross
    for t, svc in ((T_TWIN_A, "cart"), (T_TWIN_B, "stock")):
        groups.append([
            span(t, hx(0xAA), svc=svc, t0=T0 + 4 * MS),
            span(t, hx(0xAB), hx(0xAA), svc="db", t0=T0 + 5 * MS),
            span(t, "same-text-id", hx(0xAB), svc="mail", t0=T0 + 6 * MS),
            span(t, hx(0xAC), "same-text-id", svc="auth", t0=T0 + 7 * MS),
        ])

    # a span that is its own parent: the self candidate is rejected and the
    # syscall rule then finds a real parent; a second one has no other rule
    groups.append([
        span(T_SELF, hx(0x5E0), svc="front", sresp=4141, t0=T0 + 8 * MS),
        span(T_SELF, hx(0x5E1), hx(0x5E1), svc="pay", sreq=4141,
             t0=T0 + 9 * MS),
        span(T_SELF, hx(0x5E2), hx(0x5E2), svc="db", t0=T0 + 10 * MS),
    ])

    # a two-span cycle with a child hanging off it: nothing is rooted
    groups.append([
        span(T_CYCLE, hx(0xC1), hx(0xC2), svc="cart", t0=T0 + 11 * MS,
             dur=3 * MS),
        span(T_CYCLE, hx(0xC2), hx(0xC1), svc="pay", t0=T0 + 12 * MS),
        span(T_CYCLE, hx(0xC3), hx(0xC1), svc="db", t0=T0 + 13 * MS),
    ])

    # a parent id that matches nothing: two roots in one trace
    groups.append([
        span(T_ORPHAN, "o-root", svc="front", t0=T0 + 14 * MS),
        span(T_ORPHAN, "o-kid", "o-root", svc="cart", t0=T0 + 15 * MS),
        span(T_ORPHAN, "o-lost", "no-such-span", svc="mail",
             t0=T0 + 16 * MS),
        span(T_ORPHAN, hx(0x0F), hx(0xDEAD), svc="db", t0=T0 + 17 * MS),
    ])

    # syscall-only links (no span ids at all on the lower hops)
    groups.append([
        span(T_SYS, "", svc="front", sresp=777, t0=T0 + 18 * MS),
        span(T_SYS, "", svc="cart", sreq=777, sresp=888, t0=T0 + 19 * MS),
        span(T_SYS, "", svc="db", sreq=888, t0=T0 + 20 * MS),
        span(T_SYS, "", svc="mail", sreq=999, t0=T0 + 21 * MS),  # no match
    ])

    # tcp-seq links, the tap_side rule both ways
    groups.append([
        span(T_TCP, hx(0x7C0), tap=1, svc="front", tcp=5000,
             t0=T0 + 22 * MS),
        # server side of the same packet: links to the client-side span
        span(T_TCP, hx(0x7C1), tap=0, svc="cart", tcp=5000,
             t0=T0 + 23 * MS),
        # a second client-side span with that seq: rule 3 does not apply
        span(T_TCP, hx(0x7C2), tap=1, svc="pay", tcp=5000,
             t0=T0 + 24 * MS),
        # seq seen only on non-client spans: never indexed, no link
        span(T_TCP, hx(0x7C3), tap=0, svc="db", tcp=6000, t0=T0 + 25 * MS),
        span(T_TCP, hx(0x7C4), tap=2, svc="mail", tcp=6000,
             t0=T0 + 26 * MS),
    ])

    # all three rules have a candidate: priority decides
    groups.append([
        span(T_PRIO, hx(0x9A), svc="front", t0=T0 + 27 * MS),
        span(T_PRIO, hx(0x9B), hx(0x9A), svc="auth", sresp=1212,
             t0=T0 + 28 * MS),
        span(T_PRIO, hx(0x9C), hx(0x9A), tap=1, svc="cart", tcp=7000,
             t0=T0 + 29 * MS),
        # span rule wins over syscall and tcp
        span(T_PRIO, hx(0x9D), hx(0x9A), tap=0, svc="pay", sreq=1212,
             tcp=7000, t0=T0 + 30 * MS, status=3),
        # no parent id: syscall wins over tcp
        span(T_PRIO, hx(0x9E), tap=0, svc="db", sreq=1212, tcp=7000,
             t0=T0 + 31 * MS),
        # dangling parent id and syscall id: tcp is what is left
        span(T_PRIO, hx(0x9F), hx(0xBAD), tap=0, svc="mail", sreq=3434,
             tcp=7000, t0=T0 + 32 * MS, status=4),
    ])

    groups.append([span(T_SINGLE, hx(0x51), svc="stock", t0=T_SINGLE_START)])

    # 16 characters that are not hex: hashed on both sides
    groups.append([
        span(T_ZZ, "zzzzzzzzzzzzzzzz", svc="front", t0=T0 + 34 * MS),
        span(T_ZZ, hx(0x22), "zzzzzzzzzzzzzzzz", svc="db", t0=T0 + 35 * MS),
    ])

    # window case: the root starts before WINDOW_LO, its child inside
    groups.append([
        span(T_WINDOW, hx(0x31), svc="front", t0=T0 - 10_000 * MS,
             dur=20_000 * MS),
        span(T_WINDOW, hx(0x32), hx(0x31), svc="cart", t0=T0 + 36 * MS),
        span(T_WINDOW, hx(0x33), hx(0x32), svc="db", t0=T0 + 37 * MS),
    ])

    # rows without a trace id: excluded, though their ids would match
    groups.append([span("", hx(0x1000 + i), hx(0x1000 + i - 1), svc="front",
                        sreq=777, sresp=777, tcp=5000, tap=i % 2,
                        t0=T0 + (40 + i) * MS) for i in range(25)])

    # filler: traces of 2-64 spans, mixed link kinds and services
    rng = random.Random(20261020)
    n_fill = 0
    t = 0
    while n_fill < 1100:
        size = rng.choice([2, 3, 5, 9, 17, 33, 64])
        tid = hx(0xF000000 + t, 32) if t % 3 else f"filler-trace-{t}"
        g = []
        for i in range(size):
            sid = hx((t << 16) | (i + 1)) if (t + i) % 4 else f"f{t}-{i}"
            kw = dict(svc=rng.choice(SERVICES), t0=T0 + (100 + n_fill) * MS,
                      dur=rng.randrange(1, 50) * MS,
                      status=rng.choice([0, 0, 0, 0, 3, 4]))
            if i:
                j = rng.randrange(i)          # parent: an earlier span
                how = rng.randrange(4)
                if how <= 1:
                    kw["parent"] = g[j]["trace_info"]["span_id"]
                elif how == 2:                # syscall link
                    sid_j = g[j]["base"]["syscall_trace_id_response"] or \
                        10_000 + (t << 8) + j
                    g[j]["base"]["syscall_trace_id_response"] = sid_j
                    kw["sreq"] = sid_j
                else:                         # tcp link to a client span
                    if g[j]["base"]["tap_side"] == 1 and \
                            g[j]["base"]["req_tcp_seq"]:
                        kw["tcp"] = g[j]["base"]["req_tcp_seq"]
                    elif g[j]["base"]["req_tcp_seq"] == 0:
                        g[j]["base"]["tap_side"] = 1
                        g[j]["base"]["req_tcp_seq"] = 50_000 + n_fill
                        kw["tcp"] = 50_000 + n_fill
            g.append(span(tid, sid, **kw))
            n_fill += 1
        groups.append(g)
        t += 1

    # interleave the traces, keeping each trace's own order
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
        out.append(span(hx(0xEE0 + len(out), 32), hx(len(out)),
                        svc="stock", t0=T0 + 2000 * MS))
    return out


def payloads_of(spans, chunk: int = 97):
    """One frame payload per `chunk` spans: a batch has to fit the tail
    segment, and 97-row batches leave every 256-row segment part-filled."""
    return [framing.pack_records(
        [pb.encode(s, flow_log.APP_PROTO_LOGS_DATA)
         for s in spans[i:i + chunk]]) for i in range(0, len(spans), chunk)]


def trace_ids_of(spans):
    seen = []
    for s in spans:
        t = s["trace_info"]["trace_id"]
        if t and t not in seen:
            seen.append(t)
    return seen
