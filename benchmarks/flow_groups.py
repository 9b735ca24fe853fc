"""Flow groups (K12): GPU flow_groups() vs the host twin on the same window.

Builds a seeded synthetic window in its own generator: --spans spans in
groups. A group is a trace of 2-64 spans sharing a trace id, to which spans
WITHOUT a trace id are attached (about --untraced-share of all spans) by a
syscall trace id, a tcp sequence pair or an x-request-id of a traced span;
one group in eight has no trace id at all (a syscall chain). On top comes
one deliberately large group: --big-group spans on one x-request-id. Spans
are ordered by start time, so groups interleave and cross batches and
segments. Writes one JSON document (default profiles/flow_groups.json).

Timing method: host wall clock (perf_counter) around work that ends in a
device synchronise; one untimed warm-up; median of --repeats runs, spread
reported. flow_groups() is timed end to end (workspace allocation, four
kernels, compaction, D2H, hydration and sorting in Python). The per-kernel
split comes from device events in separate runs, once on the window with
the large group and once on the same window without it. The host twin runs
on host copies of the same segments (--host-repeats runs, no warm-up).

    python benchmarks/flow_groups.py [--spans 1000000 ...]
"""
import argparse
import json
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from deepflow_amd.wire import pb, flow_log, framing

T0 = 1_700_000_000_000_000_000
SIZES = [2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64]
BIG_XREQ = "big-group-request-id"


def _span(t_ns, rng, flow, trace="", sid="", **base_kw):
    base = {"start_time": t_ns,
            "end_time": t_ns + int(rng.integers(1000, 50_000_000)),
            "flow_id": flow, "vtap_id": 1, "tap_side": 0,
            "head": {"proto": 20, "msg_type": 2, "rrt": 100},
            "ip_src": 0x0A000001, "ip_dst": 0x0A000002,
            "port_src": 40000, "port_dst": 8080, "protocol": 6}
    base.update(base_kw)
    return {"base": base, "req": {"req_type": "GET", "resource": "/r"},
            "resp": {"status": 3 if rng.random() < 0.02 else 0, "code": 200},
            "trace_info": {"trace_id": trace, "span_id": sid},
            "ext_info": {"service_name": f"svc-{int(rng.integers(40))}"}}


def gen_groups(job):
    """Worker: groups [lo, hi) -> [(start_ns, encoded span)], seeded per
    group so the set does not depend on the worker split."""
    lo, hi, seed, share, window_ns = job
    out = []
    for t in range(lo, hi):
        rng = np.random.default_rng([seed, t])
        size = SIZES[int(rng.integers(len(SIZES)))]
        t_start = T0 + int(rng.integers(window_ns))
        tid = "" if t % 8 == 7 else f"{t + 1:032x}"
        spans = []
        for i in range(size):
            kw = {}
            if not tid and i:       # untraced group: a syscall chain
                kw["syscall_trace_id_request"] = (t << 8) + i
            if not tid and i < size - 1:
                kw["syscall_trace_id_response"] = (t << 8) + i + 1
            spans.append(_span(t_start + i * 1000, rng, t, tid,
                               f"{(t << 8) | (i + 1):016x}" if tid else "",
                               **kw))
        # spans without a trace id, attached to a traced span
        n_extra = int(rng.binomial(size, share / (1 - share))) if tid else 0
        for i in range(n_extra):
            host = spans[int(rng.integers(size))]
            hb, he = host["base"], host["ext_info"]
            how = int(rng.integers(3))
            s = _span(t_start + (size + i) * 1000, rng, t)
            if how == 0:
                sid = hb.setdefault("syscall_trace_id_response",
                                    (t << 8) + 128 + i)
                s["base"]["syscall_trace_id_request"] = sid
            elif how == 1:
                hb.setdefault("req_tcp_seq", 1 + ((t << 7) + i) % 0xFFFFFFF0)
                hb.setdefault("resp_tcp_seq", 1 + (t * 31 + i) % 0xFFFFFFF0)
                s["base"]["req_tcp_seq"] = hb["req_tcp_seq"]
                s["base"]["resp_tcp_seq"] = hb["resp_tcp_seq"]
            else:
                he.setdefault("x_request_id_1", f"xr-{t}-{i}")
                s["ext_info"]["x_request_id_0"] = he["x_request_id_1"]
            spans.append(s)
        out += [(s["base"]["start_time"],
                 pb.encode(s, flow_log.APP_PROTO_LOGS_DATA)) for s in spans]
    return out


def gen_big(job):
    lo, hi, seed, window_ns = job
    rng = np.random.default_rng([seed, 1 << 40, lo])
    out = []
    for i in range(lo, hi):
        s = _span(T0 + int(rng.integers(window_ns)), rng, i)
        s["ext_info"]["x_request_id_0"] = BIG_XREQ
        out.append((s["base"]["start_time"],
                    pb.encode(s, flow_log.APP_PROTO_LOGS_DATA)))
    return out


def gen_window(a):
    per_group = (sum(SIZES) / len(SIZES)) * (7 / 8 / (1 - a.untraced_share)
                                             + 1 / 8)
    n_groups = int((a.spans - a.big_group) / per_group)
    window_ns = a.window_s * 10**9
    step = max(n_groups // (a.workers * 4), 1)
    jobs = [(lo, min(lo + step, n_groups), a.seed, a.untraced_share,
             window_ns) for lo in range(0, n_groups, step)]
    bstep = max(a.big_group // a.workers, 1)
    bjobs = [(lo, min(lo + bstep, a.big_group), a.seed, window_ns)
             for lo in range(0, a.big_group, bstep)]
    with ProcessPoolExecutor(max_workers=a.workers) as ex:
        recs = [r for part in ex.map(gen_groups, jobs) for r in part]
        big = [r for part in ex.map(gen_big, bjobs) for r in part]
    return recs, big, n_groups


def payloads_of(recs, batch):
    recs = sorted(recs, key=lambda r: r[0])
    return [framing.pack_records([r[1] for r in recs[i:i + batch]])
            for i in range(0, len(recs), batch)]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "runs": len(xs)}


def host_copy(pipe):
    """A cpu pipeline whose segments are host copies of `pipe`'s, sharing
    its dictionary (same ids), for the host twin."""
    from deepflow_amd.ingest import L7IngestPipeline
    from deepflow_amd.store.segment import L7Segment
    hp = L7IngestPipeline(device="cpu", segment_rows=pipe.segments.segment_rows,
                          dict_capacity=1 << 10,
                          time_base_s=pipe.time_base_s)
    hp.dict = pipe.dict
    for seg in pipe.segments.segments:
        c = L7Segment.__new__(L7Segment)
        for k, v in vars(seg).items():
            setattr(c, k, v.cpu() if hasattr(v, "cpu") else v)
        c.device = "cpu"
        hp.segments.segments.append(c)
    return hp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, default=1_000_000)
    ap.add_argument("--untraced-share", type=float, default=0.3)
    ap.add_argument("--big-group", type=int, default=50_000)
    ap.add_argument("--window-s", type=int, default=300)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--segment-rows", type=int, default=1 << 18)
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--out", default="profiles/flow_groups.json")
    a = ap.parse_args()

    # generate before the GPU is opened: the workers are plain forks
    recs, big, n_groups = gen_window(a)

    import torch
    assert torch.cuda.is_available(), "flow_groups.py measures on a GPU"
    from deepflow_amd.ingest import L7IngestPipeline
    from deepflow_amd.query import QueryEngine
    from deepflow_amd.query.flowgroups import FlowGrouper

    sync = torch.cuda.synchronize

    def load(records):
        pipe = L7IngestPipeline(device="cuda", segment_rows=a.segment_rows,
                                dict_capacity=1 << 16)
        for p in payloads_of(records, a.batch):
            pipe.ingest_frame_payload(p)
        sync()
        return pipe

    def timed(fn, repeats, warm=True):
        if warm:
            fn()
            sync()
        ms = []
        for _ in range(repeats):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, med(ms)

    def kernel_split(grouper):
        runs = []
        for _ in range(a.repeats + 1):
            grouper.kernel_ms = {}
            grouper.flow_groups(min_spans=1)
            runs.append(grouper.kernel_ms)
        grouper.kernel_ms = None
        k = {n: med([r[n] for r in runs[1:]]) for n in runs[0]}
        total = sum(v["median"] for v in k.values())
        return {"kernels_ms": k, "sum_ms": total,
                "share": {n: v["median"] / total for n, v in k.items()}}

    # the same window without the large group first, then with it
    pipe0 = load(recs)
    split_without = kernel_split(FlowGrouper(QueryEngine(pipe0,
                                                         device="cuda")))
    del pipe0
    torch.cuda.empty_cache()

    pipe = load(recs + big)
    n_spans = len(recs) + len(big)
    gpu = FlowGrouper(QueryEngine(pipe, device="cuda"))
    g_all, g_ms = timed(lambda: gpu.flow_groups(min_spans=1), a.repeats)
    g_links, g_link_ms = timed(gpu.link_groups, a.repeats)
    assert g_all["drops"] == 0 and g_all["span_count"] == n_spans
    split_with = kernel_split(gpu)

    host = FlowGrouper(QueryEngine(host_copy(pipe), device="cpu"))
    h_all, h_ms = timed(lambda: host.flow_groups(min_spans=1),
                        a.host_repeats, warm=False)

    sizes = sorted(g["span_count"] for g in g_all["groups"])
    untraced = n_spans - sum(g["traced_spans"] for g in g_all["groups"])
    notes = []
    for name in ("extract", "union", "fold"):
        w, wo = split_with["share"][name], split_without["share"][name]
        ms_w = split_with["kernels_ms"][name]["median"]
        ms_wo = split_without["kernels_ms"][name]["median"]
        notes.append(
            f"k_flow_{name}: {ms_wo:.3f} ms ({wo:.0%} of device time) "
            f"without the large group, {ms_w:.3f} ms ({w:.0%}) with it")
    fold_w = split_with["kernels_ms"]["fold"]["median"]
    fold_wo = split_without["kernels_ms"]["fold"]["median"]
    notes.append(
        "single-root contention: every row of the large group adds to the "
        "same per-group words in k_flow_fold (and takes atomicMin on one "
        "index row word in k_flow_extract); it "
        + ("dominates" if split_with["share"]["fold"] > 0.5
           else "does not dominate")
        + f" device time (fold x{fold_w / fold_wo:.1f} with the group)")
    notes.append(
        f"device time is {split_with['sum_ms']:.2f} ms of "
        f"{g_ms['median']:.1f} ms end to end; the rest is workspace "
        "allocation and initialisation, compaction, D2H and Python "
        "hydration of the group rows")

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up; median of N runs; flow_groups timed "
                  "end to end incl. Python hydration; kernels from device "
                  "events in separate runs; host twin without warm-up",
        "shapes": {"spans": n_spans, "groups_generated": n_groups + 1,
                   "groups_found": g_all["group_count"],
                   "untraced_spans": untraced,
                   "untraced_share": untraced / n_spans,
                   "big_group_spans": len(big),
                   "largest_groups": sizes[-3:],
                   "window_s": a.window_s, "segment_rows": a.segment_rows,
                   "segments": len(pipe.segments.segments), "seed": a.seed,
                   "attach_mix": "1/3 syscall id, 1/3 tcp pair, 1/3 "
                                 "x-request-id; 1 group in 8 untraced"},
        "gpu_flow_groups_ms": g_ms,
        "gpu_link_groups_ms": g_link_ms,
        "gpu_kernels_with_big_group": split_with,
        "gpu_kernels_without_big_group": split_without,
        "host_twin_flow_groups_ms": h_ms,
        "groups_equal": g_all == h_all,
        "host_over_gpu": h_ms["median"] / g_ms["median"],
        "gpu_spans_per_s": n_spans / (g_ms["median"] / 1e3),
        "notes": notes,
    }
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
