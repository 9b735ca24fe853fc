"""Bulk trace assembly (K10): GPU trace_map vs the host twin vs looping the
per-trace assemble() over the same window.

Builds a seeded synthetic window in its own generator (gen/spans.py gives
every span its own trace): --spans spans in traces of 2-64 spans, parents
linked by span id, syscall id or tcp seq, a few dozen services so the edge
table is contended. Spans are ordered by start time, so traces interleave
and links cross batches and segments. Writes one JSON document (default
profiles/trace_map.json).

Timing method: host wall clock (perf_counter) around work that ends in a
device synchronise; one untimed warm-up; median of --repeats runs, spread
reported. trace_map() is timed end to end (workspace allocation, four
kernels, compaction, D2H, hydration and sorting in Python). The per-kernel
split comes from device events in separate runs. The host twin runs on
host copies of the same segments. assemble() is timed on the GPU engine
for --assemble-sample traces and scaled to the window's trace count.

    python benchmarks/trace_map.py [--spans 1000000 ...]
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


def gen_traces(job):
    """Worker: traces [lo, hi) -> [(start_ns, encoded span)], seeded per
    trace so the set does not depend on the worker split."""
    lo, hi, seed, n_services, window_ns = job
    out = []
    for t in range(lo, hi):
        rng = np.random.default_rng([seed, t])
        size = SIZES[int(rng.integers(len(SIZES)))]
        tid = f"{t + 1:032x}"
        t_start = T0 + int(rng.integers(window_ns))
        spans = []
        for i in range(size):
            base = {"start_time": t_start + i * 1000,
                    "end_time": t_start + i * 1000 +
                    int(rng.integers(1000, 50_000_000)),
                    "flow_id": t, "vtap_id": 1, "tap_side": 0,
                    "head": {"proto": 20, "msg_type": 2, "rrt": 100},
                    "ip_src": 0x0A000001, "ip_dst": 0x0A000002,
                    "port_src": 40000, "port_dst": 8080, "protocol": 6}
            ti = {"trace_id": tid, "span_id": f"{(t << 8) | (i + 1):016x}"}
            if i:
                j = int(rng.integers(i))
                how = int(rng.integers(20))
                pb_ = spans[j]["base"]
                if how < 14:
                    ti["parent_span_id"] = spans[j]["trace_info"]["span_id"]
                elif how < 17:
                    sid = pb_.get("syscall_trace_id_response") or \
                        (t << 8) + j + 1
                    pb_["syscall_trace_id_response"] = sid
                    base["syscall_trace_id_request"] = sid
                elif pb_.get("req_tcp_seq", 0) == 0 or pb_["tap_side"] == 1:
                    pb_["tap_side"] = 1
                    pb_["req_tcp_seq"] = pb_.get("req_tcp_seq") or \
                        1 + ((t << 6) + j) % 0xFFFFFFF0
                    base["req_tcp_seq"] = pb_["req_tcp_seq"]
            spans.append({
                "base": base,
                "req": {"req_type": "GET", "resource": "/r"},
                "resp": {"status": 3 if rng.random() < 0.02 else 0,
                         "code": 200},
                "trace_info": ti,
                "ext_info": {"service_name":
                             f"svc-{int(rng.integers(n_services))}"}})
        out += [(s["base"]["start_time"],
                 pb.encode(s, flow_log.APP_PROTO_LOGS_DATA)) for s in spans]
    return out


def gen_window(a):
    n_traces = int(a.spans / (sum(SIZES) / len(SIZES)))
    step = max(n_traces // (a.workers * 4), 1)
    jobs = [(lo, min(lo + step, n_traces), a.seed, a.services,
             a.window_s * 10**9) for lo in range(0, n_traces, step)]
    with ProcessPoolExecutor(max_workers=a.workers) as ex:
        recs = [r for part in ex.map(gen_traces, jobs) for r in part]
    recs.sort(key=lambda r: r[0])
    payloads = [framing.pack_records([r[1] for r in recs[i:i + a.batch]])
                for i in range(0, len(recs), a.batch)]
    return payloads, len(recs), n_traces


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
    ap.add_argument("--services", type=int, default=40)
    ap.add_argument("--window-s", type=int, default=300)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--segment-rows", type=int, default=1 << 18)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=5)
    ap.add_argument("--assemble-sample", type=int, default=24)
    ap.add_argument("--out", default="profiles/trace_map.json")
    a = ap.parse_args()

    # generate before the GPU is opened: the workers are plain forks
    payloads, n_spans, n_traces = gen_window(a)

    import torch
    assert torch.cuda.is_available(), "trace_map.py measures on a GPU"
    from deepflow_amd.ingest import L7IngestPipeline
    from deepflow_amd.query import QueryEngine
    from deepflow_amd.query.tracemap import TraceMapper
    from deepflow_amd.query.tracing import DistributedTracer

    sync = torch.cuda.synchronize
    pipe = L7IngestPipeline(device="cuda", segment_rows=a.segment_rows,
                            dict_capacity=1 << 16)
    for p in payloads:
        pipe.ingest_frame_payload(p)
    sync()
    engine = QueryEngine(pipe, device="cuda")
    gpu = TraceMapper(engine)

    def timed(fn, repeats):
        out = fn()                           # warm-up
        sync()
        ms = []
        for _ in range(repeats):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, med(ms)

    g_map, g_ms = timed(gpu.trace_map, a.repeats)
    g_links, g_link_ms = timed(gpu.link_spans, a.repeats)
    assert g_map["drops"] == 0 and g_map["span_count"] == n_spans

    kernel_runs = []
    for _ in range(a.repeats + 1):
        gpu.kernel_ms = {}
        gpu.trace_map()
        kernel_runs.append(gpu.kernel_ms)
    gpu.kernel_ms = None
    kernels = {k: med([r[k] for r in kernel_runs[1:]])
               for k in kernel_runs[0]}

    host = TraceMapper(QueryEngine(host_copy(pipe), device="cpu"))
    h_map, h_ms = timed(host.trace_map, a.host_repeats)

    # the only way to this information without the bulk path: assemble()
    # per trace id (GPU engine), timed on a sample and scaled
    tracer = DistributedTracer(engine)
    ids = [t["trace_id"] for t in g_map["traces"]]
    step = max(len(ids) // a.assemble_sample, 1)
    sample = ids[::step][: a.assemble_sample]
    tracer.assemble(sample[0])               # warm-up
    a_ms, a_spans = [], 0
    for tid in sample:
        sync()
        t0 = time.perf_counter()
        r = tracer.assemble(tid)
        sync()
        a_ms.append((time.perf_counter() - t0) * 1e3)
        a_spans += r["span_count"]
    per_trace = statistics.mean(a_ms)

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up; median of N runs; trace_map timed end "
                  "to end incl. Python hydration; kernels from device "
                  "events in separate runs",
        "shapes": {"spans": n_spans, "traces": n_traces,
                   "trace_sizes": SIZES, "services": a.services,
                   "window_s": a.window_s, "segment_rows": a.segment_rows,
                   "segments": len(pipe.segments.segments),
                   "edges": len(g_map["edges"]), "seed": a.seed,
                   "link_mix": "70% span id, 15% syscall id, 15% tcp seq"},
        "gpu_trace_map_ms": g_ms,
        "gpu_link_spans_ms": g_link_ms,
        "gpu_kernels_ms": kernels,
        "gpu_kernels_sum_ms": sum(v["median"] for v in kernels.values()),
        "host_twin_trace_map_ms": h_ms,
        "maps_equal": g_map == h_map,
        "host_over_gpu": h_ms["median"] / g_ms["median"],
        "assemble_loop": {
            "sample_traces": len(sample), "sample_spans": a_spans,
            "ms_per_trace": med(a_ms),
            "scaled_to_window_ms": per_trace * len(ids),
            "window_traces": len(ids)},
        "gpu_spans_per_s": n_spans / (g_ms["median"] / 1e3),
    }
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
