"""Host vs GPU profile store: folded-stack ingest rate and flame-query time.

Generates a seeded synthetic folded workload, feeds the same Profile
payloads to ProfilePipeline(device="cpu") and ProfilePipeline(device="cuda")
and runs the same flame queries on both. Writes one JSON document
(default profiles/profile_fold.json).

Timing method: host wall clock (perf_counter) around work that ends in a
device synchronise; every timed shape is run once untimed first (warm-up);
each figure is the median of --repeats runs (the spread is reported too).
Ingest is timed end to end through ingest_payload (record framing,
protobuf decode, line split, H2D copy, kernel), for two states: "first"
(empty stack dictionary, every distinct stack is new) and "steady" (the
dictionary already holds every stack, the normal state of a continuous
profiler). A "stack" in stacks/s is one folded line, i.e. one stored row.

    python benchmarks/profile_fold.py [--messages 64 --lines 4096 ...]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from deepflow_amd.ingest.profile_pipeline import ProfilePipeline
from deepflow_amd.wire import pb, metric, framing

BAR_STACKS_PER_S = 100_000      # VERDICT.md "next round" #9


def gen_workload(a):
    """-> list of payloads (one per agent push), each --messages-per-payload
    Profile messages of --lines folded lines."""
    rng = np.random.default_rng(a.seed)
    depths = rng.integers(a.min_depth, a.max_depth + 1, a.stacks)
    stacks = []
    for d in depths:
        # few distinct frames near the root, more further down: stacks
        # share prefixes the way real call trees do
        ids = [int(rng.integers(0, min(a.fanout * (k + 1), 4096)))
               for k in range(d)]
        stacks.append(";".join(f"fn_{k}_{i}" for k, i in enumerate(ids)))
    stacks = sorted(set(stacks))
    # zipf-ish popularity: hot stacks repeat, the tail is long
    w = 1.0 / np.arange(1, len(stacks) + 1) ** a.skew
    w /= w.sum()
    payloads, n_lines = [], 0
    for p in range(a.messages // a.messages_per_payload):
        recs = []
        for m in range(a.messages_per_payload):
            k = p * a.messages_per_payload + m
            pick = rng.choice(len(stacks), a.lines, p=w)
            cnt = rng.integers(1, 1000, a.lines)
            data = "\n".join(f"{stacks[i]} {c}"
                             for i, c in zip(pick, cnt)).encode()
            n_lines += a.lines
            recs.append(pb.encode({
                "name": f"svc{k % a.processes}", "format": "folded",
                "data": data, "timestamp": 1_000_000 + k,
                "event_type": 1 + k % 3, "pid": 100 + k % a.processes,
                "process_name": f"proc{k % a.processes}",
                "spy_name": "ebpf", "count": 1}, metric.PROFILE))
        payloads.append(framing.pack_records(recs))
    return payloads, n_lines, len(stacks), float(np.mean(depths))


def sync():
    torch.cuda.synchronize()


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "runs": len(xs)}


def time_ingest(device, payloads, n_lines, repeats, stack_capacity):
    first, steady, pipe = [], [], None
    for rep in range(repeats + 1):          # rep 0 is the warm-up
        pipe = ProfilePipeline(device=device, stack_capacity=stack_capacity)
        sync()
        t0 = time.perf_counter()
        for p in payloads:
            pipe.ingest_payload(p)
        sync()
        t1 = time.perf_counter()
        for p in payloads:
            pipe.ingest_payload(p)
        sync()
        t2 = time.perf_counter()
        if rep:
            first.append(n_lines / (t1 - t0))
            steady.append(n_lines / (t2 - t1))
    return pipe, med(first), med(steady)


def time_flame(pipe, kw, repeats):
    tree = pipe.flame(**kw)                 # warm-up
    sync()
    ms = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        tree = pipe.flame(**kw)
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return tree, med(ms)


def canon(n):
    kids = sorted((canon(c) for c in n["children"]),
                  key=lambda c: (-c["value"], c["name"]))
    return {"name": n["name"], "value": n["value"], "self": n["self"],
            "children": kids}


def count_nodes(n):
    return 1 + sum(count_nodes(c) for c in n["children"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=20000,
                    help="distinct stacks drawn (duplicates are merged)")
    ap.add_argument("--min-depth", type=int, default=4)
    ap.add_argument("--max-depth", type=int, default=48)
    ap.add_argument("--fanout", type=int, default=3)
    ap.add_argument("--skew", type=float, default=1.0)
    ap.add_argument("--messages", type=int, default=64)
    ap.add_argument("--messages-per-payload", type=int, default=8)
    ap.add_argument("--lines", type=int, default=4096,
                    help="folded lines per message")
    ap.add_argument("--processes", type=int, default=8)
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--stack-capacity", type=int, default=1 << 20)
    ap.add_argument("--out", default="profiles/profile_fold.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "profile_fold.py measures on a GPU"
    import sys
    sys.setrecursionlimit(10000)

    payloads, n_lines, n_stacks, mean_depth = gen_workload(a)
    host, h_first, h_steady = time_ingest("cpu", payloads, n_lines,
                                          a.host_repeats, a.stack_capacity)
    gpu, g_first, g_steady = time_ingest("cuda", payloads, n_lines,
                                         a.repeats, a.stack_capacity)
    assert gpu.store.n_rows == len(host.store.rows)
    assert gpu.store.n_stacks == len(host.store.id_to_loc)
    assert gpu.store.stack_drops == 0

    queries = {"all": {}, "one_process": {"process_name": "proc1"},
               "event_and_window": {"event_type": 2,
                                    "time_start": 1_000_010,
                                    "time_end": 1_000_040}}
    flame = {}
    for name, kw in queries.items():
        ht, h_ms = time_flame(host, kw, a.host_repeats)
        gt, g_ms = time_flame(gpu, kw, a.repeats)
        flame[name] = {"filters": kw, "tree_nodes": count_nodes(gt),
                       "trees_equal": canon(ht) == gt,
                       "host_ms": h_ms, "gpu_ms": g_ms}

    out = {
        "device": torch.cuda.get_device_name(0),
        "method": "perf_counter around device-synchronised regions; one "
                  "untimed warm-up per shape; median of N runs; ingest "
                  "timed end to end through ProfilePipeline.ingest_payload",
        "shapes": {"distinct_stacks": n_stacks,
                   "depth_range": [a.min_depth, a.max_depth],
                   "mean_depth_drawn": mean_depth, "fanout": a.fanout,
                   "skew": a.skew, "messages": a.messages,
                   "messages_per_payload": a.messages_per_payload,
                   "lines_per_message": a.lines,
                   "lines_per_pass": n_lines,
                   "rows_at_query": gpu.store.n_rows,
                   "processes": a.processes, "seed": a.seed,
                   "stack_capacity": a.stack_capacity},
        "bar_stacks_per_s": BAR_STACKS_PER_S,
        "ingest_stacks_per_s": {
            "host": {"first": h_first, "steady": h_steady},
            "gpu": {"first": g_first, "steady": g_steady}},
        "gpu_meets_bar": g_steady["median"] >= BAR_STACKS_PER_S
        and g_first["median"] >= BAR_STACKS_PER_S,
        "gpu_over_host_steady": g_steady["median"] / h_steady["median"],
        "flame": flame,
        "gpu_store_bytes": gpu.store.stored_bytes(),
    }
    path = Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
