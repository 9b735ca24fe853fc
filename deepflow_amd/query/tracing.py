"""Distributed-tracing assembly: spans -> trace tree.

The MI355X-native analog of the reference's tracing query path (the
SIGCOMM'23 join: spans related by trace_id, parent span ids,
syscall_trace_id and tcp_seq — SURVEY.md §2.5, libs/tracetree). Fetches the
trace's spans from the GPU store (string-hash filter on trace_id), links
parents three ways, and emits the tree.
"""
from __future__ import annotations

from typing import Dict, List, Optional


class DistributedTracer:
    def __init__(self, engine):
        self.engine = engine
        # assembled-tree summaries (reference: libs/tracetree rows written
        # back by the ingester; ours caches on assembly)
        self.tree_rows = []

    def fetch_spans(self, trace_id: str) -> List[Dict]:
        r = self.engine.query(
            "SELECT trace_id, span_id, parent_span_id, request_resource, "
            "service_name, start_time, end_time, response_status, "
            "syscall_trace_id_request, syscall_trace_id_response, "
            "req_tcp_seq, resp_tcp_seq, tap_side, flow_id "
            f"FROM l7_flow_log WHERE trace_id = '{trace_id}' LIMIT 10000")
        cols = r["columns"]
        return [dict(zip(cols, row)) for row in r["values"]]

    def assemble(self, trace_id: str) -> Dict:
        spans = self.fetch_spans(trace_id)
        by_span_id: Dict[str, int] = {}
        for i, s in enumerate(spans):
            sid = s.get("span_id")
            if sid:
                by_span_id.setdefault(sid, i)
        # syscall join: a span whose syscall_trace_id_request equals another
        # span's syscall_trace_id_response belongs below it (same thread
        # carried the request across the process)
        by_syscall_resp: Dict[int, int] = {}
        by_tcp_seq: Dict[int, int] = {}
        for i, s in enumerate(spans):
            v = s.get("syscall_trace_id_response") or 0
            if v:
                by_syscall_resp.setdefault(v, i)
            seq = s.get("req_tcp_seq") or 0
            if seq and s.get("tap_side") == 1:  # client-side emitter
                by_tcp_seq.setdefault(seq, i)
        nodes = []
        for i, s in enumerate(spans):
            parent: Optional[int] = None
            psid = s.get("parent_span_id")
            if psid and psid in by_span_id and by_span_id[psid] != i:
                parent = by_span_id[psid]
            if parent is None:
                v = s.get("syscall_trace_id_request") or 0
                if v and v in by_syscall_resp and by_syscall_resp[v] != i:
                    parent = by_syscall_resp[v]
            if parent is None and s.get("tap_side") != 1:
                seq = s.get("req_tcp_seq") or 0
                if seq and seq in by_tcp_seq and by_tcp_seq[seq] != i:
                    parent = by_tcp_seq[seq]
            nodes.append({
                "index": i,
                "span_id": s.get("span_id"),
                "parent_index": parent,
                "service": s.get("service_name"),
                "resource": s.get("request_resource"),
                "start_time": s.get("start_time"),
                "duration_ns": max((s.get("end_time") or 0) -
                                   (s.get("start_time") or 0), 0),
                "status": s.get("response_status"),
                "children": [],
            })
        roots = []
        for n in nodes:
            if n["parent_index"] is not None:
                nodes[n["parent_index"]]["children"].append(n["index"])
            else:
                roots.append(n["index"])
        result = {"trace_id": trace_id, "spans": nodes, "roots": roots,
                  "span_count": len(nodes)}
        if nodes:
            def depth(i, d=0):
                n = nodes[i]
                return max([d] + [depth(c, d + 1) for c in n["children"]])
            root = nodes[roots[0]] if roots else nodes[0]
            self.tree_rows.append({
                "time": (root["start_time"] or 0) // 10**9,
                "trace_id": trace_id,
                "span_count": len(nodes),
                "max_depth": max(depth(r) for r in roots) if roots else 0,
                "root_service": root["service"] or "",
                "duration_us": root["duration_ns"] // 1000,
            })
        return result

    # ------------------------------------------------- bulk assembly (K10)
    def trace_map(self, time_start: Optional[int] = None,
                  time_end: Optional[int] = None) -> Dict:
        """Per-trace summaries and the service -> service edge table for
        every trace with spans in [time_start, time_end] (ns, inclusive);
        see query/tracemap.py."""
        from .tracemap import TraceMapper
        return TraceMapper(self.engine).trace_map(time_start, time_end)

    def build_trace_trees(self, time_start: Optional[int] = None,
                          time_end: Optional[int] = None) -> Dict:
        """Upsert one `trace_tree` row per trace in the window (the same
        six fields `assemble()` caches), replacing a row with the same
        trace_id."""
        tm = self.trace_map(time_start, time_end)
        at = {r["trace_id"]: i for i, r in enumerate(self.tree_rows)}
        for t in tm["traces"]:
            row = {k: t[k] for k in ("time", "trace_id", "span_count",
                                     "max_depth", "root_service",
                                     "duration_us")}
            i = at.get(t["trace_id"])
            if i is None:
                at[t["trace_id"]] = len(self.tree_rows)
                self.tree_rows.append(row)
            else:
                self.tree_rows[i] = row
        return {"traces": tm["trace_count"], "spans": tm["span_count"],
                "drops": tm["drops"], "rows": len(self.tree_rows)}

    # ----------------------------------------------------- flow groups (K12)
    def flow_groups(self, time_start: Optional[int] = None,
                    time_end: Optional[int] = None,
                    min_spans: int = 2) -> Dict:
        """Summaries of the groups that the spans in [time_start, time_end]
        form through shared trace ids, syscall trace ids, tcp sequence
        pairs and x-request-ids, spans without a trace id included; see
        query/flowgroups.py."""
        from .flowgroups import FlowGrouper
        return FlowGrouper(self.engine).flow_groups(time_start, time_end,
                                                    min_spans)

    def flow_trace(self, time_start: Optional[int] = None,
                   time_end: Optional[int] = None, *,
                   trace_id: Optional[str] = None,
                   syscall_trace_id: Optional[int] = None,
                   x_request_id: Optional[str] = None,
                   limit: int = 10000) -> Dict:
        """The spans of the flow group that one id belongs to, in row
        order. Exactly one of the three ids must be given."""
        from .flowgroups import FlowGrouper
        return FlowGrouper(self.engine).flow_trace(
            time_start, time_end, trace_id=trace_id,
            syscall_trace_id=syscall_trace_id, x_request_id=x_request_id,
            limit=limit)

    def register(self, app) -> None:
        # fixed paths first: the parameterised route below would swallow them
        @app.get("/v1/tracing/map")
        def tracing_map(time_start: Optional[int] = None,
                        time_end: Optional[int] = None):
            return self.trace_map(time_start, time_end)

        @app.get("/v1/tracing/groups")
        def tracing_groups(time_start: Optional[int] = None,
                           time_end: Optional[int] = None,
                           min_spans: int = 2):
            return self.flow_groups(time_start, time_end, min_spans)

        @app.get("/v1/tracing/flow")
        def tracing_flow(time_start: Optional[int] = None,
                         time_end: Optional[int] = None,
                         trace_id: Optional[str] = None,
                         syscall_trace_id: Optional[int] = None,
                         x_request_id: Optional[str] = None,
                         limit: int = 10000):
            try:
                return self.flow_trace(
                    time_start, time_end, trace_id=trace_id,
                    syscall_trace_id=syscall_trace_id,
                    x_request_id=x_request_id, limit=limit)
            except ValueError as e:
                from fastapi import HTTPException
                raise HTTPException(status_code=400, detail=str(e))

        @app.post("/v1/tracing/trees/build")
        def tracing_build(time_start: Optional[int] = None,
                          time_end: Optional[int] = None):
            return self.build_trace_trees(time_start, time_end)

        @app.get("/v1/tracing/{trace_id}")
        def tracing(trace_id: str):
            return self.assemble(trace_id)
