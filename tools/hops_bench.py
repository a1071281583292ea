#!/usr/bin/env python3
"""What the path hops cost on top of the distance rows they consume ("Path hops").

  hops : shd_route_hops_async, 1,024 sources x all vertices (hop counts + row maxima)
  rows : shd_route_rows_async, latency only, the same sources on the same build
  dump : shd_topology_dump_routes on C2 with every vertex attached (to /dev/null)

Prints one JSON line per measurement: the median of --reps timed calls after --warmup.
    python tools/hops_bench.py [--configs c4,c3] [--sources 1024] [--reps 5] [--no-dump]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn(); sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(); sync()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c3")
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dump", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    from shadow_amd import build, route, topology
    from shadow_amd.graph import config
    dev = torch.device("cuda:0")
    bid = build.source_id()
    for name in [c for c in a.configs.split(",") if c]:
        g = config(name)
        eng = route.RouteEngine(g)
        ns = min(a.sources, g.n)
        src = torch.from_numpy(np.linspace(0, g.n - 1, ns).astype(np.int32)).to(dev)
        tgt = torch.arange(g.n, dtype=torch.int32, device=dev)
        lat = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        hops = torch.empty((ns, g.n), dtype=torch.int32, device=dev)
        mx = torch.empty(ns, dtype=torch.int32, device=dev)
        t_rows = timed(lambda: eng.rows_async(src, tgt, lat, None, None, dispatch=False), eng.sync, a.warmup, a.reps)
        t_hops = timed(lambda: eng.hops_async(src, tgt, hops, mx, dispatch=False), eng.sync, a.warmup, a.reps)
        print(json.dumps({"what": "hops_vs_rows", "config": name, "n": g.n, "sources": ns, "kernel": eng.info["kernel"],
                          "rows_ms": round(1e3 * t_rows[0], 3), "hops_ms": round(1e3 * t_hops[0], 3),
                          "ratio": round(t_hops[0] / t_rows[0], 3), "max_hops": int(mx.max().item()),
                          "build": bid}), flush=True)
        eng.close()
        del lat, hops
    if not a.no_dump:
        g = config("c2")
        t = topology.Topology.from_graph(g)
        t.attach_all(range(g.n))
        t.fill()
        t0 = time.perf_counter()
        t.dump_routes(os.devnull)
        dt = time.perf_counter() - t0
        pairs = g.n * (g.n + 1) // 2
        print(json.dumps({"what": "dump_routes", "config": "c2", "attached": g.n, "pairs": pairs,
                          "seconds": round(dt, 3), "build": bid}), flush=True)
        t.close()


if __name__ == "__main__":
    main()
