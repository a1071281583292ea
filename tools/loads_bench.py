#!/usr/bin/env python3
"""What the link loads cost next to the hop counts and the distance rows they are built on
("Link loads").

  loads  : shd_route_loads_async, 1,024 sources x all vertices, unit weights (dense) and
           weights on ~1% of the targets, the rest zero (sparse)
  hops   : shd_route_hops_async, the same sources on the same build
  rows   : shd_route_rows_async, latency only, the same sources

Prints one JSON line per config: the median of --reps timed calls after --warmup.
    python tools/loads_bench.py [--configs c4,c3] [--sources 1024] [--reps 5]
For the per-kernel breakdown run it once under a kernel trace with --reps 1 --warmup 0.
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
    ap.add_argument("--sparse", type=float, default=0.01, help="share of the targets that carry weight in the sparse run")
    a = ap.parse_args()
    torch.cuda.init()
    from shadow_amd import build, route
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
        el = torch.empty(eng.info["n_edges"], dtype=torch.int64, device=dev)
        tr = torch.empty(g.n, dtype=torch.int64, device=dev)
        un = torch.empty(1, dtype=torch.int64, device=dev)
        gen = torch.Generator(device=dev).manual_seed(1)
        wt = (torch.rand((ns, g.n), device=dev, generator=gen) < a.sparse).to(torch.int64)
        t_rows = timed(lambda: eng.rows_async(src, tgt, lat, None, None, dispatch=False), eng.sync, a.warmup, a.reps)
        t_hops = timed(lambda: eng.hops_async(src, tgt, hops, mx, dispatch=False), eng.sync, a.warmup, a.reps)

        def sync_loads():  # a source without a self-loop fails its own entry: not an error here
            try:
                eng.sync()
            except route.RouteError as err:
                if err.code not in (route.ENOEDGE, route.EUNREACH):
                    raise

        t_dense = timed(lambda: eng.loads_async(src, tgt, None, el, tr, un, dispatch=False), sync_loads, a.warmup, a.reps)
        dense_sum = int(el.sum().item())
        t_sparse = timed(lambda: eng.loads_async(src, tgt, wt, el, tr, un, dispatch=False), sync_loads, a.warmup, a.reps)
        print(json.dumps({"what": "loads_vs_hops_vs_rows", "config": name, "n": g.n, "edges": eng.info["n_edges"],
                          "sources": ns, "kernel": eng.info["kernel"], "rows_ms": round(1e3 * t_rows[0], 3),
                          "hops_ms": round(1e3 * t_hops[0], 3), "loads_ms": round(1e3 * t_dense[0], 3),
                          "loads_sparse_ms": round(1e3 * t_sparse[0], 3), "sparse_share": a.sparse,
                          "loads_over_rows": round(t_dense[0] / t_rows[0], 3),
                          "edge_load_sum": dense_sum, "sparse_edge_load_sum": int(el.sum().item()), "build": bid}),
              flush=True)
        eng.close()
        del lat, hops, wt


if __name__ == "__main__":
    main()
