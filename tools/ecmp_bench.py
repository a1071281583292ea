#!/usr/bin/env python3
"""What the ECMP link loads cost beside the calls they share their distance rows with
("ECMP link loads").

  ecmp  : shd_route_ecmp_loads_async, 1,024 sources x all vertices, unit weights
  ties  : shd_route_ties_async, the same sources on the same build
  loads : shd_route_loads_async, the single-path loads of the same block
  hops  : shd_route_hops_async
  rows  : shd_route_rows_async, latency only

Prints one JSON line per configuration: the medians of --reps timed calls after --warmup, the
ecmp / ties and ecmp / loads ratios, and the share of edges whose ECMP load differs from the
single-path load.  A diagnostic rate: every call runs the sources' SSSP.
    python tools/ecmp_bench.py [--configs c3,c4] [--sources 1024] [--reps 5]
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
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    from shadow_amd import build, route
    from shadow_amd.graph import config
    dev = torch.device("cuda:0")
    bid = build.source_id()

    def sync_soft(eng):
        try:
            eng.sync()
        except route.RouteError as err:          # a source without a self-loop: its own entry
            if err.code not in (route.ENOEDGE, route.EUNREACH):
                raise

    for name in [c for c in a.configs.split(",") if c]:
        g = config(name)
        eng = route.RouteEngine(g)
        sync = lambda: sync_soft(eng)
        ns, m = min(a.sources, g.n), len(g.src)
        src = torch.from_numpy(np.linspace(0, g.n - 1, ns).astype(np.int32)).to(dev)
        tgt = torch.arange(g.n, dtype=torch.int32, device=dev)
        lat = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        hops = torch.empty((ns, g.n), dtype=torch.int32, device=dev)
        mx = torch.empty(ns, dtype=torch.int32, device=dev)
        cnt = torch.empty((ns, g.n), dtype=torch.int64, device=dev)
        lo = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        hi = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        el, tr, un = (torch.empty(k, dtype=torch.int64, device=dev) for k in (m, g.n, 1))
        eel, etr = (torch.empty(k, dtype=torch.float64, device=dev) for k in (m, g.n))
        eun = torch.empty(1, dtype=torch.int64, device=dev)
        t_rows = timed(lambda: eng.rows_async(src, tgt, lat, None, None, dispatch=False), sync, a.warmup, a.reps)
        t_hops = timed(lambda: eng.hops_async(src, tgt, hops, mx, dispatch=False), sync, a.warmup, a.reps)
        t_loads = timed(lambda: eng.loads_async(src, tgt, None, el, tr, un, dispatch=False), sync, a.warmup, a.reps)
        t_ties = timed(lambda: eng.ties_async(src, tgt, cnt, lo, hi, dispatch=False), sync, a.warmup, a.reps)
        t_ecmp = timed(lambda: eng.ecmp_loads_async(src, tgt, None, eel, etr, eun, dispatch=False), sync, a.warmup,
                       a.reps)
        one = el.to(torch.float64)
        used = (one != 0) | (eel != 0)
        differ = used & ((eel - one).abs() > 1e-9 * torch.maximum(eel, one))
        tdiff = (etr - tr.to(torch.float64)).abs() > 1e-9 * torch.maximum(etr, tr.to(torch.float64))
        print(json.dumps({"what": "ecmp_vs_ties_and_loads", "config": name, "n": g.n, "edges": m, "sources": ns,
                          "kernel": eng.info["kernel"],
                          "rows_ms": round(1e3 * t_rows[0], 3), "hops_ms": round(1e3 * t_hops[0], 3),
                          "loads_ms": round(1e3 * t_loads[0], 3), "ties_ms": round(1e3 * t_ties[0], 3),
                          "ecmp_ms": round(1e3 * t_ecmp[0], 3), "ecmp_min_ms": round(1e3 * t_ecmp[1], 3),
                          "ecmp_over_ties": round(t_ecmp[0] / t_ties[0], 3),
                          "ecmp_over_loads": round(t_ecmp[0] / t_loads[0], 3),
                          "edges_used": int(used.sum().item()), "edges_differ": int(differ.sum().item()),
                          "edges_differ_share": round(float(differ.sum().item()) / max(1, int(used.sum().item())), 4),
                          "edges_differ_share_of_all": round(float(differ.sum().item()) / m, 4),
                          "vertices_differ": int(tdiff.sum().item()),
                          "max_edge_load": float(eel.max().item()), "max_single_path_load": int(el.max().item()),
                          "unrouted": int(eun.item()), "build": bid}), flush=True)
        eng.close()
        del lat, hops, cnt, lo, hi


if __name__ == "__main__":
    main()
