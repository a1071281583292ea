#!/usr/bin/env python3
"""What the tie envelope costs beside the calls it shares its distance rows with (DESIGN.md,
"Tie envelope").

  ties : shd_route_ties_async, 1,024 sources x all vertices (count, rel_lo, rel_hi)
  hops : shd_route_hops_async, the same sources on the same build (hop counts + row maxima)
  rows : shd_route_rows_async, latency only

Prints one JSON line per configuration: the medians of --reps timed calls after --warmup, the
ties / hops and ties / rows ratios, and what the envelope found (tied, sensitive and saturated
entries, the largest spread).  A diagnostic rate: every call runs the sources' SSSP.
    python tools/ties_bench.py [--configs c4,c3] [--sources 1024] [--reps 5]
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
        ns = min(a.sources, g.n)
        src = torch.from_numpy(np.linspace(0, g.n - 1, ns).astype(np.int32)).to(dev)
        tgt = torch.arange(g.n, dtype=torch.int32, device=dev)
        lat = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        hops = torch.empty((ns, g.n), dtype=torch.int32, device=dev)
        mx = torch.empty(ns, dtype=torch.int32, device=dev)
        cnt = torch.empty((ns, g.n), dtype=torch.int64, device=dev)
        lo = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        hi = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        t_rows = timed(lambda: eng.rows_async(src, tgt, lat, None, None, dispatch=False), sync, a.warmup, a.reps)
        t_hops = timed(lambda: eng.hops_async(src, tgt, hops, mx, dispatch=False), sync, a.warmup, a.reps)
        t_ties = timed(lambda: eng.ties_async(src, tgt, cnt, lo, hi, dispatch=False), sync, a.warmup, a.reps)
        off = tgt[None, :] != src[:, None]
        ok = off & (cnt != 0)
        sens = ok & (lo != hi)
        spread = torch.where(sens, (hi - lo) / hi, torch.zeros_like(hi))
        print(json.dumps({"what": "ties_vs_hops", "config": name, "n": g.n, "sources": ns, "kernel": eng.info["kernel"],
                          "rows_ms": round(1e3 * t_rows[0], 3), "hops_ms": round(1e3 * t_hops[0], 3),
                          "ties_ms": round(1e3 * t_ties[0], 3), "ties_min_ms": round(1e3 * t_ties[1], 3),
                          "ties_over_hops": round(t_ties[0] / t_hops[0], 3),
                          "ties_over_rows": round(t_ties[0] / t_rows[0], 3),
                          "entries": int(ok.sum().item()), "tied": int((ok & (cnt != 1)).sum().item()),
                          "sensitive": int(sens.sum().item()), "saturated": int((ok & (cnt == -1)).sum().item()),
                          "max_spread": float(spread.max().item()), "max_hops": int(mx.max().item()),
                          "build": bid}), flush=True)
        eng.close()
        del lat, hops, cnt, lo, hi, spread, off, ok, sens


if __name__ == "__main__":
    main()
