#!/usr/bin/env python3
"""What the path folds cost next to the hop counts they share their trees with (DESIGN.md,
"Path folds").

  fold1  : shd_route_fold_async, 1,024 sources x all vertices, one fold (SUM of the latencies)
  fold4  : the same call with four folds (SUM, MIN, MAX, PROD over four value columns)
  hops   : shd_route_hops_async, the same sources on the same build

Prints one JSON line per config: the median of --reps timed calls after --warmup, the ratios
to the hops call and whether four folds in one call cost less than four calls of one.
    python tools/fold_bench.py [--configs c4,c3] [--sources 1024] [--reps 5]
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
    ops = [route.FOLD_SUM, route.FOLD_MIN, route.FOLD_MAX, route.FOLD_PROD]
    for name in [c for c in a.configs.split(",") if c]:
        g = config(name)
        eng = route.RouteEngine(g)
        ns, m = min(a.sources, g.n), eng.info["n_edges"]
        src = torch.from_numpy(np.linspace(0, g.n - 1, ns).astype(np.int32)).to(dev)
        tgt = torch.arange(g.n, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(1)
        vals = np.stack([np.asarray(g.latency, np.float64), rng.integers(1, 10, size=m).astype(np.float64),
                         1.0 - rng.random(m), 1.0 - np.asarray(g.packetloss, np.float64)])
        val = torch.from_numpy(vals).to(dev)
        out = torch.empty((4, ns, g.n), dtype=torch.float64, device=dev)
        hops = torch.empty((ns, g.n), dtype=torch.int32, device=dev)
        mx = torch.empty(ns, dtype=torch.int32, device=dev)

        def sync():  # a source without a self-loop fails its own entry: not an error here
            try:
                eng.sync()
            except route.RouteError as err:
                if err.code not in (route.ENOEDGE, route.EUNREACH):
                    raise

        t_hops = timed(lambda: eng.hops_async(src, tgt, hops, mx, dispatch=False), sync, a.warmup, a.reps)
        t_1 = timed(lambda: eng.fold_async(src, tgt, ops[:1], val, out, dispatch=False), sync, a.warmup, a.reps)
        t_4 = timed(lambda: eng.fold_async(src, tgt, ops, val, out, dispatch=False), sync, a.warmup, a.reps)
        print(json.dumps({"what": "fold_vs_hops", "config": name, "n": g.n, "edges": m, "sources": ns,
                          "kernel": eng.info["kernel"], "hops_ms": round(1e3 * t_hops[0], 3),
                          "fold1_ms": round(1e3 * t_1[0], 3), "fold4_ms": round(1e3 * t_4[0], 3),
                          "fold1_over_hops": round(t_1[0] / t_hops[0], 3), "fold4_over_hops": round(t_4[0] / t_hops[0], 3),
                          "fold4_over_4x_fold1": round(t_4[0] / (4 * t_1[0]), 3),
                          "fold4_cheaper_than_4x_fold1": bool(t_4[0] < 4 * t_1[0]),
                          "lat_sum_nan": int(torch.isnan(out[0]).sum().item()), "build": bid}), flush=True)
        eng.close()
        del out, hops, val


if __name__ == "__main__":
    main()
