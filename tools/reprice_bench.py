#!/usr/bin/env python3
"""What a sweep of link repricing scenarios costs next to what a user does today, a context per
scenario ("Link repricing").  A diagnostic rate: it has no target and no test gates it.

  reprice : shd_route_reprice_async, --sources sources x all vertices, unit weights, lat not
            asked for, --scenarios single-edge scenarios, in four variants:
              top_half, top_double        the edges with the highest shd_route_loads load of the
                                          same block at half and at twice their latency
              random_half, random_double  random edges likewise
  fresh   : shd_route_create on the repriced graph plus a lat-only rows call of the block, the
            median over 4 of the top_half scenarios

Prints one JSON line per config: the medians of --reps timed calls after --warmup, per call and
per scenario, and the ratio of the fresh context to one scenario of every variant.
    python tools/reprice_bench.py [--configs c4,c3] [--sources 1024] [--scenarios 256] [--reps 5]
"""
import argparse
import dataclasses
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
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.cuda.init()
    from shadow_amd import build, route
    from shadow_amd.graph import config
    dev = torch.device("cuda:0")
    bid = build.source_id()
    for name in [c for c in a.configs.split(",") if c]:
        g = config(name)
        eng = route.RouteEngine(g)
        ns, m = min(a.sources, g.n), eng.info["n_edges"]
        S = np.linspace(0, g.n - 1, ns).astype(np.int32)
        src = torch.from_numpy(S).to(dev)
        tgt = torch.arange(g.n, dtype=torch.int32, device=dev)

        def sync(e=eng):  # a source without a self-loop fails its own entry: not an error here
            try:
                e.sync()
            except route.RouteError as err:
                if err.code not in (route.ENOEDGE, route.EUNREACH):
                    raise

        load = torch.zeros(m, dtype=torch.int64, device=dev)
        eng.loads_async(src, tgt, None, load, None, None, dispatch=False)
        sync()
        nscn = min(a.scenarios, m)
        glat = np.asarray(g.latency, np.float64)
        top = np.argsort(-load.cpu().numpy(), kind="stable")[:nscn].astype(np.int32)
        rnd = np.random.default_rng(g.n).choice(m, size=nscn, replace=False).astype(np.int32)
        off = torch.arange(nscn + 1, dtype=torch.int64, device=dev)
        stats = torch.zeros((nscn, route.REPRICE_NSTAT), dtype=torch.int64, device=dev)
        mx, mg, mn = (torch.zeros(nscn, dtype=torch.float64, device=dev) for _ in range(3))
        res = {}
        for label, ids, f in (("top_half", top, 0.5), ("top_double", top, 2.0), ("random_half", rnd, 0.5),
                              ("random_double", rnd, 2.0)):
            edge = torch.from_numpy(ids).to(dev)
            nl = torch.from_numpy(glat[ids] * f).to(dev)
            t = timed(lambda: eng.reprice_async(src, tgt, None, off, edge, nl, stats, mx, mg, mn, None, None), sync,
                      a.warmup, a.reps)
            st = stats.cpu().numpy()
            res[label] = {"ms": round(1e3 * t[0], 3), "ms_per_scenario": round(1e3 * t[0] / nscn, 4),
                          "hit_share": round(float(st[:, route.REPRICE_HIT].sum()) / (nscn * ns * g.n), 6),
                          "slower": int(st[:, route.REPRICE_SLOWER].sum()), "faster": int(st[:, route.REPRICE_FASTER].sum()),
                          "max_add": float(mx.max().item()), "max_gain": float(mg.max().item()),
                          "min_new": float(mn.min().item())}
        # today: a context of the repriced graph and its rows, per scenario
        lat = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        fresh = []
        for e in top[:4].tolist():
            w = glat.copy(); w[e] *= 0.5
            gk = dataclasses.replace(g, latency=w)
            t0 = time.perf_counter()
            ek = route.RouteEngine(gk)
            ek.rows_async(src, tgt, lat, None, None, dispatch=False)
            sync(ek)
            fresh.append(time.perf_counter() - t0)
            ek.close()
        f_ms = 1e3 * statistics.median(fresh)
        print(json.dumps({"what": "reprice_vs_fresh_context", "diagnostic": True, "config": name, "n": g.n, "edges": m,
                          "sources": ns, "scenarios": nscn, "kernel": eng.info["kernel"], **res,
                          "fresh_context_ms": round(f_ms, 3),
                          "fresh_over_scenario": {k: round(f_ms / v["ms_per_scenario"], 1) for k, v in res.items()},
                          "build": bid}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
