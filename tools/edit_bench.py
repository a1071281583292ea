#!/usr/bin/env python3
"""What a sweep of link edit scenarios costs next to what a user does today, a context per
scenario ("Link edits").  A diagnostic rate: it has no target and no test gates it.

  edit  : shd_route_edit_async, --sources sources x all vertices, unit weights, lat not asked
          for, --scenarios scenarios, in three variants:
            add         a new link at the graph's median latency between two of the 64 vertices
                        with the highest shd_route_loads transit load of the same block
            rewire      one of the --scenarios busiest links removed and a new link at its latency
                        between its tail and a random vertex
            random_add  a new link at the median latency between a random pair of vertices
  fresh : shd_route_create on the edited graph plus a lat-only rows call of the block, the median
          over 4 scenarios of the variant

Prints one JSON line per config: the medians of --reps timed calls after --warmup, per call and
per scenario, and the ratio of the fresh context to one scenario of every variant.
    python tools/edit_bench.py [--configs c4,c3] [--sources 1024] [--scenarios 256] [--reps 5]
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


def edited(g, rec):
    """g under one scenario's records (edge, a, b, lat): removed edges out, new links appended."""
    keep = np.ones(len(g.src), bool)
    lat = np.array(g.latency, np.float64)
    new = [(a, b, w) for e, a, b, w in rec if e < 0]
    for e, _, _, w in rec:
        if e >= 0 and np.isinf(w):
            keep[e] = False
        elif e >= 0:
            lat[e] = w
    cat = lambda old, col, t: np.concatenate([np.asarray(old)[keep], np.array([r[col] for r in new], t)]).astype(t)
    return dataclasses.replace(g, src=cat(g.src, 0, np.int32), dst=cat(g.dst, 1, np.int32), latency=cat(lat, 2, np.float64),
                               packetloss=np.concatenate([np.asarray(g.packetloss, np.float64)[keep], np.zeros(len(new))]))


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
        transit = torch.zeros(g.n, dtype=torch.int64, device=dev)
        eng.loads_async(src, tgt, None, load, transit, None, dispatch=False)
        sync()
        nscn = min(a.scenarios, m)
        gsrc, gdst = np.asarray(g.src), np.asarray(g.dst)
        glat = np.asarray(g.latency, np.float64)
        med = float(np.median(glat[gsrc != gdst]))
        rng = np.random.default_rng(g.n)
        hubs = np.argsort(-transit.cpu().numpy(), kind="stable")[:64]
        busy = [int(e) for e in np.argsort(-load.cpu().numpy(), kind="stable") if gsrc[e] != gdst[e]][:nscn]

        def pair(pool):
            while True:
                u, v = (int(x) for x in rng.choice(pool, size=2, replace=False))
                if u != v:
                    return u, v

        def other(u):
            while True:
                v = int(rng.integers(0, g.n))
                if v != u:
                    return v
        variants = {
            "add": [[(-1, *pair(hubs), med)] for _ in range(nscn)],
            "rewire": [[(-1, int(gsrc[e]), other(int(gsrc[e])), float(glat[e])), (e, 0, 0, float("inf"))] for e in busy],
            "random_add": [[(-1, *pair(g.n), med)] for _ in range(nscn)],
        }
        res, fresh = {}, {}
        lat = torch.empty((ns, g.n), dtype=torch.float64, device=dev)
        for label, scn in variants.items():
            k = len(scn)
            rec = [r for f in scn for r in f]
            off = torch.from_numpy(np.cumsum([0] + [len(f) for f in scn]).astype(np.int64)).to(dev)
            col = lambda i, t: torch.from_numpy(np.array([r[i] for r in rec], t)).to(dev)
            edge, ea, eb, nl = col(0, np.int32), col(1, np.int32), col(2, np.int32), col(3, np.float64)
            stats = torch.zeros((k, route.EDIT_NSTAT), dtype=torch.int64, device=dev)
            mx, mg, mn = (torch.zeros(k, dtype=torch.float64, device=dev) for _ in range(3))
            t = timed(lambda: eng.edit_async(src, tgt, None, off, edge, ea, eb, nl, stats, mx, mg, mn, None, None), sync,
                      a.warmup, a.reps)
            st = stats.cpu().numpy()
            res[label] = {"ms": round(1e3 * t[0], 3), "ms_per_scenario": round(1e3 * t[0] / k, 4),
                          "hit_share": round(float(st[:, route.EDIT_HIT].sum()) / (k * ns * g.n), 6),
                          "cut": int(st[:, route.EDIT_CUT].sum()), "slower": int(st[:, route.EDIT_SLOWER].sum()),
                          "faster": int(st[:, route.EDIT_FASTER].sum()), "max_add": float(mx.max().item()),
                          "max_gain": float(mg.max().item()), "min_new": float(mn.min().item())}
            # today: a context of the edited graph and its rows, per scenario
            took = []
            for f in scn[:4]:
                gk = edited(g, f)
                t0 = time.perf_counter()
                try:
                    ek = route.RouteEngine(gk)
                except Exception:  # the removal disconnects the graph: no context takes it
                    continue
                ek.rows_async(src, tgt, lat, None, None, dispatch=False)
                sync(ek)
                took.append(time.perf_counter() - t0)
                ek.close()
            fresh[label] = round(1e3 * statistics.median(took), 3) if took else None
        print(json.dumps({"what": "edit_vs_fresh_context", "diagnostic": True, "config": name, "n": g.n, "edges": m,
                          "sources": ns, "scenarios": nscn, "kernel": eng.info["kernel"], **res,
                          "fresh_context_ms": fresh,
                          "fresh_over_scenario": {k: round(fresh[k] / v["ms_per_scenario"], 1) if fresh[k] else None
                                                  for k, v in res.items()},
                          "build": bid}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
