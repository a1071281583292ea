#!/usr/bin/env python3
"""What the link loss costs next to the link loads it shares its trees with ("Link
loss").  A diagnostic rate: it has no target and no test gates it.

  loss   : shd_route_loss_async, 1,024 sources x all vertices, unit weights, all five outputs
  loads  : shd_route_loads_async, the same sources and outputs of the same run

Prints one JSON line per config: the median of --reps timed calls after --warmup and the ratio
to the loads call.
    python tools/loss_bench.py [--configs c4,c3] [--sources 1024] [--reps 5]
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
    for name in [c for c in a.configs.split(",") if c]:
        g = config(name)
        eng = route.RouteEngine(g)
        ns, m = min(a.sources, g.n), eng.info["n_edges"]
        src = torch.from_numpy(np.linspace(0, g.n - 1, ns).astype(np.int32)).to(dev)
        tgt = torch.arange(g.n, dtype=torch.int32, device=dev)
        f = [torch.empty(k, dtype=torch.float64, device=dev) for k in (m, m, g.n, g.n)]
        u = [torch.empty(k, dtype=torch.int64, device=dev) for k in (m, g.n, 1, 1)]

        def sync():  # a source without a self-loop fails its own entry: not an error here
            try:
                eng.sync()
            except route.RouteError as err:
                if err.code not in (route.ENOEDGE, route.EUNREACH):
                    raise

        t_loads = timed(lambda: eng.loads_async(src, tgt, None, u[0], u[1], u[2], dispatch=False), sync, a.warmup,
                        a.reps)
        t_loss = timed(lambda: eng.loss_async(src, tgt, None, f[0], f[1], f[2], f[3], u[3], dispatch=False), sync,
                       a.warmup, a.reps)
        sent = ns * g.n - int(u[3].item())
        print(json.dumps({"what": "loss_vs_loads", "diagnostic": True, "config": name, "n": g.n, "edges": m,
                          "sources": ns, "kernel": eng.info["kernel"], "state": "lds" if g.n <= 7442 else "hbm",
                          "loads_ms": round(1e3 * t_loads[0], 3), "loss_ms": round(1e3 * t_loss[0], 3),
                          "loss_over_loads": round(t_loss[0] / t_loads[0], 3),
                          "delivered_share": round(float(f[3].sum().item()) / max(sent, 1), 6),
                          "dropped_share": round(float((f[1].sum() + f[2].sum()).item()) / max(sent, 1), 6),
                          "build": bid}), flush=True)
        eng.close()
        del f, u


if __name__ == "__main__":
    main()
