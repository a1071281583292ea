"""The cases of tests/golden/select_info.json: a graph and a creation-time SHD_ROUTE_*
environment each.  shd_route_create decides from these alone which rows kernel a context
gets; the fixture holds what shd_route_get_info reported for each case when the selection
still lived inside engine.hip (tests/golden/make_select_info.py), test_select.py checks the
host-only selection against it without a GPU, and test_select_gpu.py the created context.

  every graph of shape_graphs.SUITE and range_graphs.SUITE with a clean environment
  frac1024 / frac5000 / frac20000   two-decimal latencies: KF with 256 threads, KF with 1024,
                                    KFH (the per-vertex state in HBM)
  lat75k                            integer latencies up to 75000 (no u16 kernel takes them)
  the multigraphs of multi_graphs.SUITE (all but multi_k24) with a clean environment: no integer
                                    kernel takes parallel edges or a second self-loop
  the overrides below, each on the graphs whose decision it can move
"""
from __future__ import annotations

import dataclasses

from shadow_amd.graph import Graph, fractional

from . import multi_graphs, range_graphs, shape_graphs

# what the fixture records of Engine.info
FIELDS = ("kernel", "block", "reserved", "dist_bound", "lat16", "lds_resident", "device_bytes",
          "integer_weights", "multigraph", "is_complete", "n_arcs", "min_edge_latency")


def _lat75k() -> Graph:
    g = shape_graphs.sized(257)
    return dataclasses.replace(g, latency=g.latency * 300.0, name="lat75k")


EXTRA = {
    "frac1024": lambda: fractional(shape_graphs.sized(1024), 3, name="frac1024"),
    "frac5000": lambda: fractional(shape_graphs.sized(5000), 4, name="frac5000"),
    "frac20000": lambda: fractional(shape_graphs.sized(20000), 5, name="frac20000"),
    "lat75k": _lat75k,
}

MULTI = ("multi389", "multi389_dir", "multi389_frac", "multi389_vloss", "multi389_manyrel", "loops_only",
         "multi8000", "count_complete")

_cache: dict = {}


def graph(name: str) -> Graph:
    if name in shape_graphs.SUITE:
        return shape_graphs.get(name)
    if name in range_graphs.SUITE:
        return range_graphs.get(name)
    if name in MULTI:
        return multi_graphs.get(name)
    if name not in _cache:
        _cache[name] = EXTRA[name]()
    return _cache[name]


def _cases():
    """name -> (graph name, environment)."""
    c = {}
    for g in (*shape_graphs.SUITE, *range_graphs.SUITE, *EXTRA):
        c[g] = (g, {})

    def add(g, **env):
        env = {f"SHD_ROUTE_{k}": str(v) for k, v in env.items()}
        c[g + ":" + ",".join(f"{k[10:]}={v}" for k, v in env.items())] = (g, env)

    for g in ("sized2048", "sized4097", "dir_grid", "tiny7_some"):
        for k in ("kd", "kb", "k32", "kf", "f64", "auto", ""):
            add(g, KERNEL=k)
    for g, blk in (("sized2048", 1024), ("sized16385", 256)):
        add(g, KDBLOCK=blk)
    for g in ("sized2048", "sized16385"):
        add(g, DELTA=7)
        add(g, QCAP=64)
        add(g, KDPACK=0)
        add(g, HUB1024=0)
        add(g, KDWALK=0)
        add(g, KDGRID=7)
    add("sized1024", KBFUSE=0)
    add("sized1024", KBTCAP=64)
    add("sized1024", KBGRID=3)
    for g in ("frac1024", "dec100"):
        add(g, KFH=1)
        add(g, KFPK=0)
        add(g, KFH=1, KFPK=0)
        add(g, KFDELTA=2.5)
    add("frac20000", KFPK=0)
    add("frac1024", KERNEL="kf")
    add("frac1024", KERNEL="f64")
    add("frac1024", KERNEL="kd")
    for g in MULTI:
        c[g] = (g, {})
    for g in ("multi389", "multi389_frac"):
        add(g, KERNEL="kd")
        add(g, KERNEL="kf")
        add(g, KFH=1)
        add(g, KFH=1, KFPK=0)
    return c


CASES = _cases()


def graph_text(g: Graph) -> str:
    """The topology as tests/select_main.cpp reads it: `n m directed`, one `src dst latency
    loss` line per edge, then the n vertex losses (nan: absent).  repr() of a double parses
    back to the same double."""
    lines = [f"{g.n} {g.m} {int(bool(g.directed))}"]
    lines += [f"{int(a)} {int(b)} {float(w)!r} {float(p)!r}"
              for a, b, w, p in zip(g.src, g.dst, g.latency, g.packetloss)]
    vl = g.vertex_packetloss
    lines.append(" ".join("nan" if vl is None else repr(float(x)) for x in (range(g.n) if vl is None else vl)))
    return "\n".join(lines) + "\n"
