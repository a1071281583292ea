"""Deterministic topologies with fractional latencies whose shortest paths tie, or miss a tie by
an ulp, in f64: for test_frac_paths_gpu.py.  The path calls (hops, loads, ties, ECMP loads,
folds) take an arc u -> v as being on a shortest path exactly when d[u] + w == d[v] in double;
with latencies such as 0.1, 0.2 and 0.3 that is a statement about rounding (0.1 + 0.2 is not the
double 0.3), and only inputs like these tell a kernel that compares with a tolerance, sums in
another order or reads a latency through another conversion from one that follows the rule.
test_frac_graphs.py asserts the properties the builders are named for with the Python
references alone, without the engine.

Every latency is k / scale for an integer k (scale 10, 100 or 1000): the one correctly rounded
division, the double its decimal text parses to.  Every vertex has a self-loop.  All losses are
k / 2**21 with k below 200: 1 - loss is exact, distinct per k, and few enough for KF and KFH.

  frac_grid        side x side lattice, latencies drawn from `vals`
  frac_grid_cents  the same lattice with seven two-decimal values (KFH packs it at scale 100)
  frac_grid_dir    the lattice as a directed graph: both arcs of an edge with latencies of
                   their own, so the in-CSR and the out-CSR weights of a pair differ
  frac_cents       BA(n, 3), latencies k / 100 from seven values, vertex loss on a fifth of the
                   vertices (absent on the others)
  frac_hub         K(6, 140) and a ring through all 146 vertices (its hub-to-leaf steps are
                   biclique edges), latencies from {0.1, 0.2, 0.3}: in-lists of 141 arcs
  frac_multi       frac_grid plus 30 parallel edges: 15 with their twin's latency and a loss of
                   their own, 15 one tenth above or below their twin
  frac_thousandths BA(n, 3), latencies k / 1000 with k in U[500, 90000): many distinct doubles,
                   next to no ties (the control)
"""
from __future__ import annotations

import numpy as np

from shadow_amd.graph import Graph, barabasi_albert_edges

_LOSS_DEN = float(2 ** 21)
NLOSS = 200
TENTHS = (0.1, 0.2, 0.3, 0.7)
CENTS = (5, 10, 15, 20, 30, 45, 70)


def _losses(rng, k):
    return rng.integers(0, NLOSS, size=k) / _LOSS_DEN


def _ks(vals, scale):
    """The integers k of the decimals vals = k / scale, each checked to be that double."""
    k = np.rint(np.asarray(vals, np.float64) * scale).astype(np.int64)
    assert np.array_equal(k / float(scale), np.asarray(vals, np.float64)) and k.min() >= 1
    return k


def _graph(n, src, dst, k, scale, loss, rng, name, **kw) -> Graph:
    """The edges (latency k / scale) plus a self-loop on every vertex, latency drawn from k."""
    lv = np.arange(n, dtype=np.int32)
    lk = rng.choice(np.unique(k), size=n)
    return Graph(n=n, src=np.concatenate([src, lv]).astype(np.int32), dst=np.concatenate([dst, lv]).astype(np.int32),
                 latency=np.concatenate([k, lk]).astype(np.float64) / float(scale),
                 packetloss=np.concatenate([loss, _losses(rng, n)]), name=name, **kw)


def _grid_edges(side):
    v = np.arange(side * side, dtype=np.int32).reshape(side, side)
    return (np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()]),
            np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()]))


def frac_grid(side: int = 14, vals=TENTHS, scale: int = 10, seed: int = 14, name: str = "frac_grid") -> Graph:
    """The undirected side x side lattice (vertex i side + j), latencies drawn from vals."""
    rng = np.random.default_rng(seed)
    src, dst = _grid_edges(side)
    k = rng.choice(_ks(vals, scale), size=len(src))
    return _graph(side * side, src, dst, k, scale, _losses(rng, len(src)), rng, name)


def frac_grid_cents(side: int = 14, seed: int = 15) -> Graph:
    return frac_grid(side, np.array(CENTS) / 100.0, 100, seed, "frac_grid_cents")


def frac_grid_dir(side: int = 14, vals=TENTHS, scale: int = 10, seed: int = 16) -> Graph:
    """Both arcs of every lattice edge, each with a latency and a loss of its own."""
    rng = np.random.default_rng(seed)
    a, b = _grid_edges(side)
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    k = rng.choice(_ks(vals, scale), size=len(src))
    return _graph(side * side, src, dst, k, scale, _losses(rng, len(src)), rng, "frac_grid_dir", directed=True)


def frac_cents(n: int = 300, seed: int = 17) -> Graph:
    """BA(n, 3) with latencies k / 100, k from CENTS; vertex loss U{1..10} * 1e-4 on about a
    fifth of the vertices, the attribute absent (NaN) on the others."""
    rng = np.random.default_rng(seed)
    e = barabasi_albert_edges(n, 3, rng)
    k = rng.choice(np.array(CENTS), size=len(e))
    vl = np.where(rng.random(n) < 0.2, rng.integers(1, 11, size=n) * 1e-4, np.nan)
    return _graph(n, e[:, 0], e[:, 1], k, 100, _losses(rng, len(e)), rng, f"frac_cents{n}", vertex_packetloss=vl)


def frac_hub(a: int = 6, b: int = 140, seed: int = 18) -> Graph:
    """K(a, b), the hubs 0 .. a - 1 against the leaves a .. a + b - 1, and the ring 0 - 1 - ... -
    (a + b - 1) - 0, whose steps a - 1 to a and a + b - 1 to 0 are biclique edges already (the
    graph stays simple).  Latencies from {0.1, 0.2, 0.3}."""
    rng = np.random.default_rng(seed)
    n = a + b
    hub, leaf = np.arange(a - 1, dtype=np.int32), np.arange(a, n - 1, dtype=np.int32)
    src = np.concatenate([np.repeat(np.arange(a, dtype=np.int32), b), hub, leaf])
    dst = np.concatenate([np.tile(np.arange(a, n, dtype=np.int32), a), hub + 1, leaf + 1])
    k = rng.integers(1, 4, size=len(src))
    return _graph(n, src, dst, k, 10, _losses(rng, len(src)), rng, f"frac_hub{a}_{b}")


N_PARALLEL = 30


def frac_multi(side: int = 14, seed: int = 19) -> Graph:
    """frac_grid(side) plus N_PARALLEL parallel edges in the opposite orientation: the first half
    with the latency of the edge they double and a loss of their own (two tight arcs from one
    tail whenever one is tight), the second half one tenth above or below it (never tight
    together with it)."""
    g = frac_grid(side, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    pick = rng.choice(np.flatnonzero(g.src != g.dst), size=N_PARALLEL, replace=False)
    k = np.rint(g.latency[pick] * 10.0).astype(np.int64)
    step = np.where(k > 1, rng.choice([-1, 1], size=N_PARALLEL), 1)
    step[: N_PARALLEL // 2] = 0
    loss = (g.packetloss[pick] * _LOSS_DEN + 1 + rng.integers(0, 50, size=N_PARALLEL)) % NLOSS / _LOSS_DEN
    return Graph(n=g.n, src=np.concatenate([g.src, g.dst[pick]]).astype(np.int32),
                 dst=np.concatenate([g.dst, g.src[pick]]).astype(np.int32),
                 latency=np.concatenate([g.latency, (k + step) / 10.0]),
                 packetloss=np.concatenate([g.packetloss, loss]), name="frac_multi")


def frac_thousandths(n: int = 300, seed: int = 20) -> Graph:
    rng = np.random.default_rng(seed)
    e = barabasi_albert_edges(n, 3, rng)
    k = rng.integers(500, 90000, size=len(e))
    return _graph(n, e[:, 0], e[:, 1], k, 1000, _losses(rng, len(e)), rng, f"frac_thousandths{n}")


SUITE = {
    "frac_grid": frac_grid,
    "frac_grid_cents": frac_grid_cents,
    "frac_grid_dir": frac_grid_dir,
    "frac_cents": frac_cents,
    "frac_hub": frac_hub,
    "frac_multi": frac_multi,
    "frac_thousandths": frac_thousandths,
}
TIED = tuple(k for k in SUITE if k != "frac_thousandths")
SCALE = {"frac_grid": 10, "frac_grid_cents": 100, "frac_grid_dir": 10, "frac_cents": 100, "frac_hub": 10,
         "frac_multi": 10, "frac_thousandths": 1000}

_cache: dict = {}


def get(name: str) -> Graph:
    """The suite's graph of that name (built once per process; treat it as read-only)."""
    if name not in _cache:
        g = SUITE[name]()
        for a in (g.src, g.dst, g.latency, g.packetloss):
            a.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def sources(name: str, k: int = 24) -> np.ndarray:
    """About k sources spread over the graph, the first and the last vertex among them."""
    n = get(name).n
    return np.unique(np.linspace(0, n - 1, k).astype(np.int32))


def absorbs(g: Graph) -> bool:
    """shd_route_create's refusal, from the arrays: over the edges that are no self-loops, the
    smallest latency is at most (n - 1) * the largest * 2^-52, so that some d[u] + w might round
    to d[u]."""
    nl = g.src != g.dst
    if not nl.any():
        return False
    w = np.asarray(g.latency, np.float64)[nl]
    return bool(w.min() <= (g.n - 1) * (w.max() * 2.0 ** -52))
