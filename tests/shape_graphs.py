"""Deterministic topologies on the shape axis, for test_shape_gpu.py: vertex counts on both
sides of every size limit of shadow_amd/csrc, degrees on both sides of every degree limit,
tie-dominated graphs, deep trees and graphs of fewer than ten vertices.  The value axis stays
narrow on purpose (tests/range_graphs.py covers it): integer latencies below 256 and at most
200 distinct losses k / 2**21, so that the packed / fused / seeded encodings stay eligible and
only the shape varies.  Self-loops sit on the vertices v with v % 3 != 1 unless stated
otherwise; every graph is strongly connected.  test_shape_graphs.py asserts the properties the
builders are named for with a plain Dijkstra, without the engine.

  tiny       a path of 1, 2, 3, 7, 8 or 9 vertices (self-loops on all, none or some); one
             vertex without a self-loop has no edge at all
  sized      internet_like(n, 3, seed=n): the vertex count alone selects the code path
  star       one vertex adjacent to all others: an in-row of n - 1 arcs, one expansion that
             improves n - 1 vertices; every other vertex has degree 1 or 2
  biclique   K_{a,b}, latencies in {3, 4}: a + b vertices of more than 16 in-arcs, depth 2,
             many equal-cost paths for every pair
  bireg      a d-regular bipartite circulant, latencies in {3, 4}: 2 p vertices of exactly d
             in-arcs each with only d p edges (K_{17,b} needs 17 b), the hub count that the
             batched kernel's LDS still holds
  grid       r x c lattice, every latency 2: 63 hops corner to corner at 32 x 33, equal-cost
             paths almost everywhere (grid_vloss: with vertex loss; dir_grid: directed, both
             arcs of every edge with attributes of their own)
  lollipop   K_k (k above the whole-wave scan widths) joined to a long path
"""
from __future__ import annotations

import dataclasses

import numpy as np

from shadow_amd.graph import Graph, internet_like

_LOSS_DEN = float(2 ** 21)
NLOSS = 200

TINY_N = (1, 2, 3, 7, 8, 9)
TINY_LOOPS = ("all", "none", "some")
SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2688, 2689, 4096, 4097,
         11212, 11213, 16384, 16385)


def _losses(rng, k):
    return rng.integers(0, NLOSS, size=k) / _LOSS_DEN


def _with_loops(n, src, dst, lat, loss, lv, **kw) -> Graph:
    """The edges plus a self-loop (latency 1 + v % 9, loss (v % 4) / 2**21) on the vertices lv."""
    lv = np.asarray(lv, np.int32)
    return Graph(n=n, src=np.concatenate([src, lv]).astype(np.int32), dst=np.concatenate([dst, lv]).astype(np.int32),
                 latency=np.concatenate([lat, 1.0 + (lv % 9)]).astype(np.float64),
                 packetloss=np.concatenate([loss, (lv % 4) / _LOSS_DEN]).astype(np.float64), **kw)


def _some(n):
    return np.flatnonzero(np.arange(n) % 3 != 1)


def tiny(n: int, loops: str = "some") -> Graph:
    """The path 0 - 1 - ... - (n - 1), latencies 1 + i % 5; self-loops on every vertex ("all"),
    on none ("none") or on the vertices v % 3 != 1 ("some").  tiny(1, "none") has no edge."""
    a = np.arange(n - 1, dtype=np.int32)
    lv = {"all": np.arange(n), "none": np.arange(0), "some": _some(n)}[loops]
    return _with_loops(n, a, a + 1, 1.0 + (a % 5), (a % 6) / _LOSS_DEN, lv, name=f"tiny{n}_{loops}")


def sized(n: int) -> Graph:
    """internet_like(n, 3, seed=n) (BA(n, 3), latencies U[1, 250], about 100 distinct losses)
    without the self-loops of the vertices v % 3 == 1 and without its all-zero vertex loss."""
    g = internet_like(n, 3, seed=n, name=f"sized{n}")
    keep = (g.src != g.dst) | (g.src % 3 != 1)
    return dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], latency=g.latency[keep],
                               packetloss=g.packetloss[keep], vertex_packetloss=None)


def star(n: int) -> Graph:
    """Vertex 0 adjacent to every other vertex (latencies U[1, 5]); the leaves 4 k + 1 and
    4 k + 2 are joined by an edge of latency 5, which no path between other vertices takes."""
    rng = np.random.default_rng(n)
    leaf = np.arange(1, n, dtype=np.int32)
    a = np.arange(1, n - 1, 4, dtype=np.int32)
    src = np.concatenate([np.zeros(n - 1, np.int32), a])
    dst = np.concatenate([leaf, a + 1])
    lat = np.concatenate([rng.integers(1, 6, size=n - 1), np.full(len(a), 5)]).astype(np.float64)
    return _with_loops(n, src, dst, lat, _losses(rng, len(src)), _some(n), name=f"star{n}")


def biclique(a: int, b: int) -> Graph:
    """K_{a,b}: the vertices 0 .. a - 1 against a .. a + b - 1, latencies U{3, 4}."""
    rng = np.random.default_rng(1000 * a + b)
    src = np.repeat(np.arange(a, dtype=np.int32), b)
    dst = np.tile(np.arange(a, a + b, dtype=np.int32), a)
    lat = rng.integers(3, 5, size=a * b).astype(np.float64)
    return _with_loops(a + b, src, dst, lat, _losses(rng, a * b), _some(a + b), name=f"biclique{a}_{b}")


def bireg(p: int, d: int = 17) -> Graph:
    """Left vertex i (0 <= i < p) adjacent to the right vertices p + (i + k) % p, 0 <= k < d:
    every one of the 2 p vertices has exactly d in-arcs.  Latencies U{3, 4}."""
    rng = np.random.default_rng(100 * p + d)
    i = np.repeat(np.arange(p, dtype=np.int32), d)
    k = np.tile(np.arange(d, dtype=np.int32), p)
    lat = rng.integers(3, 5, size=p * d).astype(np.float64)
    return _with_loops(2 * p, i, p + (i + k) % p, lat, _losses(rng, p * d), _some(2 * p), name=f"bireg{p}_{d}")


def _grid_edges(r, c):
    v = np.arange(r * c, dtype=np.int32).reshape(r, c)
    src = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    dst = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    return src, dst


def grid(r: int, c: int, vloss: bool = False) -> Graph:
    """The r x c lattice (vertex i c + j), every edge latency 2, random losses; vloss: vertex
    loss U{0..10} * 1e-4."""
    rng = np.random.default_rng(100 * r + c)
    src, dst = _grid_edges(r, c)
    vl = rng.integers(0, 11, size=r * c) * 1e-4 if vloss else None
    return _with_loops(r * c, src, dst, np.full(len(src), 2.0), _losses(rng, len(src)), _some(r * c),
                       vertex_packetloss=vl, name=f"grid{r}x{c}" + ("_vloss" if vloss else ""))


def dir_grid(r: int = 16, c: int = 16) -> Graph:
    """The r x c lattice as a directed graph: both arcs of every edge, each with a latency
    (2, or 3 for one arc in eight) and a loss of its own."""
    rng = np.random.default_rng(7 * r + c)
    a, b = _grid_edges(r, c)
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    lat = np.where(rng.random(len(src)) < 0.125, 3.0, 2.0)
    return _with_loops(r * c, src, dst, lat, _losses(rng, len(src)), _some(r * c), directed=True,
                       name=f"dirgrid{r}x{c}")


def lollipop(k: int = 40, tail: int = 300) -> Graph:
    """K_k on the vertices 0 .. k - 1, then the path k - 1, k, ..., k + tail - 1; latencies
    U[1, 3] throughout."""
    rng = np.random.default_rng(1000 * k + tail)
    iu, ju = np.triu_indices(k, 1)
    p = np.arange(k - 1, k + tail - 1, dtype=np.int32)
    src, dst = np.concatenate([iu, p]), np.concatenate([ju, p + 1])
    lat = rng.integers(1, 4, size=len(src)).astype(np.float64)
    return _with_loops(k + tail, src, dst, lat, _losses(rng, len(src)), _some(k + tail), name=f"lollipop{k}_{tail}")


# K_{17,b}: 17 + b vertices of more than 16 in-arcs (the b side has 17 each)
BICLIQUES = ("biclique1000", "biclique1030")
# 17-regular: 1024 and 1026 such vertices, with half the arcs of K_{17,b}
BIREGS = ("bireg512", "bireg513")

SUITE = {
    "star300": lambda: star(300),
    "star1100": lambda: star(1100),
    "biclique1000": lambda: biclique(17, 1000),
    "biclique1030": lambda: biclique(17, 1030),
    "bireg512": lambda: bireg(512),
    "bireg513": lambda: bireg(513),
    "grid": lambda: grid(32, 33),
    "grid_vloss": lambda: grid(32, 33, vloss=True),
    "lollipop": lambda: lollipop(40, 300),
    "dir_grid": lambda: dir_grid(16, 16),
}
SUITE.update({f"sized{n}": (lambda n=n: sized(n)) for n in SIZES})
SUITE.update({f"tiny{n}_{lp}": (lambda n=n, lp=lp: tiny(n, lp)) for n in TINY_N for lp in TINY_LOOPS})

_cache: dict = {}


def get(name: str) -> Graph:
    """The suite's graph of that name (built once per process; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = SUITE[name]()
    return _cache[name]
