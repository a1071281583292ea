"""Deterministic multigraphs (info.multigraph, SURVEY hazard H3: parallel edges, several
self-loops on one vertex) for test_multi_gpu.py.  include/shd_route.h promises on them: latency
is the true shortest distance, the parent of a hop is the tight in-arc with the smallest
(dist[u], u, edge id), a direct path goes over the lowest edge id joining the pair, the diagonal
takes the lowest self-loop.  tests/multi_ref.py is the reference of those rules, and
test_multi_graphs.py asserts, without the engine, that the inputs below let them decide numbers:

  multi389         internet_like(389, 3, seed 33) without vertex loss, the self-loops of every third
                   vertex removed, a second self-loop (another latency and loss) on a share of the
                   others, and half of the non-loop edges doubled: a third of the doubles with
                   the latency of their twin, a third lighter, a third heavier, each with a loss
                   of its own and a random orientation; at most 254 distinct reliabilities
  multi389_dir     directed: every base edge as two arcs, half of the arcs doubled a -> b, a -> b
  multi389_frac    multi389 with two-decimal latencies k / 100: the doubles have the k of their
                   twin, or a k one off it (a near miss inside a key interval), or another one
  multi389_vloss   multi389 with vertex packet loss on half of the vertices
  multi389_manyrel multi389 with a loss of its own on every edge (KF gives up above 254)
  loops_only       a simple graph in which a few vertices carry two self-loops
  multi8000        internet_like(8000, 3) doubled the same way (the generic kernel's HBM state)
  multi_k24        the complete graph k24 of tests/golden/small_tables.npz plus parallel edges:
                   lighter, heavier and equal ones
  count_complete   12 vertices, each joined twice to its three neighbours on either side of a
                   ring: 12 incident edges by count, yet most pairs are not adjacent

The doubles are appended after every base edge, so an added edge has the higher id of its pair.
Edge losses are k * 1e-4; BASE_M[name] is the number of base edges (ids below it are not added).
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np

from shadow_amd.graph import Graph, internet_like

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def base(n: int, seed: int, loops2: bool = True) -> Graph:
    """internet_like(n, 3, seed) without vertex loss and without the self-loops of the vertices
    v % 3 == 1; with loops2 a second self-loop, after the base edges, on the vertices v % 6 == 0:
    one ms cheaper than the first where that is above 1 ms, 4 ms dearer otherwise, with another
    loss."""
    g = internet_like(n, 3, seed=seed, name=f"ba{n}")
    keep = (g.src != g.dst) | (g.src % 3 != 1)
    src, dst, lat, loss = g.src[keep], g.dst[keep], g.latency[keep], g.packetloss[keep]
    if loops2:
        first = np.flatnonzero((src == dst) & (src % 6 == 0))
        v = src[first]
        l2 = np.where(lat[first] > 1.0, lat[first] - 1.0, lat[first] + 4.0)
        p2 = ((np.rint(loss[first] * 1e4).astype(np.int64) + 7 + v % 5) % 101) * 1e-4
        src, dst = np.concatenate([src, v]), np.concatenate([dst, v])
        lat, loss = np.concatenate([lat, l2]), np.concatenate([loss, p2])
    return dataclasses.replace(g, src=src.astype(np.int32), dst=dst.astype(np.int32), latency=lat,
                               packetloss=loss, vertex_packetloss=None)


def doubled(g: Graph, seed: int, name: str, flip: bool = True, frac: bool = False) -> Graph:
    """g plus a parallel edge for a random half of its non-loop edges, appended in random order:
    double i has its twin's latency (i % 3 == 0), a lighter one (1) or a heavier one (2), a
    loss k * 1e-4 (k in 1..120) other than its twin's, and with `flip` a random orientation.
    frac: every latency becomes k / 100 with k = 100 latency + U{0..99}; an equal double keeps
    its twin's k, a lighter one is k - 1 and a heavier one k + 1 for half of them (the others as
    before: whole milliseconds away)."""
    rng = np.random.default_rng(seed)
    nl = np.flatnonzero(g.src != g.dst)
    pick = rng.permutation(nl)[: len(nl) // 2]
    k = np.rint(g.latency * 100.0).astype(np.int64) + (rng.integers(0, 100, size=g.m) if frac else 0)
    kind = np.arange(len(pick)) % 3
    step = rng.integers(1, 4, size=len(pick)) * 100
    if frac:
        step = np.where(rng.random(len(pick)) < 0.5, 1, step)
    k2 = k[pick] + np.where(kind == 0, 0, np.where(kind == 1, -step, step))
    k2 = np.where(k2 < (1 if frac else 100), k[pick], k2)
    p = np.rint(g.packetloss[pick] * 1e4).astype(np.int64)
    p2 = rng.integers(1, 121, size=len(pick))
    p2 = np.where(p2 == p, p2 % 120 + 1, p2)
    a, b = g.src[pick], g.dst[pick]
    if flip:
        sw = rng.random(len(pick)) < 0.5
        a, b = np.where(sw, b, a), np.where(sw, a, b)
    return dataclasses.replace(
        g, src=np.concatenate([g.src, a]).astype(np.int32), dst=np.concatenate([g.dst, b]).astype(np.int32),
        latency=np.concatenate([k, k2]).astype(np.float64) / 100.0,
        packetloss=np.concatenate([g.packetloss, p2 * 1e-4]), name=name)


def directed_base(n: int, seed: int) -> Graph:
    """base(n, seed) as a directed graph: every non-loop edge a - b becomes a -> b (its own
    attributes) and b -> a (latency and loss drawn anew), the self-loops stay."""
    g = base(n, seed)
    rng = np.random.default_rng(seed + 1000)
    nl = g.src != g.dst
    a, b = g.src[nl], g.dst[nl]
    k = len(a)
    lat = rng.integers(1, 251, size=k).astype(np.float64)
    loss = np.where(rng.random(k) >= 0.8, rng.integers(1, 101, size=k) * 1e-4, 0.0)
    return dataclasses.replace(
        g, src=np.concatenate([a, b, g.src[~nl]]), dst=np.concatenate([b, a, g.dst[~nl]]),
        latency=np.concatenate([g.latency[nl], lat, g.latency[~nl]]),
        packetloss=np.concatenate([g.packetloss[nl], loss, g.packetloss[~nl]]), directed=True)


def with_vloss(g: Graph, seed: int, name: str) -> Graph:
    """Vertex loss U{0..10} * 1e-4 on a random half of the vertices, absent (NaN) on the rest."""
    rng = np.random.default_rng(seed)
    vl = np.where(rng.random(g.n) < 0.5, rng.integers(0, 11, size=g.n) * 1e-4, np.nan)
    return dataclasses.replace(g, vertex_packetloss=vl, name=name)


def many_rel(g: Graph, name: str) -> Graph:
    """Edge e's loss becomes (e + 1) / 2**21: every edge its own reliability."""
    return dataclasses.replace(g, packetloss=(np.arange(g.m) + 1) / float(2 ** 21), name=name)


def loops_only() -> Graph:
    """base(150, 41): simple but for the second self-loops."""
    return dataclasses.replace(base(150, 41), name="loops_only")


def k24() -> Graph:
    z = np.load(os.path.join(GOLD, "small_tables.npz"))
    p = "k24__"
    vl = z[p + "vertex_packetloss"]
    return Graph(n=int(z[p + "n"]), src=z[p + "src"], dst=z[p + "dst"], latency=z[p + "latency"],
                 packetloss=z[p + "packetloss"], vertex_packetloss=vl if len(vl) else None,
                 directed=bool(z[p + "directed"]), prefer_direct=bool(z[p + "prefer_direct"]), name="k24")


def count_complete() -> Graph:
    """Vertex v of 12 joined to v + 1, v + 2 and v + 3 (mod 12), each pair by two edges of
    different latency and loss (the second, higher id is the lighter one for every other
    pair): 12 incident edges per vertex, which is the reference's test for a complete graph,
    and no edge between v and v + 4 .. v + 8.  Self-loops on the vertices v % 3 != 1, two of
    them on 0 and 6."""
    n = 12
    rng = np.random.default_rng(12)
    a = np.repeat(np.arange(n), 3)
    b = (a + np.tile([1, 2, 3], n)) % n
    k = len(a)
    lat = rng.integers(5, 60, size=k).astype(np.float64)
    lat2 = lat + np.where(np.arange(k) % 2 == 0, -3.0, 4.0)
    loss = rng.integers(0, 50, size=k) * 1e-4
    loss2 = rng.integers(50, 100, size=k) * 1e-4
    lv = np.array([v for v in range(n) if v % 3 != 1] + [0, 6])
    llat = rng.integers(2, 11, size=len(lv)).astype(np.float64)
    llat[-2], llat[-1] = llat[0] - 1.0, llat[list(lv).index(6)]   # 0: a cheaper second loop; 6: an equal one
    lloss = np.arange(1, len(lv) + 1) * 7e-4
    return Graph(n=n, src=np.concatenate([a, lv, b]).astype(np.int32), dst=np.concatenate([b, lv, a]).astype(np.int32),
                 latency=np.concatenate([lat, llat, lat2]), packetloss=np.concatenate([loss, lloss, loss2]),
                 vertex_packetloss=None, name="count_complete")


SUITE = {
    "multi389": lambda: doubled(base(389, 33), 389, "multi389"),
    "multi389_dir": lambda: doubled(directed_base(389, 33), 390, "multi389_dir", flip=False),
    "multi389_frac": lambda: doubled(base(389, 33), 391, "multi389_frac", frac=True),
    "multi389_vloss": lambda: with_vloss(get("multi389"), 392, "multi389_vloss"),
    "multi389_manyrel": lambda: many_rel(get("multi389"), "multi389_manyrel"),
    "loops_only": loops_only,
    "multi8000": lambda: doubled(base(8000, 35), 8000, "multi8000"),
    "multi_k24": lambda: doubled(k24(), 24, "multi_k24"),
    "count_complete": count_complete,
}

# base edges per graph: an edge id at or above it is an added parallel edge (or second loop)
BASE_M = {"multi389": lambda: base(389, 33).m, "multi389_dir": lambda: directed_base(389, 33).m,
          "multi389_frac": lambda: base(389, 33).m, "multi389_vloss": lambda: base(389, 33).m,
          "multi389_manyrel": lambda: base(389, 33).m, "multi8000": lambda: base(8000, 35).m,
          "multi_k24": lambda: k24().m}

# the fixtures with parallel arcs, and the 389-vertex ones every rows kernel runs on
PARALLEL = ("multi389", "multi389_dir", "multi389_frac", "multi389_vloss", "multi389_manyrel", "multi8000",
            "multi_k24")
ROWS389 = ("multi389", "multi389_dir", "multi389_frac", "multi389_vloss", "multi389_manyrel")

_cache: dict = {}


def get(name: str) -> Graph:
    """The suite's graph of that name (built once per process; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = SUITE[name]()
    return _cache[name]


def added_from(name: str) -> int:
    """The lowest edge id of the fixture's added parallel edges."""
    return BASE_M[name]()


def without_second_loops(g: Graph) -> Graph:
    """g with only the lowest-id self-loop of every vertex kept."""
    keep = np.ones(g.m, bool)
    seen = set()
    for e in np.flatnonzero(g.src == g.dst):
        v = int(g.src[e])
        keep[e] = v not in seen
        seen.add(v)
    return dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], latency=g.latency[keep],
                               packetloss=g.packetloss[keep], name=g.name + "_simple")


def sources(name: str) -> np.ndarray:
    """The sources the tests use: every vertex up to 400 vertices; of multi8000 five, vertex 0,
    the highest one, one with two self-loops, one with one and one without."""
    g = get(name)
    if g.n <= 400:
        return np.arange(g.n, dtype=np.int32)
    return np.array([0, g.n - 1, 3000, 3002, 3001], np.int32)
