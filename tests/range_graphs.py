"""Deterministic topologies outside the narrow distribution of shadow_amd.graph's generators
(integer latencies 1..250, a self-loop on every vertex, ~100 distinct losses), for
test_range_gpu.py and test_contract_gpu.py.  Each builder is named for the property of its
input that a kernel's compact encoding depends on; test_range_graphs.py asserts those
properties with a plain Dijkstra, without the engine:

  wide       latencies up to 65534 ms, shortest paths past 32768 ms (the sign bit of a u16
             distance), tentative sums past 65535, > 1000 distinct reliabilities, self-loops
             (latency up to 60000 ms) on a share of the vertices only
  long_path  latencies below 256 and few reliabilities (the narrow encodings), distances up
             to 0xFFFE
  dumbbell   bound = ecc_out(0) + ecc_in(0) = the largest distance = `total` exactly
  many_rel   more distinct reliabilities than a u16 (or u8) table index holds
  decimal    latencies k / scale with k up to 65535 (KFH's packed arcs), or one arc past it
  front_pair the front end's compact-triangle rule, 2 * max edge latency < 0xFFFF, alone

All losses are k / 2**21: 1 - loss is then exact and distinct per k.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from shadow_amd.graph import Graph, barabasi_albert_edges, internet_like

_LOSS_DEN = float(2 ** 21)


def wide(n: int, seed: int, scale: int, loops: float = 0.66, directed: bool = False,
         vloss: bool = False, nloss: int = 2 ** 20) -> Graph:
    """BA(n, 3); integer latencies U[2 scale, 40 scale), about 10% of the edges redrawn from
    U[30000, 65535); loss k / 2**21, k in U[0, nloss); a self-loop (latency U[1, 60000)) on a
    random `loops` share of the vertices; vertex loss absent, or U{0..10} * 1e-4 with vloss.
    directed: every BA edge becomes two arcs, one each way, with their own attributes."""
    rng = np.random.default_rng(seed)
    e = barabasi_albert_edges(n, 3, rng)
    if directed:
        e = np.concatenate([e, e[:, ::-1]])
    k = len(e)
    lat = rng.integers(2 * scale, 40 * scale, size=k)
    heavy = rng.random(k) < 0.10
    lat = np.where(heavy, rng.integers(30000, 65535, size=k), lat).astype(np.float64)
    loss = rng.integers(0, nloss, size=k) / _LOSS_DEN
    lv = np.flatnonzero(rng.random(n) < loops).astype(np.int32)
    llat = rng.integers(1, 60000, size=len(lv)).astype(np.float64)
    lloss = rng.integers(0, 2 ** 20, size=len(lv)) / _LOSS_DEN
    vl = (rng.integers(0, 11, size=n) * 1e-4) if vloss else None
    return Graph(n=n, src=np.concatenate([e[:, 0], lv]).astype(np.int32),
                 dst=np.concatenate([e[:, 1], lv]).astype(np.int32),
                 latency=np.concatenate([lat, llat]), packetloss=np.concatenate([loss, lloss]),
                 vertex_packetloss=vl, directed=directed, name=f"wide{n}_s{scale}")


def dumbbell(total: int) -> Graph:
    """The path 2 - 1 - 0 - 3 - 4 (total even): each arm, {0-1, 1-2} and {0-3, 3-4}, sums to
    total / 2, so bound = ecc_out(0) + ecc_in(0) = total and d(2, 4) = total.  An undirected
    graph's bound is even: 65534 and 65536 are the two sides of the u16 rule bound < 65535.
    Self-loops on 0, 1 and 4 only."""
    a = b = total // 2
    src = np.array([0, 1, 0, 3, 0, 1, 4], np.int32)
    dst = np.array([1, 2, 3, 4, 0, 1, 4], np.int32)
    lat = np.array([a // 2, a - a // 2, b // 2, b - b // 2, 7, 40000, 65534], np.float64)
    loss = np.array([1, 2, 3, 4, 5, 6, 7], np.float64) / _LOSS_DEN
    return Graph(n=5, src=src, dst=dst, latency=lat, packetloss=loss, name=f"dumbbell{total}")


def long_path(total: int, n: int = 389) -> Graph:
    """A path of n vertices with vertex 0 in the middle, every latency below 256 and six
    distinct losses, each arm summing to total / 2: the narrow encodings (KD's packed records
    and seeded plans, KB's fused rows) with distances up to `total` = bound.  Self-loops on the
    vertices v with v % 3 != 1."""
    h = (n - 1) // 2
    arms = []
    for k in (h, n - 1 - h):
        w = np.full(k, (total // 2) // k, np.int64)
        w[: (total // 2) - int(w.sum())] += 1
        arms.append(w)
    assert max(int(a.max()) for a in arms) < 256 and all(int(a.sum()) == total // 2 for a in arms)
    # arm 1: 0 - 1 - ... - h; arm 2: 0 - (h+1) - ... - (n-1)
    src = np.concatenate([np.arange(0, h), [0], np.arange(h + 1, n - 1)]).astype(np.int32)
    dst = np.concatenate([np.arange(1, h + 1), np.arange(h + 1, n)]).astype(np.int32)
    lat = np.concatenate(arms).astype(np.float64)
    loss = (np.arange(len(src)) % 6) / _LOSS_DEN
    lv = np.flatnonzero(np.arange(n) % 3 != 1).astype(np.int32)
    return Graph(n=n, src=np.concatenate([src, lv]), dst=np.concatenate([dst, lv]),
                 latency=np.concatenate([lat, 1.0 + (lv % 9)]),
                 packetloss=np.concatenate([loss, (lv % 4) / _LOSS_DEN]), name=f"path{n}_{total}")


def many_rel(n: int, m: int, nrel: int | None = None, seed: int = 5) -> Graph:
    """A simple connected graph of m edges (a ring plus random chords), latencies U[1, 250],
    edge e's loss ((e mod nrel) + 1) / 2**21 (nrel None: m, every edge its own reliability).
    Self-loops (loss 0) on the even vertices."""
    rng = np.random.default_rng(seed)
    have = {(i, (i + 1) % n) if i + 1 < n else (0, n - 1) for i in range(n)}
    edges = sorted(have)
    while len(edges) < m:
        ab = rng.integers(0, n, size=(4 * (m - len(edges)) + 16, 2))
        for a, b in ab:
            a, b = int(min(a, b)), int(max(a, b))
            if a != b and (a, b) not in have:
                have.add((a, b)); edges.append((a, b))
                if len(edges) == m:
                    break
    e = np.asarray(edges, np.int32)
    nrel = m if nrel is None else nrel
    lat = rng.integers(1, 251, size=m).astype(np.float64)
    loss = ((np.arange(m) % nrel) + 1) / _LOSS_DEN
    lv = np.arange(0, n, 2, dtype=np.int32)
    return Graph(n=n, src=np.concatenate([e[:, 0], lv]), dst=np.concatenate([e[:, 1], lv]),
                 latency=np.concatenate([lat, rng.integers(1, 11, size=len(lv)).astype(np.float64)]),
                 packetloss=np.concatenate([loss, np.zeros(len(lv))]), name=f"manyrel{n}_{nrel}")


def decimal(g: Graph, scale: int, kmax: int = 65535, seed: int = 0, over: bool = False) -> Graph:
    """g's topology with latencies k / scale, k in U[1, kmax] (edge 0: kmax itself, edge 1: a
    k that is no multiple of 10, so that no smaller scale fits; with `over` edge 2 gets
    kmax + 1).  Each value is the double its decimal text parses to: the one correctly rounded
    division k / scale, as in shadow_amd.graph.fractional."""
    rng = np.random.default_rng(20_000 + seed)
    k = rng.integers(1, kmax + 1, size=g.m)
    nl = np.flatnonzero(g.src != g.dst)
    k[nl[0]] = kmax
    k[nl[1]] = kmax - 4 if (kmax - 4) % 10 else kmax - 3
    if over:
        k[nl[2]] = kmax + 1
    return dataclasses.replace(g, latency=k.astype(np.float64) / float(scale),
                               name=f"{g.name}_dec{scale}" + ("_over" if over else ""))


def decimal_base() -> Graph:
    """The narrow graph the decimal variants are made from (about 100 distinct reliabilities,
    so KF and KFH take them), with the self-loops of every third vertex removed."""
    g = internet_like(389, 3, seed=21, name="ba389")
    keep = (g.src != g.dst) | (g.src % 3 != 1)
    return dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], latency=g.latency[keep],
                               packetloss=g.packetloss[keep], vertex_packetloss=None)


def front_pair():
    """Two prefer-direct graphs that differ in one edge: 1 - 3 with latency 32767 or 32768, the
    largest of the graph.  The path 2 - 1 - 0 - 3 - 4 beside it is shorter (29000 ms from 1 to
    3), so the engine's bound (60000) and info.lat16 are the same for both, and only the front
    end's rule 2 * max edge latency < 0xFFFF tells them apart; prefer-direct stores the heavy
    edge itself as the Path of {1, 3}.  d(2, 4) = 59000 is past the sign bit of a u16.
    Self-loops on 0, 3 and 5 only; vertex 5 hangs off 0."""
    out = []
    for w in (32767, 32768):
        src = np.array([0, 1, 0, 3, 1, 0, 0, 3, 5], np.int32)
        dst = np.array([1, 2, 3, 4, 3, 5, 0, 3, 5], np.int32)
        lat = np.array([15000, 15000, 14000, 15000, w, 9, 3, 31000, 11], np.float64)
        loss = np.arange(1, 10, dtype=np.float64) / _LOSS_DEN
        out.append(Graph(n=6, src=src, dst=dst, latency=lat, packetloss=loss, prefer_direct=True,
                         name=f"front{w}"))
    return tuple(out)


# the two wide scales of the suite (n = 389, seed 7): see test_range_graphs.py for the bounds
WIDE_HI_SCALE = 480
WIDE_MID_SCALE = 200

SUITE = {
    "wide_hi": lambda: wide(389, 7, WIDE_HI_SCALE),
    "wide_mid": lambda: wide(389, 7, WIDE_MID_SCALE),
    "wide_vloss": lambda: wide(389, 9, WIDE_MID_SCALE, vloss=True),
    "wide_fewrel": lambda: wide(389, 8, WIDE_MID_SCALE, vloss=True, nloss=200),
    "wide_dir": lambda: wide(389, 13, WIDE_MID_SCALE, directed=True),
    "dumbbell65534": lambda: dumbbell(65534),
    "dumbbell65536": lambda: dumbbell(65536),
    "path65534": lambda: long_path(65534),
    "manyrel70k": lambda: many_rel(1200, 70000),
    "manyrel255": lambda: many_rel(300, 900, nrel=255),
    "manyrel257": lambda: many_rel(300, 900, nrel=257),
    "dec1": lambda: decimal(decimal_base(), 1),
    "dec10": lambda: decimal(decimal_base(), 10),
    "dec100": lambda: decimal(decimal_base(), 100),
    "dec1000": lambda: decimal(decimal_base(), 1000),
    "dec100_over": lambda: decimal(decimal_base(), 100, over=True),
    "front32767": lambda: front_pair()[0],
    "front32768": lambda: front_pair()[1],
}

_cache: dict = {}


def get(name: str) -> Graph:
    """The suite's graph of that name (built once per process; treat it as read-only)."""
    if name not in _cache:
        _cache[name] = SUITE[name]()
    return _cache[name]
