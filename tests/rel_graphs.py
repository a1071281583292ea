"""Deterministic topologies on the reliability axis, for test_rel_gpu.py and
test_rel_paths_gpu.py.  Every other builder of the suite keeps its reliabilities in (0.5, 1],
every product in the normal range, and puts a lossless arc into every graph whose reliability
table is small enough for the compact kernel forms; shd_route_create accepts any loss and any
vertex loss in [0, 1].  Each builder here is named for the reliabilities it feeds a kernel;
test_rel_graphs.py asserts those properties with the oracle and the Python references alone,
without the engine.  The latencies stay narrow (integers 1..250 unless stated), so that the
packed, fused and seeded encodings stay eligible and the reliabilities alone decide.

  rel_zero        BA(389, 3), self-loops on the vertices v % 3 != 1: 12% of the non-loop edges
                  have loss exactly 1.0 (r = 0.0, q = 1.0), 8% loss exactly 0.0 (r = 1.0), the
                  rest k / 2**21 with k in [1, 150); five self-loops have loss 1.0
  rel_zero_ties   the same with latencies 1..3: heavy ties, envelopes with rel_lo == 0 < rel_hi
                  and with rel_hi == 0
  rel_zero_dir    directed, every BA edge two arcs: the forward arc of 12% of the pairs has loss
                  1.0, its reverse arc never
  rel_zero8000    rel_zero at 8000 vertices: past the size at which the generic kernel keeps its
                  per-source state in LDS
  rel_vzero       BA(389, 3) with narrow edge losses; vertex loss 1.0 on 6 vertices (three of
                  them the hubs 0, 1, 2), one of {0.5, 0.999, 1 - 2**-30} on 30, 0.0 on 100,
                  absent (NaN) on the rest
  rel_tinyloss    15% of the edges have loss 2**-60: 1.0 - loss == 1.0 (the slot of the lossless
                  arcs) while q = loss > 0
  rel_lossy254,   a ring of 300 plus chords, 900 edges: exactly 254 / 255 distinct
  rel_lossy255    reliabilities over the non-loop edges, none of them 1.0; lossy self-loops
  rel_one254      the same shape: 253 lossy values and 1.0
  rel_256, 257    the same shape: 256 / 257 distinct values (1.0 among them)
  rel_65535, 65536  a ring of 1200 plus chords, 70000 edges: 65535 / 65536 distinct values
  rel_deep        a chain of 600 vertices, latencies 1..9, a lossless self-loop on every vertex,
                  arc reliabilities m / 64 with m odd in 3..15: a row's products run through the
                  subnormals to 0.0
  rel_deep_frac   rel_deep with latencies k / 100

Every loss is chosen so that 1.0 - loss is exact (k / 2**21, 1 - m / 64, 0.5, 0.999,
1 - 2**-30, 0.0, 1.0) or is exactly 1.0 (2**-60).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from shadow_amd.graph import Graph, barabasi_albert_edges
from tests.range_graphs import many_rel

_LOSS_DEN = float(2 ** 21)
NLOSS = 150
TINY = 2.0 ** -60
VHALF = (0.5, 0.999, 1.0 - 2.0 ** -30)
N_BA = 389
N_DEEP = 600

# seeds: test_rel_graphs.py asserts the shares and the tie envelopes these give
SEED_ZERO, SEED_TIES, SEED_DIR, SEED_VZERO, SEED_TINY, SEED_DEEP, SEED_BIG = 31, 32, 33, 34, 35, 1, 36


def _narrow(rng, k, lo=1):
    """Losses k / 2**21, k in [lo, NLOSS): lo = 0 is the suite's default, with lossless arcs."""
    return rng.integers(lo, NLOSS, size=k) / _LOSS_DEN


def _ba(n, seed, latmax, directed=False):
    """(rng, edges, latencies, looped vertices, loop latencies) of BA(n, 3)."""
    rng = np.random.default_rng(seed)
    e = barabasi_albert_edges(n, 3, rng)
    if directed:
        e = np.concatenate([e, e[:, ::-1]])
    lat = rng.integers(1, latmax + 1, size=len(e)).astype(np.float64)
    lv = np.flatnonzero(np.arange(n) % 3 != 1).astype(np.int32)
    return rng, e, lat, lv, 1.0 + (lv % 9)


def _graph(n, e, lat, loss, lv, llat, lloss, **kw) -> Graph:
    return Graph(n=n, src=np.concatenate([e[:, 0], lv]).astype(np.int32),
                 dst=np.concatenate([e[:, 1], lv]).astype(np.int32),
                 latency=np.concatenate([lat, llat]).astype(np.float64),
                 packetloss=np.concatenate([loss, lloss]).astype(np.float64), **kw)


def rel_zero(seed: int = SEED_ZERO, latmax: int = 250, directed: bool = False, name: str = "rel_zero",
             n: int = N_BA) -> Graph:
    rng, e, lat, lv, llat = _ba(n, seed, latmax, directed)
    k = len(e)
    u = rng.random(k)
    loss = np.where(u < 0.12, 1.0, np.where(u < 0.20, 0.0, _narrow(rng, k)))
    if directed:                                      # the reverse arc of a dead arc is alive
        h = k // 2
        loss[h:] = np.where(loss[h:] == 1.0, _narrow(rng, h), loss[h:])
        assert not np.any((loss[:h] == 1.0) & (loss[h:] == 1.0))
    lloss = _narrow(rng, len(lv))
    lloss[rng.choice(len(lv), size=5, replace=False)] = 1.0
    return _graph(n, e, lat, loss, lv, llat, lloss, directed=directed, name=name)


def rel_vzero(seed: int = SEED_VZERO) -> Graph:
    rng, e, lat, lv, llat = _ba(N_BA, seed, 250)
    n = N_BA
    vl = np.full(n, np.nan)
    rest = rng.permutation(np.arange(3, n))
    dead = np.concatenate([[0, 1, 2], rest[:3]])      # BA's first vertices carry the most paths
    vl[dead] = 1.0
    vl[rest[3:33]] = rng.choice(np.array(VHALF), size=30)
    vl[rest[33:133]] = 0.0
    return _graph(n, e, lat, _narrow(rng, len(e), 0), lv, llat, _narrow(rng, len(lv), 0), vertex_packetloss=vl,
                  name="rel_vzero")


def rel_tinyloss(seed: int = SEED_TINY) -> Graph:
    rng, e, lat, lv, llat = _ba(N_BA, seed, 250)
    k = len(e)
    loss = np.where(rng.random(k) < 0.15, TINY, _narrow(rng, k, 0))
    return _graph(N_BA, e, lat, loss, lv, llat, _narrow(rng, len(lv), 0), name="rel_tinyloss")


def without_loss(g: Graph) -> Graph:
    """g with every 2**-60 loss set to 0.0: the same reliabilities, no drop on those links."""
    return dataclasses.replace(g, packetloss=np.where(g.packetloss == TINY, 0.0, g.packetloss),
                               name=g.name + "_noloss")


def rel_table(n: int, m: int, nrel: int, one: bool, name: str) -> Graph:
    """range_graphs.many_rel(n, m): non-loop edge e has loss ((e mod nrel) + 1) / 2**21, or with
    `one` loss (e mod nrel) / 2**21 (so that 1.0 is one of the nrel values); self-loop k has the
    loss (k mod 7 + 1) / 2**21, one of the edges' values."""
    g = many_rel(n, m, nrel=nrel)
    nl = g.src != g.dst
    loss = g.packetloss.copy()
    if one:
        loss[nl] = loss[nl] - 1.0 / _LOSS_DEN
    loss[~nl] = (np.arange(int((~nl).sum())) % 7 + 1) / _LOSS_DEN
    return dataclasses.replace(g, packetloss=loss, name=name)


def rel_deep(seed: int = SEED_DEEP, frac: bool = False) -> Graph:
    rng = np.random.default_rng(seed)
    n = N_DEEP
    a = np.arange(n - 1, dtype=np.int32)
    k = rng.integers(1, 10, size=n - 1)
    m = 2 * rng.integers(1, 8, size=n - 1) + 1        # odd, 3..15
    lv = np.arange(n, dtype=np.int32)
    lk = 1 + (lv % 9)
    sc = 100.0 if frac else 1.0
    return _graph(n, np.stack([a, a + 1], axis=1), k / sc, 1.0 - m / 64.0, lv, lk / sc, np.zeros(n),
                  name="rel_deep_frac" if frac else "rel_deep")


SUITE = {
    "rel_zero": lambda: rel_zero(),
    "rel_zero_ties": lambda: rel_zero(SEED_TIES, latmax=3, name="rel_zero_ties"),
    "rel_zero_dir": lambda: rel_zero(SEED_DIR, directed=True, name="rel_zero_dir"),
    "rel_zero8000": lambda: rel_zero(SEED_BIG, name="rel_zero8000", n=8000),
    "rel_vzero": lambda: rel_vzero(),
    "rel_tinyloss": lambda: rel_tinyloss(),
    "rel_lossy254": lambda: rel_table(300, 900, 254, False, "rel_lossy254"),
    "rel_lossy255": lambda: rel_table(300, 900, 255, False, "rel_lossy255"),
    "rel_one254": lambda: rel_table(300, 900, 254, True, "rel_one254"),
    "rel_256": lambda: rel_table(300, 900, 256, True, "rel_256"),
    "rel_257": lambda: rel_table(300, 900, 257, True, "rel_257"),
    "rel_65535": lambda: rel_table(1200, 70000, 65535, True, "rel_65535"),
    "rel_65536": lambda: rel_table(1200, 70000, 65536, True, "rel_65536"),
    "rel_deep": lambda: rel_deep(),
    "rel_deep_frac": lambda: rel_deep(frac=True),
}
# table size over the non-loop edges, and whether 1.0 is one of the values
TABLES = {"rel_lossy254": (254, False), "rel_lossy255": (255, False), "rel_one254": (254, True),
          "rel_256": (256, True), "rel_257": (257, True), "rel_65535": (65535, True), "rel_65536": (65536, True)}

_cache: dict = {}


def get(name: str) -> Graph:
    """The suite's graph of that name (built once per process; read-only)."""
    if name not in _cache:
        g = SUITE[name]()
        for a in (g.src, g.dst, g.latency, g.packetloss):
            a.setflags(write=False)
        _cache[name] = g
    return _cache[name]


def vclasses(g: Graph):
    """rel_vzero's vertices by class: (loss 1.0, a loss strictly between, loss 0.0, absent)."""
    vl = g.vertex_packetloss
    return (np.flatnonzero(vl == 1.0), np.flatnonzero((vl > 0.0) & (vl < 1.0)), np.flatnonzero(vl == 0.0),
            np.flatnonzero(np.isnan(vl)))


def sources(name: str, k: int = 24) -> np.ndarray:
    """At most k sources, sorted: spread over the graph with the first and the last vertex; both
    ends and the middle of the chain; on rel_vzero two vertices of every class of vertex loss (the
    hub 0 among them)."""
    g = get(name)
    pick = np.linspace(0, g.n - 1, k - 8 if name == "rel_vzero" else k).astype(np.int64).tolist()
    if name.startswith("rel_deep"):
        pick[len(pick) // 2] = g.n // 2
    if name == "rel_vzero":
        for c in vclasses(g):
            pick += [int(c[0]), int(c[-1])]
    S = np.unique(np.array(pick, np.int32))
    assert len(S) <= k
    return S
