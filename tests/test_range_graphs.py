"""The range_graphs builders have the input properties they are named for (no GPU, no
engine, no oracle: a plain heap Dijkstra over the arcs).  These are conditions on the test
inputs of test_range_gpu.py / test_contract_gpu.py: if a builder drifted back into the narrow
range, those tests would still pass while no longer reaching the encodings they are for."""
import heapq

import numpy as np
import pytest

from tests import range_graphs as rg


def _arcs(g, reverse=False):
    adj = [[] for _ in range(g.n)]
    for a, b, w in zip(g.src.tolist(), g.dst.tolist(), g.latency.tolist()):
        if a == b:
            continue
        if reverse:
            a, b = b, a
        adj[a].append((b, w))
        if not g.directed:
            adj[b].append((a, w))
    return adj


def _dijkstra(adj, s):
    dist = [float("inf")] * len(adj)
    dist[s] = 0.0
    heap = [(0.0, s)]
    while heap:
        d, u = heapq.heappop(heap)
        if d > dist[u]:
            continue
        for v, w in adj[u]:
            nd = d + w
            if nd < dist[v]:
                dist[v] = nd
                heapq.heappush(heap, (nd, v))
    return dist


def props(g, all_pairs=True):
    """bound = ecc_out(0) + ecc_in(0) (the engine's u16 eligibility), connectivity, and over
    all sources the largest distance and the largest tentative sum d(s, u) + w(u, v)."""
    out, inn = _arcs(g), _arcs(g, reverse=True)
    d0, r0 = _dijkstra(out, 0), _dijkstra(inn, 0)
    p = {"connected": max(d0) < float("inf") and max(r0) < float("inf"), "bound": max(d0) + max(r0)}
    nl = g.src != g.dst
    p["nrel"] = len(np.unique(1.0 - g.packetloss[nl]))
    p["noloop"] = 1.0 - len(np.unique(g.src[~nl])) / g.n
    p["maxw"] = float(g.latency.max())
    p["integer"] = bool(np.all(g.latency == np.floor(g.latency)))
    if all_pairs:
        wmax = [max(w for _, w in a) for a in out]
        dmax = tmax = 0.0
        for s in range(g.n):
            d = _dijkstra(out, s)
            dmax = max(dmax, max(d))
            tmax = max(tmax, max(du + w for du, w in zip(d, wmax)))
        p["dmax"], p["tmax"] = dmax, tmax
    return p


@pytest.mark.parametrize("name", ["wide_hi", "wide_mid", "wide_vloss", "wide_fewrel", "wide_dir"])
def test_wide(name):
    g = rg.get(name)
    p = props(g)
    assert g.n % 64 != 0 and p["connected"] and p["integer"]
    assert p["tmax"] > 65535                 # tentative sums leave u16
    if name == "wide_fewrel":
        assert p["nrel"] <= 200              # (within the u8 tables: KD's walks, KF)
    else:
        assert p["nrel"] > 1000              # past KD's packed records, KF's and KB's u8 tables
    assert p["maxw"] >= 32768 and g.latency[g.src != g.dst].max() <= 65535
    assert 0.2 < p["noloop"] < 0.5           # vertices of both kinds
    if name == "wide_hi":
        assert 50000 <= p["bound"] <= 65534 and p["dmax"] >= 32768
    else:
        assert 12000 <= p["bound"] < 40000
    assert p["dmax"] <= p["bound"]
    assert (g.vertex_packetloss is not None) == (name in ("wide_vloss", "wide_fewrel"))
    assert g.directed == (name == "wide_dir")


@pytest.mark.parametrize("total", [65534, 65536])
def test_dumbbell(total):
    g = rg.get(f"dumbbell{total}")
    p = props(g)
    assert p["connected"] and p["integer"]
    assert p["bound"] == total and p["dmax"] == total   # 0xFFFE: the top legal u16 distance
    assert p["tmax"] > 65535
    assert 0 < p["noloop"] < 1
    assert g.latency[g.src == g.dst].max() < 65535      # the diagonal alone never costs lat16


def test_long_path():
    g = rg.get("path65534")
    p = props(g)
    assert g.n % 64 != 0 and p["connected"] and p["integer"]
    assert p["bound"] == 65534 and p["dmax"] == 65534 and p["tmax"] > 65535
    assert p["maxw"] < 256 and p["nrel"] <= 6 and 0 < p["noloop"] < 1


def test_many_rel():
    g = rg.get("manyrel70k")
    p = props(g, all_pairs=False)
    assert p["connected"] and p["nrel"] == 70000 > 65535 and g.m_nonloop == 70000
    assert p["bound"] < 65535 and p["maxw"] <= 250
    pairs = set(zip(np.minimum(g.src, g.dst).tolist(), np.maximum(g.src, g.dst).tolist()))
    assert len(pairs) == g.m                            # simple
    for nrel in (255, 257):                             # past the u8 tables, within the u16 ones
        g = rg.get(f"manyrel{nrel}")
        p = props(g, all_pairs=False)
        assert p["connected"] and p["nrel"] == nrel and p["maxw"] <= 250 and 0 < p["noloop"] < 1


@pytest.mark.parametrize("scale", [1, 10, 100, 1000])
def test_decimal(scale):
    for name in [f"dec{scale}"] + (["dec100_over"] if scale == 100 else []):
        g = rg.get(name)
        k = np.rint(g.latency * scale)
        assert np.array_equal(k / scale, g.latency)     # each the double the decimal parses to
        nl = g.src != g.dst
        assert k[nl].max() == (65536 if name.endswith("over") else 65535) and k.min() >= 1
        assert np.count_nonzero(k[nl] > 65535) == (1 if name.endswith("over") else 0)
        if scale > 1:                                   # no smaller scale holds them
            k10 = g.latency[nl] * (scale // 10)
            assert not np.array_equal(k10, np.rint(k10))
        p = props(g, all_pairs=False)
        assert p["connected"] and p["nrel"] <= 254 and 0 < p["noloop"] < 1
        assert p["integer"] == (scale == 1)
        if scale == 1:
            assert p["bound"] >= 65535                  # integer, but no u16 kernel


def test_front_pair():
    a, b = rg.front_pair()
    assert a.latency.max() == 32767 and b.latency.max() == 32768
    assert 2 * a.latency.max() < 0xFFFF <= 2 * b.latency.max()
    for g in (a, b):
        p = props(g)
        assert p["connected"] and p["integer"] and g.prefer_direct
        assert p["bound"] == 60000 and p["dmax"] == 59000   # the same u16-eligible bound for both
        assert 0 < p["noloop"] < 1
