"""The shape_graphs builders have the properties they are named for (no GPU, no engine: numpy
and a plain heap Dijkstra over the arcs; the CPU oracle only for the share of entries its two
tie rules disagree on).  These are conditions on the test inputs of test_shape_gpu.py: if a
builder drifted off a limit, those tests would still pass while no longer standing on both
sides of it."""
import heapq

import numpy as np
import pytest

from tests import shape_graphs as sg

KB_SEG, KB_BLOCK, KB_RIT, KF_HUB, HP_WIDE, KD_IMP, WALK = 16, 1024, 3, 24, 32, 192, 32   # shadow_amd/csrc


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


def hop_range(adj, s):
    """(fewest, most) hops of a shortest path from s to its farthest-in-hops vertex: bounds on
    the depth of the shortest-path tree under any tie rule."""
    dist = _dijkstra(adj, s)
    lo = [0] * len(adj); hi = [0] * len(adj)
    seen = [False] * len(adj)
    for u in sorted(range(len(adj)), key=dist.__getitem__):   # positive latencies: parents first
        for v, w in adj[u]:
            if dist[u] + w == dist[v]:
                lo[v] = min(lo[v], lo[u] + 1) if seen[v] else lo[u] + 1
                hi[v] = max(hi[v], hi[u] + 1)
                seen[v] = True
    return max(lo), max(hi)


def in_degree(g):
    """In-arcs per vertex, as prepare_k32 builds irow: one per non-loop arc into the vertex,
    an undirected edge being an arc each way."""
    nl = g.src != g.dst
    d = np.bincount(g.dst[nl], minlength=g.n)
    return d if g.directed else d + np.bincount(g.src[nl], minlength=g.n)


def has_loop(g):
    m = np.zeros(g.n, bool)
    m[g.src[g.src == g.dst]] = True
    return m


@pytest.mark.parametrize("name", list(sg.SUITE))
def test_counts_connectivity_and_encodings(name):
    """Vertex and edge counts, strong connectivity, and the narrow value range: integer
    latencies below 256, at most 254 reliabilities, bound = ecc_out(0) + ecc_in(0) < 65535."""
    g = sg.get(name)
    nl = g.src != g.dst
    m = int(nl.sum())
    if name.startswith("tiny"):
        assert g.n in sg.TINY_N and m == g.n - 1
        want = {"all": g.n, "none": 0, "some": len(range(0, g.n, 3)) + len(range(2, g.n, 3))}[name.split("_")[1]]
        assert int((~nl).sum()) == want
        if name == "tiny1_none":
            assert g.m == 0 and g.nnz == 0
    else:
        assert np.array_equal(has_loop(g), np.arange(g.n) % 3 != 1)
    if name.startswith("sized"):
        assert g.n == int(name[5:]) and m == 3 * (g.n - 3) and g.vertex_packetloss is None
    want_nm = {"star300": (300, 299 + 75), "star1100": (1100, 1099 + 275), "biclique1000": (1017, 17000),
               "biclique1030": (1047, 17510), "bireg512": (1024, 8704), "bireg513": (1026, 8721),
               "grid": (1056, 32 * 32 + 31 * 33), "grid_vloss": (1056, 32 * 32 + 31 * 33), "lollipop": (340, 780 + 300),
               "dir_grid": (256, 2 * 2 * 16 * 15)}
    if name in want_nm:
        assert (g.n, m) == want_nm[name]
    assert g.directed == (name == "dir_grid") and not g.prefer_direct
    assert (g.vertex_packetloss is not None) == (name == "grid_vloss")
    pairs = set(zip(g.src.tolist(), g.dst.tolist())) if g.directed else \
        set(zip(np.minimum(g.src, g.dst).tolist(), np.maximum(g.src, g.dst).tolist()))
    assert len(pairs) == g.m                                   # simple: no parallel edges
    out, inn = _arcs(g), _arcs(g, reverse=True)
    d0, r0 = _dijkstra(out, 0), _dijkstra(inn, 0)
    assert max(d0) < float("inf") and max(r0) < float("inf")   # strongly connected
    assert max(d0) + max(r0) < 65535
    if g.m == 0:
        return
    assert np.all(g.latency == np.floor(g.latency)) and g.latency.min() >= 1 and g.latency.max() < 256
    k = g.packetloss * 2.0 ** 21
    if not name.startswith("sized"):                           # (internet_like: k * 1e-4)
        assert np.all(k == np.floor(k)) and k.max() < sg.NLOSS
    assert len(np.unique(1.0 - g.packetloss[nl])) <= 200 and len(np.unique(1.0 - g.packetloss)) <= 254
    assert g.nnz < 0xFFFF or g.n >= 11212


def test_sizes_straddle_the_limits():
    for a in (64, 256, 1024, 2048, 4096, 16384):     # nw, latency blocks, KB_SRC n, KD block
        assert {a - 1, a, a + 1} <= set(sg.SIZES) or {a, a + 1} <= set(sg.SIZES)
    assert {2688, 2689, 11212, 11213} <= set(sg.SIZES)   # where the KF forms' LDS state ends
    assert set(sg.TINY_N) == {1, 2, 3, 7, 8, 9}      # below and around qcap's floor of 8


def test_hub_counts():
    """Vertices of more than 16 (KB_SEG), 24 (KF_HUB) and 32 (HP_WIDE) in-arcs."""
    count = lambda name: tuple(int((in_degree(sg.get(name)) > k).sum()) for k in (KB_SEG, KF_HUB, HP_WIDE))
    for name, n in (("star300", 300), ("star1100", 1100)):
        d = in_degree(sg.get(name))
        assert count(name) == (1, 1, 1) and d[0] == n - 1 > KD_IMP and set(d[1:].tolist()) == {1, 2}
    assert -(-1099 // KB_SEG) == 69                  # hub parts of the star's one in-row
    # K_{17,b}: every vertex is past KB_SEG (the b side by one arc), the 17 past the others
    assert count("biclique1000") == (1017, 17, 17) and count("biclique1030") == (1047, 17, 17)
    assert count("biclique1000")[0] <= KB_BLOCK < count("biclique1030")[0]
    # the same on both sides of KB_BLOCK exactly, in-rows of 17 = KB_SEG + 1 arcs each
    assert count("bireg512") == (1024, 0, 0) and count("bireg513") == (1026, 0, 0)
    assert count("bireg512")[0] <= KB_BLOCK < count("bireg513")[0]
    for name in sg.BIREGS:                           # segments per thread within KB_RIT
        d = in_degree(sg.get(name))
        assert int(np.ceil(d / KB_SEG).sum()) <= KB_RIT * KB_BLOCK
    d = in_degree(sg.get("lollipop"))
    assert int((d > HP_WIDE).sum()) == 40 and d.max() == 40 and d[40:].max() == 2
    for n in (300, 700):                             # what the suite had before: BA(n, 3)
        d = in_degree(sg.sized(n))
        assert 0 < (d > KB_SEG).sum() < 40 and d.max() < KD_IMP
    assert in_degree(sg.get("grid")).max() == 4 and in_degree(sg.get("dir_grid")).max() == 4


def test_depths():
    """Trees deeper than the 32-arc walk windows (KD_MAXD, KB_MAXD) under any tie rule on the
    grid, the lollipop and the regular bipartite graphs; at most two hops on the star and the
    bicliques.  (BA graphs stay shallow: 14 hops at most on sized1025.)"""
    g = sg.get("grid")
    assert hop_range(_arcs(g), 0) == (63, 63) and hop_range(_arcs(g), g.n - 1) == (63, 63)
    assert hop_range(_arcs(sg.get("lollipop")), 0)[0] > 300
    assert hop_range(_arcs(sg.get("dir_grid")), 0) == (30, 30)
    for name in sg.BIREGS:
        assert hop_range(_arcs(sg.get(name)), 0)[0] > WALK
    for name in ("star300", "star1100") + sg.BICLIQUES:
        g = sg.get(name)
        adj = _arcs(g)
        for s in (0, 1, 2, g.n - 1):
            assert hop_range(adj, s)[1] <= 2
    assert hop_range(_arcs(sg.get("sized1025")), 0)[1] < WALK


@pytest.mark.parametrize("name", ["grid", "grid_vloss", "dir_grid"] + list(sg.BICLIQUES + sg.BIREGS))
def test_tie_rules_disagree_on_most_entries(oracle_mod, name):
    """A condition on the inputs: from sampled self-looped sources, the oracle's two tie rules
    give the same latencies and different reliabilities for at least half of the entries, so
    a kernel that picks another parent among equals changes bits in most of a row.  (Measured:
    grid 0.87, dir_grid 0.75, K_{17,1000} 0.78, K_{17,1030} 0.75, bireg 0.71 / 0.74.)"""
    g = sg.get(name)
    og = oracle_mod.OracleGraph(g)
    hl = np.flatnonzero(has_loop(g))
    S = hl[:: len(hl) // 8][:8]
    T = np.arange(g.n, dtype=np.int32)
    a = og.source_rows(S, T, oracle_mod.TIE_MINKEY)
    b = og.source_rows(S, T, oracle_mod.TIE_IGRAPH)
    assert np.array_equal(a[0], b[0])
    share = float(np.mean(a[1] != b[1]))
    print(name, "share of entries the tie rules disagree on: %.3f" % share)
    assert share >= 0.5
    assert np.count_nonzero(~a[2]) >= 0.5 * a[2].size          # non-unique shortest paths
