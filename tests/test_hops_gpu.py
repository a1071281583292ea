"""GPU: path hops -- hop counts (shd_route_hops), explicit routes (shd_route_paths) and the
front end's route line -- against the oracle's min-key parent chain.

Oracle paths are rebuilt here from OracleGraph.dijkstra(s, TIE_MINKEY)'s parent_eid: the
path to t is the chain of parent edges back to s.  check_chain() compares every returned
path with that chain at once (each hop's edge must be the oracle's parent edge of the hop's
head and its other end the hop's tail, first vertex s, last vertex t: the chain is the only
sequence that passes); oracle_path() rebuilds single chains for literal comparison."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from shadow_amd.graph import Graph, internet_like, to_graphml

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
SMALL = ["ba60", "ba64_ties", "ba80_prefer", "ba100_attached", "dir40", "ba90_frac", "ba120_vloss", "k24"]


@pytest.fixture(scope="module")
def route():
    from shadow_amd import route
    route.load_library()
    return route


@pytest.fixture(scope="module")
def topo():
    from shadow_amd import topology
    topology.load_library()
    return topology


def _ring():
    """Directed ring 0 -> 1 -> ... -> 514 -> 0, integer latencies 1-3, no self-loops."""
    n = 515
    rng = np.random.default_rng(515)
    src = np.arange(n, dtype=np.int32)
    return Graph(n=n, src=src, dst=((src + 1) % n).astype(np.int32), latency=rng.integers(1, 4, size=n).astype(np.float64),
                 packetloss=rng.integers(0, 3, size=n) * 1e-3, vertex_packetloss=None, directed=True, name="ring515")


def _multi():
    """ba60 plus 10 parallel edges of differing latency."""
    g = _graph("ba60")[0]
    rng = np.random.default_rng(60)
    nl = np.flatnonzero(g.src != g.dst)
    pick = rng.choice(nl, size=10, replace=False)
    lat = g.latency[pick] + rng.choice([-1.0, 1.0, 2.0], size=10)
    lat = np.where(lat < 1.0, g.latency[pick] + 1.0, lat)
    return Graph(n=g.n, src=np.concatenate([g.src, g.dst[pick]]).astype(np.int32),
                 dst=np.concatenate([g.dst, g.src[pick]]).astype(np.int32), latency=np.concatenate([g.latency, lat]),
                 packetloss=np.concatenate([g.packetloss, g.packetloss[pick]]), vertex_packetloss=g.vertex_packetloss,
                 name="ba60_multi")


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(graph, attached sources) of a fixture: a small_tables.npz graph or a generated one."""
    if name == "ring515":
        g = _ring()
        return g, np.arange(0, g.n, 33, dtype=np.int32)[:16]
    if name == "i2000":
        g = internet_like(2000, 4, 1)
        return g, (np.arange(8, dtype=np.int32) * 249)
    if name == "ring66k":
        # above 65535 vertices the u16 forms do not apply: a ring with as many random chords
        n = 66000
        rng = np.random.default_rng(66)
        a = np.arange(n, dtype=np.int32)
        c0 = rng.integers(0, n, size=n).astype(np.int32); c1 = rng.integers(0, n, size=n).astype(np.int32)
        keep = c0 != c1
        src = np.concatenate([a, c0[keep]]); dst = np.concatenate([(a + 1) % n, c1[keep]]).astype(np.int32)
        g = Graph(n=n, src=src, dst=dst, latency=rng.integers(1, 21, size=len(src)).astype(np.float64),
                  packetloss=np.zeros(len(src)), vertex_packetloss=None, name="ring66k")
        return g, np.array([5, 65999], np.int32)
    if name == "ba60_multi":
        g = _multi()
        return g, np.arange(g.n, dtype=np.int32)
    if name == "ba60_holes":
        # ba60 (a self-loop at every vertex) without the self-loops of the odd vertices
        g, A = _graph("ba60")
        keep = ~((g.src == g.dst) & (g.src % 2 == 1))
        return Graph(n=g.n, src=g.src[keep], dst=g.dst[keep], latency=g.latency[keep], packetloss=g.packetloss[keep],
                     vertex_packetloss=g.vertex_packetloss, name=name), A
    z = np.load(os.path.join(GOLD, "small_tables.npz"))
    p = f"{name}__"
    vl = z[p + "vertex_packetloss"]
    g = Graph(n=int(z[p + "n"]), src=z[p + "src"], dst=z[p + "dst"], latency=z[p + "latency"],
              packetloss=z[p + "packetloss"], vertex_packetloss=vl if len(vl) else None,
              directed=bool(z[p + "directed"]), prefer_direct=bool(z[p + "prefer_direct"]), name=name)
    return g, np.asarray(z[p + "attached"], np.int32)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import OracleGraph
    return OracleGraph(_graph(name)[0])


@functools.lru_cache(maxsize=None)
def _parents(name, s):
    """The oracle's min-key parent edge of every vertex for source s (-1: s itself)."""
    from oracle.oracle import TIE_MINKEY
    par = _oracle(name).dijkstra(int(s), TIE_MINKEY)[1]
    par.setflags(write=False)
    return par


@functools.lru_cache(maxsize=None)
def _oracle_hops(name, k):
    """Oracle hop rows of the first k sources of the fixture over all vertices."""
    from oracle.oracle import TIE_MINKEY
    g, A = _graph(name)
    h = _oracle(name).source_rows(A[:k], np.arange(g.n, dtype=np.int32), TIE_MINKEY)[3]
    h.setflags(write=False)
    return h


def _self_eid(g, s):
    e = np.flatnonzero((g.src == s) & (g.dst == s))
    return int(e[0]) if len(e) else -1


def oracle_path(name, s, t):
    """(vertices, edge ids) of the oracle's chain s -> t; the [s, s] self entry for t == s."""
    g = _graph(name)[0]
    if s == t:
        return [s, s], [_self_eid(g, s)]
    par = _parents(name, s)
    vs, es, v = [t], [], t
    while v != s:
        e = int(par[v])
        assert e >= 0
        u = int(g.src[e]) if (g.directed or int(g.dst[e]) == v) else int(g.dst[e])
        es.append(e); vs.append(u); v = u
    return vs[::-1], es[::-1]


def split_paths(route, off, vert, edge):
    """[(vertices, edges)] per pair from shd_route_paths' arrays; checks off is consistent."""
    off = np.asarray(off)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == len(vert)
    eoff = route.path_edge_offsets(off)
    nv = np.diff(off)
    assert np.all((nv == 0) | (nv >= 2))
    assert len(edge) == int(off[-1]) - int(np.count_nonzero(nv))
    return [(vert[off[k]:off[k + 1]], edge[eoff[k]:eoff[k] + max(nv[k] - 1, 0)]) for k in range(len(nv))]


def check_chain(name, route, S, T, off, vert, edge):
    """Every returned path of the pairs (S[k], T[k]), T[k] != S[k], is the oracle's chain."""
    g = _graph(name)[0]
    off = np.asarray(off); S = np.asarray(S); T = np.asarray(T)
    nv = np.diff(off)
    assert np.all(nv >= 2)
    eoff = route.path_edge_offsets(off)
    assert np.array_equal(vert[off[:-1]], S) and np.array_equal(vert[off[1:] - 1], T)
    srcs = np.unique(S)
    PE = np.stack([_parents(name, int(s)) for s in srcs])
    row = np.searchsorted(srcs, S)
    h = nv - 1
    pair = np.repeat(np.arange(len(S)), h)                    # the pair of every hop
    q = np.arange(int(h.sum())) - np.repeat(np.cumsum(h) - h, h)  # its position in the path
    tail = vert[off[pair] + q]; head = vert[off[pair] + q + 1]; e = edge[eoff[pair] + q]
    assert np.array_equal(e, PE[row[pair], head])
    other = np.where(g.directed | (g.dst[e] == head), g.src[e], g.dst[e])
    assert np.array_equal(other, tail)
    assert np.all(g.dst[e] == head) if g.directed else np.all((g.src[e] == head) | (g.dst[e] == head))


def _all_pairs(A, n, rng, dup=50):
    S = np.repeat(A, n).astype(np.int32); T = np.tile(np.arange(n, dtype=np.int32), len(A))
    k = rng.permutation(len(S))
    k = np.concatenate([k, rng.choice(k, size=dup)])
    return S[k], T[k]


# -- 3: hop counts ------------------------------------------------------------------------

@pytest.mark.parametrize("name", SMALL)
def test_hop_counts(route, name):
    g, A = _graph(name)
    eng = route.RouteEngine(g)
    hops, mx = eng.hops(A, np.arange(g.n), dispatch=False)
    want = _oracle_hops(name, len(A))
    assert hops.dtype == np.int32 and np.array_equal(hops, want)
    assert np.array_equal(mx, want.max(axis=1))


def test_tie_rule_is_discriminating():
    """ba64_ties: many entries are non-unique and the oracle's two tie rules disagree on the
    hop count of more than 100 of them, so test_hop_counts[ba64_ties] pins the rule."""
    from oracle.oracle import TIE_IGRAPH, TIE_MINKEY
    g, A = _graph("ba64_ties")
    og = _oracle("ba64_ties")
    T = np.arange(g.n, dtype=np.int32)
    a = og.source_rows(A[:40], T, TIE_MINKEY)
    b = og.source_rows(A[:40], T, TIE_IGRAPH)
    assert np.count_nonzero(~a[2]) >= 1000
    assert np.count_nonzero(a[3] != b[3]) >= 100


# -- 4 + 5: paths against the oracle and against rows() -------------------------------------

def _refold(g, s, t, vs, es):
    """(lat, rel) of a path as the reference folds them (topology.c:1407-1523)."""
    vf = g.vertex_packetloss
    rel = 1.0
    if vf is not None and not np.isnan(vf[s]):
        rel = rel * (1.0 - vf[s])
    if s != t and vf is not None and not np.isnan(vf[t]):
        rel = rel * (1.0 - vf[t])
    lat = 0.0
    for e in es:
        lat = lat + float(g.latency[e])
        rel = rel * (1.0 - float(g.packetloss[e]))
    return lat, rel


@pytest.mark.parametrize("name", SMALL)
def test_paths_match_oracle_and_rows(route, name):
    g, A = _graph(name)
    A = A[:16]
    eng = route.RouteEngine(g)
    S, T = _all_pairs(A, g.n, np.random.default_rng(4))
    off, vert, edge = eng.paths(S, T, dispatch=False)
    paths = split_paths(route, off, vert, edge)
    ns = S != T
    sub = np.flatnonzero(ns)
    # the non-self pairs, re-packed, against the oracle's chains
    o2 = np.concatenate([[0], np.cumsum(np.diff(off)[sub])])
    v2 = np.concatenate([paths[k][0] for k in sub]); e2 = np.concatenate([paths[k][1] for k in sub])
    check_chain(name, route, S[sub], T[sub], o2, v2, e2)
    hops = _oracle_hops(name, len(_graph(name)[1]))
    pos = {int(a): i for i, a in enumerate(A)}
    lat, rel, _ = eng.rows(A, np.arange(g.n), dispatch=False)
    vlossy = g.vertex_packetloss is not None and bool(np.any(np.nan_to_num(g.vertex_packetloss) != 0.0))
    assert vlossy == (name == "ba120_vloss")
    for k in range(0, len(S)):
        s, t = int(S[k]), int(T[k])
        vs, es = paths[k]
        assert len(es) == hops[pos[s], t]
        if s == t:
            assert list(vs) == [s, s] and list(es) == [_self_eid(g, s)]
        elif k % 7 == 0:  # literal sequences for a sample (check_chain covered all)
            ov, oe = oracle_path(name, s, t)
            assert list(vs) == ov and list(es) == oe
        # the path is the one the engine's numbers come from
        L, R = _refold(g, s, t, vs, es)
        assert L == lat[pos[s], t], (s, t)
        if vlossy:
            assert abs(R - rel[pos[s], t]) <= 1e-12 * abs(R), (s, t)
        else:
            assert R == rel[pos[s], t], (s, t)


# -- 6: depth -------------------------------------------------------------------------------

def test_ring_depth(route):
    g, A = _graph("ring515")
    n = g.n
    par = _parents("ring515", int(A[0]))
    assert len(oracle_path("ring515", int(A[0]), int((A[0] - 1) % n))[1]) == 514
    eng = route.RouteEngine(g)
    with pytest.raises(route.RouteError) as ei:
        eng.hops(A, np.arange(n), dispatch=False)
    assert ei.value.code == route.ENOEDGE
    hops, mx = ei.value.partial
    want = (np.arange(n)[None, :] - A[:, None]) % n
    want[want == 0] = -1                      # no self-loop: the self entry fails, the rest is written
    assert np.array_equal(hops, want) and np.array_equal(mx, np.full(len(A), 514))
    S = np.repeat(A, n - 1).astype(np.int32)
    T = ((S + np.tile(np.arange(1, n), len(A))) % n).astype(np.int32)
    off, vert, edge = eng.paths(S, T, dispatch=False)
    check_chain("ring515", route, S, T, off, vert, edge)
    assert np.array_equal(np.diff(off) - 1, (T - S) % n)
    k = int(np.argmax(np.diff(off)))
    assert np.array_equal(vert[off[k]:off[k + 1]], (S[k] + np.arange(n)) % n)
    assert par[int(A[0])] < 0
    # the self pair alone: no room taken, SHD_ROUTE_ENOEDGE, the others still extracted
    with pytest.raises(route.RouteError) as ei:
        eng.paths([A[0], A[0], A[1]], [A[0] + 2, A[0], A[1] + 1], dispatch=False)
    assert ei.value.code == route.ENOEDGE
    off, vert, edge = ei.value.partial
    assert list(off) == [0, 3, 3, 5]
    assert list(vert) == [A[0], A[0] + 1, A[0] + 2, A[1], A[1] + 1] and list(edge) == [A[0], A[0] + 1, A[1]]


# -- 7: hubs and tiles ----------------------------------------------------------------------

def test_hubs_and_tiles(route):
    g, A = _graph("i2000")
    nl = g.src != g.dst
    assert np.bincount(np.concatenate([g.src[nl], g.dst[nl]])).max() > 128  # wider than two waves
    assert g.n % 256 != 0 and g.n % 1024 != 0
    eng = route.RouteEngine(g)
    hops, mx = eng.hops(A, np.arange(g.n), dispatch=False)
    want = _oracle_hops("i2000", len(A))
    assert want.max() >= 10
    assert np.array_equal(hops, want) and np.array_equal(mx, want.max(axis=1))
    rng = np.random.default_rng(7)
    S = rng.choice(A, size=2000).astype(np.int32); T = rng.integers(0, g.n, size=2000).astype(np.int32)
    T = np.where(T == S, (T + 1) % g.n, T).astype(np.int32)
    off, vert, edge = eng.paths(S, T, dispatch=False)
    check_chain("i2000", route, S, T, off, vert, edge)
    for k in range(0, 2000, 40):
        ov, oe = oracle_path("i2000", int(S[k]), int(T[k]))
        assert list(vert[off[k]:off[k + 1]]) == ov


def test_beyond_u16(route):
    """66,000 vertices: vertex ids and hop counters no longer fit u16 (the u32 HBM form of
    the hop counting, whatever rows kernel the context selects)."""
    g, A = _graph("ring66k")
    eng = route.RouteEngine(g)
    tg = np.arange(65000, g.n, dtype=np.int32)
    with pytest.raises(route.RouteError) as ei:   # no self-loops: 65999's own entry fails
        eng.hops(A, tg, dispatch=False)
    hops, mx = ei.value.partial
    from oracle.oracle import TIE_MINKEY
    og = _oracle("ring66k")
    assert ei.value.code == route.ENOEDGE
    want0 = og.source_rows([int(A[0])], tg, TIE_MINKEY)[3][0]
    want1 = og.source_rows([int(A[1])], tg[:-1], TIE_MINKEY)[3][0]
    assert np.array_equal(hops[0], want0) and np.array_equal(hops[1, :-1], want1) and hops[1, -1] == -1
    assert mx[0] == want0.max() and mx[1] == want1.max()
    rng = np.random.default_rng(66)
    S = rng.choice(A, size=400).astype(np.int32); T = rng.integers(0, g.n, size=400).astype(np.int32)
    T = np.where(T == S, (T + 1) % g.n, T).astype(np.int32)
    off, vert, edge = eng.paths(S, T, dispatch=False)
    check_chain("ring66k", route, S, T, off, vert, edge)
    assert vert.max() > 65535


# -- 8: fallbacks on small shapes --------------------------------------------------------------

def _hops_and_paths(route, name, k=16):
    g, A = _graph(name)
    A = A[:k]
    eng = route.RouteEngine(g)
    tg = np.arange(g.n)
    S, T = _all_pairs(A, g.n, np.random.default_rng(8), dup=10)
    keep = S != T
    S, T = S[keep], T[keep]
    try:
        hops, mx = eng.hops(A, tg, dispatch=False)
    except route.RouteError as err:  # the ring's self entries
        assert err.code == route.ENOEDGE
        hops, mx = err.partial
    return (hops, mx) + tuple(eng.paths(S, T, dispatch=False)), eng.info


@pytest.mark.parametrize("name", ["ba64_ties", "ring515"])
@pytest.mark.parametrize("var", ["SHD_ROUTE_HOPS_LDS", "SHD_ROUTE_HOPS_SCRATCH"])
def test_fallbacks(route, monkeypatch, name, var):
    """The HBM form of the hop counting, and several chunks of sources (the scratch of four
    sources of shd_route_paths: 16 sources take four chunks there and in shd_route_hops),
    give what the default run gives."""
    base, _ = _hops_and_paths(route, name)
    n = _graph(name)[0].n
    monkeypatch.setenv(var, "0" if var.endswith("LDS") else str(4 * 16 * n))
    got, _ = _hops_and_paths(route, name)
    assert base[0].max() == (514 if name == "ring515" else _oracle_hops(name, 16).max())
    for a, b in zip(base, got):
        assert np.array_equal(a, b)


def test_paths_in_chunks_with_failed_pairs(route, monkeypatch):
    """ba60_holes, 16 sources, scratch for four sources per chunk: shd_route_paths takes the
    sorted sources in four chunks.  The self pairs of the odd sources of the two middle chunks
    fail (no self-loop) and take no room, so every path behind them is staged and copied out
    at an offset that the chunks before it moved.  Offsets, vertices, edges and the code equal
    the run in one chunk."""
    g, _ = _graph("ba60_holes")
    A = np.arange(2, 50, 3, dtype=np.int32)              # sorted: chunks of A[0:4] .. A[12:16]
    rng = np.random.default_rng(16)
    S, T = _all_pairs(A, g.n, rng, dup=10)
    keep = S != T
    holes = A[4:12][A[4:12] % 2 == 1]                    # in neither the first nor the last chunk
    loops = A[A % 2 == 0]
    assert len(holes) == 4 and all(_self_eid(g, int(v)) < 0 for v in holes)
    assert all(_self_eid(g, int(v)) >= 0 for v in loops)
    S = np.concatenate([S[keep], holes, loops]); T = np.concatenate([T[keep], holes, loops])
    k = rng.permutation(len(S))
    S, T = S[k], T[k]

    def paths():
        with pytest.raises(route.RouteError) as err:
            route.RouteEngine(g).paths(S, T, dispatch=False)
        return err.value.code, err.value.partial

    code0, base = paths()
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 16 * g.n))
    code1, got = paths()
    assert code0 == code1 == route.ENOEDGE
    for a, b in zip(base, got):
        assert np.array_equal(a, b)
    off, vert, edge = got
    failed = np.isin(S, holes) & (S == T)
    assert np.array_equal(np.diff(off) == 0, failed)
    sp = split_paths(route, off, vert, edge)
    for q in np.flatnonzero(~failed):
        assert sp[q][0][0] == S[q] and sp[q][0][-1] == T[q]
    ok = ~failed & (S != T)
    o2 = np.concatenate([[0], np.cumsum(np.diff(off)[ok])])
    v2 = np.concatenate([sp[q][0] for q in np.flatnonzero(ok)]); e2 = np.concatenate([sp[q][1] for q in np.flatnonzero(ok)])
    check_chain("ba60_holes", route, S[ok], T[ok], o2, v2, e2)


def test_kernel_kf_same_paths(route, monkeypatch):
    base, info0 = _hops_and_paths(route, "ba60")
    monkeypatch.setenv("SHD_ROUTE_KERNEL", "kf")
    got, info1 = _hops_and_paths(route, "ba60")
    assert info1["kernel"] == 5 and info0["kernel"] != 5
    for a, b in zip(base, got):
        assert np.array_equal(a, b)


# -- 9: dispatch ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["k24", "ba80_prefer"])
def test_dispatch(route, name):
    g, A = _graph(name)
    og = _oracle(name)
    eng = route.RouteEngine(g)
    assert bool(eng.info["is_complete"]) == (name == "k24")
    A = A[:16]
    tg = np.arange(g.n)
    hops, _ = eng.hops(A, tg, dispatch=True)
    tree, _ = eng.hops(A, tg, dispatch=False)
    S = np.repeat(A, g.n).astype(np.int32); T = np.tile(tg, len(A)).astype(np.int32)
    paths = split_paths(route, *eng.paths(S, T, dispatch=True))
    tpaths = split_paths(route, *eng.paths(S, T, dispatch=False))
    dlat = eng.direct(A, tg)[0] if name == "k24" else None
    ndirect = 0
    for k, (s, t) in enumerate(zip(S.tolist(), T.tolist())):
        i = k // g.n
        vs, es = paths[k]
        eid = og.get_eid(s, t)
        if s == t:
            assert list(vs) == [s, s] and list(es) == [_self_eid(g, s)] and hops[i, t] == 1
        elif eid >= 0:  # complete, or prefer-direct and adjacent: the one-hop direct path
            ndirect += 1
            assert list(vs) == [s, t] and list(es) == [eid] and hops[i, t] == 1
            assert g.latency[eid] == og.direct(s, t)[0]
            if dlat is not None:
                assert dlat[i, t] == g.latency[eid]
        else:
            assert name == "ba80_prefer"
            assert np.array_equal(vs, tpaths[k][0]) and np.array_equal(es, tpaths[k][1])
            assert hops[i, t] == tree[i, t] and len(es) == tree[i, t]
    if name == "k24":
        assert ndirect == len(A) * (g.n - 1)
    else:
        assert 0 < ndirect < len(A) * (g.n - 1)


# -- 10: multigraph -----------------------------------------------------------------------------

def test_multigraph(route):
    g, A = _graph("ba60_multi")
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1
    A = A[:16]
    S, T = _all_pairs(A, g.n, np.random.default_rng(10), dup=0)
    keep = S != T
    S, T = S[keep], T[keep]
    lat = eng.rows(A, np.arange(g.n), dispatch=False)[0]
    pos = {int(a): i for i, a in enumerate(A)}
    used_parallel = 0
    for (vs, es), s, t in zip(split_paths(route, *eng.paths(S, T, dispatch=False)), S.tolist(), T.tolist()):
        assert vs[0] == s and vs[-1] == t and len(set(vs.tolist())) == len(vs)
        L = 0.0
        for q, e in enumerate(es.tolist()):
            assert {int(g.src[e]), int(g.dst[e])} == {int(vs[q]), int(vs[q + 1])}
            L = L + float(g.latency[e])
            used_parallel += e >= g.m - 10
        assert L == lat[pos[s], t]
    assert used_parallel > 0  # some added edge is the lighter of its pair and gets used


# -- 11: sizing -----------------------------------------------------------------------------------

def test_sizing_call(route):
    g, A = _graph("ba60")
    eng = route.RouteEngine(g)
    L = route.load_library()
    S = np.array([A[0], A[3], A[0]], np.int32); T = np.array([A[7], A[9], A[0]], np.int32)
    off, vert, edge = eng.paths(S, T, dispatch=False)
    need = int(off[-1])
    p = lambda a: C.c_void_p(a.ctypes.data)
    off2 = np.full(4, -7, np.int64)
    v2 = np.full(need, -7, np.int32); e2 = np.full(need, -7, np.int32)
    rc = L.shd_route_paths(eng._h, p(S), p(T), 3, 0, p(off2), p(v2), p(e2), need - 1)
    assert rc == route.EINVAL
    assert np.array_equal(off2, off) and np.all(v2 == -7) and np.all(e2 == -7)
    rc = L.shd_route_paths(eng._h, p(S), p(T), 3, 0, p(off2), p(v2), p(e2), need)
    assert rc == route.OK and np.array_equal(v2, vert) and np.array_equal(e2[: len(edge)], edge)
    off3 = np.full(1, -7, np.int64)
    assert L.shd_route_paths(eng._h, None, None, 0, 0, p(off3), None, None, 0) == route.OK and off3[0] == 0
    o0, ve0, ed0 = eng.paths([], [])
    assert list(o0) == [0] and len(ve0) == 0 and len(ed0) == 0


# -- 12: front end ------------------------------------------------------------------------------------

def _ref_line(g, ids, a, b, vs, es, lat, rel):
    nm = (lambda v: ids[v]) if ids else (lambda v: "%d" % v)
    sep = "-->" if g.directed else "<-->"
    s = "shortest path %s%s%s (%i%s%i) is %f ms with %f loss, path: %s" % (nm(a), sep, nm(b), a, sep, b, lat, 1 - rel,
                                                                        nm(a))
    for q, e in enumerate(es):
        s += "%s[%f,%f]-->%s" % ("--" if g.directed else "<--", g.latency[e], 1.0 - (1.0 - g.packetloss[e]),
                                  nm(int(vs[q + 1])))
    return s


def _dump_paths_text(topo, t, path):
    libc = C.CDLL(None)
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    fp = libc.fopen(str(path).encode(), b"w")
    assert topo.load_library().shd_topology_dump_paths(t._h, fp) == 0
    libc.fclose(fp)
    return open(path).read()


@pytest.mark.parametrize("name", ["ba80_prefer", "dir40", "ba60_graphml"])
def test_front_end_routes(topo, tmp_path, name):
    gname = "ba60" if name == "ba60_graphml" else name
    g, A = _graph(gname)
    og = _oracle(gname)
    ids = None
    if name == "ba60_graphml":
        pth = tmp_path / "ba60.graphml.xml"
        to_graphml(g, str(pth))
        t = topo.Topology.new(str(pth))
        ids = [g.vertex_id(v) for v in range(g.n)]
    else:
        t = topo.Topology.from_graph(g)
    A = np.sort(A)
    t.attach_all(A)
    for a, b in ((A[0], A[5]), (A[2], A[2]), (A[9], A[1])):
        for _ in range(3):
            t.increment_path_packet_counter(int(a), int(b))
    sample = [int(x) for x in A[:: max(1, len(A) // 9)]]
    snap = lambda: (t.table(sample), [t.packet_count(a, b) for a in sample for b in sample], t.min_path_latency(),
                    [t.is_direct(a, b) for a in sample for b in sample],
                    _dump_paths_text(topo, t, tmp_path / "paths.txt"))
    before = snap()

    def expect(a, b):  # the oracle route of the stored pair a <= b
        if a == b:
            return [a, a], [_self_eid(g, a)]
        if t.is_direct(a, b) == 1:
            return [a, b], [og.get_eid(a, b)]
        return oracle_path(gname, a, b)

    want = []
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            if t.is_direct(a, b) == 1:
                continue
            vs, es = expect(a, b)
            want.append(_ref_line(g, ids, a, b, vs, es, t.get_latency(a, b), t.get_reliability(a, b)))
    out = tmp_path / "routes.txt"
    t.dump_routes(str(out))
    got = out.read_text().splitlines()
    assert len(got) == len(want) and got == want
    if name == "ba80_prefer":
        assert 0 < len(want) < len(A) * (len(A) + 1) // 2
    # get_path / format_path on a sample of pairs, both argument orders, self pairs included
    rng = np.random.default_rng(12)
    pairs = [(int(a), int(b)) for a, b in zip(rng.choice(A, 60), rng.choice(A, 60))] + [(sample[1], sample[1])]
    nd = 0
    for s, d in pairs:
        a, b = min(s, d), max(s, d)
        vs, es = expect(a, b)
        gv, ge = t.get_path(s, d)
        assert list(gv) == list(vs) and list(ge) == list(es), (s, d)
        line = t.format_path(s, d)
        assert line == _ref_line(g, ids, a, b, vs, es, t.get_latency(a, b), t.get_reliability(a, b))
        if t.is_direct(a, b) != 1:
            nd += 1
            assert line in got
    assert nd > 0 or name == "ba80_prefer"
    assert t.get_path(int(A[0]), -1) is None and t.format_path(g.n, int(A[0])) is None
    after = snap()
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
    assert before[1:] == after[1:]
    t.close()
