"""GPU: link loads -- shd_route_loads / shd_route_pair_loads / shd_route_loads_async and the
front end's shd_topology_link_loads -- against the oracle's min-key parents.

The expected loads are accumulated in numpy from OracleGraph.dijkstra(s, TIE_MINKEY)'s parent
edges: the row's weights go onto their targets, the vertices are taken in decreasing distance
(latencies are positive, so every child comes before its parent) and each non-zero sum is
added to its parent edge and to its parent; what a vertex received from below is its transit.
Self entries, direct-dispatched entries and failed entries follow include/shd_route.h.  All
comparisons are array_equal on uint64.  Fixtures are those of tests/test_hops_gpu.py."""
import functools

import numpy as np
import pytest

from shadow_amd.graph import Graph
from tests import test_hops_gpu as hg
from tests.test_hops_gpu import SMALL, _self_eid

pytestmark = pytest.mark.gpu
BIG = np.uint64(2 ** 40 + 3)


@functools.lru_cache(maxsize=None)
def _graph(name):
    """The fixtures of tests/test_hops_gpu.py, and ba60_holes: ba60 (a self-loop at every
    vertex) without the self-loops of the odd vertices, every vertex attached."""
    if name != "ba60_holes":
        return hg._graph(name)
    g, A = hg._graph("ba60")
    keep = ~((g.src == g.dst) & (g.src % 2 == 1))
    assert 0 < np.count_nonzero(~keep) < np.count_nonzero(g.src == g.dst)
    return Graph(n=g.n, src=g.src[keep], dst=g.dst[keep], latency=g.latency[keep], packetloss=g.packetloss[keep],
                 vertex_packetloss=g.vertex_packetloss, name=name), A


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import OracleGraph
    return OracleGraph(_graph(name)[0])


def oracle_path(name, s, t):
    """(vertices, edge ids) of the oracle's chain s -> t, s != t."""
    _, par, pv, _ = _tree(name, s)
    vs, es, v = [t], [], t
    while v != s:
        es.append(int(par[v])); v = int(pv[v]); vs.append(v)
    return vs[::-1], es[::-1]


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


@functools.lru_cache(maxsize=None)
def _tree(name, s):
    """(dist, parent edge, parent vertex, vertices in decreasing distance) of source s."""
    from oracle.oracle import TIE_MINKEY
    g = _graph(name)[0]
    dist, par = _oracle(name).dijkstra(int(s), TIE_MINKEY)
    e = np.maximum(par, 0)
    V = np.arange(g.n)
    pv = np.where(g.directed | (g.dst[e] == V), g.src[e], g.dst[e])
    pv = np.where(par >= 0, pv, -1)
    reach = np.flatnonzero(par >= 0)             # an unreached vertex has distance -1 and no parent
    order = reach[np.argsort(-dist[reach], kind="stable")]
    for a in (dist, par, pv, order):
        a.setflags(write=False)
    return dist, par, pv, order


@functools.lru_cache(maxsize=None)
def _mode(name, dispatch):
    g = _graph(name)[0]
    if not dispatch:
        return 0
    return 2 if _oracle(name).is_complete() else 1 if g.prefer_direct else 0


@functools.lru_cache(maxsize=None)
def _direct_eid(name):
    """{(s, t): the lowest edge id joining s -> t} of a small fixture."""
    g = _graph(name)[0]
    d = {}
    for e in range(len(g.src) - 1, -1, -1):
        a, b = int(g.src[e]), int(g.dst[e])
        if a == b:
            continue
        d[(a, b)] = e
        if not g.directed:
            d[(b, a)] = e
    return d


def ref_loads(route, name, S, T, W, dispatch):
    """(edge_load, transit, unrouted, codes raised, sum of weight x hops) of the block S x T
    with weights W (None = 1 per entry)."""
    g = _graph(name)[0]
    mode = _mode(name, dispatch)
    S = np.asarray(S); T = np.asarray(T)
    el = np.zeros(len(g.src), np.uint64); tr = np.zeros(g.n, np.uint64)
    un = 0; codes = set(); wh = 0
    deid = _direct_eid(name) if mode else {}
    for i, s in enumerate(S.tolist()):
        w = np.ones(len(T), np.uint64) if W is None else np.asarray(W[i], np.uint64)
        tree = np.ones(len(T), bool)
        for j in np.flatnonzero(T == s).tolist():      # the self entries
            tree[j] = False
            e = _self_eid(g, s)
            if e < 0:
                codes.add(route.ENOEDGE); un += int(w[j])
            else:
                el[e] += w[j]; wh += int(w[j])
        if mode:                                          # direct-dispatched entries
            for j in np.flatnonzero(tree).tolist():
                e = deid.get((s, int(T[j])), -1)
                if e >= 0:
                    tree[j] = False
                    el[e] += w[j]; wh += int(w[j])
                elif mode == 2:
                    tree[j] = False
                    codes.add(route.ENOEDGE); un += int(w[j])
        if mode == 2:
            continue
        dist, par, pv, order = _tree(name, s)
        dead = tree & (dist[T] < 0)
        if dead.any():
            codes.add(route.EUNREACH); un += int(w[dead].sum(dtype=np.uint64))
            tree &= ~dead
        acc = np.zeros(g.n, np.uint64)
        np.add.at(acc, T[tree], w[tree])
        own = acc.copy()
        for v in order.tolist():
            a = acc[v]
            if a:
                el[par[v]] += a
                wh += int(a)
                if pv[v] != s:
                    acc[pv[v]] += a
        tr += acc - own
    return el, tr, un, codes, wh


def run(route, call, *args, **kw):
    """(edge_load, transit, unrouted, code) of a loads call, failed entries or not."""
    try:
        return tuple(call(*args, **kw)) + (route.OK,)
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return tuple(err.partial) + (err.code,)


def hops_weight(route, eng, S, T, W, dispatch):
    """Sum of weight x shd_route_hops over the entries that did not fail."""
    try:
        h = eng.hops(S, T, dispatch=dispatch)[0]
    except route.RouteError as err:
        h = err.partial[0]
    w = np.ones(h.shape, np.uint64) if W is None else np.asarray(W, np.uint64)
    return int((w[h > 0] * h[h > 0].astype(np.uint64)).sum(dtype=np.uint64))     # modulo 2^64, as the loads


def weights(rng, S, T):
    """Mostly zero, small values, one above 2^32 per row, one whole row of zeros, and the
    self entry of every second row weighted (so a missing self-loop shows in unrouted)."""
    ns, nt = len(S), len(T)
    W = (rng.integers(0, 5, size=(ns, nt)) * (rng.random((ns, nt)) < 0.3)).astype(np.uint64)
    W[np.arange(ns), rng.integers(0, nt, size=ns)] = BIG
    for i in range(0, ns, 2):
        W[i, np.flatnonzero(np.asarray(T) == S[i])] = 3 + i
    if ns > 1:
        W[ns // 2, :] = 0
    return W


def check(route, name, eng, S, T, W, dispatch, got=None):
    """The block's loads against the reference and against shd_route_hops."""
    el, tr, un, codes, wh = ref_loads(route, name, S, T, W, dispatch)
    if got is None:
        got = run(route, eng.loads, S, T, W, dispatch=dispatch)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
    assert np.array_equal(got[0], el)
    assert np.array_equal(got[1], tr)
    assert got[2] == un
    assert (got[3] in codes) if codes else got[3] == route.OK
    assert int(el.sum(dtype=np.uint64)) == wh % 2 ** 64 == hops_weight(route, eng, S, T, W, dispatch) % 2 ** 64
    return got


# -- every small golden graph -----------------------------------------------------------------

@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", SMALL + ["ba60_holes"])
def test_small_graphs(route, name, dispatch, weighted):
    g, A = _graph(name)
    S = np.arange(g.n, dtype=np.int32) if g.n <= 64 else A   # every vertex a source on 60-64 vertices
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    W = weights(np.random.default_rng(g.n), S, T) if weighted else None
    got = check(route, name, eng, S, T, W, dispatch)
    loops = sum(_self_eid(g, int(s)) >= 0 for s in S)
    assert (loops < len(S)) == (name == "ba60_holes")
    if loops < len(S):                      # self entries without a self-loop: the code and unrouted
        assert got[3] == route.ENOEDGE and 0 < loops
        if not weighted:
            assert got[2] == len(S) - loops
    else:
        assert got[3] == route.OK and got[2] == 0
    if name == "k24" and dispatch:          # a complete graph under dispatch: direct edges only
        assert not got[1].any()
    else:
        assert got[1].any()
    if name == "ba80_prefer":               # prefer-direct peels the adjacent pairs off the tree
        other = run(route, eng.loads, S, T, W, dispatch=not dispatch)
        assert not np.array_equal(other[0], got[0])


# -- depth, multigraph, tiles, chunks, slots, u32 ------------------------------------------------

def test_ring_levels(route, monkeypatch):
    """514 levels of one vertex each; the LDS and the HBM form give the same."""
    g, A = _graph("ring515")
    T = np.arange(g.n, dtype=np.int32)
    W = weights(np.random.default_rng(515), A, T)
    eng = route.RouteEngine(g)
    got = check(route, "ring515", eng, A, T, W, False)
    assert got[3] == route.ENOEDGE          # no self-loops
    unit = check(route, "ring515", eng, A, T, None, False)
    assert unit[2] == len(A)                # the 16 self entries
    monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    hbm = run(route, route.RouteEngine(g).loads, A, T, W, dispatch=False)
    for a, b in zip(got, hbm):
        assert np.array_equal(a, b)


def test_lds_and_hbm_forms_agree(route, monkeypatch):
    g, A = _graph("ba60")
    S = np.arange(g.n, dtype=np.int32)
    W = weights(np.random.default_rng(6), S, S)
    base = check(route, "ba60", route.RouteEngine(g), S, S, W, False)
    monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    hbm = run(route, route.RouteEngine(g).loads, S, S, W, dispatch=False)
    for a, b in zip(base, hbm):
        assert np.array_equal(a, b)


def test_multigraph(route):
    """The load lands on the lowest tight parallel edge (the oracle's parent edge)."""
    g, A = _graph("ba60_multi")
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1
    S = A[:16]; T = np.arange(g.n, dtype=np.int32)
    got = check(route, "ba60_multi", eng, S, T, weights(np.random.default_rng(10), S, T), False)
    m0 = len(g.src) - 10
    assert got[0][m0:].any()                # some added parallel edge is the lighter one and carries load
    pairs = {}
    for e in range(len(g.src)):
        pairs.setdefault(frozenset((int(g.src[e]), int(g.dst[e]))), []).append(e)
    assert any(len(v) > 1 and sum(got[0][e] > 0 for e in v) == 1 for v in pairs.values())


def test_tiles_hubs_and_chunks(route, monkeypatch):
    """i2000: more vertices than threads, hub in-lists; then the same with scratch for three
    sources per chunk (8 sources: three chunks, which must add and not overwrite)."""
    g, A = _graph("i2000")
    T = np.arange(g.n, dtype=np.int32)
    W = weights(np.random.default_rng(2000), A, T)
    base = check(route, "i2000", route.RouteEngine(g), A, T, W, False)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    got = run(route, route.RouteEngine(g).loads, A, T, W, dispatch=False)
    for a, b in zip(base, got):
        assert np.array_equal(a, b)


def test_slot_takes_several_sources(route, monkeypatch):
    """i2000, 40 sources, the HBM form.  A slot's state is 22 bytes per vertex (44,016 bytes)
    and the slots take a quarter of the scratch budget, 16 at the least: with a budget of
    2,000,000 bytes (62 sources per chunk: one chunk) there are 16 slots, so every workgroup
    takes two or three sources and must find nothing left of the one before."""
    g, _ = _graph("i2000")
    S = (np.arange(40, dtype=np.int32) * 49)
    T = np.arange(g.n, dtype=np.int32)
    W = weights(np.random.default_rng(40), S, T)
    monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", "2000000")
    check(route, "i2000", route.RouteEngine(g), S, T, W, False)


def test_beyond_u16(route):
    """66,000 vertices: the HBM form with u32 order entries."""
    g, A = _graph("ring66k")
    T = np.arange(g.n, dtype=np.int32)
    rng = np.random.default_rng(66)
    W = (rng.integers(0, 5, size=(2, g.n)) * (rng.random((2, g.n)) < 0.3)).astype(np.uint64)
    W[0, 65990] = BIG; W[1, 7] = BIG; W[1, A[1]] = 5
    el, tr, un, codes, wh = ref_loads(route, "ring66k", A, T, W, False)
    got = run(route, route.RouteEngine(g).loads, A, T, W, dispatch=False)
    assert np.array_equal(got[0], el) and np.array_equal(got[1], tr)
    assert got[2] == un == 5 + int(W[0, A[0]]) and got[3] == route.ENOEDGE
    assert int(el.sum(dtype=np.uint64)) == wh % 2 ** 64 and np.flatnonzero(tr).max() > 65535


# -- cross-checks within the library ------------------------------------------------------------------

def test_matches_explicit_routes(route):
    """ba60: the loads rebuilt by adding each pair's weight along its shd_route_paths edges."""
    g, _ = _graph("ba60")
    eng = route.RouteEngine(g)
    S = np.arange(g.n, dtype=np.int32)
    W = weights(np.random.default_rng(61), S, S)
    got = run(route, eng.loads, S, S, W, dispatch=False)
    ps = np.repeat(S, g.n); pt = np.tile(S, g.n)
    try:
        off, vert, edge = eng.paths(ps, pt, dispatch=False)
    except route.RouteError as err:
        off, vert, edge = err.partial
    eoff = route.path_edge_offsets(off)
    el = np.zeros(len(g.src), np.uint64); tr = np.zeros(g.n, np.uint64); un = 0
    for k, w in enumerate(W.reshape(-1)):
        nv = int(off[k + 1] - off[k])
        if nv == 0:
            un += int(w)
            continue
        np.add.at(el, edge[eoff[k]:eoff[k] + nv - 1], w)
        np.add.at(tr, vert[off[k] + 1:off[k + 1] - 1], w)
    assert np.array_equal(got[0], el) and np.array_equal(got[1], tr) and got[2] == un


@pytest.mark.parametrize("name,dispatch", [("ba60", False), ("ba80_prefer", True), ("k24", True)])
def test_sparse_equals_dense(route, name, dispatch):
    g, A = _graph(name)
    eng = route.RouteEngine(g)
    S = A[:12]; T = np.arange(g.n, dtype=np.int32)
    rng = np.random.default_rng(12)
    W = weights(rng, S, T)
    dense = run(route, eng.loads, S, T, W, dispatch=dispatch)
    # every entry as a pair, some split into two pairs of half the weight, all shuffled
    ps = np.repeat(S, g.n); pt = np.tile(T, len(S)); pw = W.reshape(-1).copy()
    dup = rng.choice(len(ps), size=100, replace=False)
    half = pw[dup] // np.uint64(2)
    pw[dup] -= half
    ps = np.concatenate([ps, ps[dup]]); pt = np.concatenate([pt, pt[dup]]); pw = np.concatenate([pw, half])
    k = rng.permutation(len(ps))
    sparse = run(route, eng.pair_loads, ps[k], pt[k], pw[k], dispatch=dispatch)
    for a, b in zip(dense, sparse):
        assert np.array_equal(a, b)
    # unit weights: how many of the listed pairs route over each link
    unit = run(route, eng.pair_loads, ps[k], pt[k], None, dispatch=dispatch)
    cnt = np.ones((len(S), g.n), np.uint64)
    np.add.at(cnt.reshape(-1), dup, np.uint64(1))
    want = run(route, eng.loads, S, T, cnt, dispatch=dispatch)
    for a, b in zip(unit, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("weighted", [True, False])
def test_pair_loads_in_chunks(route, monkeypatch, weighted):
    """ba60, the shuffled and split pairs of test_sparse_equals_dense over 12 sources, with scratch
    for three sources per chunk: the sparse lists run in four chunks, whose offsets index the one
    target list and the one weight list of the whole call.  Edge loads, transit, unrouted and the
    code equal the run in one chunk and the dense loads of the same block."""
    g, A = _graph("ba60")
    S = A[:12]; T = np.arange(g.n, dtype=np.int32)
    assert len(np.unique(S)) == 12
    rng = np.random.default_rng(12)
    W = weights(rng, S, T)
    ps = np.repeat(S, g.n); pt = np.tile(T, len(S)); pw = W.reshape(-1).copy()
    dup = rng.choice(len(ps), size=100, replace=False)
    half = pw[dup] // np.uint64(2)
    pw[dup] -= half
    ps = np.concatenate([ps, ps[dup]]); pt = np.concatenate([pt, pt[dup]]); pw = np.concatenate([pw, half])
    k = rng.permutation(len(ps))
    if not weighted:                        # unit weights: how many of the listed pairs route over each link
        W = np.ones((len(S), g.n), np.uint64)
        np.add.at(W.reshape(-1), dup, np.uint64(1))
    pw = pw[k] if weighted else None
    dense = run(route, route.RouteEngine(g).loads, S, T, W, dispatch=False)
    whole = run(route, route.RouteEngine(g).pair_loads, ps[k], pt[k], pw, dispatch=False)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    got = run(route, route.RouteEngine(g).pair_loads, ps[k], pt[k], pw, dispatch=False)
    assert got[0].any() and got[1].any()
    for a, b, c in zip(got, whole, dense):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_add_flag(route):
    g, A = _graph("ba60")
    eng = route.RouteEngine(g)
    S = A[:8]; T = np.arange(g.n, dtype=np.int32)
    W = weights(np.random.default_rng(3), S, T)
    one = run(route, eng.loads, S, T, W, dispatch=False)
    out = (np.full(len(g.src), 9, np.uint64), np.full(g.n, 9, np.uint64), np.full(1, 9, np.uint64))
    again = run(route, eng.loads, S, T, W, dispatch=False, out=out)      # no flag: overwrites
    assert np.array_equal(again[0], one[0]) and np.array_equal(again[1], one[1]) and again[2] == one[2]
    twice = run(route, eng.loads, S, T, W, dispatch=False, out=out, add=True)
    assert twice[0] is out[0]
    assert np.array_equal(twice[0], one[0] * np.uint64(2)) and np.array_equal(twice[1], one[1] * np.uint64(2))
    assert twice[2] == 2 * one[2]
    ps = np.repeat(S, g.n); pt = np.tile(T, len(S))
    thrice = run(route, eng.pair_loads, ps, pt, W.reshape(-1), dispatch=False, out=out, add=True)
    assert np.array_equal(thrice[0], one[0] * np.uint64(3)) and np.array_equal(thrice[1], one[1] * np.uint64(3))
    back = run(route, eng.pair_loads, ps, pt, W.reshape(-1), dispatch=False, out=out)
    assert np.array_equal(back[0], one[0]) and back[2] == one[2]


def test_empty_and_invalid(route):
    g, A = _graph("ba60")
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    dirty = lambda: (np.full(len(g.src), 9, np.uint64), np.full(g.n, 9, np.uint64), np.full(1, 9, np.uint64))
    for S2, T2 in (([], T), (A[:4], [])):
        el, tr, un = eng.loads(S2, T2, None, dispatch=False, out=dirty())
        assert not el.any() and not tr.any() and un == 0
    el, tr, un = eng.pair_loads([], [], None, out=dirty())
    assert not el.any() and not tr.any() and un == 0
    for bad in (-1, g.n):
        for call, args in ((eng.loads, ([A[0], bad], T)), (eng.loads, (A[:2], [0, bad])),
                           (eng.pair_loads, ([A[0], bad], [1, 2])), (eng.pair_loads, ([A[0], A[1]], [1, bad]))):
            with pytest.raises(route.RouteError) as ei:
                call(*args)
            assert ei.value.code == route.EINVAL


def test_async_device_pointers(route):
    """shd_route_loads_async: a row stride above nt, repeated targets, NULL outputs, the ADD
    flag, and an out-of-range target reported by the next sync."""
    import torch
    g, A = _graph("ba64_ties")
    eng = route.RouteEngine(g)
    dev = torch.device("cuda:0")
    S = A[:10].astype(np.int32)
    T = np.concatenate([np.arange(g.n), [5, 5, 17]]).astype(np.int32)
    nt, ld = len(T), len(T) + 7
    W = weights(np.random.default_rng(64), S, T)
    Wp = np.full((len(S), ld), 77, np.uint64)
    Wp[:, :nt] = W
    el, tr, un, codes, _ = ref_loads(route, "ba64_ties", S, T, W, False)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    ds, dt, dw = d(S), d(T), d(Wp)
    de = torch.full((len(g.src),), 9, dtype=torch.int64, device=dev)
    dtr = torch.full((g.n,), 9, dtype=torch.int64, device=dev)
    du = torch.full((1,), 9, dtype=torch.int64, device=dev)

    def sync():
        try:
            eng.sync()
            return route.OK
        except route.RouteError as err:
            return err.code

    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    eng.loads_async(ds, dt, dw, de, dtr, du, dispatch=False, ld=ld)
    code = sync()
    assert (code in codes) if codes else code == route.OK
    assert np.array_equal(u64(de), el) and np.array_equal(u64(dtr), tr) and int(u64(du)[0]) == un
    eng.loads_async(ds, dt, dw, de, None, None, dispatch=False, ld=ld, add=True)
    sync()
    assert np.array_equal(u64(de), el * np.uint64(2)) and np.array_equal(u64(dtr), tr)
    e1, t1, u1, c1, _ = ref_loads(route, "ba64_ties", S, T, None, False)
    eng.loads_async(ds, dt, None, None, dtr, du, dispatch=False)
    sync()
    assert np.array_equal(u64(dtr), t1) and int(u64(du)[0]) == u1 and np.array_equal(u64(de), el * np.uint64(2))
    t0 = int(np.setdiff1d(np.arange(g.n), S)[0])
    eng.loads_async(ds, d(np.array([t0, g.n], np.int32)), None, de, dtr, du, dispatch=False)
    assert sync() == route.EINVAL


# -- front end ----------------------------------------------------------------------------------------------

def _dump_text(t, fn, path):
    fn(str(path))
    return open(path).read()


@pytest.mark.parametrize("name", ["ba100_attached", "ba80_prefer", "k24", "ba60_holes", "dir40"])
def test_front_end_link_loads(topo, tmp_path, name):
    """Counters on a few hundred random attached pairs, both lookup directions, one pair past
    2^32: bulk-added to just below the u32 wrap, then single increments through the wrap (the
    increment's own spill path; 2^32 single increments are 40 s of atomic adds alone, in a C
    loop as much as from here).  The odd
    vertices of ba60_holes have no self-loop: their self pairs are stored as the path to self
    and count as unrouted."""
    g, A = _graph(name)
    og = _oracle(name)
    t = topo.Topology.from_graph(g)
    A = np.sort(A)
    t.attach_all(A)
    m = len(g.src)
    assert t.edge_count() == m
    z = t.link_loads()
    assert len(z[0]) == m and len(z[1]) == g.n and not z[0].any() and not z[1].any() and z[2] == 0  # before the fill
    assert t.get_latency(int(A[0]), int(A[1])) >= 0
    z = t.link_loads()
    assert not z[0].any() and not z[1].any() and z[2] == 0
    rng = np.random.default_rng(len(A))
    P = rng.choice(A, size=(300, 2))
    P[:8, 0] = A[:8]
    P[:8, 1] = P[:8, 0]                              # some self pairs, odd vertices among them
    for a, b in P.tolist():
        t.increment_path_packet_counter(a, b)
    for a, b in P[::3].tolist():
        t.increment_path_packet_counter(b, a)
    hot = P[8:][P[8:, 0] != P[8:, 1]][0]
    ha, hb = int(hot[1]), int(hot[0])
    before = t.packet_count(ha, hb)
    t.add_path_packets(ha, hb, 2 ** 32 - 3 - before)
    for _ in range(8):
        t.increment_path_packet_counter(hb, ha)
    assert t.packet_count(ha, hb) == 2 ** 32 + 5
    sample = [int(x) for x in A[:: max(1, len(A) // 9)]]
    snap = lambda: ([t.get_latency(a, b) for a in sample for b in sample],
                    [t.get_reliability(a, b) for a in sample for b in sample],
                    [t.packet_count(a, b) for a in sample for b in sample], t.packet_count(ha, hb))
    was = snap()

    # the numpy accumulation of packet_count over the stored orientation (lower -> higher)
    el = np.zeros(m, np.uint64); tr = np.zeros(g.n, np.uint64); un = 0
    npairs = 0
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            c = t.packet_count(a, b)
            if not c:
                continue
            npairs += 1
            if a == b:
                e = _self_eid(g, a)
                if e < 0:
                    un += c
                else:
                    el[e] += np.uint64(c)
            elif t.is_direct(a, b) == 1:
                el[og.get_eid(a, b)] += np.uint64(c)
            else:
                vs, es = oracle_path(name, a, b)
                np.add.at(el, np.asarray(es), np.uint64(c))
                np.add.at(tr, np.asarray(vs[1:-1], np.int64), np.uint64(c))
    assert npairs > 50
    got = t.link_loads()
    assert np.array_equal(got[0], el) and np.array_equal(got[1], tr) and got[2] == un
    assert el.max() >= 2 ** 32
    assert (un > 0) == (name == "ba60_holes")
    if name == "k24":
        assert not tr.any()
    sep = "-->" if g.directed else "<-->"
    want = ["link %d%s%d (%d%s%d) edge %d is %f ms with %f loss, %d packets"
            % (g.src[e], sep, g.dst[e], g.src[e], sep, g.dst[e], e, g.latency[e], g.packetloss[e], int(el[e]))
            for e in np.flatnonzero(el).tolist()]
    assert _dump_text(t, t.dump_link_loads, tmp_path / "links.txt").splitlines() == want
    assert snap() == was
    t.close()
