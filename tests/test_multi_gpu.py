"""GPU: multigraphs (info.multigraph, SURVEY hazard H3: parallel edges, several self-loops on a
vertex) through every rows kernel that takes them, the hops / paths / loads calls, the dispatch,
plans, the triangle fill and the front end, against tests/multi_ref.py: a plain heap Dijkstra
with the header's tie rule (parent = the tight in-arc with the smallest (dist[u], u, edge id),
direct paths over the lowest edge id of a pair, the diagonal over the lowest self-loop).  The
oracle helper of the other rows tests replays igraph_get_eid per hop and so yields the
reference's H3 numbers, which are no distances; test_multi_graphs.py shows both, and that the
fixtures of tests/multi_graphs.py let the edge id of the tie key decide numbers.

Latency is bit-exact everywhere.  Reliability is bit-exact without vertex loss; on
multi389_vloss it is within REL_TOL, the rule for kernels that multiply f_t last (no walk kernel
runs on a multigraph: select_inrows turns KB, KD, K32, the K2 path attributes and FW off, and
the graphs go to the generic f64 kernel, KF or KFH).
"""
import dataclasses
import re

import numpy as np
import pytest

from tests import multi_graphs as mg
from tests.multi_ref import Ref
from tests.test_contract_gpu import CAN64, Padded, run
from tests.test_range_gpu import REL_TOL, SELECTIONS, dev_rows, host_rows, read_triangle, row_min_of, select

pytestmark = pytest.mark.gpu

KF_TAKES = ("multi389", "multi389_dir", "multi389_frac", "multi389_vloss")   # <= 254 reliabilities
HOP_GRAPHS = ("multi389", "multi389_dir", "multi389_frac")


@pytest.fixture(scope="module")
def route():
    from shadow_amd import route as r
    r.load_library()
    return r


@pytest.fixture(autouse=True)
def close_engines(route, monkeypatch):
    """Every context and pinned buffer a test makes is closed when the test ends, also when it
    fails half-way: none is left for the collector to finalise during a later test."""
    made, bufs = [], []
    real, real_b = route.RouteEngine, route.PinnedBuffer

    def tracked(*a, **k):
        made.append(real(*a, **k))
        return made[-1]

    def buffer(*a, **k):
        bufs.append(real_b(*a, **k))
        return bufs[-1]
    monkeypatch.setattr(route, "RouteEngine", tracked)
    monkeypatch.setattr(route, "PinnedBuffer", buffer)
    for k in ("SHD_ROUTE_HOPS_LDS", "SHD_ROUTE_LOADS_LDS", "SHD_ROUTE_FILL_STAGE", "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)
    yield
    for e in reversed(made):
        e.close()
    for b in reversed(bufs):
        b.close()


# ---- the reference, once per graph ------------------------------------------------------------

_REF = {}


def graph_of(name):
    if name == "multi389_prefer":
        return dataclasses.replace(mg.get("multi389"), prefer_direct=True, name=name)
    if name == "loops_only_simple":
        return mg.without_second_loops(mg.get("loops_only"))
    return mg.get(name)


def reference(name, dispatch=False):
    """g, the Ref, the test's sources S, T = every vertex and the (lat, rel, hops) rows of S;
    read-only."""
    key = (name, dispatch)
    if key not in _REF:
        g = graph_of(name)
        ref = _REF[name, False]["ref"] if (name, False) in _REF else Ref(g)
        S = mg.sources(name) if name in mg.SUITE else np.arange(g.n, dtype=np.int32)
        T = np.arange(g.n, dtype=np.int32)
        lat, rel, hops = ref.rows(S, T, dispatch)
        for a in (lat, rel, hops):
            a.setflags(write=False)
        loops = np.zeros(g.n, bool)
        loops[g.src[g.src == g.dst]] = True
        _REF[key] = dict(g=g, ref=ref, S=S, T=T, lat=lat, rel=rel, hops=hops, loops=loops)
    return _REF[key]


def check_rows(route, ref, lat, rel, mn, code, rows=None, exact=None):
    g = ref["g"]
    rows = slice(None) if rows is None else rows
    el, er = ref["lat"][rows], ref["rel"][rows]
    assert np.array_equal(lat, el, equal_nan=True)
    exact = g.vertex_packetloss is None or not np.any(np.nan_to_num(g.vertex_packetloss) > 0) if exact is None else exact
    if exact:
        assert np.array_equal(rel, er, equal_nan=True)
    else:
        assert np.array_equal(np.isnan(rel), np.isnan(er))
        np.testing.assert_allclose(rel, er, rtol=REL_TOL, atol=0)
    assert np.array_equal(mn, row_min_of(el))
    assert code == (route.ENOEDGE if np.isnan(el).any() else route.OK)


def call(route, fn, *a, **k):
    """A host call that raises on failed entries: (its arrays, its code)."""
    try:
        return fn(*a, **k), route.OK
    except route.RouteError as e:
        assert e.code == route.ENOEDGE, e
        return e.partial, e.code


def expect_kernel(name, sel):
    """info["kernel"] as include/shd_route.h implies it on a multigraph: no integer kernel; KF
    (auto, kf, kfh) up to 254 distinct reliabilities; else the generic f64 kernel."""
    if sel in ("auto", "kf", "kfh") and name in KF_TAKES:
        return 5
    return 0


# ---- rows: every selection --------------------------------------------------------------------

@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("name", mg.ROWS389)
def test_rows(route, monkeypatch, name, sel):
    """The whole table under one kernel selection: shd_route_rows, shd_route_rows_async, and one
    strided launch (ld = nt + 5, a base that is 8- but not 16-byte aligned, canaries around)."""
    ref = reference(name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    select(monkeypatch, sel)
    eng = route.RouteEngine(g)
    info = eng.info
    print(name, sel, {k: info[k] for k in ("kernel", "reserved", "lds_resident", "block", "dist_bound", "lat16")})
    assert info["multigraph"] == 1 and info["kernel"] == expect_kernel(name, sel)
    assert info["dist_bound"] == 0 and info["lat16"] == 0          # k32.bound is 0: no u16 payload
    if sel == "kfh" and info["kernel"] == 5:
        assert info["lds_resident"] == 0
        assert info["reserved"] == (100 if name == "multi389_frac" else 1)
    lat, rel, mn, code = host_rows(route, eng, S, T)
    assert code == route.ENOEDGE                                    # a third of the sources has no self-loop
    check_rows(route, ref, lat, rel, mn, code)
    l2, r2, m2, c2 = dev_rows(route, eng, S, T)
    assert np.array_equal(l2, lat, equal_nan=True) and np.array_equal(r2, rel, equal_nan=True)
    assert np.array_equal(m2, mn) and c2 == code

    def launch(d_s, d_t, la, re_, mi, ld):
        eng.rows_async(d_s, d_t, la, re_, mi, dispatch=False, ld=ld)
    a, b, m, c = run(route, eng, launch, S, T, len(T) + 5, shift=1)   # (ENOEDGE once: run() syncs twice)
    assert np.array_equal(a.view(np.float64), lat, equal_nan=True) and np.array_equal(b.view(np.float64), rel, equal_nan=True)
    assert np.array_equal(m.view(np.float64)[:, 0], mn) and c == code


@pytest.mark.parametrize("name", mg.ROWS389)
def test_kfh_f64_arcs(route, monkeypatch, name):
    """SHD_ROUTE_KFPK=0 with KFH: f64 arcs instead of the packed ones, the same table."""
    ref = reference(name)
    select(monkeypatch, "kfh")
    monkeypatch.setenv("SHD_ROUTE_KFPK", "0")
    eng = route.RouteEngine(ref["g"])
    assert eng.info["multigraph"] == 1 and eng.info["kernel"] == expect_kernel(name, "kfh")
    assert eng.info["reserved"] == 0
    if eng.info["kernel"] == 5:
        assert eng.info["lds_resident"] == 0
    check_rows(route, ref, *host_rows(route, eng, ref["S"], ref["T"]))


@pytest.mark.parametrize("sel", ["auto", "f64"])
def test_rows_8000(route, monkeypatch, sel):
    """multi8000, five sources: KF with 1024 threads, and the generic kernel with its per-source
    state in HBM."""
    ref = reference("multi8000")
    select(monkeypatch, sel)
    eng = route.RouteEngine(ref["g"])
    assert eng.info["multigraph"] == 1
    if sel == "f64":
        assert eng.info["kernel"] == 0 and eng.info["lds_resident"] == 0
    else:
        assert eng.info["kernel"] == 5 and eng.info["block"] == 1024
    out = host_rows(route, eng, ref["S"], ref["T"])
    assert out[3] == route.ENOEDGE
    check_rows(route, ref, *out)
    o2 = dev_rows(route, eng, ref["S"], ref["T"])
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(o2[:3], out[:3])) and o2[3] == out[3]


def test_loops_only(route, oracle_mod, monkeypatch):
    """Two self-loops on a few vertices of a simple graph make it a multigraph; off the diagonal
    its rows are those of the graph without the second loops (simple: KB runs), and the diagonal,
    like shd_route_self, sees the lowest-id loop only."""
    select(monkeypatch, "auto")
    ref = reference("loops_only")
    g, S, T = ref["g"], ref["S"], ref["T"]
    simple = graph_of("loops_only_simple")
    e1, e0 = route.RouteEngine(g), route.RouteEngine(simple)
    assert e1.info["multigraph"] == 1 and e1.info["kernel"] == 5 and e1.info["lat16"] == 0
    assert e0.info["multigraph"] == 0 and e0.info["kernel"] == 2
    out1, out0 = host_rows(route, e1, S, T), host_rows(route, e0, S, T)
    check_rows(route, ref, *out1)
    for a, b in zip(out1, out0):
        assert np.array_equal(a, b, equal_nan=True)               # (the diagonal too: the first loop)
    two = np.flatnonzero(np.bincount(g.src[g.src == g.dst], minlength=g.n) == 2)
    assert len(two) > 3
    for v in two:
        first = int(np.flatnonzero((g.src == v) & (g.dst == v))[0])
        assert out1[0][v, v] == g.latency[first] and out1[1][v, v] == 1.0 - g.packetloss[first]
    v = np.arange(g.n, dtype=np.int32)
    sl, sr = e1.self_paths(v)
    og = oracle_mod.OracleGraph(simple)
    want = [og.self_path(int(k)) for k in v]
    assert np.array_equal(sl, [w[0] for w in want]) and np.array_equal(sr, [w[1] for w in want])
    s0 = e0.self_paths(v)
    assert np.array_equal(sl, s0[0]) and np.array_equal(sr, s0[1])


# ---- hops, paths, loads -----------------------------------------------------------------------

def some_sources(ref, k=24):
    """k sources: vertex 0, the highest one, and vertices with two, one and no self-loop."""
    g = ref["g"]
    cnt = np.bincount(g.src[g.src == g.dst], minlength=g.n)
    pick = [0, g.n - 1]
    for c in (2, 1, 0):
        v = np.flatnonzero(cnt == c)
        pick += [int(v[i * len(v) // 8]) for i in range(8)]
    return np.array(list(dict.fromkeys(pick))[:k], np.int32)


def split(route, off, vert, edge):
    eoff = route.path_edge_offsets(off)
    out = []
    for k in range(len(off) - 1):
        nv = int(off[k + 1] - off[k])
        out.append(None if nv == 0 else (vert[off[k]: off[k + 1]].tolist(), edge[eoff[k]: eoff[k] + nv - 1].tolist()))
    return out


def check_routes(route, eng, ref, S, dispatch):
    """hops, paths, loads and pair_loads of the sources S over every vertex against the Ref, and
    the returned edge ids against the rows' numbers."""
    g, R = ref["g"], ref["ref"]
    T = ref["T"]
    rows = np.searchsorted(ref["S"], S)
    assert np.array_equal(ref["S"][rows], S)
    eh = ref["hops"][rows]
    failed = bool((eh < 0).any())
    code = route.ENOEDGE if failed else route.OK
    (hops, mx), c = call(route, eng.hops, S, T, dispatch=dispatch)
    assert np.array_equal(hops, eh) and np.array_equal(mx, eh.max(axis=1)) and c == code
    (lat, rel, _), c = call(route, eng.rows, S, T, dispatch=dispatch)
    assert np.array_equal(lat, ref["lat"][rows], equal_nan=True) and c == code
    ps, pt = np.repeat(S, len(T)).astype(np.int32), np.tile(T, len(S)).astype(np.int32)
    (off, vert, edge), c = call(route, eng.paths, ps, pt, dispatch=dispatch)
    assert c == code
    got = split(route, off, vert, edge)
    erel = 1.0 - g.packetloss
    for k, (s, t) in enumerate(zip(ps.tolist(), pt.tolist())):
        want = R.path(s, t, dispatch)
        if want is None:
            assert got[k] is None
            continue
        assert got[k] == (want[0], want[1]), (s, t)
        # the edges it returned give the rows' numbers: (1.0 * f_s) * f_t (f_s alone on the batch
        # self entry), then the hops from s on
        L, r = 0.0, R.base(s, t)
        if s == t and not R.is_direct(s, t, dispatch):
            r = 1.0 if np.isnan(R.vf[s]) else 1.0 * R.vf[s]
        for e in want[1]:
            L = L + g.latency[e]
            r = r * erel[e]
        i, j = k // len(T), k % len(T)
        assert L == lat[i, j] and r == rel[i, j], (s, t)
    rng = np.random.default_rng(len(S))
    W = rng.integers(1, 1 << 40, size=(len(S), len(T)), dtype=np.uint64)
    el, tr, un = R.loads(ps, pt, W.reshape(-1), dispatch)
    (gel, gtr, gun), c = call(route, eng.loads, S, T, W, dispatch=dispatch)
    assert np.array_equal(gel, el) and np.array_equal(gtr, tr) and gun == un and c == code
    q = rng.integers(0, len(ps), size=600)
    q = np.concatenate([q, q[:40]])
    pw = rng.integers(1, 1 << 40, size=len(q), dtype=np.uint64)
    el, tr, un = R.loads(ps[q], pt[q], pw, dispatch)
    (gel, gtr, gun), c = call(route, eng.pair_loads, ps[q], pt[q], pw, dispatch=dispatch)
    assert np.array_equal(gel, el) and np.array_equal(gtr, tr) and gun == un
    return el


@pytest.mark.parametrize("form", ["lds", "hbm"])
@pytest.mark.parametrize("name", HOP_GRAPHS)
def test_hops_paths_loads(route, monkeypatch, name, form):
    select(monkeypatch, "auto")
    if form == "hbm":
        monkeypatch.setenv("SHD_ROUTE_HOPS_LDS", "0")
        monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    ref = reference(name)
    eng = route.RouteEngine(ref["g"])
    assert eng.info["multigraph"] == 1
    el = check_routes(route, eng, ref, some_sources(ref), False)
    assert el[mg.added_from(name):].any()                # added edges carry load


# ---- dispatch ---------------------------------------------------------------------------------

def test_complete_dispatch_takes_the_lowest_edge_id(route, monkeypatch):
    """multi_k24 is complete: with SHD_ROUTE_DISPATCH every entry goes over the lowest edge id
    of its pair, also where the added parallel edge is lighter; without the flag the tree path
    takes the lighter edge.  shd_route_direct is the same dense rule."""
    select(monkeypatch, "auto")
    rd, rt = reference("multi_k24", True), reference("multi_k24", False)
    g, S, T, R = rd["g"], rd["S"], rd["T"], rd["ref"]
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1 and eng.info["is_complete"] == 1 and R.complete
    for ref, dispatch in ((rd, True), (rt, False)):
        out = host_rows(route, eng, S, T, dispatch=dispatch)
        assert out[3] == route.OK
        check_rows(route, ref, *out)
        check_routes(route, eng, ref, S, dispatch)
    first = mg.added_from("multi_k24")
    lighter = 0
    for s in S:
        for t in T:
            if s != t:
                e0 = R.first[int(s), int(t)]
                assert e0 < first and rd["lat"][s, t] == g.latency[e0]
                tree = R.path(int(s), int(t), False)
                if len(tree[1]) == 1 and tree[1][0] >= first:
                    lighter += 1
                    assert rt["lat"][s, t] < rd["lat"][s, t]
    assert lighter > 0
    dl, dr, dm = eng.direct(S, T)
    wl, wr = R.direct(S, T)
    assert np.array_equal(dl, wl) and np.array_equal(dr, wr) and np.array_equal(dm, row_min_of(wl))
    assert np.array_equal(dl, rd["lat"])


@pytest.mark.parametrize("form", ["lds", "hbm"])
def test_prefer_direct_dispatch(route, monkeypatch, form):
    """A prefer-direct copy of multi389: adjacent pairs direct over the lowest edge id, the
    others by tree."""
    select(monkeypatch, "auto")
    if form == "hbm":
        monkeypatch.setenv("SHD_ROUTE_HOPS_LDS", "0")
        monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    ref = reference("multi389_prefer", True)
    tree = reference("multi389")
    g, S, T, R = ref["g"], ref["S"], ref["T"], ref["ref"]
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1 and eng.info["prefer_direct"] == 1 and eng.info["is_complete"] == 0
    out = host_rows(route, eng, S, T, dispatch=True)
    check_rows(route, ref, *out)
    adj = np.zeros((g.n, g.n), bool)
    nl = g.src != g.dst
    adj[g.src[nl], g.dst[nl]] = True; adj[g.dst[nl], g.src[nl]] = True
    assert np.array_equal(out[0][~adj], tree["lat"][~adj], equal_nan=True)
    assert (out[0][adj] > tree["lat"][adj]).sum() > 100          # a direct edge that is no shortest path
    check_routes(route, eng, ref, some_sources(ref, 12), True)


def test_count_complete_dispatch(route, monkeypatch):
    """Twelve incident edges on each of twelve vertices: complete by the reference's count, so
    the dispatch looks every pair up directly, and the pairs without an edge fail."""
    select(monkeypatch, "auto")
    ref = reference("count_complete", True)
    g, S, T, R = ref["g"], ref["S"], ref["T"], ref["ref"]
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1 and eng.info["is_complete"] == 1
    lat, rel, mn, code = host_rows(route, eng, S, T, dispatch=True)
    assert code == route.ENOEDGE
    check_rows(route, ref, lat, rel, mn, code)
    missing = np.array([[(int(s), int(t)) not in R.first for t in T] for s in S])
    assert missing.sum() == 12 * 5 + 4 and np.array_equal(np.isnan(lat), missing) and np.array_equal(np.isnan(rel), missing)
    assert np.isfinite(mn).all()

    def launch(d_s, d_t, la, re_, mi, ld):
        eng.rows_async(d_s, d_t, la, re_, mi, dispatch=True, ld=ld)
    a, b, m, c = run(route, eng, launch, S, T, len(T) + 5, shift=1)   # (run() checks: reported once)
    assert c == route.ENOEDGE and np.array_equal(a.view(np.float64), lat, equal_nan=True)
    assert np.array_equal(m.view(np.float64)[:, 0], mn)
    check_routes(route, eng, ref, S, True)
    (hops, _), c = call(route, eng.hops, S, T, dispatch=True)
    assert np.array_equal(hops < 0, missing) and c == route.ENOEDGE
    (_, _, un), c = call(route, eng.loads, S, T, None, dispatch=True)
    assert un == missing.sum()
    check_rows(route, reference("count_complete"), *host_rows(route, eng, S, T, dispatch=False))


# ---- plans, the fill, what a multigraph refuses -----------------------------------------------

@pytest.mark.parametrize("sel", ["auto", "kd"])
@pytest.mark.parametrize("world", [1, 3])
def test_plans_fall_back(route, monkeypatch, sel, world):
    """A seeded plan needs KD, which a multigraph never gets: plain rows, the same table."""
    ref = reference("multi389")
    g, S, T = ref["g"], ref["S"], ref["T"]
    select(monkeypatch, sel)
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == (5 if sel == "auto" else 0)
    seen = []
    for rank in range(world):
        plan = eng.plan(S[::-1].copy(), world, rank)
        assert plan.info["seeded"] == 0 and plan.info["rows"] == len(plan.positions)
        rows = S[::-1][plan.positions]
        seen += rows.tolist()

        def launch(d_s, d_t, lat, rel, mn):
            plan.rows_async(d_t, lat, rel, mn, dispatch=False)
        lat, rel, mn, code = dev_rows(route, eng, rows, T, launch)
        check_rows(route, ref, lat, rel, mn, code, rows=rows)
        plan.close()
    assert sorted(seen) == S.tolist()


def attached(g):
    return np.arange(0, g.n, 2, dtype=np.int32)


@pytest.mark.parametrize("world", [1, 3])
def test_fill_triangle(route, monkeypatch, world):
    """shd_route_fill_triangle, interleaved, one row per stage chunk: every rank's rows of the
    triangle hold row i's entries (first writer wins under ascending sources)."""
    select(monkeypatch, "auto")
    monkeypatch.setenv("SHD_ROUTE_FILL_STAGE", "1")
    ref = reference("multi389")
    g = ref["g"]
    A = attached(g)
    na = len(A)
    eng = route.RouteEngine(g)
    buf = route.PinnedBuffer(16 * na * (na + 1) // 2)
    buf.array()[:] = -7.0
    mins = []
    for rank in range(world):
        mn, _ = eng.fill_triangle(A, buf, world=world, rank=rank, dispatch=True, lat16=False)
        assert eng.last_fill_code in (route.OK, route.ENOEDGE)
        mins.append(mn)
    lat, rel = read_triangle(route, buf, na, False)
    el, er = ref["lat"][np.ix_(A, A)], ref["rel"][np.ix_(A, A)]
    iu = np.triu_indices(na)
    assert np.array_equal(lat[iu], el[iu], equal_nan=True) and np.array_equal(rel[iu], er[iu], equal_nan=True)
    assert 0 < np.isnan(el[iu]).sum() == int((~ref["loops"][A]).sum())
    assert min(mins) == np.nanmin(el[iu])


def test_what_a_multigraph_refuses(route, monkeypatch):
    """info.lat16 is 0 (k32.bound is 0), so the compact triangle and the u16 payload are
    SHD_ROUTE_EUNSUPPORTED, as are the K4 table and its rows; nothing is written."""
    import torch
    from shadow_amd.shard import pack_triangle_host, tri_offsets
    select(monkeypatch, "auto")
    ref = reference("multi389")
    g = ref["g"]
    A = attached(g)
    na = len(A)
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 0 and eng.info["dist_bound"] == 0
    nbytes = 64 * route.tri16_lines(na)
    buf = route.PinnedBuffer(nbytes)
    raw = buf.array().view(np.uint64)
    raw[:] = CAN64
    with pytest.raises(route.RouteError) as ei:
        eng.fill_triangle(A, buf, dispatch=True, lat16=True)
    assert ei.value.code == route.EUNSUPPORTED and np.all(raw == CAN64)
    dev = torch.device("cuda", 0)
    pos = np.arange(na - 1, -1, -3, dtype=np.int32)
    lat, rel = ref["lat"][np.ix_(A[pos], A)], ref["rel"][np.ix_(A[pos], A)]
    off, tot = tri_offsets(pos, na)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_lat, d_rel, d_pos, d_off = d(lat), d(rel), d(pos), d(off[:-1].copy())
    o16 = torch.full((tot,), 0x5EAD, dtype=torch.int16, device=dev)
    orr = Padded(1, tot)
    with pytest.raises(route.RouteError) as ei:
        eng.tri_payload_async(d_lat, d_rel, d_pos, d_off, na, o16, orr.t, lat16=True)
    assert ei.value.code == route.EUNSUPPORTED
    eng.sync()
    assert bool((o16 == 0x5EAD).all()) and orr.untouched()
    ol = Padded(1, tot)
    eng.tri_payload_async(d_lat, d_rel, d_pos, d_off, na, ol.t, orr.t, lat16=False)
    eng.sync()
    hl, hr = pack_triangle_host(lat, rel, pos, na, lat16=False)
    assert np.array_equal(ol.bits(tot).view(np.float64)[0], hl, equal_nan=True)
    assert np.array_equal(orr.bits(tot).view(np.float64)[0], hr, equal_nan=True)
    assert np.isnan(hl).any()
    # K4
    S = ref["S"][:7]
    d_s, d_t = d(S), d(ref["T"])
    a, b, m = Padded(len(S), g.n), Padded(len(S), g.n), Padded(len(S), 1)
    for _ in range(2):
        with pytest.raises(route.RouteError) as ei:
            eng.fw_table_async()
        assert ei.value.code == route.EUNSUPPORTED
        with pytest.raises(route.RouteError) as ei:
            eng.fw_rows_async(d_s, d_t, a.t, b.t, m.t)
        assert ei.value.code == route.EUNSUPPORTED
    eng.sync()
    assert a.untouched() and b.untouched() and m.untouched()
    # (a simple graph that K4 takes, before its table: a misuse, SHD_ROUTE_EINVAL)
    e0 = route.RouteEngine(graph_of("loops_only_simple"))
    with pytest.raises(route.RouteError) as ei:
        e0.fw_rows_async(d_s, d_t[:150], a.t, b.t, m.t)
    assert ei.value.code == route.EINVAL
    e0.fw_table_async()
    e0.sync()


# ---- the front end ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["multi389", "multi389_dir"])
def test_front_end(route, oracle_mod, monkeypatch, tmp_path, name):
    """The graph through graphml into shd_topology: the cache holds, for the pair {a, b} of
    attached vertices, a <= b, the entry of row a (the path to self where a has no self-loop),
    and the route behind it is the Ref's, edge ids included; the [latency, loss] hops of the
    route line are the edges the cached numbers came from."""
    from shadow_amd import topology
    from shadow_amd.graph import to_graphml
    from tests.test_hops_gpu import _ref_line
    topology.load_library()
    select(monkeypatch, "auto")
    ref = reference(name)
    g, R = ref["g"], ref["ref"]
    pth = tmp_path / f"{name}.graphml.xml"
    to_graphml(g, str(pth))
    t = topology.Topology.new(str(pth))
    A = np.arange(1, g.n, 4, dtype=np.int32)[:90]          # vertices with no, one and two self-loops
    A = np.unique(np.concatenate([A, [0, 6, 12, g.n - 1]])).astype(np.int32)
    t.attach_all(A)
    na = len(A)
    og = oracle_mod.OracleGraph(g)
    el, er = ref["lat"][np.ix_(A, A)].copy(), ref["rel"][np.ix_(A, A)].copy()
    noloop = np.flatnonzero(np.isnan(np.diag(el)))
    assert 0 < len(noloop) < na
    for i in noloop:
        el[i, i], er[i, i] = og.self_path(int(A[i]))
    il = np.tril_indices(na, -1)
    el[il], er[il] = el.T[il], er.T[il]
    lat, rel = t.table(A)
    assert np.array_equal(lat, el) and np.array_equal(rel, er)
    assert t.min_path_latency() == el.min()
    assert t.triangle_bytes() == 16 * na * (na + 1) // 2          # interleaved: lat16 is 0
    ids = [g.vertex_id(v) for v in range(g.n)]
    rng = np.random.default_rng(na)
    pairs = [(int(a), int(b)) for a, b in zip(rng.choice(A, 40), rng.choice(A, 40))] + [(0, 0), (6, 6), (12, 0)]
    hop = re.compile(r"\[([0-9.]+),([0-9.]+)\]")
    added = 0
    for s, d in pairs:
        a, b = min(s, d), max(s, d)
        if a == b and not ref["loops"][a]:
            continue
        vs, es = R.path(a, b, False)
        gv, ge = t.get_path(s, d)
        assert gv.tolist() == vs and ge.tolist() == es, (s, d)
        added += sum(e >= mg.added_from(name) for e in es)
        line = t.format_path(s, d)
        assert line == _ref_line(g, ids, a, b, vs, es, t.get_latency(a, b), t.get_reliability(a, b))
        nums = [(float(x), float(y)) for x, y in hop.findall(line)]
        assert len(nums) == len(es)
        L, r = 0.0, 1.0
        for w, p in nums:
            L += w; r *= 1.0 - p
        # %f prints six decimals: each hop's latency and loss within 5e-7 of the edge's
        assert abs(L - t.get_latency(a, b)) <= 5e-7 * len(es) + 1e-9
        assert abs(r - t.get_reliability(a, b)) <= 5e-7 * len(es) + 1e-9
    assert added > 0
    t.close()
