"""GPU: the path folds -- shd_route_fold*, shd_route_pair_fold, RouteEngine's wrappers and the
front end's shd_topology_edge_jitter / shd_topology_fold_pairs -- against tests/fold_ref.py (the
plain Python left fold over Ref.path's edge ids, held to Ref.rows by tests/test_fold.py).

Every comparison is exact, NaN where NaN belongs, over every entry: the engine's folds are
deterministic left folds from the source, so there is no tolerance anywhere in this file."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fold_ref as fr
from tests import shape_graphs as sg
from tests import stream_order as so
from tests import test_hops_gpu as hg
from tests import test_ties_gpu as tg

pytestmark = pytest.mark.gpu
OPS = fr.ALL_OPS                      # over fold_ref.columns: decimals, integers, (0, 1], +-inf
# eight folds, ops repeated, a column of its own each (never SUM over the +-inf column)
OPS8 = [fr.SUM, fr.MIN, fr.MAX, fr.PROD, fr.PROD, fr.MAX, fr.MIN, fr.SUM]


@pytest.fixture(scope="module")
def route():
    from shadow_amd import route as r
    r.load_library()
    return r


@pytest.fixture(scope="module")
def topo():
    from shadow_amd import topology
    topology.load_library()
    return topology


@pytest.fixture(autouse=True)
def close_engines(route, monkeypatch):
    """Every context a test makes is closed when the test ends, also when it fails half-way."""
    made = []
    real = route.RouteEngine

    def tracked(*a, **k):
        made.append(real(*a, **k))
        return made[-1]
    monkeypatch.setattr(route, "RouteEngine", tracked)
    yield
    for e in reversed(made):
        e.close()


@pytest.fixture(autouse=True)
def default_forms(monkeypatch):
    for k in ("SHD_ROUTE_FOLD_LDS", "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in ("ba60_multi", "ba60_holes", "ring66k"):
        return hg._graph(name)[0]
    return tg.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return fr.FoldRef(graph(name))


@functools.lru_cache(maxsize=None)
def cols(name):
    """The four value columns of a graph (fold_ref.columns), read-only."""
    c = fr.columns(graph(name), graph(name).n)
    c.setflags(write=False)
    return c


def cols8(name):
    c = cols(name)
    more = fr.columns(graph(name), graph(name).n + 77)
    return np.stack([c[0], c[1], c[2], c[3], more[2], more[3], more[0], c[2] * 0.5])


def run(route, call, *args, **kw):
    """(result, code) of a call, failed entries or not."""
    try:
        return call(*args, **kw), route.OK
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return err.partial, err.code


def check(route, name, S, dispatch=False, T=None, eng=None, ops=OPS, vals=None):
    """eng.fold(S, T, ops, vals) equals the reference in every entry; the code is one the failed
    entries give."""
    g = graph(name)
    T = np.arange(g.n, dtype=np.int32) if T is None else np.asarray(T, np.int32)
    S = np.asarray(S, np.int32)
    vals = cols(name)[: len(ops)] if vals is None else vals
    want, codes = ref(name).rows(S, T, ops, vals, dispatch)
    eng = eng or route.RouteEngine(g)
    got, code = run(route, eng.fold, S, T, ops, vals, dispatch=dispatch)
    assert (code in codes) if codes else code == route.OK, (code, codes)
    assert got.dtype == np.float64 and got.shape == (len(ops), len(S), len(T))
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert fr.same(got, want), (len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])
    return got, want, code


# ---- small goldens ------------------------------------------------------------------------------

@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", hg.SMALL)
def test_small_goldens(route, name, dispatch):
    """All attached sources x all vertices: prefer-direct (ba80_prefer), complete (k24),
    directed, fractional and vertex loss among them."""
    g, A = hg._graph(name)
    got, want, _ = check(route, name, A, dispatch)
    assert np.count_nonzero(~np.isnan(got[0])) > g.n
    if name == "ba80_prefer":
        other, _ = run(route, route.RouteEngine(g).fold, A, np.arange(g.n), OPS, cols(name), dispatch=not dispatch)
        assert not fr.same(other, got)                  # adjacent pairs take their direct edge


@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", hg.SMALL)
def test_identities_on_the_device(route, name, dispatch):
    """SUM of the latencies is the rows' lat and SUM of ones the hops' count, bit for bit, and
    PROD of 1 - loss the rows' rel on graphs without vertex loss."""
    g, A = hg._graph(name)
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    vals = np.stack([g.latency, np.ones(g.m), 1.0 - np.asarray(g.packetloss, np.float64)])
    got, code = run(route, eng.fold, A, T, [fr.SUM, fr.SUM, fr.PROD], vals, dispatch=dispatch)
    (lat, rel, _), rcode = run(route, eng.rows, A, T, dispatch=dispatch)
    (hops, _), hcode = run(route, eng.hops, A, T, dispatch=dispatch)
    assert (code == route.OK) == (rcode == route.OK) == (hcode == route.OK)
    assert fr.same(got[0], lat)
    assert fr.same(got[1], np.where(hops < 0, np.nan, hops.astype(np.float64)))
    assert fr.no_vertex_loss(g) == (name != "ba120_vloss")
    if fr.no_vertex_loss(g):
        assert fr.same(got[2], rel)
    else:
        assert np.array_equal(np.isnan(got[2]), np.isnan(rel))


# ---- the shape suite ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["star1100", "lollipop", "grid", "dir_grid", "biclique1030"])
def test_shapes(route, name):
    """star1100: a level wider than the workgroup; lollipop: 300 levels; grid: ties; dir_grid:
    directed, every arc with values of its own (strongly connected: its failed entries are the
    self entries without a self-loop; a context takes no graph with unreachable vertices); biclique1030: wide in-lists."""
    g = graph(name)
    S = tg._spread(g.n)
    if name == "biclique1030":
        S = np.array([0, 16, 17, 500, g.n - 1], np.int32)
    if name == "star1100":
        S = np.array([0, 1, 2, 600, g.n - 1], np.int32)
    if name == "dir_grid":
        S = np.array([0, 1, 52, 130, g.n - 1], np.int32)        # 1, 52 and 130 have no self-loop
    got, want, code = check(route, name, S)
    (hops, _), _ = run(route, route.RouteEngine(g).hops, S, np.arange(g.n), dispatch=False)
    if name == "star1100":
        assert np.count_nonzero(hops[1] == 2) > 1024        # source 1: one level of more than 1,024 vertices
    if name == "lollipop":
        assert hops.max() >= 300
    if name == "grid":
        assert hops.max() == 63
    if name == "dir_grid":
        assert g.directed and code == route.ENOEDGE and np.isnan(got[0]).sum() == np.count_nonzero(S % 3 == 1)


@pytest.mark.parametrize("loops", sg.TINY_LOOPS)
@pytest.mark.parametrize("n", sg.TINY_N)
def test_tiny(route, n, loops):
    """Paths of 1 to 9 vertices: SHD_ROUTE_ENOEDGE entries are NaN, the rest is written."""
    name = f"tiny{n}_{loops}"
    g = graph(name)
    got, want, code = check(route, name, np.arange(n))
    noloop = ~np.isin(np.arange(n), g.src[g.src == g.dst])
    assert np.array_equal(np.isnan(got[0]), np.diag(noloop)) and (code == route.ENOEDGE) == bool(noloop.any())


def test_multigraph(route):
    """ba60 with 10 edges doubled at another latency and other values: every hop uses the edge
    shd_route_paths reports, and folding over eng.paths' edge ids on the host gives the same."""
    name = "ba60_multi"
    g = graph(name)
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1
    c = np.array(cols(name))
    key = lambda e: (min(int(g.src[e]), int(g.dst[e])), max(int(g.src[e]), int(g.dst[e])))
    first = {}
    for e in range(g.m - 10):
        first.setdefault(key(e), e)
    twins = [(first[key(e)], e) for e in range(g.m - 10, g.m)]
    for a, b in twins:                                          # the doubled edge: other values in every column
        c[0, b], c[1, b], c[2, b] = c[0, a] + 0.25, c[1, a] % 9 + 1, c[2, a] * 0.5
        c[3, b] = -c[3, a] if np.isinf(c[3, a]) else c[3, a] % 9 + 1
    assert len(twins) == 10 and all(np.all(c[:, a] != c[:, b]) for a, b in twins)
    S = T = np.arange(g.n, dtype=np.int32)
    got, want, code = check(route, name, S, eng=eng, vals=c)
    ps, pt = np.repeat(S, g.n), np.tile(T, g.n)
    (off, vert, edge), pcode = run(route, eng.paths, ps, pt, dispatch=False)
    assert pcode == code
    eoff = route.path_edge_offsets(off)
    host = np.full((4, len(ps)), np.nan)
    used = set()
    for p in range(len(ps)):
        h = int(off[p + 1] - off[p]) - 1
        if h < 0:
            continue
        es = edge[eoff[p]: eoff[p] + h].tolist()
        used.update(es)
        for k, op in enumerate(OPS):
            host[k, p] = fr.fold_one(op, [float(c[k, e]) for e in es])
    assert fr.same(got.reshape(4, -1), host)
    assert any(b in used for _, b in twins) and any(a in used for a, _ in twins)


# ---- the state forms --------------------------------------------------------------------------------

@pytest.mark.parametrize("over", [0, 1])
def test_lds_limit(route, over):
    """sized(n) at the largest n whose state layout fits the LDS and at n + 1 (the HBM form)."""
    n = fr.lds_max_n() + over
    assert fr.fits_lds(n) == (over == 0)
    check(route, f"sized{n}", [0, n - 1, n // 2], ops=[fr.SUM, fr.MIN], T=np.arange(0, n, 3))


@pytest.mark.parametrize("name", ["grid", "ba64_ties"])
def test_hbm_form(route, monkeypatch, name):
    monkeypatch.setenv("SHD_ROUTE_FOLD_LDS", "0")
    g = graph(name)
    check(route, name, tg._spread(g.n, 8) if name == "grid" else hg._graph(name)[1])


def test_beyond_u16(route):
    """66,000 vertices: u32 order entries, the state in HBM slices."""
    g, A = hg._graph("ring66k")
    assert g.n > 65535 and not fr.fits_lds(g.n) and len(A) <= 4
    T = np.unique(np.concatenate([np.arange(0, g.n, 41), np.arange(g.n - 40, g.n), A])).astype(np.int32)
    got, _, code = check(route, "ring66k", A, T=T, ops=[fr.SUM, fr.PROD], vals=cols("ring66k")[[0, 2]])
    assert code == route.ENOEDGE and np.isnan(got[0]).sum() == 2 and T.max() > 65535


def test_hbm_slices_reused(route, monkeypatch):
    """The HBM form on dir_grid with 600 sources over the 512 slots a small graph gets: 88
    workgroups take a second source, another one than their first, with a failed set of its own,
    and nothing of the first (level offsets, order list, carried values) may survive.  (A
    context only takes a strongly connected graph, so no vertex is ever unreached and the failed
    entries are the self entries without a self-loop; the kernel still resets every value to NaN
    per source.)"""
    name = "dir_grid"
    g = graph(name)
    monkeypatch.setenv("SHD_ROUTE_FOLD_LDS", "0")
    assert (256 << 20) // fr.layout_total(g.n, 2) > 512
    v = np.arange(g.n)
    S = np.concatenate([v, v[::-1], (v + g.n // 2) % g.n])[:600].astype(np.int32)
    assert len(S) == 600 and np.all(S[512:] != S[:88])
    T = v[v % 3 != 2]                                            # (the reference walks every entry's path)
    got, want, code = check(route, name, S, ops=[fr.SUM, fr.MAX], T=T)
    nan = np.isnan(got[0])
    assert code == route.ENOEDGE and not np.array_equal(nan[512:], nan[:88])


@pytest.mark.parametrize("lds", [None, "0"])
def test_three_chunks(route, monkeypatch, lds):
    """SHD_ROUTE_HOPS_SCRATCH of three sources (16 n bytes each): 7 sources take three chunks,
    each of which lands at its own rows of both planes."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_FOLD_LDS", lds)
    got, want, _ = check(route, "ba64_ties", A[:7], ops=[fr.SUM, fr.MIN])
    assert so.rows_differ(want[0], np.roll(want[0], 3, axis=0)) and not fr.same(want[0], want[1])


# ---- nf ---------------------------------------------------------------------------------------------

def test_one_call_equals_single_calls(route):
    g, A = hg._graph("ba64_ties")
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    got, want, code = check(route, "ba64_ties", A[:9], eng=eng)
    for k, op in enumerate(OPS):
        one, c1 = run(route, eng.fold, A[:9], T, [op], cols("ba64_ties")[k], dispatch=False)
        assert one.shape == (1, 9, g.n) and c1 == code and fr.same(one[0], got[k])


@pytest.mark.parametrize("name,dispatch", [("ba64_ties", False), ("ba80_prefer", True)])
def test_eight_folds(route, name, dispatch):
    g, A = hg._graph(name)
    v = cols8(name)
    assert len({c.tobytes() for c in v}) == 8
    check(route, name, A[:6], dispatch, ops=OPS8, vals=v)


# ---- the contract -----------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))


def _sync(route, eng):
    try:
        eng.sync()
        return route.OK
    except route.RouteError as err:
        return err.code


def test_strides(route):
    """ld = nt + 3 and plane = ns * ld + 5 in a sentinel-filled buffer: every entry is right and
    every element outside the entries still holds the sentinel."""
    from tests.test_contract_gpu import Padded
    g, A = hg._graph("ba64_ties")
    S, T = A[:7].astype(np.int32), np.arange(g.n, dtype=np.int32)[::-1].copy()
    ns, nt = len(S), len(T)
    ld, plane = nt + 3, ns * (nt + 3) + 5
    want, codes = ref("ba64_ties").rows(S, T, OPS, cols("ba64_ties"))
    out = Padded(1, 4 * plane)
    eng = route.RouteEngine(g)
    eng.fold_async(_dev(S), _dev(T), OPS, _dev(cols("ba64_ties")), out.t, dispatch=False, ld=ld, plane=plane)
    code = _sync(route, eng)
    assert (code in codes) if codes else code == route.OK
    bits = out.bits(4 * plane)[0]                               # (the guards around the buffer checked)
    entry = np.zeros(4 * plane, bool)
    for k in range(4):
        body = bits[k * plane: k * plane + ns * ld].reshape(ns, ld)
        entry[k * plane: k * plane + ns * ld].reshape(ns, ld)[:, :nt] = True
        assert fr.same(body[:, :nt].copy().view(np.float64), want[k])
    assert np.all(bits[~entry] == out.can) and np.count_nonzero(~entry) == 4 * (3 * ns + 5)


def _raw(route, eng, name, *args):
    return getattr(route.load_library(), name)(eng._h, *args)


def test_empty_and_invalid(route):
    """ns == 0 and nt == 0 are OK; nf of 0 or 9, an op of 4, a vertex out of range, a null val
    and a NaN in val are SHD_ROUTE_EINVAL with the outputs untouched."""
    from tests.test_contract_gpu import Padded
    g, A = hg._graph("ba60")
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    c = cols("ba60")
    assert eng.fold([], T, OPS, c).shape == (4, 0, g.n) and eng.fold(A[:3], [], OPS, c).shape == (4, 3, 0)
    assert eng.pair_fold([], [], OPS, c).shape == (4, 0)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    S = A[:2].astype(np.int32)
    ops4 = np.array(OPS, np.int32)
    nan = np.array(c); nan[2, g.m // 2] = np.nan
    many = np.zeros(9, np.int32)
    cases = [  # (sources, targets, ops, nf, values)
        (S, T, ops4, 0, c), (S, T, many, 9, np.ones((9, g.m))), (S, T, np.array([0, 4], np.int32), 2, c),
        (S, T, np.array([-1], np.int32), 1, c), (np.array([A[0], g.n], np.int32), T, ops4, 4, c),
        (np.array([-1, A[0]], np.int32), T, ops4, 4, c), (S, np.array([0, g.n], np.int32), ops4, 4, c),
        (S, T, ops4, 4, None), (S, T, ops4, 4, nan), (S, T, None, 1, c),
    ]
    for s, t, ops, nf, v in cases:
        out = np.full((max(nf, 1), len(s), len(t)), 7.5)
        rc = _raw(route, eng, "shd_route_fold", P(s), len(s), P(t), len(t), 0, P(ops), nf, P(v), P(out))
        assert rc == route.EINVAL and np.all(out == 7.5), (nf, rc)
        pt = np.resize(t, len(s)).astype(np.int32)
        out = np.full((max(nf, 1), len(s)), 7.5)
        rc = _raw(route, eng, "shd_route_pair_fold", P(s), P(pt), len(s), 0, P(ops), nf, P(v), P(out))
        assert rc == route.EINVAL and np.all(out == 7.5), (nf, rc)
    with pytest.raises(route.RouteError) as ei:
        eng.fold(S, T, OPS, nan)
    assert ei.value.code == route.EINVAL
    # the async call: the host-side arguments at once, a vertex out of range by the next sync
    ds, dt, dv = _dev(S), _dev(T), _dev(c)
    ns, nt = len(S), len(T)
    out = Padded(4 * ns, nt)
    for kw, ops, val in (({}, [], dv), ({}, [0] * 9, dv), ({}, [0, 4], dv), ({}, OPS, None), ({"ld": nt - 1}, OPS, dv),
                         ({"plane": ns * nt - 1}, OPS, dv)):
        with pytest.raises(route.RouteError) as ei:
            eng.fold_async(ds, dt, ops, val, out.t, dispatch=False, **kw)
        assert ei.value.code == route.EINVAL
    assert _sync(route, eng) == route.OK and out.untouched()
    eng.fold_async(_dev(np.zeros(0, np.int32)), dt, OPS, dv, out.t)
    eng.fold_async(ds, _dev(np.zeros(0, np.int32)), OPS, dv, out.t)
    assert _sync(route, eng) == route.OK and out.untouched()
    eng.fold_async(ds, _dev(np.array([0, g.n], np.int32)), OPS, dv, out.t, dispatch=False, ld=nt)
    assert _sync(route, eng) == route.EINVAL
    check(route, "ba60", A[:4], eng=eng)                       # and the context goes on working


def test_failed_entries_leave_the_rest(route):
    """A missing self-loop is SHD_ROUTE_ENOEDGE: those entries NaN in every fold, everything else
    written.  (SHD_ROUTE_EUNREACH needs an unreachable target, and shd_route_create refuses a
    graph that is not strongly connected, topology.c:738-806: no context can show one.)"""
    g, A = hg._graph("ba60_holes")
    got, want, code = check(route, "ba60_holes", np.arange(8))
    assert code == route.ENOEDGE
    assert np.array_equal(np.isnan(got), np.broadcast_to((np.arange(8)[:, None] == np.arange(g.n)) &
                                                          (np.arange(8)[:, None] % 2 == 1), got.shape))


@pytest.mark.parametrize("name,dispatch", [("ba64_ties", False), ("ba80_prefer", True), ("k24", True),
                                           ("ba60_holes", False)])
def test_pairs_equal_the_block(route, name, dispatch):
    """Every entry as a pair, a hundred of them twice, all shuffled: the pair form gives the
    block's entries in the caller's order, failed pairs (ba60_holes: the odd self pairs) in the
    middle of the list."""
    g, A = hg._graph(name)
    eng = route.RouteEngine(g)
    S = np.sort(A[:12]); T = np.arange(g.n, dtype=np.int32)
    rng = np.random.default_rng(12)
    got, want, code = check(route, name, S, dispatch, eng=eng)
    si, ti = np.repeat(np.arange(len(S)), g.n), np.tile(T, len(S))
    dup = rng.choice(len(si), size=100, replace=False)
    si, ti = np.concatenate([si, si[dup]]), np.concatenate([ti, ti[dup]])
    k = rng.permutation(len(si))
    si, ti = si[k], ti[k]
    pairs, pcode = run(route, eng.pair_fold, S[si], ti, OPS, cols(name), dispatch=dispatch)
    assert pcode == code and pairs.shape == (4, len(si))
    assert fr.same(pairs, want[:, si, ti])
    pr, codes = ref(name).pairs(S[si], ti, OPS, cols(name), dispatch)
    assert fr.same(pairs, pr)
    if name == "ba60_holes":
        bad = np.flatnonzero(np.isnan(pairs[0]))
        assert code == route.ENOEDGE and len(bad) >= 1 and bad.min() > 0 and bad.max() < len(si) - 1


# ---- stream order -----------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", [None, "0"])
def test_gated_fold(route, monkeypatch, lds):
    """fold_async behind the timed gate of tests/stream_order.py, in three chunks, in each state
    form: d_val, d_src and d_tgt hold decoys until earlier work of the same non-blocking stream
    writes them, two calls with the canary in between, and the call returns while the gate is
    shut."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_FOLD_LDS", lds)
    S = A[:7].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    ops = [fr.SUM, fr.MIN]
    V = np.array(cols("ba64_ties")[:2])
    R = ref("ba64_ties")
    want, codes = R.rows(S, T, ops, V)
    Sd, Td, Vd = so.decoy_sources(S), so.decoy_targets(T), np.roll(V, 11, axis=1).copy()
    for s, t, v in ((Sd, T, V), (S, Td, V), (S, T, Vd), (Sd, Td, Vd)):   # an early reader gets other folds
        one = R.rows(s, t, ops, v)[0]
        assert so.rows_differ(one[0], want[0]) and so.rows_differ(one[1], want[1])
    eng = route.RouteEngine(g)
    i_s, i_t, i_v = so.In(S, Sd), so.In(T, Td), so.In(V, Vd)
    out = so.Out(2 * ns, nt + 1)
    code = so.gated(route, eng, [i_s, i_t, i_v], [out],
                    lambda sh: eng.fold_async(i_s.t, i_t.t, ops, i_v.t, out.t, stream=sh, dispatch=False, ld=nt + 1),
                    f"fold_async FOLD_LDS={lds}")
    assert (code in codes) if codes else code == route.OK
    assert fr.same(out.f64(nt).reshape(2, ns, nt), want)


# ---- two live contexts ------------------------------------------------------------------------------

def test_two_live_contexts(route):
    """A context at the LDS limit and one of 64 vertices, both in the LDS form, used in turn:
    the dynamic-LDS limit of the kernel is raised once per context, and each still gets its own."""
    big, small = f"sized{fr.lds_max_n()}", "ba64_ties"
    gb, gs = graph(big), graph(small)
    assert fr.fits_lds(gb.n) and fr.fits_lds(gs.n) and fr.layout_total(gb.n) > 100 * fr.layout_total(gs.n)
    eb = route.RouteEngine(gb)
    es = route.RouteEngine(gs)
    Sb, Ss = [0, gb.n - 1, gb.n // 2], hg._graph(small)[1][:8]
    Tb = np.arange(0, gb.n, 3)
    for _ in range(2):
        check(route, big, Sb, eng=eb, ops=[fr.SUM, fr.MIN], T=Tb)
        check(route, small, Ss, eng=es)


# ---- the front end ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ba64_ties", "ba100_attached", "k24"])
def test_front_end_fold_pairs(topo, route, name):
    """fold_pairs over a few hundred pairs in either order: the reference over the stored
    orientation (lower -> higher) under the cache's dispatch; NaN for the pairs the getters
    reject and for self pairs stored as the path to self; nothing cached moves."""
    g, A = hg._graph(name)
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    assert t.edge_jitter() is None                                  # made from arrays: no graphml, no jitter
    rng = np.random.default_rng(len(A))
    P = rng.choice(A, size=(300, 2))
    P[:8, 1] = P[:8, 0]                                              # some self pairs
    loose = np.setdiff1d(np.arange(g.n), A)
    rejected = [(int(loose[0]), int(A[0])), (int(A[1]), int(loose[-1]))] if len(loose) else []
    rejected += [(-1, int(A[0])), (int(A[0]), g.n)]
    P = np.concatenate([P[:150], np.array(rejected), P[150:]])
    sample = [int(x) for x in A[:: max(1, len(A) // 9)]]
    snap = lambda: [t.get_latency(a, b) for a in sample for b in sample]
    was = snap()
    R = ref(name)
    ok = np.array([(min(a, b) >= 0 and max(a, b) < g.n and a in A and b in A) for a, b in P.tolist()])
    assert np.count_nonzero(~ok) == len(rejected)
    lo, hi = P.min(axis=1), P.max(axis=1)
    for k, op in enumerate(OPS):
        got = t.fold_pairs(op, cols(name)[k], P[:, 0], P[:, 1])
        want = np.full(len(P), np.nan)
        want[ok] = R.pairs(lo[ok], hi[ok], [op], [cols(name)[k]], dispatch=True)[0][0]
        assert got.shape == (len(P),) and fr.same(got, want)
        assert np.all(np.isnan(got[~ok])) and np.count_nonzero(~np.isnan(got)) > 200
    for a, b in P[ok][:40].tolist():                                # the same route get_path reports
        p = t.get_path(a, b)
        one = t.fold_pairs(fr.SUM, cols(name)[0], [a], [b])[0]
        assert np.isnan(one) if p is None else one == fr.fold_one(fr.SUM, [float(cols(name)[0][e]) for e in p[1]])
    with pytest.raises(RuntimeError):
        t.fold_pairs(4, cols(name)[0], P[:, 0], P[:, 1])
    assert snap() == was
    t.close()


def test_front_end_edge_jitter(topo, tmp_path):
    """A six-edge graphml with a jitter key: edge_jitter() in document order, and
    fold_pairs(FOLD_SUM, edge_jitter()) the host sum along get_path, the jitter budget of a path."""
    from tests.test_fold import _JKEY, _graphml
    t = topo.Topology.new(_graphml(tmp_path, _JKEY % "<default>1.5</default>"))
    j = t.edge_jitter()
    assert j.tolist() == [0.5, 1.5, 2.25, 0.0, 1.5, 7.0]
    t.attach_all(range(4))
    ps, pt = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    got = t.fold_pairs(fr.SUM, j, ps, pt)
    for a, b, x in zip(ps.tolist(), pt.tolist(), got.tolist()):
        p = t.get_path(a, b)
        if p is None:
            assert a == b != 0 and np.isnan(x)                       # only vertex a (0) has a self-loop
        else:
            assert x == fr.fold_one(fr.SUM, [float(j[e]) for e in p[1]])
    assert np.count_nonzero(~np.isnan(got)) == 13 and got[0] == 0.0
    worst = t.fold_pairs(fr.MAX, j, ps, pt)
    assert np.nanmax(worst) == 7.0                                   # d - b directly: the worst single hop
    t.close()
    t = topo.Topology.new(_graphml(tmp_path, "", name="nokey.xml"))
    assert t.edge_jitter() is None
    t.close()
