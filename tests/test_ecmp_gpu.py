"""GPU: the ECMP link loads -- shd_route_ecmp_loads*, shd_route_pair_ecmp_loads, RouteEngine's
wrappers and the front end's shd_topology_ecmp_link_loads -- against tests/ecmp_ref.py (the
programme in f64, held to exact fractions and to networkx by tests/test_ecmp.py).

Edge loads and transit are compared within ecmp_ref's derived tolerance (the sums across
sources are floating-point atomic adds); the zero pattern, `unrouted` and the codes exactly."""
import functools
import math
import os

import numpy as np
import pytest

from tests import ecmp_ref as er
from tests import shape_graphs as sg
from tests import stream_order as so
from tests import test_hops_gpu as hg
from tests import test_ties_gpu as tg
from tests import ties_ref as tr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
U = 2.0 ** -53


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
    for k in ("SHD_ROUTE_ECMP_LDS", "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)


graph = tg.graph


@functools.lru_cache(maxsize=None)
def ref(name):
    return er.EcmpRef(graph(name))


def same(got, want, rtol):
    """got equals want within rtol relative, element by element, with the same zeros."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(got == 0, want == 0):
        return False
    err = np.abs(got - want)
    print("  worst / u", float(np.max(err[want != 0] / want[want != 0], initial=0.0) / U), "rtol / u", rtol / U)
    return bool(np.all(err <= rtol * want))


def run(route, call, *args, **kw):
    """(edge_load, transit, unrouted, code) of a call, failed entries or not."""
    try:
        return tuple(call(*args, **kw)) + (route.OK,)
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return tuple(err.partial) + (err.code,)


def weights(seed, ns, nt):
    return np.random.default_rng(seed).integers(0, 1 << 20, size=(ns, nt)).astype(np.uint64)


def check(route, name, S, W=None, dispatch=False, T=None, eng=None):
    """eng.ecmp_loads(S, T, W) equals the reference; the code is one the failed entries give."""
    g = graph(name)
    T = np.arange(g.n, dtype=np.int32) if T is None else np.asarray(T, np.int32)
    S = np.asarray(S, np.int32)
    want = ref(name).rows(S, T, W, dispatch)
    rtol = ref(name).tol(S, dispatch=dispatch)
    eng = eng or route.RouteEngine(g)
    got = run(route, eng.ecmp_loads, S, T, W, dispatch=dispatch)
    assert got[0].dtype == np.float64 and got[1].dtype == np.float64
    assert got[0].shape == (g.m,) and got[1].shape == (g.n,)
    assert same(got[0], want[0], rtol) and same(got[1], want[1], rtol)
    assert got[2] == want[2]
    assert (got[3] in want[3]) if want[3] else got[3] == route.OK, (got[3], want[3])
    return got, want


# ---- small goldens ------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", hg.SMALL)
def test_small_goldens(route, name, dispatch, weighted):
    """All attached sources x all vertices, weights NULL and random below 2^20."""
    g, A = hg._graph(name)
    W = weights(g.n, len(A), g.n) if weighted else None
    eng = route.RouteEngine(g)
    got, want = check(route, name, A, W, dispatch, eng=eng)
    R = ref(name).ref
    if name == "k24" and dispatch:            # no sweep: every pair on its direct edge, nothing in transit
        assert R.complete and not got[1].any()
        el = np.zeros(g.m)
        for i, s in enumerate(A.tolist()):
            for t in range(g.n):
                e = R.self_entry(s)[3] if t == s else R.direct_entry(s, t)[3]
                assert e >= 0
                el[e] += float(W[i, t]) if weighted else 1.0
        assert np.array_equal(got[0], el)     # integers below 2^53: exact in any order
    else:
        assert got[1].any()
    if name == "ba80_prefer":                 # adjacent pairs undivided under dispatch
        adj = [(int(s), t) for s in A for t in range(g.n) if t != s and R.is_direct(int(s), t, True)]
        assert len(adj) > 50
        other = run(route, eng.ecmp_loads, A, np.arange(g.n, dtype=np.int32), W, dispatch=not dispatch)
        assert not np.array_equal(other[0], got[0])
    if name == "ba64_ties" and not weighted:  # ties split: loads that are no whole numbers
        assert np.count_nonzero(got[0] != np.floor(got[0])) > 20


# ---- the shape suite ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "lollipop", "star1100", "biclique1030", "dir_grid"])
def test_shapes(route, name):
    """grid: 63 levels and sigma past 2^53; lollipop: 302 levels; star1100: an out-list of more
    than 1,024 arcs on the whole wave, in both sweeps; biclique1030: wide in-lists, most pairs
    tied."""
    g = graph(name)
    S = tg._spread(g.n)
    if name == "biclique1030":
        S = np.array([0, 16, 17, 500, g.n - 1], np.int32)
    got, want = check(route, name, S)
    Rm, D = ref(name).shape(S)
    nl = g.src != g.dst
    deg = np.bincount(np.concatenate([g.src[nl], g.dst[nl]]), minlength=g.n)
    if name == "grid":
        far = ref(name).sigma(0)[g.n - 1]
        assert Rm == 63 and far > 2.0 ** 53 and abs(far - math.comb(63, 31)) <= 64 * U * far
    if name == "lollipop":
        assert Rm == 302
    if name == "star1100":
        assert deg.max() > 1024 and D > 1024
    if name == "biclique1030":
        assert np.count_nonzero(deg > 1024) == 17 and D >= 17
        tied = sum(sum(1 for x in ref(name).sigma(int(s)) if x > 1) for s in S)
        assert tied > len(S) * g.n // 2 and np.count_nonzero(got[0] != np.floor(got[0])) > g.m // 3


@pytest.mark.parametrize("loops", sg.TINY_LOOPS)
@pytest.mark.parametrize("n", sg.TINY_N)
def test_tiny(route, n, loops):
    """Paths of 1 to 9 vertices: SHD_ROUTE_ENOEDGE entries land in unrouted, the rest is written."""
    name = f"tiny{n}_{loops}"
    g = graph(name)
    W = weights(n, n, n) + np.uint64(1)
    got, want = check(route, name, np.arange(n), W)
    noloop = ~np.isin(np.arange(n), g.src[g.src == g.dst])
    assert got[2] == int(np.diag(W)[noloop].sum()) and (got[3] == route.ENOEDGE) == bool(noloop.any())
    if n > 1:
        assert got[0].any()


def test_multigraph(route):
    """ba60 with 10 edges doubled at equal latency: each doubled tight edge carries what its
    twin carries."""
    name = "ba60_multi_equal"
    g = graph(name)
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1
    S = np.arange(g.n, dtype=np.int32)
    got, want = check(route, name, S, eng=eng)
    rtol = ref(name).tol(S)
    key = lambda e: (min(int(g.src[e]), int(g.dst[e])), max(int(g.src[e]), int(g.dst[e])), float(g.latency[e]))
    first = {}
    for e in range(g.m - 10):
        first.setdefault(key(e), e)
    twins = [(first[key(e)], e) for e in range(g.m - 10, g.m)]
    assert len(twins) == 10
    for a, b in twins:
        assert want[0][a] == want[0][b]                     # (an edge on no shortest path: both 0)
        assert abs(got[0][a] - got[0][b]) <= rtol * want[0][a]
    assert sum(want[0][a] > 0 for a, _ in twins) >= 5


def test_unique_paths_equal_the_loads(route):
    """ba90_frac: every listed pair has exactly one shortest path, so the call equals
    shd_route_loads converted to double, exactly."""
    g, A = hg._graph("ba90_frac")
    T = np.arange(g.n, dtype=np.int32)
    cnt = tr.TiesRef(g).rows(A, T)[0]
    assert np.all(cnt[T[None, :] != np.asarray(A)[:, None]] == 1)
    eng = route.RouteEngine(g)
    for W in (None, weights(90, len(A), g.n)):
        for dispatch in (False, True):
            one = run(route, eng.loads, A, T, W, dispatch=dispatch)
            got = run(route, eng.ecmp_loads, A, T, W, dispatch=dispatch)
            assert int(one[0].max()) < 2 ** 53 and one[0].any() and one[1].any()
            assert np.array_equal(got[0], one[0].astype(np.float64))
            assert np.array_equal(got[1], one[1].astype(np.float64))
            assert got[2] == one[2] and got[3] == one[3]


# ---- the state forms --------------------------------------------------------------------------------

@pytest.mark.parametrize("over", [0, 1])
def test_lds_limit(route, over):
    """sized(n) at the largest n whose state layout fits the LDS and at n + 1 (the HBM form)."""
    n = er.lds_max_n() + over
    assert er.fits_lds(n) == (over == 0)
    check(route, f"sized{n}", [0, n - 1, n // 2, 17, n // 3])


@pytest.mark.parametrize("name", ["grid", "ba64_ties"])
def test_hbm_form(route, monkeypatch, name):
    monkeypatch.setenv("SHD_ROUTE_ECMP_LDS", "0")
    g = graph(name)
    check(route, name, tg._spread(g.n, 8) if name == "grid" else hg._graph(name)[1])


def test_hbm_slots_reused(route, monkeypatch):
    """64 sources over the 16 workgroup slots a small scratch budget leaves, forwards and then
    reversed: a workgroup that takes a second source finds nothing of the first."""
    g = graph("ba64_ties")
    stride = er.layout_total(g.n, 2)
    budget = 4 * 16 * stride
    assert budget // (12 * g.n) >= g.n == 64 and budget // 4 // stride == 16
    monkeypatch.setenv("SHD_ROUTE_ECMP_LDS", "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(budget))
    eng = route.RouteEngine(g)
    S = np.arange(g.n, dtype=np.int32)
    W = weights(64, g.n, g.n)
    check(route, "ba64_ties", S, W, eng=eng)
    check(route, "ba64_ties", S[::-1].copy(), W, eng=eng)


@pytest.mark.parametrize("lds", [None, "0"])
def test_three_chunks(route, monkeypatch, lds):
    """SHD_ROUTE_HOPS_SCRATCH of four sources (12 n bytes each): 11 sources take three chunks,
    which add up in the outputs."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 12 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_ECMP_LDS", lds)
    check(route, "ba64_ties", A[:11], weights(11, 11, g.n))


def test_beyond_u16(route):
    """66,000 vertices: u32 order entries, the state in HBM slices."""
    g, A = hg._graph("ring66k")
    assert g.n > 65535 and not er.fits_lds(g.n)
    got, _ = check(route, "ring66k", A)
    assert got[2] == 2 and got[3] == route.ENOEDGE and np.flatnonzero(got[1]).max() > 65535


# ---- the contract -----------------------------------------------------------------------------------

def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def _sync(route, eng):
    try:
        eng.sync()
        return route.OK
    except route.RouteError as err:
        return err.code


def test_add_flag(route):
    """SHD_ROUTE_LOADS_ADD adds on top of pre-filled outputs; without it they are overwritten."""
    g, A = hg._graph("ba64_ties")
    S, T = A[:8], np.arange(g.n, dtype=np.int32)
    W = weights(3, len(S), g.n)
    eng = route.RouteEngine(g)
    (el, trn, un, code), want = check(route, "ba64_ties", S, W, eng=eng)
    rtol = ref("ba64_ties").tol(S) + 2 * U
    out = (np.full(g.m, 9.5), np.full(g.n, 9.5), np.full(1, 9, np.uint64))
    again = run(route, eng.ecmp_loads, S, T, W, dispatch=False, out=out)
    assert again[0] is out[0] and same(again[0], want[0], rtol) and same(again[1], want[1], rtol) and again[2] == un
    out = (np.full(g.m, 9.5), np.full(g.n, 9.5), np.full(1, 9, np.uint64))
    added = run(route, eng.ecmp_loads, S, T, W, dispatch=False, out=out, add=True)
    assert same(added[0], want[0] + 9.5, rtol) and same(added[1], want[1] + 9.5, rtol) and added[2] == un + 9
    ps, pt = np.repeat(S, g.n), np.tile(T, len(S))
    more = run(route, eng.pair_ecmp_loads, ps, pt, W.reshape(-1), dispatch=False, out=out, add=True)
    assert same(more[0], 2 * want[0] + 9.5, rtol) and same(more[1], 2 * want[1] + 9.5, rtol) and more[2] == 2 * un + 9
    back = run(route, eng.pair_ecmp_loads, ps, pt, W.reshape(-1), dispatch=False, out=out)
    assert same(back[0], want[0], rtol) and same(back[1], want[1], rtol) and back[2] == un


def test_null_outputs_and_row_stride(route):
    """shd_route_ecmp_loads_async: every combination of NULL outputs (a NULL one stays
    untouched), a weight row stride above nt, repeated targets, ADD, and an out-of-range target
    raised by the next sync."""
    import torch
    g, A = hg._graph("ba64_ties")
    eng = route.RouteEngine(g)
    S = A[:10].astype(np.int32)
    T = np.concatenate([np.arange(g.n), [5, 5, 17]]).astype(np.int32)
    nt, ld = len(T), len(T) + 7
    W = weights(64, len(S), nt)
    Wp = np.full((len(S), ld), 77, np.uint64)
    Wp[:, :nt] = W
    want = ref("ba64_ties").rows(S, T, W)
    rtol = ref("ba64_ties").tol(S, mult=3)
    ds, dt, dw = _dev(S), _dev(T), _dev(Wp)
    dev = torch.device("cuda", 0)
    for mask in range(8):
        de = torch.full((g.m,), 7.25, dtype=torch.float64, device=dev)
        dtr = torch.full((g.n,), 7.25, dtype=torch.float64, device=dev)
        du = torch.full((1,), 7, dtype=torch.int64, device=dev)
        eng.ecmp_loads_async(ds, dt, dw, de if mask & 1 else None, dtr if mask & 2 else None,
                             du if mask & 4 else None, dispatch=False, ld=ld)
        code = _sync(route, eng)
        assert (code in want[3]) if want[3] else code == route.OK
        e, t, u = de.cpu().numpy(), dtr.cpu().numpy(), int(du.cpu().numpy().view(np.uint64)[0])
        assert same(e, want[0], rtol) if mask & 1 else np.all(e == 7.25)
        assert same(t, want[1], rtol) if mask & 2 else np.all(t == 7.25)
        assert u == (want[2] if mask & 4 else 7)
    # ADD on the device, unit weights on top
    one = ref("ba64_ties").rows(S, T, None)
    eng.ecmp_loads_async(ds, dt, None, de, dtr, du, dispatch=False, add=True)
    _sync(route, eng)
    assert same(de.cpu().numpy(), want[0] + one[0], rtol + 2 * U) and same(dtr.cpu().numpy(), want[1] + one[1], rtol + 2 * U)
    assert int(du.cpu().numpy().view(np.uint64)[0]) == want[2] + one[2]
    # the host form with a NULL output
    el, trn, un, _ = run(route, eng.ecmp_loads, S, T, W, dispatch=False, out=(None, np.full(g.n, 3.0), np.zeros(1, np.uint64)))
    assert el is None and same(trn, want[1], rtol) and un == want[2]
    # ld < nt is refused at once; a vertex out of range comes back from the device
    with pytest.raises(route.RouteError) as ei:
        eng.ecmp_loads_async(ds, dt, dw, de, dtr, du, dispatch=False, ld=nt - 1)
    assert ei.value.code == route.EINVAL
    t0 = int(np.setdiff1d(np.arange(g.n), S)[0])
    eng.ecmp_loads_async(ds, _dev(np.array([t0, g.n], np.int32)), None, de, dtr, du, dispatch=False)
    assert _sync(route, eng) == route.EINVAL
    check(route, "ba64_ties", S, eng=eng)                       # and the context goes on working


def test_empty_and_invalid(route):
    """ns == 0 / nt == 0 zero the outputs; a vertex out of range is EINVAL with nothing written."""
    import torch
    g, A = hg._graph("ba60")
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    dirty = lambda: (np.full(g.m, 9.0), np.full(g.n, 9.0), np.full(1, 9, np.uint64))
    for S2, T2 in (([], T), (A[:4], [])):
        el, trn, un = eng.ecmp_loads(S2, T2, None, dispatch=False, out=dirty())
        assert not el.any() and not trn.any() and un == 0
        out = dirty()
        eng.ecmp_loads(S2, T2, None, dispatch=False, out=out, add=True)
        assert np.all(out[0] == 9.0) and np.all(out[1] == 9.0) and out[2][0] == 9
    el, trn, un = eng.pair_ecmp_loads([], [], None, out=dirty())
    assert not el.any() and not trn.any() and un == 0
    dev = torch.device("cuda", 0)
    de = torch.full((g.m,), 9.0, dtype=torch.float64, device=dev)
    du = torch.full((1,), 9, dtype=torch.int64, device=dev)
    eng.ecmp_loads_async(_dev(np.zeros(0, np.int32)), _dev(T), None, de, None, du)
    assert _sync(route, eng) == route.OK and not de.cpu().numpy().any() and int(du.cpu()[0]) == 0
    for bad in (-1, g.n):
        for call, args in ((eng.ecmp_loads, ([A[0], bad], T)), (eng.ecmp_loads, (A[:2], [0, bad])),
                           (eng.pair_ecmp_loads, ([A[0], bad], [1, 2])), (eng.pair_ecmp_loads, ([A[0], A[1]], [1, bad]))):
            out = dirty()
            with pytest.raises(route.RouteError) as ei:
                call(*args, out=out)
            assert ei.value.code == route.EINVAL
            assert np.all(out[0] == 9.0) and np.all(out[1] == 9.0) and out[2][0] == 9


@pytest.mark.parametrize("name,dispatch", [("ba64_ties", False), ("ba80_prefer", True), ("k24", True)])
def test_pairs_equal_the_block(route, name, dispatch):
    """Every entry as a pair, some split into two pairs of half the weight, all shuffled: the
    pair form gives the block's loads."""
    g, A = hg._graph(name)
    eng = route.RouteEngine(g)
    S = np.sort(A[:12]); T = np.arange(g.n, dtype=np.int32)
    rng = np.random.default_rng(12)
    W = weights(12, len(S), g.n)
    (el, trn, un, code), want = check(route, name, S, W, dispatch, eng=eng)
    ps = np.repeat(S, g.n); pt = np.tile(T, len(S)); pw = W.reshape(-1).copy()
    dup = rng.choice(len(ps), size=100, replace=False)
    half = pw[dup] // np.uint64(2)
    pw[dup] -= half
    ps = np.concatenate([ps, ps[dup]]); pt = np.concatenate([pt, pt[dup]]); pw = np.concatenate([pw, half])
    k = rng.permutation(len(ps))
    rtol = ref(name).tol(S, mult=2, dispatch=dispatch)
    got = run(route, eng.pair_ecmp_loads, ps[k], pt[k], pw[k], dispatch=dispatch)
    assert same(got[0], want[0], rtol) and same(got[1], want[1], rtol) and got[2] == un
    assert (got[3] in want[3]) if want[3] else got[3] == route.OK
    pr = ref(name).pairs(ps[k], pt[k], pw[k], dispatch)
    assert same(got[0], pr[0], rtol) and same(got[1], pr[1], rtol) and got[2] == pr[2]


# ---- stream order -----------------------------------------------------------------------------------

@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("lds", [None, "0"])
def test_gated_ecmp_loads(route, monkeypatch, lds, add):
    """ecmp_loads_async behind the timed gate of tests/stream_order.py, in three chunks, in each
    state form, with and without ADD: decoy inputs until the gate opens, two calls with the
    canary in between, and the call returns while the gate is shut."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 12 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_ECMP_LDS", lds)
    S = A[:11].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    R = ref("ba64_ties")
    W = weights(5, ns, nt)
    Wp = np.zeros((ns, nt + 1), np.uint64); Wp[:, :nt] = W
    want = R.rows(S, T, W)
    rtol = R.tol(S) + 2 * U
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    Wd = np.roll(W, 7, axis=1)
    Wdp = np.zeros_like(Wp); Wdp[:, :nt] = Wd
    for s, t, w in ((Sd, T, W), (S, Td, W), (S, T, Wd), (Sd, Td, Wd)):   # an early reader gets other loads
        one = R.rows(s, t, w)
        assert not same(one[0], want[0], rtol) and not same(one[1], want[1], rtol)
    rng = np.random.default_rng(7)
    base = [rng.integers(1, 1 << 20, size=k).astype(np.float64) for k in (g.m, g.n)]
    base.append(rng.integers(1, 1 << 40, size=1).astype(np.uint64))
    eng = route.RouteEngine(g)
    i_s, i_t, i_w = so.In(S, Sd), so.In(T, Td), so.In(Wp, Wdp)
    outs = [so.Out(1, g.m), so.Out(1, g.n), so.Out(1, 1, i64=True)]
    one_more = lambda b: b + (np.uint64(1) if b.dtype == np.uint64 else 1.0)
    accum = [so.In(b[None, :], one_more(b)[None, :], into=o.t) for b, o in zip(base, outs)] if add else []
    code = so.gated(route, eng, [i_s, i_t, i_w], outs,
                    lambda sh: eng.ecmp_loads_async(i_s.t, i_t.t, i_w.t, outs[0].t, outs[1].t, outs[2].t, stream=sh,
                                                    dispatch=False, ld=nt + 1, add=add),
                    f"ecmp_loads_async ECMP_LDS={lds} add={int(add)}", accum=accum)
    assert (code in want[3]) if want[3] else code == route.OK
    el, trn = outs[0].f64(g.m)[0], outs[1].f64(g.n)[0]
    un = int(outs[2].snap_bits(1)[0].view(np.uint64)[0])
    assert same(el, want[0] + base[0] if add else want[0], rtol)
    assert same(trn, want[1] + base[1] if add else want[1], rtol)
    assert un == (want[2] + int(base[2][0]) if add else want[2])


# ---- two live contexts ------------------------------------------------------------------------------

def test_two_live_contexts(route):
    """A context at the LDS limit and one of 64 vertices, both in the LDS form, used in turn:
    the dynamic-LDS limit of the kernel is the last context's, and each still gets its own."""
    big, small = f"sized{er.lds_max_n()}", "ba64_ties"
    gb, gs = graph(big), graph(small)
    assert er.fits_lds(gb.n) and er.fits_lds(gs.n) and er.layout_total(gb.n) > 50 * er.layout_total(gs.n)
    eb = route.RouteEngine(gb)
    es = route.RouteEngine(gs)
    Sb, Ss = [0, gb.n - 1, gb.n // 2, 17, gb.n // 3], hg._graph(small)[1][:8]
    for _ in range(2):
        check(route, big, Sb, eng=eb)
        check(route, small, Ss, eng=es)


# ---- the front end ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ba64_ties", "ba100_attached", "k24"])
def test_front_end_ecmp_link_loads(topo, name):
    """Packet counters on a few hundred stored pairs, one past 2^32: the ECMP totals equal the
    reference over the stored pairs (lower -> higher) under the cache's dispatch; all zero
    before the first fill; nothing cached moves."""
    g, A = hg._graph(name)
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    z = t.ecmp_link_loads()
    assert z[0].dtype == np.float64 and len(z[0]) == g.m and len(z[1]) == g.n
    assert not z[0].any() and not z[1].any() and z[2] == 0           # before the fill
    assert t.get_latency(int(A[0]), int(A[1])) >= 0
    z = t.ecmp_link_loads()
    assert not z[0].any() and not z[1].any() and z[2] == 0           # no packets yet
    rng = np.random.default_rng(len(A))
    P = rng.choice(A, size=(300, 2))
    P[:6, 1] = P[:6, 0]                                              # some self pairs
    for (a, b), k in zip(P.tolist(), rng.integers(1, 1000, size=len(P)).tolist()):
        t.add_path_packets(a, b, k)
    hot = P[6:][P[6:, 0] != P[6:, 1]][0]
    t.add_path_packets(int(hot[0]), int(hot[1]), 2 ** 32 + 5)
    sample = [int(x) for x in A[:: max(1, len(A) // 9)]]
    snap = lambda: ([t.get_latency(a, b) for a in sample for b in sample],
                    [t.packet_count(a, b) for a in sample for b in sample])
    was = snap()
    ps, pt, pw = [], [], []
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            c = t.packet_count(a, b)
            if c:
                ps.append(a); pt.append(b); pw.append(c)
    assert len(ps) > 100 and max(pw) > 2 ** 32
    R = ref(name)
    want = R.pairs(ps, pt, pw, dispatch=True)
    got = t.ecmp_link_loads()
    rtol = R.tol(sorted(set(ps)), dispatch=True)
    assert same(got[0], want[0], rtol) and same(got[1], want[1], rtol) and got[2] == want[2]
    one = t.link_loads()
    if name == "k24":                                                # complete under dispatch: direct edges only
        assert not got[1].any() and np.array_equal(got[0], one[0].astype(np.float64))
    else:
        assert got[1].any() and (name != "ba64_ties" or not np.array_equal(got[0], one[0].astype(np.float64)))
    assert snap() == was
    t.close()
