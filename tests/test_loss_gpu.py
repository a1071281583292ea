"""GPU: the link loss calls -- shd_route_loss*, shd_route_pair_loss, RouteEngine's wrappers and the
front end's shd_topology_link_loss -- against tests/loss_ref.py (the programme of the header in
Python floats and in exact fractions, held together by tests/test_loss.py).

A call in which no element takes more than two addends (one source with distinct targets is
one) must equal the f64 programme bit for bit; every other call must lie within
(R + 4 + A) * 2^-52 relative of the exact fractions, R and A counted by the reference, and an
exact 0 must be 0.  unrouted is always exact."""
import functools

import numpy as np
import pytest

from tests import loss_ref as lr
from tests import shape_graphs as sg
from tests import stream_order as so
from tests import test_hops_gpu as hg
from tests import test_loss as tl
from tests import test_ties_gpu as tg

pytestmark = pytest.mark.gpu


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
    for k in ("SHD_ROUTE_LOSS_LDS", "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in tl.GRAPHS:
        return tl.graph(name)
    if name == "grid_dec":
        return lr.decimal_losses(sg.get("grid"), 32, vloss=False)
    if name == "ring66k_dec":
        return lr.decimal_losses(hg._graph("ring66k")[0], 66, vloss=False)
    if name.startswith("sized") and name.endswith("_dec"):
        return lr.decimal_losses(sg.sized(int(name[5:-4])), 7)
    return tg.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return lr.LossRef(graph(name))


def run(route, call, *args, **kw):
    """((edge_reach, edge_drop, vertex_drop, delivered, unrouted), code) of a call, failed entries or not."""
    try:
        return call(*args, **kw), route.OK
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return err.partial, err.code


def compare(route, got, code, f64, exact):
    """The four outputs, unrouted and the code of a call against the reference's two runs."""
    assert (exact.unrouted, exact.codes, exact.R, exact.A) == (f64.unrouted, f64.codes, f64.R, f64.A)
    assert got[4] == exact.unrouted
    assert (code in exact.codes) if exact.codes else code == route.OK, (code, exact.codes)
    for k, (g, a, b) in enumerate(zip(got[:4], f64.arrays(), exact.outs())):
        assert g.dtype == np.float64 and g.shape == a.shape
        if exact.A <= 2:
            bad = np.flatnonzero(g != a)
            assert np.array_equal(g, a), (lr.NAMES[k], len(bad), bad[:5].tolist(), g[bad[:5]].tolist(),
                                          a[bad[:5]].tolist())
        else:
            assert lr.close(g, b, exact.R, exact.A), (lr.NAMES[k], exact.R, exact.A)


def check(route, name, S, W=None, dispatch=False, T=None, eng=None):
    """eng.loss(S, T, W) against the reference; returns (got, code, exact)."""
    g = graph(name)
    T = np.arange(g.n, dtype=np.int32) if T is None else np.asarray(T, np.int32)
    S = np.asarray(S, np.int32)
    R = ref(name)
    f64, exact = R.block(S, T, W, dispatch), R.block(S, T, W, dispatch, exact=True)
    eng = eng or route.RouteEngine(g)
    got, code = run(route, eng.loss, S, T, W, dispatch=dispatch)
    compare(route, got, code, f64, exact)
    return got, code, exact


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


def _outs(g, fill=7.25, ufill=7):
    import torch
    dev = torch.device("cuda", 0)
    return ([torch.full((k,), fill, dtype=torch.float64, device=dev) for k in (g.m, g.m, g.n, g.n)]
            + [torch.full((1,), ufill, dtype=torch.int64, device=dev)])


def _host(outs):
    return [o.cpu().numpy() for o in outs[:4]] + [int(outs[4].cpu().numpy().view(np.uint64)[0])]


# ---- every form on the small builders --------------------------------------------------------------

@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", tl.GRAPHS)
def test_every_form(route, name, dispatch):
    """The weighted block, the same entries as shuffled pairs with a hundred repeats, and the
    async call with a weight row stride above nt, on one context."""
    g = graph(name)
    eng = route.RouteEngine(g)
    S, T = tl.sources(name), np.arange(g.n, dtype=np.int32)
    W = tl.weights(name, len(S), len(T))
    got, code, exact = check(route, name, S, W, dispatch, eng=eng)
    if g.n > 2:
        assert np.count_nonzero(got[0]) >= 2 and got[3].sum() > 0
    R = ref(name)
    rng = np.random.default_rng(len(S))
    ps, pt, pw = np.repeat(S, len(T)), np.tile(T, len(S)), W.ravel()
    k = np.concatenate([rng.permutation(len(ps)), rng.integers(0, len(ps), size=100)])
    pg, pcode = run(route, eng.pair_loss, ps[k], pt[k], pw[k], dispatch=dispatch)
    compare(route, pg, pcode, R.pairs(ps[k], pt[k], pw[k], dispatch),
            R.pairs(ps[k], pt[k], pw[k], dispatch, exact=True))
    ld = len(T) + 5
    Wp = np.full((len(S), ld), 77, np.uint64)
    Wp[:, :len(T)] = W
    outs = _outs(g)
    eng.loss_async(_dev(S), _dev(T), _dev(Wp), *outs, dispatch=dispatch, ld=ld)
    acode = _sync(route, eng)
    compare(route, _host(outs), acode, R.block(S, T, W, dispatch), exact)


@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", tl.GRAPHS)
def test_one_source_is_the_f64_programme(route, name, dispatch):
    """One source, distinct targets, weighted: no element takes more than two addends, and the
    outputs equal the plain f64 programme bit for bit."""
    g = graph(name)
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    for s in tl.sources(name, 3).tolist():
        W = tl.weights(name, 1, g.n, s)
        got, code, exact = check(route, name, [s], W, dispatch, eng=eng)
        assert exact.A <= 2


@pytest.mark.parametrize("name", ["star1100", "lollipop", "grid", "dir_grid", "biclique1030", "grid_dec"])
def test_shapes(route, name):
    """star1100: a level wider than the workgroup; lollipop: 300 levels; grid: ties; dir_grid:
    directed, failed self entries; biclique1030: wide in-lists; grid_dec: decimal losses."""
    g = graph(name)
    S = tg._spread(g.n)
    if name == "biclique1030":
        S = np.array([0, 16, 17, 500, g.n - 1], np.int32)
    if name == "star1100":
        S = np.array([0, 1, 2, 600, g.n - 1], np.int32)
    if name == "dir_grid":
        S = np.array([0, 1, 52, 130, g.n - 1], np.int32)        # 1, 52 and 130 have no self-loop
    got, code, exact = check(route, name, S, tl.weights(name, len(S), g.n, 4))
    if name == "lollipop":
        assert exact.R >= 300
    if name == "dir_grid":
        assert code == route.ENOEDGE and got[4] > 0
    check(route, name, S[:1])


# ---- identities on the device ----------------------------------------------------------------------

def test_zero_loss_equals_the_loads(route):
    """No loss anywhere, all sources x all vertices, weighted: edge_reach is shd_route_loads'
    edge load converted to double, exactly (integer addends below 2^53 add exactly in any
    order); nothing is dropped and everything routed is delivered."""
    g = graph("ba60_zero")
    eng = route.RouteEngine(g)
    S = T = np.arange(g.n, dtype=np.int32)
    W = tl.weights("ba60_zero", g.n, g.n, 5)
    for dispatch in (False, True):
        got, code = run(route, eng.loss, S, T, W, dispatch=dispatch)
        (el, _, un), lcode = run(route, eng.loads, S, T, W, dispatch=dispatch)
        assert code == lcode and got[4] == un
        assert np.array_equal(got[0], el.astype(np.float64)) and el.max() > 1000
        assert not got[1].any() and not got[2].any()
        assert got[3].sum() == float(int(W.sum(dtype=np.uint64)) - un)


@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", ["ba60", "ba64_ties", "ba80_prefer", "dir40", "ba90_frac", "k24", "ba60_multi_equal"])
def test_unit_weights_deliver_the_rows_rel(route, name, dispatch):
    """One source, unit weights, a graph without vertex loss: delivered[t] is rel of
    shd_route_rows, bit for bit (a failed entry delivers nothing)."""
    g = graph(name)
    from tests import fold_ref as fr
    assert fr.no_vertex_loss(g)
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    for s in tl.sources(name, 3).tolist():
        got, code = run(route, eng.loss, [s], T, None, dispatch=dispatch)
        (_, rel, _), rcode = run(route, eng.rows, [s], T, dispatch=dispatch)
        assert code == rcode
        assert np.array_equal(got[3], np.nan_to_num(rel[0])) and np.count_nonzero(got[3]) >= g.n - 1


@pytest.mark.parametrize("name", ["ba120_vloss", "ba60_dec", "multi389_vloss", "ba64_ties"])
def test_unit_weights_deliver_the_ties_rel(route, name):
    """The same delivered equals rel_lo of shd_route_ties wherever its count is 1, vertex loss included."""
    g = graph(name)
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    seen = 0
    for s in tl.sources(name, 3).tolist():
        got, code = run(route, eng.loss, [s], T, None, dispatch=False)
        try:
            cnt, lo, _ = eng.ties([s], T, dispatch=False)
        except route.RouteError as err:
            cnt, lo, _ = err.partial
        one = cnt[0] == 1
        assert np.array_equal(got[3][one], lo[0][one])
        seen += int(one.sum())
    assert seen > g.n


# ---- the state forms --------------------------------------------------------------------------------

@pytest.mark.parametrize("over", [0, 1])
def test_lds_limit(route, over):
    """sized(n) with decimal losses at the largest n whose state fits the LDS and at n + 1 (the HBM form)."""
    n = lr.lds_max_n() + over
    assert lr.fits_lds(n) == (over == 0) and lr.lds_max_n() == 7442
    S = [0, n - 1, n // 2]
    T = np.arange(0, n, 3)
    check(route, f"sized{n}_dec", S, tl.weights("sized", len(S), len(T), 6), T=T)


@pytest.mark.parametrize("name", ["grid_dec", "ba64_ties", "ba60_dec"])
def test_hbm_form(route, monkeypatch, name):
    monkeypatch.setenv("SHD_ROUTE_LOSS_LDS", "0")
    g = graph(name)
    S = tg._spread(g.n, 8) if name == "grid_dec" else tl.sources(name)
    check(route, name, S, tl.weights(name, len(S), g.n, 7))
    check(route, name, S[:1])


def test_beyond_u16(route):
    """66,000 vertices with decimal losses: u32 order entries, the state in HBM slices."""
    g, A = hg._graph("ring66k")
    assert g.n > 65535 and not lr.fits_lds(g.n) and len(A) <= 4
    T = np.unique(np.concatenate([np.arange(0, g.n, 41), np.arange(g.n - 40, g.n), A])).astype(np.int32)
    got, code, exact = check(route, "ring66k_dec", A, tl.weights("ring", len(A), len(T), 8), T=T)
    assert code == route.ENOEDGE and got[4] > 0 and np.flatnonzero(got[3]).max() > 65535
    check(route, "ring66k_dec", A[:1], T=T)


def test_hbm_slices_reused(route, monkeypatch):
    """64 sources over the 16 slices a small scratch budget leaves, as pairs: the sources
    16 k .. 16 k + 15 have every vertex for a target when k is even and one target when k is odd,
    so a slice goes from a source with many reached entries to one with few and back, and
    nothing of the one before (sums, level offsets, order list, products) may survive."""
    name = "ba64_ties"
    g = graph(name)
    stride = lr.layout_total(g.n, 2)
    budget = 4 * 16 * stride
    assert budget // (16 * g.n) >= g.n == 64 and budget // 4 // stride == 16
    monkeypatch.setenv("SHD_ROUTE_LOSS_LDS", "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(budget))
    ps, pt = [], []
    for s in range(g.n):
        ts = range(g.n) if (s // 16) % 2 == 0 else [(s * 7 + 3) % g.n]
        ps += [s] * len(ts); pt += list(ts)
    pw = tl.weights(name, 1, len(ps), 9)[0]
    eng = route.RouteEngine(g)
    R = ref(name)
    for order in (slice(None), slice(None, None, -1)):
        a, b, w = np.array(ps)[order], np.array(pt)[order], pw[order]
        got, code = run(route, eng.pair_loss, a, b, w, dispatch=False)
        compare(route, got, code, R.pairs(a, b, w), R.pairs(a, b, w, exact=True))


@pytest.mark.parametrize("lds", [None, "0"])
def test_three_chunks(route, monkeypatch, lds):
    """SHD_ROUTE_HOPS_SCRATCH of three sources (16 n bytes each): 7 sources take three chunks,
    which add up in the outputs."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_LOSS_LDS", lds)
    check(route, "ba64_ties", A[:7], tl.weights("ba64_ties", 7, g.n, 10))


# ---- the contract -----------------------------------------------------------------------------------

def test_null_outputs(route):
    """shd_route_loss_async with every combination of NULL outputs: a NULL one stays untouched,
    the others are the full call's; then the host forms with NULL outputs."""
    name = "ba60_dec"
    g = graph(name)
    eng = route.RouteEngine(g)
    S = tl.sources(name)[:10]
    T = np.concatenate([np.arange(g.n), [5, 5, 17]]).astype(np.int32)      # repeated targets are summed first
    W = tl.weights(name, len(S), len(T), 11)
    R = ref(name)
    f64, exact = R.block(S, T, W), R.block(S, T, W, exact=True)
    ds, dt, dw = _dev(S), _dev(T), _dev(W)
    for mask in range(32):
        outs = _outs(g)
        eng.loss_async(ds, dt, dw, *[o if mask >> k & 1 else None for k, o in enumerate(outs)], dispatch=False)
        code = _sync(route, eng)
        assert (code in exact.codes) if exact.codes else code == route.OK
        h = _host(outs)
        for k in range(4):
            if mask >> k & 1:
                assert lr.close(h[k], exact.outs()[k], exact.R, exact.A), (mask, k)
            else:
                assert np.all(h[k] == 7.25), (mask, k)
        assert h[4] == (exact.unrouted if mask & 16 else 7)
    for mask in (0, 5, 10, 31):
        out = [np.full(k, 3.0) if mask >> j & 1 else None for j, k in enumerate((g.m, g.m, g.n, g.n))]
        out.append(np.full(1, 3, np.uint64) if mask & 16 else None)
        for call, args in ((eng.loss, (S, T, W)),
                           (eng.pair_loss, (np.repeat(S, len(T)), np.tile(T, len(S)), W.ravel()))):
            got, code = run(route, call, *args, dispatch=False, out=list(out))
            for k in range(4):
                assert (got[k] is None) if out[k] is None else lr.close(got[k], exact.outs()[k], exact.R, exact.A)
            assert got[4] == (exact.unrouted if mask & 16 else None)
    assert f64.A > 2


def test_add_flag(route):
    """SHD_ROUTE_LOADS_ADD adds on top of non-zero outputs (one more addend each); without it
    they are overwritten."""
    name = "ba60_dec"
    g = graph(name)
    eng = route.RouteEngine(g)
    S, T = tl.sources(name)[:8], np.arange(g.n, dtype=np.int32)
    W = tl.weights(name, len(S), g.n, 12)
    R = ref(name)
    rng = np.random.default_rng(12)
    init = [rng.integers(1, 1000, size=k) / 8.0 for k in (g.m, g.m, g.n, g.n)]
    fresh = lambda: [a.copy() for a in init] + [np.full(1, 9, np.uint64)]
    exact, plus = R.block(S, T, W, exact=True), R.block(S, T, W, exact=True, init=init)
    assert plus.A == exact.A + 1
    got, _ = run(route, eng.loss, S, T, W, dispatch=False, out=fresh())
    compare(route, got, route.OK, R.block(S, T, W), exact)
    got, _ = run(route, eng.loss, S, T, W, dispatch=False, out=fresh(), add=True)
    assert got[4] == exact.unrouted + 9
    for k in range(4):
        assert lr.close(got[k], plus.outs()[k], plus.R, plus.A)
    got, _ = run(route, eng.pair_loss, np.repeat(S, g.n), np.tile(T, len(S)), W.ravel(), dispatch=False, out=fresh(),
                 add=True)
    for k in range(4):
        assert lr.close(got[k], plus.outs()[k], plus.R, plus.A)
    outs = [_dev(a) for a in init] + [_dev(np.full(1, 9, np.uint64))]
    eng.loss_async(_dev(S), _dev(T), _dev(W), *outs, dispatch=False, add=True)
    assert _sync(route, eng) == route.OK
    h = _host(outs)
    assert h[4] == exact.unrouted + 9
    for k in range(4):
        assert lr.close(h[k], plus.outs()[k], plus.R, plus.A)


def test_empty_and_invalid(route):
    """ns == 0, nt == 0 and npairs == 0 zero the outputs (and leave them under ADD); a vertex
    out of range is EINVAL with nothing written."""
    g, A = hg._graph("ba60")
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    dirty = lambda: [np.full(k, 9.0) for k in (g.m, g.m, g.n, g.n)] + [np.full(1, 9, np.uint64)]
    clean = lambda o: not any(a.any() for a in o[:4])
    kept = lambda o: all(np.all(a == 9.0) for a in o[:4]) and o[4][0] == 9
    for S2, T2 in (([], T), (A[:4], [])):
        got = eng.loss(S2, T2, None, dispatch=False, out=dirty())
        assert clean(got) and got[4] == 0
        out = dirty()
        eng.loss(S2, T2, None, dispatch=False, out=out, add=True)
        assert kept(out)
    got = eng.pair_loss([], [], None, out=dirty())
    assert clean(got) and got[4] == 0
    outs = _outs(g)
    eng.loss_async(_dev(np.zeros(0, np.int32)), _dev(T), None, *outs)
    assert _sync(route, eng) == route.OK
    h = _host(outs)
    assert clean(h) and h[4] == 0
    outs = _outs(g)
    eng.loss_async(_dev(A[:2].astype(np.int32)), _dev(np.zeros(0, np.int32)), None, *outs)
    assert _sync(route, eng) == route.OK and clean(_host(outs)) and _host(outs)[4] == 0
    for bad in (-1, g.n):
        for call, args in ((eng.loss, ([A[0], bad], T)), (eng.loss, (A[:2], [0, bad])),
                           (eng.pair_loss, ([A[0], bad], [1, 2])), (eng.pair_loss, ([A[0], A[1]], [1, bad]))):
            out = dirty()
            with pytest.raises(route.RouteError) as ei:
                call(*args, out=out)
            assert ei.value.code == route.EINVAL and kept(out)
    outs = _outs(g)
    with pytest.raises(route.RouteError) as ei:
        eng.loss_async(_dev(A[:2].astype(np.int32)), _dev(T), None, *outs, ld=g.n - 1)
    assert ei.value.code == route.EINVAL and all(np.all(a == 7.25) for a in _host(outs)[:4])
    eng.loss_async(_dev(A[:2].astype(np.int32)), _dev(np.array([0, g.n], np.int32)), None, *outs, dispatch=False)
    assert _sync(route, eng) == route.EINVAL
    check(route, "ba60", A[:4], eng=eng)                        # and the context goes on working


def test_failed_zero_and_huge_weights(route):
    """ba60 without the odd vertices' self-loops: a failed self entry returns ENOEDGE at the end,
    adds its weight to unrouted alone and leaves every other element as the reference has it;
    zero weights add nothing, and a failed entry of weight 0 still fails; one entry of 2^60
    packets is converted to double once."""
    name = "ba60_holes"
    g = graph(name)
    eng = route.RouteEngine(g)
    T = np.arange(g.n, dtype=np.int32)
    S = np.arange(8, dtype=np.int32)
    W = tl.weights(name, len(S), g.n, 13)
    got, code, exact = check(route, name, S, W, eng=eng)
    assert code == route.ENOEDGE and got[4] == int(sum(int(W[i, i]) for i in range(8) if i % 2))
    Z = np.zeros((1, g.n), np.uint64)
    got, code, _ = check(route, name, [3], Z, eng=eng)          # all weights zero, the self entry fails all the same
    assert code == route.ENOEDGE and got[4] == 0 and not any(a.any() for a in got[:4])
    got, code, _ = check(route, name, [2], Z, eng=eng)
    assert code == route.OK and not any(a.any() for a in got[:4])
    H = tl.weights(name, 1, g.n, 14)
    far = int(np.argmax(ref(name).ref._chains(4)[0]))
    H[0, far] = np.uint64((1 << 60) + 12345)
    got, code, exact = check(route, name, [4], H, eng=eng)
    assert exact.A <= 2 and got[3][far] > 2.0 ** 59
    pg, pcode = run(route, eng.pair_loss, [4, 4, 5], [far, far, 5], np.array([1 << 60, 1 << 60, 0], np.uint64),
                    dispatch=False)
    assert pcode == route.ENOEDGE and pg[4] == 0 and pg[0].max() > 2.0 ** 60


# ---- stream order -----------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", [None, "0"])
def test_gated_loss(route, monkeypatch, lds):
    """loss_async behind the timed gate of tests/stream_order.py, in three chunks, in each state
    form: decoy inputs until the gate opens, two calls with the canary in between, and the call
    returns while the gate is shut."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_LOSS_LDS", lds)
    S = A[:7].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    R = ref(name)
    W = tl.weights(name, ns, nt, 15)
    Wp = np.zeros((ns, nt + 1), np.uint64); Wp[:, :nt] = W
    exact = R.block(S, T, W, exact=True)
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    Wd = np.roll(W, 7, axis=1)
    Wdp = np.zeros_like(Wp); Wdp[:, :nt] = Wd
    for s, t, w in ((Sd, T, W), (S, Td, W), (S, T, Wd), (Sd, Td, Wd)):   # an early reader gets other totals
        one = R.block(s, t, w)
        assert not lr.close(one.edge_reach, exact.edge_reach, exact.R, exact.A)
        assert not lr.close(one.delivered, exact.delivered, exact.R, exact.A)
    eng = route.RouteEngine(g)
    i_s, i_t, i_w = so.In(S, Sd), so.In(T, Td), so.In(Wp, Wdp)
    outs = [so.Out(1, g.m), so.Out(1, g.m), so.Out(1, g.n), so.Out(1, g.n), so.Out(1, 1, i64=True)]
    code = so.gated(route, eng, [i_s, i_t, i_w], outs,
                    lambda sh: eng.loss_async(i_s.t, i_t.t, i_w.t, *[o.t for o in outs], stream=sh, dispatch=False,
                                              ld=nt + 1),
                    f"loss_async LOSS_LDS={lds}")
    assert (code in exact.codes) if exact.codes else code == route.OK
    got = [o.f64(k)[0] for o, k in zip(outs[:4], (g.m, g.m, g.n, g.n))]
    got.append(int(outs[4].snap_bits(1)[0].view(np.uint64)[0]))
    compare(route, got, code, R.block(S, T, W), exact)


# ---- two live contexts ------------------------------------------------------------------------------

def test_two_live_contexts(route):
    """A context at the LDS limit and one of 64 vertices, both in the LDS form, used in turn:
    the dynamic-LDS limit of the kernel is raised once per context, and each still gets its own."""
    big, small = f"sized{lr.lds_max_n()}_dec", "ba64_ties"
    gb, gs = graph(big), graph(small)
    assert lr.fits_lds(gb.n) and lr.fits_lds(gs.n) and lr.layout_total(gb.n) > 100 * lr.layout_total(gs.n)
    eb = route.RouteEngine(gb)
    es = route.RouteEngine(gs)
    Sb, Ss = [0, gb.n - 1, gb.n // 2], tl.sources(small)[:8]
    Tb = np.arange(0, gb.n, 3)
    Wb, Ws = tl.weights("sized", len(Sb), len(Tb), 6), tl.weights(small, len(Ss), gs.n, 16)
    for _ in range(2):
        check(route, big, Sb, Wb, eng=eb, T=Tb)
        check(route, small, Ss, Ws, eng=es)


# ---- the front end ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ba64_ties", "ba120_vloss", "k24"])
def test_front_end_link_loss(topo, route, name):
    """Packet counters on a few hundred stored pairs, one past 2^32: link_loss equals the
    reference over the stored pairs (lower -> higher) under the cache's dispatch; all zero
    before the first fill; nothing cached moves."""
    g, A = hg._graph(name)
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    z = t.link_loss()
    assert z[0].dtype == np.float64 and [len(a) for a in z[:4]] == [g.m, g.m, g.n, g.n]
    assert not any(a.any() for a in z[:4]) and z[4] == 0              # before the fill
    assert t.get_latency(int(A[0]), int(A[1])) >= 0
    z = t.link_loss()
    assert not any(a.any() for a in z[:4]) and z[4] == 0              # no packets yet
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
    R = lr.LossRef(g)
    f64, exact = R.pairs(ps, pt, pw, dispatch=True), R.pairs(ps, pt, pw, dispatch=True, exact=True)
    got = t.link_loss()
    assert got[4] == exact.unrouted
    for k in range(4):
        assert lr.close(got[k], exact.outs()[k], exact.R, exact.A), lr.NAMES[k]
    loads = t.link_loads()
    # fewer packets reach a link than are sent over it
    assert np.all(got[0] <= loads[0].astype(np.float64)) and got[4] == loads[2]
    assert got[0].sum() > 0 and got[3].sum() > 0 and exact.A > 2
    assert snap() == was
    t.close()
