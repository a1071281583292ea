"""GPU: the link edit calls -- shd_route_edit*, shd_route_pair_edit, RouteEngine's wrappers and
the front end's shd_topology_link_edit -- against tests/edit_ref.py (the definition and the
kernel's programme, held together bit for bit by tests/test_edit.py), against a context created
from every edited graph, and against the repricing and the outage calls where a scenario is
theirs.

Everything is exact: stats, max_add, max_gain and min_new are compared with ==, unrouted too, the
new latencies with array_equal (NaNs matched)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import edit_ref as er
from tests import stream_order as so
from tests import test_edit as ted
from tests import test_hops_gpu as hg
from tests import test_outage as tout
from tests import test_reprice as trp
from tests.multi_ref import Ref
from tests.test_range_gpu import select

pytestmark = pytest.mark.gpu

INF = math.inf
KNOB = "SHD_ROUTE_EDIT_LDS"


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
    for k in (KNOB, "SHD_ROUTE_REPRICE_LDS", "SHD_ROUTE_OUTAGE_LDS", "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)


def run(route, call, *args, **kw):
    """((stats, max_add, max_gain, min_new, lat, unrouted), code) of a call, failed entries or not."""
    try:
        return call(*args, **kw), route.OK
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return err.partial, err.code


def compare(got, code, want, shape=None):
    st, mx, mg, mn, lat, un = got
    assert code in want.codes, (code, want.codes)
    assert un == want.unrouted
    assert st.dtype == np.uint64 and np.array_equal(st, want.stats), (st.tolist(), want.stats.tolist())
    assert mx.dtype == np.float64 and np.array_equal(mx, want.max_add), (mx.tolist(), want.max_add.tolist())
    assert mg.dtype == np.float64 and np.array_equal(mg, want.max_gain), (mg.tolist(), want.max_gain.tolist())
    assert mn.dtype == np.float64 and np.array_equal(mn, want.min_new), (mn.tolist(), want.min_new.tolist())
    if lat is not None:
        w = want.lat if shape is None else want.lat.reshape(shape)
        bad = np.argwhere(~((lat == w) | (np.isnan(lat) & np.isnan(w))))
        assert lat.shape == w.shape and len(bad) == 0, (len(bad), bad[:5].tolist())


def check_block(route, name, eng=None, scn=None, S=None, T=None, W=None):
    g = ted.graph(name)
    if S is None:
        S, T, W = ted.entries(name)
    scn = ted.scenarios(name) if scn is None else scn
    default = S is ted.entries(name)[0] and scn is ted.scenarios(name)
    want = ted.programmed(name) if default else er.EditRef(g).programme(*er.block_entries(S, T, W), scn)
    eng = eng or route.RouteEngine(g)
    got, code = run(route, eng.edit, S, T, scn, W, lat=True)
    compare(got, code, want, (len(scn), len(S), len(T)))
    return got, code, want


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


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """The block's entries as shuffled pairs with a hundred repeats, and the reference over them."""
    S, T, W = ted.entries(name)
    ps, pt, pw = er.block_entries(S, T, W)
    rng = np.random.default_rng(len(ps))
    k = np.concatenate([rng.permutation(len(ps)), rng.integers(0, max(len(ps), 1), size=100 if len(ps) else 0)])
    ps, pt, pw = ps[k], pt[k], pw[k]
    return ps, pt, pw, er.EditRef(ted.graph(name)).programme(ps, pt, pw, ted.scenarios(name))


def _packed(scn):
    off, edge, a, b, nl = er.pack(scn, sort=True)
    if not len(edge):
        edge, a, b, nl = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1)
    return off, edge, a, b, nl


# ---- every form on the small builders --------------------------------------------------------------

@pytest.mark.parametrize("lds", [None, "0"])
@pytest.mark.parametrize("name", ted.SMALL + ["lolli20", "dring12"])
def test_every_form(route, monkeypatch, name, lds):
    """The block, the same entries as shuffled pairs with repeats, and the async call with
    ld > nt, each against the reference, in the LDS form and in HBM slices."""
    import torch
    if lds is not None:
        monkeypatch.setenv(KNOB, lds)
    g = ted.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = ted.entries(name)
    scn = ted.scenarios(name)
    _, _, want = check_block(route, name, eng)
    ps, pt, pw, wantp = pair_case(name)
    got, code = run(route, eng.pair_edit, ps, pt, scn, pw, lat=True)
    compare(got, code, wantp)
    # async: padded rows, canaries in the padding and in the outputs
    ns, nt, ld, nscn = len(S), len(T), len(T) + 3, len(scn)
    Wp = np.zeros((ns, ld), np.uint64); Wp[:, :nt] = W
    off, edge, a, b, nl = _packed(scn)
    dev = torch.device("cuda", 0)
    d_st = torch.full((nscn, er.NSTAT), 7, dtype=torch.int64, device=dev)
    d_mx, d_mg, d_mn = (torch.full((nscn,), 7.25, dtype=torch.float64, device=dev) for _ in range(3))
    d_lat = torch.full((nscn, ns, ld), 7.25, dtype=torch.float64, device=dev)
    d_un = torch.full((1,), 7, dtype=torch.int64, device=dev)
    eng.edit_async(_dev(S), _dev(T), _dev(Wp), _dev(off), _dev(edge), _dev(a), _dev(b), _dev(nl), d_st, d_mx, d_mg,
                   d_mn, d_lat, d_un, ld=ld)
    code = _sync(route, eng)
    lat = d_lat.cpu().numpy()
    assert np.all(lat[:, :, nt:] == 7.25)
    compare((d_st.cpu().numpy().view(np.uint64), d_mx.cpu().numpy(), d_mg.cpu().numpy(), d_mn.cpu().numpy(),
             np.ascontiguousarray(lat[:, :, :nt]), int(d_un.cpu().numpy().view(np.uint64)[0])), code, want,
            (nscn, ns, nt))


# ---- the larger shapes -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ted.LARGE)
def test_shapes(route, name):
    """grid, the multigraph, the directed lattice, fractional latencies, the lollipop, second
    self-loops, the hub's wide frontier, the layers, and the builders of this feature: the path's
    long chain of gains, the rejoined tail, the one-way ring, the star's 1,100 new links -- the
    block and the pair form."""
    check_block(route, name)
    assert len(ted.scenarios(name)) >= 3
    ps, pt, pw, wantp = pair_case(name)
    eng = route.RouteEngine(ted.graph(name))
    got, code = run(route, eng.pair_edit, ps, pt, ted.scenarios(name), pw, lat=True)
    compare(got, code, wantp)


@pytest.mark.parametrize("name", ["star1100", "hub1100", "path65"])
def test_long_lists_in_hbm(route, monkeypatch, name):
    """The list above the workgroup, the frontier above it and the long chain with the state in
    HBM slices."""
    monkeypatch.setenv(KNOB, "0")
    check_block(route, name)


def test_natural_hbm16(route):
    """One vertex past the LDS limit: the u16 state in HBM slices without the knob."""
    name = ted.HBM16
    g = ted.graph(name)
    assert g.n == er.lds_max_n() + 1 and not er.fits_lds(g.n) and g.n <= 65535
    check_block(route, name)


@functools.lru_cache(maxsize=None)
def ring_case():
    """(source, scenario, targets) on ring66k: an edge near the far side removed and a new link
    from the source's neighbourhood to a vertex behind it."""
    R = trp.ref("ring66k")
    s = 5
    d, pe, pu, hops, order = R.base._tree(s)
    v = order[-1]
    for _ in range(8):
        v = int(pu[v])
    e = int(pe[v])
    scn = [(e, INF), (s + 1, int(order[-1]), float(R.lat[e]))]
    E = er.EditRef(ted.graph("ring66k"))
    cur, mark, live = E._one(s, *er.split(scn), None)
    moved = np.flatnonzero(cur != d)
    ts = sorted(set(moved[:: max(1, len(moved) // 40)].tolist()) | set(list(mark)[:40]) | {s, 0, 33000, 65999})
    return s, scn, ts, E


def test_hbm32_ring(route):
    """66,000 vertices: u32 lists.  A removal half-way round and a new link across the ring."""
    s, scn, ts, E = ring_case()
    want = E.programme([s] * len(ts), ts, None, [scn])
    assert want.same(E.fresh([s] * len(ts), ts, None, [scn]))
    assert want.stats[0, er.HIT] >= 1 and want.stats[0, er.FASTER] >= 1
    eng = route.RouteEngine(ted.graph("ring66k"))
    got, code = run(route, eng.edit, [s], ts, [scn], lat=True)
    compare(got, code, want, (1, 1, len(ts)))


# ---- against a context of the edited graph -------------------------------------------------------------

@pytest.mark.parametrize("sel", ["auto", "kd"])
@pytest.mark.parametrize("name", ["sized63", "multi389", "grid", "lolli20", "dring12", "path65", "frac_cents"])
def test_fresh_context(route, monkeypatch, name, sel):
    """lat[k] is bit-equal to the rows of a context created from edited(g, scenario), flags 0: every
    scenario of the case that leaves the graph connected, none left out, each case under both
    selections."""
    select(monkeypatch, sel)
    g = ted.graph(name)
    S, T, W = ted.entries(name)
    scn = [f for f in ted.scenarios(name) if er.connected(er.edited(g, f))]
    assert len(scn) >= 4 and any(len(it) == 3 for f in scn for it in f) and any(it[-1] == INF for f in scn for it in f)
    eng = route.RouteEngine(g)
    got, _ = run(route, eng.edit, S, T, scn, W, lat=True)
    old_failed = np.isnan(ted.programmed(name).lat[0].reshape(len(S), len(T)))
    for k, f in enumerate(scn):
        ek = route.RouteEngine(er.edited(g, f))
        try:
            lat = ek.rows(S, T, dispatch=False)[0]
        except route.RouteError as err:
            lat = err.partial[0]
        lat = np.where(old_failed, np.nan, lat)       # an entry that fails in the graph itself takes no part
        assert np.array_equal(got[4][k], lat, equal_nan=True), (name, sel, k, f)
        ek.close()
    assert got[0][:, er.HIT].any() and got[0][:, er.FASTER].any()


# ---- against the calls that exist ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sized63", "multi389", "dir_grid", "loops_only"])
def test_finite_scenarios_equal_reprice(route, name):
    g = trp.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = trp.entries(name)
    scn = trp.scenarios(name)
    a, ca = run(route, eng.edit, S, T, scn, W, lat=True)
    b, cb = run(route, eng.reprice, S, T, scn, W, lat=True)
    assert ca == cb and a[5] == b[5]
    assert np.array_equal(a[0][:, [er.HIT, er.SLOWER, er.FASTER]], b[0]) and not a[0][:, er.CUT].any()
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in (1, 2, 3, 4))
    assert b[0][:, 0].any() and b[0][:, 1].any() and b[0][:, 2].any()


@pytest.mark.parametrize("name", ["sized63", "multi389", "dir_grid", "lollipop", "loops_only"])
def test_removals_equal_outage(route, name):
    g = tout.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = tout.entries(name)
    oscn = tout.scenarios(name)
    scn = [[(e, INF) for e in sorted(set(f))] for f in oscn]
    a, ca = run(route, eng.edit, S, T, scn, W, lat=True)
    b, cb = run(route, eng.outage, S, T, oscn, W, lat=True)
    assert ca == cb and a[5] == b[3]
    assert np.array_equal(a[0][:, [er.HIT, er.CUT, er.SLOWER]], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[4], b[2].reshape(a[4].shape), equal_nan=True)
    assert b[0][:, 0].any() and b[0][:, 2].any()


# ---- many units ------------------------------------------------------------------------------------

def test_more_units_than_slots(route, monkeypatch):
    """The HBM form with 16 slices and 3 sources x 60 scenarios in 180 units."""
    name = "sized63"
    g = ted.graph(name)
    monkeypatch.setenv(KNOB, "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 16 * g.n))
    S = np.array([0, 31, 62], np.int32)
    lat = np.asarray(g.latency, np.float64)
    scn = [[(e, INF), (e % g.n, (e * 7 + 3) % g.n, float(lat[e] / 2))] if (e * 7 + 3) % g.n != e % g.n else [(e, INF)]
           for e in range(60)]
    form = er.state_form(g.n, er.units(len(S), len(scn))[2], True, 4 * 16 * g.n // 4)
    assert form[0] == 2 and form[4] == 16 and er.units(len(S), len(scn))[2] == 180 > form[1]
    check_block(route, name, scn=scn, S=S, T=np.arange(g.n, dtype=np.int32), W=ted.weights(name, 3, g.n))


@pytest.mark.parametrize("lds", [None, "0"])
def test_source_chunks(route, monkeypatch, lds):
    """Scratch for three sources per chunk, seven sources: the statistics add up across three
    chunks and every chunk writes its rows of every scenario's latencies."""
    name = "ba64_ties"
    g = ted.graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv(KNOB, lds)
    S = ted.sources(name)[:7]
    T = np.arange(g.n, dtype=np.int32)
    scn = ted.scenarios(name)[:10]
    check_block(route, name, scn=scn, S=S, T=T, W=ted.weights(name, 7, g.n))
    ps, pt, pw = er.block_entries(S, T, ted.weights(name, 7, g.n))
    eng = route.RouteEngine(g)
    got, code = run(route, eng.pair_edit, ps[::-1], pt[::-1], scn, pw[::-1], lat=True)
    compare(got, code, er.EditRef(g).programme(ps[::-1], pt[::-1], pw[::-1], scn))


# ---- failed entries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny3_none", "tiny9_some"])
def test_failed_entries(route, name):
    """Entries that fail in the graph itself: the code, their weight in unrouted once whatever the
    number of scenarios, NaN in every scenario's latencies and no part in any statistic."""
    g = ted.graph(name)
    S, T, W = ted.entries(name)
    scn = ted.scenarios(name)
    got, rc, want = check_block(route, name)
    failed = np.isnan(want.lat[0]).reshape(len(S), len(T))
    assert er.ENOEDGE in want.codes and rc in want.codes and failed.any() and len(scn) >= 2
    assert got[5] == int(W[failed].sum()) > 0
    assert np.all(np.isnan(got[4][:, failed]))
    only = np.where(failed, W, 0).astype(np.uint64)                # the failed entries alone: no statistic
    eng = route.RouteEngine(g)
    g2, rc2 = run(route, eng.edit, S, T, scn, only)
    assert not g2[0].any() and g2[5] == got[5] and rc2 == rc
    assert np.array_equal(g2[1], want.max_add) and np.array_equal(g2[3], want.min_new)   # weight 0 is still an entry


# ---- arguments and outputs ---------------------------------------------------------------------------

def test_refused_arguments(route):
    import torch
    name = "sized63"
    g = ted.graph(name)
    eng = route.RouteEngine(g)
    L = route.load_library()
    S, T = np.array([0, 5], np.int32), np.arange(g.n, dtype=np.int32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    st, un = np.full((2, 4), 7, np.uint64), np.full(1, 7, np.uint64)
    mx, mg, mn = np.full(2, 7.25), np.full(2, 7.25), np.full(2, 7.25)
    lat = np.full((2, 2, g.n), 7.25)
    cols = lambda off, edge, a, b, nl: (np.asarray(off, np.int64), np.asarray(edge, np.int32), np.asarray(a, np.int32),
                                        np.asarray(b, np.int32), np.asarray(nl, np.float64))

    def host(s, t, rec, flags=0):
        off, edge, a, b, nl = cols(*rec)
        return L.shd_route_edit(eng._h, P(s), len(s), P(t), len(t), flags, None, P(off), P(edge), P(a), P(b), P(nl),
                                len(off) - 1, P(st), P(mx), P(mg), P(mn), P(lat), P(un))

    def pairs(s, t, rec, flags=0):
        off, edge, a, b, nl = cols(*rec)
        return L.shd_route_pair_edit(eng._h, P(s), P(t), None, len(s), flags, P(off), P(edge), P(a), P(b), P(nl),
                                     len(off) - 1, P(st), P(mx), P(mg), P(mn), P(lat), P(un))
    # scenario 0: edge 4 at 3.5; scenario 1: a new link 7 - 20 at 2.0 and edge 2 removed (given id first)
    ok = ([0, 1, 3], [4, 2, -1], [0, 0, 7], [0, 0, 20], [3.5, INF, 2.0])
    with_ = lambda i, col, v: tuple([*c[:col], v, *c[col + 1:]] if k == i else c for k, c in enumerate(ok))
    lo = float(np.asarray(g.latency)[np.asarray(g.src) != np.asarray(g.dst)].min())
    tiny = lo * (g.n - 1) * 2.0 ** -52 * 0.5            # min(lo, tiny) <= (n - 1) * hi * 2^-52 whatever hi is
    loop = int(np.flatnonzero(np.asarray(g.src) == np.asarray(g.dst))[0])
    for call in (host, pairs):
        s, t = (S, T) if call is host else (np.array([0, 5], np.int32), np.array([7, 9], np.int32))
        assert call(s, t, ok, route.DISPATCH) == route.EINVAL
        assert call(s, t, ok, 0x400) == route.EINVAL
        assert call(s, t, with_(1, 1, g.m)) == route.EINVAL
        assert call(s, t, with_(1, 1, -2)) == route.EINVAL
        assert call(s, t, ([0, 1, 3], [4, 2, 2], [0, 0, 0], [0, 0, 0], [3.5, INF, 2.0])) == route.EINVAL    # a repeated id
        for bad in (0.0, -1.0, -np.inf, np.nan):
            assert call(s, t, with_(4, 0, bad)) == route.EINVAL, bad
            assert call(s, t, with_(4, 2, bad)) == route.EINVAL, bad
        assert call(s, t, with_(4, 2, INF)) == route.EINVAL                                      # +inf on a new link
        assert call(s, t, with_(3, 2, g.n)) == route.EINVAL and call(s, t, with_(2, 2, -1)) == route.EINVAL
        assert call(s, t, with_(3, 2, 7)) == route.EINVAL                                        # a new self-loop
        assert call(s, t, with_(0, 1, 4)) == route.EINVAL                                        # offsets that fall
        assert call(s, t, with_(4, 2, tiny)) == route.EUNSUPPORTED
        assert call(s, t, with_(4, 0, tiny)) == route.EUNSUPPORTED
        assert call(np.array([0, g.n], np.int32), t, ok) == route.EINVAL
        assert call(s, np.where(t == 9, -1, t).astype(np.int32), ok) == route.EINVAL
        assert np.all(st == 7) and np.all(mx == 7.25) and np.all(mg == 7.25) and np.all(mn == 7.25)
        assert np.all(lat == 7.25) and un[0] == 7                                                # nothing written
    # the same id in two scenarios and the same new link twice are fine; a self-loop's latency is outside the rule
    assert host(S, T, ([0, 2, 5], [4, -1, 4, -1, loop], [0, 7, 0, 7, 0], [0, 20, 0, 20, 0], [3.5, 2.0, INF, 2.0, tiny])) == route.OK
    assert host(S, T, ok) == route.OK and un[0] == 0 and not np.any(lat == 7.25)
    # async: the flags at once, the rest by the validation kernel on the error word
    dS, dT = _dev(S), _dev(T)
    d_st = torch.zeros((2, 4), dtype=torch.int64, device=dS.device)
    dv = lambda rec: [_dev(c) for c in cols(*rec)]
    good = ([0, 1, 3], [4, -1, 2], [0, 7, 0], [0, 20, 0], [3.5, 2.0, INF])                       # the order it asks for
    with pytest.raises(route.RouteError) as ei:
        eng.edit_async(dS, dT, None, *dv(good), d_st, None, None, None, None, None, flags=route.DISPATCH)
    assert ei.value.code == route.EINVAL
    gw = lambda i, col, v: tuple([*c[:col], v, *c[col + 1:]] if k == i else c for k, c in enumerate(good))
    cases = [ok, gw(1, 2, g.m), gw(1, 2, -5), gw(1, 0, -3), gw(0, 1, 4), ([1, 1, 3], *good[1:]),
             ([0, 1, 3], [4, 2, 2], [0, 0, 0], [0, 0, 0], [3.5, 1.0, 2.0]), ([0, 1, 3], [4, 9, 2], [0, 0, 0], [0, 0, 0], [3.5, 1.0, 2.0]),
             gw(2, 1, g.n), gw(3, 1, -1), gw(3, 1, 7), gw(4, 1, INF)]
    cases += [gw(4, c, bad) for c in (0, 1, 2) for bad in (0.0, -1.0, np.nan)]
    for rec in cases:
        eng.edit_async(dS, dT, None, *dv(rec), d_st, None, None, None, None, None)
        assert _sync(route, eng) == route.EINVAL, rec
    for c in (0, 1):
        eng.edit_async(dS, dT, None, *dv(gw(4, c, tiny)), d_st, None, None, None, None, None)
        assert _sync(route, eng) == route.EUNSUPPORTED
    eng.edit_async(dS, dT, None, *dv(good), d_st, None, None, None, None, None)
    assert _sync(route, eng) == route.OK
    want = er.EditRef(g).programme(*er.block_entries(S, T), [[(4, 3.5)], [(7, 20, 2.0), (2, INF)]])
    assert np.array_equal(d_st.cpu().numpy().view(np.uint64), want.stats)


def test_no_and_empty_scenarios(route):
    """nscn == 0 writes only unrouted; empty scenarios give zeros, the old rows and their minimum."""
    name = "ba60_holes"
    g = ted.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = ted.entries(name)
    want = er.EditRef(g).programme(*er.block_entries(S, T, W), [[], []])
    assert want.unrouted > 0
    got, code = run(route, eng.edit, S, T, [], W, lat=True)
    assert got[0].shape == (0, 4) and got[1].shape == (0,) and got[5] == want.unrouted and code == route.ENOEDGE
    got, code = run(route, eng.pair_edit, *er.block_entries(S, T)[:2], [], er.block_entries(S, T, W)[2])
    assert got[5] == want.unrouted and code == route.ENOEDGE
    got, code = run(route, eng.edit, S, T, [[], []], W, lat=True)
    compare(got, code, want, (2, len(S), len(T)))
    assert not got[0].any() and not got[1].any() and not got[2].any()
    try:
        old = eng.rows(S, T, dispatch=False)[0]
    except route.RouteError as err:
        old = err.partial[0]
    assert np.array_equal(got[4][0], old, equal_nan=True) and np.array_equal(got[4][1], old, equal_nan=True)
    assert got[3][0] == got[3][1] == np.nanmin(old)
    # nothing to route
    z = eng.edit(np.zeros(0, np.int32), T, [[(1, 2.0), (0, 3, 1.0)]], lat=True)
    assert not z[0].any() and z[5] == 0 and np.all(np.isinf(z[3]))


def test_each_output_alone(route):
    name = "sized63"
    g = ted.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = ted.entries(name)
    scn = ted.scenarios(name)
    want = ted.programmed(name)
    nscn = len(scn)
    full = [want.stats, want.max_add, want.max_gain, want.min_new, want.lat.reshape(nscn, len(S), len(T)), want.unrouted]
    for keep in range(6):
        out = [np.full((nscn, 4), 7, np.uint64), np.full(nscn, 7.25), np.full(nscn, 7.25), np.full(nscn, 7.25),
               np.full((nscn, len(S), len(T)), 7.25), np.full(1, 7, np.uint64)]
        out = [o if k == keep else None for k, o in enumerate(out)]
        got, code = run(route, eng.edit, S, T, scn, W, lat=True, out=tuple(out))
        assert [x is None for x in got] == [k != keep for k in range(6)]
        assert np.array_equal(got[keep], full[keep], equal_nan=True) if keep < 5 else got[5] == full[5]
    ps, pt, pw, wantp = pair_case(name)
    got, code = run(route, eng.pair_edit, ps, pt, scn, pw, out=(None, None, np.full(nscn, 7.25), None, None, None))
    assert np.array_equal(got[2], wantp.max_gain)


# ---- stream order --------------------------------------------------------------------------------------

def test_gated_edit(route, monkeypatch):
    """edit_async behind the timed gate of tests/stream_order.py, in three chunks: decoy inputs
    until the gate opens, two calls with the canary in between, and the call returns while the
    gate is shut."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    S = A[:7].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    R = er.EditRef(g)
    scn = [f for f in ted.scenarios(name) if len(f) <= 3][:8]
    nscn = len(scn)
    assert nscn == 8 and any(len(it) == 3 for f in scn for it in f) and any(it[-1] == INF for f in scn for it in f)
    W = ted.weights(name, ns, nt)
    Wp = np.zeros((ns, nt + 1), np.uint64); Wp[:, :nt] = W
    want = R.programme(*er.block_entries(S, T, W), scn)
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    Wd = np.roll(W, 7, axis=1)
    Wdp = np.zeros_like(Wp); Wdp[:, :nt] = Wd
    scd = scn[::-1]                                                     # a decoy: the scenarios reversed
    scl = [[(*it[:-1], it[-1] * 1.5) for it in f] for f in scn]          # another: other latencies
    sce = [[(it[1], it[0], it[2]) if len(it) == 3 else it for it in f][::-1] for f in scn[::-1]]   # and other ends
    for s, t, w, q in ((Sd, T, W, scn), (S, Td, W, scn), (S, T, Wd, scn), (S, T, W, scd), (S, T, W, scl)):
        one = R.programme(*er.block_entries(s, t, w), q)                # an early reader gets other results
        assert not (np.array_equal(one.stats, want.stats) and np.array_equal(one.max_add, want.max_add) and
                    np.array_equal(one.max_gain, want.max_gain))
    off, edge, a, b, nl = er.pack(scn, sort=True)
    offd, edged, ad, bd, _ = er.pack(sce, sort=True)
    _, _, _, _, nld = er.pack(scl, sort=True)
    eng = route.RouteEngine(g)
    ins = [so.In(S, Sd), so.In(T, Td), so.In(Wp, Wdp), so.In(off, offd), so.In(edge, edged), so.In(a, ad), so.In(b, bd),
           so.In(nl, nld)]
    outs = [so.Out(nscn, 4, i64=True), so.Out(1, nscn), so.Out(1, nscn), so.Out(1, nscn), so.Out(nscn * ns, nt + 1),
            so.Out(1, 1, i64=True)]
    code = so.gated(route, eng, ins, outs,
                    lambda sh: eng.edit_async(*[i.t for i in ins], *[o.t for o in outs], stream=sh, ld=nt + 1),
                    "edit_async")
    got = (outs[0].snap_bits(4).view(np.uint64), outs[1].f64(nscn)[0], outs[2].f64(nscn)[0], outs[3].f64(nscn)[0],
           outs[4].f64(nt).reshape(nscn, ns, nt), int(outs[5].snap_bits(1)[0].view(np.uint64)[0]))
    compare(got, code, want, (nscn, ns, nt))


# ---- the context is left as it was -----------------------------------------------------------------------

def test_context_left_intact(route):
    """rows, hops, the outages and the repricing on the same context before and after edit calls
    still equal their references."""
    name = "multi389"
    g = ted.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = trp.entries(name)
    assert S is not None and np.array_equal(S, ted.entries(name)[0])
    R = Ref(g)
    lat, rel, hops = R.rows(S, T, dispatch=False)
    oscn, owant = tout.scenarios(name), tout.repaired(name)
    rscn, rwant = trp.scenarios(name), trp.programmed(name)

    def partial(call, *a, **k):
        try:
            return call(*a, **k)
        except route.RouteError as err:
            assert err.code == route.ENOEDGE              # multi389 lacks some self-loops
            return err.partial

    def others():
        got = partial(eng.rows, S, T, dispatch=False)
        assert np.array_equal(got[0], lat, equal_nan=True)        # (no edit call computes a reliability)
        assert np.array_equal(partial(eng.hops, S, T, dispatch=False)[0], hops)
        st, mx, la, un = partial(eng.outage, S, T, oscn, W, lat=True)
        assert np.array_equal(st, owant.stats) and np.array_equal(mx, owant.max_add) and un == owant.unrouted
        assert np.array_equal(la.reshape(owant.lat.shape), owant.lat, equal_nan=True)
        rp = partial(eng.reprice, S, T, rscn, W, lat=True)
        assert np.array_equal(rp[0], rwant.stats) and np.array_equal(rp[4].reshape(rwant.lat.shape), rwant.lat, equal_nan=True)
    others()
    check_block(route, name, eng)
    check_block(route, name, eng)
    others()
    check_block(route, name, eng)


# ---- the front end -------------------------------------------------------------------------------------

def test_front_end_link_edit(topo, route):
    """Packet counters on a few hundred stored pairs, one past 2^32: link_edit equals the
    reference over the stored pairs (lower -> higher); zeros and +inf before the first fill;
    nothing cached moves."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    assert not g.prefer_direct
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    scn = ted.scenarios(name)
    z = t.link_edit(scn)
    assert z[0].shape == (len(scn), 4) and not z[0].any() and not z[1].any() and not z[2].any()   # before the fill
    assert np.all(np.isinf(z[3])) and z[4] == 0
    every = [(e, 2.5) for e in range(g.m - 1, -1, -1)]                # every id once, descending: accepted
    assert not t.link_edit([every])[0].any()
    for bad in ([[(0, 1.0), (0, INF)]], [every + [(g.m // 2, INF)]], [[(g.m, 1.0)]], [[(3, 3, 1.0)]]):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):            # refused before the first fill too
            t.link_edit(bad)
    assert t.get_latency(int(A[0]), int(A[1])) >= 0
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
    ps, pt, pw = [], [], []
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            c = t.packet_count(a, b)
            if c:
                ps.append(a); pt.append(b); pw.append(c)
    assert len(ps) > 100 and max(pw) > 2 ** 32
    # and a new link between the ends of the hot pair, at half of what the pair takes now
    scn = scn + [[(int(min(hot)), int(max(hot)), float(t.get_latency(int(hot[0]), int(hot[1])) / 2))]]
    was = snap()
    want = er.EditRef(g).programme(ps, pt, pw, scn)
    got = t.link_edit(scn)
    assert np.array_equal(got[0], want.stats) and np.array_equal(got[1], want.max_add)
    assert np.array_equal(got[2], want.max_gain) and np.array_equal(got[3], want.min_new) and got[4] == want.unrouted
    assert want.stats[:, er.HIT].any() and want.stats[:, er.FASTER].any() and want.stats.max() > 2 ** 32
    assert np.array_equal(t.link_edit(er.pack(scn))[0], want.stats)                           # the tuple form
    for bad in ([[(g.m, 1.0)]], [[(0, 0.0)]], [[(0, 1.0), (0, INF)]], [[(0, 0, 1.0)]], [[(0, g.n, 1.0)]], [[(0, 1, INF)]]):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            t.link_edit(bad)
    assert snap() == was
    t.close()


@pytest.mark.parametrize("name", ["ba80_prefer", "k24"])
def test_front_end_dispatching_cache_is_unsupported(topo, route, name):
    g, A = hg._graph(name)
    t = topo.Topology.from_graph(g)
    t.attach_all(np.sort(A))
    assert route.EUNSUPPORTED == -6
    with pytest.raises(RuntimeError, match=r"\(-6\)"):
        t.link_edit([[(0, 1, 1.0)]])
    t.close()


# ---- two live contexts ------------------------------------------------------------------------------------

def test_two_live_contexts(route):
    """A context at the LDS limit and one of 64 vertices, both in the LDS form, their calls
    alternated: each launch takes its own context's state size, columns and scratch, and each
    still equals its reference."""
    big, small = f"sized{er.lds_max_n()}", "ba64_ties"
    gb, gs = ted.graph(big), ted.graph(small)
    assert er.fits_lds(gb.n) and er.fits_lds(gs.n) and er.layout_total(gb.n) > 100 * er.layout_total(gs.n)
    S = ted.sources(big)
    d, pe, pu, hops, order = ted.ref(big).base._tree(int(S[0]))
    far = top = int(order[-1])
    while hops[top] > 1:                                              # the first vertex on the way to the deepest one
        top = int(pu[top])
    T = np.unique(np.append(ted.targets(big), far)).astype(np.int32)
    W = ted.weights(big, len(S), len(T))
    scn = [[], [(int(S[0]), far, float(d[far] / 2))], [(int(pe[top]), INF), (int(S[0]), far, float(d[far] / 4))]]
    wb = er.EditRef(gb).programme(*er.block_entries(S, T, W), scn)
    eb = route.RouteEngine(gb)
    es = route.RouteEngine(gs)
    for _ in range(2):
        got, code = run(route, eb.edit, S, T, scn, W, lat=True)
        compare(got, code, wb, (len(scn), len(S), len(T)))
        _, _, ws = check_block(route, small, es)
    assert wb.stats[:, er.HIT].any() and wb.stats[:, er.FASTER].any() and ws.stats[:, er.HIT].any()
