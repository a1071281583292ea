"""GPU: the link repricing calls -- shd_route_reprice*, shd_route_pair_reprice, RouteEngine's
wrappers and the front end's shd_topology_link_reprice -- against tests/reprice_ref.py (the
definition and the kernel's programme, held together bit for bit by tests/test_reprice.py).

Everything is exact: stats, max_add, max_gain and min_new are compared with ==, unrouted too, the
new latencies with array_equal (NaNs matched)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import outage_ref as orf
from tests import reprice_ref as rr
from tests import stream_order as so
from tests import test_hops_gpu as hg
from tests import test_outage as tout
from tests import test_reprice as trp
from tests.multi_ref import Ref
from tests.test_range_gpu import select

pytestmark = pytest.mark.gpu

KNOB = "SHD_ROUTE_REPRICE_LDS"


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
    for k in (KNOB, "SHD_ROUTE_OUTAGE_LDS", "SHD_ROUTE_HOPS_SCRATCH"):
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
    g = trp.graph(name)
    if S is None:
        S, T, W = trp.entries(name)
    scn = trp.scenarios(name) if scn is None else scn
    default = S is trp.entries(name)[0] and scn is trp.scenarios(name)
    want = trp.programmed(name) if default else rr.RepriceRef(g).programme(*rr.block_entries(S, T, W), scn)
    eng = eng or route.RouteEngine(g)
    got, code = run(route, eng.reprice, S, T, scn, W, lat=True)
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
    S, T, W = trp.entries(name)
    ps, pt, pw = rr.block_entries(S, T, W)
    rng = np.random.default_rng(len(ps))
    k = np.concatenate([rng.permutation(len(ps)), rng.integers(0, max(len(ps), 1), size=100 if len(ps) else 0)])
    ps, pt, pw = ps[k], pt[k], pw[k]
    return ps, pt, pw, rr.RepriceRef(trp.graph(name)).programme(ps, pt, pw, trp.scenarios(name))


# ---- every form on the small builders --------------------------------------------------------------

@pytest.mark.parametrize("lds", [None, "0"])
@pytest.mark.parametrize("name", tout.SMALL)
def test_every_form(route, monkeypatch, name, lds):
    """The block, the same entries as shuffled pairs with repeats, and the async call with
    ld > nt, each against the reference, in the LDS form and in HBM slices."""
    import torch
    if lds is not None:
        monkeypatch.setenv(KNOB, lds)
    g = trp.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = trp.entries(name)
    scn = trp.scenarios(name)
    _, _, want = check_block(route, name, eng)
    ps, pt, pw, wantp = pair_case(name)
    got, code = run(route, eng.pair_reprice, ps, pt, scn, pw, lat=True)
    compare(got, code, wantp)
    # async: padded rows, canaries in the padding and in the outputs
    ns, nt, ld, nscn = len(S), len(T), len(T) + 3, len(scn)
    Wp = np.zeros((ns, ld), np.uint64); Wp[:, :nt] = W
    off, edge, nl = rr.pack(scn, sort=True)
    if not len(edge):
        edge, nl = np.zeros(1, np.int32), np.ones(1)
    dev = torch.device("cuda", 0)
    d_st = torch.full((nscn, 3), 7, dtype=torch.int64, device=dev)
    d_mx, d_mg, d_mn = (torch.full((nscn,), 7.25, dtype=torch.float64, device=dev) for _ in range(3))
    d_lat = torch.full((nscn, ns, ld), 7.25, dtype=torch.float64, device=dev)
    d_un = torch.full((1,), 7, dtype=torch.int64, device=dev)
    eng.reprice_async(_dev(S), _dev(T), _dev(Wp), _dev(off), _dev(edge), _dev(nl), d_st, d_mx, d_mg, d_mn, d_lat, d_un,
                      ld=ld)
    code = _sync(route, eng)
    lat = d_lat.cpu().numpy()
    assert np.all(lat[:, :, nt:] == 7.25)
    compare((d_st.cpu().numpy().view(np.uint64), d_mx.cpu().numpy(), d_mg.cpu().numpy(), d_mn.cpu().numpy(),
             np.ascontiguousarray(lat[:, :, :nt]), int(d_un.cpu().numpy().view(np.uint64)[0])), code, want,
            (nscn, ns, nt))


# ---- the larger shapes -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", trp.LARGE)
def test_shapes(route, name):
    """grid (tied detours), the multigraphs, the directed graphs, fractional latencies, the
    lollipop's tail, second self-loops, and the three builders of this feature: the chord's long
    chain of gains, the hub's wide frontier and fan, the layers' 48 tails per vertex -- the block
    and the pair form."""
    got, code, want = check_block(route, name)
    assert len(trp.scenarios(name)) >= 3
    ps, pt, pw, wantp = pair_case(name)
    eng = route.RouteEngine(trp.graph(name))
    got, code = run(route, eng.pair_reprice, ps, pt, trp.scenarios(name), pw, lat=True)
    compare(got, code, wantp)


def test_natural_hbm16(route):
    """One vertex past the LDS limit: the u16 state in HBM slices without the knob."""
    name = trp.HBM16
    g = trp.graph(name)
    assert g.n == rr.lds_max_n() + 1 and not rr.fits_lds(g.n) and g.n <= 65535
    check_block(route, name)


def test_hbm32_ring(route):
    """66,000 vertices: u32 lists.  One edge half-way round lowered to a tenth."""
    s, scn, ts = trp.ring_case()
    R = trp.ref("ring66k")
    want = R.programme([s] * len(ts), ts, None, [scn])
    assert want.stats[0, rr.HIT] >= 1 and want.stats[0, rr.FASTER] >= 1
    eng = route.RouteEngine(trp.graph("ring66k"))
    got, code = run(route, eng.reprice, [s], ts, [scn], lat=True)
    compare(got, code, want, (1, 1, len(ts)))


# ---- against a context of the repriced graph ---------------------------------------------------------

@pytest.mark.parametrize("name,sel", [("sized63", "auto"), ("sized63", "kd"), ("multi389", "auto"), ("multi389", "kd"),
                                      ("grid", "auto"), ("grid", "kd"), ("frac_cents", "auto")])
def test_fresh_context(route, monkeypatch, name, sel):
    """lat[k] is bit-equal to the rows of a context created from the repriced graph, flags 0: every
    scenario of the case, at most 12 (connectivity does not change, so none is left out).  The
    integer graphs are also repriced to fractional latencies (the factor 0.37)."""
    select(monkeypatch, sel)
    g = trp.graph(name)
    S, T, W = trp.entries(name)
    scn = [f for f in trp.scenarios(name) if f][:11] + [[]]
    assert any(not float(w).is_integer() for f in scn for _, w in f)
    eng = route.RouteEngine(g)
    got, _ = run(route, eng.reprice, S, T, scn, W, lat=True)
    old_failed = np.isnan(trp.programmed(name).lat[0].reshape(len(S), len(T)))
    for k, f in enumerate(scn):
        ek = route.RouteEngine(rr.repriced(g, f))
        try:
            lat = ek.rows(S, T, dispatch=False)[0]
        except route.RouteError as err:
            lat = err.partial[0]
        lat = np.where(old_failed, np.nan, lat)       # an entry that fails in the graph itself takes no part
        assert np.array_equal(got[4][k], lat, equal_nan=True), (name, sel, k)
        ek.close()
    assert got[0][:, rr.HIT].any() and got[0][:, rr.FASTER].any() and got[0][:, rr.SLOWER].any()


# ---- many units ------------------------------------------------------------------------------------

def test_more_units_than_slots(route, monkeypatch):
    """The HBM form with 16 slices and 3 sources x 60 single-edge scenarios in 180 units."""
    name = "sized63"
    g = trp.graph(name)
    monkeypatch.setenv(KNOB, "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 16 * g.n))
    S = np.array([0, 31, 62], np.int32)
    lat = np.asarray(g.latency, np.float64)
    scn = [[(e, float(lat[e] * (0.25 if e % 2 else 3)))] for e in range(60)]
    form = rr.state_form(g.n, rr.units(len(S), len(scn))[2], True, 4 * 16 * g.n // 4)
    assert form[0] == 2 and form[4] == 16 and rr.units(len(S), len(scn))[2] == 180 > form[1]
    check_block(route, name, scn=scn, S=S, T=np.arange(g.n, dtype=np.int32), W=trp.weights(name, 3, g.n))


@pytest.mark.parametrize("lds", [None, "0"])
def test_source_chunks(route, monkeypatch, lds):
    """Scratch for three sources per chunk, seven sources: the statistics add up across three
    chunks and every chunk writes its rows of every scenario's latencies."""
    name = "ba64_ties"
    g = trp.graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv(KNOB, lds)
    S = trp.sources(name)[:7]
    T = np.arange(g.n, dtype=np.int32)
    scn = trp.scenarios(name)[:8]
    check_block(route, name, scn=scn, S=S, T=T, W=trp.weights(name, 7, g.n))
    ps, pt, pw = rr.block_entries(S, T, trp.weights(name, 7, g.n))
    eng = route.RouteEngine(g)
    got, code = run(route, eng.pair_reprice, ps[::-1], pt[::-1], scn, pw[::-1], lat=True)
    compare(got, code, rr.RepriceRef(g).programme(ps[::-1], pt[::-1], pw[::-1], scn))


# ---- failed entries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiny3_none", "tiny9_some"])
def test_failed_entries(route, name):
    """Entries that fail in the graph itself: the code, their weight in unrouted once whatever the
    number of scenarios, NaN in every scenario's latencies and no part in any statistic."""
    g = trp.graph(name)
    S, T, W = trp.entries(name)
    scn = trp.scenarios(name)
    got, rc, want = check_block(route, name)
    failed = np.isnan(want.lat[0]).reshape(len(S), len(T))
    assert rr.ENOEDGE in want.codes and rc in want.codes and failed.any() and len(scn) >= 3
    assert got[5] == int(W[failed].sum()) > 0
    assert np.all(np.isnan(got[4][:, failed]))
    only = np.where(failed, W, 0).astype(np.uint64)                # the failed entries alone: no statistic
    eng = route.RouteEngine(g)
    g2, rc2 = run(route, eng.reprice, S, T, scn, only)
    assert not g2[0].any() and g2[5] == got[5] and rc2 == rc
    assert np.array_equal(g2[1], want.max_add) and np.array_equal(g2[3], want.min_new)   # weight 0 is still an entry


# ---- arguments and outputs ---------------------------------------------------------------------------

def test_refused_arguments(route):
    import torch
    name = "sized63"
    g = trp.graph(name)
    eng = route.RouteEngine(g)
    L = route.load_library()
    S, T = np.array([0, 5], np.int32), np.arange(g.n, dtype=np.int32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    st, un = np.full((2, 3), 7, np.uint64), np.full(1, 7, np.uint64)
    mx, mg, mn = np.full(2, 7.25), np.full(2, 7.25), np.full(2, 7.25)
    lat = np.full((2, 2, g.n), 7.25)

    def host(s, t, off, edge, nl, flags=0):
        off, edge, nl = np.asarray(off, np.int64), np.asarray(edge, np.int32), np.asarray(nl, np.float64)
        return L.shd_route_reprice(eng._h, P(s), len(s), P(t), len(t), flags, None, P(off), P(edge), P(nl),
                                   len(off) - 1, P(st), P(mx), P(mg), P(mn), P(lat), P(un))

    def pairs(s, t, off, edge, nl, flags=0):
        off, edge, nl = np.asarray(off, np.int64), np.asarray(edge, np.int32), np.asarray(nl, np.float64)
        return L.shd_route_pair_reprice(eng._h, P(s), P(t), None, len(s), flags, P(off), P(edge), P(nl), len(off) - 1,
                                        P(st), P(mx), P(mg), P(mn), P(lat), P(un))
    ok_off, ok_edge, ok_lat = [0, 1, 3], [4, 9, 2], [3.5, 80.0, 1.0]
    lo = float(np.asarray(g.latency)[np.asarray(g.src) != np.asarray(g.dst)].min())
    tiny = lo * (g.n - 1) * 2.0 ** -52 * 0.5            # min(lo, tiny) <= (n - 1) * hi * 2^-52 whatever hi is
    loop = int(np.flatnonzero(np.asarray(g.src) == np.asarray(g.dst))[0])
    for call in (host, pairs):
        s, t = (S, T) if call is host else (np.array([0, 5], np.int32), np.array([7, 9], np.int32))
        assert call(s, t, ok_off, ok_edge, ok_lat, route.DISPATCH) == route.EINVAL
        assert call(s, t, ok_off, ok_edge, ok_lat, 0x400) == route.EINVAL
        assert call(s, t, ok_off, [4, g.m, 2], ok_lat) == route.EINVAL
        assert call(s, t, ok_off, [4, -1, 2], ok_lat) == route.EINVAL
        assert call(s, t, ok_off, [4, 9, 9], ok_lat) == route.EINVAL                    # a repeated id
        for bad in (0.0, -1.0, np.inf, -np.inf, np.nan):
            assert call(s, t, ok_off, ok_edge, [3.5, bad, 1.0]) == route.EINVAL, bad
        assert call(s, t, [0, 2, 1], ok_edge, ok_lat) == route.EINVAL
        assert call(s, t, ok_off, ok_edge, [3.5, tiny, 1.0]) == route.EUNSUPPORTED
        assert call(np.array([0, g.n], np.int32), t, ok_off, ok_edge, ok_lat) == route.EINVAL
        assert call(s, np.where(t == 9, -1, t).astype(np.int32), ok_off, ok_edge, ok_lat) == route.EINVAL
        assert np.all(st == 7) and np.all(mx == 7.25) and np.all(mg == 7.25) and np.all(mn == 7.25)
        assert np.all(lat == 7.25) and un[0] == 7                                       # nothing written
    # the same id in two scenarios is fine, and a self-loop's latency is outside the absorption rule
    assert host(S, T, [0, 1, 3], [4, 4, loop], [3.5, 80.0, tiny]) == route.OK
    assert host(S, T, ok_off, ok_edge, ok_lat) == route.OK and un[0] == 0 and not np.any(lat == 7.25)
    # async: the flags at once, the rest by the validation kernel on the error word
    dS, dT = _dev(S), _dev(T)
    d_st = torch.zeros((2, 3), dtype=torch.int64, device=dS.device)
    f64 = lambda a: _dev(np.array(a, np.float64))
    with pytest.raises(route.RouteError) as ei:
        eng.reprice_async(dS, dT, None, _dev(np.array(ok_off, np.int64)), _dev(np.array([4, 2, 9], np.int32)),
                          f64(ok_lat), d_st, None, None, None, None, None, flags=route.DISPATCH)
    assert ei.value.code == route.EINVAL
    cases = [(ok_off, [4, 9, 2], ok_lat), (ok_off, [4, 2, 2], ok_lat), (ok_off, [4, 2, g.m], ok_lat),
             (ok_off, [4, -5, 2], ok_lat), ([0, 2, 1], [4, 2, 9], ok_lat), ([1, 1, 3], [4, 2, 9], ok_lat)]
    cases += [(ok_off, [4, 2, 9], [3.5, bad, 1.0]) for bad in (0.0, -1.0, np.inf, np.nan)]
    for off, edge, nl in cases:
        eng.reprice_async(dS, dT, None, _dev(np.array(off, np.int64)), _dev(np.array(edge, np.int32)), f64(nl), d_st,
                          None, None, None, None, None)
        assert _sync(route, eng) == route.EINVAL, (off, edge, nl)
    eng.reprice_async(dS, dT, None, _dev(np.array(ok_off, np.int64)), _dev(np.array([4, 2, 9], np.int32)),
                      f64([3.5, tiny, 1.0]), d_st, None, None, None, None, None)
    assert _sync(route, eng) == route.EUNSUPPORTED
    eng.reprice_async(dS, dT, None, _dev(np.array(ok_off, np.int64)), _dev(np.array([4, 2, 9], np.int32)),
                      f64([3.5, 1.0, 80.0]), d_st, None, None, None, None, None)
    assert _sync(route, eng) == route.OK
    want = rr.RepriceRef(g).programme(*rr.block_entries(S, T), [[(4, 3.5)], [(2, 1.0), (9, 80.0)]])
    assert np.array_equal(d_st.cpu().numpy().view(np.uint64), want.stats)


def test_no_and_empty_scenarios(route):
    """nscn == 0 writes only unrouted; empty scenarios give zeros, the old rows and their minimum."""
    name = "ba60_holes"
    g = trp.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = trp.entries(name)
    want = rr.RepriceRef(g).programme(*rr.block_entries(S, T, W), [[], []])
    assert want.unrouted > 0
    got, code = run(route, eng.reprice, S, T, [], W, lat=True)
    assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[5] == want.unrouted and code == route.ENOEDGE
    got, code = run(route, eng.pair_reprice, *rr.block_entries(S, T)[:2], [], rr.block_entries(S, T, W)[2])
    assert got[5] == want.unrouted and code == route.ENOEDGE
    got, code = run(route, eng.reprice, S, T, [[], []], W, lat=True)
    compare(got, code, want, (2, len(S), len(T)))
    assert not got[0].any() and not got[1].any() and not got[2].any()
    try:
        old = eng.rows(S, T, dispatch=False)[0]
    except route.RouteError as err:
        old = err.partial[0]
    assert np.array_equal(got[4][0], old, equal_nan=True) and np.array_equal(got[4][1], old, equal_nan=True)
    assert got[3][0] == got[3][1] == np.nanmin(old)
    # nothing to route
    z = eng.reprice(np.zeros(0, np.int32), T, [[(1, 2.0)]], lat=True)
    assert not z[0].any() and z[5] == 0 and np.all(np.isinf(z[3]))


def test_each_output_alone(route):
    name = "sized63"
    g = trp.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = trp.entries(name)
    scn = trp.scenarios(name)
    want = trp.programmed(name)
    nscn = len(scn)
    full = [want.stats, want.max_add, want.max_gain, want.min_new, want.lat.reshape(nscn, len(S), len(T)), want.unrouted]
    for keep in range(6):
        out = [np.full((nscn, 3), 7, np.uint64), np.full(nscn, 7.25), np.full(nscn, 7.25), np.full(nscn, 7.25),
               np.full((nscn, len(S), len(T)), 7.25), np.full(1, 7, np.uint64)]
        out = [o if k == keep else None for k, o in enumerate(out)]
        got, code = run(route, eng.reprice, S, T, scn, W, lat=True, out=tuple(out))
        assert [x is None for x in got] == [k != keep for k in range(6)]
        assert np.array_equal(got[keep], full[keep], equal_nan=True) if keep < 5 else got[5] == full[5]
    ps, pt, pw, wantp = pair_case(name)
    got, code = run(route, eng.pair_reprice, ps, pt, scn, pw, out=(None, None, np.full(nscn, 7.25), None, None, None))
    assert np.array_equal(got[2], wantp.max_gain)


# ---- stream order --------------------------------------------------------------------------------------

def test_gated_reprice(route, monkeypatch):
    """reprice_async behind the timed gate of tests/stream_order.py, in three chunks: decoy inputs
    until the gate opens, two calls with the canary in between, and the call returns while the
    gate is shut."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    S = A[:7].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    R = rr.RepriceRef(g)
    scn = trp.scenarios(name)[:8]                                       # lists of 0, 1 and 2 ids
    nscn = len(scn)
    W = trp.weights(name, ns, nt)
    Wp = np.zeros((ns, nt + 1), np.uint64); Wp[:, :nt] = W
    want = R.programme(*rr.block_entries(S, T, W), scn)
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    Wd = np.roll(W, 7, axis=1)
    Wdp = np.zeros_like(Wp); Wdp[:, :nt] = Wd
    scd = scn[::-1]                                                     # a decoy: the scenarios reversed
    scl = [[(e, w * 1.5) for e, w in f] for f in scn]                   # another: other latencies
    for s, t, w, q in ((Sd, T, W, scn), (S, Td, W, scn), (S, T, Wd, scn), (S, T, W, scd), (S, T, W, scl)):
        one = R.programme(*rr.block_entries(s, t, w), q)                # an early reader gets other results
        assert not (np.array_equal(one.stats, want.stats) and np.array_equal(one.max_add, want.max_add) and
                    np.array_equal(one.max_gain, want.max_gain))
    off, edge, nl = rr.pack(scn, sort=True)
    offd, edged, _ = rr.pack(scd, sort=True)
    _, _, nld = rr.pack(scl, sort=True)
    eng = route.RouteEngine(g)
    i_s, i_t, i_w, i_o, i_e, i_l = (so.In(S, Sd), so.In(T, Td), so.In(Wp, Wdp), so.In(off, offd), so.In(edge, edged),
                                    so.In(nl, nld))
    outs = [so.Out(nscn, 3, i64=True), so.Out(1, nscn), so.Out(1, nscn), so.Out(1, nscn), so.Out(nscn * ns, nt + 1),
            so.Out(1, 1, i64=True)]
    code = so.gated(route, eng, [i_s, i_t, i_w, i_o, i_e, i_l], outs,
                    lambda sh: eng.reprice_async(i_s.t, i_t.t, i_w.t, i_o.t, i_e.t, i_l.t, *[o.t for o in outs],
                                                 stream=sh, ld=nt + 1),
                    "reprice_async")
    got = (outs[0].snap_bits(3).view(np.uint64), outs[1].f64(nscn)[0], outs[2].f64(nscn)[0], outs[3].f64(nscn)[0],
           outs[4].f64(nt).reshape(nscn, ns, nt), int(outs[5].snap_bits(1)[0].view(np.uint64)[0]))
    compare(got, code, want, (nscn, ns, nt))


# ---- the context is left as it was -----------------------------------------------------------------------

def test_context_left_intact(route):
    """rows, hops and the outages on the same context before and after repricing calls still equal
    their references."""
    name = "multi389"
    g = trp.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = trp.entries(name)
    R = Ref(g)
    lat, rel, hops = R.rows(S, T, dispatch=False)
    oscn = tout.scenarios(name)
    owant = tout.repaired(name)

    def partial(call, *a, **k):
        try:
            return call(*a, **k)
        except route.RouteError as err:
            assert err.code == route.ENOEDGE              # multi389 lacks some self-loops
            return err.partial

    def others():
        got = partial(eng.rows, S, T, dispatch=False)
        assert np.array_equal(got[0], lat, equal_nan=True)
        assert np.allclose(got[1], rel, rtol=1e-12, atol=0, equal_nan=True)
        assert np.array_equal(partial(eng.hops, S, T, dispatch=False)[0], hops)
        st, mx, la, un = partial(eng.outage, S, T, oscn, W, lat=True)
        assert np.array_equal(st, owant.stats) and np.array_equal(mx, owant.max_add) and un == owant.unrouted
        assert np.array_equal(la.reshape(owant.lat.shape), owant.lat, equal_nan=True)
    others()
    check_block(route, name, eng)
    check_block(route, name, eng)
    others()
    check_block(route, name, eng)


# ---- the front end -------------------------------------------------------------------------------------

def test_front_end_link_reprice(topo, route):
    """Packet counters on a few hundred stored pairs, one past 2^32: link_reprice equals the
    reference over the stored pairs (lower -> higher); zeros and +inf before the first fill;
    nothing cached moves."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    assert not g.prefer_direct
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    scn = trp.scenarios(name)
    z = t.link_reprice(scn)
    assert z[0].shape == (len(scn), 3) and not z[0].any() and not z[1].any() and not z[2].any()   # before the fill
    assert np.all(np.isinf(z[3])) and z[4] == 0
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
    was = snap()
    ps, pt, pw = [], [], []
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            c = t.packet_count(a, b)
            if c:
                ps.append(a); pt.append(b); pw.append(c)
    assert len(ps) > 100 and max(pw) > 2 ** 32
    want = rr.RepriceRef(g).programme(ps, pt, pw, scn)
    got = t.link_reprice(scn)
    assert np.array_equal(got[0], want.stats) and np.array_equal(got[1], want.max_add)
    assert np.array_equal(got[2], want.max_gain) and np.array_equal(got[3], want.min_new) and got[4] == want.unrouted
    assert want.stats[:, rr.HIT].any() and want.stats[:, rr.FASTER].any() and want.stats.max() > 2 ** 32
    assert np.array_equal(t.link_reprice(rr.pack(scn))[0], want.stats)                        # the (off, edge, lat) form
    for bad in ([[(g.m, 1.0)]], [[(0, 0.0)]], [[(0, 1.0), (0, 2.0)]]):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            t.link_reprice(bad)
    assert snap() == was
    t.close()


@pytest.mark.parametrize("name", ["ba80_prefer", "k24"])
def test_front_end_dispatching_cache_is_unsupported(topo, route, name):
    g, A = hg._graph(name)
    t = topo.Topology.from_graph(g)
    t.attach_all(np.sort(A))
    assert route.EUNSUPPORTED == -6
    with pytest.raises(RuntimeError, match=r"\(-6\)"):
        t.link_reprice([[(0, 1.0)]])
    t.close()


# ---- two live contexts ------------------------------------------------------------------------------------

def test_two_live_contexts(route):
    """A context at the LDS limit and one of 64 vertices, both in the LDS form, their calls
    alternated: each launch takes its own context's state size, columns and scratch, and each
    still equals its reference."""
    big, small = f"sized{rr.lds_max_n()}", "ba64_ties"
    gb, gs = trp.graph(big), trp.graph(small)
    assert rr.fits_lds(gb.n) and rr.fits_lds(gs.n) and rr.layout_total(gb.n) > 100 * rr.layout_total(gs.n)
    eb = route.RouteEngine(gb)
    es = route.RouteEngine(gs)
    for _ in range(2):
        _, _, wb = check_block(route, big, eb)
        _, _, ws = check_block(route, small, es)
    assert wb.stats[:, rr.HIT].any() and ws.stats[:, rr.HIT].any()
