"""GPU: the link outage calls -- shd_route_outage*, shd_route_pair_outage, RouteEngine's wrappers
and the front end's shd_topology_link_outage -- against tests/outage_ref.py (the definition and
the kernel's programme, held together bit for bit by tests/test_outage.py).

Everything is exact: stats and max_add are compared with ==, unrouted too, the new latencies
with array_equal (NaNs matched)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import outage_ref as orf
from tests import stream_order as so
from tests import test_hops_gpu as hg
from tests import test_outage as tout
from tests.multi_ref import Ref
from tests.test_range_gpu import select

pytestmark = pytest.mark.gpu

KNOB = "SHD_ROUTE_OUTAGE_LDS"


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
    for k in (KNOB, "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)


def run(route, call, *args, **kw):
    """((stats, max_add, lat, unrouted), code) of a call, failed entries or not."""
    try:
        return call(*args, **kw), route.OK
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return err.partial, err.code


def compare(got, code, want, shape=None):
    st, mx, lat, un = got
    assert code in want.codes, (code, want.codes)
    assert un == want.unrouted
    assert st.dtype == np.uint64 and np.array_equal(st, want.stats), (st.tolist(), want.stats.tolist())
    assert mx.dtype == np.float64 and np.array_equal(mx, want.max_add), (mx.tolist(), want.max_add.tolist())
    if lat is not None:
        w = want.lat if shape is None else want.lat.reshape(shape)
        bad = np.argwhere(~((lat == w) | (np.isnan(lat) & np.isnan(w))))
        assert lat.shape == w.shape and len(bad) == 0, (len(bad), bad[:5].tolist())


def check_block(route, name, eng=None, scn=None, S=None, T=None, W=None):
    g = tout.graph(name)
    if S is None:
        S, T, W = tout.entries(name)
    scn = tout.scenarios(name) if scn is None else scn
    default = S is tout.entries(name)[0] and scn is tout.scenarios(name)
    want = tout.repaired(name) if default else tout.ref(name).repair(*orf.block_entries(S, T, W), scn)
    eng = eng or route.RouteEngine(g)
    got, code = run(route, eng.outage, S, T, scn, W, lat=True)
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


def sorted_pack(scn):
    return orf.pack([sorted(f) for f in scn])


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """The block's entries as shuffled pairs with a hundred repeats, and the reference over them."""
    S, T, W = tout.entries(name)
    ps, pt, pw = orf.block_entries(S, T, W)
    rng = np.random.default_rng(len(ps))
    k = np.concatenate([rng.permutation(len(ps)), rng.integers(0, max(len(ps), 1), size=100 if len(ps) else 0)])
    ps, pt, pw = ps[k], pt[k], pw[k]
    return ps, pt, pw, tout.ref(name).repair(ps, pt, pw, tout.scenarios(name))


# ---- every form on the small builders --------------------------------------------------------------

@pytest.mark.parametrize("lds", [None, "0"])
@pytest.mark.parametrize("name", tout.SMALL)
def test_every_form(route, monkeypatch, name, lds):
    """The block, the same entries as shuffled pairs with repeats, and the async call with
    ld > nt, each against the reference, in the LDS form and in HBM slices."""
    import torch
    if lds is not None:
        monkeypatch.setenv(KNOB, lds)
    g = tout.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = tout.entries(name)
    scn = tout.scenarios(name)
    _, _, want = check_block(route, name, eng)
    ps, pt, pw, wantp = pair_case(name)
    got, code = run(route, eng.pair_outage, ps, pt, scn, pw, lat=True)
    compare(got, code, wantp)
    # async: padded rows, canaries in the padding and in the outputs
    ns, nt, ld, nscn = len(S), len(T), len(T) + 3, len(scn)
    Wp = np.zeros((ns, ld), np.uint64); Wp[:, :nt] = W
    off, edge = sorted_pack(scn)
    dev = torch.device("cuda", 0)
    d_st = torch.full((nscn, 3), 7, dtype=torch.int64, device=dev)
    d_mx = torch.full((nscn,), 7.25, dtype=torch.float64, device=dev)
    d_lat = torch.full((nscn, ns, ld), 7.25, dtype=torch.float64, device=dev)
    d_un = torch.full((1,), 7, dtype=torch.int64, device=dev)
    eng.outage_async(_dev(S), _dev(T), _dev(Wp), _dev(off), _dev(edge) if len(edge) else _dev(np.zeros(1, np.int32)),
                     d_st, d_mx, d_lat, d_un, ld=ld)
    code = _sync(route, eng)
    lat = d_lat.cpu().numpy()
    assert np.all(lat[:, :, nt:] == 7.25)
    compare((d_st.cpu().numpy().view(np.uint64), d_mx.cpu().numpy(), np.ascontiguousarray(lat[:, :, :nt]),
             int(d_un.cpu().numpy().view(np.uint64)[0])), code, want, (nscn, ns, nt))


# ---- the larger shapes -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", tout.LARGE)
def test_shapes(route, name):
    """grid (1,056 vertices: more than one workgroup's threads, tied detours), the multigraphs,
    the directed graphs, fractional latencies, the lollipop's tail, second self-loops."""
    got, code, want = check_block(route, name)
    assert len(tout.scenarios(name)) >= 3
    if name == "grid":
        assert tout.graph(name).n == 1056


def test_natural_hbm16(route):
    """One vertex past the LDS limit: the u16 state in HBM slices without the knob."""
    name = tout.HBM16
    g = tout.graph(name)
    assert g.n == orf.lds_max_n() + 1 and not orf.fits_lds(g.n) and g.n <= 65535
    check_block(route, name)


def test_hbm32_ring(route):
    """66,000 vertices: u32 lists.  One failed edge near the antipode of the source, at most 16
    affected vertices, so the repair takes a few sweeps."""
    s, e, ts = tout.ring_case()
    R = tout.ref("ring66k")
    want = R.repair([s] * len(ts), ts, None, [[e]])
    assert want.stats[0, orf.HIT] >= 1
    eng = route.RouteEngine(tout.graph("ring66k"))
    got, code = run(route, eng.outage, [s], ts, [[e]], lat=True)
    compare(got, code, want, (1, 1, len(ts)))


# ---- against a context of the reduced graph ----------------------------------------------------------

@pytest.mark.parametrize("name,sel", [("sized63", "auto"), ("sized63", "kd"), ("multi389", "auto"), ("multi389", "kd"),
                                      ("frac_multi", "kf"), ("dir_grid", "auto")])
def test_fresh_context(route, monkeypatch, name, sel):
    """lat[k] is bit-equal to the rows of a context created from the reduced graph, flags 0.
    (shd_route_create refuses a reduced graph that is no longer connected: a scenario that cuts
    vertices off has no such context and is compared with the reference alone.)"""
    select(monkeypatch, sel)
    g = tout.graph(name)
    S, T, W = tout.entries(name)
    scn = [f for f in tout.scenarios(name) if f][:6] + [[]]
    eng = route.RouteEngine(g)
    got, _ = run(route, eng.outage, S, T, scn, W, lat=True)
    want = tout.ref(name).repair(*orf.block_entries(S, T, W), scn)
    done = 0
    for k, f in enumerate(scn):
        try:
            ek = route.RouteEngine(orf.reduced(g, f))
        except route.RouteError as err:
            assert err.code == route.EINVAL and want.stats[k, orf.CUT] > 0
            continue
        done += 1
        try:
            lat = ek.rows(S, T, dispatch=False)[0]
        except route.RouteError as err:
            lat = err.partial[0]
        old_failed = np.isnan(tout.repaired(name).lat[0].reshape(len(S), len(T)))
        lat = np.where(old_failed, np.nan, lat)       # an entry that fails in the whole graph takes no part
        assert np.array_equal(got[2][k], lat, equal_nan=True), (name, sel, k)
        ek.close()
    assert done >= 4 and want.stats[:, orf.HIT].any()


# ---- many scenarios, many units ----------------------------------------------------------------------

def test_full_sweep(route):
    """One source of sized1000, every edge its own scenario: 3,658 scenarios in 915 slabs of 4."""
    g = tout.graph("sized1000")
    S, T, want = tout.sweep_case()
    eng = route.RouteEngine(g)
    got, code = run(route, eng.outage, S, T, [[e] for e in range(g.m)], lat=True)
    compare(got, code, want, (g.m, 1, g.n))
    assert g.m > 3000 and orf.units(1, g.m) == (4, 915, 915) and want.stats[:, orf.SLOWER].any()


def test_more_units_than_slots(route, monkeypatch):
    """The HBM form with 16 slices and 3 sources x 60 single-edge scenarios in 180 units."""
    name = "sized63"
    g = tout.graph(name)
    monkeypatch.setenv(KNOB, "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 16 * g.n))
    stride = orf.a16(orf.layout_total(g.n))
    S = np.array([0, 31, 62], np.int32)
    scn = [[e] for e in range(60)]
    form = orf.state_form(g.n, orf.units(len(S), len(scn))[2], True, 4 * 16 * g.n // 4)
    assert form[0] == 2 and form[4] == 16 and orf.units(len(S), len(scn))[2] == 180 > form[1] and stride > 0
    check_block(route, name, scn=scn, S=S, T=np.arange(g.n, dtype=np.int32), W=tout.weights(name, 3, g.n))


@pytest.mark.parametrize("lds", [None, "0"])
def test_source_chunks(route, monkeypatch, lds):
    """Scratch for three sources per chunk, seven sources: the statistics add up across three
    chunks and every chunk writes its rows of every scenario's latencies."""
    name = "ba64_ties"
    g = tout.graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    if lds is not None:
        monkeypatch.setenv(KNOB, lds)
    S = tout.sources(name)[:7]
    T = np.arange(g.n, dtype=np.int32)
    check_block(route, name, scn=tout.scenarios(name)[:6], S=S, T=T, W=tout.weights(name, 7, g.n))
    ps, pt, pw = orf.block_entries(S, T, tout.weights(name, 7, g.n))
    eng = route.RouteEngine(g)
    got, code = run(route, eng.pair_outage, ps[::-1], pt[::-1], tout.scenarios(name)[:6], pw[::-1], lat=True)
    compare(got, code, tout.ref(name).repair(ps[::-1], pt[::-1], pw[::-1], tout.scenarios(name)[:6]))


# ---- failed entries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name,code", [("tiny3_none", orf.ENOEDGE), ("tiny9_some", orf.ENOEDGE),
                                       ("ba60_holes", orf.ENOEDGE)])
def test_failed_entries(route, name, code):
    """Entries that fail in the whole graph: the code, their weight in unrouted once whatever the
    number of scenarios, NaN in every scenario's latencies and no part in any statistic.  (An
    unreachable target cannot be had on a device: shd_route_create refuses a graph that is not
    connected; tests/test_outage.py holds the references together on one.)"""
    g = tout.graph(name)
    S, T, W = tout.entries(name)
    scn = tout.scenarios(name)
    got, rc, want = check_block(route, name)
    failed = np.isnan(want.lat[0]).reshape(len(S), len(T))
    assert code in want.codes and rc in want.codes and failed.any() and len(scn) >= 3
    assert got[3] == int(W[failed].sum()) > 0
    assert np.all(np.isnan(got[2][:, failed]))
    only = np.where(failed, W, 0).astype(np.uint64)                # the failed entries alone: no statistic
    eng = route.RouteEngine(g)
    g2, rc2 = run(route, eng.outage, S, T, scn, only)
    assert not g2[0].any() and g2[3] == got[3] and rc2 == rc
    assert np.array_equal(g2[1], want.max_add)                      # (an entry of weight 0 is still an entry)


# ---- arguments and outputs ---------------------------------------------------------------------------

def test_refused_arguments(route):
    import torch
    name = "sized63"
    g = tout.graph(name)
    eng = route.RouteEngine(g)
    L = route.load_library()
    S, T = np.array([0, 5], np.int32), np.arange(g.n, dtype=np.int32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    st, mx, un = np.full((2, 3), 7, np.uint64), np.full(2, 7.25), np.full(1, 7, np.uint64)
    lat = np.full((2, 2, g.n), 7.25)

    def host(s, t, off, edge, flags=0):
        off, edge = np.asarray(off, np.int64), np.asarray(edge, np.int32)
        return L.shd_route_outage(eng._h, P(s), len(s), P(t), len(t), flags, None, P(off), P(edge), len(off) - 1,
                                  P(st), P(mx), P(lat), P(un))

    def pairs(s, t, off, edge, flags=0):
        off, edge = np.asarray(off, np.int64), np.asarray(edge, np.int32)
        return L.shd_route_pair_outage(eng._h, P(s), P(t), None, len(s), flags, P(off), P(edge), len(off) - 1,
                                       P(st), P(mx), P(lat), P(un))
    ok_off, ok_edge = [0, 1, 3], [4, 9, 2]
    for call in (host, pairs):
        s, t = (S, T) if call is host else (np.array([0, 5], np.int32), np.array([7, 9], np.int32))
        assert call(s, t, ok_off, ok_edge, route.DISPATCH) == route.EINVAL
        assert call(s, t, ok_off, ok_edge, 0x400) == route.EINVAL
        assert call(s, t, ok_off, [4, g.m, 2]) == route.EINVAL
        assert call(s, t, ok_off, [4, -1, 2]) == route.EINVAL
        assert call(s, t, [0, 2, 1], ok_edge) == route.EINVAL
        assert call(np.array([0, g.n], np.int32), t, ok_off, ok_edge) == route.EINVAL
        assert call(s, np.where(t == 9, -1, t).astype(np.int32), ok_off, ok_edge) == route.EINVAL
        assert np.all(st == 7) and np.all(mx == 7.25) and np.all(lat == 7.25) and un[0] == 7   # nothing written
    assert host(S, T, ok_off, ok_edge) == route.OK and un[0] == 0 and not np.any(lat == 7.25)
    # async: the flags at once, the scenarios' order and range by the validation kernel
    dS, dT = _dev(S), _dev(T)
    d_st = torch.zeros((2, 3), dtype=torch.int64, device=dS.device)
    with pytest.raises(route.RouteError) as ei:
        eng.outage_async(dS, dT, None, _dev(np.array(ok_off, np.int64)), _dev(np.array([4, 2, 9], np.int32)), d_st, None,
                         None, None, flags=route.DISPATCH)
    assert ei.value.code == route.EINVAL
    for off, edge in ((ok_off, [4, 9, 2]), (ok_off, [4, 2, g.m]), (ok_off, [4, -5, 2]), ([0, 2, 1], [4, 2, 9]),
                      ([1, 1, 3], [4, 2, 9])):
        eng.outage_async(dS, dT, None, _dev(np.array(off, np.int64)), _dev(np.array(edge, np.int32)), d_st, None, None,
                         None)
        assert _sync(route, eng) == route.EINVAL, (off, edge)
    eng.outage_async(dS, dT, None, _dev(np.array(ok_off, np.int64)), _dev(np.array([4, 2, 9], np.int32)), d_st, None,
                     None, None)
    assert _sync(route, eng) == route.OK
    want = tout.ref(name).repair(*orf.block_entries(S, T), [[4], [2, 9]])
    assert np.array_equal(d_st.cpu().numpy().view(np.uint64), want.stats)


def test_no_and_empty_scenarios(route):
    """nscn == 0 writes only unrouted; empty scenarios give zeros and the old rows."""
    name = "ba60_holes"
    g = tout.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = tout.entries(name)
    want = tout.ref(name).repair(*orf.block_entries(S, T, W), [[], []])
    assert want.unrouted > 0
    got, code = run(route, eng.outage, S, T, [], W, lat=True)
    assert got[0].shape == (0, 3) and got[1].shape == (0,) and got[3] == want.unrouted and code == route.ENOEDGE
    got, code = run(route, eng.pair_outage, *orf.block_entries(S, T)[:2], [], orf.block_entries(S, T, W)[2])
    assert got[3] == want.unrouted and code == route.ENOEDGE
    got, code = run(route, eng.outage, S, T, [[], []], W, lat=True)
    compare(got, code, want, (2, len(S), len(T)))
    assert not got[0].any() and not got[1].any()
    try:
        old = eng.rows(S, T, dispatch=False)[0]
    except route.RouteError as err:
        old = err.partial[0]
    assert np.array_equal(got[2][0], old, equal_nan=True) and np.array_equal(got[2][1], old, equal_nan=True)
    # nothing to route
    z = eng.outage(np.zeros(0, np.int32), T, [[1]], lat=True)
    assert not z[0].any() and z[3] == 0


def test_each_output_alone(route):
    name = "sized63"
    g = tout.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = tout.entries(name)
    scn = tout.scenarios(name)
    want = tout.repaired(name)
    nscn = len(scn)
    for keep in range(4):
        out = [np.full((nscn, 3), 7, np.uint64), np.full(nscn, 7.25), np.full((nscn, len(S), len(T)), 7.25),
               np.full(1, 7, np.uint64)]
        out = [o if k == keep else None for k, o in enumerate(out)]
        got, code = run(route, eng.outage, S, T, scn, W, lat=True, out=tuple(out))
        assert [x is None for x in got] == [k != keep for k in range(4)]
        full = [want.stats, want.max_add, want.lat.reshape(nscn, len(S), len(T)), want.unrouted]
        assert np.array_equal(got[keep], full[keep], equal_nan=True) if keep < 3 else got[3] == full[3]
    ps, pt, pw, wantp = pair_case(name)
    got, code = run(route, eng.pair_outage, ps, pt, scn, pw, out=(None, np.full(nscn, 7.25), None, None))
    assert np.array_equal(got[1], wantp.max_add)


# ---- stream order --------------------------------------------------------------------------------------

def test_gated_outage(route, monkeypatch):
    """outage_async behind the timed gate of tests/stream_order.py, in three chunks: decoy inputs
    until the gate opens, two calls with the canary in between, and the call returns while the
    gate is shut."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(3 * 16 * g.n))
    S = A[:7].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    R = orf.OutageRef(g)
    scn = tout.scenarios(name)[:6]
    nscn = len(scn)
    W = tout.weights(name, ns, nt)
    Wp = np.zeros((ns, nt + 1), np.uint64); Wp[:, :nt] = W
    want = R.repair(*orf.block_entries(S, T, W), scn)
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    Wd = np.roll(W, 7, axis=1)
    Wdp = np.zeros_like(Wp); Wdp[:, :nt] = Wd
    scd = scn[::-1]                                                     # the decoy: the scenarios reversed
    for s, t, w, q in ((Sd, T, W, scn), (S, Td, W, scn), (S, T, Wd, scn), (S, T, W, scd)):
        one = R.repair(*orf.block_entries(s, t, w), q)                  # an early reader gets other results
        assert not np.array_equal(one.stats, want.stats)
    off, edge = sorted_pack(scn)
    offd, edged = sorted_pack(scd)
    pad = max(len(edge), len(edged))
    edge, edged = np.resize(edge, pad), np.resize(edged, pad)
    eng = route.RouteEngine(g)
    i_s, i_t, i_w, i_o, i_e = so.In(S, Sd), so.In(T, Td), so.In(Wp, Wdp), so.In(off, offd), so.In(edge, edged)
    outs = [so.Out(nscn, 3, i64=True), so.Out(1, nscn), so.Out(nscn * ns, nt + 1), so.Out(1, 1, i64=True)]
    code = so.gated(route, eng, [i_s, i_t, i_w, i_o, i_e], outs,
                    lambda sh: eng.outage_async(i_s.t, i_t.t, i_w.t, i_o.t, i_e.t, *[o.t for o in outs], stream=sh,
                                                ld=nt + 1),
                    "outage_async")
    got = (outs[0].snap_bits(3).view(np.uint64), outs[1].f64(nscn)[0], outs[2].f64(nt).reshape(nscn, ns, nt),
           int(outs[3].snap_bits(1)[0].view(np.uint64)[0]))
    compare(got, code, want, (nscn, ns, nt))


# ---- the context is left as it was -----------------------------------------------------------------------

def test_context_left_intact(route):
    """rows, hops and loads on the same context after outage calls still equal their references."""
    name = "multi389"
    g = tout.graph(name)
    eng = route.RouteEngine(g)
    S, T, W = tout.entries(name)
    check_block(route, name, eng)
    check_block(route, name, eng)
    R = Ref(g)
    lat, rel, hops = R.rows(S, T, dispatch=False)

    def partial(call, *a, **k):
        try:
            return call(*a, **k)
        except route.RouteError as err:
            assert err.code == route.ENOEDGE              # multi389 lacks some self-loops
            return err.partial
    got = partial(eng.rows, S, T, dispatch=False)
    assert np.array_equal(got[0], lat, equal_nan=True) and np.allclose(got[1], rel, rtol=1e-12, atol=0, equal_nan=True)
    assert np.array_equal(partial(eng.hops, S, T, dispatch=False)[0], hops)
    ps, pt, pw = orf.block_entries(S, T, W)
    el, tr, un = R.loads(ps, pt, pw, dispatch=False)
    gl = partial(eng.loads, S, T, W, dispatch=False)
    assert np.array_equal(gl[0], el) and np.array_equal(gl[1], tr) and gl[2] == un
    check_block(route, name, eng)


# ---- the front end -------------------------------------------------------------------------------------

def test_front_end_link_outage(topo, route):
    """Packet counters on a few hundred stored pairs, one past 2^32: link_outage equals the
    reference over the stored pairs (lower -> higher); all zero before the first fill; nothing
    cached moves."""
    name = "ba64_ties"
    g, A = hg._graph(name)
    assert not g.prefer_direct
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    scn = tout.scenarios(name)
    z = t.link_outage(scn)
    assert z[0].shape == (len(scn), 3) and not z[0].any() and not z[1].any() and z[2] == 0   # before the fill
    assert t.get_latency(int(A[0]), int(A[1])) >= 0
    z = t.link_outage(scn)
    assert not z[0].any() and not z[1].any() and z[2] == 0                                   # no packets yet
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
    want = orf.OutageRef(g).repair(ps, pt, pw, scn)
    got = t.link_outage(scn)
    assert np.array_equal(got[0], want.stats) and np.array_equal(got[1], want.max_add) and got[2] == want.unrouted
    assert want.stats[:, orf.HIT].any() and want.stats.max() > 2 ** 32
    assert np.array_equal(t.link_outage(orf.pack(scn))[0], want.stats)                       # the (off, edge) form
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        t.link_outage([[g.m]])
    assert snap() == was
    t.close()


@pytest.mark.parametrize("name", ["ba80_prefer", "k24"])
def test_front_end_dispatching_cache_is_unsupported(topo, route, name):
    g, A = hg._graph(name)
    t = topo.Topology.from_graph(g)
    t.attach_all(np.sort(A))
    assert route.EUNSUPPORTED == -6
    with pytest.raises(RuntimeError, match=r"\(-6\)"):
        t.link_outage([[0]])
    t.close()


# ---- two live contexts ------------------------------------------------------------------------------------

def test_two_live_contexts(route):
    """A context at the LDS limit and one of 64 vertices, both in the LDS form, their calls
    alternated: the dynamic-LDS limit of the kernel is raised once per context, each launch takes
    its own context's state size, columns and scratch, and each still equals its reference."""
    big, small = f"sized{orf.lds_max_n()}", "ba64_ties"
    gb, gs = tout.graph(big), tout.graph(small)
    assert orf.fits_lds(gb.n) and orf.fits_lds(gs.n) and orf.layout_total(gb.n) > 100 * orf.layout_total(gs.n)
    eb = route.RouteEngine(gb)
    es = route.RouteEngine(gs)
    for _ in range(2):
        _, _, wb = check_block(route, big, eb)
        _, _, ws = check_block(route, small, es)
    assert wb.stats[:, orf.HIT].any() and ws.stats[:, orf.HIT].any()
