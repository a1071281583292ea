"""GPU: the seven families of path calls -- hops / routes / loads, the tie envelope, the ECMP loads,
the path folds, the link loss and the link outages -- on the fractional-latency graphs of
tests/frac_graphs.py, whose shortest paths tie or miss a tie by an ulp in f64
(tests/test_frac_graphs.py holds the builders to that).  All of them read the chosen paths out of finished distance rows by one rule: an arc u -> v is on
a shortest path exactly when d[u] + w == d[v] in double.  A kernel that compares with a tolerance,
sums in another order, or reads a latency through another conversion than the rows kernel did
(KFH's packed k / scale arcs against the f64 in-CSR of the path calls, the out-CSR copy of a
weight against the in-CSR copy) passes every integer-latency test and fails here.

Every builder runs under four rows selections, each asserted through eng.info --

  default   no knob                                  KF (kernel 5), state in LDS
  kfh       SHD_ROUTE_KFH=1                          KF with HBM slices, arcs packed at the builder's
                                                     decimal scale (reserved = 10, 100; 0 where k
                                                     passes 65535: frac_thousandths)
  kfh_f64   SHD_ROUTE_KFH=1 SHD_ROUTE_KFPK=0         the same with f64 arcs (reserved 0)
  f64       SHD_ROUTE_KERNEL=f64                     the generic kernel (kernel 0)

-- and in both state forms of every path call ("lds": no knob; "hbm": SHD_ROUTE_HOPS_LDS,
LOADS_LDS, TIES_LDS, ECMP_LDS, FOLD_LDS, LOSS_LDS and OUTAGE_LDS all 0): the whole cross product,
up to half a second a case.
About 24 sources spread over the graph, every vertex a target.

What is compared, and how:
  hops, routes, loads   equal multi_ref.Ref exactly; every route's latencies folded from the source
                        equal the rows' entry bit for bit
  ties                  count, rel_lo, rel_hi equal ties_ref.TiesRef exactly (test_ties_gpu.check)
  ECMP                  within ecmp_ref's derived tolerance (test_ecmp_gpu.check), unit weights and
                        one weighted run; exactly shd_route_loads on the entries with one path
  folds                 sum / min / max of the latency column and the product of 1 - loss in one
                        call, to the bit against fold_ref (test_fold_gpu.check); the sum is the
                        rows' lat, the product the rows' rel where neither end has a vertex factor
  loss                  the weighted block within loss_ref's derived bound (R + 4 + A) * 2^-52 of the
                        exact fractions; six one-source calls bit-equal to the plain f64 programme
                        (no element takes more than two addends); with unit weights delivered is
                        the rows' rel where neither end has a vertex factor
  outages               the scenarios of tests/test_frac_graphs.py (the edges of the route from the
                        first to the last source, singly and the first two together, and none):
                        stats, max_add, unrouted and every new latency equal outage_ref.OutageRef
                        exactly.  SLOWER is new > old in f64, max_add one f64 subtraction, and some
                        entries get slower by exactly one ulp (frac_hub: 2^-54).  In the "lds" form
                        up to three scenarios are also held to a context created from the reduced
                        graph under the same selection: lat[k] is bit-equal to its rows
  across selections     hops, routes, loads, ties, folds, the outage outputs and the one-source loss
                        outputs are array_equal to the default selection's; the block loss outputs
                        within twice their bound, as the ECMP loads are.  The ECMP loads are compared
                        within twice the derived tolerance: a vertex's state is a fixed-order sum, but the per-source
                        contributions reach the output arrays by floating-point atomic adds, whose
                        order is not fixed from launch to launch.
"""
import functools

import numpy as np
import pytest

from shadow_amd.graph import to_graphml
from tests import fold_ref as fr
from tests import frac_graphs as fg
from tests import loss_ref as lr
from tests import outage_ref as orf
from tests import test_ecmp_gpu as eg
from tests import test_fold_gpu as dg
from tests import test_frac_graphs as tfg
from tests import test_hops_gpu as hg
from tests import test_ties_gpu as tg
from tests.multi_ref import Ref
from tests.test_multi_gpu import call, split
from tests.test_range_gpu import REL_TOL, select

pytestmark = pytest.mark.gpu

SELECTIONS = {
    "default": {},
    "kfh": {"SHD_ROUTE_KFH": "1"},
    "kfh_f64": {"SHD_ROUTE_KFH": "1", "SHD_ROUTE_KFPK": "0"},
    "f64": {"SHD_ROUTE_KERNEL": "f64"},
}
FORM_KNOBS = ("SHD_ROUTE_HOPS_LDS", "SHD_ROUTE_LOADS_LDS", "SHD_ROUTE_TIES_LDS", "SHD_ROUTE_ECMP_LDS",
              "SHD_ROUTE_FOLD_LDS", "SHD_ROUTE_LOSS_LDS", "SHD_ROUTE_OUTAGE_LDS")
LOSS_ONE = 6        # one-source loss calls per builder
REDUCED = 3         # scenarios held to a context of the reduced graph
OPS = [fr.SUM, fr.MIN, fr.MAX, fr.PROD]


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


def choose(monkeypatch, sel, form):
    select(monkeypatch, "auto")                               # every rows knob unset
    for k in FORM_KNOBS + ("SHD_ROUTE_HOPS_SCRATCH",):
        monkeypatch.delenv(k, raising=False)
    for k, v in SELECTIONS[sel].items():
        monkeypatch.setenv(k, v)
    if form == "hbm":
        for k in FORM_KNOBS:
            monkeypatch.setenv(k, "0")


def packed_scale(name):
    """The scale KFH packs the builder's arcs at: the smallest of 1, 10, 100, 1000 that holds
    every latency as an integer up to 65535; 0 where none does."""
    g = fg.get(name)
    w = g.latency[g.src != g.dst]
    for sc in (1, 10, 100, 1000):
        k = np.rint(w * sc)
        if k.min() >= 1 and k.max() <= 65535 and np.array_equal(k / sc, w):
            return sc
    return 0


def expect_info(name, sel, info):
    if sel == "f64":
        assert info["kernel"] == 0
        return
    assert info["kernel"] == 5 and info["lds_resident"] == (1 if sel == "default" else 0), info
    if sel == "kfh":
        assert info["reserved"] == packed_scale(name)
        if name in ("frac_cents", "frac_grid_cents"):         # two decimals, as C2f in test_kf_packed_arcs
            assert info["reserved"] == 100
        assert (info["reserved"] == 0) == (name == "frac_thousandths")
    else:
        assert info["reserved"] == 0


def columns(g):
    """The four value columns of the one fold call: latency three times, then 1 - loss."""
    return np.stack([g.latency, g.latency, g.latency, 1.0 - np.asarray(g.packetloss, np.float64)])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The Ref's answers for the builder's sources over every vertex, computed once: rows, every
    route, and the loads of one fixed weight block; read-only."""
    g = fg.get(name)
    R = Ref(g)
    S, T = fg.sources(name), np.arange(g.n, dtype=np.int32)
    lat, rel, hops = R.rows(S, T)
    ps, pt = np.repeat(S, g.n).astype(np.int32), np.tile(T, len(S)).astype(np.int32)
    routes = [R.path(s, t) for s, t in zip(ps.tolist(), pt.tolist())]
    assert all(p is not None for p in routes) and not np.isnan(lat).any()
    W = np.random.default_rng(g.n).integers(1, 1 << 40, size=(len(S), g.n), dtype=np.uint64)
    loads = R.loads(ps, pt, W.reshape(-1))
    cnt = tg.ref(name).rows(S, T, False)[0]
    for a in (lat, rel, hops, W, cnt) + loads[:2]:
        a.setflags(write=False)
    vf = R.vf
    plain = np.isnan(vf)[S][:, None] & np.isnan(vf)[None, :]  # neither end has a vertex factor
    bare = np.isnan(vf)[None, :] | (T[None, :] == S[:, None])  # no factor of the target's to place
    # link loss: the weighted block in exact fractions, LOSS_ONE one-source calls in plain f64
    assert np.array_equal(W, tfg.path_weights(name))
    L = lr.LossRef(g)
    loss = L.block(S, T, W, exact=True)
    one_at = np.unique(np.linspace(0, len(S) - 1, LOSS_ONE).astype(int))
    loss_one = [L.block(S[i:i + 1], T, W[i:i + 1]) for i in one_at.tolist()]
    assert not loss.codes and loss.unrouted == 0 and loss.A > 2 and all(o.A <= 2 and not o.codes for o in loss_one)
    # link outages: the scenario rule and the programme's result of tests/test_frac_graphs.py
    _, scn, outage = tfg.outage_case(name)
    assert outage.codes == frozenset({0}) and not outage.stats[:, orf.CUT].any()
    return dict(g=g, R=R, S=S, T=T, lat=lat, rel=rel, hops=hops, ps=ps, pt=pt, routes=routes, W=W, loads=loads,
                cnt=cnt, plain=plain, bare=bare, loss=loss, one_at=one_at, loss_one=loss_one, scn=scn, outage=outage)


def run_all(route, name, form):
    """Every path call of one context against its reference; the outputs for the comparison
    across selections.  form "lds": also the outage's new latencies against contexts of the
    reduced graphs, created under the selection in force."""
    ref = reference(name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    eng = route.RouteEngine(g)
    out = {"info": dict(eng.info)}
    off = T[None, :] != S[:, None]
    # rows, hops, routes, loads
    (lat, rel, _), c = call(route, eng.rows, S, T, dispatch=False)
    assert c == route.OK and np.array_equal(lat, ref["lat"])
    # rel: to the bit where the target has no vertex factor (or is the source itself); with one, a
    # kernel that walks the route folds it in first, as the reference does, and a level sweep
    # multiplies it in last: within REL_TOL, the rule of test_range_gpu.py
    assert np.array_equal(rel[ref["bare"]], ref["rel"][ref["bare"]])
    np.testing.assert_allclose(rel, ref["rel"], rtol=REL_TOL, atol=0)
    (hops, mx), c = call(route, eng.hops, S, T, dispatch=False)
    assert c == route.OK and np.array_equal(hops, ref["hops"]) and np.array_equal(mx, ref["hops"].max(axis=1))
    (poff, vert, edge), c = call(route, eng.paths, ref["ps"], ref["pt"], dispatch=False)
    assert c == route.OK
    got = split(route, poff, vert, edge)
    w = g.latency.tolist()
    for k, want in enumerate(ref["routes"]):
        assert got[k] == (want[0], want[1]), (ref["ps"][k], ref["pt"][k])
        L = 0.0
        for e in got[k][1]:
            L = L + w[e]
        assert L == lat[k // g.n, k % g.n], (ref["ps"][k], ref["pt"][k])
    (el, trn, un), c = call(route, eng.loads, S, T, ref["W"], dispatch=False)
    assert c == route.OK and np.array_equal(el, ref["loads"][0]) and np.array_equal(trn, ref["loads"][1])
    assert un == ref["loads"][2] == 0
    out.update(lat=lat, rel=rel, hops=hops, poff=poff, vert=vert, edge=edge, el=el, trn=trn)
    # ties
    (cnt, lo, hi), _ = tg.check(route, name, S, eng=eng)
    assert np.array_equal(cnt, ref["cnt"])
    one = cnt == 1
    assert np.array_equal(lo[one], hi[one]) and np.array_equal(rel[one & ref["plain"]], lo[one & ref["plain"]])
    out.update(cnt=cnt, lo=lo, hi=hi)
    # ECMP: unit weights, a weighted run, and the entries with one path against shd_route_loads
    e1, _ = eg.check(route, name, S, eng=eng)
    W20 = eg.weights(g.n, len(S), g.n)
    e2, _ = eg.check(route, name, S, W20, eng=eng)
    W1 = np.where(one, ref["W"], np.uint64(0)).astype(np.uint64)
    assert np.count_nonzero(one & off) > g.n
    single = eg.run(route, eng.loads, S, T, W1, dispatch=False)
    e3 = eg.run(route, eng.ecmp_loads, S, T, W1, dispatch=False)
    assert int(single[0].max()) < 2 ** 53 and single[0].any() and single[1].any()
    assert np.array_equal(e3[0], single[0].astype(np.float64)) and np.array_equal(e3[1], single[1].astype(np.float64))
    assert e3[2] == single[2] == 0 and e3[3] == single[3] == route.OK
    out.update(e1=e1[:2], e2=e2[:2], e3=e3[:2])
    # folds: four in one call
    fold, _, c = dg.check(route, name, S, eng=eng, ops=OPS, vals=columns(g))
    assert c == route.OK
    assert np.array_equal(fold[0][off], lat[off])
    assert np.all(fold[1] <= fold[2]) and np.all(fold[2] <= fold[0])
    assert np.array_equal(fold[3][ref["plain"]], rel[ref["plain"]])
    out.update(fold=fold)
    # link loss: the block, the one-source calls, unit weights
    want = ref["loss"]
    lb, c = call(route, eng.loss, S, T, ref["W"], dispatch=False)
    assert c == route.OK and lb[4] == 0
    for k in range(4):
        assert lr.close(lb[k], want.outs()[k], want.R, want.A), (lr.NAMES[k], want.R, want.A)
    ones = []
    for i, w1 in zip(ref["one_at"].tolist(), ref["loss_one"]):
        lo1, c = call(route, eng.loss, S[i:i + 1], T, ref["W"][i:i + 1], dispatch=False)
        assert c == route.OK and lo1[4] == 0
        for k in range(4):
            assert np.array_equal(lo1[k], w1.arrays()[k]), (int(S[i]), lr.NAMES[k])
        ones.append(np.concatenate(lo1[:4]))
    i = len(S) // 2
    lu, c = call(route, eng.loss, S[i:i + 1], T, None, dispatch=False)
    assert c == route.OK and np.array_equal(lu[3][ref["plain"][i]], rel[i][ref["plain"][i]])
    out.update(loss=lb[:4], loss_one=np.stack(ones))
    # link outages
    scn, wo = ref["scn"], ref["outage"]
    (st, mx, nl, un), c = call(route, eng.outage, S, T, scn, ref["W"], lat=True)
    assert c == route.OK and un == wo.unrouted == 0
    assert np.array_equal(st, wo.stats) and np.array_equal(mx, wo.max_add), (st.tolist(), mx.tolist())
    assert np.array_equal(nl, wo.lat.reshape(len(scn), len(S), len(T)))
    assert np.array_equal(nl[-1], lat) and scn[-1] == []      # no failed edge: the rows themselves
    out.update(ostats=st, omax=mx, olat=nl)
    if form == "lds":
        for k, f in [(k, f) for k, f in enumerate(scn) if f][:REDUCED]:
            assert wo.stats[k, orf.HIT] > 0 and wo.stats[k, orf.CUT] == 0
            ek = route.RouteEngine(orf.reduced(g, f))
            assert ek.info["kernel"] == eng.info["kernel"] and ek.info["lds_resident"] == eng.info["lds_resident"]
            (rl, _, _), c = call(route, ek.rows, S, T, dispatch=False)
            assert c == route.OK and np.array_equal(nl[k], rl), (name, k, f)
            ek.close()
    return out


_BASE = {}


def base_outputs(route, monkeypatch, name, form):
    """The default selection's outputs of (builder, form), run once per session."""
    if (name, form) not in _BASE:
        with monkeypatch.context() as m:
            choose(m, "default", form)
            _BASE[name, form] = run_all(route, name, form)
    return _BASE[name, form]


@pytest.mark.parametrize("form", ["lds", "hbm"])
@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("name", list(fg.SUITE))
def test_path_calls(route, monkeypatch, name, sel, form):
    base = base_outputs(route, monkeypatch, name, form)
    expect_info(name, "default", base["info"])
    if sel == "default":
        if form == "hbm":                                     # the two state forms against each other
            lds = base_outputs(route, monkeypatch, name, "lds")
            for k in ("hops", "poff", "vert", "edge", "el", "trn", "cnt", "lo", "hi", "fold", "loss_one", "ostats",
                      "omax", "olat"):
                assert np.array_equal(base[k], lds[k], equal_nan=True), k
        return
    choose(monkeypatch, sel, form)
    got = run_all(route, name, form)
    expect_info(name, sel, got["info"])
    for k in ("lat", "hops", "poff", "vert", "edge", "el", "trn", "cnt", "lo", "hi", "fold", "loss_one", "ostats", "omax",
              "olat"):
        assert np.array_equal(got[k], base[k], equal_nan=True), k
    bare = reference(name)["bare"]                            # (the rows' rel is no path call: see run_all)
    assert np.array_equal(got["rel"][bare], base["rel"][bare])
    rtol = 2 * eg.ref(name).tol(fg.sources(name))
    exact = True
    for k in ("e1", "e2"):
        for a, b in zip(got[k], base[k]):
            exact &= bool(np.array_equal(a, b))
            assert np.array_equal(a == 0, b == 0) and np.all(np.abs(a - b) <= rtol * b), k
    for a, b in zip(got["e3"], base["e3"]):
        assert np.array_equal(a, b)                           # whole numbers below 2^53: any order
    print(f"{name} {sel} {form}: ECMP loads bit-equal to the default selection's: {exact}")
    want = reference(name)["loss"]
    b2 = float(2 * lr.bound(want.R, want.A))
    for a, b in zip(got["loss"], base["loss"]):
        assert np.array_equal(a == 0, b == 0) and np.all(np.abs(a - b) <= b2 * b), "loss"


# ---- the pair forms ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(fg.SUITE))
def test_pair_forms(route, monkeypatch, name):
    """200 random pairs, 20 of them twice, a few self pairs: pair_loads, pair_ecmp_loads, pair_fold
    and paths in the caller's order."""
    choose(monkeypatch, "default", "lds")
    ref = reference(name)
    g, R = ref["g"], ref["R"]
    rng = np.random.default_rng(200 + g.n)
    S = fg.sources(name)
    ps = rng.choice(S, size=200).astype(np.int32)
    pt = rng.integers(0, g.n, size=200).astype(np.int32)
    pt[:5] = ps[:5]
    ps, pt = np.concatenate([ps, ps[40:60]]), np.concatenate([pt, pt[40:60]])
    pw = rng.integers(1, 1 << 20, size=len(ps), dtype=np.uint64)
    eng = route.RouteEngine(g)
    expect_info(name, "default", eng.info)
    (off, vert, edge), c = call(route, eng.paths, ps, pt, dispatch=False)
    want = [R.path(s, t) for s, t in zip(ps.tolist(), pt.tolist())]
    assert c == route.OK and split(route, off, vert, edge) == [(p[0], p[1]) for p in want]
    el, trn, un = R.loads(ps, pt, pw)
    (gel, gtr, gun), c = call(route, eng.pair_loads, ps, pt, pw, dispatch=False)
    assert c == route.OK and np.array_equal(gel, el) and np.array_equal(gtr, trn) and gun == un == 0
    E = eg.ref(name)
    pr = E.pairs(ps, pt, pw)
    mult = int(np.unique(ps.astype(np.int64) * g.n + pt, return_counts=True)[1].max())
    rtol = E.tol(sorted(set(ps.tolist())), mult=mult)
    got = eg.run(route, eng.pair_ecmp_loads, ps, pt, pw, dispatch=False)
    assert eg.same(got[0], pr[0], rtol) and eg.same(got[1], pr[1], rtol) and got[2] == pr[2] == 0 and got[3] == route.OK
    fw, codes = dg.ref(name).pairs(ps, pt, OPS, columns(g))
    pf, c = dg.run(route, eng.pair_fold, ps, pt, OPS, columns(g), dispatch=False)
    assert c == route.OK and not codes and fr.same(pf, fw)
    k = np.searchsorted(S, ps)
    assert np.array_equal(pf[0], ref["lat"][k, pt])           # self pairs too: 0.0 + w is w


# ---- the front end ------------------------------------------------------------------------------------

def test_front_end(topo, tmp_path, monkeypatch):
    """frac_cents through graphml: get_path and format_path give the route calls' routes, the line
    in route_fmt's format with the fractional latencies as %f prints them, and ecmp_link_loads the
    reference's split of the packet counters."""
    choose(monkeypatch, "default", "lds")
    name = "frac_cents"
    ref = reference(name)
    g, R = ref["g"], ref["R"]
    pth = tmp_path / "frac_cents.graphml.xml"
    to_graphml(g, str(pth))
    t = topo.Topology.new(str(pth))
    ids = [g.vertex_id(v) for v in range(g.n)]
    A = np.arange(0, g.n, 3, dtype=np.int32)
    t.attach_all(A)
    rng = np.random.default_rng(g.n)
    P = rng.choice(A, size=(120, 2))
    P[:4, 1] = P[:4, 0]
    lat = {}
    for s, d in P.tolist():
        a, b = min(s, d), max(s, d)
        vs, es = R.path(a, b, True)
        gv, ge = t.get_path(s, d)
        assert list(gv) == vs and list(ge) == es, (s, d)
        if a not in lat:
            lat[a] = R.row(a, True)
        assert t.get_latency(a, b) == lat[a][0][b]
        line = t.format_path(s, d)
        assert line == hg._ref_line(g, ids, a, b, vs, es, t.get_latency(a, b), t.get_reliability(a, b))
        assert "[%f," % g.latency[es[0]] in line
    for (a, b), k in zip(P.tolist(), rng.integers(1, 1000, size=len(P)).tolist()):
        t.add_path_packets(a, b, k)
    ps, pt, pw = [], [], []
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            c = t.packet_count(a, b)
            if c:
                ps.append(a); pt.append(b); pw.append(c)
    assert len(ps) > 100
    E = eg.ref(name)
    want = E.pairs(ps, pt, pw, dispatch=True)
    got = t.ecmp_link_loads()
    rtol = E.tol(sorted(set(ps)), dispatch=True)
    assert eg.same(got[0], want[0], rtol) and eg.same(got[1], want[1], rtol) and got[2] == want[2] == 0
    one = t.link_loads()
    el, trn, un = R.loads(ps, pt, pw, True)
    assert np.array_equal(one[0], el) and np.array_equal(one[1], trn)
    assert not np.array_equal(got[0], one[0].astype(np.float64))      # tied pairs are split
    t.close()
