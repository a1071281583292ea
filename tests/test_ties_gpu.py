"""GPU: the tie envelope -- shd_route_ties*, RouteEngine.ties / ties_async and the front end's
tie statistics -- against tests/ties_ref.py (a plain-Python programme over multi_ref.Ref's
Dijkstra, held to a brute-force enumeration and to the oracle by tests/test_ties.py).

Unless a test says otherwise all three outputs are compared bit for bit (NaN = NaN): the
saturating u64 count, the smallest and the largest reliability of any shortest path."""
import functools
import json
import math
import os

import numpy as np
import pytest

from shadow_amd.graph import Graph, config
from tests import frac_graphs as fgr
from tests import shape_graphs as sg
from tests import stream_order as so
from tests import test_hops_gpu as hg
from tests import ties_ref as tr
from tests.test_contract_gpu import Padded
from tests.test_range_gpu import select

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


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
    for k in ("SHD_ROUTE_TIES_LDS", "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _multi_equal():
    """ba60 plus 10 parallel edges, picked as test_hops_gpu._multi picks them, each with the
    latency of the edge it doubles and a loss of its own: tight together, two paths."""
    g = hg._graph("ba60")[0]
    rng = np.random.default_rng(60)
    nl = np.flatnonzero(g.src != g.dst)
    pick = rng.choice(nl, size=10, replace=False)
    return Graph(n=g.n, src=np.concatenate([g.src, g.dst[pick]]).astype(np.int32),
                 dst=np.concatenate([g.dst, g.src[pick]]).astype(np.int32),
                 latency=np.concatenate([g.latency, g.latency[pick]]),
                 packetloss=np.concatenate([g.packetloss, g.packetloss[pick] + 1.0 / 64]),
                 vertex_packetloss=g.vertex_packetloss, name="ba60_multi_equal")


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "ba60_multi_equal":
        return _multi_equal()
    if name.startswith("grid34x"):
        return sg.grid(34, int(name[7:]))
    if name.startswith("sized"):
        return sg.sized(int(name[5:]))
    if name in sg.SUITE:
        return sg.get(name)
    if name in fgr.SUITE:
        return fgr.get(name)
    return hg._graph(name)[0]


@functools.lru_cache(maxsize=None)
def ref(name):
    return tr.TiesRef(graph(name))


def run(route, eng, S, T, dispatch):
    try:
        return eng.ties(S, T, dispatch=dispatch), route.OK
    except route.RouteError as err:
        assert err.code in (route.ENOEDGE, route.EUNREACH)
        return err.partial, err.code


def check(route, name, S, dispatch=False, T=None, eng=None):
    """eng.ties(S, T) equals the reference, the code is one the failed entries give."""
    g = graph(name)
    T = np.arange(g.n, dtype=np.int32) if T is None else np.asarray(T, np.int32)
    S = np.asarray(S, np.int32)
    want = ref(name).rows(S, T, dispatch)
    eng = eng or route.RouteEngine(g)
    got, code = run(route, eng, S, T, dispatch)
    assert (code in want[3]) if want[3] else code == route.OK, (code, want[3])
    assert got[0].dtype == np.uint64 and got[0].shape == (len(S), len(T))
    assert np.array_equal(got[0], want[0])
    assert eq(got[1], want[1]) and eq(got[2], want[2])
    return got, want


# ---- small goldens ------------------------------------------------------------------------------

@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", hg.SMALL)
def test_small_goldens(route, name, dispatch):
    """All attached sources x all vertices: prefer-direct (ba80_prefer), complete (k24),
    directed, fractional and vertex loss among them."""
    g, A = hg._graph(name)
    got, want = check(route, name, A, dispatch)
    off = np.arange(g.n)[None, :] != np.asarray(A)[:, None]
    if name == "k24" and dispatch:
        assert np.all(got[0] == 1) and eq(got[1], got[2])
    if name == "ba80_prefer":
        R = ref(name).ref
        adj = np.array([[R.is_direct(int(s), t, True) for t in range(g.n)] for s in A])
        assert adj.any() and (not dispatch or np.all(got[0][adj & off] == 1))
    if name == "ba64_ties":
        assert np.count_nonzero(got[0] > 1) >= 1000 and np.count_nonzero(got[1] < got[2]) >= 100


# ---- the shape suite ------------------------------------------------------------------------------

def _spread(n, k=6):
    return np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, k).astype(int)])).astype(np.int32)


@pytest.mark.parametrize("name", ["grid", "lollipop", "star1100", "biclique1030", "dir_grid"])
def test_shapes(route, name):
    """grid: 63 rounds and counts near 2^60; lollipop: 302 rounds; star1100: a vertex with more
    than 1,024 out-arcs released by its wave; biclique1030: in-lists past 1,024 and heavy ties."""
    g = graph(name)
    S = _spread(g.n)
    if name == "biclique1030":
        S = np.array([0, 16, 17, 500, g.n - 1], np.int32)
    got, want = check(route, name, S)
    nl = g.src != g.dst
    deg = np.bincount(np.concatenate([g.src[nl], g.dst[nl]]), minlength=g.n)
    if name == "grid":
        assert int(got[0][0].max()) == math.comb(63, 31) > 2 ** 59
    if name == "star1100":
        assert deg.max() > 1024
    if name == "biclique1030":
        assert np.count_nonzero(deg > 1024) == 17 and np.count_nonzero(got[0] > 1) > got[0].size // 2
    if name == "lollipop":
        assert g.n == 340 and np.all(got[0][0][40:] == got[0][0][39])   # one way down the tail


@pytest.mark.parametrize("cols", [35, 36])
def test_saturation(route, cols):
    """34 x 35: C(67, 33) paths corner to corner, below 2^64; 34 x 36: the count saturates, and
    what builds on a saturated count stays saturated.  From both far corners."""
    name = f"grid34x{cols}"
    g = graph(name)
    got, _ = check(route, name, [0, g.n - 1])
    top = int(got[0][0][g.n - 1])
    assert top == int(got[0][1][0])
    assert top == (math.comb(67, 33) if cols == 35 else 2 ** 64 - 1)
    assert (int(got[0].max()) == 2 ** 64 - 1) == (cols == 36)


@pytest.mark.parametrize("loops", sg.TINY_LOOPS)
@pytest.mark.parametrize("n", sg.TINY_N)
def test_tiny(route, n, loops):
    """Paths of 1 to 9 vertices: SHD_ROUTE_ENOEDGE entries with the rest of the row written."""
    name = f"tiny{n}_{loops}"
    g = graph(name)
    got, want = check(route, name, np.arange(n))
    noloop = ~np.isin(np.arange(n), g.src[g.src == g.dst])
    assert np.array_equal(np.diag(got[0]) == 0, noloop) and np.all(got[0][~np.eye(n, dtype=bool)] == 1)


def test_multigraph(route):
    """Parallel tight edges are distinct paths: ba60 with 10 edges doubled at equal latency."""
    name = "ba60_multi_equal"
    g = graph(name)
    eng = route.RouteEngine(g)
    assert eng.info["multigraph"] == 1
    got, _ = check(route, name, np.arange(g.n), eng=eng)
    base = ref("ba60").rows(np.arange(g.n), np.arange(g.n))
    assert np.all(got[0] >= base[0]) and np.count_nonzero(got[0] > base[0]) > 100
    assert np.count_nonzero((got[1] < got[2]) & (base[0] == 1)) > 50   # sensitive through the doubled edge alone
    # test_hops_gpu's own multigraph: the doubled edges differ in latency, so never tie with their twin
    g2, A2 = hg._graph("ba60_multi")
    check(route, "ba60_multi", A2)


# ---- both state forms -----------------------------------------------------------------------------

@pytest.mark.parametrize("over", [0, 1])
def test_lds_limit(route, over):
    """sized(n) at the largest n whose state layout fits the LDS and at n + 1 (the HBM form)."""
    n = tr.lds_max_n() + over
    assert tr.fits_lds(n) == (over == 0)
    check(route, f"sized{n}", [0, n - 1, n // 2, 17, n // 3])


@pytest.mark.parametrize("name", ["grid", "ba64_ties"])
def test_hbm_form(route, monkeypatch, name):
    monkeypatch.setenv("SHD_ROUTE_TIES_LDS", "0")
    g = graph(name)
    check(route, name, _spread(g.n, 8) if name == "grid" else hg._graph(name)[1])


def test_hbm_slots_reused(route, monkeypatch):
    """64 sources over the 16 workgroup slots a small scratch budget leaves: a workgroup that
    takes a second source finds nothing of the first."""
    g = graph("ba64_ties")
    stride = tr.layout_total(g.n, 2)
    budget = 4 * 16 * stride
    assert budget // (12 * g.n) >= g.n >= 40                  # one chunk of all sources
    monkeypatch.setenv("SHD_ROUTE_TIES_LDS", "0")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(budget))
    eng = route.RouteEngine(g)
    S = np.arange(g.n, dtype=np.int32)
    check(route, "ba64_ties", S, eng=eng)
    check(route, "ba64_ties", S[::-1].copy(), eng=eng)


@pytest.mark.parametrize("lds", [None, "0"])
def test_three_chunks(route, monkeypatch, lds):
    """SHD_ROUTE_HOPS_SCRATCH of four sources (12 n bytes each): 11 sources take three chunks."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 12 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_TIES_LDS", lds)
    check(route, "ba64_ties", A[:11])


def test_beyond_u16(route):
    """66,000 vertices: u32 frontier entries, the state in HBM slices."""
    g, A = hg._graph("ring66k")
    assert g.n > 65535 and not tr.fits_lds(g.n)
    got, _ = check(route, "ring66k", A)
    assert int(got[0].max()) > 1 and got[0][1][g.n - 1] == 0   # 65999's own entry: no self-loop


# ---- against the rows call ------------------------------------------------------------------------

@pytest.mark.parametrize("sel", ["auto", "kd", "kf", "f64"])
@pytest.mark.parametrize("name", ["ba64_ties", "grid_vloss"])
def test_rows_inside_the_envelope(route, monkeypatch, name, sel):
    """The rows' rel with the same flags lies in [lo, hi] and equals both where count == 1: to
    the bit where the target has no lossy vertex factor, within 1e-12 with one."""
    select(monkeypatch, sel)
    g = graph(name)
    S = hg._graph(name)[1][:24] if name == "ba64_ties" else _spread(g.n, 8)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    print(name, sel, "kernel", eng.info["kernel"])
    (cnt, lo, hi), code = run(route, eng, S, T, False)
    try:
        rel = eng.rows(S, T, dispatch=False)[1]
    except route.RouteError as err:
        rel = err.partial[1]
    assert np.array_equal(np.isnan(rel), cnt == 0) and np.count_nonzero(cnt > 1) > 100
    vl = g.vertex_packetloss
    lossy = np.zeros(g.n, bool) if vl is None else np.nan_to_num(vl) != 0.0
    assert lossy.any() == (name == "grid_vloss")
    ok = cnt > 0
    self_ = T[None, :] == np.asarray(S)[:, None]
    exact = ok & (~lossy[None, :] | self_)
    loose = ok & lossy[None, :] & ~self_
    one = cnt == 1
    assert np.all((lo[exact] <= rel[exact]) & (rel[exact] <= hi[exact]))
    assert np.array_equal(rel[exact & one], lo[exact & one]) and np.array_equal(rel[exact & one], hi[exact & one])
    assert np.all((rel[loose] >= lo[loose] * (1 - 1e-12)) & (rel[loose] <= hi[loose] * (1 + 1e-12)))
    assert np.all(np.abs(rel[loose & one] - lo[loose & one]) <= 1e-12 * lo[loose & one])
    assert np.array_equal(lo[one], hi[one])


# ---- the independent pin on C2 --------------------------------------------------------------------

def test_c2_pin(route, oracle_mod):
    """internet_like C2, all 2,000 sources x all vertices: the number of off-diagonal entries
    with one shortest path is the 3,877,454 that networkx confirmed for the golden digests, and
    the 447 entries on which the oracle's min-key and igraph rules differ in reliability all
    have rel_lo < rel_hi.  Both figures come from rows_digests.json and the oracle."""
    stats = json.load(open(os.path.join(GOLD, "rows_digests.json")))["c2"]["stats"]
    assert stats["nx_unique_rel_pairs_equal"] == 3877454 == stats["unique"] - 2000 and stats["rel_diff_on_ties"] == 447
    g = config("c2")
    T = g.targets()
    assert len(T) == g.n == 2000 and np.array_equal(T, np.arange(g.n))
    eng = route.RouteEngine(g)
    (cnt, lo, hi), _ = run(route, eng, T, T, False)
    off = ~np.eye(g.n, dtype=bool)
    assert np.count_nonzero(cnt[off] == 1) == stats["nx_unique_rel_pairs_equal"]
    og = oracle_mod.OracleGraph(g)
    rel_m = og.source_rows(T, T, oracle_mod.TIE_MINKEY)[1]
    rel_i = og.source_rows(T, T, oracle_mod.TIE_IGRAPH)[1]
    diff = rel_m != rel_i
    assert np.count_nonzero(diff) == stats["rel_diff_on_ties"] and not diff[~off].any()
    assert np.all(lo[diff] < hi[diff]) and np.all(cnt[diff] > 1)
    for rel in (rel_m, rel_i):
        assert np.all((lo[off] <= rel[off]) & (rel[off] <= hi[off]))


# ---- the contract -----------------------------------------------------------------------------------

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _i64(p):
    """The body of a Padded output as the int64 tensor the counts go to."""
    return p.big[p.off: p.off + p.ns * p.ld].view(p.ns, p.ld)


def test_contract(route):
    """NULL outputs one at a time, a row stride above nt (the padding and the guards keep
    their canary), ns == 0, and an out-of-range vertex: SHD_ROUTE_EINVAL."""
    g, A = hg._graph("ba64_ties")
    S = A[:7].astype(np.int32)
    T = np.concatenate([np.arange(0, g.n, 3), [5, 5, int(S[2])]]).astype(np.int32)
    nt, ld = len(T), len(T) + 3
    want = ref("ba64_ties").rows(S, T, False)
    eng = route.RouteEngine(g)
    ds, dt = _dev(S), _dev(T)

    def sync():
        try:
            eng.sync()
            return route.OK
        except route.RouteError as err:
            return err.code

    for keep in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        c, l, h = Padded(len(S), ld), Padded(len(S), ld), Padded(len(S), ld)
        eng.ties_async(ds, dt, _i64(c) if keep[0] else None, l.t if keep[1] else None, h.t if keep[2] else None, ld=ld)
        code = sync()
        assert (code in want[3]) if want[3] else code == route.OK
        for p, k, w in zip((c, l, h), keep, want[:3]):
            if not k:
                assert p.untouched()
            elif w.dtype == np.uint64:
                assert np.array_equal(p.bits(nt).view(np.uint64), w)
            else:
                assert eq(p.bits(nt).view(np.float64), w)
    # ns == 0: nothing enqueued, nothing written
    c = Padded(1, ld)
    eng.ties_async(ds[:0], dt, _i64(c), None, None, ld=ld)
    assert sync() == route.OK and c.untouched()
    out = eng.ties([], T)
    assert out[0].shape == (0, nt)
    # ld < nt is refused at once; a vertex out of range comes back from the device
    with pytest.raises(route.RouteError) as ei:
        eng.ties_async(ds, dt, _i64(c), None, None, ld=nt - 1)
    assert ei.value.code == route.EINVAL
    for bad in (-1, g.n):
        with pytest.raises(route.RouteError) as ei:
            eng.ties(S[:2], [0, bad, 3], dispatch=False)
        assert ei.value.code == route.EINVAL
        with pytest.raises(route.RouteError) as ei:
            eng.ties([int(S[0]), bad], [0, 3], dispatch=False)
        assert ei.value.code == route.EINVAL
    check(route, "ba64_ties", S, eng=eng)                     # and the context goes on working


# ---- stream order -----------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", [None, "0"])
def test_gated_ties(route, monkeypatch, lds):
    """ties_async behind the timed gate of tests/stream_order.py, in three chunks, in each
    state form: decoy inputs until the gate opens, two calls with the canary in between, and
    the call returns while the gate is shut."""
    g, A = hg._graph("ba64_ties")
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 12 * g.n))
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_TIES_LDS", lds)
    S = A[:11].astype(np.int32)
    T = np.arange(g.n, dtype=np.int32)
    ns, nt = len(S), len(T)
    want = ref("ba64_ties").rows(S, T, False)
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    rows = np.roll(np.arange(ns), -1)
    for x in want[:3]:   # an early reader of either list, or of both, gets every row wrong
        assert so.rows_differ(x[rows], x) and so.rows_differ(x[:, Td], x) and so.rows_differ(x[rows][:, Td], x)
    eng = route.RouteEngine(g)
    i_s, i_t = so.In(S, Sd), so.In(T, Td)
    c, l, h = so.Out(ns, nt + 1, i64=True), so.Out(ns, nt + 1), so.Out(ns, nt + 1)
    code = so.gated(route, eng, [i_s, i_t], [c, l, h],
                    lambda sh: eng.ties_async(i_s.t, i_t.t, c.t, l.t, h.t, stream=sh, dispatch=False, ld=nt + 1),
                    f"ties_async TIES_LDS={lds}")
    assert (code in want[3]) if want[3] else code == route.OK
    assert np.array_equal(c.snap_bits(nt).view(np.uint64), want[0])
    assert eq(l.f64(nt), want[1]) and eq(h.f64(nt), want[2])


# ---- the front end ------------------------------------------------------------------------------------

def _front_ref(name, A):
    """(stats, lines) of the stored off-diagonal pairs A[i] -> A[j], i < j, under dispatch."""
    g = graph(name)
    cnt, lo, hi, _ = ref(name).rows(A, A, True)
    st = dict(pairs=0, tied=0, sensitive=0, saturated=0, max_spread=0.0, worst_src=-1, worst_dst=-1, worst_count=0,
              worst_lo=0.0, worst_hi=0.0)
    sep = "-->" if g.directed else "<-->"
    lines = []
    for i in range(len(A)):
        for j in range(i + 1, len(A)):
            c, l, h = int(cnt[i, j]), float(lo[i, j]), float(hi[i, j])
            if c == 0:
                continue
            st["pairs"] += 1
            st["tied"] += c > 1
            st["saturated"] += c == 2 ** 64 - 1
            if l == h:
                continue
            st["sensitive"] += 1
            spread = (h - l) / h
            if spread > st["max_spread"]:
                st.update(max_spread=spread, worst_src=int(A[i]), worst_dst=int(A[j]), worst_count=c, worst_lo=l, worst_hi=h)
            lines.append("tie %d%s%d (%d%s%d) has %d shortest paths, reliability %.17g to %.17g, spread %.17g"
                         % (A[i], sep, A[j], A[i], sep, A[j], c, l, h, spread))
    lines.append("ties: %d pairs, %d tied, %d sensitive, %d saturated, max spread %.17g at (%d%s%d) with %d paths"
                 % (st["pairs"], st["tied"], st["sensitive"], st["saturated"], st["max_spread"], st["worst_src"], sep,
                    st["worst_dst"], st["worst_count"]))
    return st, lines


@pytest.mark.parametrize("name", ["ba64_ties", "ba100_attached"])
def test_front_end_ties(topo, tmp_path, name):
    g, A = hg._graph(name)
    A = np.sort(A)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    sample = [int(x) for x in A[:: max(1, len(A) // 9)]]
    snap = lambda: (t.table(sample), [t.packet_count(a, b) for a in sample for b in sample], t.min_path_latency())
    t.increment_path_packet_counter(int(A[0]), int(A[3]))
    was = snap()
    want, lines = _front_ref(name, A)
    got = t.tie_stats()
    assert got == want
    assert want["pairs"] == len(A) * (len(A) - 1) // 2 and want["sensitive"] > 0 and want["tied"] >= want["sensitive"]
    out = tmp_path / "ties.txt"
    t.dump_ties(str(out))
    assert out.read_text().splitlines() == lines and len(lines) == want["sensitive"] + 1
    now = snap()
    assert eq(was[0][0], now[0][0]) and eq(was[0][1], now[0][1]) and was[1:] == now[1:]   # nothing cached, nothing moved
    t.close()


def test_front_end_complete(topo, tmp_path):
    """The bundled complete topology: every pair is direct, one path each, nothing sensitive."""
    t = topo.Topology.new(os.path.join(GOLD, "topology.graphml.xml.xz"))
    n = t.vertex_count()
    t.attach_all(range(n))
    st = t.tie_stats()
    assert st == dict(pairs=n * (n - 1) // 2, tied=0, sensitive=0, saturated=0, max_spread=0.0, worst_src=-1,
                      worst_dst=-1, worst_count=0, worst_lo=0.0, worst_hi=0.0)
    out = tmp_path / "ties.txt"
    t.dump_ties(str(out))
    assert out.read_text().splitlines() == [
        "ties: %d pairs, 0 tied, 0 sensitive, 0 saturated, max spread 0 at (-1<-->-1) with 0 paths" % st["pairs"]]
    assert st["pairs"] == 183 * 182 // 2
    t.close()
