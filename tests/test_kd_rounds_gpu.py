"""GPU parity of KD's bucket rounds and of phase A' on small graphs (sssp_delta.hpp).

A bucket round no longer scans wmin[] for its minimum: every writer of wmin (the init, the
gather, and the two stay-pending paths of kd_relax_list: a far improvement and a push that
found the queue full) folds the value it leaves into the next round's slot.  Phase A'
evaluates each tie event once and min-combines the events that beat a vertex's present record
in an LDS table, in chunks (SHD_ROUTE_EVCHUNK caps a chunk, so that small graphs take several
and a vertex meets its events in different ones).  Everything is bit-exact against the oracle
(engine tie rule); a wrong minimum shows as a row that ends early (distances left at infinity)
or as a bucket opened in the wrong order (wrong parents, so wrong reliabilities).

The oracle tables are computed once per graph and shared, read-only, with
tests/test_kd_split_gpu.py.
"""
import functools

import numpy as np
import pytest

from shadow_amd.graph import Graph

from tests.test_kd_gpu import _graph
from tests.test_kd_split_gpu import _case, _check

pytestmark = pytest.mark.gpu

_KNOBS = ("SHD_ROUTE_SEED", "SHD_ROUTE_EVCAP", "SHD_ROUTE_EVCHUNK", "SHD_ROUTE_SEEDS", "SHD_ROUTE_DELTA",
          "SHD_ROUTE_QCAP", "SHD_ROUTE_KDWALK", "SHD_ROUTE_KDPACK", "SHD_ROUTE_PLAN_DELTA", "SHD_ROUTE_SEEDDROP",
          "SHD_ROUTE_KDBLOCK", "SHD_ROUTE_LANDMARKS", "SHD_ROUTE_SEED_ROOTS", "SHD_ROUTE_SEED2HOP")


@pytest.fixture
def kd(monkeypatch, oracle_mod):
    """Forced KD with a grid of 7: each workgroup runs many rows back to back, so a row's
    leftover minimum (or table entry) would show in the next."""
    monkeypatch.setenv("SHD_ROUTE_KERNEL", "kd")
    monkeypatch.setenv("SHD_ROUTE_KDGRID", "7")
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _set(kd, **knobs):
    for k, v in knobs.items():
        if v is not None:
            kd.setenv("SHD_ROUTE_" + k, str(v))


def _engine(g, block):
    from shadow_amd import route
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 4 and eng.info["block"] == block, eng.info
    return eng


@functools.lru_cache(maxsize=None)
def _c2():
    """c2 (about 2,000 vertices): every third vertex as a source, as tests/test_seed_gpu.py"""
    from oracle import oracle
    g = _graph("c2")
    T = g.targets()
    S = np.ascontiguousarray(T[::3])
    olat, orel, _, _ = oracle.OracleGraph(g).source_rows(S, T, oracle.TIE_MINKEY)
    for a in (olat, orel):
        a.setflags(write=False)
    return g, S, T, olat, orel


# bucket widths: the default, 1 (a round per distinct distance: many rounds, every improvement
# is a far one), 7 (several arcs per bucket) and one bucket for the whole row (a single round,
# whose next minimum must come out empty); queue capacities: the default, 64 and 8 (the
# selection takes 64 at least), at which pushes find the queue full and gathers run past it
WIDTHS = [(None, None), (1, None), (7, None), (100000, None), (None, 64), (None, 8), (7, 64), (7, 8), (1, 8),
          (100000, 64), (100000, 8), (1, 64)]


@pytest.mark.parametrize("seed", [None, "0"])
@pytest.mark.parametrize("delta,qcap", WIDTHS)
@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("name", ["ba400", "ties", "chain", "dir", "stars"])
def test_rounds_bitexact(kd, name, block, delta, qcap, seed):
    """Every vertex a source, plain rows (seed "0") and the seeded plan.  `dir` is directed: no
    fused parents, slices with empty rows, and plans that fall back to plain rows."""
    _set(kd, KDBLOCK=block, DELTA=delta, QCAP=qcap, SEED=seed)
    g, _, olat, orel = _case(name)
    eng = _engine(g, block)
    T = g.targets()
    lat, rel, mn = eng.rows(T, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, T, T)


@pytest.mark.parametrize("seed", [None, "0"])
@pytest.mark.parametrize("delta,qcap", [(None, None), (1, 8), (7, 64), (100000, 8)])
@pytest.mark.parametrize("block", [1024, 256])
def test_rounds_bitexact_c2(kd, block, delta, qcap, seed):
    """The same on c2: rows of some thirty bitmask words, queues that really fill."""
    _set(kd, KDBLOCK=block, DELTA=delta, QCAP=qcap, SEED=seed)
    g, S, T, olat, orel = _c2()
    eng = _engine(g, block)
    lat, rel, mn = eng.rows(S, T, dispatch=False)
    assert np.array_equal(lat, olat)
    assert np.array_equal(rel, orel)
    assert np.array_equal(mn, olat.min(axis=1))


def test_no_context_holds_an_unreachable_component(kd):
    """A row whose loop ends on an empty pending set while distances are still 0xFFFF needs a
    vertex the source cannot reach.  shd_route_create takes strongly connected graphs only
    (topology.c:738-806), so no context can show one: the refusal is what there is to check.
    (The end of the loop on an empty pending set is every row's last round.)"""
    from shadow_amd import route
    a = _graph("ba400")
    m = a.n
    # a second component: a triangle of three more vertices, with self-loops as every vertex has
    src = np.concatenate([a.src, [m, m + 1, m + 2, m, m + 1, m + 2]]).astype(np.int32)
    dst = np.concatenate([a.dst, [m + 1, m + 2, m, m, m + 1, m + 2]]).astype(np.int32)
    lat = np.concatenate([a.latency, [3.0, 4.0, 5.0, 1.0, 1.0, 1.0]])
    loss = np.concatenate([a.packetloss, np.zeros(6)])
    g = Graph(n=m + 3, src=src, dst=dst, latency=lat, packetloss=loss, vertex_packetloss=np.zeros(m + 3),
              directed=a.directed, name="ba400_plus_triangle")
    with pytest.raises(route.RouteError):
        route.RouteEngine(g)


def test_no_context_holds_an_absorbed_latency(kd):
    """Every kernel takes fl(d[u] + w) > d[u] for granted (include/shd_route.h, "Absorbed
    latencies"): shd_route_create refuses min_w <= (n - 1) max_w 2^-52 over the edges that are no
    self-loops with SHD_ROUTE_EUNSUPPORTED, at the threshold itself too, and takes the graphs just
    on the other side of it, a tiny self-loop latency among them.  Contexts are made and closed;
    nothing is launched on any of these graphs."""
    from shadow_amd import route
    from tests import frac_graphs as fg
    from tests.test_frac_graphs import chain
    a = _graph("ba400")
    nl = a.src != a.dst
    e = int(np.flatnonzero(nl)[7])

    def with_latency(w, at=e):
        lat = a.latency.copy()
        lat[at] = w
        return Graph(n=a.n, src=a.src, dst=a.dst, latency=lat, packetloss=a.packetloss,
                     vertex_packetloss=a.vertex_packetloss, directed=a.directed, name="ba400_tiny")

    thr = (a.n - 1) * (float(a.latency[nl].max()) * 2.0 ** -52)
    up = float(np.nextafter(thr, 1.0))
    for g in (with_latency(thr), with_latency(thr / 3), with_latency(5e-324), chain(1e-17), chain(3 * 2.0 ** -52)):
        assert fg.absorbs(g)
        with pytest.raises(route.RouteError) as ei:
            route.RouteEngine(g)
        assert ei.value.code == route.EUNSUPPORTED
    loop = int(np.flatnonzero(~nl)[0])
    for g in (with_latency(up), with_latency(1e-300, at=loop), chain(float(np.nextafter(3 * 2.0 ** -52, 1.0))), chain(1e-3)):
        assert not fg.absorbs(g)
        eng = route.RouteEngine(g)
        assert eng.info["n_vertices"] == g.n
        eng.close()


@pytest.mark.parametrize("seeds", ["1", "2", "3"])
@pytest.mark.parametrize("evcap", [None, "2"])
@pytest.mark.parametrize("evchunk", [None, "1", "8"])
@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("name", ["ties", "ba400"])
def test_tie_events_bitexact(kd, name, block, evchunk, evcap, seeds):
    """Seeded plans over every vertex: chunks of 1 and 8 events (a vertex's events in different
    chunks, each chunk's base the record the last one stored), lists capped at 2 events (rows
    with more rerun unseeded), one to three seeds per row."""
    _set(kd, KDBLOCK=block, EVCHUNK=evchunk, EVCAP=evcap, SEEDS=seeds)
    g, _, olat, orel = _case(name)
    eng = _engine(g, block)
    T = g.targets()
    plan = eng.plan(T)
    assert plan.info["seeded"] == 1 and plan.info["stored_rows"] > 0
    lat, rel, mn = eng.rows(T, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, T, T)


@pytest.mark.parametrize("drop", ["2", "4", "6"])
@pytest.mark.parametrize("evchunk", [None, "1", "8"])
@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("name", ["ties", "ba400"])
def test_tie_events_dropped_seeds(kd, name, block, evchunk, drop):
    """Three seeds planned, the second, the third or both dropped at the row's start: D0 then
    comes from the seeds that are left, and A' reads the compacted job."""
    _set(kd, KDBLOCK=block, EVCHUNK=evchunk, SEEDS="3", SEEDDROP=drop)
    g, _, olat, orel = _case(name)
    eng = _engine(g, block)
    T = g.targets()
    lat, rel, mn = eng.rows(T, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, T, T)


# ---- four candidates in one table slot ----------------------------------------------------------

S_, U_, Q_, T_, A1, A2, A3 = range(7)
PAD = 120  # a tail of heavy arcs behind u, so that the graph is worth a seeded plan


def _meet(wa3):
    """s has four neighbours u, a1, a2, a3, and t lies 21 behind each of them:
        s -1- u -10- q -10- t,   s -16- a1 -5- t,   s -14- a2 -7- t,   s -(21 - wa3)- a3 -wa3- t.
    All four paths are shortest, so whichever neighbour x seeds the row of s, t keeps D0 with the
    seed-derived parent on x's path, and the other three branches improve on D0 (their own path
    from s is shorter than any path through x) and report their arc into t as a tie event: three
    valid events with distinct weights and the seed's record meet in t's slot.  The tie rule
    takes the largest weight: a3 for wa3 = 12, q (w = 10) for wa3 = 9.  Every arc has its own
    loss, far apart, so the parent shows in rel(s, t)."""
    e = [(S_, U_, 1, .01), (U_, Q_, 10, .02), (Q_, T_, 10, .03), (S_, A1, 16, .04), (A1, T_, 5, .05),
         (S_, A2, 14, .06), (A2, T_, 7, .07), (S_, A3, 21 - wa3, .08), (A3, T_, wa3, .09)]
    prev = U_
    for k in range(PAD):
        e.append((prev, 7 + k, 200, .001 * (1 + k % 5)))
        prev = 7 + k
    n = 7 + PAD
    src = np.array([x[0] for x in e] + list(range(n)), np.int32)
    dst = np.array([x[1] for x in e] + list(range(n)), np.int32)
    lat = np.array([x[2] for x in e] + [1.0] * n, np.float64)
    loss = np.array([x[3] for x in e] + [0.0] * n, np.float64)
    g = Graph(n=n, src=src, dst=dst, latency=lat, packetloss=loss, vertex_packetloss=np.zeros(n),
              name=f"meet{wa3}")
    return g, {(a, b): (w, l) for a, b, w, l in e}


@pytest.mark.parametrize("evchunk", [None, "1"])
@pytest.mark.parametrize("block", [1024, 256])
@pytest.mark.parametrize("wa3,via", [(12, A3), (9, Q_)])
def test_four_candidates_meet_in_one_slot(kd, oracle_mod, wa3, via, block, evchunk):
    # one neighbour seed per row: no landmark rows (s would seed from its own), one root (the most
    # central row, in the middle of the tail), no two-hop seeds
    _set(kd, KDBLOCK=block, EVCHUNK=evchunk, SEEDS="1", LANDMARKS="0", SEED_ROOTS="1", SEED2HOP="0")
    g, arcs = _meet(wa3)
    allv = np.arange(g.n, dtype=np.int32)
    olat, orel, _, _ = oracle_mod.OracleGraph(g).source_rows(allv, allv, oracle_mod.TIE_MINKEY)
    # the oracle's own parent of t from s is the one worked out by hand: the path's losses
    assert olat[S_, T_] == 21.0
    first = {A3: (S_, A3), Q_: (U_, Q_)}[via]
    want = (1 - arcs[first][1]) * (1 - arcs[(via, T_)][1]) * ((1 - arcs[(S_, U_)][1]) if via == Q_ else 1.0)
    others = [(1 - arcs[(S_, a)][1]) * (1 - arcs[(a, T_)][1]) for a in (A1, A2, A3) if a != via]
    assert abs(orel[S_, T_] - want) < 1e-12 and all(abs(orel[S_, T_] - o) > 1e-3 for o in others)
    eng = _engine(g, block)
    plan = eng.plan(allv)
    assert plan.info["seeded"] == 1
    jobs = plan.jobs()
    js = jobs[jobs["s"] == S_]
    # the row of s starts from one seed that lies on a shortest s -> t path, so t keeps D0
    assert len(js) == 1 and js["nseed"][0] == 1, js
    useed = int(js["u"][0][0])
    assert useed in (U_, A1, A2, A3) and olat[S_, useed] + olat[useed, T_] == 21.0, js
    lat, rel, mn = eng.rows(allv, allv, dispatch=False)
    _check(lat, rel, mn, olat, orel, allv, allv)
