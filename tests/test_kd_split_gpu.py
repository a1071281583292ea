"""GPU parity of KD's 1024-thread rows on small graphs (sssp_delta.hpp, the split region).

After phase A' a 1024-thread row splits its waves: the first KD_BWAVES run phase B (parent
fix-ups, wave-local lists, long in-row tails eight vertices at a time) while the others
store the distance row of a kept row and write the latency row; both meet at one barrier,
after which the row's ready flag is raised.  Graphs of C4's size are the only ones that
take 1024-thread rows by default, so every test here forces them (SHD_ROUTE_KDBLOCK=1024)
on graphs of a few hundred vertices, with a small grid so that each workgroup runs many
rows back to back.  Everything is bit-exact against the oracle (engine tie rule).
"""
import functools

import numpy as np
import pytest

from shadow_amd.graph import Graph

from tests.test_kd_gpu import _graph

pytestmark = pytest.mark.gpu

# in-row sizes around every block boundary of the fix-up: KD_TAIL = 4 speculative arcs, then
# blocks of 8 arcs, two per trip (12, 20, 36), and of 64 (68: one wave per vertex, the earlier form)
STAR_DEGS = [4, 5, 12, 13, 16, 17, 20, 21, 36, 37, 64, 65, 68, 69, 200]


def _stars(directed):
    """Hubs with in-rows of exactly STAR_DEGS arcs: two ring arcs (w = 9, first in the
    (-w, u, eid) order) and deg - 2 spokes of equal weight 5, so the spokes sort by leaf id.
    From a hub's last leaf the only tight in-arc of the hub is the row's last arc.  Vertex z
    hangs off two leaves of the 200-arc hub (positions 42 and 152 of its row) with equal
    weights: from z the hub has two tight arcs in different blocks, and the lower must win.
    Every arc has its own loss, so a wrong parent shows in the reliabilities too."""
    m = len(STAR_DEGS)
    e, w = [], []
    for h in range(m):
        e.append((h, (h + 1) % m)); w.append(9)
    nxt = m
    last_leaf, leaves200 = [], None
    for h, d in enumerate(STAR_DEGS):
        ids = list(range(nxt, nxt + d - 2))
        nxt += d - 2
        for x in ids:
            e.append((x, h)); w.append(5)
        last_leaf.append(ids[-1])
        if d == 200:
            leaves200 = ids
    z = nxt
    n = z + 1
    for x in (leaves200[40], leaves200[150]):
        e.append((z, x)); w.append(3)
    e = np.array(e, np.int32)
    if directed:
        e = np.concatenate([e, e[:, ::-1]])
        w = w + w
    k = len(e)
    rng = np.random.default_rng(43)
    loops = np.arange(n, dtype=np.int32)
    lat = np.concatenate([np.array(w, np.float64), rng.integers(1, 5, size=n).astype(np.float64)])
    loss = np.concatenate([rng.integers(1, 200, size=k) * 1e-4, np.zeros(n)])
    g = Graph(n=n, src=np.concatenate([e[:, 0], loops]).astype(np.int32),
              dst=np.concatenate([e[:, 1], loops]).astype(np.int32), latency=lat, packetloss=loss,
              vertex_packetloss=np.zeros(n), directed=directed, name="stars_dir" if directed else "stars")
    return g, np.array(last_leaf + [z] + list(range(m)) + [m, leaves200[40]], np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """graph, sources of interest, and the oracle's full table (all vertices x all vertices),
    computed once per graph and shared, read-only, by every test"""
    from oracle import oracle
    if name in ("stars", "stars_dir"):
        g, S = _stars(name == "stars_dir")
    else:
        g, S = _graph(name), None
    allv = np.arange(g.n, dtype=np.int32)
    olat, orel, _, _ = oracle.OracleGraph(g).source_rows(allv, allv, oracle.TIE_MINKEY)
    for a in (olat, orel):
        a.setflags(write=False)
    return g, S, olat, orel


@pytest.fixture
def kd1024(monkeypatch, oracle_mod):
    monkeypatch.setenv("SHD_ROUTE_KERNEL", "kd")
    monkeypatch.setenv("SHD_ROUTE_KDBLOCK", "1024")
    monkeypatch.setenv("SHD_ROUTE_KDGRID", "7")
    for k in ("SHD_ROUTE_SEED", "SHD_ROUTE_EVCAP", "SHD_ROUTE_SEEDS", "SHD_ROUTE_DELTA", "SHD_ROUTE_QCAP",
              "SHD_ROUTE_KDWALK", "SHD_ROUTE_KDPACK", "SHD_ROUTE_PLAN_DELTA", "SHD_ROUTE_SEEDDROP"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _engine(g):
    from shadow_amd import route
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 4 and eng.info["block"] == 1024, eng.info
    return eng


def _check(lat, rel, mn, olat, orel, S, T):
    ol, orl = olat[np.ix_(S, T)], orel[np.ix_(S, T)]
    assert np.array_equal(lat, ol)
    assert np.array_equal(rel, orl)
    assert np.array_equal(mn, ol.min(axis=1))


@pytest.mark.parametrize("delta", [None, 1, 100000])
@pytest.mark.parametrize("name", ["ba400", "ties", "chain"])
def test_seeded_plans_widths(kd1024, name, delta):
    """Seeded plans over every vertex: the default width, D = 1 (every arc heavy: no
    fix-ups) and one bucket (every improved vertex goes through phase B)."""
    if delta is not None:
        kd1024.setenv("SHD_ROUTE_DELTA", str(delta))
    g, _, olat, orel = _case(name)
    eng = _engine(g)
    T = g.targets()
    plan = eng.plan(T)
    assert plan.info["seeded"] == 1 and plan.info["stored_rows"] > 0
    lat, rel, mn = eng.rows(T, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, T, T)


@pytest.mark.parametrize("seed", [None, "0"])
@pytest.mark.parametrize("delta", [None, 100000])
@pytest.mark.parametrize("name", ["stars", "stars_dir"])
def test_long_tail_boundaries(kd1024, name, delta, seed):
    """In-rows of exactly 4 .. 200 light arcs whose first tight arc is the last one, and
    one with two tight arcs in different blocks; directed: lrec holds whole in-rows.  seed
    "0": plain rows, so the hubs' parents come from phase B and not from a seed's records."""
    if delta is not None:
        kd1024.setenv("SHD_ROUTE_DELTA", str(delta))
    if seed is not None:
        kd1024.setenv("SHD_ROUTE_SEED", seed)
    g, S, olat, orel = _case(name)
    eng = _engine(g)
    T = g.targets()
    lat, rel, mn = eng.rows(S, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, S, T)
    # the oracle's parents are the ones the graph was built for: from a last leaf the hub is
    # one spoke away, from z the 200-arc hub is reached through the lower leaf's loss
    m = len(STAR_DEGS)
    assert all(olat[S[h], h] == 5.0 for h in range(m))
    h200 = STAR_DEGS.index(200)
    assert olat[S[m], h200] == 8.0


@pytest.mark.parametrize("omit", [False, True])
@pytest.mark.parametrize("shuffled", [True, False])
def test_target_lists(kd1024, shuffled, omit):
    """The general latency loop on the store waves: an unsorted target list with duplicates
    (nt = 1000 on ba400); and lists, unsorted and sorted, that omit the sources."""
    g, _, olat, orel = _case("ba400")
    eng = _engine(g)
    S = np.array([0, 199, 399, 17, 200, 201, 202, 5], np.int32)
    rng = np.random.default_rng(1000 + 2 * shuffled + omit)
    if shuffled:
        T = rng.integers(0, g.n, size=1000).astype(np.int32)
    else:
        T = np.arange(g.n, dtype=np.int32)
    if omit:
        T = T[~np.isin(T, S)]
    lat, rel, mn = eng.rows(S, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, S, T)


def test_helper_rows_two_ranks(kd1024):
    """A two-rank partitioned plan: helper rows (no output row) store their distances and
    raise their flags from the store waves, and write nothing."""
    import torch
    g, _, olat, orel = _case("ba400")
    eng = _engine(g)
    T = g.targets()
    dev = torch.device("cuda", 0)
    d_tgt = torch.from_numpy(np.ascontiguousarray(T, np.int32)).to(dev)
    seen = []
    for r in range(2):
        plan = eng.plan(T, 2, r)
        assert plan.info["seeded"] == 1 and plan.info["helpers"] > 0
        k = plan.info["rows"]
        # one spare row after the plan's own, which no row may touch
        d_lat = torch.full((k + 1, len(T)), -7.0, dtype=torch.float64, device=dev)
        d_rel = torch.full((k + 1, len(T)), -7.0, dtype=torch.float64, device=dev)
        d_min = torch.full((k + 1,), -7.0, dtype=torch.float64, device=dev)
        plan.rows_async(d_tgt, d_lat, d_rel, d_min, dispatch=False)
        eng.sync()
        pos = plan.positions
        _check(d_lat[:k].cpu().numpy(), d_rel[:k].cpu().numpy(), d_min[:k].cpu().numpy(), olat, orel, T[pos], T)
        assert bool((d_lat[k] == -7.0).all()) and bool((d_rel[k] == -7.0).all()) and float(d_min[k]) == -7.0
        seen.extend(pos.tolist())
    assert sorted(seen) == list(range(len(T)))


def test_kept_rows_read_by_other_workgroup(kd1024):
    """Two workgroups on the chain graph's deep seed forest: every row waits on flags the
    other workgroup raised, so a flag raised before the distance row or phase B's records
    landed would show as a mismatch."""
    kd1024.setenv("SHD_ROUTE_KDGRID", "2")
    g, _, olat, orel = _case("chain")
    eng = _engine(g)
    T = g.targets()
    plan = eng.plan(T)
    assert plan.info["seeded"] == 1 and plan.info["levels"] > 2
    lat, rel, mn = eng.rows(T, T, dispatch=False)
    _check(lat, rel, mn, olat, orel, T, T)
