"""GPU: every rows kernel on the reliability graphs of tests/rel_graphs.py -- arcs and vertices of
reliability exactly 0, tables with no lossless arc, tables on both sides of every size limit
(254 | 255, 256 | 257, 65535 | 65536), products that run through the subnormals to 0.0, and a
loss too small to change 1 - loss -- against the CPU oracle under the engine's tie rule
(TIE_MINKEY).  The latencies stay narrow (tests/test_range_gpu.py and tests/test_shape_gpu.py
cover them), so the reliabilities alone decide what a kernel does.

lat and row_min are bit-exact.  rel is bit-exact, subnormal and zero entries included, on every
graph without vertex loss: the engine promises left folds from the source, and a flush to zero,
or a product regrouped by pointer jumping, by the walks' blocks of four arcs, by a level sweep or
by KFH's folds of 16 arcs, changes bits on rel_deep.  On rel_vzero rel is bit-exact where a walk
kernel ran (fused KB; KD's walks: every path of that graph fits their 32-arc window) and
otherwise, where a level sweep multiplies f_t last, within REL_TOL on the entries the oracle
gives as normal numbers; every entry the oracle gives as 0.0 must be exactly 0.0 (the graph has
no subnormal entry: tests/test_rel_graphs.py).

A context's `info` has kernel, block and reserved (KB: fused; KF: the decimal scale of KFH's
packed arcs), and every case asserts the ones its selection must give, so that a selection that
fell back does not pass as another kernel.  KD's walk and packed flags are not in `info`:
tests/test_rel_graphs.py reads them from the host-only selection on both sides of each limit,
and every KD case here asks for a plan, which is seeded exactly where the records are packed
and the graph undirected: the packed flag as the GPU side shows it.  REFUSED lists the
(graph, selection) pairs a kernel refuses, with the reason; those contexts must report the
generic kernel, and their rows are the f64 selection's.
"""
import dataclasses
import functools

import numpy as np
import pytest

from tests import plan_check
from tests import rel_graphs as rg
from tests.test_range_gpu import (INFO_KEYS, LDS_BUDGET, REL_TOL, close_engines, dev_rows, dispatch_ref,  # noqa: F401
                                  has_loop, host_rows, oracle_rows, route, row_min_of)

pytestmark = pytest.mark.gpu

TINY = float(np.finfo(np.float64).tiny)
KD_MAXD = 32                                               # sssp_delta.hpp: arcs a KD walk takes

KD, KF = {"SHD_ROUTE_KERNEL": "kd"}, {"SHD_ROUTE_KERNEL": "kf"}
SELECTIONS = {
    "auto": {},
    "kd": KD,                                              # (256 threads below 16385 vertices)
    "kd256": {**KD, "SHD_ROUTE_KDBLOCK": "256"},
    "kd1024": {**KD, "SHD_ROUTE_KDBLOCK": "1024"},
    "kdwalk0": {**KD, "SHD_ROUTE_KDWALK": "0"},
    "kdpack0": {**KD, "SHD_ROUTE_KDPACK": "0"},
    "kb": {"SHD_ROUTE_KERNEL": "kb"},
    "kbfuse0": {"SHD_ROUTE_KERNEL": "kb", "SHD_ROUTE_KBFUSE": "0"},
    "k32": {"SHD_ROUTE_KERNEL": "k32"},
    "kf": KF,
    "kfh": {**KF, "SHD_ROUTE_KFH": "1"},
    "kfpk0": {**KF, "SHD_ROUTE_KFH": "1", "SHD_ROUTE_KFPK": "0"},
    "f64": {"SHD_ROUTE_KERNEL": "f64"},
}
KD_SELS = ("kd", "kd256", "kd1024", "kdwalk0", "kdpack0")
KB_SELS = ("kb", "kbfuse0")
KF_SELS = ("kf", "kfh", "kfpk0")

GRAPHS = tuple(n for n in rg.SUITE if n != "rel_zero8000")
BIG = ("rel_65535", "rel_65536")

_FRAC = "fractional latencies: no u16 distances, so no integer kernel"
_KF254 = "more than 254 distinct reliabilities: KF's u8 table index does not hold them"
_KBLDS = "140,000 arcs of 4 bytes do not fit KB's LDS"
REFUSED = {("rel_deep_frac", s): _FRAC for s in KD_SELS + KB_SELS + ("k32",)}
REFUSED.update({(n, s): _KF254 for n in ("rel_lossy255", "rel_256", "rel_257") + BIG for s in KF_SELS})
REFUSED.update({(n, s): _KBLDS for n in BIG for s in KB_SELS})
REFUSED.update({("rel_65536", s): "65536 distinct reliabilities: KD's u16 table index does not hold them" for s in KD_SELS})


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith(("SHD_ROUTE_", "SHD_TOPOLOGY_"))]:
        monkeypatch.delenv(k)


def choose(monkeypatch, sel, **knobs):
    for k, v in SELECTIONS[sel].items():
        monkeypatch.setenv(k, v)
    for k, v in knobs.items():
        monkeypatch.setenv("SHD_ROUTE_" + k, v)


def nrel_of(g):
    nl = g.src != g.dst
    return len(np.unique(1.0 - g.packetloss[nl]))


def expect(name, sel):
    """(kernel, fused) that `info` must report for a pair that is not in REFUSED (fused: None
    where the kernel has no such form): 0 f64, 1 K32, 2 KB, 4 KD, 5 KF / KFH."""
    nrel = nrel_of(rg.get(name))
    fused = int(nrel <= 254 and sel != "kbfuse0")
    if sel == "f64":
        return 0, None
    if sel in KF_SELS:
        return 5, None
    if sel in KD_SELS:
        return 4, None
    if sel == "k32":
        return 1, None
    if sel in KB_SELS:
        return 2, fused
    if name == "rel_deep_frac":
        return 5, None
    if name in BIG:
        return (4 if nrel <= 65535 else 1), None
    return 2, fused


def check_info(name, sel, info):
    g = rg.get(name)
    if (name, sel) in REFUSED:
        assert info["kernel"] == 0, (name, sel, REFUSED[name, sel])
        return
    kernel, fused = expect(name, sel)
    assert info["kernel"] == kernel, (name, sel, info)
    if kernel == 2:
        assert info["reserved"] == fused
    if kernel == 4:
        assert info["block"] == (1024 if sel == "kd1024" else 256) and info["reserved"] >= 1   # the bucket width
    if kernel == 5:
        assert info["lds_resident"] == (1 if sel in ("kf", "auto") else 0)
        scale = (100 if name == "rel_deep_frac" else 1) if sel == "kfh" else 0
        assert info["reserved"] == scale                      # KFH's packed arcs: head | k << 16 at that scale
    if kernel in (1, 2, 4):
        assert 0 < info["dist_bound"] < 65535 and info["lat16"] == 1
    assert info["n_vertices"] == g.n


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per graph, computed once and read-only: the sources, the oracle's rows of them over all
    vertices (NaN at a source without a self-loop), its hop counts."""
    from oracle import oracle
    g = rg.get(name)
    og = oracle.OracleGraph(g)
    S = rg.sources(name)
    if name == "rel_zero8000":
        S = S[::3]
    T = np.arange(g.n, dtype=np.int32)
    lat, rel, hops = oracle_rows(oracle, og, g, S, T)
    ref = dict(g=g, S=S, T=T, lat=lat, rel=rel, hops=hops, loops=has_loop(g), nrel=nrel_of(g))
    for k in ("lat", "rel", "hops", "loops"):
        ref[k].setflags(write=False)
    return ref


def walk_form(ref, info, sel):
    """Did a kernel run that folds ((1.0 * f_s) * f_t) and then the arcs from the source on?"""
    if info["kernel"] == 2:
        return info["reserved"] == 1
    if info["kernel"] == 4:
        return ref["nrel"] <= 254 and sel != "kdwalk0" and int(ref["hops"].max()) <= KD_MAXD
    return False


def check(ref, out, route, exact, rows=None, cols=None):
    """(lat, rel, row_min, code) against the reference's rows `rows` and columns `cols`."""
    lat, rel, mn, code = out
    rows = np.arange(len(ref["S"])) if rows is None else np.asarray(rows)
    cols = ref["T"] if cols is None else np.asarray(cols)
    S = ref["S"][rows]
    want_lat, want_rel = ref["lat"][np.ix_(rows, cols)], ref["rel"][np.ix_(rows, cols)]
    assert np.array_equal(lat, want_lat, equal_nan=True)
    nan = np.isnan(want_rel)
    assert np.array_equal(np.isnan(rel), nan)
    if exact:
        assert np.array_equal(rel, want_rel, equal_nan=True)
    else:
        zero, nrm = want_rel == 0.0, want_rel >= TINY
        assert np.all(zero | nrm | nan)                       # the reference has no subnormal entry here
        assert np.all(rel[zero] == 0.0)
        np.testing.assert_allclose(rel[nrm], want_rel[nrm], rtol=REL_TOL, atol=0)
    assert np.array_equal(mn, row_min_of(want_lat))
    failed = bool((~ref["loops"][S][:, None] & (cols[None, :] == S[:, None])).any())
    assert code == (route.ENOEDGE if failed else route.OK)


def subset(ref):
    """40 targets in no order, one of them twice, the first and the last source among them."""
    n, S = ref["g"].n, ref["S"]
    t = np.random.default_rng(n).permutation(n)[:37].astype(np.int32)
    return np.concatenate([t[:20], [S[-1], S[0]], t[20:], t[3:4]]).astype(np.int32)


# ---- every graph under every selection ---------------------------------------------------------

@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("name", GRAPHS)
def test_rows(route, monkeypatch, name, sel):
    """The sources' rows over all vertices (the host call, then a launch on the same context),
    and once over an unsorted subset of the targets with a duplicate."""
    ref = reference(name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, sel)
    eng = route.RouteEngine(g)
    info = eng.info
    print(name, sel, {k: info[k] for k in INFO_KEYS})
    check_info(name, sel, info)
    if (name, sel) in REFUSED:                                # the generic kernel: the f64 case
        eng.close()
        return
    exact = g.vertex_packetloss is None or walk_form(ref, info, sel)
    if name == "rel_vzero":
        assert int(ref["hops"].max()) <= KD_MAXD
        assert exact == (sel in ("auto", "kb", "kd", "kd256", "kd1024", "kdpack0"))
    out = host_rows(route, eng, S, T)
    check(ref, out, route, exact)
    again = dev_rows(route, eng, S, T)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again[:3], out[:3])) and again[3] == out[3]
    T2 = subset(ref)
    assert len(np.unique(T2)) == len(T2) - 1 and np.any(np.diff(T2) < 0)
    check(ref, host_rows(route, eng, S, T2), route, exact, cols=T2)
    if info["kernel"] == 4:
        # packed records from the GPU side: a plan is seeded exactly where KD found its parents
        # during the expansion, which takes an undirected graph and packed records (w < 256, at
        # most 256 reliabilities, SHD_ROUTE_KDPACK unset)
        packed = ref["nrel"] <= 256 and sel != "kdpack0"
        plan = eng.plan(S)
        assert plan.info["seeded"] == int(packed and not g.directed), (name, sel, plan.info)
        plan.close()
    eng.close()


def test_refused_pairs_are_the_listed_ones():
    """The table names existing pairs only, and the sizes it argues from are the graphs'."""
    assert all(n in GRAPHS and s in SELECTIONS for n, s in REFUSED)
    for name in GRAPHS:
        g = rg.get(name)
        nrel = nrel_of(g)
        frac = not np.all(g.latency == np.floor(g.latency))
        assert ((name, "kf") in REFUSED) == (nrel > 254)
        assert ((name, "kd") in REFUSED) == (nrel > 65535 or frac)
        assert ((name, "kb") in REFUSED) == (frac or 304 + 4 * g.nnz > LDS_BUDGET)
        assert ((name, "k32") in REFUSED) == frac
        assert (name, "auto") not in REFUSED and (name, "f64") not in REFUSED
    assert rg.get("rel_65535").nnz == 140000


def test_f64_state_in_hbm(route, monkeypatch):
    """The generic kernel with its per-source state in HBM slices (8000 vertices): arcs of
    reliability 0 and self-loops of reliability 0."""
    ref = reference("rel_zero8000")
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, "f64")
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 0 and eng.info["lds_resident"] == 0
    out = host_rows(route, eng, S, T)
    check(ref, out, route, True)
    assert (ref["rel"] == 0.0).mean() > 0.2
    eng.close()
    monkeypatch.delenv("SHD_ROUTE_KERNEL")
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 4 and eng.info["block"] == 256
    check(ref, host_rows(route, eng, S, T), route, True)
    eng.close()


# ---- K4 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in GRAPHS if n != "rel_deep_frac"])
def test_fw_rows(route, monkeypatch, name):
    """shd_route_fw_table_async + shd_route_fw_rows_async on every integer graph: the rows fold
    source-first down the tree and multiply f_t last (the tolerance rule on rel_vzero); the
    reliabilities come from a u8 table up to 255 values and from the dense matrix above."""
    ref = reference(name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, "auto")
    eng = route.RouteEngine(g)
    a16 = lambda x: (x + 15) & ~15
    assert a16(8 * g.n) + a16(2 * g.n) + a16(4 * (eng.info["dist_bound"] + 2)) <= LDS_BUDGET    # fw_prepare accepts

    def launch(d_s, d_t, lat, rel, mn):
        eng.fw_table_async()
        eng.fw_rows_async(d_s, d_t, lat, rel, mn)
    out = dev_rows(route, eng, S, T, launch)
    eng.sync()
    check(ref, out, route, g.vertex_packetloss is None)
    eng.close()


def test_fractional_graph_has_no_fw(route, monkeypatch):
    choose(monkeypatch, "auto")
    eng = route.RouteEngine(rg.get("rel_deep_frac"))
    with pytest.raises(route.RouteError) as ei:
        eng.fw_table_async()
    assert ei.value.code == route.EUNSUPPORTED
    eng.close()


# ---- the dispatch ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rel_zero", "rel_zero8000"])
def test_prefer_direct_dispatch(route, oracle_mod, monkeypatch, name):
    """rows(dispatch=True) on a prefer-direct copy: adjacent pairs take the edge itself (a dead
    edge gives 0.0 where the tree path may be alive, and the other way round), the others the
    tree path; the generic kernel runs them with the dispatch bits, state in LDS or in HBM."""
    ref = reference(name)
    g = dataclasses.replace(ref["g"], prefer_direct=True)
    S, T = ref["S"], ref["T"]
    choose(monkeypatch, "auto")
    eng = route.RouteEngine(g)
    assert eng.info["prefer_direct"] == 1
    lat, rel, mn, code = host_rows(route, eng, S, T, dispatch=True)
    el, er = dispatch_ref(oracle_mod, g, S, T)
    assert np.array_equal(lat, el, equal_nan=True) and np.array_equal(rel, er, equal_nan=True)
    assert np.array_equal(mn, row_min_of(el))
    assert code == (route.ENOEDGE if (~ref["loops"][S]).any() else route.OK)
    off = T[None, :] != S[:, None]
    assert np.count_nonzero((er == 0.0) & (ref["rel"] > 0.0) & off) >= 3      # a dead edge, a live tree path
    assert np.count_nonzero((er > 0.0) & (ref["rel"] == 0.0) & off) >= 3      # and the other way round
    eng.close()


# ---- plans -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def full_table(name):
    """The oracle's rows of every vertex (the plan validation asks for any d(s, u))."""
    from oracle import oracle
    g = rg.get(name)
    V = np.arange(g.n, dtype=np.int32)
    lat, rel, _ = oracle_rows(oracle, oracle.OracleGraph(g), g, V, V)
    for a in (lat, rel):
        a.setflags(write=False)
    return dict(g=g, S=V, T=V, lat=lat, rel=rel, loops=has_loop(g))


def plan_rows(route, eng, plan, T, reuse=False):
    import torch
    dev = torch.device("cuda", 0)
    nr = plan.info["rows"]
    d_t = torch.from_numpy(np.ascontiguousarray(T, np.int32)).to(dev)
    lat = torch.empty((nr, len(T)), dtype=torch.float64, device=dev)
    rel = torch.empty_like(lat)
    mn = torch.empty(nr, dtype=torch.float64, device=dev)
    plan.rows_async(d_t, lat, rel, mn, dispatch=False, reuse=reuse)
    code = route.OK
    try:
        eng.sync()
    except route.RouteError as e:
        code = e.code
    eng.sync()
    return lat.cpu().numpy(), rel.cpu().numpy(), mn.cpu().numpy(), code


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("name", ["rel_zero", "rel_lossy254", "rel_deep"])
def test_plan_rows(route, monkeypatch, name, world):
    """Neighbour-seeded plans over every vertex, one rank or three run in turn (seven workgroups,
    so that rows wait for the rows they start from): the job records are validated on the host
    before anything is launched, then every row is the oracle's."""
    ref = full_table(name)
    g, V = ref["g"], ref["S"]
    choose(monkeypatch, "kd", KDGRID="7")
    eng = route.RouteEngine(g)
    check_info(name, "kd", eng.info)
    seen = []
    for rank in range(world):
        plan = eng.plan(V, world, rank)
        pi = plan.info
        print(name, "rank", rank, "of", world, pi)
        assert pi["seeded"] == 1 and pi["world"] == world and pi["rank"] == rank      # packed records, fused parents
        assert pi["rows"] == len(plan.positions) > 0 and plan.landmarks() is None
        plan_check.validate(plan.jobs(), V, plan.positions, lambda s: ref["lat"][s])
        out = plan_rows(route, eng, plan, V)
        check(ref, out, route, True, rows=plan.positions)
        seen.extend(plan.positions.tolist())
        plan.close()
    assert sorted(seen) == list(range(g.n))
    eng.close()


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_landmark_only_plan(route, monkeypatch, world, rank):
    """rel_lossy254 on the context's own grid: fewer rows than workgroup slots, so every row is
    seeded from landmark rows alone, all at level 0, by a plan built on the device.  No arc of
    the landmark rows' trees is lossless."""
    ref = full_table("rel_lossy254")
    g, V = ref["g"], ref["S"]
    choose(monkeypatch, "kd")
    eng = route.RouteEngine(g)
    check_info("rel_lossy254", "kd", eng.info)
    plan = eng.plan(V, world, rank)
    lm = plan.landmarks()
    info = dict(plan.info)
    print("rel_lossy254 landmark-only", world, rank, info)
    assert lm is not None and info["seeded"] == 1 and info["levels"] == 1 and info["helpers"] == 0
    assert info["stored_rows"] == 0 and info["rows"] == len(range(rank, g.n, world))
    plan.refresh_async()
    eng.sync()
    summary = plan_check.validate(plan.jobs(), V, plan.positions, lambda s: ref["lat"][s], lm)
    assert summary["landmark_seeds"] > 0 and summary["row_seeds"] == 0
    out = plan_rows(route, eng, plan, V, reuse=True)
    check(ref, out, route, True, rows=plan.positions)
    plan.close(); eng.close()


# ---- the front end -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def topo():
    from shadow_amd import topology
    topology.load_library()
    return topology


@pytest.mark.parametrize("lat16", ["0", "1"])
@pytest.mark.parametrize("name", ["rel_zero", "rel_vzero", "rel_deep"])
def test_front_end(route, topo, oracle_mod, monkeypatch, name, lat16):
    """Topology.from_graph over the self-looped sources and their neighbours in the list, in the
    interleaved and the compact triangle: every stored pair's latency and reliability is the
    oracle's eager table's (first writer wins: row min(i, j)); a reliability of 0, or a
    subnormal one, is a routable pair like any other."""
    g = rg.get(name)
    hl = has_loop(g)
    A = np.unique(np.concatenate([rg.sources(name), np.arange(0, g.n, 7)])).astype(np.int32)
    A = A[hl[A]]
    assert len(A) >= 40
    tab = oracle_mod.OracleGraph(g).eager_table(A, prefer_direct=False, tiebreak=oracle_mod.TIE_MINKEY)
    monkeypatch.setenv("SHD_TOPOLOGY_LAT16", lat16)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    lat, rel = t.table(A)
    na = len(A)
    assert t.triangle_bytes() == (64 * route.tri16_lines(na) if lat16 == "1" else 16 * na * (na + 1) // 2)
    assert np.array_equal(lat, tab["lat"])
    want = tab["rel"]
    if g.vertex_packetloss is None:
        assert np.array_equal(rel, want)
    else:                                                       # the tolerance rule of the module docstring
        zero = want == 0.0
        assert np.all(zero | (want >= TINY)) and np.all(rel[zero] == 0.0)
        np.testing.assert_allclose(rel[~zero], want[~zero], rtol=REL_TOL, atol=0)
    assert t.min_path_latency() == tab["min_latency"]
    zi, zj = np.nonzero(want == 0.0)
    assert len(zi) >= 10
    for i, j in list(zip(zi.tolist(), zj.tolist()))[:50]:
        assert t.is_routable(int(A[i]), int(A[j])) and t.get_reliability(int(A[i]), int(A[j])) == 0.0
    if name == "rel_deep":
        sub = (want > 0.0) & (want < TINY)
        assert sub.sum() >= 2 and np.array_equal(rel[sub], want[sub])
        i, j = np.argwhere(sub)[0]
        assert t.is_routable(int(A[i]), int(A[j]))
    assert all(t.is_routable(int(a), int(b)) for a in A[:12] for b in A)
    t.close()


def test_format_path_across_a_dead_edge(topo, oracle_mod, monkeypatch):
    """One "shortest path" line whose route crosses an edge of loss 1: the line is route_fmt's
    (tests/test_hops_gpu._ref_line) with the packet loss 1.000000 of that hop and reliability 0."""
    from tests import test_hops_gpu as hg
    from tests.multi_ref import Ref
    g = rg.get("rel_zero")
    R = Ref(g)
    hl = has_loop(g)
    A = np.flatnonzero(hl).astype(np.int32)[:60]
    found = None
    for a in A.tolist():
        for b in A.tolist():
            if a < b:
                vs, es = R.path(a, b)
                if len(es) >= 2 and any(g.packetloss[e] == 1.0 for e in es):
                    found = (a, b, vs, es)
                    break
        if found:
            break
    assert found
    a, b, vs, es = found
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    assert t.is_routable(a, b) and t.get_reliability(a, b) == 0.0
    gv, ge = t.get_path(a, b)
    assert list(gv) == vs and list(ge) == es
    line = t.format_path(a, b)
    assert line == hg._ref_line(g, None, a, b, vs, es, t.get_latency(a, b), 0.0)   # (no graphml ids: the indices)
    assert "1.000000" in line
    t.close()
