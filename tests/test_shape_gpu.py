"""GPU: every rows kernel on the degenerate shapes of tests/shape_graphs.py -- vertex counts on
both sides of each size limit of shadow_amd/csrc, degrees on both sides of each degree limit,
tie-dominated graphs, trees deeper than the walk windows, graphs of one to nine vertices --
against the CPU oracle.  The value axis stays narrow (tests/test_range_gpu.py covers it): every
graph is eligible for the packed, fused and seeded encodings, so the shape alone decides.

Latency and row_min are bit-exact against the oracle's engine tie rule (TIE_MINKEY), and
latency a second time against an independent reference: the oracle's plain Floyd-Warshall of
the weight matrix up to 1200 vertices, a heap Dijkstra written here above that.  Reliability is
bit-exact without vertex loss; with it (grid_vloss) bit-exact where a walk kernel ran and within
REL_TOL otherwise (the rule of test_range_gpu.py), with one addition that no graph of that file
reaches: KD walks at most KD_MAXD = 32 arcs per target, and a row with a deeper target is redone
by its level sweep, which multiplies f_t last (sssp_delta.hpp says so: "within 1e-12"; the
public contract of include/shd_route.h is "a few ulp").  So under KD a row is held to the bits
only if the oracle's deepest path of that row has at most 32 hops -- the row of the grid's
centre, 32 hops exactly, is among the sources for that -- and to REL_TOL otherwise.  KB's fused
rows refold deeper walks in chunks and stay bit-exact at any depth.  A source without a self-loop
holds NaN at its own entry, the next sync answers SHD_ROUTE_ENOEDGE and the one after it nothing.

The limits, the expression in shadow_amd/csrc each stands for, and the sizes on either side
(test_limits_are_straddled asserts the two forms from `info`):

  fused KB rows     KB_SRC * n <= KB_CV * KB_BLOCK (prepare_k32)     sized2048 | sized2049
  fused KB rows     hubs.size() <= KB_BLOCK (prepare_k32)            bireg512 (1024 in-rows past
                    KB_SEG) | bireg513 (1026).  K_{17,1000} and K_{17,1030} (1017 | 1047 such
                    in-rows) stand on the two sides as well, but their 34000 and 35020 arcs
                    (4 bytes each) with 16 bytes per vertex and per hub part are 197 and 203 KB:
                    `kbl <= kLdsBudget` decides first and neither is a KB graph at all (asserted).
                    A d-regular graph has the hub count with half the arcs, and fits.
  KF 256 -> 1024    n <= 16 * 256 && kf_lds_bytes<256>(n) <= kLdsBudget / 4 (prepare_kf)
                    sized2688 | sized2689: the LDS term decides (40896 | 40976 bytes against
                    40960), so n <= 16 * 256 never does; sized4096 | sized4097 are both 1024.
  KF -> KFH         n <= 16 * 1024 && kf_lds_bytes<1024>(n) <= kLdsBudget (prepare_kf)
                    sized11212 | sized11213: the LDS term again; sized16384 | sized16385 are
                    both KFH.
  KD block          n > 16384 ? 1024 : 256 (prepare_k32)             sized16384 | sized16385
  bitmask words     nw = (n + 63) / 64                                sized63 | 64 | 65
  latency blocks    256 vertices, tails of eight (kd_lat_row)         sized255 | 256 | 257
  KB / K32 threads  KB_BLOCK, one vertex per thread of 1024           sized1023 | 1024 | 1025
  queue capacity    qcap = max(8, qcap & ~7) (prepare_k32)            tiny 1, 2, 3, 7 | 8, 9
  hub parts         KB_SEG = 16 arcs per segment                      star1100: one in-row of 69
  whole-wave scans  KF_HUB = 24, HP_WIDE = 32                         lollipop (K_40), bicliques
  improving arcs    KD_IMP = 192, flushed past 128                    star: n - 1 from one vertex
  walk windows      KD_MAXD = KB_MAXD = 32 arcs                       grid (63 hops), lollipop
                    (300), bireg (35); ties on nearly every entry of grid, dir_grid, bicliques
"""
import heapq

import numpy as np
import pytest

from tests import shape_graphs as sg
from tests import test_hops_gpu as hg
from tests import test_loads_gpu as lg
from tests.test_range_gpu import (INFO_KEYS, LDS_BUDGET, REL_TOL, SELECTIONS, close_engines, dev_rows,  # noqa: F401
                                  has_loop, host_rows, oracle_rows, read_triangle, route, row_min_of, select,
                                  walk_kernel)
from tests.test_shape_graphs import in_degree

pytestmark = pytest.mark.gpu

SIZED = tuple(f"sized{n}" for n in sg.SIZES)
SHAPES = SIZED + ("star300", "star1100") + sg.BICLIQUES + sg.BIREGS + ("grid", "grid_vloss", "lollipop", "dir_grid")
KD_MAXD = 32                                                       # sssp_delta.hpp
GRID_CENTRE = 16 * 33 + 16                                         # 32 hops from the farthest corner
BIG_SELS = ("auto", "kd", "kdwalk0", "kf", "kfh", "f64")          # the two 16k graphs
_EXTRA_KNOBS = ("SHD_ROUTE_QCAP", "SHD_ROUTE_DELTA", "SHD_ROUTE_KDGRID", "SHD_ROUTE_KBGRID", "SHD_ROUTE_EVCAP",
                "SHD_ROUTE_SEEDS", "SHD_ROUTE_KDBLOCK", "SHD_ROUTE_LANDMARKS", "SHD_ROUTE_PLAN_DELTA")


def choose(monkeypatch, sel, **knobs):
    select(monkeypatch, sel)
    for k in _EXTRA_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv("SHD_ROUTE_" + k, v)


def sources(g):
    """Every vertex of a graph up to 400 vertices; else at most 16: vertex 0, vertex n - 1, the
    vertex of the highest degree, a leaf (the lowest), and vertices with and without a self-loop
    (on the 32 x 33 grid also its centre, whose row is exactly KD_MAXD hops deep)."""
    if g.n <= 400:
        return np.arange(g.n, dtype=np.int32)
    hl, d = has_loop(g), in_degree(g)
    a, b = np.flatnonzero(hl), np.flatnonzero(~hl)
    pick = [0, g.n - 1, int(np.argmax(d)), int(np.argmin(d))]
    if g.name.startswith("grid32x33"):
        pick.append(GRID_CENTRE)
    pick += [int(a[k * len(a) // 6]) for k in range(6)] + [int(b[k * len(b) // 6]) for k in range(6)]
    return np.array(list(dict.fromkeys(pick)), np.int32)


def dijkstra_rows(g, S):
    """Latencies from the sources S by a binary-heap Dijkstra over adjacency lists."""
    adj = [[] for _ in range(g.n)]
    for a, b, w in zip(g.src.tolist(), g.dst.tolist(), g.latency.tolist()):
        if a != b:
            adj[a].append((b, w))
            if not g.directed:
                adj[b].append((a, w))
    out = np.empty((len(S), g.n))
    for i, s in enumerate(S.tolist()):
        dist = [float("inf")] * g.n
        dist[s] = 0.0
        heap = [(0.0, s)]
        while heap:
            d, u = heapq.heappop(heap)
            if d > dist[u]:
                continue
            for v, w in adj[u]:
                if d + w < dist[v]:
                    dist[v] = d + w
                    heapq.heappush(heap, (d + w, v))
        out[i] = dist
    return out


_REF = {}


def reference(oracle_mod, name, every_vertex=False):
    """Per graph, computed once and never written to: the oracle graph, the sources, their
    oracle rows (latency, reliability, hops) over all vertices under TIE_MINKEY and the
    independent latencies of those sources."""
    key = (name, every_vertex)
    if key not in _REF:
        g = sg.get(name)
        og = oracle_mod.OracleGraph(g)
        S = np.arange(g.n, dtype=np.int32) if every_vertex else sources(g)
        T = np.arange(g.n, dtype=np.int32)
        lat, rel, hops = oracle_rows(oracle_mod, og, g, S, T)
        if g.n <= 1200:
            d = np.full((g.n, g.n), np.inf)
            np.fill_diagonal(d, 0.0)
            nl = g.src != g.dst
            a, b, w = g.src[nl], g.dst[nl], g.latency[nl]
            np.minimum.at(d, (a, b), w)
            if not g.directed:
                np.minimum.at(d, (b, a), w)
            ind = oracle_mod.floyd_warshall(d)[S]
        else:
            ind = dijkstra_rows(g, S)
        nl = g.src != g.dst
        ref = dict(g=g, og=og, S=S, T=T, lat=lat, rel=rel, hops=hops, ind=ind, loops=has_loop(g),
                   nrel=len(np.unique(1.0 - g.packetloss[nl])))
        for k in ("lat", "rel", "hops", "ind", "loops"):
            ref[k].setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def check_rows(ref, out, route, exact_rel=True, rows=None):
    """(lat, rel, row_min, code) of the reference's sources (or of its rows `rows`, repeats
    allowed) against both references."""
    lat, rel, mn, code = out
    rows = np.arange(len(ref["S"])) if rows is None else np.asarray(rows)
    S, want_lat, want_rel = ref["S"][rows], ref["lat"][rows], ref["rel"][rows]
    assert np.array_equal(lat, want_lat, equal_nan=True)
    ex = np.broadcast_to(np.asarray(exact_rel, bool), (len(ref["S"]),))[rows]       # per source
    assert np.array_equal(np.isnan(rel), np.isnan(want_rel))
    np.testing.assert_allclose(rel[~ex], want_rel[~ex], rtol=REL_TOL, atol=0)
    assert np.array_equal(rel[ex], want_rel[ex], equal_nan=True)
    assert np.array_equal(mn, row_min_of(want_lat))
    assert code == (route.ENOEDGE if (~ref["loops"][S]).any() else route.OK)
    off = ref["T"][None, :] != S[:, None]
    assert np.array_equal(np.isnan(lat), ~off & ~ref["loops"][S][:, None])
    assert np.array_equal(lat[off], ref["ind"][rows][off])       # the second, independent reference


def launch_rows(route, eng, S, T, launch=None):
    """dev_rows, and the sync after it: a failure is reported once."""
    out = dev_rows(route, eng, S, T, launch)
    eng.sync()
    return out


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def kb_fits(g):
    """KB's LDS rule (prepare_k32: AttrLayout and `kbl <= kLdsBudget`): 32 + 10 bytes per vertex
    for K2, and 304 + 4 per arc + 16 per vertex + 16 per hub part for the batch kernel."""
    a16 = lambda x: (x + 15) & ~15
    d = in_degree(g)
    npart = int(np.ceil(d[d > 16] / 16).sum())
    return (32 + a16(8 * g.n) + a16(2 * g.n) <= LDS_BUDGET
            and 304 + a16(4 * g.nnz) + a16(16 * g.n) + a16(16 * npart) <= LDS_BUDGET)


def expect_kernel(g, sel):
    """info["kernel"] by the eligibility rules of shd_route_create for a narrow-range graph
    (0 f64, 1 K32, 2 KB, 4 KD, 5 KF/KFH): a forced kernel that cannot take the graph falls back
    to the generic one."""
    if sel == "f64":
        return 0
    if g.nnz == 0 and sel in ("kd", "kdwalk0", "kf", "kfh"):
        return 0                                                       # KD and KF need an arc
    if sel in ("kf", "kfh"):
        return 5
    if sel in ("kd", "kdwalk0"):
        return 4
    if sel == "k32":
        return 1 if 14.2 * g.n + 2048 <= LDS_BUDGET else 0             # K32Layout: key, relv, par, bits
    if sel in ("kb", "kbfuse0"):
        return 2 if kb_fits(g) else 0
    return 2 if kb_fits(g) else 4


def exact_rel(ref, info, sel):
    """Per source of the reference: is its reliability row held to the bits?  Always without
    vertex loss; with it where a walk kernel ran, and under KD only the rows whose deepest path
    fits the walk window (a deeper row is redone by the level sweep)."""
    ns = len(ref["S"])
    if ref["g"].vertex_packetloss is None:
        return np.ones(ns, bool)
    if not walk_kernel(info, sel, ref["nrel"]):
        return np.zeros(ns, bool)
    if info["kernel"] == 4:
        return ref["hops"].max(axis=1) <= KD_MAXD
    return np.ones(ns, bool)


# ---- every shape under every selection -------------------------------------------------------

ROW_CASES = [(n, s) for n in SHAPES for s in SELECTIONS if n not in ("sized16384", "sized16385") or s in BIG_SELS]


@pytest.mark.parametrize("name,sel", ROW_CASES)
def test_rows(route, oracle_mod, monkeypatch, name, sel):
    """The sources' rows over all vertices under one kernel selection: the host call, then
    three launches on the same context, all identical."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, sel)
    eng = route.RouteEngine(g)
    info = eng.info
    print(name, sel, {k: info[k] for k in INFO_KEYS})
    assert info["kernel"] == expect_kernel(g, sel)
    if sel in ("f64", "kf", "kfh"):
        assert info["dist_bound"] == 0 and info["lat16"] == 0
    else:
        assert 0 < info["dist_bound"] < 65535 and info["lat16"] == 1
    if sel == "kfh":
        assert info["lds_resident"] == 0
    exact = exact_rel(ref, info, sel)
    if name == "grid_vloss" and sel == "kd":
        assert 0 < exact.sum() < len(S) and ref["hops"][list(S).index(GRID_CENTRE)].max() == KD_MAXD
    out = host_rows(route, eng, S, T)
    check_rows(ref, out, route, exact_rel=exact)
    for _ in range(3):
        assert same(launch_rows(route, eng, S, T), out)
    eng.close()


def test_limits_are_straddled(route, monkeypatch):
    """From `info`: the two neighbouring sizes of each limit took the two different forms (the
    table in the module docstring).  Where a condition of shd_route_create is shadowed by an LDS
    size -- n <= 16 * 256 and n <= 16 * 1024 in prepare_kf, and `kbl <= kLdsBudget` for
    K_{17,b} -- the pair stands on the two sides of the size that does decide, and the
    shadowed pair is asserted to take one form."""
    def info(name, sel):
        choose(monkeypatch, sel)
        e = route.RouteEngine(sg.get(name))
        i = dict(e.info)
        e.close()
        print(name, sel, {k: i[k] for k in INFO_KEYS})
        return i

    # fused KB rows: KB_SRC * n <= KB_CV * KB_BLOCK
    a, b = info("sized2048", "kb"), info("sized2049", "kb")
    assert (a["kernel"], a["reserved"]) == (2, 1) and (b["kernel"], b["reserved"]) == (2, 0)
    # KF's 256-thread rows, then its 1024-thread rows
    a, b = info("sized2688", "kf"), info("sized2689", "kf")
    assert (a["kernel"], a["block"], a["lds_resident"]) == (5, 256, 1)
    assert (b["kernel"], b["block"], b["lds_resident"]) == (5, 1024, 1)
    for name in ("sized4096", "sized4097"):
        i = info(name, "kf")
        assert (i["kernel"], i["block"], i["lds_resident"]) == (5, 1024, 1)
    # KF, then KFH
    a, b = info("sized11212", "kf"), info("sized11213", "kf")
    assert (a["kernel"], a["block"], a["lds_resident"]) == (5, 1024, 1)
    assert (b["kernel"], b["block"], b["lds_resident"]) == (5, 1024, 0)
    for name in ("sized16384", "sized16385"):
        i = info(name, "kf")
        assert (i["kernel"], i["block"], i["lds_resident"]) == (5, 1024, 0)
    # KD's block size
    a, b = info("sized16384", "kd"), info("sized16385", "kd")
    assert (a["kernel"], a["block"]) == (4, 256) and (b["kernel"], b["block"]) == (4, 1024)
    # fused and unfused KB by the number of hub in-rows
    a, b = info("bireg512", "kb"), info("bireg513", "kb")
    assert (a["kernel"], a["reserved"]) == (2, 1) and (b["kernel"], b["reserved"]) == (2, 0)
    for name in sg.BICLIQUES:
        assert not kb_fits(sg.get(name))
        assert info(name, "kb")["kernel"] == 0 and info(name, "auto")["kernel"] == 4


# ---- one to nine vertices --------------------------------------------------------------------

@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("loops", sg.TINY_LOOPS)
@pytest.mark.parametrize("n", sg.TINY_N)
def test_tiny_kernels(route, oracle_mod, monkeypatch, n, loops, sel):
    """A kernel launch (no dispatch) on a path of n vertices: as selected; KD also with a
    64-entry queue and bucket width 1; and from seven vertices on with grids of 7 (KD) and 3
    (KB) workgroups over every source three times, so that a workgroup runs several in turn."""
    name = f"tiny{n}_{loops}"
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    variants = [({}, None)]
    if sel in ("kd", "kdwalk0"):
        variants.append((dict(QCAP="64", DELTA="1"), None))
    if n >= 7:
        variants.append((dict(KDGRID="7", KBGRID="3"), np.tile(np.arange(n), 3)))
    for knobs, rows in variants:
        choose(monkeypatch, sel, **knobs)
        eng = route.RouteEngine(g)
        info = eng.info
        print(name, sel, knobs, {k: info[k] for k in INFO_KEYS})
        assert info["kernel"] == expect_kernel(g, sel)
        src = S if rows is None else S[rows]
        out = host_rows(route, eng, src, T)
        check_rows(ref, out, route, rows=rows)
        for _ in range(2):
            assert same(launch_rows(route, eng, src, T), out)
        if name == "tiny1_none":
            assert np.isnan(out[0]).all() and np.isnan(out[1]).all() and out[0].shape == (1, 1)
            assert out[2][0] == np.inf and out[3] == route.ENOEDGE
        eng.close()


# ---- plans -----------------------------------------------------------------------------------

def plan_rows(route, eng, plan, T):
    """The plan's rows (buffers of one row at least) -> host arrays, the sync's code."""
    import torch
    dev = torch.device("cuda", 0)
    nr = plan.info["rows"]
    d_t = torch.from_numpy(np.ascontiguousarray(T, np.int32)).to(dev)
    lat = torch.full((max(1, nr), len(T)), -7.0, dtype=torch.float64, device=dev)
    rel = torch.full_like(lat, -7.0)
    mn = torch.full((max(1, nr),), -7.0, dtype=torch.float64, device=dev)
    plan.rows_async(d_t, lat, rel, mn, dispatch=False)
    code = route.OK
    try:
        eng.sync()
    except route.RouteError as e:
        code = e.code
    eng.sync()
    assert nr > 0 or (float(lat.min()) == -7.0 and float(mn.min()) == -7.0)      # nothing written
    return lat[:nr].cpu().numpy(), rel[:nr].cpu().numpy(), mn[:nr].cpu().numpy(), code


def want_seeded(g, info, nrel, nrows):
    """As test_range_gpu.test_plan_rows derives it: KD selected, undirected, packed records
    (w < 256 and <= 256 reliabilities), no prefer-direct; a plan of two rows at least."""
    nl = g.src != g.dst
    packed = g.latency[nl].max() < 256 and nrel <= 256
    return int(info["kernel"] == 4 and packed and not g.directed and not g.prefer_direct and nrows >= 2)


PLAN_SHAPES = ("star1100", "grid", "biclique1000", "biclique1030", "lollipop", "sized1025")


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("sel", ["auto", "kd"])
@pytest.mark.parametrize("name", PLAN_SHAPES)
def test_plan_rows(route, oracle_mod, monkeypatch, name, sel, world):
    """Plans over the sources in an order of their own, one rank or three run in turn: the
    ranks' positions cover the sources exactly once, a plan is seeded where the code says so,
    and the rows are the reference's."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, sel)
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == expect_kernel(g, sel)
    order = np.arange(len(S))[::-1].copy()
    seen = []
    for rank in range(world):
        plan = eng.plan(S[order], world, rank)
        pi = plan.info
        print(name, sel, "kernel", eng.info["kernel"], "rank", rank, "of", world, pi)
        assert pi["world"] == world and pi["rank"] == rank and pi["rows"] == len(plan.positions) > 0
        assert pi["seeded"] == want_seeded(g, eng.info, ref["nrel"], len(S))
        rows = order[plan.positions]
        exact = exact_rel(ref, eng.info, sel)
        out = plan_rows(route, eng, plan, T)
        check_rows(ref, out, route, exact_rel=exact, rows=rows)
        if world == 1:
            assert same(plan_rows(route, eng, plan, T), out)
        seen.extend(plan.positions.tolist())
        plan.close()
    assert sorted(seen) == list(range(len(S)))
    eng.close()


@pytest.mark.parametrize("name", ["tiny1_all", "tiny2_none", "tiny3_some", "tiny9_some"])
def test_plan_ranks_without_rows(route, oracle_mod, monkeypatch, name):
    """Eight ranks over one to nine sources under KD: a rank without rows makes its plan, runs
    it and writes nothing; the others' rows are the reference's."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, "kd")
    eng = route.RouteEngine(g)
    seen, empty = [], 0
    for rank in range(8):
        plan = eng.plan(S, 8, rank)
        print(name, "rank", rank, plan.info)
        assert plan.info["rows"] == len(plan.positions)
        out = plan_rows(route, eng, plan, T)
        if plan.info["rows"] == 0:
            empty += 1
            assert out[3] == route.OK
        else:
            check_rows(ref, out, route, rows=plan.positions)
        seen.extend(plan.positions.tolist())
        plan.close()
    assert sorted(seen) == list(range(len(S))) and empty >= 8 - len(S)
    eng.close()


@pytest.mark.parametrize("seeds,evcap", [(None, "0"), (None, "2"), ("1", None), ("3", None)])
def test_seeded_rows_where_ties_are_the_rule(route, oracle_mod, monkeypatch, seeds, evcap):
    """The knobs of test_seed_gpu.test_seeded_rows_bitexact on the whole grid (every vertex a
    source, seven workgroups): a tie-event list of 0 or 2 entries, which nearly every seeded
    row overflows (it reruns unseeded), and rows started from one or three neighbour rows."""
    ref = reference(oracle_mod, "grid", every_vertex=True)
    g, S, T = ref["g"], ref["S"], ref["T"]
    knobs = dict(KDGRID="7")
    if evcap is not None:
        knobs["EVCAP"] = evcap
    if seeds is not None:
        knobs["SEEDS"] = seeds
    choose(monkeypatch, "kd", **knobs)
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 4
    plan = eng.plan(S)
    print("grid", knobs, plan.info)
    assert plan.info["seeded"] == 1 and plan.info["rows"] == g.n and plan.info["stored_rows"] > 0
    out = plan_rows(route, eng, plan, T)
    check_rows(ref, out, route, rows=plan.positions)
    plan.close(); eng.close()


# ---- K4 ----------------------------------------------------------------------------------------

FW_SHAPES = ("sized63", "sized64", "sized65", "sized255", "sized256", "sized257", "sized1023", "sized1024", "sized1025",
             "sized2049", "sized16384", "star300", "biclique1030", "bireg513", "grid", "grid_vloss", "lollipop",
             "dir_grid", "tiny1_none", "tiny1_all", "tiny2_all", "tiny3_some", "tiny9_none")


def fw_accepts(info, n):
    """fw_prepare: integer latencies, 0 < bound < 0xFFFF, at most 12000 vertices, and the rows'
    LDS state (10 n + 4 (bound + 2) bytes) within the budget."""
    a16 = lambda x: (x + 15) & ~15
    return (0 < info["dist_bound"] < 65535 and n <= 12000
            and a16(8 * n) + a16(2 * n) + a16(4 * (info["dist_bound"] + 2)) <= LDS_BUDGET)


@pytest.mark.parametrize("name", FW_SHAPES)
def test_fw_rows(route, oracle_mod, monkeypatch, name):
    """shd_route_fw_table_async + shd_route_fw_rows_async at the sizes around the tile (64) and
    region (128, 256) edges and on the shapes; EUNSUPPORTED, every time, where fw_prepare
    refuses (a graph without an arc has bound 0; 16384 vertices are past the rows' LDS)."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, "auto")
    eng = route.RouteEngine(g)
    accepts = fw_accepts(eng.info, g.n)
    assert accepts == (name not in ("sized16384", "tiny1_none", "tiny1_all"))
    if not accepts:
        for _ in range(2):
            with pytest.raises(route.RouteError) as ei:
                eng.fw_table_async()
            assert ei.value.code == route.EUNSUPPORTED
        eng.close()
        return

    def launch(d_s, d_t, lat, rel, mn):
        eng.fw_table_async()
        eng.fw_rows_async(d_s, d_t, lat, rel, mn)
    out = launch_rows(route, eng, S, T, launch)
    check_rows(ref, out, route, exact_rel=g.vertex_packetloss is None)
    assert same(launch_rows(route, eng, S, T, launch), out)
    eng.close()


# ---- hops, routes, loads -----------------------------------------------------------------------

HOP_SHAPES = ("star1100", "grid", "biclique1000", "biclique1030", "lollipop", "tiny1_none", "tiny1_all", "tiny2_none",
              "tiny3_some", "tiny8_all", "tiny9_some")


@pytest.fixture
def shape_fixtures(monkeypatch, oracle_mod):
    """tests/test_hops_gpu.py's and tests/test_loads_gpu.py's host statements look their graph
    up by name: the name "shape:<name>" gives a shape_graphs graph and its reference sources."""
    real = hg._graph

    def lookup(name):
        if name.startswith("shape:"):
            return sg.get(name[6:]), reference(oracle_mod, name[6:])["S"]
        return real(name)
    monkeypatch.setattr(hg, "_graph", lookup)


@pytest.mark.parametrize("name", HOP_SHAPES)
def test_hops_and_loads(route, oracle_mod, monkeypatch, shape_fixtures, name):
    """Hop counts against the oracle's, explicit routes against its parent chain, and unit
    loads against the host sum over its routes (test_loads_gpu.ref_loads).  The star sends
    nearly every path through one vertex; the grid gives the depth counting sort 63 levels,
    the lollipop 300."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    key = "shape:" + name
    choose(monkeypatch, "auto")
    eng = route.RouteEngine(g)
    noloop = bool((~ref["loops"][S]).any())
    try:
        hops, mx = eng.hops(S, T, dispatch=False)
        code = route.OK
    except route.RouteError as err:
        (hops, mx), code = err.partial, err.code
    assert code == (route.ENOEDGE if noloop else route.OK)
    assert hops.dtype == np.int32 and np.array_equal(hops, ref["hops"])
    assert np.array_equal(mx, ref["hops"].max(axis=1))
    if name == "grid":
        assert mx.max() == 63
    # routes: the first 16 sources to every vertex, themselves included
    A = S[:16]
    ps = np.repeat(A, g.n).astype(np.int32); pt = np.tile(T, len(A)).astype(np.int32)
    try:
        off, vert, edge = eng.paths(ps, pt, dispatch=False)
        code = route.OK
    except route.RouteError as err:
        (off, vert, edge), code = err.partial, err.code
    assert code == (route.ENOEDGE if (~ref["loops"][A]).any() else route.OK)
    paths = hg.split_paths(route, off, vert, edge)
    assert np.array_equal(np.maximum(np.diff(off) - 1, -1)[ps != pt], ref["hops"][:len(A)].reshape(-1)[ps != pt])
    for k in np.flatnonzero(ps == pt).tolist():
        s = int(ps[k])
        if ref["loops"][s]:
            assert list(paths[k][0]) == [s, s] and list(paths[k][1]) == [hg._self_eid(g, s)]
        else:
            assert len(paths[k][0]) == 0
    sub = np.flatnonzero(ps != pt)
    if len(sub):
        o2 = np.concatenate([[0], np.cumsum(np.diff(off)[sub])])
        v2 = np.concatenate([paths[k][0] for k in sub]); e2 = np.concatenate([paths[k][1] for k in sub])
        hg.check_chain(key, route, ps[sub], pt[sub], o2, v2, e2)
    # loads, one unit per entry
    if g.m == 0:
        el, tr, un, code = lg.run(route, eng.loads, S, T, None, dispatch=False)
        assert len(el) == 0 and not tr.any() and un == 1 and code == route.ENOEDGE
    else:
        got = lg.check(route, key, eng, S, T, None, False)
        assert got[2] == int((~ref["loops"][S]).sum())
        if name.startswith("star"):                       # nearly everything passes through vertex 0
            assert got[1][0] >= (len(S) - 2) * (g.n - 3) and got[1][1:].max() <= len(S)
    eng.close()


# ---- the front end's triangle ------------------------------------------------------------------

@pytest.mark.parametrize("lat16", [False, True])
@pytest.mark.parametrize("name", ["grid", "tiny3_some"])
def test_fill_triangle(route, oracle_mod, monkeypatch, name, lat16):
    """shd_route_fill_triangle in both layouts over the self-looped vertices, against the
    oracle's eager table of them."""
    g = sg.get(name)
    A = np.flatnonzero(has_loop(g)).astype(np.int32)
    na = len(A)
    tab = oracle_mod.OracleGraph(g).eager_table(A, prefer_direct=False, tiebreak=oracle_mod.TIE_MINKEY)
    choose(monkeypatch, "auto")
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1
    nbytes = 64 * route.tri16_lines(na) if lat16 else 16 * na * (na + 1) // 2
    buf = route.PinnedBuffer(nbytes)
    buf.array()[:] = -7.0
    mn, _ = eng.fill_triangle(A, buf, dispatch=True, lat16=lat16)
    lat, rel = read_triangle(route, buf, na, lat16)
    iu = np.triu_indices(na)
    assert np.array_equal(lat[iu], tab["lat"][iu]) and np.array_equal(rel[iu], tab["rel"][iu])
    assert mn == tab["min_latency"] == tab["lat"][iu].min()
    buf.close(); eng.close()
