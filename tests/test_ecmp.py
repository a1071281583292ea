"""CPU: the reference of the ECMP link loads (tests/ecmp_ref.py) in f64 against the same
programme in exact fractions, against networkx's betweenness, against Ref.loads where paths
are unique and on parallel tight edges; the interface through every layer; and the state
layout of the sweep (shadow_amd/csrc/ecmp_layout.hpp) through a stand-alone program under the
host sanitizers."""
import functools
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from shadow_amd.graph import Graph
from tests import ecmp_ref as er
from tests import shape_graphs as sg
from tests import test_ties_gpu as tg
from tests import ties_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_ecmp_loads_async", "shd_route_ecmp_loads", "shd_route_pair_ecmp_loads")
TOPO_SYMS = ("shd_topology_ecmp_link_loads",)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "grid6x7":
        return sg.grid(6, 7)
    if name == "dir_grid6x6":
        return sg.dir_grid(6, 6)
    if name == "lollipop8_20":
        return sg.lollipop(8, 20)
    if name == "biclique3_4":
        return sg.biclique(3, 4)
    return tg.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return er.EcmpRef(graph(name))


TINY = [f"tiny{n}_{lp}" for n in sg.TINY_N for lp in sg.TINY_LOOPS]
GRAPHS = ["grid6x7", "dir_grid6x6", "lollipop8_20", "sized63", "ba60_multi_equal", "ba64_ties"] + TINY


def sources(name):
    g = graph(name)
    if name == "ba64_ties":
        return tg.hg._graph(name)[1][:8]
    return np.arange(g.n, dtype=np.int32)


# ---- the interface -------------------------------------------------------------------------------

def test_declarations():
    import ctypes
    from shadow_amd import build, route, topology
    build.build()
    text = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("shd_route.h", "shd_topology.h")}
    assert set(ROUTE_SYMS) <= set(re.findall(r"\b(shd_route_[a-z_]+)\s*\(", text["shd_route.h"]))
    assert set(TOPO_SYMS) <= set(re.findall(r"\b(shd_topology_[a-z_]+)\s*\(", text["shd_topology.h"]))
    assert set(ROUTE_SYMS) <= set(route.EXPORTS) and set(TOPO_SYMS) <= set(topology.EXPORTS)
    eng, front = ctypes.CDLL(route.LIB_PATH), ctypes.CDLL(topology.LIB_PATH)
    for sym in ROUTE_SYMS:
        assert hasattr(eng, sym), sym
    for sym in TOPO_SYMS:
        assert hasattr(front, sym), sym
    for name in ("ecmp_loads", "pair_ecmp_loads", "ecmp_loads_async"):
        assert callable(getattr(route.RouteEngine, name))
    assert callable(topology.Topology.ecmp_link_loads)
    # the prototypes: double outputs, a uint64_t unrouted, the weights const uint64_t
    h = re.sub(r"\s+", " ", text["shd_route.h"])
    assert ("int shd_route_ecmp_loads_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, "
            "int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt, double* d_edge_load, double* d_transit, "
            "uint64_t* d_unrouted, void* stream);") in h
    assert ("int shd_route_ecmp_loads(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, "
            "uint32_t flags, const uint64_t* wt, double* edge_load_out, double* transit_out, "
            "uint64_t* unrouted_out);") in h
    assert ("int shd_route_pair_ecmp_loads(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, "
            "const uint64_t* pair_wt, int64_t npairs, uint32_t flags, double* edge_load_out, double* transit_out, "
            "uint64_t* unrouted_out);") in h
    t = re.sub(r"\s+", " ", text["shd_topology.h"])
    assert ("int shd_topology_ecmp_link_loads(shd_topology_t* top, double* edge_packets, double* transit_packets, "
            "uint64_t* unrouted);") in t


# ---- f64 against exact fractions ---------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_f64_against_fractions(name, weighted):
    """The f64 programme stays within tol of the exact one and has its zero pattern."""
    g, R = graph(name), ref(name)
    S = sources(name)
    T = np.arange(g.n, dtype=np.int32)
    W = np.random.default_rng(g.n).integers(0, 1 << 20, size=(len(S), g.n)) if weighted else None
    f = R.rows(S, T, W)
    x = R.rows(S, T, W, exact=True)
    rtol = R.tol(S)
    print(name, "R, D", R.shape(S), "rtol / u", rtol * 2 ** 53, "worst / u", er.worst(f[0], x[0]), er.worst(f[1], x[1]))
    assert er.close(f[0], x[0], rtol) and er.close(f[1], x[1], rtol)
    assert f[2] == x[2] and f[3] == x[3]
    if not name.startswith("tiny"):
        assert np.count_nonzero(f[0]) > 0 and np.count_nonzero(f[1]) > 0
    # conservation, exactly: every routed entry's weight is on the edges once per hop, and
    # what passes through vertices is what the edges carry less one hop per routed entry
    routed = sum(x[0]) - sum(x[1])
    total = Fraction(int(np.sum(W, dtype=object)) if weighted else len(S) * g.n)
    assert routed == total - x[2]


# ---- networkx ------------------------------------------------------------------------------------

def _simple(g):
    nl = g.src != g.dst
    a, b = g.src[nl].astype(np.int64), g.dst[nl].astype(np.int64)
    key = a * g.n + b if g.directed else np.minimum(a, b) * g.n + np.maximum(a, b)
    return len(np.unique(key)) == len(key)


@pytest.mark.parametrize("name", ["grid6x7", "dir_grid6x6", "lollipop8_20", "sized63"] + TINY)
def test_networkx_betweenness(name):
    """Weight 1 on all ordered pairs: the edge loads are the edge betweenness and the transit
    the vertex betweenness of networkx, twice on undirected graphs (it counts unordered pairs)."""
    nx = pytest.importorskip("networkx")
    g = graph(name)
    assert _simple(g)
    G = nx.DiGraph() if g.directed else nx.Graph()
    G.add_nodes_from(range(g.n))
    for e in np.flatnonzero(g.src != g.dst).tolist():
        G.add_edge(int(g.src[e]), int(g.dst[e]), weight=float(g.latency[e]), eid=e)
    S = np.arange(g.n, dtype=np.int32)
    el, trn, un, codes = ref(name).rows(S, S)
    eb = nx.edge_betweenness_centrality(G, normalized=False, weight="weight")
    vb = nx.betweenness_centrality(G, normalized=False, weight="weight")
    k = 1.0 if g.directed else 2.0
    want_e = np.zeros(g.m)
    for (a, b), v in eb.items():
        want_e[G.edges[a, b]["eid"]] = k * v
    loops = np.flatnonzero(g.src == g.dst)
    got_e = el.copy()
    for v in range(g.n):                                      # the self entries are no betweenness
        lv = loops[g.src[loops] == v]
        if len(lv):
            assert got_e[lv[0]] == 1.0 and not got_e[lv[1:]].any()
            got_e[lv[0]] = 0.0
    assert un == g.n - len(np.unique(g.src[loops]))
    assert np.allclose(got_e, want_e, rtol=1e-12, atol=1e-12)
    assert np.allclose(trn, k * np.array([vb[v] for v in range(g.n)]), rtol=1e-12, atol=1e-12)


# ---- unique paths: the single-path loads -----------------------------------------------------------

def test_unique_paths_equal_the_loads():
    """ba90_frac (fractional latencies): every listed pair has exactly one shortest path, so
    the f64 programme gives Ref.loads converted to double, exactly."""
    name = "ba90_frac"
    g, A = tg.hg._graph(name)
    T = np.arange(g.n, dtype=np.int32)
    cnt = tr.TiesRef(g).rows(A, T)[0]
    off = T[None, :] != np.asarray(A)[:, None]
    assert np.all(cnt[off] == 1)
    W = np.random.default_rng(90).integers(0, 1 << 20, size=(len(A), g.n))
    for w in (None, W):
        f = ref(name).rows(A, T, w)
        ps, pt = np.repeat(A, g.n), np.tile(T, len(A))
        el, trn, un = ref(name).ref.loads(ps, pt, None if w is None else w.reshape(-1))
        assert np.array_equal(f[0], el.astype(np.float64)) and np.array_equal(f[1], trn.astype(np.float64))
        assert f[2] == un and int(el.max()) < 2 ** 53
        p = ref(name).pairs(ps[::-1], pt[::-1], None if w is None else w.reshape(-1)[::-1])
        assert np.array_equal(p[0], f[0]) and np.array_equal(p[1], f[1]) and p[2] == f[2]


# ---- parallel tight edges and heavy ties -----------------------------------------------------------

def test_parallel_tight_edges_share():
    """Two parallel edges of one latency between 0 and 1, then 1 - 2: each parallel edge gets
    half of what crosses, a slower third parallel edge nothing."""
    g = Graph(n=3, src=np.array([0, 0, 1, 0], np.int32), dst=np.array([1, 1, 2, 1], np.int32),
              latency=np.array([2.0, 2.0, 1.0, 3.0]), packetloss=np.zeros(4), name="par")
    R = er.EcmpRef(g)
    el, trn, un, codes = R.rows([0], [1, 2], np.array([[6, 10]], np.uint64))
    assert el.tolist() == [8.0, 8.0, 10.0, 0.0] and trn.tolist() == [0.0, 10.0, 0.0] and un == 0 and not codes
    el, trn, un, codes = R.rows([2], [0, 2], None)
    assert el.tolist() == [0.5, 0.5, 1.0, 0.0] and trn.tolist() == [0.0, 1.0, 0.0]
    assert un == 1 and codes == {er.ENOEDGE}                   # no self-loop at 2


def test_biclique_splits_over_the_middle_vertices():
    """K_{3,4}: a pair within one side has its shortest paths over the vertices of the other
    side that minimise the two latencies, 1 / sigma of its weight through each; a pair across
    takes its edge."""
    g = graph("biclique3_4")
    lat = {}
    for e in range(g.m):
        lat[(int(g.src[e]), int(g.dst[e]))] = lat[(int(g.dst[e]), int(g.src[e]))] = float(g.latency[e])
    side = lambda v: v < 3
    want = [Fraction(0)] * g.n
    tied = 0
    for s in range(g.n):
        for t in range(g.n):
            if s == t or side(s) != side(t):
                continue
            mid = [x for x in range(g.n) if side(x) != side(s)]
            best = min(lat[(s, x)] + lat[(x, t)] for x in mid)
            via = [x for x in mid if lat[(s, x)] + lat[(x, t)] == best]
            tied += len(via) > 1
            for x in via:
                want[x] += Fraction(1, len(via))
    assert tied >= 6
    S = np.arange(g.n, dtype=np.int32)
    x = ref("biclique3_4").rows(S, S, exact=True)
    noloop = g.n - len(np.unique(g.src[g.src == g.dst]))
    assert x[1] == want and x[2] == noloop > 0 and x[3] == {er.ENOEDGE}
    f = ref("biclique3_4").rows(S, S)
    assert er.close(f[1], want, ref("biclique3_4").tol(S))


# ---- the state layout --------------------------------------------------------------------------

def test_layout_mirror_matches_header(tmp_path):
    """tests/ecmp_ref.py's layout_total / fits_lds (which the GPU tests size their graphs by)
    against shadow_amd/csrc/ecmp_layout.hpp, read by tests/ecmp_layout_main.cpp: built with
    -fsanitize=address,undefined and run as its own process, which also writes every section
    of every layout end to end."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover", *extra]
        if subprocess.run([cxx, *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("g++ lacks the sanitizer runtime")
    exe = tmp_path / "ecmp_layout"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "ecmp_layout_main.cpp")], check=True)
    nmax = er.lds_max_n()
    ns = [1, 2, 7, 63, nmax - 1, nmax, nmax + 1, 65535, 65536, 66000]
    r = subprocess.run([str(exe), *map(str, ns)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert lines[0] == (er.LDS_BUDGET, er.SMALL)
    assert lines[1:] == [(n, er.layout_total(n, 2), er.layout_total(n, 4), int(er.fits_lds(n))) for n in ns]
    assert er.fits_lds(nmax) and not er.fits_lds(nmax + 1) and 4700 < nmax < 4900
