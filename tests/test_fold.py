"""CPU: the reference of the path folds (tests/fold_ref.py) against Ref.rows -- SUM of the
latencies is lat, PROD of 1 - loss is rel, SUM of ones the hop count --; the interface through
every layer; the state layout of the sweep (shadow_amd/csrc/fold_layout.hpp) through a
stand-alone program under the host sanitizers; and the loader's jitter column."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import fold_ref as fr
from tests import shape_graphs as sg
from tests import test_ecmp as te
from tests import test_hops_gpu as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_fold_async", "shd_route_fold", "shd_route_pair_fold")
TOPO_SYMS = ("shd_topology_edge_jitter", "shd_topology_fold_pairs")
GRAPHS = te.GRAPHS + ["ba60_multi", "ba60", "ba80_prefer", "dir40", "ba90_frac", "k24"]


@functools.lru_cache(maxsize=None)
def graph(name):
    return hg._graph(name)[0] if name == "ba60_multi" else te.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return fr.FoldRef(graph(name))


# ---- the interface -------------------------------------------------------------------------------

def test_declarations():
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
    for name in ("fold", "pair_fold", "fold_async"):
        assert callable(getattr(route.RouteEngine, name))
    assert callable(topology.Topology.edge_jitter) and callable(topology.Topology.fold_pairs)
    assert (route.FOLD_SUM, route.FOLD_MIN, route.FOLD_MAX, route.FOLD_PROD) == (fr.SUM, fr.MIN, fr.MAX, fr.PROD)
    h = re.sub(r"\s+", " ", text["shd_route.h"])
    for name, value in (("SUM", 0), ("MIN", 1), ("MAX", 2), ("PROD", 3), ("MAX_N", 8)):
        assert re.search(rf"#define SHD_ROUTE_FOLD_{name} {value}\b", h), name
    assert route.FOLD_MAX_N == 8
    assert ("int shd_route_fold_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, "
            "int32_t nt, int64_t ld, uint32_t flags, const int32_t* ops, int32_t nf, const double* d_val, "
            "double* d_out, int64_t plane, void* stream);") in h
    assert ("int shd_route_fold(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, "
            "uint32_t flags, const int32_t* ops, int32_t nf, const double* val, double* out);") in h
    assert ("int shd_route_pair_fold(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, "
            "int64_t npairs, uint32_t flags, const int32_t* ops, int32_t nf, const double* val, double* out);") in h
    t = re.sub(r"\s+", " ", text["shd_topology.h"])
    assert "int shd_topology_edge_jitter(shd_topology_t* top, double* out);" in t
    assert ("int shd_topology_fold_pairs(shd_topology_t* top, int32_t op, const double* edge_val, const int32_t* src, "
            "const int32_t* dst, int64_t npairs, double* out);") in t
    assert "double* edge_jitter; } shd_graphml_t;" in t          # the last field
    assert topology._GraphML._fields_[-1][0] == "edge_jitter"


# ---- the reference against Ref.rows --------------------------------------------------------------

def test_fold_one():
    inf = float("inf")
    assert fr.fold_one(fr.SUM, []) == 0.0 and fr.fold_one(fr.PROD, []) == 1.0
    assert fr.fold_one(fr.MIN, []) == inf and fr.fold_one(fr.MAX, []) == -inf
    assert fr.fold_one(fr.SUM, [0.1, 0.2, 0.3]) == (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    assert fr.fold_one(fr.PROD, [0.1, 0.2, 0.3]) == (0.1 * 0.2) * 0.3
    assert fr.fold_one(fr.MIN, [3.0, -inf, 2.0]) == -inf and fr.fold_one(fr.MAX, [3.0, inf, 2.0]) == inf
    assert fr.fold_one(fr.PROD, [2.0, -inf, 3.0]) == -inf


@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_identities_against_rows(name, dispatch):
    """All sources x all vertices: SUM of the latencies is lat, SUM of ones the hop count, PROD
    of 1 - loss is rel on graphs without vertex loss; failed entries are NaN with their codes."""
    g, R = graph(name), ref(name)
    S = te.sources(name) if name in te.GRAPHS else np.arange(g.n, dtype=np.int32)
    T = np.arange(g.n, dtype=np.int32)
    lat, rel, hops = R.ref.rows(S, T, dispatch)
    ones = np.ones(g.m)
    erel = 1.0 - np.asarray(g.packetloss, np.float64)
    out, codes = R.rows(S, T, [fr.SUM, fr.SUM, fr.PROD], [g.latency, ones, erel], dispatch)
    assert out.shape == (3, len(S), g.n)
    assert fr.same(out[0], lat)
    assert fr.same(out[1], np.where(hops < 0, np.nan, hops.astype(np.float64)))
    if fr.no_vertex_loss(g):
        assert fr.same(out[2], rel)
    failed = np.isnan(lat)
    assert np.array_equal(np.isnan(out[0]), failed) and np.array_equal(np.isnan(out[2]), failed)
    assert bool(codes) == bool(failed.any()) and codes <= {fr.ENOEDGE, fr.EUNREACH}
    if g.n > 3:
        assert np.count_nonzero(~failed) > g.n


def test_some_graph_has_no_vertex_loss():
    assert sum(fr.no_vertex_loss(graph(n)) for n in GRAPHS) >= len(GRAPHS) - 2
    assert sum(graph(n).vertex_packetloss is None for n in GRAPHS) >= 6
    assert any(graph(n).directed for n in GRAPHS) and graph("k24").n == 24


def test_pairs_are_the_rows_entries():
    g, R = graph("ba64_ties"), ref("ba64_ties")
    cols = fr.columns(g, 1)
    S, T = [3, 9, 40], list(range(g.n))
    rows, _ = R.rows(S, T, fr.ALL_OPS, cols)
    k = np.random.default_rng(0).permutation(len(S) * len(T))
    ps, pt = np.repeat(S, len(T))[k], np.tile(T, len(S))[k]
    pairs, _ = R.pairs(ps, pt, fr.ALL_OPS, cols)
    assert fr.same(pairs, rows.reshape(4, -1)[:, k])
    assert np.isinf(cols[3]).sum() >= 2 and not np.isnan(cols).any()


# ---- the state layout ----------------------------------------------------------------------------

def test_layout_mirror_matches_header(tmp_path):
    """tests/fold_ref.py's layout arithmetic (which the GPU tests size their graphs by) against
    shadow_amd/csrc/fold_layout.hpp, read by tests/fold_layout_main.cpp: built with
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
    exe = tmp_path / "fold_layout"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "fold_layout_main.cpp")], check=True)
    nmax = fr.lds_max_n()
    ns = [1, 2, 7, 8, 9, 65535, 65536, nmax, nmax + 1]
    r = subprocess.run([str(exe), *map(str, ns)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert lines[0] == (fr.LDS_BUDGET, fr.SMALL)
    assert len(lines) == 1 + len(ns)
    for n, ln in zip(ns, lines[1:]):
        assert ln == (n, *fr.layout_offsets(n, 2), *fr.layout_offsets(n, 4), int(fr.fits_lds(n)))
        for tsize, (val, lvl, order, total) in ((2, ln[1:5]), (4, ln[5:9])):
            assert val % 16 == lvl % 16 == order % 16 == total % 16 == 0              # aligned
            assert val + 8 * n <= lvl and lvl + 4 * (n + 1) <= order and order + tsize * n <= total  # disjoint
            assert total == fr.layout_total(n, tsize)
    # the limit: the state of nmax vertices is the last that fits beside the small header
    assert fr.fits_lds(nmax) and not fr.fits_lds(nmax + 1) and 11600 < nmax < 11800
    assert fr.SMALL + fr.layout_total(nmax) <= fr.LDS_BUDGET < fr.SMALL + fr.layout_total(nmax + 1)


# ---- the loader's jitter column -------------------------------------------------------------------

_KEYS = """<key attr.name="packetloss" attr.type="double" for="edge" id="el" />
  <key attr.name="latency" attr.type="double" for="edge" id="lt" />
  <key attr.name="bandwidthup" attr.type="int" for="node" id="bu" />
  <key attr.name="bandwidthdown" attr.type="int" for="node" id="bd" />"""
_JKEY = """<key attr.name="jitter" attr.type="double" for="edge" id="jt">%s</key>"""
# six edges in document order: (source, target, jitter or None)
_EDGES = [("a", "b", "0.5"), ("b", "c", None), ("c", "a", "2.25"), ("a", "a", "0"), ("c", "d", None), ("d", "b", "7")]


def _graphml(tmp_path, jkey, edges=_EDGES, name="j.xml"):
    nodes = "".join(f'<node id="{v}"><data key="bu">100</data><data key="bd">100</data></node>' for v in "abcd")
    es = "".join(f'<edge source="{a}" target="{b}"><data key="lt">{3 + i}.0</data><data key="el">0.0</data>'
                 + (f'<data key="jt">{j}</data>' if j is not None and jkey else "") + "</edge>"
                 for i, (a, b, j) in enumerate(edges))
    p = tmp_path / name
    p.write_text(f'<graphml xmlns="http://graphml.graphdrawing.org/xmlns">\n  {_KEYS}\n  {jkey}\n'
                 f'  <graph edgedefault="undirected">{nodes}{es}</graph>\n</graphml>')
    return str(p)


def _load(topology, path):
    L = topology.load_library()
    out = topology._GraphML()
    err = ctypes.create_string_buffer(512)
    rc = L.shd_graphml_load(path.encode(), ctypes.byref(out), err, 512)
    assert rc == 0, err.value
    try:
        m = out.graph.n_edges
        return m, (None if not out.edge_jitter else [out.edge_jitter[e] for e in range(m)])
    finally:
        L.shd_graphml_free(ctypes.byref(out))
        assert not out.edge_jitter


def test_loader_hands_the_jitter_over(tmp_path):
    """No device: edge_jitter in document order, the key's default where an edge has no value,
    NaN there without a default, a NULL pointer without the key; a negative jitter is refused."""
    from shadow_amd import build, topology
    build.build()
    m, j = _load(topology, _graphml(tmp_path, _JKEY % "<default>1.5</default>"))
    assert m == 6 and j == [0.5, 1.5, 2.25, 0.0, 1.5, 7.0]
    m, j = _load(topology, _graphml(tmp_path, _JKEY % "", name="nodefault.xml"))
    assert m == 6 and j[0] == 0.5 and j[2:4] == [2.25, 0.0] and j[5] == 7.0 and np.isnan(j[1]) and np.isnan(j[4])
    m, j = _load(topology, _graphml(tmp_path, "", name="nokey.xml"))
    assert m == 6 and j is None
    bad = [e if i != 2 else (e[0], e[1], "-0.125") for i, e in enumerate(_EDGES)]
    with pytest.raises(ValueError, match="jitter negative"):
        topology.load_graphml(_graphml(tmp_path, _JKEY % "", edges=bad, name="neg.xml"))
    g = topology.load_graphml(_graphml(tmp_path, _JKEY % ""))          # the graph itself is unchanged by the key
    assert g.n == 4 and g.m == 6 and g.latency.tolist() == [3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
