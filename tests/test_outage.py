"""CPU: the reference of the link outage calls (tests/outage_ref.py) -- the definition (a fresh
reference of every reduced graph) against the kernel's programme (mark, seed, sweeps), bit for
bit, on every graph and scenario set the GPU tests use; the coverage conditions those sets must
meet, so that no GPU test passes vacuously; the mutants the tests must see --; the interface
through every layer; and the state layout and unit arithmetic
(shadow_amd/csrc/outage_layout.hpp) through a stand-alone program under the host sanitizers."""
import ctypes
import dataclasses
import functools
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import frac_graphs as fgr
from tests import multi_graphs as mg
from tests import outage_ref as orf
from tests import shape_graphs as sg
from tests import test_hops_gpu as hg
from tests import test_loss as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_outage_async", "shd_route_outage", "shd_route_pair_outage")
TOPO_SYMS = ("shd_topology_link_outage",)
# the small builders of tests/test_loss.py that do not dispatch
SMALL = [n for n in tl.GRAPHS if n not in ("ba80_prefer", "k24", "count_complete")]
# and the larger ones of the GPU tests: the lattice with tied detours, a multigraph, the directed
# lattice, a directed multigraph, fractional latencies with f64 ties and one-ulp near misses, the
# lollipop, a BA graph and second self-loops; dir_path9 is the path 0 -> 1 -> ... -> 8 as a directed
# graph, where no vertex reaches a lower one
LARGE = ["grid", "multi389", "dir_grid", "multi389_dir", "frac_multi", "frac_cents", "frac_hub", "lollipop",
         "sized1000", "loops_only"]
# the references' alone: shd_route_create refuses a graph that is not (strongly) connected, so an
# entry that is unreachable in the whole graph reaches no kernel
CPU_ONLY = ["dir_path9"]
HBM16 = f"sized{orf.lds_max_n() + 1}"      # one vertex past the LDS limit
CASES = SMALL + LARGE + [HBM16] + CPU_ONLY


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in sg.SUITE:
        return sg.get(name)
    if name.startswith("sized"):
        return sg.sized(int(name[5:]))
    if name in mg.SUITE:
        return mg.get(name)
    if name in fgr.SUITE:
        return fgr.get(name)
    if name == "ring66k":
        return hg._graph(name)[0]
    if name == "dir_path9":
        return dataclasses.replace(sg.tiny(9, "some"), directed=True, name=name)
    return tl.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return orf.OutageRef(graph(name))


def sources(name):
    n = graph(name).n
    if name in SMALL:
        return tl.sources(name)
    return np.unique(np.linspace(0, n - 1, 4).astype(np.int32))


def targets(name):
    """Every vertex of a small builder, else about 150 spread over the graph and the sources."""
    n = graph(name).n
    if n <= 400:
        return np.arange(n, dtype=np.int32)
    return np.unique(np.concatenate([np.arange(0, n, max(1, n // 150)), sources(name)])).astype(np.int32)


def weights(name, ns, nt):
    return tl.weights(name, ns, nt, 21)


@functools.lru_cache(maxsize=None)
def scenarios(name):
    """The scenario lists of a case, from the tree of its first source: none, an empty one, tree
    edges near and far, a non-tree edge, two nested tree edges given descending, a tree edge with
    the other edges into its head, the lowest self-loop alone and with the vertex's others, a
    vertex outage and a random set with a repeat."""
    g, R, S = graph(name), ref(name), sources(name)
    out = [[]]
    if g.m == 0:
        return out
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    s0 = int(S[0])
    d, pe, pu, hops, order = R._tree(s0)
    loops = {e for ls in R.loops for e in ls}
    tree = [int(pe[v]) for v in order]
    nontree = sorted(set(range(g.m)) - set(tree) - loops)
    if tree:
        out += [[tree[0]], [tree[-1]], [tree[len(tree) // 2]]]
        es = R.ref.path(s0, order[-1])[1]
        if len(es) >= 2:
            out.append([es[-1], es[0]])
        v = order[len(order) // 3]
        out.append(sorted({int(pe[v])} | {e for _, e, _ in R.inarcs[v]}, reverse=True)[:4] + [int(pe[v])])
        v = order[0]
        out.append([e for e in range(g.m) if v in (int(g.src[e]), int(g.dst[e]))])
    if nontree:
        out.append([nontree[0]])
        out.append([int(x) for x in rng.choice(nontree, size=min(3, len(nontree)), replace=False)])
    for s in S.tolist():
        if R.loops[s]:
            out += [[R.loops[s][0]], list(reversed(R.loops[s]))]
            break
    for s in S.tolist():
        if len(R.loops[s]) > 1:
            out += [[R.loops[s][0]], list(R.loops[s])]
            break
    pick = [int(x) for x in rng.integers(0, g.m, size=min(6, g.m))]
    out.append(pick + pick[:1])
    return out


@functools.lru_cache(maxsize=None)
def entries(name):
    S, T = sources(name), targets(name)
    W = weights(name, len(S), len(T))
    return S, T, W


@functools.lru_cache(maxsize=None)
def repaired(name):
    S, T, W = entries(name)
    return ref(name).repair(*orf.block_entries(S, T, W), scenarios(name))


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
    for name in ("outage", "pair_outage", "outage_async"):
        assert callable(getattr(route.RouteEngine, name))
    assert callable(topology.Topology.link_outage)
    h = re.sub(r"\s+", " ", text["shd_route.h"])
    assert ("int shd_route_outage_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, "
            "int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt, const int64_t* d_scn_off, "
            "const int32_t* d_scn_edge, int32_t nscn, uint64_t* d_stats, double* d_max_add, double* d_lat, "
            "uint64_t* d_unrouted, void* stream);") in h
    assert ("int shd_route_outage(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, "
            "uint32_t flags, const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge, int32_t nscn, "
            "uint64_t* stats_out, double* max_add_out, double* lat_out, uint64_t* unrouted_out);") in h
    assert ("int shd_route_pair_outage(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, "
            "const uint64_t* pair_wt, int64_t npairs, uint32_t flags, const int64_t* scn_off, "
            "const int32_t* scn_edge, int32_t nscn, uint64_t* stats_out, double* max_add_out, double* lat_out, "
            "uint64_t* unrouted_out);") in h
    for k, v in (("HIT", 0), ("CUT", 1), ("SLOWER", 2), ("NSTAT", 3)):
        assert f"#define SHD_ROUTE_OUTAGE_{k} {v}" in text["shd_route.h"]
        assert getattr(route, f"OUTAGE_{k}") == v == getattr(orf, k)
    assert "SHD_ROUTE_OUTAGE_LDS=0" in h and "vertex outage" in h
    assert (route.ENOEDGE, route.EUNREACH) == (orf.ENOEDGE, orf.EUNREACH)
    t = re.sub(r"\s+", " ", text["shd_topology.h"])
    assert ("int shd_topology_link_outage(shd_topology_t* top, const int64_t* scn_off, const int32_t* scn_edge, "
            "int32_t nscn, uint64_t* stats, double* max_add, uint64_t* unrouted);") in t


# ---- the two references ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_fresh_equals_repair(name):
    """The definition and the kernel's programme agree bit for bit: stats, max_add, every new
    latency (NaNs matched), unrouted and the codes."""
    S, T, W = entries(name)
    R = ref(name)
    a = R.fresh(*orf.block_entries(S, T, W), scenarios(name))
    b = repaired(name)
    assert a.same(b), (name, a.stats.tolist(), b.stats.tolist())
    assert a.stats.dtype == np.uint64 and a.lat.shape == (len(scenarios(name)), len(S) * len(T))
    # an empty scenario: zeros and the old rows
    assert not a.stats[0].any() and a.max_add[0] == 0.0
    old = np.array([R.old(s, t)[0] for s, t in zip(*orf.block_entries(S, T)[:2])])
    assert np.array_equal(a.lat[0], old, equal_nan=True)


@functools.lru_cache(maxsize=None)
def sweep_case():
    """(sources, targets, the programme's result) of the full N-1 sweep of vertex 0 of sized1000."""
    g = graph("sized1000")
    S, T = np.array([0], np.int32), np.arange(g.n, dtype=np.int32)
    return S, T, ref("sized1000").repair(*orf.block_entries(S, T), [[e] for e in range(g.m)])


def test_special_sets_agree():
    """The sets of the GPU tests that are not the generic ones: the full N-1 sweep of one source
    of sized1000 (the definition on every 20th scenario and on the 40 largest subtrees), and
    ring66k with one failed edge near the antipode of the source."""
    name = "sized1000"
    g, R = graph(name), ref(name)
    S, T, _ = orf.block_entries([0], np.arange(g.n))
    scn = [[e] for e in range(g.m)]
    rep = sweep_case()[2]
    size = [len(R.affected(0, f)) for f in scn]
    pick = sorted(set(range(0, g.m, 20)) | set(np.argsort(size)[-40:].tolist()))
    fr = R.fresh(S, T, None, [scn[k] for k in pick])
    assert np.array_equal(fr.stats, rep.stats[pick]) and np.array_equal(fr.max_add, rep.max_add[pick])
    assert np.array_equal(fr.lat, rep.lat[pick], equal_nan=True)
    live = np.flatnonzero(rep.stats[:, orf.HIT])
    assert 900 <= len(live) <= g.n and g.m > 2900 and orf.units(1, g.m)[1] >= 3    # several slabs
    s, e, ts = ring_case()
    R = ref("ring66k")
    A = R.affected(s, [e])
    assert 1 <= len(A) <= 16
    a, b = R.fresh([s] * len(ts), ts, None, [[e]]), R.repair([s] * len(ts), ts, None, [[e]])
    assert a.same(b) and a.stats[0, orf.HIT] >= 1


@functools.lru_cache(maxsize=None)
def ring_case():
    """(source, failed edge, targets) on ring66k: the parent edge of a vertex whose subtree has at
    most 16 vertices, 16 hops above one of the deepest vertices of the source's tree."""
    R = ref("ring66k")
    s = 5
    d, pe, pu, hops, order = R._tree(s)
    v = order[-1]
    best = None
    for _ in range(16):
        if len(R.affected(s, [int(pe[v])])) <= 16:
            best = v
        v = int(pu[v])
        if v == s:
            break
    assert best is not None
    A = R.affected(s, [int(pe[best])])
    ts = sorted(set(A) | {s, 0, 33000, 65999, int(pu[best])})
    return s, int(pe[best]), ts


def test_coverage_conditions():
    """What the scenario sets must contain, asserted on the reference's results here so that a
    GPU test that equals the reference has seen each."""
    seen, hit0, tied, slower, cut = set(), [], [], [], []
    for name in CASES:
        r = repaired(name)
        seen |= ref(name).seen
        st = r.stats.astype(np.int64)
        for k in range(1, len(st)):
            if st[k, orf.HIT] == 0:
                hit0.append(name)
            elif st[k, orf.SLOWER] == 0 and st[k, orf.CUT] == 0:
                tied.append(name)
            if st[k, orf.SLOWER]:
                slower.append(name)
                assert r.max_add[k] > 0
            else:
                assert r.max_add[k] == 0
            if st[k, orf.CUT]:
                cut.append(name)
    assert hit0 and "grid" in tied and "sized1000" in slower and "sized63" in slower
    assert "lollipop" in cut and "lollipop8_20" in cut
    assert {"nested_roots", "nontree_skip", "loop_alone", "loop_with_second", "many_sweeps"} <= seen, seen
    # fractional latencies, a multigraph, a directed graph and unreachable vertices are among them
    assert not float(graph("frac_multi").latency[0]).is_integer() and graph("dir_grid").directed
    assert orf.EUNREACH in repaired("dir_path9").codes and orf.ENOEDGE in repaired("tiny3_none").codes
    assert repaired("dir_path9").unrouted > 0 and repaired("dir_path9").stats[:, orf.CUT].any()


@pytest.mark.parametrize("mutant", orf.MUTANTS)
def test_mutants_are_seen(mutant):
    """Each wrong variant of the programme changes an asserted output on some case."""
    seen = []
    for name in CASES:
        S, T, W = entries(name)
        bad = ref(name).repair(*orf.block_entries(S, T, W), scenarios(name), mutant=mutant)
        if not bad.same(repaired(name)):
            seen.append(name)
    assert seen, mutant
    print(mutant, seen)


# ---- the state layout and the units ----------------------------------------------------------------

UNIT_CASES = [(1, 0), (1, 1), (1, 3000), (1, 1024), (1, 1025), (1024, 1), (1024, 256), (5000, 1), (7, 100000),
              (3, 1023), (2048, 4096)]


def test_layout_mirror_matches_header(tmp_path):
    """tests/outage_ref.py's layout, state form and unit arithmetic (which the GPU tests size
    their graphs and scenario counts by) against shadow_amd/csrc/outage_layout.hpp and
    path_host.hpp's state_form, read by tests/outage_layout_main.cpp: built with
    -fsanitize=address,undefined and run as its own process, which also writes every section of
    every layout end to end and walks every unit of every unit case."""
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
    exe = tmp_path / "outage_layout"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "outage_layout_main.cpp")], check=True)
    nmax = orf.lds_max_n()
    ns = [1, 2, 7, 8, 9, 65535, 65536, nmax, nmax + 1]
    args = [str(n) for n in ns] + ["units"] + [f"{k}x{q}" for k, q in UNIT_CASES]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert lines[0] == (orf.LDS_BUDGET, orf.SMALL, orf.SLAB_MAX, orf.UNITS)
    assert len(lines) == 1 + len(ns) + len(UNIT_CASES)
    budget = 1 << 28
    for n, ln in zip(ns, lines[1:]):
        want = (n, *orf.layout_offsets(n, 2), *orf.layout_offsets(n, 4), int(orf.fits_lds(n)))
        assert ln[:len(want)] == want
        forms = ln[len(want):]
        # state_form with the knob unset and set, 1,000 units: (form, grid, lds, stride, slots) each
        assert forms[:5] == orf.state_form(n, 1000, False, budget)
        assert forms[5:] == orf.state_form(n, 1000, True, budget)
        for tsize, (dn, lvl, order, aff, mark, total) in ((2, ln[1:7]), (4, ln[7:13])):
            assert all(x % 16 == 0 for x in (dn, lvl, order, aff, mark, total))
            assert dn + 8 * n <= lvl and lvl + 4 * (n + 1) <= order and order + tsize * n <= aff
            assert aff + tsize * n <= mark and mark + n <= total == orf.layout_total(n, tsize)
            assert total <= (13 + 2 * tsize) * n + 4 + 5 * 15
    # both sides of the LDS limit and of 65,535 vertices
    assert orf.fits_lds(nmax) and not orf.fits_lds(nmax + 1)
    assert orf.state_form(nmax, 9, False, budget)[0] == 1 and orf.state_form(nmax + 1, 9, False, budget)[0] == 2
    assert orf.state_form(65535, 9, False, budget)[0] == 2 and orf.state_form(65536, 9, False, budget)[0] == 3
    assert orf.state_form(65536, 9, False, budget)[1] == 9 and orf.state_form(65536, 1000, False, 0)[1] == 16
    text = open(os.path.join(ROOT, "shadow_amd", "csrc", "outage_layout.hpp")).read()
    assert f"n <= {nmax}" in text
    assert f"{nmax:,} vertices" in open(os.path.join(ROOT, "include", "shd_route.h")).read()
    # the units: every scenario of every source in exactly one unit, no slab above the limit
    for (k, q), ln in zip(UNIT_CASES, lines[1 + len(ns):]):
        assert ln == (k, q, *orf.units(k, q), 1)
        slab, nslab, nu = orf.units(k, q)
        assert 1 <= slab <= orf.SLAB_MAX and nu == k * nslab and (nslab - 1) * slab < max(q, 1) <= nslab * slab
    assert orf.units(1, 3000) == (3, 1000, 1000) and orf.units(1024, 256) == (256, 1, 1024)
    assert orf.units(5000, 1) == (1, 1, 5000) and orf.units(7, 100000)[0] == 681
