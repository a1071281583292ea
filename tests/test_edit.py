"""CPU: the reference of the link edit calls (tests/edit_ref.py) -- the definition (a fresh
reference of every edited graph) against the kernel's programme (live test, mark, seed, sweeps,
rounds over the new arcs and the frontier), bit for bit, on every graph and scenario set the GPU
tests use; the coverage conditions those sets must meet, so that no GPU test passes vacuously; the
mutants the tests must see; the interface through every layer; and the host stages
(shadow_amd/csrc/edit_host.hpp, edit_layout.hpp) through a stand-alone program under the host
sanitizers."""
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import edit_ref as er
from tests import reprice_ref as rr
from tests import test_outage as tout
from tests import test_reprice as trp

INF = math.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_edit_async", "shd_route_edit", "shd_route_pair_edit")
TOPO_SYMS = ("shd_topology_link_edit",)
SMALL = tout.SMALL
MINE = ["path65", "lolli20", "dring12", "star1100"]
LARGE = ["grid", "multi389", "dir_grid", "frac_multi", "frac_cents", "frac_hub", "lollipop", "sized1000", "loops_only",
         "hub1100", "layers48"] + MINE
FRAC = ["frac_multi", "frac_cents", "frac_hub"]
HBM16 = f"sized{er.lds_max_n() + 1}"       # one vertex past the LDS limit
CPU_ONLY = ["dpath9"]                      # not strongly connected: no context takes it
GPU_CASES = SMALL + LARGE + [HBM16]
CASES = GPU_CASES + CPU_ONLY


@functools.lru_cache(maxsize=None)
def graph(name):
    return er.BUILDERS[name]() if name in er.BUILDERS else trp.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return er.EditRef(graph(name))


def sources(name):
    own = {"path65": [0, 40, 64], "lolli20": [0, 12, 19], "dring12": [0, 6, 9], "star1100": [3, 0], "dpath9": [0, 4, 8]}
    return np.array(own[name], np.int32) if name in own else trp.sources(name)


def targets(name):
    n = graph(name).n
    if n <= 400:
        return np.arange(n, dtype=np.int32)
    return np.unique(np.concatenate([np.arange(0, n, max(1, n // 150)), sources(name)])).astype(np.int32)


weights = trp.weights


@functools.lru_cache(maxsize=None)
def entries(name):
    S, T = sources(name), targets(name)
    return S, T, weights(name, len(S), len(T))


def find_ulp(name):
    """(s0, v, d[v]) of the deepest vertex of the first source's tree that is among the targets, at
    least two hops down; None without one."""
    R = ref(name)
    s0 = int(sources(name)[0])
    d, pe, pu, hops, order = R.base._tree(s0)
    T = set(targets(name).tolist())
    deep = [v for v in order if v in T and hops[v] >= 2]
    return (s0, int(deep[-1]), float(d[deep[-1]])) if deep else None


def _special(name, g):
    m = g.m
    if name == "path65":
        return [[(0, 32, 1.0)], [(0, 2, 2.0)], [(0, 32, 5.0), (0, 32, 1.0)], [(0, 32, 1.0), (33, 64, 1.0)], [(31, INF)],
                [(31, INF), (0, 40, 3.0)], [(10, 50, 1.0), (31, INF)], [(40, 2.5), (20, 60, 1.0), (5, INF)]]
    if name == "lolli20":
        return [[(19, INF)], [(2, 15, 1.5), (19, INF)], [(19, INF), (0, 19, 1.0)], [(0, 19, 1.0)],
                [(19, INF), (3, 12, 0.5), (15, 3.0)], [(28, INF)], [(16, 0.25), (0, 6, 0.5)]]
    if name == "dring12":
        return [[(0, 6, 1.0)], [(6, 0, 1.0)], [(3, INF), (2, 5, 1.0)], [(3, INF), (3, 4, 2.5)], [(3, 0.5), (9, 2, 0.25)]]
    if name == "star1100":
        ring = [(v, v % 1100 + 1, 1.0) for v in range(1, 1101)]
        return [ring, [(5, 700, 0.5)], ring[:600] + [(2, INF), (9, 30.0)] + ring[600:], [(2, INF)], [(2, INF), (3, 700, 4.0)]]
    if name == "dpath9":
        return [[(8, 0, 1.0)], [(3, INF)], [(3, INF), (2, 5, 1.0)], [(0, 4, 1.0)]]
    if name == "hub1100":
        return [[(0, 1, 5.0)], [(0, INF), (0, 1, 5.0)], [(0, INF)], [(1101, INF), (0, INF)], [(0, INF), (0, 500, 2.0)],
                [(1101, 5.0), (7, 900, 0.5)]]
    if name == "layers48":
        return [[(0, 1, 1.0)], [(m - 1, INF), (0, 1, 1.0)], [(0, INF), (0, 150, 3.0)]]
    return None


@functools.lru_cache(maxsize=None)
def scenarios(name):
    """The scenario lists of a case: an empty one, then what the builder is there for, or from
    the tree of the first source: new links to the deepest vertex at half, twice and exactly its
    distance, two parallel ones with the dearer first, tree edges removed near and far, a tree edge
    removed and a new link that rejoins what it cut, a mixed set of a raise, a removal and a new
    link given out of order, the lowest self-loop removed alone, with the vertex's others and with
    the second one repriced, a random mix, and on the fractional builders a new link one ulp
    better and one ulp worse than the distance it rivals."""
    g, R, S = graph(name), ref(name), sources(name)
    out = [[]]
    sp = _special(name, g)
    if sp is not None:
        return [[tuple(it) for it in f] for f in out + sp]
    if g.m == 0:
        return out + ([[(0, g.n - 1, 1.0)]] if g.n >= 2 else [])
    if g.n < 2:                                             # no room for a link: the self-loops alone
        ls = ref(name).loops[0]
        return out + ([[(ls[0], INF)], [(ls[0], 2.5)], [(e, INF) for e in ls]] if ls else [])
    lat = R.lat
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 13)
    s0 = int(S[0])
    d, pe, pu, hops, order = R.base._tree(s0)
    loops = {e for ls in R.loops for e in ls}
    tree = [int(pe[v]) for v in order]
    nontree = sorted(set(range(g.m)) - set(tree) - loops)
    if name == HBM16:                                       # a Python Dijkstra per scenario and source: a few
        far = int(order[-1])
        return out + [[(s0, far, float(d[far] / 2))], [(tree[len(tree) // 2], INF), (s0, far, float(d[far] / 4))],
                      [(tree[0], INF)]]
    if order:
        far, mid = int(order[-1]), int(order[len(order) // 2])
        df = float(d[far])
        out += [[(s0, far, df / 2)], [(s0, far, df * 2)], [(s0, mid, float(d[mid]))], [(s0, far, df / 2 + 1), (s0, far, df / 2)]]
        out += [[(tree[0], INF)], [(tree[-1], INF)], [(int(pe[far]), INF), (s0, far, df * 3)]]
        a = tree[len(tree) // 2]
        u, v = (int(x) for x in rng.choice(g.n, size=2, replace=False))
        out.append([(a, INF), (u, v, float(lat[a] / 2))])
        mixed = [(tree[0], float(lat[tree[0]] * 2)), (far, s0, df / 3)]
        if nontree:
            mixed.append((nontree[0], INF))
            out.append([(nontree[0], INF)])
        out.append(mixed[::-1] if len(mixed) < 3 else [mixed[2], mixed[1], mixed[0]])
    for s in S.tolist():
        if R.loops[s]:
            e = R.loops[s][0]
            out += [[(e, INF)], [(x, INF) for x in reversed(R.loops[s])], [(e, INF), (s, (s + 1) % g.n, 1.0)]]
            break
    for s in S.tolist():
        if len(R.loops[s]) > 1:
            out += [[(R.loops[s][0], INF)], [(R.loops[s][1], 7.0), (R.loops[s][0], INF)]]
            break
    pick = sorted(set(int(x) for x in rng.integers(0, g.m, size=min(5, g.m))), reverse=True)
    mix = [(e, (INF, float(lat[e] * 2), float(lat[e] / 2), INF, float(lat[e]))[i]) for i, e in enumerate(pick)]
    for _ in range(2):
        u, v = (int(x) for x in rng.choice(g.n, size=2, replace=False))
        mix.insert(1, (u, v, float(np.median(lat))))
    out.append(mix)
    if name in FRAC and find_ulp(name):
        s, v, dv = find_ulp(name)
        out += [[(s, v, float(np.nextafter(dv, 0.0)))], [(s, v, float(np.nextafter(dv, np.inf)))]]
    return [[tuple(it) for it in f] for f in out]


@functools.lru_cache(maxsize=None)
def programmed(name):
    S, T, W = entries(name)
    r = ref(name).programme(*er.block_entries(S, T, W), scenarios(name))
    r.log = list(ref(name).log)                           # the records of this call
    return r


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
    for name in ("edit", "pair_edit", "edit_async"):
        assert callable(getattr(route.RouteEngine, name))
    assert callable(topology.Topology.link_edit) and callable(route.pack_edits)
    h = re.sub(r"\s+", " ", text["shd_route.h"])
    assert ("int shd_route_edit_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, "
            "int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt, const int64_t* d_scn_off, "
            "const int32_t* d_scn_edge, const int32_t* d_scn_a, const int32_t* d_scn_b, const double* d_scn_lat, "
            "int32_t nscn, uint64_t* d_stats, double* d_max_add, double* d_max_gain, double* d_min_new, double* d_lat, "
            "uint64_t* d_unrouted, void* stream);") in h
    assert ("int shd_route_edit(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, "
            "uint32_t flags, const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge, "
            "const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, int32_t nscn, uint64_t* stats_out, "
            "double* max_add_out, double* max_gain_out, double* min_new_out, double* lat_out, "
            "uint64_t* unrouted_out);") in h
    assert ("int shd_route_pair_edit(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, "
            "const uint64_t* pair_wt, int64_t npairs, uint32_t flags, const int64_t* scn_off, "
            "const int32_t* scn_edge, const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, "
            "int32_t nscn, uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out, "
            "double* lat_out, uint64_t* unrouted_out);") in h
    for k, v in (("HIT", 0), ("CUT", 1), ("SLOWER", 2), ("FASTER", 3), ("NSTAT", 4)):
        assert f"#define SHD_ROUTE_EDIT_{k} {v}" in text["shd_route.h"]
        assert getattr(route, f"EDIT_{k}") == v == getattr(er, k)
    assert "SHD_ROUTE_EDIT_LDS=0" in h and "This is a limit" in h and "stays out of scope" in h
    t = re.sub(r"\s+", " ", text["shd_topology.h"])
    assert ("int shd_topology_link_edit(shd_topology_t* top, const int64_t* scn_off, const int32_t* scn_edge, "
            "const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, int32_t nscn, uint64_t* stats, "
            "double* max_add, double* max_gain, double* min_new, uint64_t* unrouted);") in t


def test_pack_edits():
    from shadow_amd import route
    scn = [[(4, 2.5), (1, 2, 3.0), (7, INF)], [], [(0, 5, 1.0)]]
    off, edge, a, b, lat = route.pack_edits(scn)
    assert off.tolist() == [0, 3, 3, 4] and edge.tolist() == [4, -1, 7, -1]
    assert a.tolist() == [0, 1, 0, 0] and b.tolist() == [0, 2, 0, 5] and lat.tolist() == [2.5, 3.0, INF, 1.0]
    assert [x.dtype for x in (off, edge, a, b, lat)] == [np.int64, np.int32, np.int32, np.int32, np.float64]
    for x, y in zip(route.pack_edits(scn), er.pack(scn)):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(route.pack_edits((off, edge, a, b, lat)), (off, edge, a, b, lat)))
    so = er.pack(scn, sort=True)
    assert so[1].tolist() == [-1, 4, 7, -1] and so[2].tolist() == [1, 0, 0, 0] and so[4].tolist() == [3.0, 2.5, INF, 1.0]
    with pytest.raises(ValueError):
        route.pack_edits([[(1,)]])


# ---- the two references ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_fresh_equals_programme(name):
    """The definition and the kernel's programme agree bit for bit: stats, the maxima, the
    minimum, every new latency (NaNs matched), unrouted and the codes."""
    S, T, W = entries(name)
    R = ref(name)
    a = R.fresh(*er.block_entries(S, T, W), scenarios(name))
    b = programmed(name)
    assert a.same(b), (name, a.stats.tolist(), b.stats.tolist())
    assert a.stats.dtype == np.uint64 and a.lat.shape == (len(scenarios(name)), len(S) * len(T))
    # an empty scenario: zeros, the old rows and their minimum
    assert not a.stats[0].any() and a.max_add[0] == 0.0 and a.max_gain[0] == 0.0
    old = np.array([R.old(s, t)[0] for s, t in zip(*er.block_entries(S, T)[:2])])
    assert np.array_equal(a.lat[0], old, equal_nan=True)
    assert a.min_new[0] == (np.nanmin(old) if np.isfinite(old).any() else np.inf)
    for k in range(len(a.lat)):
        assert a.min_new[k] == (np.nanmin(a.lat[k]) if np.isfinite(a.lat[k]).any() else np.inf)
        # what is NaN beyond the entries that fail in G is what CUT counts (weights are >= 1 here or 0)
        assert (np.isnan(a.lat[k]) & ~np.isnan(old)).any() or not a.stats[k, er.CUT]


def test_pure_scenarios_equal_the_other_references():
    """Scenarios of finite latencies only equal the repricing reference, scenarios of removals
    only the outage reference, in every output they share."""
    for name in ("sized63", "grid", "multi389", "loops_only"):
        S, T, W = trp.entries(name)
        E = er.block_entries(S, T, W)
        scn = trp.scenarios(name)
        a, b = ref(name).programme(*E, scn), trp.programmed(name)
        assert np.array_equal(a.stats[:, [er.HIT, er.SLOWER, er.FASTER]], b.stats) and not a.stats[:, er.CUT].any()
        assert np.array_equal(a.max_add, b.max_add) and np.array_equal(a.max_gain, b.max_gain)
        assert np.array_equal(a.min_new, b.min_new) and np.array_equal(a.lat, b.lat, equal_nan=True)
        oscn = [sorted(set(f)) for f in tout.scenarios(name)]
        a = ref(name).programme(*E, [[(e, INF) for e in f] for f in oscn])
        b = tout.ref(name).repair(*E, oscn)
        # (FASTER is no zero here: a removed lowest self-loop may uncover a cheaper second one)
        assert np.array_equal(a.stats[:, [er.HIT, er.CUT, er.SLOWER]], b.stats)
        assert np.array_equal(a.max_add, b.max_add) and np.array_equal(a.lat, b.lat, equal_nan=True)


def _scn(name, *items):
    return scenarios(name).index([tuple(it) for it in items])


def test_coverage_conditions():
    """What the scenario sets must contain, asserted on the reference's results here so that a
    GPU test that equals the reference has seen each."""
    seen, logs = set(), {}
    for name in CASES:
        logs[name] = programmed(name).log
        seen |= ref(name).seen
    P = programmed("path65")
    st = P.stats.astype(np.int64)
    # a new link that ties the old latency: no FASTER, no HIT, nothing else
    k = _scn("path65", (0, 2, 2.0))
    assert not st[k].any() and np.array_equal(P.lat[k], P.lat[0], equal_nan=True)
    # two parallel new links, the dearer one first: the cheaper one counts
    assert np.array_equal(P.lat[_scn("path65", (0, 32, 5.0), (0, 32, 1.0))], P.lat[_scn("path65", (0, 32, 1.0))],
                          equal_nan=True)
    assert P.stats[_scn("path65", (0, 32, 1.0)), er.FASTER] > 0
    # a gain over >= 8 rounds through vertices that no subtree marks
    assert any(x["rounds"] >= 16 and x["outside"] and x["marked"] == 0 for x in logs["path65"])
    # a scenario dead for one source and live for another
    assert "dead_and_live" in seen
    # a rewire where a removal's CUT is undone by a new link: the same removal alone cuts
    for name, cut, join in (("path65", [(31, INF)], [(31, INF), (0, 40, 3.0)]), ("lolli20", [(19, INF)], [(2, 15, 1.5), (19, INF)])):
        r = programmed(name)
        assert r.stats[_scn(name, *cut), er.CUT] > 0 and r.stats[_scn(name, *join), er.CUT] == 0
        assert r.stats[_scn(name, *join), er.HIT] == r.stats[_scn(name, *cut), er.HIT] > 0
    # a rewire that leaves entries SLOWER and others FASTER in one scenario
    L = programmed("lolli20")
    k = _scn("lolli20", (19, INF), (0, 19, 1.0))
    assert L.stats[k, er.SLOWER] > 0 and L.stats[k, er.FASTER] > 0 and L.max_add[k] > 0 and L.max_gain[k] > 0
    # a marked vertex repaired only through a new link
    assert "marked_through_new_link" in ref("lolli20").seen
    # a removed lowest self-loop, with and without a second one
    assert {"loop_removed_alone", "loop_removed_with_second"} <= seen, seen
    # a list above 1,024 new links; a frontier above 1,024 vertices; more than 1,024 marked
    assert any(x["new"] > 2048 and x["rounds"] >= 8 for x in logs["star1100"])
    assert any(x["frontier"] > 1024 and x["marked"] == 0 for x in logs["hub1100"])
    assert any(x["marked"] > 1024 and x["frontier"] > 1024 for x in logs["hub1100"])
    assert any(x["frontier"] >= 48 for x in logs["layers48"])
    # a directed ring where a new arc helps one direction only
    D = programmed("dring12")
    S, T, _ = entries("dring12")
    row = lambda k, s: D.lat[k].reshape(len(S), len(T))[list(S).index(s)]
    k = _scn("dring12", (0, 6, 1.0))
    assert row(k, 0)[6] == 1.0 and np.array_equal(row(k, 6), row(0, 6), equal_nan=True)
    # on the fractional builders a new link one ulp better and one ulp worse
    # than the distance it rivals: all three builders, the rivalled vertex among the targets
    for name in FRAC:
        p = find_ulp(name)
        assert p is not None, name
        s, v, dv = p
        lo, hi = float(np.nextafter(dv, 0.0)), float(np.nextafter(dv, np.inf))
        assert lo < dv < hi
        r = programmed(name)
        kb, kw = _scn(name, (s, v, lo)), _scn(name, (s, v, hi))
        S, T, W = entries(name)
        j = np.flatnonzero(T == v)
        assert len(j) == 1, (name, v)
        i = list(S).index(s)
        rows = lambda k: r.lat[k].reshape(len(S), len(T))
        assert rows(kb)[i, j[0]] == lo and rows(0)[i, j[0]] == dv and r.stats[kb, er.HIT] == 0
        assert rows(kw)[i, j[0]] == dv and not r.stats[kw].any()
        assert np.array_equal(rows(kw), rows(0), equal_nan=True)
        # the block's FASTER is the weight of exactly the entries that fell, this one among them
        fell = rows(kb) < rows(0)
        assert fell[i, j[0]] and int(r.stats[kb, er.FASTER]) == int(W[fell].sum()) & er.MASK
        assert r.max_gain[kb] == np.nanmax(np.where(fell, rows(0) - rows(kb), 0.0)) >= dv - lo
        # and the entry alone: it counts in FASTER with max_gain exactly one ulp
        one = ref(name).programme([s], [v], [5], [[(s, v, lo)], [(s, v, hi)]])
        assert one.same(ref(name).fresh([s], [v], [5], [[(s, v, lo)], [(s, v, hi)]]))
        assert one.stats[0].tolist() == [0, 0, 0, 5] and one.max_gain[0] == dv - lo > 0 and one.max_add[0] == 0.0
        assert one.lat[0, 0] == lo and one.min_new[0] == lo
        assert not one.stats[1].any() and one.max_gain[1] == 0.0 and one.lat[1, 0] == dv
    # entries that fail in G take no part, even where a new link would route them
    Q = programmed("dpath9")
    assert er.EUNREACH in Q.codes and Q.unrouted > 0
    k = _scn("dpath9", (8, 0, 1.0))
    assert np.array_equal(np.isnan(Q.lat[k]), np.isnan(Q.lat[0])) and not Q.stats[k].any()
    assert er.ENOEDGE in programmed("tiny3_none").codes and programmed("tiny3_none").unrouted > 0
    # every edited graph of the fresh-context cases on the device stays connected somewhere, and one is cut
    assert any(not er.connected(er.edited(graph("dring12"), f)) for f in scenarios("dring12"))


@pytest.mark.parametrize("mutant", er.MUTANTS)
def test_mutants_are_seen(mutant):
    """Each wrong variant of the programme changes an asserted output on some case."""
    seen = []
    for name in CASES:
        if graph(name).n > 2000:
            continue
        S, T, W = entries(name)
        bad = er.EditRef(graph(name)).programme(*er.block_entries(S, T, W), scenarios(name), mutant=mutant)
        if not bad.same(programmed(name)):
            seen.append(name)
            break
    assert seen, mutant


@pytest.mark.parametrize("mutant", er.FRAC_MUTANTS)
def test_frac_mutants_are_seen(mutant):
    seen = []
    for name in FRAC:
        S, T, W = entries(name)
        bad = er.EditRef(graph(name)).programme(*er.block_entries(S, T, W), scenarios(name), mutant=mutant)
        if not bad.same(programmed(name)):
            seen.append(name)
    assert seen, mutant


# ---- the host stages ---------------------------------------------------------------------------------

HOST_CASES = [
    # (off, edge, a, b, lat) on the graph of tests/edit_host_main.cpp: n = 6, edges 0-1, 1-2, 2-3, 3-4, 4-5 at 1..5, the loop 2-2 at 9
    ([0, 4, 4, 6], [3, -1, 0, -1, 5, -1], [0, 4, 0, 1, 0, 2], [0, 5, 0, 3, 0, 0], [2.0, 1.5, INF, 0.5, INF, 7.0]),
    ([0, 0], [], [], [], []),
    ([0, 2], [1, 1], [0, 0], [0, 0], [1.0, 2.0]),            # a repeated id
    ([0, 1], [6], [0], [0], [1.0]),                          # no edge id
    ([0, 1], [-2], [0], [1], [1.0]),
    ([0, 1], [-1], [0], [6], [1.0]),                         # an end out of range
    ([0, 1], [-1], [3], [3], [1.0]),                         # a new self-loop
    ([0, 1], [-1], [0], [3], [INF]),                         # +inf on a new link
    ([0, 1], [2], [0], [0], [0.0]),
    ([0, 1], [2], [0], [0], [float("nan")]),
    ([0, 1], [2], [0], [0], [-1.0]),
    ([0, 2, 1], [2, 3], [0, 0], [0, 0], [1.0, 1.0]),         # offsets that fall
    ([0, 1], [-1], [0], [3], [1e-17]),                       # absorbed: a new link
    ([0, 1], [2], [0], [0], [1e17]),                         # absorbed: a listed latency
    ([0, 2], [5, -1], [0, 0], [0, 1], [1e-17, 1.0]),         # a self-loop's latency is outside the rule
]


def _host_want(case):
    off, edge, a, b, lat = case
    n, m, loop = 6, 6, 5
    if any(off[k + 1] < off[k] for k in range(len(off) - 1)):
        return [-1]
    lo, hi = 1.0, 5.0
    for k in range(len(off) - 1):
        ids = [e for e in edge[off[k]:off[k + 1]] if e >= 0]
        if len(ids) != len(set(ids)):
            return [-1]
    for e, u, v, w in zip(edge, a, b, lat):
        if e < -1 or e >= m or not w > 0 or (e == -1 and (math.isinf(w) or not 0 <= u < n or not 0 <= v < n or u == v)):
            return [-1]
        if not math.isinf(w) and e != loop:
            lo, hi = min(lo, w), max(hi, w)
    if lo <= (n - 1) * (hi * 2.0 ** -52):
        return [-6]
    scn = [[(int(edge[x]), float(lat[x])) if edge[x] >= 0 else (int(a[x]), int(b[x]), float(lat[x]))
            for x in range(off[k], off[k + 1])] for k in range(len(off) - 1)]
    so = er.pack(scn, sort=True)
    return [0, len(so[1])] + [(int(e), int(u), int(v), float(w)) for e, u, v, w in zip(*so[1:])]


def test_host_stages_under_sanitizers(tmp_path):
    """edit_host.hpp's packing, sorting, refusals and absorbed-latency rule and edit_layout.hpp's
    small header, read by tests/edit_host_main.cpp: built with -fsanitize=address,undefined and
    run as its own process, against this file's expectations."""
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
    exe = tmp_path / "edit_host"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "edit_host_main.cpp")], check=True)
    fmt = lambda xs: ",".join(repr(float(x)) if isinstance(x, float) else str(x) for x in xs) or "-"
    lines = []
    for case in HOST_CASES:
        r = subprocess.run([str(exe), *[fmt(col) for col in case]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines.append(r.stdout.split())
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == [er.ACC, er.NACC, er.OLDMIN, er.LIVE, er.SMALL, rr.SMALL]
    assert er.OLDMIN + 8 <= er.LIVE
    for case, got in zip(HOST_CASES, lines):
        want = _host_want(case)
        assert int(got[0]) == want[0], (case, got)
        if want[0] == 0:
            assert int(got[1]) == want[1]
            rec = [(int(got[2 + 4 * i]), int(got[3 + 4 * i]), int(got[4 + 4 * i]), float(got[5 + 4 * i])) for i in range(want[1])]
            assert rec == want[2:], (case, rec, want[2:])
    assert [_host_want(c)[0] for c in HOST_CASES] == [0, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -6, -6, 0]
