"""CPU: the reference of the link repricing calls (tests/reprice_ref.py) -- the definition (a
fresh reference of every repriced graph) against the kernel's programme (live test, mark, seed,
sweeps, propagation rounds), bit for bit, on every graph and scenario set the GPU tests use; the
coverage conditions those sets must meet, so that no GPU test passes vacuously; the mutants the
tests must see; the interface through every layer; and the state layout
(shadow_amd/csrc/reprice_layout.hpp) through a stand-alone program under the host sanitizers."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from tests import outage_ref as orf
from tests import reprice_ref as rr
from tests import test_outage as tout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_reprice_async", "shd_route_reprice", "shd_route_pair_reprice")
TOPO_SYMS = ("shd_topology_link_reprice",)
SMALL = tout.SMALL
LARGE = ["grid", "multi389", "dir_grid", "multi389_dir", "frac_multi", "frac_cents", "frac_hub", "lollipop",
         "sized1000", "loops_only"] + sorted(rr.BUILDERS)
FRAC = ["frac_multi", "frac_cents", "frac_hub"]
HBM16 = f"sized{rr.lds_max_n() + 1}"       # one vertex past the LDS limit
CASES = SMALL + LARGE + [HBM16]


@functools.lru_cache(maxsize=None)
def graph(name):
    return rr.BUILDERS[name]() if name in rr.BUILDERS else tout.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return rr.RepriceRef(graph(name))


def sources(name):
    if name == "hub1100":
        return np.array([0, 2], np.int32)                     # the source and a leaf
    if name == "chord65":
        return np.array([0, 40, 64], np.int32)
    if name == "layers48":
        return np.array([0, 100], np.int32)
    return tout.sources(name)


def targets(name):
    n = graph(name).n
    if n <= 400:
        return np.arange(n, dtype=np.int32)
    return np.unique(np.concatenate([np.arange(0, n, max(1, n // 150)), sources(name)])).astype(np.int32)


def weights(name, ns, nt):
    return tout.weights(name, ns, nt)


@functools.lru_cache(maxsize=None)
def entries(name):
    S, T = sources(name), targets(name)
    return S, T, weights(name, len(S), len(T))


def find_ulp_edge(name):
    """A tree edge of the first source whose latency, lowered by one ulp, leaves its head's
    distance where it was: (edge id, the lowered latency), or None."""
    R = ref(name)
    d, pe, pu, hops, order = R.base._tree(int(sources(name)[0]))
    for v in order:
        e, u = int(pe[v]), int(pu[v])
        w = np.nextafter(R.lat[e], 0.0)
        if d[u] + w == d[v]:
            return e, float(w)
    return None


def find_parallel(name):
    """Two parallel edges the tighter of which is a tree arc of the first source: (the tree
    edge, a latency above the other edge's), or None."""
    R = ref(name)
    d, pe, pu, hops, order = R.base._tree(int(sources(name)[0]))
    for v in order:
        e = int(pe[v])
        ends = {int(R.src[e]), int(R.dst[e])}
        for u, x, w in R.base.inarcs[v]:
            if x != e and {int(R.src[x]), int(R.dst[x])} == ends and w > R.lat[e]:
                return e, float(w + 1.0)
    return None


def find_mixed(name):
    """A raised tree edge and a lowered edge from outside its subtree into it, such that a vertex
    marked by the raise ends on a value it only reaches through the lowered edge: the scenario,
    or None."""
    R = rr.RepriceRef(graph(name))                       # its own: the search leaves no mark on ref(name)
    s = int(sources(name)[0])
    d, pe, pu, hops, order = R.base._tree(s)
    for r in order[: 40]:
        e = int(pe[r])
        up = [(e, float(R.lat[e] * 4))]
        sub = set(R.base.affected(s, [e]))
        for v in sub:
            for u, x, w in R.base.inarcs[v]:
                if u in sub or x == e or np.isinf(d[u]):
                    continue
                low = float(w / 8)
                with_low = R._one(s, dict(up + [(x, low)]), None)[0]
                without = R._one(s, dict(up), None)[0]
                if with_low[v] < without[v] and with_low[v] > d[v] and with_low[v] == d[u] + low:
                    return sorted(up + [(x, low)], reverse=True)
    return None


@functools.lru_cache(maxsize=None)
def _found(kind, name):
    return {"ulp": find_ulp_edge, "parallel": find_parallel, "mixed": find_mixed}[kind](name)


@functools.lru_cache(maxsize=None)
def scenarios(name):
    """The scenario lists of a case, from the tree of its first source: an empty one, tree edges
    raised and lowered near and far, one kept at its latency, a non-tree edge lowered and raised,
    two nested tree edges one up one down given descending, the lowest self-loop alone and with
    the vertex's others, a random mixed set, an integer latency made fractional, and what the
    builder is there for."""
    g, R, S = graph(name), ref(name), sources(name)
    out = [[]]
    if g.m == 0:
        return out
    lat = R.lat
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    s0 = int(S[0])
    d, pe, pu, hops, order = R.base._tree(s0)
    loops = {e for ls in R.loops for e in ls}
    tree = [int(pe[v]) for v in order]
    nontree = sorted(set(range(g.m)) - set(tree) - loops)
    if tree:
        a, b, c = tree[0], tree[-1], tree[len(tree) // 2]
        out += [[(a, lat[a] * 2)], [(b, lat[b] / 2)], [(c, lat[c] * 3)], [(c, lat[c])], [(a, lat[a] * 0.37)]]
        es = R.base.ref.path(s0, order[-1])[1]
        if len(es) >= 2:
            out.append([(es[-1], lat[es[-1]] * 2), (es[0], lat[es[0]] / 4)])
    if nontree:
        e = nontree[0]
        out += [[(e, lat[e] / 4)], [(e, lat[e] * 2)]]
        pick = [int(x) for x in rng.choice(nontree, size=min(3, len(nontree)), replace=False)]
        out.append([(e, lat[e] / 10) for e in pick])
    for s in S.tolist():
        if R.loops[s]:
            e = R.loops[s][0]
            out += [[(e, lat[e] + 2)], [(x, lat[x] / 2) for x in reversed(R.loops[s])]]
            break
    for s in S.tolist():
        if len(R.loops[s]) > 1:
            out += [[(R.loops[s][0], 0.5)], [(x, 7.0) for x in R.loops[s]]]
            break
    pick = sorted(set(int(x) for x in rng.integers(0, g.m, size=min(6, g.m))))
    out.append([(e, lat[e] * f) for e, f in zip(pick, (0.5, 2, 0.25, 3, 1, 0.75))])
    special = {"chord65": [[(64, 1.0)]], "hub1100": [[(0, 5.0)], [(1101, 5.0)], [(1101, 55.0)]],
               "layers48": [[(g.m - 1, 1.0)]]}.get(name, [])
    if name in FRAC and find_ulp_edge(name):
        special.append([find_ulp_edge(name)])
    if name.startswith("multi389") and find_parallel(name):
        special.append([find_parallel(name)])
    if name in ("sized1000", "grid", "sized63") and find_mixed(name):
        special.append(find_mixed(name))
    return [[(int(e), float(w)) for e, w in f] for f in out + special]


@functools.lru_cache(maxsize=None)
def programmed(name):
    S, T, W = entries(name)
    scn = scenarios(name)
    r = ref(name).programme(*rr.block_entries(S, T, W), scn)
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
    for name in ("reprice", "pair_reprice", "reprice_async"):
        assert callable(getattr(route.RouteEngine, name))
    assert callable(topology.Topology.link_reprice)
    h = re.sub(r"\s+", " ", text["shd_route.h"])
    assert ("int shd_route_reprice_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, "
            "int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt, const int64_t* d_scn_off, "
            "const int32_t* d_scn_edge, const double* d_scn_lat, int32_t nscn, uint64_t* d_stats, double* d_max_add, "
            "double* d_max_gain, double* d_min_new, double* d_lat, uint64_t* d_unrouted, void* stream);") in h
    assert ("int shd_route_reprice(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, "
            "uint32_t flags, const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge, "
            "const double* scn_lat, int32_t nscn, uint64_t* stats_out, double* max_add_out, double* max_gain_out, "
            "double* min_new_out, double* lat_out, uint64_t* unrouted_out);") in h
    assert ("int shd_route_pair_reprice(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, "
            "const uint64_t* pair_wt, int64_t npairs, uint32_t flags, const int64_t* scn_off, "
            "const int32_t* scn_edge, const double* scn_lat, int32_t nscn, uint64_t* stats_out, "
            "double* max_add_out, double* max_gain_out, double* min_new_out, double* lat_out, "
            "uint64_t* unrouted_out);") in h
    for k, v in (("HIT", 0), ("SLOWER", 1), ("FASTER", 2), ("NSTAT", 3)):
        assert f"#define SHD_ROUTE_REPRICE_{k} {v}" in text["shd_route.h"]
        assert getattr(route, f"REPRICE_{k}") == v == getattr(rr, k)
    assert "SHD_ROUTE_REPRICE_LDS=0" in h and "conservative" in h
    t = re.sub(r"\s+", " ", text["shd_topology.h"])
    assert ("int shd_topology_link_reprice(shd_topology_t* top, const int64_t* scn_off, const int32_t* scn_edge, "
            "const double* scn_lat, int32_t nscn, uint64_t* stats, double* max_add, double* max_gain, "
            "double* min_new, uint64_t* unrouted);") in t


# ---- the two references ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_fresh_equals_programme(name):
    """The definition and the kernel's programme agree bit for bit: stats, the maxima, the
    minimum, every new latency (NaNs matched), unrouted and the codes."""
    S, T, W = entries(name)
    R = ref(name)
    a = R.fresh(*rr.block_entries(S, T, W), scenarios(name))
    b = programmed(name)
    assert a.same(b), (name, a.stats.tolist(), b.stats.tolist())
    assert a.stats.dtype == np.uint64 and a.lat.shape == (len(scenarios(name)), len(S) * len(T))
    # an empty scenario: zeros, the old rows and their minimum
    assert not a.stats[0].any() and a.max_add[0] == 0.0 and a.max_gain[0] == 0.0
    old = np.array([R.old(s, t)[0] for s, t in zip(*rr.block_entries(S, T)[:2])])
    assert np.array_equal(a.lat[0], old, equal_nan=True)
    assert a.min_new[0] == (np.nanmin(old) if np.isfinite(old).any() else np.inf)
    # nothing is ever cut, and a scenario's minimum is the minimum of its latencies
    assert np.array_equal(np.isnan(a.lat), np.isnan(a.lat[:1]).repeat(len(a.lat), 0))
    for k in range(len(a.lat)):
        assert a.min_new[k] == (np.nanmin(a.lat[k]) if np.isfinite(a.lat[k]).any() else np.inf)


@functools.lru_cache(maxsize=None)
def ring_case():
    """(source, scenario, targets) on ring66k: an edge half-way round from the source lowered to
    a tenth, which marks a few vertices and lets the gain run on past them."""
    R = ref("ring66k")
    s = 5
    d, pe, pu, hops, order = R.base._tree(s)
    v = order[-1]
    for _ in range(8):
        v = int(pu[v])
    e = int(pe[v])
    scn = [(e, float(R.lat[e] / 10))]
    cur, mark, live = R._one(s, dict(scn), None)
    moved = np.flatnonzero(cur != d)
    ts = sorted(set(moved[:: max(1, len(moved) // 40)].tolist()) | set(mark) | {s, 0, 33000, 65999})
    return s, scn, ts


def test_ring_case_agrees():
    s, scn, ts = ring_case()
    R = ref("ring66k")
    a, b = R.fresh([s] * len(ts), ts, None, [scn]), R.programme([s] * len(ts), ts, None, [scn])
    assert a.same(b) and a.stats[0, rr.HIT] >= 1 and a.stats[0, rr.FASTER] >= 1
    assert 1 <= R.log[0]["marked"] <= 256 and R.log[0]["touched"] <= 4096 and R.log[0]["rounds"] >= 1, R.log


def test_coverage_conditions():
    """What the scenario sets must contain, asserted on the reference's results here so that a
    GPU test that equals the reference has seen each."""
    seen, hit_only, logs = set(), [], {}
    for name in CASES:
        r = programmed(name)
        logs[name] = r.log
        seen |= ref(name).seen
        st = r.stats.astype(np.int64)
        for k in range(1, len(st)):
            if st[k, rr.HIT] and not st[k, rr.SLOWER] and not st[k, rr.FASTER]:
                hit_only.append((name, k))
            # (an entry of weight 0 is still an entry: a maximum may stand beside a zero sum)
            assert (r.max_add[k] > 0 or not st[k, rr.SLOWER]) and (r.max_gain[k] > 0 or not st[k, rr.FASTER])
    # dead for one source and live for another; a raised tree edge whose route still crosses it;
    # a lowered non-tree edge that makes unhit entries faster; a lowered tree arc; the self-loops
    assert {"dead_and_live", "raised_still_crossed", "unhit_faster", "hit_faster", "lowered_tree_arc", "loop_alone",
            "loop_with_second"} <= seen, seen
    # a raised tree edge on grid whose entries keep their latency through a tied detour
    grid = [k for n, k in hit_only if n == "grid"]
    assert any(all(w > ref("grid").lat[e] for e, w in scenarios("grid")[k]) for k in grid), hit_only
    # the chord: >= 8 rounds through vertices that no subtree marks
    assert any(x["rounds"] >= 8 and x["outside"] and x["marked"] == 0 for x in logs["chord65"])
    # the hub: a frontier above 1,024 vertices, a frontier vertex with more than 1,024 out-arcs
    assert any(x["frontier"] > 1024 and x["fan"] > 1024 and x["marked"] == 0 for x in logs["hub1100"])
    assert any(x["marked"] > 1024 for x in logs["hub1100"])
    # the layers: 48 tails improve one vertex in one round
    assert any(x["tails"] >= 48 for x in logs["layers48"])
    # a vertex marked by a raise and repaired through a lowered edge
    mixed = [n for n in ("sized1000", "grid", "sized63") if find_mixed(n)]
    assert mixed and all(find_mixed(n) in scenarios(n) for n in mixed)
    # a tree edge one ulp lower whose head does not move: hit, not faster
    found = 0
    for name in FRAC:
        p = find_ulp_edge(name)
        if p is None:
            continue
        k = scenarios(name).index([p])
        st = programmed(name).stats[k]
        assert st[rr.HIT] > 0 and p[1] < ref(name).lat[p[0]]
        S, T, W = entries(name)
        s0 = int(S[0])
        row = programmed(name).lat[k].reshape(len(S), len(T))[0]
        old = programmed(name).lat[0].reshape(len(S), len(T))[0]
        head = [v for v in (int(ref(name).src[p[0]]), int(ref(name).dst[p[0]])) if ref(name).base._tree(s0)[1][v] == p[0]]
        j = np.flatnonzero(T == head[0])
        found += 1 if len(j) == 0 or row[j[0]] == old[j[0]] else 0
    assert found >= 1
    # of two parallel edges the tight one raised above the other
    p = find_parallel("multi389")
    assert p is not None and [p] in scenarios("multi389")
    k = scenarios("multi389").index([p])
    assert programmed("multi389").stats[k, rr.HIT] > 0
    # an integer graph repriced to a fractional latency, fractional graphs, a directed one
    assert float(graph("sized63").latency[0]).is_integer()
    assert any(not float(w).is_integer() for f in scenarios("sized63") for _, w in f)
    assert not float(graph("frac_multi").latency[0]).is_integer() and graph("dir_grid").directed
    assert rr.ENOEDGE in programmed("tiny3_none").codes and programmed("tiny3_none").unrouted > 0


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_mutants_are_seen(mutant):
    """Each wrong variant of the programme changes an asserted output on some case."""
    seen = []
    for name in CASES:
        if graph(name).n > 2000:
            continue
        S, T, W = entries(name)
        bad = rr.RepriceRef(graph(name)).programme(*rr.block_entries(S, T, W), scenarios(name), mutant=mutant)
        if not bad.same(programmed(name)):
            seen.append(name)
    assert seen, mutant
    print(mutant, seen)


@pytest.mark.parametrize("mutant", rr.FRAC_MUTANTS)
def test_frac_mutants_are_seen(mutant):
    seen = []
    for name in FRAC:
        S, T, W = entries(name)
        bad = rr.RepriceRef(graph(name)).programme(*rr.block_entries(S, T, W), scenarios(name), mutant=mutant)
        if not bad.same(programmed(name)):
            seen.append(name)
    assert seen, mutant


# ---- the state layout and the units ----------------------------------------------------------------

def test_layout_mirror_matches_header(tmp_path):
    """tests/reprice_ref.py's layout and state form (which the GPU tests size their graphs by)
    against shadow_amd/csrc/reprice_layout.hpp and path_host.hpp's state_form, read by
    tests/reprice_layout_main.cpp: built with -fsanitize=address,undefined and run as its own
    process, which also writes every section of every layout end to end; and the units at the
    outage test's cases."""
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
    exe = tmp_path / "reprice_layout"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "reprice_layout_main.cpp")], check=True)
    nmax = rr.lds_max_n()
    ns = [1, 2, 31, 32, 33, 65535, 65536, nmax, nmax + 1]
    args = [str(n) for n in ns] + ["units"] + [f"{k}x{q}" for k, q in tout.UNIT_CASES]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert lines[0] == (rr.LDS_BUDGET, rr.SMALL, rr.SLAB_MAX, orf.UNITS)
    assert len(lines) == 1 + len(ns) + len(tout.UNIT_CASES)
    budget = 1 << 28
    for n, ln in zip(ns, lines[1:]):
        want = (n, *rr.layout_offsets(n, 2), *rr.layout_offsets(n, 4), int(rr.fits_lds(n)))
        assert ln[:len(want)] == want
        forms = ln[len(want):]
        assert forms[:5] == rr.state_form(n, 1000, False, budget)
        assert forms[5:] == rr.state_form(n, 1000, True, budget)
        for tsize, off in ((2, ln[1:11]), (4, ln[11:21])):
            assert all(x % 16 == 0 for x in off)
            size = (8 * n, 4 * (n + 1), tsize * n, tsize * n, tsize * n, tsize * n, n, 4 * rr.words(n), 4 * rr.words(n))
            assert all(off[k] + size[k] <= off[k + 1] for k in range(9)) and off[9] == rr.layout_total(n, tsize)
            assert off[9] <= (13.25 + 4 * tsize) * n + 12 + 9 * 15
    assert rr.fits_lds(nmax) and not rr.fits_lds(nmax + 1) and nmax < orf.lds_max_n()
    assert rr.state_form(nmax, 9, False, budget)[0] == 1 and rr.state_form(nmax + 1, 9, False, budget)[0] == 2
    assert rr.state_form(65535, 9, False, budget)[0] == 2 and rr.state_form(65536, 9, False, budget)[0] == 3
    assert rr.state_form(65536, 9, False, budget)[1] == 9 and rr.state_form(65536, 1000, False, 0)[1] == 16
    text = open(os.path.join(ROOT, "shadow_amd", "csrc", "reprice_layout.hpp")).read()
    assert f"n <= {nmax}." in text
    assert f"{nmax:,} vertices" in open(os.path.join(ROOT, "include", "shd_route.h")).read()
    for (k, q), ln in zip(tout.UNIT_CASES, lines[1 + len(ns):]):
        assert ln == (k, q, *rr.units(k, q))
