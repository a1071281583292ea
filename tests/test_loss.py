"""CPU: the reference of the link loss calls (tests/loss_ref.py) -- the f64 programme against
exact fractions within the derived bound, conservation, the zero-loss and unit-weight identities
against Ref.loads and Ref.rows, the mutants the tests must see --; the interface through every
layer; and the state layout of the sweep (shadow_amd/csrc/loss_layout.hpp) through a stand-alone
program under the host sanitizers."""
import ctypes
import dataclasses
import functools
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import frac_graphs as fgr
from tests import loss_ref as lr
from tests import multi_graphs as mg
from tests import shape_graphs as sg
from tests import test_ecmp as te
from tests import test_hops_gpu as hg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_loss_async", "shd_route_loss", "shd_route_pair_loss")
TOPO_SYMS = ("shd_topology_link_loss",)
# the small builders: the shapes of the loads and folds tests (grid, directed grid, lollipop, BA,
# a tied multigraph, the paths of 1 to 9 vertices with and without self-loops), the star, a
# prefer-direct and a complete graph, one complete by count with parallel edges, a multigraph
# with vertex loss on half of the vertices, fractional latencies, missing self-loops, decimal
# losses with vertex loss on two vertices in three, and no loss at all
GRAPHS = te.GRAPHS + ["star40", "ba80_prefer", "k24", "count_complete", "multi389_vloss", "ba120_vloss", "frac_grid",
                      "ba60_holes", "ba60_dec", "ba60_zero"]


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "star40":
        return sg.star(40)
    if name in mg.SUITE:
        return mg.get(name)
    if name in fgr.SUITE:
        return fgr.get(name)
    if name == "ba60_dec":
        return lr.decimal_losses(hg._graph("ba60")[0], 60)
    if name == "ba60_zero":
        g = hg._graph("ba60")[0]
        return dataclasses.replace(g, packetloss=np.zeros(g.m), vertex_packetloss=None, name=name)
    if name in ("ba80_prefer", "k24", "ba120_vloss", "ba60_holes", "ba60"):
        return hg._graph(name)[0]
    return te.graph(name)


@functools.lru_cache(maxsize=None)
def ref(name):
    return lr.LossRef(graph(name))


def sources(name, k=6):
    """Every vertex of a graph of up to 64 vertices, else k spread over it, 0 and n - 1 among them."""
    n = graph(name).n
    if n <= 64:
        return np.arange(n, dtype=np.int32)
    return np.unique(np.linspace(0, n - 1, k).astype(np.int32))


def weights(name, ns, nt, seed=0):
    """Packet counts 0 .. 999 with a tenth of them zero."""
    rng = np.random.default_rng(7000 + seed + ns * nt)
    w = rng.integers(1, 1000, size=(ns, nt)).astype(np.uint64)
    w[rng.random((ns, nt)) < 0.1] = 0
    return w


def has_vertex_loss(g):
    return g.vertex_packetloss is not None and bool(np.any(~np.isnan(np.asarray(g.vertex_packetloss, np.float64))))


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
    for name in ("loss", "pair_loss", "loss_async"):
        assert callable(getattr(route.RouteEngine, name))
    assert callable(topology.Topology.link_loss)
    h = re.sub(r"\s+", " ", text["shd_route.h"])
    assert ("int shd_route_loss_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, "
            "int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt, double* d_edge_reach, double* d_edge_drop, "
            "double* d_vertex_drop, double* d_delivered, uint64_t* d_unrouted, void* stream);") in h
    assert ("int shd_route_loss(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, "
            "uint32_t flags, const uint64_t* wt, double* edge_reach_out, double* edge_drop_out, "
            "double* vertex_drop_out, double* delivered_out, uint64_t* unrouted_out);") in h
    assert ("int shd_route_pair_loss(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, "
            "const uint64_t* pair_wt, int64_t npairs, uint32_t flags, double* edge_reach_out, double* edge_drop_out, "
            "double* vertex_drop_out, double* delivered_out, uint64_t* unrouted_out);") in h
    assert "(R + 4 + A) * 2^-52" in h and "SHD_ROUTE_LOSS_LDS=0" in h
    t = re.sub(r"\s+", " ", text["shd_topology.h"])
    assert ("int shd_topology_link_loss(shd_topology_t* top, double* edge_reach, double* edge_drop, "
            "double* vertex_drop, double* delivered, uint64_t* unrouted);") in t
    assert "both directions" in t and "stored orientation" in t


# ---- the f64 programme against exact fractions ----------------------------------------------------

@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_f64_against_fractions(name, dispatch):
    """The block of some sources x all vertices, weighted, and the same entries as shuffled pairs
    with a hundred repeats: every element of the f64 programme within (R + 4 + A) * 2^-52 of the
    exact one, unrouted and the codes equal, and an exact 0 exactly 0."""
    g, R = graph(name), ref(name)
    S, T = sources(name), np.arange(g.n, dtype=np.int32)
    W = weights(name, len(S), len(T))
    got, want = R.block(S, T, W, dispatch), R.block(S, T, W, dispatch, exact=True)
    assert (got.unrouted, got.codes, got.R, got.A) == (want.unrouted, want.codes, want.R, want.A)
    for a, b in zip(got.outs(), want.outs()):
        assert lr.close(a, b, want.R, want.A)
        assert [x == 0 for x in a] == [y == 0 for y in b]
    assert want.A >= (1 if want.routed else 0) and want.R <= g.n and (want.routed > 0) == (name != "tiny1_none")
    if g.n > 2:
        assert sum(x != 0 for x in want.edge_reach) >= 2
    rng = np.random.default_rng(len(S))
    ps, pt, pw = np.repeat(S, len(T)), np.tile(T, len(S)), W.ravel()
    k = np.concatenate([rng.permutation(len(ps)), rng.integers(0, len(ps), size=100)])
    gp, wp = R.pairs(ps[k], pt[k], pw[k], dispatch), R.pairs(ps[k], pt[k], pw[k], dispatch, exact=True)
    assert (gp.unrouted, gp.codes) == (wp.unrouted, wp.codes)
    for a, b in zip(gp.outs(), wp.outs()):
        assert lr.close(a, b, wp.R, wp.A)


def test_bound_is_tight_enough_to_see_an_ulp():
    """close() refuses one part in 2^40 and an element that should be 0."""
    want = [Fraction(3, 7), Fraction(0)]
    good = [3 / 7, 0.0]
    assert lr.close(good, want, 5, 3)
    assert not lr.close([3 / 7 * (1 + 2.0 ** -40), 0.0], want, 5, 3)
    assert not lr.close([3 / 7, 1e-300], want, 5, 3)
    assert not lr.close([float("nan"), 0.0], want, 5, 3)
    assert lr.bound(5, 3) == Fraction(12, 2 ** 52)


@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", GRAPHS)
def test_conservation(name, dispatch):
    """In fractions every routed packet is dropped by an edge, dropped by a vertex or delivered:
    exactly where 1.0 - loss is exact in f64 (the dyadic losses of the shape, fractional and BA
    builders), else within the rounding of the R + 2 factors 1.0 - loss of a route."""
    g, R = graph(name), ref(name)
    S, T = sources(name), np.arange(g.n, dtype=np.int32)
    W = weights(name, len(S), len(T), 1)
    x = R.block(S, T, W, dispatch, exact=True)
    total = sum(x.edge_drop) + sum(x.vertex_drop) + sum(x.delivered)
    comp = all(Fraction(r) + Fraction(q) == 1 for r, q in zip(R.r, R.q)) and \
        all(p != p or Fraction(f) + Fraction(p) == 1 for f, p in zip(R.f, R.p))
    print(name, "complements exact" if comp else "complements rounded")
    dyadic = ("grid6x7", "dir_grid6x6", "lollipop8_20", "star40", "frac_grid", "ba60_zero")
    if name in dyadic or name.startswith("tiny"):
        assert comp
    if name in ("ba60_dec", "count_complete"):
        assert not comp
    if comp:
        assert total == x.routed
    else:
        assert abs(total - x.routed) <= Fraction(x.R + 2, 1 << 53) * x.routed
    assert x.routed + x.unrouted == int(W.sum(dtype=np.uint64)) and (x.routed > 0) == (name != "tiny1_none")


def test_zero_loss_is_the_loads():
    """No loss anywhere: edge_reach is Ref.loads' edge load as doubles, both drops are all zero
    and everything routed is delivered."""
    name = "ba60_zero"
    g, R = graph(name), ref(name)
    S, T = sources(name), np.arange(g.n, dtype=np.int32)
    W = weights(name, len(S), len(T), 2)
    for dispatch in (False, True):
        x = R.block(S, T, W, dispatch)
        el, _, un = R.ref.loads(np.repeat(S, len(T)), np.tile(T, len(S)), W.ravel(), dispatch)
        er, ed, vd, dl = x.arrays()
        assert np.array_equal(er, el.astype(np.float64)) and un == x.unrouted
        assert not ed.any() and not vd.any() and dl.sum() == float(x.routed)


@pytest.mark.parametrize("dispatch", [False, True])
@pytest.mark.parametrize("name", [n for n in GRAPHS if n not in ("multi389_vloss", "ba120_vloss", "ba60_dec")])
def test_unit_weights_deliver_rel(name, dispatch):
    """One source, unit weights, no vertex loss: delivered[t] is Ref.rows' rel, bit for bit."""
    g, R = graph(name), ref(name)
    assert not has_vertex_loss(g) or not np.any(np.nan_to_num(np.asarray(g.vertex_packetloss)))
    T = np.arange(g.n, dtype=np.int32)
    for s in sources(name, 3).tolist():
        _, rel, _ = R.ref.rows([s], T, dispatch)
        x = R.block([s], T, None, dispatch)
        assert x.A <= 2
        assert np.array_equal(x.arrays()[3], np.nan_to_num(rel[0]))       # a failed entry delivers nothing


def test_some_graph_has_each_feature():
    assert sum(has_vertex_loss(graph(n)) for n in GRAPHS) >= 3
    vl = np.asarray(graph("ba60_dec").vertex_packetloss)
    assert np.isnan(vl).any() and (~np.isnan(vl)).any()
    q = np.asarray(graph("ba60_dec").packetloss)
    assert np.all(q.astype(np.float32).astype(np.float64) != q)             # no float32 holds these losses
    assert any(graph(n).directed for n in GRAPHS) and ref("k24").ref.complete and ref("count_complete").ref.complete
    assert graph("ba80_prefer").prefer_direct and graph("tiny1_none").m == 0 and graph("tiny2_all").n == 2


# ---- the mutants ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", lr.MUTANTS)
def test_mutants_are_seen(mutant):
    """A wrong kernel shows: each mutant of the programme changes an element that the one-source
    comparison (array_equal with the f64 programme) asserts on some builder, and the ones that
    are wrong by more than rounding also leave the bound of the many-source comparison."""
    seen_bits, seen_bound = [], []
    for name in GRAPHS:
        g, R = graph(name), ref(name)
        T = np.arange(g.n, dtype=np.int32)
        S = sources(name, 3)
        for s in S.tolist():
            a, b = R.block([s], T, None, False), R.block([s], T, None, False, mutant=mutant)
            if any(not np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays())):
                seen_bits.append(name)
                break
        W = weights(name, len(S), len(T), 3)
        want, bad = R.block(S, T, W, False, exact=True), R.block(S, T, W, False, mutant=mutant)
        if any(not lr.close(x, y, want.R, want.A) for x, y in zip(bad.outs(), want.outs())):
            seen_bound.append(name)
    assert seen_bits, mutant
    if mutant == "one_minus_r":
        assert "ba60_dec" in seen_bits and "grid6x7" not in seen_bits      # dyadic losses: 1 - r_e is q_e
    if mutant in ("transit_factor", "self_twice"):
        assert seen_bound and set(seen_bits) <= {n for n in GRAPHS if has_vertex_loss(graph(n))}


# ---- the state layout ----------------------------------------------------------------------------

def test_layout_mirror_matches_header(tmp_path):
    """tests/loss_ref.py's layout arithmetic (which the GPU tests size their graphs by) against
    shadow_amd/csrc/loss_layout.hpp, read by tests/loss_layout_main.cpp: built with
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
    exe = tmp_path / "loss_layout"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "loss_layout_main.cpp")], check=True)
    nmax = lr.lds_max_n()
    ns = [1, 2, 7, 8, 9, 65535, 65536, nmax, nmax + 1]
    r = subprocess.run([str(exe), *map(str, ns)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert lines[0] == (lr.LDS_BUDGET, lr.SMALL)
    assert len(lines) == 1 + len(ns)
    for n, ln in zip(ns, lines[1:]):
        assert ln == (n, *lr.layout_offsets(n, 2), *lr.layout_offsets(n, 4), int(lr.fits_lds(n)))
        for tsize, (s, pre, lvl, order, total) in ((2, ln[1:6]), (4, ln[6:11])):
            assert s % 16 == pre % 16 == lvl % 16 == order % 16 == total % 16 == 0           # aligned
            assert s + 8 * n <= pre and pre + 8 * n <= lvl and lvl + 4 * (n + 1) <= order    # disjoint
            assert order + tsize * n <= total == lr.layout_total(n, tsize)
            assert total <= (20 + tsize) * n + 4 + 4 * 15                                     # about 22 B per vertex
    # the limit: the state of nmax vertices is the last that fits beside the small header
    assert lr.fits_lds(nmax) and not lr.fits_lds(nmax + 1) and nmax == 7442
    assert lr.SMALL + lr.layout_total(nmax) <= lr.LDS_BUDGET < lr.SMALL + lr.layout_total(nmax + 1)
    # and the header says so
    text = open(os.path.join(ROOT, "shadow_amd", "csrc", "loss_layout.hpp")).read()
    assert f"n <= {nmax}" in text
