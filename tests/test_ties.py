"""CPU: the tie envelope's reference (tests/ties_ref.py) against the definition itself and the
oracle, the saturation limits of the path count, the state layout of the sweep, the interface
through every layer, and the tie line formatter (shadow_amd/csrc/tie_fmt.c) as a stand-alone
program under the host sanitizers."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from shadow_amd.graph import Graph
from tests import shape_graphs as sg
from tests import ties_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ROUTE_SYMS = ("shd_route_ties_async", "shd_route_ties")
TOPO_SYMS = ("shd_topology_tie_stats", "shd_topology_dump_ties", "shd_topology_tie_line",
             "shd_topology_tie_summary_line")
GOLDEN = ("ba60", "ba64_ties", "dir40", "ba90_frac", "ba120_vloss")


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
    for name in ("ties", "ties_async"):
        assert callable(getattr(route.RouteEngine, name))
    for name in ("tie_stats", "dump_ties"):
        assert callable(getattr(topology.Topology, name))
    # shd_tie_stats_t as the header lays it out: 4 x u64, f64, 2 x i32, u64, 2 x f64
    assert ctypes.sizeof(topology.TieStats) == 72 and topology.TieStats.worst_count.offset == 48


# ---- the reference against the definition ------------------------------------------------------

def _same(ref_row, g, s):
    """Every entry t != s of the reference's row equals the brute-force enumeration."""
    cnt, lo, hi = ref_row
    for t in range(g.n):
        if t == s:
            continue
        c, l, h = tr.brute(g, s, t)
        assert int(cnt[t]) == c, (g.name, s, t)
        assert np.array_equal([lo[t], hi[t]], [l, h], equal_nan=True), (g.name, s, t, lo[t], hi[t], l, h)


@pytest.mark.parametrize("loops", sg.TINY_LOOPS)
@pytest.mark.parametrize("n", sg.TINY_N)
def test_reference_on_tiny_paths(n, loops):
    g = sg.tiny(n, loops)
    R = tr.TiesRef(g)
    for s in range(n):
        row = R.row(s)
        _same(row, g, s)
        has_loop = bool(np.any((g.src == s) & (g.dst == s)))
        assert int(row[0][s]) == (1 if has_loop else 0) and np.isnan(row[1][s]) == (not has_loop)
        assert np.all(row[0][np.arange(n) != s] == 1)        # a path graph: one path to everything


def _random_graph(seed):
    """4 to 9 vertices, integer latencies 1-3, parallel edges and self-loops included, some
    directed, some with vertex loss; not necessarily connected."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(4, 10))
    m = int(rng.integers(n, 2 * n + 3))
    src = rng.integers(0, n, size=m).astype(np.int32)
    dst = rng.integers(0, n, size=m).astype(np.int32)
    k = int(rng.integers(1, 4))                              # parallel copies of the first k edges
    src = np.concatenate([src, src[:k] if seed % 2 else dst[:k]]).astype(np.int32)
    dst = np.concatenate([dst, dst[:k] if seed % 2 else src[:k]]).astype(np.int32)
    lat = rng.integers(1, 4, size=len(src)).astype(np.float64)
    loss = rng.integers(0, 40, size=len(src)) / 128.0
    vl = None
    if seed % 3 == 0:
        vl = rng.integers(0, 9, size=n) / 64.0
        vl[rng.integers(0, n)] = np.nan
    return Graph(n=n, src=src, dst=dst, latency=lat, packetloss=loss, vertex_packetloss=vl, directed=seed % 4 == 1,
                 name=f"rnd{seed}")


@pytest.mark.parametrize("seed", range(24))
def test_reference_on_random_graphs(seed):
    g = _random_graph(seed)
    R = tr.TiesRef(g)
    tied = 0
    for s in range(g.n):
        row = R.row(s)
        _same(row, g, s)
        tied += int(np.count_nonzero(row[0] > 1))
        ok = row[0] > 0
        assert np.all(row[1][ok] <= row[2][ok]) and np.all(row[1][ok][row[0][ok] == 1] == row[2][ok][row[0][ok] == 1])
    _TIED[seed] = tied


_TIED: dict = {}


def test_random_graphs_have_ties():
    """The random graphs are worth enumerating: most of them have tied pairs."""
    for seed in range(24):
        if seed not in _TIED:
            R = tr.TiesRef(_random_graph(seed))
            _TIED[seed] = sum(int(np.count_nonzero(R.row(s)[0] > 1)) for s in range(R.n))
    assert sum(1 for v in _TIED.values() if v > 0) >= 16 and sum(_TIED.values()) >= 100


def test_parallel_tight_edges_count_twice():
    """Two parallel edges of one latency between 0 and 1, then 1 - 2: two paths 0 -> 1 and
    0 -> 2, the bounds those of the two parallel reliabilities."""
    g = Graph(n=3, src=np.array([0, 0, 1], np.int32), dst=np.array([1, 1, 2], np.int32),
              latency=np.array([2.0, 2.0, 1.0]), packetloss=np.array([0.25, 0.5, 0.125]), name="par")
    cnt, lo, hi = tr.TiesRef(g).row(0)
    assert list(cnt) == [0, 2, 2]
    assert lo[1] == 0.5 and hi[1] == 0.75 and lo[2] == 0.5 * 0.875 and hi[2] == 0.75 * 0.875


# ---- the reference against the oracle ----------------------------------------------------------

@pytest.mark.parametrize("name", GOLDEN)
def test_reference_against_oracle(oracle_mod, name):
    """count == 1 exactly where the oracle's `unique` is set, and the oracle's reliability
    under both of its tie rules lies in [lo, hi]: to the bit where the target has no vertex
    factor, within 1e-12 relative otherwise (the oracle multiplies f_t before the edges)."""
    z = np.load(os.path.join(GOLD, "small_tables.npz"))
    p = f"{name}__"
    vl = z[p + "vertex_packetloss"]
    g = Graph(n=int(z[p + "n"]), src=z[p + "src"], dst=z[p + "dst"], latency=z[p + "latency"],
              packetloss=z[p + "packetloss"], vertex_packetloss=vl if len(vl) else None,
              directed=bool(z[p + "directed"]), prefer_direct=bool(z[p + "prefer_direct"]), name=name)
    A = np.asarray(z[p + "attached"], np.int32)
    T = np.arange(g.n, dtype=np.int32)
    og = oracle_mod.OracleGraph(g)
    cnt, lo, hi, _ = tr.TiesRef(g).rows(A, T, dispatch=False)
    off = T[None, :] != A[:, None]
    # a factor of exactly 1.0 (no loss) multiplies to the bit wherever it stands: as absent
    hasf = np.zeros(g.n, bool) if g.vertex_packetloss is None else np.nan_to_num(g.vertex_packetloss) != 0.0
    assert hasf.any() == (name == "ba120_vloss")
    exact = off & ~hasf[None, :]
    loose = off & hasf[None, :]
    for tie in (oracle_mod.TIE_IGRAPH, oracle_mod.TIE_MINKEY):
        lat, rel, uq, _ = og.source_rows(A, T, tie)
        assert np.all(np.isfinite(lat[off])) and np.all(cnt[off] >= 1)
        assert np.array_equal(cnt[off] == 1, uq[off])
        assert np.all((lo[exact] <= rel[exact]) & (rel[exact] <= hi[exact]))
        assert np.all((rel[loose] >= lo[loose] * (1 - 1e-12)) & (rel[loose] <= hi[loose] * (1 + 1e-12)))
        one = exact & (cnt == 1)
        assert np.array_equal(rel[one], lo[one]) and np.array_equal(rel[one], hi[one])
    assert (np.count_nonzero(cnt[off] > 1) > 0) == (name != "ba90_frac")   # fractional latencies leave no tie


# ---- saturation ----------------------------------------------------------------------------------

def test_saturation_limits():
    """Corner to corner of an r x c lattice there are C(r + c - 2, r - 1) shortest paths:
    34 x 35 stays below 2^64, 34 x 36 saturates, and 32 x 33 peaks at C(63, 31)."""
    assert math.comb(67, 33) == 14226520737620288370 < 2 ** 64 <= math.comb(68, 33)
    g = sg.grid(34, 35)
    cnt = tr.TiesRef(g).row(0)[0]
    assert int(cnt[g.n - 1]) == 14226520737620288370 and int(cnt.max()) == int(cnt[g.n - 1])
    g = sg.grid(34, 36)
    cnt = tr.TiesRef(g).row(0)[0]
    assert int(cnt[g.n - 1]) == tr.SAT == 2 ** 64 - 1
    assert int(cnt[g.n - 2]) == math.comb(67, 33)            # one column short of the corner: still exact
    g = sg.get("grid")
    assert g.n == 32 * 33
    cnt = tr.TiesRef(g).row(0)[0]
    assert int(cnt.max()) == math.comb(63, 31) == 916312070471295267 == int(cnt[g.n - 1])


# ---- the state layout ----------------------------------------------------------------------------

def test_layout_mirror_matches_header(tmp_path):
    """tests/ties_ref.py's layout_total / fits_lds (which the GPU tests size their graphs by)
    against shadow_amd/csrc/ties_layout.hpp, read by tests/ties_layout_main.cpp."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "ties_layout"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(ROOT, "tests", "ties_layout_main.cpp")], check=True)
    nmax = tr.lds_max_n()
    ns = [1, 2, 7, 8, 9, 63, 1056, nmax - 1, nmax, nmax + 1, 65535, 65536, 66000]
    r = subprocess.run([str(exe), *map(str, ns)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(x) for x in ln.split()) for ln in r.stdout.splitlines()]
    assert lines[0] == (tr.LDS_BUDGET, tr.SMALL)
    assert lines[1:] == [(n, tr.layout_total(n, 2), tr.layout_total(n, 4), int(tr.fits_lds(n))) for n in ns]
    assert tr.fits_lds(nmax) and not tr.fits_lds(nmax + 1)


# ---- the formatter -------------------------------------------------------------------------------

def test_tie_formatter_standalone_sanitized(tmp_path):
    """tie_fmt.c with tests/tie_fmt_main.c, built with -fsanitize=address,undefined and run as
    its own process: an undirected line, a directed line with a missing id, 40-character names
    with a saturated count (the buffer grows from 64 bytes), zero bounds, and two summaries."""
    cc = shutil.which("gcc")
    if not cc:
        pytest.skip("no gcc")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    # the runtimes linked statically where gcc has them (the program then starts whatever
    # else the process environment loads), else the shared ones
    for extra in (["-static-libasan", "-static-libubsan"], []):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover", *extra]
        if subprocess.run([cc, *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("gcc lacks the sanitizer runtime")
    exe = tmp_path / "tie_fmt_test"
    subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "tie_fmt_main.c"),
                    os.path.join(ROOT, "shadow_amd", "csrc", "tie_fmt.c")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a, b = "vertex-%033d" % 11, "vertex-%033d" % 4
    want = [
        "tie 3<-->17 (3<-->17) has 2 shortest paths, reliability 0.5 to 0.75, spread 0.33333333333333331",
        "tie poi-9-->2 (3-->2) has 6 shortest paths, reliability 0.98999999999999999 to 0.98999999999999999, spread 0",
        f"tie {a}<-->{b} (11<-->4) has 18446744073709551615+ shortest paths, reliability 0.125 to 0.25, spread 0.5",
        "tie 0<-->1 (0<-->1) has 3 shortest paths, reliability 0 to 0, spread 0",
        "ties: 4950 pairs, 321 tied, 17 sensitive, 1 saturated, max spread 0.25 at (5<-->77) with "
        "18446744073709551615+ paths",
        "ties: 276 pairs, 0 tied, 0 sensitive, 0 saturated, max spread 0 at (-1-->-1) with 0 paths",
    ]
    assert len(a) == 40 and len(want[2]) > 128
    assert r.stdout.splitlines() == want
