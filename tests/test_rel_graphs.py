"""The rel_graphs builders have the reliabilities they are named for (no GPU, no engine: the
oracle, tests/ties_ref.py, tests/loss_ref.py, networkx and the host-only kernel selection of
tests/select_main.cpp).  These are conditions on the inputs of test_rel_gpu.py and
test_rel_paths_gpu.py: if a builder drifted back into the band (0.5, 1] of the other builders,
those tests would still pass while no longer reaching the branches they are for.  The mutants at
the end show that the references themselves tell the value-level mistakes apart on these graphs:
a flushed subnormal, a regrouped fold, a vertex factor at a transit vertex, a link that drops
nothing because 1 - loss rounds to 1."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import loss_ref as lr
from tests import rel_graphs as rg
from tests import select_cases as sc
from tests import ties_ref as tr
from tests.golden.nx_pin import nx_graph, pin_row
from tests.multi_ref import Ref
from tests.test_select import select_main  # noqa: F401  (the session's sanitizer build of select_main.cpp)

TINY = float(np.finfo(np.float64).tiny)                  # the smallest normal double

# rel_deep and rel_deep_frac (the same chain): (normal, subnormal, zero) entries of each source's
# row over all 600 vertices, the source's own entry (its lossless self-loop, 1.0) included
DEEP_ROWS = {0: (337, 20, 243), 26: (365, 16, 219), 52: (392, 17, 191), 78: (421, 19, 160), 104: (447, 16, 137),
             130: (471, 20, 109), 156: (501, 18, 81), 182: (525, 16, 59), 208: (548, 19, 33), 234: (577, 18, 5),
             260: (600, 0, 0), 286: (600, 0, 0), 300: (600, 0, 0), 338: (599, 1, 0), 364: (574, 19, 7),
             390: (548, 16, 36), 416: (526, 16, 58), 442: (501, 17, 82), 468: (473, 17, 110), 494: (449, 18, 133),
             520: (423, 19, 158), 546: (394, 18, 188), 572: (369, 18, 213), 599: (342, 17, 241)}


def classes(rel):
    """(normal, subnormal, zero) entries of a reliability row."""
    return int((rel >= TINY).sum()), int(((rel > 0.0) & (rel < TINY)).sum()), int((rel == 0.0).sum())


def has_loop(g):
    m = np.zeros(g.n, bool)
    m[g.src[g.src == g.dst]] = True
    return m


@functools.lru_cache(maxsize=None)
def oracle_table(name, every_vertex=False, tie=1):
    """(S, lat, rel, unique, hops) of the oracle over all targets, NaN where t == s and s has no
    self-loop; the suite's sources, or every vertex."""
    from oracle import oracle
    g = rg.get(name)
    og = oracle.OracleGraph(g)
    S = np.arange(g.n, dtype=np.int32) if every_vertex else rg.sources(name)
    T = np.arange(g.n, dtype=np.int32)
    hl = has_loop(g)
    lat = np.full((len(S), g.n), np.nan); rel = np.full((len(S), g.n), np.nan)
    uq = np.zeros((len(S), g.n), bool); hops = np.full((len(S), g.n), -1, np.int32)
    for i, s in enumerate(S.tolist()):
        keep = np.ones(g.n, bool) if hl[s] else T != s
        lat[i, keep], rel[i, keep], uq[i, keep], hops[i, keep] = og.source_row(s, T[keep], tie)
    for a in (lat, rel, uq, hops):
        a.setflags(write=False)
    return S, lat, rel, uq, hops


def props(g):
    nl = g.src != g.dst
    r = 1.0 - g.packetloss[nl]
    return dict(nrel=len(np.unique(r)), one=bool((r == 1.0).any()), zero=bool((r == 0.0).any()),
                noloop=1.0 - len(np.unique(g.src[~nl])) / g.n, maxw=float(g.latency[nl].max()),
                integer=bool(np.all(g.latency == np.floor(g.latency))))


def connected(g):
    """Strongly connected: everything is reached from vertex 0 forwards and backwards."""
    nl = g.src != g.dst
    for a, b in ((g.src[nl], g.dst[nl]), (g.dst[nl], g.src[nl])):
        if not g.directed:
            a, b = np.concatenate([a, b]), np.concatenate([b, a])
        seen = np.zeros(g.n, bool); seen[0] = True
        while True:
            new = seen.copy(); new[b[seen[a]]] = True
            if new.sum() == seen.sum():
                break
            seen = new
        if not seen.all():
            return False
    return True


# ---- every builder: exact reliabilities, connected, the sources -----------------------------------

@pytest.mark.parametrize("name", list(rg.SUITE))
def test_losses_are_exact_and_graphs_connected(name):
    g = rg.get(name)
    loss = g.packetloss
    assert loss.min() >= 0.0 and loss.max() <= 1.0 and connected(g)
    tiny = loss == rg.TINY
    assert np.array_equal((1.0 - loss)[~tiny] + loss[~tiny], np.ones((~tiny).sum()))
    from fractions import Fraction
    for x in np.unique(loss[~tiny]).tolist():                       # 1 - loss is exact
        assert Fraction(1.0 - x) == 1 - Fraction(x)
    assert np.all(1.0 - loss[tiny] == 1.0) and tiny.any() == (name == "rel_tinyloss")
    S = rg.sources(name)
    assert len(S) <= 24 and S[0] == 0 and S[-1] == g.n - 1 and np.all(np.diff(S) > 0)
    if name.startswith("rel_deep"):
        assert g.n // 2 in S and g.n == 600
    vl = g.vertex_packetloss
    assert (vl is not None) == (name == "rel_vzero")
    if vl is not None:
        for x in np.unique(vl[~np.isnan(vl)]).tolist():
            assert Fraction(1.0 - x) == 1 - Fraction(x)


# ---- the table limits ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rg.TABLES))
def test_table_sizes(name):
    g = rg.get(name)
    p = props(g)
    nrel, one = rg.TABLES[name]
    assert p["nrel"] == nrel and p["one"] == one and not p["zero"]
    assert p["maxw"] < 256 and p["integer"] and 0 < p["noloop"] < 1
    loops = g.src == g.dst
    assert np.all(g.packetloss[loops] > 0)                          # lossy self-loops
    assert np.isin(1.0 - g.packetloss[loops], 1.0 - g.packetloss[~loops]).all()   # ... of the edges' own values


def test_narrow_tables():
    """The graphs meant for the compact forms stay within them: at most 254 reliabilities and
    latencies below 256.  rel_deep, rel_lossy254 and rel_zero_dir's dead arcs aside, which graphs
    hold a lossless arc and which an arc of reliability 0."""
    for name in ("rel_zero", "rel_zero_ties", "rel_zero_dir", "rel_zero8000", "rel_vzero", "rel_tinyloss", "rel_deep", "rel_deep_frac"):
        p = props(rg.get(name))
        assert p["nrel"] <= 254 and p["maxw"] < 256, name
        assert p["one"] == (not name.startswith("rel_deep")), name
        assert p["zero"] == name.startswith("rel_zero"), name
        assert p["integer"] == (name != "rel_deep_frac")
    g = rg.get("rel_deep")
    nl = g.src != g.dst
    m = (1.0 - g.packetloss[nl]) * 64.0
    assert set(m.tolist()) == {3.0, 5.0, 7.0, 9.0, 11.0, 13.0, 15.0}
    assert np.all(g.packetloss[~nl] == 0.0) and (~nl).sum() == g.n     # a lossless self-loop everywhere
    assert g.latency[nl].min() >= 1 and g.latency[nl].max() <= 9
    f = rg.get("rel_deep_frac")
    assert np.array_equal(f.latency, g.latency / 100.0) and np.array_equal(f.packetloss, g.packetloss)


def select_line(exe, tmp_path, name, env=None):
    """The fields of select_main's line for the graph under a clean SHD_ROUTE_* environment."""
    path = tmp_path / f"{name}.txt"
    if not path.exists():
        path.write_text(sc.graph_text(rg.get(name)))
    e = {k: v for k, v in os.environ.items() if not k.startswith("SHD_ROUTE_")}
    e.update(env or {})
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=e)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    tok = r.stdout.split()
    assert tok[0] == "select"
    return {k: v for k, v in (t.split("=") for t in tok[1:])}


def test_selection_on_both_sides_of_every_table_limit(select_main, tmp_path):  # noqa: F811
    """What select_all() decides from the table size alone (the host-only selection, built with
    the sanitizers): 254 | 255 KD's walks and KB's fused table, 256 | 257 KD's packed records,
    65535 | 65536 KD at all.  KD is staged whatever the auto choice is, except where it refuses."""
    f = {n: select_line(select_main, tmp_path, n) for n in rg.TABLES}
    for n in ("rel_lossy254", "rel_one254"):
        assert (f[n]["kd.ok"], f[n]["kd.walk"], f[n]["kb.fused"], f[n]["kd.packed"]) == ("1", "1", "1", "1"), n
        assert f[n]["kd.nrtab"] == "254" and f[n]["kb.f_nrtab"] == "254"
    assert f["rel_lossy254"]["kd.rone"] == "-1" and int(f["rel_one254"]["kd.rone"]) >= 0
    n = "rel_lossy255"
    assert (f[n]["kd.ok"], f[n]["kd.walk"], f[n]["kb.fused"], f[n]["kd.packed"]) == ("1", "0", "0", "1")
    assert f[n]["kd.nrtab"] == "255" and f[n]["kd.rone"] == "-1"
    for n, sel in (("rel_lossy254", "5"), ("rel_one254", "5"), ("rel_lossy255", "0")):   # KF's u8 table
        k = select_line(select_main, tmp_path, n, {"SHD_ROUTE_KERNEL": "kf"})
        assert (k["sel"], k["kf.ok"]) == (sel, "1" if sel == "5" else "0"), n
        assert sel == "0" or k["kf.nrtab"] == "254"
    assert (f["rel_256"]["kd.ok"], f["rel_256"]["kd.packed"], f["rel_256"]["kd.nrtab"]) == ("1", "1", "256")
    assert (f["rel_257"]["kd.ok"], f["rel_257"]["kd.packed"], f["rel_257"]["kd.nrtab"]) == ("1", "0", "257")
    assert f["rel_256"]["kd.walk"] == f["rel_257"]["kd.walk"] == "0"
    for n in ("rel_lossy254", "rel_lossy255", "rel_one254", "rel_256", "rel_257"):
        assert f[n]["sel"] == "2", n                                  # the auto choice: KB
    a, b = f["rel_65535"], f["rel_65536"]
    assert (a["sel"], a["kd.ok"], a["kd.nrtab"], a["kb.ok"]) == ("4", "1", "65535", "0")
    assert (b["sel"], b["kd.ok"], b["kb.ok"], b["k32.ok"]) == ("1", "0", "0", "1")
    for n in ("rel_65535", "rel_65536"):                               # KD forced: taken, or the generic kernel
        k = select_line(select_main, tmp_path, n, {"SHD_ROUTE_KERNEL": "kd"})
        assert k["sel"] == ("4" if n == "rel_65535" else "0")
    # the walks with no lossless arc at all: rone == -1 with walk == 1
    for n in ("rel_deep", "rel_lossy254"):
        k = select_line(select_main, tmp_path, n, {"SHD_ROUTE_KERNEL": "kd"})
        assert (k["sel"], k["kd.walk"], k["kd.rone"]) == ("4", "1", "-1"), n
    k = select_line(select_main, tmp_path, "rel_tinyloss")
    assert int(k["kd.rone"]) >= 0 and k["kd.walk"] == "1"              # 2**-60: the lossless slot


# ---- products below the normal range ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rel_deep", "rel_deep_frac"])
def test_deep_rows_run_through_the_subnormals(name):
    S, lat, rel, uq, hops = oracle_table(name)
    assert S.tolist() == sorted(DEEP_ROWS) and uq.all()
    for i, s in enumerate(S.tolist()):
        assert classes(rel[i]) == DEEP_ROWS[s], (s, classes(rel[i]))
    for s in (0, 599):
        nrm, sub, zero = DEEP_ROWS[s]
        assert nrm >= 100 and sub >= 10 and zero >= 100
    assert hops.max() == 599 and DEEP_ROWS[300] == (600, 0, 0)
    for tie in (0, 1):                                                  # one path: both tie rules agree
        assert np.array_equal(oracle_table(name, tie=tie)[2], rel)


# ---- reliability 0 on edges ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rel_zero", "rel_zero_ties", "rel_zero_dir", "rel_zero8000"])
def test_zero_edges(name):
    g = rg.get(name)
    nl = g.src != g.dst
    loss = g.packetloss[nl]
    k = len(loss) // 2 if g.directed else len(loss)
    assert 0.09 * k <= (loss[:k] == 1.0).sum() <= 0.15 * k and 0.05 * k <= (loss[:k] == 0.0).sum() <= 0.11 * k
    assert (g.packetloss[~nl] == 1.0).sum() == 5 and 0 < props(g)["noloop"] < 1
    if g.directed:                                                     # the reverse arc of a dead arc is alive
        assert np.array_equal(g.src[nl][:k], g.dst[nl][k:]) and np.array_equal(g.dst[nl][:k], g.src[nl][k:])
        assert not np.any((loss[:k] == 1.0) & (loss[k:] == 1.0)) and not np.any(loss[k:] == 1.0)
    assert g.latency[nl].max() <= (3 if name == "rel_zero_ties" else 250)
    S, lat, rel, uq, _ = oracle_table(name, every_vertex=g.n < 1000)
    off = np.arange(g.n)[None, :] != S[:, None]
    assert not np.isnan(rel[off]).any()
    z, p = float((rel[off] == 0.0).mean()), float((rel[off] > 0.0).mean())
    print(name, "share of entries with rel == 0:", z, "rel > 0:", p)
    assert z >= 0.20 and p >= 0.20 and z + p == 1.0
    assert classes(rel[off])[1] == 0                                    # no subnormal entry
    # a loop of loss 1: the source's own entry is an exact zero
    dead = g.src[~nl][g.packetloss[~nl] == 1.0]
    assert len(dead) == 5 and all(rel[i, s] == 0.0 for i, s in enumerate(S.tolist()) if s in dead)


def test_zero_ties_envelopes():
    """rel_zero_ties over its sources: envelopes that reach down to 0 (rel_lo == 0 < rel_hi) and
    tied pairs whose every path is dead (rel_hi == 0: tie_fmt.c's guard of the spread)."""
    name = "rel_zero_ties"
    g = rg.get(name)
    S, T = rg.sources(name), np.arange(g.n)
    cnt, lo, hi, codes = tr.TiesRef(g).rows(S, T)
    ok = cnt > 0
    assert codes <= {tr.ENOEDGE} and np.all(lo[ok] <= hi[ok])
    a = int(((lo == 0.0) & (hi > 0.0)).sum()); b = int(((cnt > 1) & (hi == 0.0)).sum())
    print(name, "rel_lo == 0 < rel_hi:", a, "tied with rel_hi == 0:", b, "tied:", int((cnt > 1).sum()))
    assert a >= 10 and b >= 10 and (cnt > 1).sum() >= 1000
    _, _, rel, _, _ = oracle_table(name)
    for tie in (0, 1):                                                  # both tie rules lie inside
        r = oracle_table(name, tie=tie)[2]
        assert np.all((lo[ok] <= r[ok]) & (r[ok] <= hi[ok]))
    d = tr.TiesRef(rg.get("rel_zero_dir")).rows(rg.sources("rel_zero_dir"), T)
    assert ((d[1] == 0.0) & (d[2] > 0.0)).sum() >= 10 and ((d[0] > 1) & (d[2] == 0.0)).sum() >= 10


# ---- reliability 0 on vertices ------------------------------------------------------------------------

def test_vzero():
    name = "rel_vzero"
    g = rg.get(name)
    dead, part, full, absent = rg.vclasses(g)
    assert (len(dead), len(part), len(full), len(absent)) == (6, 30, 100, 389 - 136)
    assert set(np.unique(g.vertex_packetloss[part]).tolist()) == set(rg.VHALF)
    S, lat, rel, uq, hops = oracle_table(name)
    for c in (dead, part, full, absent):                                # sources of all four classes
        assert len(np.intersect1d(S, c)) >= 2
    hl = has_loop(g)
    is_dead = np.zeros(g.n, bool); is_dead[dead] = True
    R = Ref(g)
    through = 0
    for i, s in enumerate(S.tolist()):
        ok = ~np.isnan(rel[i])
        assert np.array_equal(np.isnan(rel[i]), (np.arange(g.n) == s) & ~hl[s])
        if is_dead[s]:
            assert np.all(rel[i][ok] == 0.0)                            # f_s = 0 zeroes the row
            continue
        # elsewhere exactly the dead targets are zero, whatever the path passes through
        assert np.array_equal(rel[i] == 0.0, is_dead & ok)
        d, pe, pu, _ = R.dijkstra(s)
        thru = np.zeros(g.n, bool)                                      # a dead vertex in transit
        for v in np.argsort(d, kind="stable").tolist():
            if v != s:
                thru[v] = thru[pu[v]] or (is_dead[pu[v]] and pu[v] != s)
        assert np.all(rel[i][thru & ~is_dead] > 0.0)
        through += int((thru & ~is_dead).sum())
    assert through >= 1000
    assert classes(rel[~np.isnan(rel)])[1] == 0                         # no subnormal entry
    assert hops.max() <= 32                                             # within KD's walk window


def test_tinyloss():
    g = rg.get("rel_tinyloss")
    nl = g.src != g.dst
    tiny = g.packetloss[nl] == rg.TINY
    assert 0.10 <= tiny.mean() <= 0.20 and not np.any(g.packetloss[~nl] == rg.TINY)
    h = rg.without_loss(g)
    assert np.array_equal(1.0 - h.packetloss, 1.0 - g.packetloss) and not np.array_equal(h.packetloss, g.packetloss)
    assert np.array_equal(oracle_table("rel_tinyloss")[2], Ref(h).rows(rg.sources("rel_tinyloss"), np.arange(g.n))[1],
                          equal_nan=True)


# ---- the Python references are the oracle on these graphs ---------------------------------------------

@pytest.mark.parametrize("name", [n for n in rg.SUITE if rg.get(n).n < 1000])
def test_ref_rows_are_the_oracle(name):
    """multi_ref.Ref, which ties_ref, fold_ref and loss_ref are built on, against the oracle's
    TIE_MINKEY rows: exact zeros and subnormals included."""
    g = rg.get(name)
    S, lat, rel, _, hops = oracle_table(name)
    rl, rr, rh = Ref(g).rows(S, np.arange(g.n))
    assert np.array_equal(rl, lat, equal_nan=True) and np.array_equal(rh, hops)
    assert np.array_equal(rr, rel, equal_nan=True)   # (with vertex loss too: both multiply f_t before the arcs)


# ---- independent pinning ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rel_zero", "rel_vzero", "rel_deep"])
def test_rows_pinned_by_networkx(name):
    g = rg.get(name)
    G = nx_graph(g)
    S, lat, rel, uq, _ = oracle_table(name)
    T = np.arange(g.n)
    at = [0, len(S) // 3, 2 * len(S) // 3, len(S) - 1]
    if name == "rel_vzero":
        at[1] = int(np.flatnonzero(S == rg.vclasses(g)[0][-1])[0])     # a source of vertex loss 1.0 beside vertex 0
    checked = 0
    for i in at:
        n_lat, n_rel = pin_row(G, g, int(S[i]), T, lat[i], rel[i], uq[i])
        assert n_lat == g.n - 1 and n_rel >= int(uq[i].sum()) - 1
        checked += n_rel
    assert checked >= 4 * g.n // 2


# ---- mutants of the reference -------------------------------------------------------------------------

def fold(g, R, s, t, mutant=None):
    """Shadow's product of the entry (s, t), t != s, along Ref's route: ((1.0 * f_s) * f_t), then
    1 - loss of every hop from the source on.  Mutants: "flush" replaces a subnormal product by
    0.0, "right" groups the arcs from the target's end, "transit" also multiplies the factor of
    every vertex passed through."""
    vs, es = R.path(s, t)
    r = [float(R.erel[e]) for e in es]
    x = float(R.base(s, t))
    if mutant == "right":
        acc = r[-1]
        for y in reversed(r[:-1]):
            acc = y * acc
        return x * acc
    for k, y in enumerate(r):
        x = x * y
        if mutant == "flush" and 0.0 < x < TINY:
            x = 0.0
        if mutant == "transit" and k + 1 < len(r) and not np.isnan(R.vf[vs[k + 1]]):
            x = x * float(R.vf[vs[k + 1]])
    return x


def fold_rows(name, rows, mutant=None):
    g = rg.get(name)
    R = Ref(g)
    S = rg.sources(name)
    return np.array([[np.nan if t == s else fold(g, R, s, t, mutant) for t in range(g.n)] for s in S[rows].tolist()])


def test_mutants_of_the_rows_reference():
    """The plain fold is the oracle to the bit; each mutant is not, on the graph built for it."""
    ends = [0, 12, 23]                                                  # vertices 0, 300 and 599 of the chain
    S, lat, rel, _, _ = oracle_table("rel_deep")
    assert S[ends].tolist() == [0, 300, 599]
    off = np.arange(600)[None, :] != S[ends][:, None]
    want = rel[ends]
    assert np.array_equal(fold_rows("rel_deep", ends)[off], want[off])
    flush = fold_rows("rel_deep", ends, "flush")
    assert (flush[off] != want[off]).sum() == sum(DEEP_ROWS[s][1] for s in (0, 300, 599)) > 30
    right = fold_rows("rel_deep", ends, "right")
    d = right[off] != want[off]
    print("right fold differs from the left fold on", int(d[:599].sum()), "entries of row 0,", int(d.sum()), "in all")
    assert d[:599].sum() >= 100 and d.sum() >= 300
    S, lat, rel, _, _ = oracle_table("rel_vzero")
    dead = set(rg.vclasses(rg.get("rel_vzero"))[0].tolist())
    rows = [i for i, s in enumerate(S.tolist()) if s not in dead][:4]
    off = np.arange(389)[None, :] != S[rows][:, None]
    assert np.array_equal(fold_rows("rel_vzero", rows)[off], rel[rows][off])
    transit = fold_rows("rel_vzero", rows, "transit")
    assert ((transit[off] == 0.0) & (rel[rows][off] > 0.0)).sum() >= 100


def test_mutant_of_the_loss_reference():
    """LossRef's mutant "one_minus_r" takes q_e = 1.0 - r_e: an arc of r == 1.0 then drops nothing.
    On rel_tinyloss it differs on exactly the loaded 2**-60 edges (every other loss is 1 - r to
    the bit), and nowhere on the copy without those losses."""
    g = rg.get("rel_tinyloss")
    S, T = rg.sources("rel_tinyloss")[:6], np.arange(g.n)
    L = lr.LossRef(g)
    want, mut = L.block(S, T), L.block(S, T, mutant="one_minus_r")
    tiny = g.packetloss == rg.TINY
    reach = np.array(want.edge_reach)
    diff = np.array(want.edge_drop) != np.array(mut.edge_drop)
    assert np.array_equal(diff, tiny & (reach > 0)) and diff.sum() >= 50
    assert np.all(np.array(want.edge_drop)[diff] > 0) and np.all(np.array(mut.edge_drop)[diff] == 0)
    assert want.delivered == mut.delivered and want.edge_reach == mut.edge_reach
    h = lr.LossRef(rg.without_loss(g))
    assert h.block(S, T).edge_drop == h.block(S, T, mutant="one_minus_r").edge_drop == mut.edge_drop


# ---- link loss: watched products, conservation ----------------------------------------------------------

class _Watch(float):
    """A double whose products must stay in the normal range: a product of two non-zero factors is
    neither subnormal nor zero."""
    def __mul__(self, o):
        x = float.__mul__(self, o)
        assert (abs(x) >= TINY) if (self != 0.0 and o != 0.0) else x == 0.0, (float(self), float(o))
        return _Watch(x)
    __rmul__ = __mul__

    def __add__(self, o):
        return _Watch(float.__add__(self, o))
    __radd__ = __add__


class Watched(lr.LossRef):
    """loss_ref.LossRef whose f64 programme asserts, while it runs, that no intermediate product
    leaves the normal range (the derivation of the bound (R + 4 + A) * 2^-52 assumes it)."""
    def _run(self, programmes, dispatch, exact, init, mutant):
        assert not exact and init is None
        acc = [lr._Acc(k, _Watch(0.0), None) for k in (self.m, self.m, self.n, self.n)]
        st = {"codes": set(), "un": 0, "R": 0, "routed": 0}
        for s, entries in programmes:
            self._source(int(s), entries, dispatch, acc, _Watch, None, st)
        A = max(max(a.c, default=0) for a in acc)
        return lr.Result(*[[float(x) for x in a.v] for a in acc], st["un"] % lr.U64, st["R"], A, st["codes"], st["routed"])


@functools.lru_cache(maxsize=None)
def loss_weights(name):
    """One u64 weight below 2^40 per (source, vertex) of the builder's sources."""
    g = rg.get(name)
    W = np.random.default_rng(g.n).integers(1, 1 << 40, size=(len(rg.sources(name)), g.n), dtype=np.uint64)
    W.setflags(write=False)
    return W


@pytest.mark.parametrize("name", ["rel_zero", "rel_vzero", "rel_tinyloss"])
def test_loss_products_stay_normal_and_packets_are_conserved(name):
    """The watched f64 programme is the plain one to the bit.  In exact fractions every routed
    packet is dropped by an edge, dropped by a vertex or delivered, where loss and 1 - loss are
    exact complements; a link of loss 2**-60 passes everything on (r == 1.0) and drops 2**-60 of
    it besides, so there the three sums exceed the routed packets by exactly those drops."""
    from fractions import Fraction
    g = rg.get(name)
    S, T, W = rg.sources(name), np.arange(g.n, dtype=np.int32), loss_weights(name)
    plain, watched = lr.LossRef(g).block(S, T, W), Watched(g).block(S, T, W)
    assert plain.outs() == watched.outs() and (plain.R, plain.A, plain.codes) == (watched.R, watched.A, watched.codes)
    x = lr.LossRef(g).block(S, T, W, exact=True)
    assert x.A > 2 and (x.R, x.A, x.unrouted) == (plain.R, plain.A, plain.unrouted)
    for k in range(4):
        assert lr.close(plain.arrays()[k], x.outs()[k], x.R, x.A)
    total = sum(x.edge_drop) + sum(x.vertex_drop) + sum(x.delivered)
    tiny = g.packetloss == rg.TINY
    extra = sum((d for d, t in zip(x.edge_drop, tiny.tolist()) if t), Fraction(0))
    assert total - extra == x.routed and (extra > 0) == (name == "rel_tinyloss")
    if name == "rel_zero":                                  # a dead link drops all that reaches it
        dead = np.flatnonzero((g.packetloss == 1.0) & (np.array(plain.edge_reach) > 0))
        assert len(dead) >= 20 and all(x.edge_drop[e] == x.edge_reach[e] for e in dead.tolist())


def test_deep_loss_leaves_the_normal_range():
    """The chain is why rel_deep is held to the exact one-source form alone: its programme has
    subnormal products, which the watched reference refuses."""
    g = rg.get("rel_deep")
    S, T = rg.sources("rel_deep")[:1], np.arange(g.n, dtype=np.int32)
    with pytest.raises(AssertionError):
        Watched(g).block(S, T, loss_weights("rel_deep")[:1])
    one = lr.LossRef(g).block(S, T, loss_weights("rel_deep")[:1])
    assert one.A <= 2 and sum(0.0 < v < TINY for v in one.delivered) >= 3
