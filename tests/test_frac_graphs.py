"""The builders of tests/frac_graphs.py have the properties test_frac_paths_gpu.py depends on,
shown with the Python references alone (no engine, no GPU): if a builder drifted to inputs
without f64 ties and near misses, the GPU tests would still pass while no longer telling a kernel
that follows the rule d[u] + w == d[v] from one that does not.  Every count is printed before it
is asserted (run with -s).

Per tied builder, over the sources of frac_graphs.sources:
  ties         at least 10% of the (source, vertex) entries have more than one shortest path
  near misses  at least 50 distinct arcs have d[u] + w != d[v] within 8 ulp of d[v] for some
               source; one of them ends on an in-list of more than 128 arcs (frac_hub), one has a
               parallel twin (frac_multi)
  paper ties   the path count in exact arithmetic (fractions.Fraction over the decimals k / scale)
               differs from the f64 count in at least 20 entries
  mutants      (a) tightness within one ulp, (b) distances folded from the target (right folds
               along the reference's routes), (c) latencies read as float32: each changes the
               parent of at least 10 entries, the count of at least 10 entries and at least one
               bit of a route's latency sum.  (frac_hub, whose distances never exceed two hops
               through a hub, cannot show (b) at all and shows (a) in the counts only: the reason
               stands at the assertion.)  (d) Ref(g, tie="high") takes the highest edge id
               among tight arcs of one tail: by its definition it can differ from the rule only
               where parallel arcs from one tail are tight together, which a simple graph does not
               have, and it never changes a tail, a count or a latency.  So (d) is held to what it
               can change: on frac_multi the parent edge of at least 10 entries and a bit of the
               reliability product along the routes; on the simple builders it changes nothing,
               which is asserted as well.

Link outages and link loss (the scenario rule and the weight block test_frac_paths_gpu.py uses):
  outages      no entry fails and no scenario cuts anything (every reduced graph has a context);
               at least three tied builders have a scenario with HIT > SLOWER (a tied detour), and
               frac_multi one with HIT > 0 and SLOWER == 0 (the failed edge has a tied twin); some
               scenario's max_add lies in (0, 2^-50): entries that get slower by an ulp
  mutants      SLOWER judged with a tolerance, a repaired distance rebuilt from its root's instead
               of folded from the source, and LossRef over the highest tight edge id of a hop:
               each changes an asserted output

The last section pins the premise the path calls rest on (the tight arcs form a DAG because
d[u] + w > d[u]) on a chain whose latencies are absorbed, and the host-side refusal of
shd_route_create that keeps such a graph away from every kernel.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from shadow_amd.graph import Graph, config
from tests import ecmp_ref as er
from tests import frac_graphs as fg
from tests import loss_ref as lr
from tests import outage_ref as orf
from tests.multi_ref import Ref
from tests.ties_ref import TiesRef

WIDE = 128      # two waves: above it hops_parent_kernel and the sweeps scan an in-list wave-wide


@functools.lru_cache(maxsize=None)
def ref_of(name, tie="low"):
    return Ref(fg.get(name), tie)


def derive(R, s, d, W, ulps=0):
    """What the rule gives from the distances d and the arc weights W (in Ref's arc order): the
    parent arc of every vertex (-1: none), the number of tight-arc paths from s (Python ints) and
    the left fold of W down the parents.  ulps > 0: the mutant that takes |d[u] + w - d[v]| <=
    ulps * spacing(d[v]) for tight."""
    U, V, E, n = R.U, R.V, R.E, R.n
    with np.errstate(invalid="ignore"):
        cand = d[U] + W
        tight = (np.abs(cand - d[V]) <= ulps * np.spacing(d[V])) if ulps else (cand == d[V])
        tight &= (V != s) & np.isfinite(d[U])
    q = np.flatnonzero(tight)
    o = q[np.lexsort((E[q], U[q], d[U[q]], V[q]))]
    head = np.ones(len(o), bool)
    head[1:] = V[o][1:] != V[o][:-1]
    pa = np.full(n, -1, np.int64)
    pa[V[o[head]]] = o[head]
    start = np.searchsorted(V[q], np.arange(n + 1))
    tu = U[q].tolist()
    cnt, fs = [0] * n, [float("nan")] * n
    cnt[s], fs[s] = 1, 0.0
    for v in np.argsort(d, kind="stable").tolist():          # a tight arc's tail is strictly nearer
        if v == s or pa[v] < 0:
            continue
        cnt[v] = sum(cnt[tu[k]] for k in range(int(start[v]), int(start[v + 1])))
        fs[v] = fs[int(U[pa[v]])] + float(W[pa[v]])
    return pa, cnt, np.array(fs)


@functools.lru_cache(maxsize=None)
def base(name):
    """[(s, d, parent arc, counts, latency sums)] of the rule itself over the builder's sources."""
    R = ref_of(name)
    out = []
    for s in fg.sources(name).tolist():
        d = R.dijkstra(s)[0]
        out.append((s, d) + derive(R, s, d, R.W))
    return out


def right_fold_distances(R, s):
    """d'[v] = w_1 + (w_2 + (... + w_k)) along the reference's route s -> v: summed from the target."""
    d, pe, pu, _ = R.dijkstra(s)
    out = np.full(R.n, np.inf)
    out[s] = 0.0
    for v in range(R.n):
        if v == s or pu[v] < 0:
            continue
        acc, x = 0.0, v
        while x != s:
            acc = float(R.lat[pe[x]]) + acc
            x = int(pu[x])
        out[v] = acc
    return out


def changes(name, mutant):
    """(parents, counts, latency-sum bits) that differ from the rule, summed over the sources."""
    R = ref_of(name)
    dp = dc = df = 0
    for s, d, pa, cnt, fs in base(name):
        if mutant == "ulp":
            m = derive(R, s, d, R.W, ulps=1)
        elif mutant == "right":
            m = derive(R, s, right_fold_distances(R, s), R.W)
        else:
            g = fg.get(name)
            g32 = Graph(n=g.n, src=g.src, dst=g.dst, latency=g.latency.astype(np.float32).astype(np.float64),
                        packetloss=g.packetloss, vertex_packetloss=g.vertex_packetloss, directed=g.directed)
            R32 = changes.r32.setdefault(name, Ref(g32))
            assert np.array_equal(R32.E, R.E) and np.array_equal(R32.U, R.U)
            m = derive(R32, s, R32.dijkstra(s)[0], R32.W)
        dp += int(np.count_nonzero(m[0] != pa))
        dc += sum(1 for a, b in zip(m[1], cnt) if a != b)
        df += int(np.count_nonzero(m[2].view(np.int64) != fs.view(np.int64)))
    return dp, dc, df


changes.r32 = {}


# ---- the builders as inputs -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(fg.SUITE))
def test_shape_of_the_inputs(name):
    """Decimals k / scale with k <= 65535 where KFH is to pack them, at most 254 reliabilities (KF
    takes the graph), a self-loop on every vertex, strongly connected, about 24 sources."""
    g = fg.get(name)
    sc = fg.SCALE[name]
    k = np.rint(g.latency * sc)
    assert np.array_equal(k / sc, g.latency) and k.min() >= 1
    if sc > 1 and name != "frac_thousandths":
        assert not np.array_equal(np.rint(g.latency * (sc // 10)) / (sc // 10), g.latency)   # no smaller scale
    assert (k.max() <= 65535) == (name != "frac_thousandths")
    assert len(np.unique(1.0 - g.packetloss)) <= 254 and len(np.unique(1.0 - g.packetloss)) > 100
    assert np.array_equal(np.unique(g.src[g.src == g.dst]), np.arange(g.n)) and g.n <= 1000
    S = fg.sources(name)
    assert 20 <= len(S) <= 24 and S[0] == 0 and S[-1] == g.n - 1
    R = ref_of(name)
    assert all(np.isfinite(R.dijkstra(int(s))[0]).all() for s in S[:3])
    assert g.directed == (name == "frac_grid_dir")
    pairs = set(zip(R.U.tolist(), R.V.tolist()))
    assert (len(pairs) < len(R.U)) == (name == "frac_multi")
    assert (g.vertex_packetloss is not None) == (name == "frac_cents")
    indeg = np.bincount(R.V, minlength=g.n)
    assert (indeg.max() > WIDE) == (name == "frac_hub")
    if name == "frac_cents":
        has = ~np.isnan(g.vertex_packetloss)
        assert 0.1 < has.mean() < 0.3 and np.all(g.vertex_packetloss[has] > 0)
    if name == "frac_grid_dir":                               # the two arcs of a pair differ in latency
        w = {(u, v): x for u, v, x in zip(R.U.tolist(), R.V.tolist(), R.W.tolist())}
        assert sum(1 for (u, v), x in w.items() if w[v, u] != x) > len(w) // 2
    assert not fg.absorbs(g)


@pytest.mark.parametrize("name", list(fg.SUITE))
def test_ties_and_near_misses(name):
    R = ref_of(name)
    g = fg.get(name)
    indeg = np.bincount(R.V, minlength=g.n)
    key = R.V * g.n + R.U
    uk, c = np.unique(key, return_counts=True)
    twin = np.isin(key, uk[c > 1])
    tied = entries = events = 0
    near = np.zeros(len(R.U), bool)
    for s, d, pa, cnt, fs in base(name):
        tied += sum(1 for x in cnt if x > 1)
        entries += g.n
        cand = d[R.U] + R.W
        miss = (cand != d[R.V]) & (np.abs(cand - d[R.V]) <= 8 * np.spacing(d[R.V])) & (R.V != s)
        events += int(miss.sum())
        near |= miss
    wide, par = int((near & (indeg[R.V] > WIDE)).sum()), int((near & twin).sum())
    print(f"{name}: tied {tied} of {entries} entries ({100.0 * tied / entries:.1f}%), near-miss arcs {int(near.sum())} "
          f"({events} over the sources), on in-lists above {WIDE}: {wide}, with a parallel twin: {par}")
    if name in fg.TIED:
        assert tied >= 0.10 * entries and near.sum() >= 50
    else:
        assert tied < 0.01 * entries                          # the control
    if name == "frac_hub":
        assert wide >= 1
    if name == "frac_multi":
        assert par >= 1


def exact_counts(R, s, scale):
    """The number of shortest paths of every vertex in exact arithmetic over the decimals."""
    import heapq
    n = R.n
    Wx = [Fraction(int(k), scale) for k in np.rint(R.W * scale).tolist()]
    out = [[] for _ in range(n)]
    for a, (u, v) in enumerate(zip(R.U.tolist(), R.V.tolist())):
        out[u].append((v, a))
    d = [None] * n
    d[s] = Fraction(0)
    heap, done, order = [(Fraction(0), s)], [False] * n, []
    while heap:
        du, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        order.append(u)
        for v, a in out[u]:
            x = du + Wx[a]
            if d[v] is None or x < d[v]:
                d[v] = x
                heapq.heappush(heap, (x, v))
    cnt = [0] * n
    cnt[s] = 1
    inn = [[] for _ in range(n)]
    for a, (u, v) in enumerate(zip(R.U.tolist(), R.V.tolist())):
        if v != s and d[u] + Wx[a] == d[v]:
            inn[v].append(u)
    for v in order[1:]:
        cnt[v] = sum(cnt[u] for u in inn[v])
    return cnt


@pytest.mark.parametrize("name", fg.TIED)
def test_paper_ties_are_not_f64_ties(name):
    R = ref_of(name)
    more = fewer = 0
    for s, d, pa, cnt, fs in base(name):
        ex = exact_counts(R, s, fg.SCALE[name])
        more += sum(1 for a, b in zip(ex, cnt) if a > b)
        fewer += sum(1 for a, b in zip(ex, cnt) if a < b)
    print(f"{name}: entries whose exact path count differs from the f64 count: {more + fewer} "
          f"({more} with ties on paper that f64 breaks, {fewer} with fewer on paper)")
    assert more + fewer >= 20


@pytest.mark.parametrize("mutant", ["ulp", "right", "f32"])
@pytest.mark.parametrize("name", fg.TIED)
def test_mutants_differ(name, mutant):
    dp, dc, df = changes(name, mutant)
    print(f"{name} mutant {mutant}: parents {dp}, counts {dc}, latency-sum bits {df} entries changed")
    if name == "frac_hub" and mutant != "f32":
        # Every leaf is adjacent to every hub, so no distance of frac_hub exceeds two biclique
        # hops, 0.6, and the only sum of 0.1, 0.2 and 0.3 up to 0.6 that depends on its association
        # is 0.1 + 0.2 + 0.3 (0.6000000000000001 from the left, 0.6 from the right), which a
        # two-hop route through a hub ties or beats: folding from the target changes nothing here.
        # One ulp of slack admits more tight arcs (counts), but none from a nearer tail (parents).
        assert (dc >= 10) if mutant == "ulp" else (dp, dc, df) == (0, 0, 0)
        return
    assert dp >= 10 and dc >= 10 and df >= 1


@pytest.mark.parametrize("name", fg.TIED)
def test_highest_edge_id_mutant(name):
    """(d): see the module docstring for what Ref(g, tie="high") can change at all."""
    g = fg.get(name)
    R, M = ref_of(name), ref_of(name, "high")
    dpe = dpu = drel = dlat = 0
    for s in fg.sources(name).tolist():
        (_, pe, pu, _), (_, me, mu, _) = R.dijkstra(s), M.dijkstra(s)
        dpe += int(np.count_nonzero(pe != me)); dpu += int(np.count_nonzero(pu != mu))
        a, b = R.row(s), M.row(s)
        dlat += int(np.count_nonzero(a[0] != b[0])); drel += int(np.count_nonzero(a[1] != b[1]))
    print(f"{name} mutant high: parent edges {dpe}, parent vertices {dpu}, reliabilities {drel}, latencies {dlat}")
    assert dpu == 0 and dlat == 0
    if name == "frac_multi":
        assert dpe >= 10 and drel >= 10
    else:
        assert dpe == 0 and drel == 0


# ---- the references among themselves ----------------------------------------------------------------

@pytest.mark.parametrize("name", list(fg.SUITE))
def test_ref_equals_the_oracle(oracle_mod, name):
    """Ref's distances and parent edges are the oracle's min-key Dijkstra, bit for bit; on the
    simple builders so are the rows of OracleGraph.source_rows (on frac_multi that helper replays
    igraph_get_eid per hop, which is no distance: tests/test_multi_graphs.py), the reliabilities
    too where the graph has no vertex loss."""
    g, R = fg.get(name), ref_of(name)
    og = oracle_mod.OracleGraph(g)
    S = fg.sources(name)
    for s in S.tolist():
        d, pe, _, _ = R.dijkstra(s)
        od, op = og.dijkstra(s, oracle_mod.TIE_MINKEY)
        assert np.array_equal(d, od) and np.array_equal(pe, op), (name, s)
    if name != "frac_multi":
        T = np.arange(g.n, dtype=np.int32)
        lat, rel, _ = R.rows(S, T)
        olat, orel = og.source_rows(S, T, oracle_mod.TIE_MINKEY)[:2]
        assert np.array_equal(lat, olat)
        if g.vertex_packetloss is None:
            assert np.array_equal(rel, orel)


@pytest.mark.parametrize("name", list(fg.SUITE))
def test_ecmp_ref_against_exact_fractions(name):
    """ecmp_ref in f64 stays within its own derived tolerance of the same programme in exact
    fractions on the f64-tight DAG."""
    g = fg.get(name)
    E = er.EcmpRef(g)
    S, T = fg.sources(name)[::3], np.arange(g.n)
    got, want = E.rows(S, T), E.rows(S, T, exact=True)
    rtol = E.tol(S)
    print(f"{name}: worst edge error {er.worst(got[0], want[0]):.2f} u, transit {er.worst(got[1], want[1]):.2f} u, "
          f"tolerance {rtol * 2 ** 53:.0f} u")
    assert er.close(got[0], want[0], rtol) and er.close(got[1], want[1], rtol) and got[2] == want[2] == 0


def test_ties_ref_counts_are_the_rule():
    """TiesRef (what the GPU ties are held to) counts what derive() counts."""
    for name in ("frac_grid", "frac_multi"):
        T = TiesRef(fg.get(name))
        for s, d, pa, cnt, fs in base(name)[:4]:
            c = list(T.dag(s)[0])
            assert c == cnt


# ---- link outages and link loss on the builders -------------------------------------------------------

def path_weights(name):
    """The fixed weight block of test_frac_paths_gpu.py: 1 .. 2^40 per (source, vertex)."""
    g = fg.get(name)
    return np.random.default_rng(g.n).integers(1, 1 << 40, size=(len(fg.sources(name)), g.n), dtype=np.uint64)


def outage_scenarios(name):
    """The scenario rule: the edge ids of the reference's route from the first to the last source,
    the first six singly, the first two together, and the empty scenario."""
    S = fg.sources(name)
    es = [int(e) for e in ref_of(name).path(int(S[0]), int(S[-1]))[1]]
    assert es
    return [[e] for e in es[:6]] + ([sorted(es[:2])] if len(es) >= 2 else []) + [[]]


@functools.lru_cache(maxsize=None)
def outage_case(name):
    """(OutageRef, scenarios, the programme's Result) of the builder's sources over every vertex
    under the scenario rule, weighted with path_weights."""
    g = fg.get(name)
    O = orf.OutageRef(g)
    scn = outage_scenarios(name)
    S, T = fg.sources(name), np.arange(g.n, dtype=np.int32)
    return O, scn, O.repair(*orf.block_entries(S, T, path_weights(name)), scn)


def test_outage_scenarios_have_ties_and_ulp_steps():
    """What test_frac_paths_gpu.py relies on: nothing fails, nothing is cut (so every reduced
    graph is connected and has a context), and the scenarios hold tied detours and entries that
    get slower by less than 2^-50."""
    detour, twin, small = [], [], []
    for name in fg.SUITE:
        O, scn, r = outage_case(name)
        st = r.stats.astype(object)
        print(f"{name}: scenarios {scn}, HIT/CUT/SLOWER {st.tolist()}, max_add {r.max_add.tolist()}")
        assert r.codes == frozenset({0}) and r.unrouted == 0 and not np.isnan(r.lat).any()
        assert not r.stats[:, orf.CUT].any() and scn[-1] == [] and not r.stats[-1].any()
        assert 2 <= len(scn) <= 8 and r.stats[:-1, orf.HIT].all()        # (frac_hub's route is one biclique edge)
        for k in range(len(scn) - 1):
            if st[k][orf.HIT] > st[k][orf.SLOWER]:
                detour.append(name)
            if st[k][orf.HIT] > 0 and st[k][orf.SLOWER] == 0:
                twin.append(name)
            if 0 < r.max_add[k] < 2.0 ** -50:
                small.append((name, float(r.max_add[k])))
    assert len(set(detour) & set(fg.TIED)) >= 3 and "frac_multi" in twin
    assert small and ("frac_hub", 2.0 ** -54) in small


@pytest.mark.parametrize("mutant", orf.FRAC_MUTANTS)
def test_outage_mutants_differ(mutant):
    seen = []
    for name in fg.SUITE:
        O, scn, r = outage_case(name)
        S, T = fg.sources(name), np.arange(fg.get(name).n, dtype=np.int32)
        bad = O.repair(*orf.block_entries(S, T, path_weights(name)), scn, mutant=mutant)
        if not bad.same(r):
            seen.append(name)
    print(mutant, seen)
    assert seen, mutant


def test_loss_highest_edge_id_mutant():
    """LossRef over Ref(g, tie="high"): on frac_multi a tight hop with a tied twin of another loss
    changes the expected drops; on a simple builder it cannot."""
    for name, differs in (("frac_multi", True), ("frac_grid", False)):
        g = fg.get(name)
        S, T, W = fg.sources(name), np.arange(g.n, dtype=np.int32), path_weights(name)
        a, b = lr.LossRef(g).block(S, T, W), lr.LossRef(g, tie="high").block(S, T, W)
        same = all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays()))
        assert same != differs, name
        if differs:
            assert not np.array_equal(a.arrays()[1], b.arrays()[1]) and not np.array_equal(a.arrays()[3], b.arrays()[3])


# ---- absorbed latencies: the premise, and the refusal that keeps it ---------------------------------

def chain(w):
    """s(0) -1.0- a(2) -w- b(3) -w- c(1): c has a lower id than a."""
    return Graph(n=4, src=np.array([0, 2, 3], np.int32), dst=np.array([2, 3, 1], np.int32),
                 latency=np.array([1.0, w, w]), packetloss=np.array([1, 2, 3]) / 2.0 ** 21, name=f"chain{w}")


def test_absorbed_latency_breaks_the_premise():
    """With w = 1e-17 the distances of a, b and c are all 1.0 (1.0 + 1e-17 rounds to 1.0): b's
    in-arcs from a and from c are both tight and tie on d[u], the lower vertex id wins, so b and c
    are each other's parents and no chain of parents from b or c reaches the source.  A hop
    counter that follows the parents runs out of rounds, a Kahn sweep never releases the cycle.
    The reference's Dijkstra itself is fine.  With w = 1e-3 nothing of the kind happens."""
    R = Ref(chain(1e-17))
    d, pe, pu, _ = R.dijkstra(0)
    assert d.tolist() == [0.0, 1.0, 1.0, 1.0]
    assert pu.tolist() == [-1, 3, 0, 1]                      # c <- b, a <- s, b <- c
    for v in (1, 3):
        x = v
        for _ in range(R.n):
            x = int(pu[x])
        assert x in (1, 3)                                    # still on the cycle after n steps
    assert fg.absorbs(chain(1e-17))
    g = chain(1e-3)
    R = Ref(g)
    d, pe, pu, _ = R.dijkstra(0)
    assert pu.tolist() == [-1, 3, 0, 2] and d[1] > d[3] > d[2] == 1.0
    lat, rel, hops = R.row(0)                                 # (its own assertion: the fold is the distance)
    assert hops.tolist() == [-1, 3, 1, 2] and R.path(0, 1) == ([0, 2, 3, 1], [0, 1, 2])
    assert not fg.absorbs(g)


def test_the_threshold_is_below_every_absorption():
    """min_w > (n - 1) max_w 2^-52 implies fl(d + w) > d for every distance d a graph can have:
    checked at the largest possible d for the smallest accepted w, on the sizes of the configs."""
    for n, mx in ((4, 1.0), (2000, 250.99), (50000, 250.99), (65535, 65535.0), (10 ** 6, 1e6)):
        thr = (n - 1) * mx * 2.0 ** -52
        w = float(np.nextafter(thr, np.inf))
        top = (n - 1) * mx * (1.0 + 2.0 ** -53) ** n
        for dist in (top, float(np.nextafter(top, 0)), (n - 1) * mx, mx, 1.5 * mx):
            assert dist + w > dist, (n, mx, dist)


@pytest.mark.parametrize("name", ["c2f", "c3f", "c4f"])
def test_configs_pass_the_check(name):
    g = config(name)
    nl = g.src != g.dst
    assert not fg.absorbs(g)
    thr = (g.n - 1) * g.latency[nl].max() * 2.0 ** -52
    print(f"{name}: n {g.n}, largest latency {g.latency[nl].max()}, refused at or below {thr:.3g} ms, smallest "
          f"{g.latency[nl].min()}")
    assert g.latency[nl].min() > 1e5 * thr


def test_create_refuses_an_absorbed_latency():
    """shd_route_create answers SHD_ROUTE_EUNSUPPORTED from its host validation, before it
    touches a device: this needs no GPU and launches nothing.  At the threshold itself too; a
    self-loop does not count (it is never relaxed)."""
    from shadow_amd import route
    route.load_library()
    thr = 3 * 1.0 * 2.0 ** -52
    bad = [chain(1e-17), chain(thr), chain(5e-324)]
    g = chain(1e-3)
    big = Graph(n=4, src=g.src, dst=g.dst, latency=np.array([1e300, 1e283, 1.0]), packetloss=g.packetloss)
    for b in bad + [big]:
        assert fg.absorbs(b)
        with pytest.raises(route.RouteError) as ei:
            route.RouteEngine(b)
        assert ei.value.code == route.EUNSUPPORTED
    assert not fg.absorbs(chain(float(np.nextafter(thr, 1.0))))
