"""The reference of the link edit calls of include/shd_route.h, in plain Python and numpy: no
engine.  A scenario is a list of items: (edge id, latency) gives that edge this latency, (edge id,
inf) removes it, (a, b, latency) adds a link between a and b.  Two independent programmes over
the same entries (s, t, w) and scenarios:

  fresh      the definition: per scenario a multi_ref.Ref of edited(g, scenario) gives the new
             latencies, Ref.path on the graph itself gives hit
  programme  the kernel's steps per source: the old row as the current distances, the live test,
             the marked subtrees below the listed tree arcs (removed or repriced), the seed from
             unmarked tails and the Jacobi pull sweeps over the marked vertices with a listed arc
             at its listed latency and a removed arc left out, then Jacobi rounds that relax every
             new arc and every out-arc of the vertices that fell until a round lowers nothing, the
             entries, the restore.  It records per live (scenario, source) the number of rounds,
             the touched count and the list lengths (EditRef.log).

Both return a Result; tests/test_edit.py holds them bit-equal on everything the GPU tests use.
MUTANTS names the wrong variants of the programme that the tests must see.  The state layout and
the units are the repricing's (tests/reprice_ref.py); the small header mirrors
shadow_amd/csrc/edit_layout.hpp (tests/edit_host_main.cpp holds it to that)."""
from __future__ import annotations

import dataclasses

import numpy as np

from shadow_amd.graph import Graph
from tests import outage_ref as orf
from tests import reprice_ref as rr
from tests.multi_ref import Ref

HIT, CUT, SLOWER, FASTER, NSTAT = 0, 1, 2, 3, 4
ENOEDGE, EUNREACH = orf.ENOEDGE, orf.EUNREACH
MUTANTS = ("new_first_round", "new_one_dir", "new_both_dir", "removal_zero", "removal_push", "cut_is_slower",
           "rescue_failed")
# wrong only in the last bits of a double: held to the fractional builders
FRAC_MUTANTS = ("faster_tol",)
MASK = (1 << 64) - 1

# ---- the layout (edit_layout.hpp over reprice_layout.hpp) ------------------------------------------
ACC, NACC = 104, 7
OLDMIN = ACC + 8 * NACC
LIVE = 192
SMALL = rr.SMALL
fits_lds, lds_max_n, layout_total, state_form, units = rr.fits_lds, rr.lds_max_n, rr.layout_total, rr.state_form, rr.units


# ---- the builders of this feature --------------------------------------------------------------------
def _plain(n, src, dst, lat, name, directed=False):
    return Graph(n=n, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32), latency=np.asarray(lat, np.float64),
                 packetloss=np.zeros(len(src)), directed=directed, name=name)


def path65():
    """The path 0 - 1 - ... - 64 with unit latencies and no chord: a new link (0, 32) at 1 travels
    16 rounds each way through vertices no subtree marks."""
    a = np.arange(64)
    return _plain(65, a, a + 1, np.ones(64), "path65")


def lolli20():
    """The clique 0 .. 5 (latency 2) with the tail 5 - 6 - ... - 19 (latency 1; the edge (v, v + 1)
    has id 15 + v - 5): a removed tail edge cuts what lies behind it, a new link rejoins it."""
    i, j = np.triu_indices(6, 1)
    t = np.arange(5, 19)
    return _plain(20, np.concatenate([i, t]), np.concatenate([j, t + 1]), np.concatenate([np.full(15, 2.0), np.ones(14)]),
                  "lolli20")


def dring12():
    """The directed ring 0 -> 1 -> ... -> 11 -> 0 with unit latencies: a new arc (0, 6) helps the
    sources that reach 0 before 6 and nobody the other way round."""
    a = np.arange(12)
    return _plain(12, a, (a + 1) % 12, np.ones(12), "dring12", directed=True)


def star1100():
    """The hub 0 with the leaves 1 .. 1100 at latency 10 + v % 7: 1,100 new links between
    neighbouring leaves in one scenario are a list longer than the workgroup."""
    leaf = np.arange(1, 1101)
    return _plain(1101, np.zeros(1100, np.int64), leaf, 10.0 + leaf % 7, "star1100")


def dpath9():
    """The directed path 0 -> 1 -> ... -> 8 (CPU only: no context takes a graph that is not
    strongly connected): no vertex reaches a lower one, a new arc (8, 0) would."""
    a = np.arange(8)
    return _plain(9, a, a + 1, np.ones(8), "dpath9", directed=True)


BUILDERS = {"path65": path65, "lolli20": lolli20, "dring12": dring12, "star1100": star1100, "dpath9": dpath9}


# ---- scenarios -----------------------------------------------------------------------------------------
def split(scenario):
    """(F: id -> latency of the listed edges, inf = removed; N: the new links (a, b, latency) in
    their order) of a scenario's items."""
    F, N = {}, []
    for it in scenario:
        if len(it) == 2:
            assert int(it[0]) not in F, "an id repeated within one scenario"
            F[int(it[0])] = float(it[1])
        else:
            N.append((int(it[0]), int(it[1]), float(it[2])))
    return F, N


def pack(scenarios, sort=False):
    """(off int64 [nscn + 1], edge int32, a int32, b int32, lat float64) of a list of scenarios, as
    given or each in the order the async call asks for: new links first, then ids ascending."""
    off = np.zeros(len(scenarios) + 1, np.int64)
    rec = []
    for k, f in enumerate(scenarios):
        off[k + 1] = off[k] + len(f)
        one = [(-1, it[0], it[1], it[2]) if len(it) == 3 else (it[0], 0, 0, it[1]) for it in f]
        rec += sorted(one, key=lambda r: r[0]) if sort else one          # stable: the new links keep their order
    col = lambda i, t: np.array([r[i] for r in rec], t)
    return off, col(0, np.int32), col(1, np.int32), col(2, np.int32), col(3, np.float64)


def edited(g, scenario):
    """G_k: g without the removed edges, the others in their order with the repriced latencies
    replaced, the new links appended in list order (no loss)."""
    F, N = split(scenario)
    lat = np.array(g.latency, np.float64)
    keep = np.ones(g.m, bool)
    for e, w in F.items():
        if np.isinf(w):
            keep[e] = False
        else:
            lat[e] = w
    cat = lambda old, new, t: np.concatenate([np.asarray(old)[keep], np.asarray(new, t)]).astype(t)
    return dataclasses.replace(g, src=cat(g.src, [a for a, _, _ in N], np.int32), dst=cat(g.dst, [b for _, b, _ in N], np.int32),
                               latency=cat(lat, [w for _, _, w in N], np.float64),
                               packetloss=cat(g.packetloss, [0.0] * len(N), np.float64), name=g.name + "_edited")


def connected(g):
    """every vertex reaches every other (strongly, on a directed graph)"""
    def reach(src, dst):
        adj = [[] for _ in range(g.n)]
        for a, b in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
            adj[a].append(b)
            if not g.directed:
                adj[b].append(a)
        seen, stack = {0}, [0]
        while stack:
            for v in adj[stack.pop()]:
                if v not in seen:
                    seen.add(v)
                    stack.append(v)
        return len(seen) == g.n
    return reach(g.src, g.dst) and (not g.directed or reach(g.dst, g.src))


@dataclasses.dataclass
class Result:
    stats: np.ndarray      # uint64 (nscn, NSTAT)
    max_add: np.ndarray    # float64 (nscn,)
    max_gain: np.ndarray   # float64 (nscn,)
    min_new: np.ndarray    # float64 (nscn,), +inf without an entry routed in G and in G_k
    lat: np.ndarray        # float64 (nscn, entries), NaN = cut or failed in the graph itself
    unrouted: int
    codes: frozenset       # the codes the call may return: {0} or the per-entry codes met

    def same(self, other):
        return (np.array_equal(self.stats, other.stats) and np.array_equal(self.max_add, other.max_add) and
                np.array_equal(self.max_gain, other.max_gain) and np.array_equal(self.min_new, other.min_new) and
                np.array_equal(self.lat, other.lat, equal_nan=True) and self.unrouted == other.unrouted and
                self.codes == other.codes)


class _Acc:
    def __init__(self, ns, ne):
        self.stats = np.zeros((ns, NSTAT), np.uint64)
        self.mx, self.mg, self.mn = np.zeros(ns), np.zeros(ns), np.full(ns, np.inf)
        self.lat = np.full((ns, ne), np.nan)
        self.acc = [0] * NSTAT

    def entry(self, k, x, w, hit, o, nw, mutant=None):
        """nw: the new latency, inf or NaN where G_k has no route"""
        if hit:
            self.acc[HIT] += w
        if np.isnan(nw) or np.isinf(nw):
            self.acc[CUT] += w
            if mutant == "cut_is_slower":
                self.acc[SLOWER] += w
            return
        self.lat[k, x] = nw
        if nw > o:
            self.acc[SLOWER] += w
            self.mx[k] = max(self.mx[k], nw - o)
        elif (nw < o - 1e-12) if mutant == "faster_tol" else (nw < o):
            self.acc[FASTER] += w
            self.mg[k] = max(self.mg[k], o - nw)
        self.mn[k] = min(self.mn[k], nw)

    def close(self, k):
        self.stats[k] = [a & MASK for a in self.acc]
        self.acc = [0] * NSTAT


class EditRef:
    def __init__(self, g):
        self.g, self.n = g, int(g.n)
        self.rp = rr.RepriceRef(g)
        self.base = self.rp.base                              # the graph itself: old entries, trees, in-arcs
        self.src, self.dst, self.lat = self.base.src, self.base.dst, self.base.lat
        self.loops, self.outarcs = self.base.loops, self.rp.outarcs
        self.seen = set()                                     # the coverage conditions met so far
        self.log = []                                         # per live (scenario, source) of the last call
        self._fresh = {}

    def old(self, s, t):
        return self.base.old(s, t)

    # ---- fresh ----------------------------------------------------------------------------------
    def _ref_of(self, sc):
        key = tuple(tuple(it) for it in sc)
        if key not in self._fresh:
            if len(self._fresh) > 64:
                self._fresh.clear()
            self._fresh[key] = Ref(edited(self.g, sc)) if key else self.base.ref
        return self._fresh[key]

    def fresh(self, S, T, W, scenarios):
        W, olds, un, codes = self.base._split(S, T, W)
        A = _Acc(len(scenarios), len(S))
        for k, sc in enumerate(scenarios):
            F, _ = split(sc)
            Rk = self._ref_of(sc)
            rows = {}
            for x, (s, t, w) in enumerate(zip(S, T, W.tolist())):
                o, es = olds[x]
                if es is None:
                    continue
                s, t = int(s), int(t)
                if s == t:
                    nw = Rk.self_entry(s)[0]
                else:
                    if s not in rows:
                        rows[s] = Rk.dijkstra(s)[0]
                    nw = rows[s][t]
                A.entry(k, x, w, any(e in F for e in es), o, nw)
            A.close(k)
        return Result(A.stats, A.mx, A.mg, A.mn, A.lat, un, codes)

    # ---- the programme ----------------------------------------------------------------------------
    def _one(self, s, F, N, mutant):
        """(current distances, marked set, live) of source s under the listed edges F and the new
        links N."""
        d, pe, pu, hops, order = self.base._tree(s)
        directed = bool(self.g.directed)
        ids = sorted(F)
        NA = []                                               # the new arcs
        for a, b, w in N:
            NA.append((a, b, w))
            if (not directed and mutant != "new_one_dir") or (directed and mutant == "new_both_dir"):
                NA.append((b, a, w))

        def arcs_of(e):
            a, b = int(self.src[e]), int(self.dst[e])
            if a == b:
                return []
            return [(a, b)] if directed else [(a, b), (b, a)]

        def wk(e, w, pull):
            """the latency of an arc over edge e in G_k; None = G_k does not have it"""
            if e not in F:
                return w
            if np.isinf(F[e]):
                if mutant == "removal_zero":
                    return 0.0
                if mutant == "removal_push" and not pull:
                    return w
                return None
            return F[e]

        # 1. the live test
        live, roots = False, set()
        for e in ids:
            if int(self.src[e]) == int(self.dst[e]):
                live |= bool(self.loops[s]) and self.loops[s][0] == e
                continue
            for a, b in arcs_of(e):
                if pe[b] == e and pu[b] == a:
                    roots.add(b)
                if np.isfinite(F[e]) and d[a] + F[e] < d[b]:
                    live = True
        for a, b, w in NA:
            if d[a] + w < d[b]:
                live = True
        live |= bool(roots)
        if not live:
            return d, set(), False
        cur = d.copy()
        # 2. mark
        mark, A = set(), []
        if roots:
            d0 = min(int(hops[r]) for r in roots)
            for v in order:
                if hops[v] >= d0 and (v in roots or int(pu[v]) in mark):
                    mark.add(v)
                    A.append(v)
        # 3. seed and sweeps over the marked set
        for v in A:
            best = np.inf
            for u, e, w in self.base.inarcs[v]:
                if u in mark or np.isinf(d[u]):
                    continue
                x = wk(e, w, True)
                if x is not None:
                    best = min(best, d[u] + x)
            cur[v] = best
        sweeps = 0
        while A:
            prev, changed = cur.copy(), False
            for v in A:
                for u, e, w in self.base.inarcs[v]:
                    x = wk(e, w, True) if u in mark else None
                    if x is not None and prev[u] + x < cur[v]:
                        cur[v] = prev[u] + x
                        changed = True
            sweeps += 1
            assert sweeps <= len(A) + 1
            if not changed:
                break
        swept = cur.copy()
        # 4. propagate: the first frontier, then the rounds
        touched = set(A)
        frontier = [v for v in A if cur[v] < d[v]]
        inf = set(frontier)
        for e in ids:
            x = wk(e, self.lat[e], False)
            if x is None:                                     # removed: no arc of G_k
                continue
            for a, b in arcs_of(e):
                if cur[a] + x < cur[b]:
                    cur[b] = cur[a] + x
                    touched.add(b)
                    if b not in inf:
                        inf.add(b)
                        frontier.append(b)
        rec = {"rounds": 0, "marked": len(A), "frontier": len(frontier), "new": len(NA), "outside": False}
        while True:
            assert rec["rounds"] <= self.n + 1
            prev, low = cur.copy(), set()
            if not (mutant == "new_first_round" and rec["rounds"] > 0):
                for a, b, w in NA:
                    if prev[a] + w < cur[b]:
                        cur[b] = prev[a] + w
                        low.add(b)
            for v in frontier:
                for h, e, w in self.outarcs[v]:
                    x = wk(e, w, False)
                    if x is not None and prev[v] + x < cur[h]:
                        cur[h] = prev[v] + x
                        low.add(h)
            if not low:
                break
            rec["rounds"] += 1
            rec["outside"] |= any(h not in mark for h in low)
            rec["frontier"] = max(rec["frontier"], len(low))
            touched |= low
            frontier = sorted(low)
        rec["touched"] = len(touched)
        assert len(touched) <= self.n
        self.log.append(rec)
        if any(np.isinf(swept[v]) and np.isfinite(cur[v]) for v in A):
            self.seen.add("marked_through_new_link")          # no surviving in-arc of G, only a new link
        return cur, mark, True

    def programme(self, S, T, W, scenarios, mutant=None):
        W, olds, un, codes = self.base._split(S, T, W)
        A = _Acc(len(scenarios), len(S))
        self.log = []
        by_src = {}
        for x, s in enumerate(S):
            by_src.setdefault(int(s), []).append(x)
        for k, sc in enumerate(scenarios):
            F, N = split(sc)
            lives = set()
            for s, xs in by_src.items():
                cur, mark, live = self._one(s, F, N, mutant)
                lives.add(live)
                for x in xs:
                    o, es = olds[x]
                    t, w = int(T[x]), int(W[x])
                    if es is None:
                        if mutant == "rescue_failed" and t != s and np.isfinite(cur[t]):
                            A.lat[k, x] = cur[t]
                        continue
                    if t == s:
                        e = self.loops[s][0]
                        hit = e in F
                        nw = o
                        if hit:
                            left = [F.get(x2, self.lat[x2]) for x2 in self.loops[s]]
                            left = [x2 for x2 in left if np.isfinite(x2)]
                            nw = left[0] if left else np.nan
                            if np.isinf(F[e]):
                                self.seen.add("loop_removed_with_second" if len(self.loops[s]) > 1 else "loop_removed_alone")
                    else:
                        nw, hit = cur[t], t in mark
                    A.entry(k, x, w, hit, o, nw, mutant)
            if lives == {True, False}:
                self.seen.add("dead_and_live")
            A.close(k)
        return Result(A.stats, A.mx, A.mg, A.mn, A.lat, un, codes)


block_entries = orf.block_entries
