"""The reference of the link repricing calls of include/shd_route.h, in plain Python and numpy: no
engine.  Two independent programmes over the same entries (s, t, w) and scenarios (lists of
(edge id, new latency) pairs):

  fresh      the definition: per scenario a multi_ref.Ref of the graph with the listed latencies
             replaced gives the new latencies, Ref.path on the graph itself gives hit
  programme  the kernel's steps per source: the old row as the current distances, the live test,
             the marked subtrees below the listed tree arcs, the seed from unmarked tails and the
             Jacobi pull sweeps over the marked vertices with a listed arc at its new latency,
             then Jacobi push rounds from the vertices that fell until a round lowers nothing,
             the entries, the restore.  It records per call the number of propagation rounds, the
             touched count and the list lengths (RepriceRef.log).

Both return a Result; tests/test_reprice.py holds them bit-equal on everything the GPU tests use.
MUTANTS names the wrong variants of the programme that the tests must see.  The layout mirrors
shadow_amd/csrc/reprice_layout.hpp (tests/reprice_layout_main.cpp holds it to that); the units
are the outage calls' (tests/outage_ref.py)."""
from __future__ import annotations

import dataclasses

import numpy as np

from shadow_amd.graph import Graph
from tests import outage_ref as orf
from tests.multi_ref import Ref

HIT, SLOWER, FASTER, NSTAT = 0, 1, 2, 3
ENOEDGE, EUNREACH = orf.ENOEDGE, orf.EUNREACH
MUTANTS = ("raise_is_outage", "sweeps_old_weight", "marked_only", "one_round", "one_arc", "hit_is_changed",
           "dead_no_lowered")
# wrong only in the last bits of a double: held to the fractional builders
FRAC_MUTANTS = ("faster_tol",)
MASK = (1 << 64) - 1

# ---- the layout (reprice_layout.hpp) ---------------------------------------------------------------
LDS_BUDGET = orf.LDS_BUDGET
SLAB_MAX = orf.SLAB_MAX
SMALL = 192 + 4 * SLAB_MAX + SLAB_MAX
a16 = orf.a16
units = orf.units


def words(n):
    return (n + 31) // 32


def layout_offsets(n, tsize):
    """(d, lvl, order, tch, fr0, fr1, mark, tbit, fbit, total) of the state of n vertices."""
    o, out = 0, []
    for b in (8 * n, 4 * (n + 1), tsize * n, tsize * n, tsize * n, tsize * n, n, 4 * words(n), 4 * words(n)):
        out.append(o)
        o += a16(b)
    return (*out, o)


def layout_total(n, tsize=2):
    return layout_offsets(n, tsize)[-1]


def fits_lds(n):
    return n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET


def lds_max_n():
    lo, hi = 1, 65535
    while lo < hi:                                    # the total rises with n
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits_lds(mid) else (lo, mid - 1)
    return lo


def state_form(n, nunits, knob_off, slot_budget):
    """(form, grid, lds, stride, slots) as path_host.hpp's state_form gives them for the
    repricing kernel: form 1 LDS, 2 HBM u16, 3 HBM u32."""
    if fits_lds(n) and not knob_off:
        return 1, min(nunits, 1024), SMALL + layout_total(n, 2), 0, 0
    stride = a16(layout_total(n, 2 if n <= 65535 else 4))
    slots = max(16, min(512, slot_budget // stride))
    return (2 if n <= 65535 else 3), min(nunits, slots), SMALL, stride, slots


# ---- the builders of this feature --------------------------------------------------------------------
def _plain(n, src, dst, lat, name):
    return Graph(n=n, src=np.asarray(src, np.int32), dst=np.asarray(dst, np.int32), latency=np.asarray(lat, np.float64),
                 packetloss=np.zeros(len(src)), name=name)


def chord65():
    """The path 0 - 1 - ... - 64 with unit latencies and the chord (0, 32) at latency 100 (edge
    64): lowered to 1, its gain travels 32 rounds through vertices no subtree marks."""
    a = np.arange(64)
    return _plain(65, np.append(a, 0), np.append(a + 1, 32), np.append(np.ones(64), 100.0), "chord65")


def hub1100():
    """Source 0 - hub 1 - the leaves 2 .. 1101: the edge (0, 1) at latency 50 (edge 0), the
    leaves at 1 + v % 7, and as the last edge a parallel (0, 1) at latency 60, which no tree
    takes.  Lowering edge 0 marks everything; lowering the parallel edge marks nothing, its first
    frontier is the hub with 1,101 out-arcs and the second the 1,100 leaves."""
    leaf = np.arange(2, 1102)
    src = np.concatenate([[0], np.ones(1100, np.int64), [0]])
    dst = np.concatenate([[1], leaf, [1]])
    lat = np.concatenate([[50.0], 1.0 + leaf % 7, [60.0]])
    return _plain(1102, src, dst, lat, "hub1100")


def layers48():
    """Source 0, a feeder 1 and four layers of 48 vertices, complete between neighbouring
    layers (latencies 10 + (i + 2 j) % 7): the source reaches the first layer at 10 each, the
    feeder joins every vertex of the first layer at 1 and the source at 100 (the last edge, no
    tree arc).  Lowered to 1 it improves the feeder, then all 48 of the first layer, and each
    vertex of the next layer is then improved by 48 tails in one round."""
    L = [np.arange(2 + 48 * k, 2 + 48 * (k + 1)) for k in range(4)]
    src, dst, lat = [np.zeros(48, np.int64)], [L[0]], [np.full(48, 10.0)]
    src.append(np.ones(48, np.int64)); dst.append(L[0]); lat.append(np.ones(48))
    i, j = np.meshgrid(np.arange(48), np.arange(48), indexing="ij")
    for k in range(3):
        src.append(L[k][i.ravel()]); dst.append(L[k + 1][j.ravel()]); lat.append(10.0 + (i.ravel() + 2 * j.ravel()) % 7)
    src.append(np.array([0])); dst.append(np.array([1])); lat.append(np.array([100.0]))
    return _plain(194, np.concatenate(src), np.concatenate(dst), np.concatenate(lat), "layers48")


BUILDERS = {"chord65": chord65, "hub1100": hub1100, "layers48": layers48}


# ---- scenarios -----------------------------------------------------------------------------------------
def pack(scenarios, sort=False):
    """(off int64 [nscn + 1], edge int32, lat float64) of a list of (id, latency) lists, as given
    or each sorted by id."""
    off = np.zeros(len(scenarios) + 1, np.int64)
    for k, f in enumerate(scenarios):
        off[k + 1] = off[k] + len(f)
    flat = [p for f in scenarios for p in (sorted(f) if sort else f)]
    return off, np.array([e for e, _ in flat], np.int32), np.array([w for _, w in flat], np.float64)


def repriced(g, scenario):
    """g with the listed latencies replaced, everything else as it is."""
    lat = np.array(g.latency, np.float64)
    for e, w in scenario:
        lat[int(e)] = w
    return dataclasses.replace(g, latency=lat, name=g.name + "_repriced")


@dataclasses.dataclass
class Result:
    stats: np.ndarray      # uint64 (nscn, NSTAT)
    max_add: np.ndarray    # float64 (nscn,)
    max_gain: np.ndarray   # float64 (nscn,)
    min_new: np.ndarray    # float64 (nscn,), +inf without a routed entry
    lat: np.ndarray        # float64 (nscn, entries), NaN = failed in the graph itself
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
        self.acc = [0, 0, 0]

    def entry(self, k, x, w, hit, o, nw, tol=False):
        self.lat[k, x] = nw
        if hit:
            self.acc[HIT] += w
        if nw > o:
            self.acc[SLOWER] += w
            self.mx[k] = max(self.mx[k], nw - o)
        elif (nw < o - 1e-12) if tol else (nw < o):
            self.acc[FASTER] += w
            self.mg[k] = max(self.mg[k], o - nw)
        self.mn[k] = min(self.mn[k], nw)

    def close(self, k):
        self.stats[k] = [a & MASK for a in self.acc]
        self.acc = [0, 0, 0]


class RepriceRef:
    def __init__(self, g):
        self.g, self.n = g, int(g.n)
        self.base = orf.OutageRef(g)                          # the graph itself: old entries, trees, in-arcs
        self.src, self.dst, self.lat = self.base.src, self.base.dst, self.base.lat
        self.loops = self.base.loops
        self.outarcs = [[] for _ in range(self.n)]            # (head, edge id, latency) of every out-arc
        for v in range(self.n):
            for u, e, w in self.base.inarcs[v]:
                self.outarcs[u].append((v, e, w))
        self.seen = set()                                     # the coverage conditions met so far
        self.log = []                                         # per live (scenario, source) of the last call
        self._fresh = {}

    def old(self, s, t):
        return self.base.old(s, t)

    # ---- fresh ----------------------------------------------------------------------------------
    def _ref_of(self, F):
        key = tuple(sorted(F.items()))
        if key not in self._fresh:
            if len(self._fresh) > 64:
                self._fresh.clear()
            self._fresh[key] = Ref(repriced(self.g, key)) if key else self.base.ref
        return self._fresh[key]

    def fresh(self, S, T, W, scenarios):
        W, olds, un, codes = self.base._split(S, T, W)
        ns = len(scenarios)
        A = _Acc(ns, len(S))
        for k, sc in enumerate(scenarios):
            F = {int(e): float(w) for e, w in sc}
            Rk = self._ref_of(F)
            for x, (s, t, w) in enumerate(zip(S, T, W.tolist())):
                o, es = olds[x]
                if es is None:
                    continue
                s, t = int(s), int(t)
                nw = Rk.self_entry(s)[0] if s == t else Rk.dijkstra(s)[0][t]
                A.entry(k, x, w, any(e in F for e in es), o, nw)
            A.close(k)
        return Result(A.stats, A.mx, A.mg, A.mn, A.lat, un, codes)

    # ---- the programme ----------------------------------------------------------------------------
    def _one(self, s, F, mutant):
        """(current distances, marked set, live) of source s under the scenario F (id -> latency)."""
        d, pe, pu, hops, order = self.base._tree(s)
        directed = bool(self.g.directed)
        ids = sorted(F)

        def arcs_of(e):
            a, b = int(self.src[e]), int(self.dst[e])
            if a == b:
                return []
            return [(a, b)] if directed or mutant == "one_arc" else [(a, b), (b, a)]

        def wk(u, v, e, w, pull=False):
            """the latency of the arc u -> v over edge e in G_k; None = the arc is left out"""
            if e not in F or (u, v) not in arcs_of(e):
                return w
            if mutant == "raise_is_outage" and F[e] > w:
                return None
            if mutant == "sweeps_old_weight" and pull:
                return w
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
                if mutant != "dead_no_lowered" and d[a] + F[e] < d[b]:
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
                x = wk(u, v, e, w, pull=True)
                if x is not None:
                    best = min(best, d[u] + x)
            cur[v] = best
        sweeps = 0
        while A:
            prev, changed = cur.copy(), False
            for v in A:
                for u, e, w in self.base.inarcs[v]:
                    x = wk(u, v, e, w, pull=True) if u in mark else None
                    if x is not None and prev[u] + x < cur[v]:
                        cur[v] = prev[u] + x
                        changed = True
            sweeps += 1
            assert sweeps <= len(A) + 1
            if not changed:
                break
        # 4. propagate
        touched = set(A)
        frontier = [v for v in A if cur[v] < d[v]]
        inf = set(frontier)
        for e in ids:
            for a, b in arcs_of(e):
                x = wk(a, b, e, self.lat[e])
                if x is None or (mutant == "marked_only" and b not in mark):
                    continue
                if cur[a] + x < cur[b]:
                    cur[b] = cur[a] + x
                    touched.add(b)
                    if b not in inf:
                        inf.add(b)
                        frontier.append(b)
        rec = {"rounds": 0, "marked": len(A), "frontier": len(frontier), "fan": 0, "tails": 0, "outside": False}
        while frontier:
            assert rec["rounds"] <= self.n
            prev, nxt, tails = cur.copy(), [], {}
            for v in frontier:
                rec["fan"] = max(rec["fan"], len(self.outarcs[v]))
                for h, e, w in self.outarcs[v]:
                    x = wk(v, h, e, w)
                    if x is None or (mutant == "marked_only" and h not in mark):
                        continue
                    if prev[v] + x < prev[h]:
                        tails[h] = tails.get(h, 0) + 1
                    if prev[v] + x < cur[h]:
                        cur[h] = prev[v] + x
                        touched.add(h)
                        if h not in mark:
                            rec["outside"] = True
            nxt = [h for h in tails if cur[h] < prev[h]]
            assert len(nxt) == len(set(nxt)) <= self.n
            rec["rounds"] += 1
            rec["tails"] = max([rec["tails"], *tails.values()])
            rec["frontier"] = max(rec["frontier"], len(nxt))
            frontier = nxt
            if mutant == "one_round":
                break
        rec["touched"] = len(touched)
        assert len(touched) <= self.n
        self.log.append(rec)
        # what the scenario shows
        for r in roots:
            e, u = int(pe[r]), int(pu[r])
            if F[e] > self.lat[e] and cur[r] == cur[u] + F[e] and cur[r] > d[r] and \
                    all(cur[a] + (F[x] if x in F else w) > cur[r] for a, x, w in self.base.inarcs[r] if x != e):
                self.seen.add("raised_still_crossed")
            if F[e] < self.lat[e]:
                self.seen.add("lowered_tree_arc")
        return cur, mark, True

    def programme(self, S, T, W, scenarios, mutant=None):
        W, olds, un, codes = self.base._split(S, T, W)
        ns = len(scenarios)
        A = _Acc(ns, len(S))
        self.log = []
        by_src = {}
        for x, s in enumerate(S):
            by_src.setdefault(int(s), []).append(x)
        for k, sc in enumerate(scenarios):
            F = {int(e): float(w) for e, w in sc}
            assert len(F) == len(sc), "an id repeated within one scenario"
            lives = set()
            for s, xs in by_src.items():
                cur, mark, live = self._one(s, F, mutant)
                lives.add(live)
                for x in xs:
                    o, es = olds[x]
                    if es is None:
                        continue
                    t, w = int(T[x]), int(W[x])
                    if t == s:
                        e = self.loops[s][0]
                        nw, hit = F.get(e, self.lat[e]), e in F
                        if hit:
                            self.seen.add("loop_with_second" if len(self.loops[s]) > 1 else "loop_alone")
                    else:
                        nw, hit = cur[t], t in mark
                        if not hit and nw < o:
                            self.seen.add("unhit_faster")
                        if hit and nw < o:
                            self.seen.add("hit_faster")
                    if mutant == "hit_is_changed":
                        hit = not (nw == o)
                    A.entry(k, x, w, hit, o, nw, tol=mutant == "faster_tol")
            if lives == {True, False}:
                self.seen.add("dead_and_live")
            A.close(k)
        return Result(A.stats, A.mx, A.mg, A.mn, A.lat, un, codes)


block_entries = orf.block_entries
