"""The reference of the link outage calls of include/shd_route.h, in plain Python and numpy: no
engine.  Two independent programmes over the same entries (s, t, w) and scenarios (lists of
edge ids):

  fresh    the definition: per scenario a multi_ref.Ref of the reduced graph (the kept edges in
           their order) gives the new latencies, Ref.path on the whole graph gives hit
  repair   the kernel's programme per source: the tree of the whole graph, per scenario the roots
           (vertices whose parent arc failed), the marked subtrees top-down in level order, the
           seed from unmarked reached tails, Jacobi pull sweeps over the marked vertices until
           nothing changes, then the entries

Both return a Result; tests/test_outage.py holds them bit-equal on everything the GPU tests use.
MUTANTS names the wrong variants of repair that the tests must see.  The layout and unit
arithmetic mirror shadow_amd/csrc/outage_layout.hpp (tests/outage_layout_main.cpp holds them to
it)."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests.multi_ref import Ref

HIT, CUT, SLOWER, NSTAT = 0, 1, 2, 3
ENOEDGE, EUNREACH = -4, -5         # SHD_ROUTE_ENOEDGE, SHD_ROUTE_EUNREACH (checked in test_outage.py)
MUTANTS = ("roots_only", "seed_marked", "one_sweep", "one_arc", "hit_is_changed")
# wrong only in the last bits of a double, which integer latencies never show: tests/test_frac_graphs.py
# holds them to the fractional builders.  slower_tol judges SLOWER as new > old + 1e-12;
# root_offset rebuilds the distance of a marked vertex below its root as
# dnew[root] + (old[v] - old[root]) wherever the vertex keeps its way down from the root (the
# shifted value lies within 4 ulp of the left fold), instead of taking the left fold itself
FRAC_MUTANTS = ("slower_tol", "root_offset")
MASK = (1 << 64) - 1

# ---- the layout and the units (outage_layout.hpp) -------------------------------------------------
LDS_BUDGET = 160 * 1024
SLAB_MAX = 1024
UNITS = 1024
SMALL = 128 + 4 * SLAB_MAX + SLAB_MAX


def a16(x):
    return (x + 15) & ~15


def layout_offsets(n, tsize):
    """(dnew, lvl, order, aff, mark, total) of the state of n vertices, T of tsize bytes."""
    o, out = 0, []
    for b in (8 * n, 4 * (n + 1), tsize * n, tsize * n, n):
        out.append(o)
        o += a16(b)
    return (*out, o)


def layout_total(n, tsize=2):
    return layout_offsets(n, tsize)[-1]


def fits_lds(n):
    return n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET


def lds_max_n():
    n = 1
    while fits_lds(n + 1):
        n += 1
    return n


def units(k, nscn):
    """(slab, nslab, units) of k sources and nscn scenarios."""
    if nscn <= 0:
        return 1, 1, k
    per = (UNITS + k - 1) // max(k, 1)
    slab = min(max((nscn + per - 1) // per, 1), SLAB_MAX)
    nslab = (nscn + slab - 1) // slab
    return slab, nslab, k * nslab


def state_form(n, nunits, knob_off, slot_budget):
    """(form, grid, lds, stride, slots) as path_host.hpp's state_form gives them for the outage
    kernel: form 1 LDS, 2 HBM u16, 3 HBM u32."""
    if n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET and not knob_off:
        return 1, min(nunits, 1024), SMALL + layout_total(n, 2), 0, 0
    stride = a16(layout_total(n, 2 if n <= 65535 else 4))
    slots = max(16, min(512, slot_budget // stride))
    return (2 if n <= 65535 else 3), min(nunits, slots), SMALL, stride, slots


# ---- scenarios -----------------------------------------------------------------------------------
def pack(scenarios):
    """(off int64 [nscn + 1], edge int32) of a list of id lists, ids as given."""
    off = np.zeros(len(scenarios) + 1, np.int64)
    for k, f in enumerate(scenarios):
        off[k + 1] = off[k] + len(f)
    edge = np.array([e for f in scenarios for e in f], np.int32)
    return off, edge


def reduced(g, failed):
    """g without the edges `failed`, the others in their order."""
    keep = np.ones(g.m, bool)
    keep[np.asarray(list(failed), np.int64)] = False
    return dataclasses.replace(g, src=np.asarray(g.src)[keep], dst=np.asarray(g.dst)[keep],
                               latency=np.asarray(g.latency, np.float64)[keep],
                               packetloss=np.asarray(g.packetloss, np.float64)[keep], name=g.name + "_cut")


@dataclasses.dataclass
class Result:
    stats: np.ndarray      # uint64 (nscn, NSTAT)
    max_add: np.ndarray    # float64 (nscn,)
    lat: np.ndarray        # float64 (nscn, entries), NaN = cut or failed in the whole graph
    unrouted: int
    codes: frozenset       # the codes the call may return: {0} or the per-entry codes met

    def same(self, other):
        return (np.array_equal(self.stats, other.stats) and np.array_equal(self.max_add, other.max_add) and
                np.array_equal(self.lat, other.lat, equal_nan=True) and self.unrouted == other.unrouted and
                self.codes == other.codes)


class OutageRef:
    def __init__(self, g):
        self.g, self.n = g, int(g.n)
        self.ref = Ref(g)
        self.src, self.dst = np.asarray(g.src, np.int64), np.asarray(g.dst, np.int64)
        self.lat = np.asarray(g.latency, np.float64)
        self.loops = [[] for _ in range(self.n)]
        for e in np.flatnonzero(self.src == self.dst).tolist():
            self.loops[int(self.src[e])].append(e)
        R = self.ref
        self.inarcs = [[] for _ in range(self.n)]           # (tail, edge id, latency) of every in-arc
        for u, v, e, w in zip(R.U.tolist(), R.V.tolist(), R.E.tolist(), R.W.tolist()):
            self.inarcs[v].append((u, e, w))
        self.seen = set()                                     # the coverage conditions met so far
        self._fresh = {}
        self._trees = {}

    # ---- the whole graph ----------------------------------------------------------------------
    def old(self, s, t):
        """(latency, edges of the route) of the entry in the whole graph; (nan, None) if it fails."""
        s, t = int(s), int(t)
        if s == t:
            return (self.lat[self.loops[s][0]], [self.loops[s][0]]) if self.loops[s] else (np.nan, None)
        d, pe, pu, _ = self.ref.dijkstra(s)
        if pu[t] < 0:
            return np.nan, None
        return d[t], self.ref.path(s, t)[1]

    def _split(self, S, T, W):
        """The entries that take part, and unrouted and the codes of those that fail."""
        W = np.ones(len(S), np.uint64) if W is None else np.asarray(W, np.uint64)
        un, codes, olds = 0, set(), []
        for s, t, w in zip(S, T, W.tolist()):
            o = self.old(s, t)
            olds.append(o)
            if o[1] is None:
                un += w
                codes.add(ENOEDGE if int(s) == int(t) else EUNREACH)
        return W, olds, un & MASK, frozenset(codes or {0})

    # ---- fresh ----------------------------------------------------------------------------------
    def _reduced_ref(self, F):
        key = tuple(sorted(set(F)))
        if key not in self._fresh:
            if len(self._fresh) > 64:
                self._fresh.clear()
            self._fresh[key] = Ref(reduced(self.g, key)) if key else self.ref
        return self._fresh[key]

    def fresh(self, S, T, W, scenarios):
        W, olds, un, codes = self._split(S, T, W)
        ns = len(scenarios)
        stats, mx, lat = np.zeros((ns, NSTAT), np.uint64), np.zeros(ns), np.full((ns, len(S)), np.nan)
        for k, F in enumerate(scenarios):
            Fs = set(int(e) for e in F)
            Rk = self._reduced_ref(Fs)
            acc = [0, 0, 0]
            for x, (s, t, w) in enumerate(zip(S, T, W.tolist())):
                o, es = olds[x]
                if es is None:
                    continue
                s, t = int(s), int(t)
                if any(e in Fs for e in es):
                    acc[HIT] += w
                if s == t:
                    nw = Rk.self_entry(s)[0]
                else:
                    nw = Rk.dijkstra(s)[0][t]
                    nw = np.nan if np.isinf(nw) else nw
                lat[k, x] = nw
                if np.isnan(nw):
                    acc[CUT] += w
                elif nw > o:
                    acc[SLOWER] += w
                    mx[k] = max(mx[k], nw - o)
            stats[k] = [a & MASK for a in acc]
        return Result(stats, mx, lat, un, codes)

    # ---- repair ---------------------------------------------------------------------------------
    def _tree(self, s):
        if s in self._trees:
            return self._trees[s]
        d, pe, pu, _ = self.ref.dijkstra(s)
        hops = np.full(self.n, -1, np.int64)
        hops[s] = 0
        for v in np.argsort(d, kind="stable").tolist():      # a parent is strictly nearer (w > 0)
            if v != s and pu[v] >= 0:
                hops[v] = hops[pu[v]] + 1
        order = [v for v in np.argsort(hops, kind="stable").tolist() if hops[v] > 0]
        if len(self._trees) > 64:
            self._trees.clear()
        self._trees[s] = (d, pe, pu, hops, order)
        return self._trees[s]

    def affected(self, s, F):
        """The marked vertices of source s under the failed ids F, in level order."""
        return self._repair_one(int(s), sorted(set(int(e) for e in F)), None)[1]

    def _repair_one(self, s, F, mutant):
        """(dnew of the marked vertices, A) of source s under the sorted failed ids F."""
        d, pe, pu, hops, order = self._tree(s)
        Fs = set(F)
        directed = bool(self.g.directed)
        roots = set()
        for e in F:
            a, b = int(self.src[e]), int(self.dst[e])
            if a == b:
                continue
            if pe[b] == e:
                roots.add(b)
            if not directed and mutant != "one_arc" and pe[a] == e:
                roots.add(a)

        def failed(u, v, e):
            if e not in Fs:
                return False
            if mutant == "one_arc" and not directed:
                return (u, v) == (int(self.src[e]), int(self.dst[e]))
            return True

        mark, A = set(), []
        if roots:
            d0 = min(int(hops[r]) for r in roots)
            for v in order:
                if hops[v] < d0:
                    continue
                if v in roots or (mutant != "roots_only" and int(pu[v]) in mark):
                    if v in roots and any(int(x) in mark for x in self._ancestors(pu, v, s)):
                        self.seen.add("nested_roots")
                    mark.add(v)
                    A.append(v)
        dn = {}
        for v in A:
            best = np.inf
            for u, e, w in self.inarcs[v]:
                if u in mark and mutant != "seed_marked":
                    continue
                if np.isinf(d[u]):
                    continue
                if failed(u, v, e):
                    if e != pe[v]:
                        self.seen.add("nontree_skip")
                    continue
                best = min(best, d[u] + w)
            dn[v] = best
        sweeps = 0
        while True:                                           # Jacobi: a sweep reads the one before
            prev, changed = dict(dn), False
            for v in A:
                for u, e, w in self.inarcs[v]:
                    if u in mark and not failed(u, v, e) and prev[u] + w < dn[v]:
                        dn[v] = prev[u] + w
                        changed = True
            sweeps += 1
            assert sweeps <= len(A) + 1
            if not changed or mutant == "one_sweep":
                break
        if sweeps > 2:
            self.seen.add("many_sweeps")
        if mutant == "root_offset":
            top = {}                                          # the root a marked vertex hangs below
            for v in A:                                       # level order: a parent comes first
                top[v] = v if v in roots else top[int(pu[v])]
            true = dict(dn)
            for v in A:
                r = top[v]
                if v != r and np.isfinite(true[r]) and np.isfinite(true[v]):
                    cand = true[r] + (d[v] - d[r])
                    if abs(cand - true[v]) <= 4 * np.spacing(true[v]):
                        dn[v] = cand
        return dn, A

    @staticmethod
    def _ancestors(pu, v, s):
        v = int(pu[v])
        while v >= 0 and v != s:
            yield v
            v = int(pu[v])

    def repair(self, S, T, W, scenarios, mutant=None):
        W, olds, un, codes = self._split(S, T, W)
        ns = len(scenarios)
        stats, mx, lat = np.zeros((ns, NSTAT), np.uint64), np.zeros(ns), np.full((ns, len(S)), np.nan)
        by_src = {}
        for x, s in enumerate(S):
            by_src.setdefault(int(s), []).append(x)
        for k, F in enumerate(scenarios):
            F = sorted(set(int(e) for e in F))
            Fs = set(F)
            acc = [0, 0, 0]
            for s, xs in by_src.items():
                dn, A = self._repair_one(s, F, mutant)
                mark = set(A)
                for x in xs:
                    o, es = olds[x]
                    if es is None:
                        continue
                    t, w = int(T[x]), int(W[x])
                    if t == s:
                        left = [e for e in self.loops[s] if e not in Fs]
                        nw = self.lat[left[0]] if left else np.nan
                        hit = self.loops[s][0] in Fs
                        if hit:
                            self.seen.add("loop_with_second" if len(self.loops[s]) > 1 else "loop_alone")
                    else:
                        nw = dn[t] if t in mark else o
                        nw = np.nan if np.isinf(nw) else nw
                        hit = t in mark
                    if mutant == "hit_is_changed":
                        hit = not (nw == o)
                    lat[k, x] = nw
                    if hit:
                        acc[HIT] += w
                    if np.isnan(nw):
                        acc[CUT] += w
                    elif (nw > o + 1e-12) if mutant == "slower_tol" else (nw > o):
                        acc[SLOWER] += w
                        mx[k] = max(mx[k], nw - o)
            stats[k] = [a & MASK for a in acc]
        return Result(stats, mx, lat, un, codes)


def block_entries(S, T, W=None):
    """The block sources x targets as entry lists (row-major), weights (ns, nt) or None."""
    S, T = np.asarray(S, np.int32), np.asarray(T, np.int32)
    return np.repeat(S, len(T)), np.tile(T, len(S)), None if W is None else np.asarray(W, np.uint64).ravel()
