"""The reference of the multigraph rules of include/shd_route.h, in plain Python and numpy: no
engine, no oracle library.  (The shared helper of the rows tests, OracleGraph.source_row,
replays igraph_get_eid per hop as the reference does; on parallel edges that names an edge
Dijkstra may never have relaxed, and its latency is then not the distance: hazard H3.)

Per source:
  dist     heap Dijkstra, d[v] = the smallest left-fold sum d[u] + w over the in-arcs, in double
  parent   among the in-arcs (u -> v, edge e) with d[u] + w == d[v] exactly, the one with the
           smallest (d[u], u, e); Ref(g, tie="high") is the mutant that takes the highest e
  entry    t != s: lat = 0.0 + the path's latencies from s on, rel = ((1.0 * f_s) * f_t) times
           1 - loss of each hop from s on, absent vertex factors skipped; hops = its edges
           t == s: the lowest-id self-loop, lat = w, rel = (1.0 * f_s) * r, one hop [s, s];
           without a self-loop a failed entry (NaN, NaN, -1)
  direct   the lowest edge id joining the pair: lat = w, rel = ((1.0 * f_s) * f_t) * r
  dispatch a complete graph (every vertex has n incident edges by count): every entry direct;
           prefer-direct and an adjacent pair: direct; else the tree entry
"""
from __future__ import annotations

import heapq

import numpy as np


class Ref:
    def __init__(self, g, tie: str = "low"):
        self.g, self.n, self.tie = g, int(g.n), tie
        self.lat = np.asarray(g.latency, np.float64)
        self.erel = 1.0 - np.asarray(g.packetloss, np.float64)
        vl = g.vertex_packetloss
        self.vf = np.full(self.n, np.nan) if vl is None else 1.0 - np.asarray(vl, np.float64)
        src, dst = np.asarray(g.src, np.int64), np.asarray(g.dst, np.int64)
        e = np.flatnonzero(src != dst)
        if g.directed:
            U, V, E = src[e], dst[e], e
        else:
            U, V, E = np.concatenate([src[e], dst[e]]), np.concatenate([dst[e], src[e]]), np.concatenate([e, e])
        o = np.lexsort((E, U, V))
        self.U, self.V, self.E = U[o], V[o], E[o]          # arcs u -> v over edge e, grouped by v
        self.W = self.lat[self.E]
        self.out = [[] for _ in range(self.n)]
        for u, v, w in zip(self.U.tolist(), self.V.tolist(), self.W.tolist()):
            self.out[u].append((v, w))
        # the lowest edge id of every joined ordered pair, and of every vertex's self-loops
        self.first = {}
        for k in range(g.m):
            a, b = int(src[k]), int(dst[k])
            for key in ((a, b),) if g.directed else ((a, b), (b, a)):
                self.first.setdefault(key, k)
        cnt = np.bincount(self.U, minlength=self.n)          # out-incident edges by count
        loops = np.bincount(src[src == dst], minlength=self.n)
        cnt = cnt + (loops if g.directed else 2 * loops - (loops > 0))
        self.complete = bool(np.all(cnt >= self.n))
        self._tree = {}

    # ---- one source ---------------------------------------------------------------------
    def dijkstra(self, s: int):
        """(dist, parent edge id, parent vertex, parallel) of source s: dist inf and parents -1
        where unreachable (and at s); parallel[v] = the chosen parent was taken among two or
        more tight arcs from the same vertex whose reliabilities differ."""
        s = int(s)
        if s in self._tree:
            return self._tree[s]
        d = [float("inf")] * self.n
        d[s] = 0.0
        done = [False] * self.n
        heap = [(0.0, s)]
        while heap:
            du, u = heapq.heappop(heap)
            if done[u]:
                continue
            done[u] = True
            for v, w in self.out[u]:
                x = du + w
                if x < d[v]:
                    d[v] = x
                    heapq.heappush(heap, (x, v))
        d = np.array(d)
        U, V, E, W = self.U, self.V, self.E, self.W
        tight = (d[U] + W == d[V]) & (V != s) & np.isfinite(d[U])
        q = np.flatnonzero(tight)
        o = q[np.lexsort((E[q] if self.tie == "low" else -E[q], U[q], d[U[q]], V[q]))]
        head = np.ones(len(o), bool)
        head[1:] = V[o][1:] != V[o][:-1]
        best = o[head]                                       # the chosen arc of every reached vertex
        pe = np.full(self.n, -1, np.int64); pu = np.full(self.n, -1, np.int64)
        pe[V[best]], pu[V[best]] = E[best], U[best]
        # tight arcs that share the chosen arc's tail: how many, and do their reliabilities differ
        key = V[q] * self.n + U[q]
        ck = V[best] * self.n + U[best]
        r = self.erel[E[q]]
        uk, inv = np.unique(key, return_inverse=True)
        rmin = np.full(len(uk), np.inf); rmax = np.full(len(uk), -np.inf)
        np.minimum.at(rmin, inv, r); np.maximum.at(rmax, inv, r)
        at = np.searchsorted(uk, ck)
        par = np.zeros(self.n, bool)
        par[V[best]] = (np.bincount(inv, minlength=len(uk))[at] >= 2) & (rmin[at] != rmax[at])
        self._tree[s] = (d, pe, pu, par)
        return self._tree[s]

    def _chains(self, s: int):
        """hops[v] and back[k][v] = the edge k hops before v on the tree path of v (-1 past s)."""
        d, pe, pu, _ = self.dijkstra(s)
        hops = np.full(self.n, -1, np.int64)
        hops[s] = 0
        for v in np.argsort(d, kind="stable").tolist():      # a parent is strictly nearer (w > 0)
            if v != s and pu[v] >= 0:
                hops[v] = hops[pu[v]] + 1
        back, cur = [], np.arange(self.n)
        for _ in range(int(hops.max())):
            back.append(np.where(cur >= 0, pe[np.maximum(cur, 0)], -1))
            cur = np.where(cur >= 0, pu[np.maximum(cur, 0)], -1)
        return hops, back

    def self_entry(self, s: int):
        e = self.first.get((int(s), int(s)))
        if e is None:
            return np.nan, np.nan, -1, -1
        r = 1.0
        if not np.isnan(self.vf[s]):
            r = r * self.vf[s]
        return self.lat[e], r * self.erel[e], 1, e

    def base(self, s, t):
        r = 1.0
        if not np.isnan(self.vf[s]):
            r = r * self.vf[s]
        if not np.isnan(self.vf[t]):
            r = r * self.vf[t]
        return r

    def direct_entry(self, s: int, t: int):
        """(lat, rel, hops, edge) over the lowest edge id joining s and t; failed without one."""
        e = self.first.get((int(s), int(t)))
        if e is None:
            return np.nan, np.nan, -1, -1
        return self.lat[e], self.base(s, t) * self.erel[e], 1, e

    def is_direct(self, s: int, t: int, dispatch: bool) -> bool:
        if not dispatch:
            return False
        return self.complete or (bool(self.g.prefer_direct) and (int(s), int(t)) in self.first)

    def row(self, s: int, dispatch: bool = False):
        """(lat, rel, hops) of source s over all vertices."""
        s = int(s)
        d, pe, pu, _ = self.dijkstra(s)
        hops, back = self._chains(s)
        lat = np.zeros(self.n)
        fs = 1.0 if np.isnan(self.vf[s]) else 1.0 * self.vf[s]
        rel = np.where(np.isnan(self.vf), fs, fs * self.vf)  # (1.0 * f_s) * f_t
        idx = np.arange(self.n)
        back = np.stack(back) if back else np.zeros((0, self.n), np.int64)
        for j in range(len(back)):                           # hop j of every path, from s on
            k = hops - 1 - j
            ok = k >= 0
            e = back[k[ok], idx[ok]]
            lat[ok] = lat[ok] + self.lat[e]
            rel[ok] = rel[ok] * self.erel[e]
        un = hops < 0
        lat[un] = np.nan; rel[un] = np.nan
        assert np.array_equal(lat[~un], d[~un])              # the fold down the parents is the distance
        h = hops.astype(np.int32)
        lat[s], rel[s], h[s], _ = self.self_entry(s)
        if dispatch:
            for t in range(self.n):
                if self.is_direct(s, t, True):
                    lat[t], rel[t], h[t], _ = self.direct_entry(s, t)
        return lat, rel, h

    def rows(self, S, T, dispatch: bool = False):
        T = np.asarray(T, np.int64)
        out = [self.row(s, dispatch) for s in S]
        return (np.array([o[0][T] for o in out]).reshape(len(S), len(T)),
                np.array([o[1][T] for o in out]).reshape(len(S), len(T)),
                np.array([o[2][T] for o in out], np.int32).reshape(len(S), len(T)))

    def direct(self, S, T):
        lat = np.full((len(S), len(T)), np.nan); rel = np.full((len(S), len(T)), np.nan)
        for i, s in enumerate(S):
            for j, t in enumerate(T):
                lat[i, j], rel[i, j] = self.direct_entry(int(s), int(t))[:2]
        return lat, rel

    # ---- routes and loads ---------------------------------------------------------------
    def path(self, s: int, t: int, dispatch: bool = False):
        """(vertices, edge ids) of the entry (s, t), or None for a failed one."""
        s, t = int(s), int(t)
        if s == t and not (dispatch and self.complete):
            e = self.self_entry(s)[3]
            return None if e < 0 else ([s, s], [e])
        if self.is_direct(s, t, dispatch):
            e = self.direct_entry(s, t)[3]
            return None if e < 0 else ([s, t], [e])
        _, pe, pu, _ = self.dijkstra(s)
        if pu[t] < 0:
            return None
        vs, es, v = [t], [], t
        while v != s:
            es.append(int(pe[v])); v = int(pu[v]); vs.append(v)
        return vs[::-1], es[::-1]

    def loads(self, S, T, W=None, dispatch: bool = False):
        """(edge_load, transit, unrouted) of the pairs (S[k], T[k]) with weights W[k] (None: 1):
        u64 sums over the routes of path()."""
        el = np.zeros(self.g.m, np.uint64); tr = np.zeros(self.n, np.uint64)
        un = 0
        for k, (s, t) in enumerate(zip(S, T)):
            w = 1 if W is None else int(W[k])
            p = self.path(s, t, dispatch)
            if p is None:
                un += w
                continue
            for e in p[1]:
                el[e] += np.uint64(w)
            for v in p[0][1:-1]:
                tr[v] += np.uint64(w)
        return el, tr, un % (1 << 64)


def triangle(lat, rel):
    """First writer wins under ascending sources: the upper triangle of a square table over the
    sorted attached vertices, mirrored (pair {i, j} holds row min(i, j)'s entry)."""
    lat, rel = lat.copy(), rel.copy()
    il = np.tril_indices(len(lat), -1)
    lat[il], rel[il] = lat.T[il], rel.T[il]
    return lat, rel
