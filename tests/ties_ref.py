"""The reference of the tie envelope (shd_route_ties*, include/shd_route.h), in plain Python on
top of multi_ref.Ref: no engine, no oracle library.

Per source s, with d = Ref's Dijkstra row (d[s] = 0.0):
  arcs     the tight ones, d[u] + w == d[v] exactly, v != s, self-loops left out, every parallel
           edge an arc of its own
  order    the vertices in ascending distance (stable): every tight in-arc of v comes from a
           vertex that is strictly nearer (w > 0) and therefore done
  values   count[s] = 1, lo[s] = hi[s] = 1.0 * f_s;  count[v] = the sum of count[u] as Python
           ints, clipped at 2^64 - 1 (a clipped summand keeps the sum clipped);
           lo[v] = min lo[u] * r_e, hi[v] = max hi[u] * r_e
  entry    t != s: (count[t], lo[t], hi[t]), the bounds times f_t last where t has a factor;
           unreachable: (0, NaN, NaN), EUNREACH
           t == s: (1, r, r) with r = Ref.self_entry's reliability; without a loop (0, NaN, NaN),
           ENOEDGE
  dispatch Ref.is_direct (t != s): (1, r, r) with r = Ref.direct_entry's reliability; a pair
           without an edge on a complete graph: (0, NaN, NaN), ENOEDGE
"""
from __future__ import annotations

import numpy as np

from tests.multi_ref import Ref

SAT = (1 << 64) - 1
ENOEDGE, EUNREACH = -4, -5


class TiesRef:
    def __init__(self, g):
        self.ref = Ref(g)
        self.n = self.ref.n
        self._dag = {}

    def dag(self, s: int):
        """(count as Python ints, lo, hi) over all vertices before f_t; count 0 = unreached."""
        s = int(s)
        if s in self._dag:
            return self._dag[s]
        R = self.ref
        d = R.dijkstra(s)[0]
        U, V, E, W = R.U, R.V, R.E, R.W
        with np.errstate(invalid="ignore"):
            tight = (d[U] + W == d[V]) & (V != s) & np.isfinite(d[U])
        q = np.flatnonzero(tight)                            # grouped by v already (Ref sorts by v)
        start = np.searchsorted(V[q], np.arange(self.n + 1))
        tu, tr = U[q].tolist(), R.erel[E[q]].tolist()
        cnt = [0] * self.n
        lo = [float("nan")] * self.n
        hi = [float("nan")] * self.n
        fs = 1.0 if np.isnan(R.vf[s]) else 1.0 * float(R.vf[s])
        cnt[s], lo[s], hi[s] = 1, fs, fs
        for v in np.argsort(d, kind="stable").tolist():
            if v == s or not np.isfinite(d[v]):
                continue
            c, l, h = 0, float("inf"), float("-inf")
            for k in range(int(start[v]), int(start[v + 1])):
                u, r = tu[k], tr[k]
                assert cnt[u] > 0                            # the tail is nearer, so it is done
                c = min(SAT, c + cnt[u])
                l = min(l, lo[u] * r)
                h = max(h, hi[u] * r)
            assert c > 0
            cnt[v], lo[v], hi[v] = c, l, h
        self._dag[s] = (cnt, np.array(lo), np.array(hi))
        return self._dag[s]

    def row(self, s: int, dispatch: bool = False):
        """(count u64, rel_lo, rel_hi) of source s over all vertices; failed entries (0, NaN, NaN)."""
        s = int(s)
        R = self.ref
        if dispatch and R.complete:                          # no rows and no DAG
            count = np.zeros(self.n, np.uint64)
            lo = np.full(self.n, np.nan)
            hi = np.full(self.n, np.nan)
        else:
            cnt, lo, hi = self.dag(s)
            count = np.array(cnt, dtype=np.uint64)
            has = ~np.isnan(R.vf)
            lo = np.where(has, lo * R.vf, lo)                # f_t last
            hi = np.where(has, hi * R.vf, hi)
        for t in range(self.n):
            if t != s and R.is_direct(s, t, dispatch):
                r = R.direct_entry(s, t)[1]
                count[t], lo[t], hi[t] = (0 if np.isnan(r) else 1), r, r
        r = R.self_entry(s)[1]
        count[s], lo[s], hi[s] = (0 if np.isnan(r) else 1), r, r
        return count, lo, hi

    def rows(self, S, T, dispatch: bool = False):
        """(count, rel_lo, rel_hi, codes) of the block S x T."""
        T = np.asarray(T, np.int64)
        out = [self.row(s, dispatch) for s in S]
        codes = set()
        for i, o in enumerate(out):
            failed = o[0][T] == 0
            if np.any(failed & (T == int(S[i]))):
                codes.add(ENOEDGE)
            if np.any(failed & (T != int(S[i]))):
                codes.add(ENOEDGE if (dispatch and self.ref.complete) else EUNREACH)
        return (np.array([o[0][T] for o in out], np.uint64).reshape(len(S), len(T)),
                np.array([o[1][T] for o in out]).reshape(len(S), len(T)),
                np.array([o[2][T] for o in out]).reshape(len(S), len(T)), codes)


def brute(g, s: int, t: int):
    """(count, lo, hi) of s -> t (t != s) by enumerating every simple arc path and keeping those
    of minimum left-fold latency: the definition itself, for graphs of a few vertices."""
    R = Ref(g)
    out = [[] for _ in range(R.n)]
    for u, v, e in zip(R.U.tolist(), R.V.tolist(), R.E.tolist()):
        out[u].append((v, e))
    fs = 1.0 if np.isnan(R.vf[s]) else 1.0 * float(R.vf[s])
    found = []

    def walk(v, lat, rel, seen):
        if v == t:
            found.append((lat, rel))
            return
        for x, e in out[v]:
            if x not in seen:
                walk(x, lat + float(R.lat[e]), rel * float(R.erel[e]), seen | {x})

    walk(int(s), 0.0, fs, {int(s)})
    if not found:
        return 0, np.nan, np.nan
    best = min(f[0] for f in found)
    rels = [f[1] for f in found if f[0] == best]
    ft = R.vf[t]
    if not np.isnan(ft):
        rels = [r * float(ft) for r in rels]
    return len(rels), min(rels), max(rels)


# ---- the state layout of the sweep (shadow_amd/csrc/ties_layout.hpp), mirrored -----------------
# tests/test_ties.py holds these to the header through tests/ties_layout_main.cpp.
LDS_BUDGET = 160 * 1024
SMALL = 16


def _a16(x: int) -> int:
    return (x + 15) & ~15


def layout_total(n: int, tsize: int = 2) -> int:
    """TiesLayout<T>::make(n).total: count, lo, hi (8 bytes each), rem (4), two frontiers of T."""
    return 3 * _a16(8 * n) + _a16(4 * n) + 2 * _a16(tsize * n)


def fits_lds(n: int) -> bool:
    return n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET


def lds_max_n() -> int:
    """The largest n whose state still lives in LDS."""
    lo, hi = 1, 65535
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits_lds(mid) else (lo, mid - 1)
    return lo
