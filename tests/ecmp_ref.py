"""The reference of the ECMP link loads (shd_route_ecmp_loads*, include/shd_route.h), in plain
Python on top of multi_ref.Ref: no engine, no oracle library.

Per source s, with d = Ref's Dijkstra row (d[s] = 0.0):
  arcs     the tight ones, d[u] + w == d[v] exactly, v != s, self-loops left out, every parallel
           edge an arc of its own (what tests/ties_ref.py takes)
  sigma    sigma[s] = 1, sigma[v] = the sum of sigma[u] over the tight in-arcs of v in the order
           of the in-CSR (tail, then edge id)
  own      own[x] = the weights of the entries with target x, summed as integers modulo 2^64 and
           converted once
  delta    delta[v] = the sum over the tight out-arcs (v -> x, e) of f_e in the order of the
           out-CSR (head, then edge id), f_e = (sigma[v] / sigma[x]) * (own[x] + delta[x]);
           edge[e] += f_e, transit[v] += delta[v] for v != s
  entry    t == s: the weight on the lowest self-loop edge; without one ENOEDGE and unrouted
           unreachable t: EUNREACH and unrouted
  dispatch Ref.is_direct (t != s): the weight on the lowest edge id of the pair; a pair without
           an edge on a complete graph: ENOEDGE and unrouted

`exact=False` runs the programme in f64 (Python floats, the operations in the order above),
`exact=True` in fractions.Fraction.  The sums across sources are taken in the order of the call.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests.multi_ref import Ref

ENOEDGE, EUNREACH = -4, -5
M64 = (1 << 64) - 1


class EcmpRef:
    def __init__(self, g):
        self.ref = Ref(g)
        self.n = self.ref.n
        self.m = int(g.m)
        self._dag = {}

    def dag(self, s: int):
        """The tight arcs of source s: (reach, order, tin, tout, depth).  order = the reached
        vertices other than s in ascending distance; tin[v] = [(u, e)] in in-CSR order,
        tout[v] = [(x, e)] in out-CSR order; depth[v] = the longest chain of tight arcs from s
        (the level of the forward sweep)."""
        s = int(s)
        if s in self._dag:
            return self._dag[s]
        R = self.ref
        d = R.dijkstra(s)[0]
        U, V, E, W = R.U, R.V, R.E, R.W
        with np.errstate(invalid="ignore"):
            tight = (d[U] + W == d[V]) & (V != s) & np.isfinite(d[U])
        q = np.flatnonzero(tight)                            # (v, u, e) order: the in-CSR's
        tin = [[] for _ in range(self.n)]
        for u, v, e in zip(U[q].tolist(), V[q].tolist(), E[q].tolist()):
            tin[v].append((u, e))
        qo = q[np.lexsort((E[q], V[q], U[q]))]               # (u, v, e) order: the out-CSR's
        tout = [[] for _ in range(self.n)]
        for u, v, e in zip(U[qo].tolist(), V[qo].tolist(), E[qo].tolist()):
            tout[u].append((v, e))
        reach = np.isfinite(d)
        order = [v for v in np.argsort(d, kind="stable").tolist() if v != s and reach[v]]
        depth = [0] * self.n
        for v in order:
            depth[v] = 1 + max(depth[u] for u, _ in tin[v])
        self._dag[s] = (reach, order, tin, tout, depth)
        return self._dag[s]

    def shape(self, S):
        """(R, D) of the sources S: the deepest level, the most tight in- or out-arcs of a vertex."""
        Rm, D = 0, 1
        for s in {int(x) for x in S}:
            _, _, tin, tout, depth = self.dag(s)
            Rm = max(Rm, max(depth))
            D = max(D, max(map(len, tin)), max(map(len, tout)))
        return Rm, D

    def sigma(self, s: int, exact: bool = False):
        _, order, tin, _, _ = self.dag(s)
        sig = [0 if exact else 0.0] * self.n
        sig[int(s)] = 1 if exact else 1.0
        for v in order:
            c = 0 if exact else 0.0
            for u, _ in tin[v]:
                c = c + sig[u]
            sig[v] = c
        return sig

    def _sweep(self, s, own, edge, transit, exact):
        """delta of source s from the integer own weights, added into edge / transit."""
        _, order, _, tout, _ = self.dag(s)
        sig = self.sigma(s, exact)
        zero = Fraction(0) if exact else 0.0
        num = (lambda x: Fraction(x)) if exact else float
        dl = [zero] * self.n
        for v in order[::-1] + [int(s)]:
            acc = zero
            for x, e in tout[v]:
                below = num(own[x]) + dl[x]
                f = (Fraction(sig[v], sig[x]) if exact else sig[v] / sig[x]) * below
                if f == 0:
                    continue
                acc = acc + f
                edge[e] = edge[e] + f
            dl[v] = acc
            if v != s and acc != 0:
                transit[v] = transit[v] + acc

    def _entries(self, lists, dispatch, exact):
        """lists: [(s, [(t, w)])] in the order of the call."""
        R = self.ref
        zero = Fraction(0) if exact else 0.0
        num = (lambda x: Fraction(x)) if exact else float
        edge = [zero] * self.m
        transit = [zero] * self.n
        un, codes = 0, set()
        for s, ent in lists:
            s = int(s)
            sweep = not (dispatch and R.complete)
            reach = self.dag(s)[0] if sweep else None
            own = [0] * self.n
            for t, w in ent:
                t, w = int(t), int(w)
                if t == s:
                    e = R.self_entry(s)[3]
                    if e < 0:
                        codes.add(ENOEDGE); un += w
                    elif w:
                        edge[e] = edge[e] + num(w)
                elif R.is_direct(s, t, dispatch) and R.direct_entry(s, t)[3] >= 0:
                    if w:
                        e = R.direct_entry(s, t)[3]
                        edge[e] = edge[e] + num(w)
                elif not sweep:
                    codes.add(ENOEDGE); un += w
                elif not reach[t]:
                    codes.add(EUNREACH); un += w
                else:
                    own[t] = (own[t] + w) & M64
            if sweep:
                self._sweep(s, own, edge, transit, exact)
        if not exact:
            edge, transit = np.array(edge, np.float64), np.array(transit, np.float64)
        return edge, transit, un & M64, codes

    def rows(self, S, T, W=None, dispatch: bool = False, exact: bool = False):
        """(edge, transit, unrouted, codes) of the block S x T with weights W (None = 1 each)."""
        T = [int(t) for t in T]
        lists = [(int(s), [(t, 1 if W is None else int(W[i][j])) for j, t in enumerate(T)]) for i, s in enumerate(S)]
        return self._entries(lists, dispatch, exact)

    def pairs(self, PS, PT, PW=None, dispatch: bool = False, exact: bool = False):
        """The same of the pairs (PS[k], PT[k], PW[k]) in any order: grouped by source, the
        sources ascending (what shd_route_pair_ecmp_loads does)."""
        by = {}
        for k, (s, t) in enumerate(zip(PS, PT)):
            by.setdefault(int(s), []).append((int(t), 1 if PW is None else int(PW[k])))
        return self._entries(sorted(by.items()), dispatch, exact)

    def tol(self, S, mult: int = 1, dispatch: bool = False):
        """The relative tolerance of a call over the sources S in which no (source, target)
        pair is listed more than `mult` times.  u = 2^-53; all terms are non-negative, so the
        errors only add up relatively.  A sigma is a chain of at most R sums of at most D terms:
        R D u.  A flow takes a quotient of two sigmas, one add and one multiply per level, delta
        adds at most D flows per level, over at most R + 1 levels; an output element then takes
        at most A = ns (1 + mult) atomic adds.  (Under dispatch on a complete graph there is no
        sweep: R = 0, D = 1.)"""
        Rm, D = (0, 1) if dispatch and self.ref.complete else self.shape(S)
        A = len(list(S)) * (1 + mult)
        return ((Rm + 1) * (2 * (Rm + 1) * D + D + 4) + A) * 2.0 ** -52


def close(got, want, rtol):
    """got equals want within rtol relative, with the same zero pattern (want: floats or Fractions)."""
    got = np.asarray(got, np.float64)
    if len(got) != len(want):
        return False
    for a, b in zip(got.tolist(), want):
        if (a == 0) != (b == 0):
            return False
        if b != 0 and abs(Fraction(a) - Fraction(b)) > Fraction(rtol) * abs(Fraction(b)):
            return False
    return True


def worst(got, want):
    """The largest relative error of got against the exact want, in units of 2^-53."""
    w = Fraction(0)
    for a, b in zip(np.asarray(got, np.float64).tolist(), want):
        if b != 0:
            w = max(w, abs(Fraction(a) - Fraction(b)) / abs(Fraction(b)))
    return float(w * 2 ** 53)


# ---- the state layout of the sweep (shadow_amd/csrc/ecmp_layout.hpp), mirrored -----------------
# tests/test_ecmp.py holds these to the header through tests/ecmp_layout_main.cpp.
LDS_BUDGET = 160 * 1024
SMALL = 16


def _a16(x: int) -> int:
    return (x + 15) & ~15


def layout_total(n: int, tsize: int = 2) -> int:
    """EcmpLayout<T>::make(n).total: sigma, delta, own (8 bytes each), rem (4), the order list
    of T and the n + 1 level offsets (4)."""
    return 3 * _a16(8 * n) + _a16(4 * n) + _a16(tsize * n) + _a16(4 * (n + 1))


def fits_lds(n: int) -> bool:
    return n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET


def lds_max_n() -> int:
    """The largest n whose state still lives in LDS."""
    lo, hi = 1, 65535
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits_lds(mid) else (lo, mid - 1)
    return lo
