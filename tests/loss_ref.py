"""The reference of the link loss calls (shd_route_loss*, shd_route_pair_loss,
include/shd_route.h), in plain Python on top of multi_ref.Ref for paths, dispatch and the tie
rule: no engine, no oracle library.

The programme of the header, once in Python floats (IEEE doubles, in the stated order) and once
in exact fractions.Fraction over the same f64 inputs.  Per source s, with r_e = 1.0 - loss_e,
q_e = loss_e, f_v = 1.0 - vertex loss and p_v = the vertex loss (NaN = absent: no factor, no drop):

  F_s = 1.0 * f_s (1.0 when absent); pre[s] = F_s; pre[v] = pre[parent(v)] * r_e, a left fold
  own[t] = the u64 sum of the weights of the tree-routed entries with target t
  W_sub(v) = the u64 sum of own over the subtree of v; every integer is converted once
  tree arc u -> v over e, W_sub(v) != 0:   reach = W_sub(v) * pre[u]
                                           edge_reach[e] += reach; edge_drop[e] += reach * q_e
  tree target t, own[t] != 0:              arrive = own[t] * pre[t]
                                           vertex_drop[t] += arrive * p_t; delivered[t] += arrive * f_t
  direct entry (s, t, w) over e:           reach = w * F_s; the two edge adds; arrive = reach * r_e,
                                           then the target's step
  self entry with the self-loop e:         reach = w * F_s; the two edge adds;
                                           delivered[s] += reach * r_e
  the source:                              vertex_drop[s] += W_routed * p_s, one addend
  a failed entry:                          unrouted += w, nothing else

A block call runs one programme per row (a source listed twice is two programmes); a pair call
groups the pairs by distinct source first, as the engine does.

The bound.  An addend is an integer conversion and at most R + 3 multiplications on a tree
(R for pre[t], then by own, by f_t or p_t) or 4 on a direct entry: at most R + 4 roundings.  An
element is the sum of at most A non-negative addends: the first add onto 0.0 is exact, every
later one rounds once.  Every factor is non-negative and nothing is subtracted, so the relative
errors compound: (1 + 2^-53)^(R + 3 + A) - 1, which (R + 4 + A) * 2^-52 bounds with a factor of
two to spare for the second-order terms.  An exact 0 stays 0.

The module also mirrors the state layout of the sweep (shadow_amd/csrc/loss_layout.hpp);
tests/test_loss.py holds the mirror to the header through tests/loss_layout_main.cpp.
"""
from __future__ import annotations

import dataclasses
from fractions import Fraction

import numpy as np

from tests.multi_ref import Ref

ENOEDGE, EUNREACH = -4, -5
U64 = 1 << 64
MUTANTS = ("right_fold", "one_minus_r", "transit_factor", "self_twice")
NAMES = ("edge_reach", "edge_drop", "vertex_drop", "delivered")


@dataclasses.dataclass
class Result:
    edge_reach: list
    edge_drop: list
    vertex_drop: list
    delivered: list
    unrouted: int
    R: int           # the deepest level of any source with a tree-routed entry
    A: int           # the largest number of addends into one element
    codes: set
    routed: int      # the weight of the entries that did not fail (not reduced modulo 2^64)

    def outs(self):
        return [getattr(self, k) for k in NAMES]

    def arrays(self):
        """The four outputs as float64 arrays (of an f64 run)."""
        return [np.array(x, np.float64) for x in self.outs()]


class _Acc:
    def __init__(self, size, zero, init):
        self.v = [zero] * size if init is None else list(init)
        self.c = [0] * size if init is None else [int(x != 0) for x in init]

    def add(self, i, x):
        self.v[i] = self.v[i] + x
        self.c[i] += 1


class LossRef:
    def __init__(self, g, tie: str = "low"):
        """tie="high" is the mutant that takes the highest edge id among the tight parallel arcs
        of a hop (multi_ref.Ref's), which tests/test_frac_graphs.py must see on frac_multi."""
        self.g = g
        self.ref = Ref(g, tie)
        self.n, self.m = self.ref.n, int(g.m)
        self.q = np.asarray(g.packetloss, np.float64).tolist()
        self.r = self.ref.erel.tolist()
        vl = g.vertex_packetloss
        self.p = [float("nan")] * self.n if vl is None else np.asarray(vl, np.float64).tolist()
        self.f = self.ref.vf.tolist()

    # ---- one programme ----------------------------------------------------------------------
    def _source(self, s, entries, dispatch, acc, N, mutant, st):
        er, ed, vd, dl = acc
        ref, r, q, f, p = self.ref, self.r, self.q, self.f, self.p
        qq = (lambda e: N(1.0) - N(r[e])) if mutant == "one_minus_r" else (lambda e: N(q[e]))
        F = N(1.0) if f[s] != f[s] else N(1.0) * N(f[s])

        def edge(e, reach):
            er.add(e, reach)
            ed.add(e, reach * qq(e))

        def target(t, arrive):
            if p[t] == p[t]:
                vd.add(t, arrive * N(p[t]))
            dl.add(t, arrive if f[t] != f[t] else arrive * N(f[t]))

        own, routed = {}, 0
        _, pe, pu, _ = ref.dijkstra(s)
        for t, w in entries:
            t, w = int(t), int(w)
            if t == s:
                e = ref.first.get((s, s))
                if e is None:
                    st["codes"].add(ENOEDGE); st["un"] += w
                elif w:
                    routed += w
                    reach = N(float(w)) * F if N is float else N(w) * F
                    edge(e, reach)
                    x = reach * N(r[e])
                    if mutant == "self_twice" and f[s] == f[s]:
                        x = x * N(f[s])
                    dl.add(s, x)
            elif ref.is_direct(s, t, dispatch):
                e = ref.first.get((s, t))
                if e is None:
                    st["codes"].add(ENOEDGE); st["un"] += w
                elif w:
                    routed += w
                    reach = N(float(w)) * F if N is float else N(w) * F
                    edge(e, reach)
                    target(t, reach * N(r[e]))
            elif pu[t] < 0:
                st["codes"].add(EUNREACH); st["un"] += w
            elif w:
                routed += w
                own[t] = (own.get(t, 0) + w) % U64
        st["routed"] += routed
        wr = routed % U64
        if wr and p[s] == p[s]:
            vd.add(s, (N(float(wr)) if N is float else N(wr)) * N(p[s]))
        own = {t: w for t, w in own.items() if w}
        if not own:
            return
        hops = ref._chains(s)[0]
        st["R"] = max(st["R"], int(hops.max()))
        # the vertices on the way to a target, by level
        need = set()
        for t in own:
            v = t
            while v != s and v not in need:
                need.add(v)
                v = int(pu[v])
        by = sorted(need, key=lambda v: (int(hops[v]), v))
        pre = {s: F}
        for v in by:
            u, e = int(pu[v]), int(pe[v])
            if mutant == "right_fold":
                vals, x = [], v
                while x != s:
                    vals.append(N(r[int(pe[x])])); x = int(pu[x])
                a = vals[0]                      # the last hop first: F * (r_1 * (r_2 * ... r_k))
                for y in vals[1:]:
                    a = y * a
                pre[v] = F * a
            elif mutant == "transit_factor":
                a = pre[u]
                if u != s and f[u] == f[u]:
                    a = a * N(f[u])
                pre[v] = a * N(r[e])
            else:
                pre[v] = pre[u] * N(r[e])
        conv = (lambda w: N(float(w))) if N is float else (lambda w: N(w))
        for t in sorted(own, key=lambda v: (int(hops[v]), v)):
            target(t, conv(own[t]) * pre[t])
        sub = dict(own)
        for v in reversed(by):
            u = int(pu[v])
            if u != s and sub.get(v, 0):
                sub[u] = (sub.get(u, 0) + sub[v]) % U64
        for v in by:
            if sub.get(v, 0):
                edge(int(pe[v]), conv(sub[v]) * pre[int(pu[v])])

    def _run(self, programmes, dispatch, exact, init, mutant):
        N = Fraction if exact else float
        zero = N(0)
        sizes = (self.m, self.m, self.n, self.n)
        init = init or (None,) * 4
        acc = [_Acc(k, zero, None if a is None else [N(float(x)) for x in a]) for k, a in zip(sizes, init)]
        st = {"codes": set(), "un": 0, "R": 0, "routed": 0}
        for s, entries in programmes:
            self._source(int(s), entries, dispatch, acc, N, mutant, st)
        A = max([max(a.c, default=0) for a in acc], default=0)
        return Result(acc[0].v, acc[1].v, acc[2].v, acc[3].v, st["un"] % U64, st["R"], A, st["codes"], st["routed"])

    # ---- the call forms ---------------------------------------------------------------------
    def pairs(self, PS, PT, W=None, dispatch=False, exact=False, init=None, mutant=None):
        """The pairs (PS[k], PT[k]) with weights W[k] (None: 1), grouped by distinct source."""
        groups = {}
        for k, (s, t) in enumerate(zip(PS, PT)):
            groups.setdefault(int(s), []).append((int(t), 1 if W is None else int(W[k])))
        return self._run(sorted(groups.items()), dispatch, exact, init, mutant)

    def block(self, S, T, W=None, dispatch=False, exact=False, init=None, mutant=None):
        """The block S x T with weights W[i][j] (None: 1): one programme per row."""
        progs = [(int(s), [(int(t), 1 if W is None else int(W[i][j])) for j, t in enumerate(T)])
                 for i, s in enumerate(S)]
        return self._run(progs, dispatch, exact, init, mutant)


def bound(R: int, A: int) -> Fraction:
    return Fraction(R + 4 + A, 1 << 52)


def close(got, want, R: int, A: int) -> bool:
    """Every element of got (doubles) within the derived bound of want (exact fractions)."""
    b = bound(R, A)
    got = np.asarray(got, np.float64).tolist()
    if len(got) != len(want):
        return False
    for x, w in zip(got, want):
        if x != x or x in (float("inf"), float("-inf")):
            return False
        x = Fraction(x)
        if (x != 0) if w == 0 else (abs(x - w) > b * w):
            return False
    return True


def decimal_losses(g, seed: int = 0, vloss: bool = True):
    """g with decimal losses no float32 holds (k / 1000, k in 1 .. 60, on every edge) and, with
    vloss, a vertex loss k / 1000 on two vertices in three and NaN on the rest."""
    rng = np.random.default_rng(5000 + seed)
    loss = rng.integers(1, 61, size=int(g.m)) / 1000.0
    vl = None
    if vloss:
        vl = np.where(np.arange(g.n) % 3 == 1, np.nan, rng.integers(1, 41, size=g.n) / 1000.0)
    return dataclasses.replace(g, packetloss=loss, vertex_packetloss=vl, name=g.name + "_dec")


# ---- the state layout of the sweep (shadow_amd/csrc/loss_layout.hpp), mirrored -----------------
LDS_BUDGET = 160 * 1024
SMALL = 96


def _a16(x: int) -> int:
    return (x + 15) & ~15


def layout_offsets(n: int, tsize: int = 2):
    """(sum, pre, lvl, order, total) of LossLayout<T>::make(n): the u64 sums and the f64
    products (8 bytes per vertex each), the n + 1 level offsets (4) and the order list of T."""
    s = 0
    pre = s + _a16(8 * n)
    lvl = pre + _a16(8 * n)
    order = lvl + _a16(4 * (n + 1))
    return s, pre, lvl, order, order + _a16(tsize * n)


def layout_total(n: int, tsize: int = 2) -> int:
    return layout_offsets(n, tsize)[4]


def fits_lds(n: int) -> bool:
    return n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET


def lds_max_n() -> int:
    """The largest n whose state still lives in LDS."""
    lo, hi = 1, 65535
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits_lds(mid) else (lo, mid - 1)
    return lo
