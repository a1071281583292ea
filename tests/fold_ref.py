"""The reference of the path folds (shd_route_fold*, shd_route_pair_fold, include/shd_route.h),
in plain Python on top of multi_ref.Ref: no engine, no oracle library.

An entry (s, t) is Ref.path(s, t, dispatch): the edge ids shd_route_paths reports, from the
source on.  Fold k of the entry is the left fold of values[k] over those edge ids in Python
floats (IEEE doubles), from the op's start value:

  SUM   acc = acc + a, from 0.0          MIN   acc = a if a < acc else acc, from +inf
  PROD  acc = acc * a, from 1.0          MAX   acc = a if a > acc else acc, from -inf

A failed entry is NaN in every fold, with its code: ENOEDGE for a self entry without a
self-loop and for a pair without an edge on a complete graph under dispatch, EUNREACH for an
unreachable target.  The engine's folds are deterministic left folds too, so the tests compare
exactly: no tolerance.

The module also mirrors the state layout of the sweep (shadow_amd/csrc/fold_layout.hpp);
tests/test_fold.py holds the mirror to the header through tests/fold_layout_main.cpp.
"""
from __future__ import annotations

import math

import numpy as np

from tests.multi_ref import Ref

ENOEDGE, EUNREACH = -4, -5
SUM, MIN, MAX, PROD = 0, 1, 2, 3
START = {SUM: 0.0, MIN: math.inf, MAX: -math.inf, PROD: 1.0}
ALL_OPS = [SUM, MIN, MAX, PROD]


def fold_one(op: int, vals) -> float:
    """The left fold of the Python floats vals."""
    acc = START[op]
    if op == SUM:
        for a in vals:
            acc = acc + a
    elif op == MIN:
        for a in vals:
            acc = a if a < acc else acc
    elif op == MAX:
        for a in vals:
            acc = a if a > acc else acc
    else:
        for a in vals:
            acc = acc * a
    return acc


class FoldRef:
    def __init__(self, g):
        self.ref = Ref(g)
        self.n = self.ref.n
        self.m = int(g.m)
        self._path = {}

    def edges(self, s: int, t: int, dispatch: bool):
        """(edge ids, 0) of the entry, or (None, code) of a failed one."""
        key = (int(s), int(t), bool(dispatch))
        if key not in self._path:
            p = self.ref.path(key[0], key[1], key[2])
            if p is not None:
                self._path[key] = (p[1], 0)
            elif key[0] == key[1] or self.ref.is_direct(key[0], key[1], key[2]):
                self._path[key] = (None, ENOEDGE)
            else:
                self._path[key] = (None, EUNREACH)
        return self._path[key]

    def pairs(self, PS, PT, ops, values, dispatch: bool = False):
        """(out (nf, npairs), codes) of the pairs (PS[p], PT[p]) in the caller's order."""
        ops = [int(o) for o in ops]
        cols = [np.asarray(v, np.float64).tolist() for v in values]
        assert len(cols) == len(ops) and all(len(c) == self.m for c in cols)
        out = np.full((len(ops), len(PS)), np.nan)
        codes = set()
        for p, (s, t) in enumerate(zip(PS, PT)):
            es, code = self.edges(s, t, dispatch)
            if es is None:
                codes.add(code)
                continue
            for k, (op, col) in enumerate(zip(ops, cols)):
                out[k, p] = fold_one(op, [col[e] for e in es])
        return out, codes

    def rows(self, S, T, ops, values, dispatch: bool = False):
        """(out (nf, ns, nt), codes) of the block S x T."""
        S, T = [int(s) for s in S], [int(t) for t in T]
        out, codes = self.pairs(np.repeat(S, len(T)), np.tile(T, len(S)), ops, values, dispatch)
        return out.reshape(len(ops), len(S), len(T)), codes


def columns(g, seed: int = 0):
    """Four value columns (4, m) from a seeded generator: decimals with two places, integers in
    1..9, values in (0, 1] and integers in 1..9 with a few +inf and -inf among them.  (SUM is
    not taken over the last one: +inf + -inf is NaN, which is reserved for failed entries.)"""
    rng = np.random.default_rng(1000 + seed)
    m = int(g.m)
    dec = rng.integers(1, 10000, size=m) / 100.0
    ints = rng.integers(1, 10, size=m).astype(np.float64)
    unit = 1.0 - rng.random(m)
    infs = rng.integers(1, 10, size=m).astype(np.float64)
    if m:
        k = max(1, min(6, m // 8))
        at = rng.choice(m, size=min(m, 2 * k), replace=False)
        infs[at[:k]] = np.inf
        infs[at[k:]] = -np.inf
    return np.stack([dec, ints, unit, infs])


def no_vertex_loss(g) -> bool:
    """No vertex of g loses packets: no vertex loss array, or one of absent (NaN) and zero entries,
    whose factors 1.0 - 0.0 multiply a reliability exactly."""
    vl = g.vertex_packetloss
    return vl is None or not np.any(np.nan_to_num(np.asarray(vl, np.float64)))


def same(got, want) -> bool:
    """Exactly equal, NaN where NaN is: no tolerance."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


# ---- the state layout of the sweep (shadow_amd/csrc/fold_layout.hpp), mirrored -----------------
LDS_BUDGET = 160 * 1024
SMALL = 96


def _a16(x: int) -> int:
    return (x + 15) & ~15


def layout_offsets(n: int, tsize: int = 2):
    """(val, lvl, order, total) of FoldLayout<T>::make(n): the carried folds (8 bytes per
    vertex), the n + 1 level offsets (4) and the order list of T."""
    val = 0
    lvl = val + _a16(8 * n)
    order = lvl + _a16(4 * (n + 1))
    return val, lvl, order, order + _a16(tsize * n)


def layout_total(n: int, tsize: int = 2) -> int:
    return layout_offsets(n, tsize)[3]


def fits_lds(n: int) -> bool:
    return n <= 65535 and SMALL + layout_total(n, 2) <= LDS_BUDGET


def lds_max_n() -> int:
    """The largest n whose state still lives in LDS."""
    lo, hi = 1, 65535
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits_lds(mid) else (lo, mid - 1)
    return lo
