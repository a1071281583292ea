"""GPU: the path calls that read reliabilities -- the tie envelope, the path folds and the link
loss -- on the graphs of tests/rel_graphs.py: arcs and vertices of reliability exactly 0
(envelopes with rel_lo == 0 < rel_hi and with rel_hi == 0, links that drop everything), products
that run through the subnormals to 0.0, and losses of 2**-60, whose arcs are lossless to the rows
kernels and must still drop packets.  Every call in both state forms ("lds": no knob; "hbm":
SHD_ROUTE_TIES_LDS, FOLD_LDS and LOSS_LDS all 0), the folds and the loss also in their pair form.

  ties    count, rel_lo and rel_hi equal tests/ties_ref.py exactly; the engine's own rows and the
          oracle's under both tie rules lie inside [rel_lo, rel_hi] (where the target has a vertex
          factor the envelope multiplies it last and a walk kernel first, so there only on the
          entries without one, and on the exact zeros)
  folds   the product of 1 - loss along the route equals the rows' reliability bit for bit on every
          graph without vertex loss: two different kernels, one left fold, through the subnormals;
          min and max of the same column against tests/fold_ref.py
  loss    one-source calls equal the f64 programme of tests/loss_ref.py bit for bit, rel_deep's
          subnormal products included; the weighted block over all sources lies within
          (R + 4 + A) * 2^-52 of the exact fractions on the graphs whose products stay normal (the
          bound's derivation assumes normal numbers; test_rel_graphs.Watched asserts it of every
          product of the f64 programme), exact zeros exactly zero
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fold_ref as fr
from tests import loss_ref as lr
from tests import rel_graphs as rg
from tests import ties_ref as tr
from tests.test_range_gpu import close_engines, has_loop, route  # noqa: F401
from tests.test_rel_graphs import Watched, loss_weights
from tests.test_rel_gpu import reference as rows_reference

pytestmark = pytest.mark.gpu

FORMS = ("lds", "hbm")
FORM_KNOBS = ("SHD_ROUTE_TIES_LDS", "SHD_ROUTE_FOLD_LDS", "SHD_ROUTE_LOSS_LDS")
TIES_GRAPHS = ("rel_zero_ties", "rel_zero_dir", "rel_vzero", "rel_deep")
FOLD_GRAPHS = tuple(n for n in rg.SUITE if n not in ("rel_vzero", "rel_zero8000"))
LOSS_GRAPHS = ("rel_zero", "rel_vzero", "rel_tinyloss", "rel_deep")
LOSS_BLOCK = ("rel_zero", "rel_vzero", "rel_tinyloss")
LOSS_ONE = 4


@pytest.fixture(scope="module")
def topo():
    from shadow_amd import topology
    topology.load_library()
    return topology


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith(("SHD_ROUTE_", "SHD_TOPOLOGY_"))]:
        monkeypatch.delenv(k)


def choose(monkeypatch, form):
    if form == "hbm":
        for k in FORM_KNOBS:
            monkeypatch.setenv(k, "0")


def call(route, fn, *a, **k):
    try:
        return fn(*a, **k), route.OK
    except route.RouteError as e:
        assert e.code in (route.ENOEDGE, route.EUNREACH), e
        return e.partial, e.code


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def vfree(g):
    """Vertices without a vertex factor."""
    vl = g.vertex_packetloss
    return np.ones(g.n, bool) if vl is None else np.isnan(np.asarray(vl))


# ---- ties ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ties_reference(name):
    g = rg.get(name)
    out = tr.TiesRef(g).rows(rg.sources(name), np.arange(g.n))
    for a in out[:3]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TIES_GRAPHS)
def test_ties(route, oracle_mod, monkeypatch, name, form):
    g = rg.get(name)
    S, T = rg.sources(name), np.arange(g.n, dtype=np.int32)
    cnt, lo, hi, codes = ties_reference(name)
    choose(monkeypatch, form)
    eng = route.RouteEngine(g)
    (gc, gl, gh), code = call(route, eng.ties, S, T, dispatch=False)
    assert (code in codes) if codes else code == route.OK
    assert gc.dtype == np.uint64 and np.array_equal(gc, cnt)
    assert eq(gl, lo) and eq(gh, hi)
    ok = cnt > 0
    if name.startswith("rel_zero"):
        assert ((lo == 0.0) & (hi > 0.0)).sum() >= 10 and ((cnt > 1) & (hi == 0.0)).sum() >= 10
    if name == "rel_deep":
        assert np.all(cnt[ok] == 1) and eq(lo, hi) and ((lo > 0.0) & (lo < np.finfo(np.float64).tiny)).sum() >= 100
    # the rows of the engine and of the oracle under both tie rules lie inside the envelope
    plain = vfree(g)[S][:, None] & vfree(g)[None, :]
    (_, rel, _), _ = call(route, eng.rows, S, T, dispatch=False)
    og = oracle_mod.OracleGraph(g)
    hl = has_loop(g)
    rows = [rel]
    for tie in (oracle_mod.TIE_IGRAPH, oracle_mod.TIE_MINKEY):
        r = np.full(rel.shape, np.nan)
        for i, s in enumerate(S.tolist()):
            keep = np.ones(g.n, bool) if hl[s] else T != s
            r[i, keep] = og.source_row(s, T[keep], tie)[1]
        rows.append(r)
    assert eq(rows[0][plain], rows[2][plain])                          # the engine's rule is TIE_MINKEY
    for r in rows:
        assert np.array_equal(np.isnan(r), ~ok)
        inside = ok & (plain | (hi == 0.0))
        assert np.all((lo[inside] <= r[inside]) & (r[inside] <= hi[inside]))
        assert np.all(r[ok & (hi == 0.0)] == 0.0)
    one = ok & (cnt == 1) & plain
    assert eq(rows[0][one], lo[one])
    eng.close()


def front_ties(g, A, cnt, lo, hi):
    """tests/test_ties_gpu._front_ref over the given envelope of A x A: (stats, lines)."""
    st = dict(pairs=0, tied=0, sensitive=0, saturated=0, max_spread=0.0, worst_src=-1, worst_dst=-1, worst_count=0,
              worst_lo=0.0, worst_hi=0.0)
    sep = "-->" if g.directed else "<-->"
    lines = []
    for i in range(len(A)):
        for j in range(i + 1, len(A)):
            c, l, h = int(cnt[i, j]), float(lo[i, j]), float(hi[i, j])
            if c == 0:
                continue
            st["pairs"] += 1
            st["tied"] += c > 1
            st["saturated"] += c == 2 ** 64 - 1
            if l == h:
                continue
            st["sensitive"] += 1
            spread = (h - l) / h
            if spread > st["max_spread"]:
                st.update(max_spread=spread, worst_src=int(A[i]), worst_dst=int(A[j]), worst_count=c, worst_lo=l, worst_hi=h)
            lines.append("tie %d%s%d (%d%s%d) has %d shortest paths, reliability %.17g to %.17g, spread %.17g"
                         % (A[i], sep, A[j], A[i], sep, A[j], c, l, h, spread))
    lines.append("ties: %d pairs, %d tied, %d sensitive, %d saturated, max spread %.17g at (%d%s%d) with %d paths"
                 % (st["pairs"], st["tied"], st["sensitive"], st["saturated"], st["max_spread"], st["worst_src"], sep,
                    st["worst_dst"], st["worst_count"]))
    return st, lines


def test_front_end_ties(topo, route, tmp_path):
    """Topology.tie_stats and dump_ties on rel_zero_ties: lines whose envelope reaches down to 0
    (spread 1), and tied pairs whose every path is dead: rel_lo == rel_hi == 0 is no sensitive
    pair (no line, no division by rel_hi); shd_topology_tie_line, asked for one of them, prints
    the spread 0 that tie_fmt.c's guard gives, as tests/tie_fmt_main.c states it."""
    name = "rel_zero_ties"
    g = rg.get(name)
    A = np.flatnonzero(has_loop(g))[::4].astype(np.int32)
    assert len(A) >= 60
    cnt, lo, hi, _ = tr.TiesRef(g).rows(A, A, True)
    want, lines = front_ties(g, A, cnt, lo, hi)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    assert t.tie_stats() == want
    assert want["pairs"] == len(A) * (len(A) - 1) // 2 and want["sensitive"] >= 10 and want["max_spread"] == 1.0
    assert want["worst_lo"] == 0.0 < want["worst_hi"]
    out = tmp_path / "ties.txt"
    t.dump_ties(str(out))
    assert out.read_text().splitlines() == lines and len(lines) == want["sensitive"] + 1
    assert sum(", reliability 0 to " in ln and ln.endswith(", spread 1") for ln in lines) >= 5
    iu = np.triu_indices(len(A), 1)
    dead = np.flatnonzero((cnt[iu] > 1) & (hi[iu] == 0.0))
    assert len(dead) >= 3
    i, j = int(iu[0][dead[0]]), int(iu[1][dead[0]])
    L = topo.load_library()
    L.shd_topology_tie_line.restype = C.c_int64
    L.shd_topology_tie_line.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_uint64, C.c_double, C.c_double, C.c_int]
    buf, cap = C.c_void_p(), C.c_size_t(0)
    k = L.shd_topology_tie_line(C.byref(buf), C.byref(cap), None, int(A[i]), int(A[j]), int(cnt[i, j]),
                                float(lo[i, j]), float(hi[i, j]), 0)
    text = C.string_at(buf.value, k).decode()
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(buf)
    assert text == "tie %d<-->%d (%d<-->%d) has %d shortest paths, reliability 0 to 0, spread 0" % (
        A[i], A[j], A[i], A[j], cnt[i, j])
    t.close()


# ---- folds -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", FOLD_GRAPHS)
def test_fold_product_is_the_rows_reliability(route, monkeypatch, name, form):
    """PROD of 1 - loss: the fold kernel's left fold along the route against the rows kernel's
    (and the oracle's), exact zeros and subnormals included; a failed self entry is NaN in both."""
    ref = rows_reference(name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    choose(monkeypatch, form)
    eng = route.RouteEngine(g)
    vals = (1.0 - np.asarray(g.packetloss, np.float64))[None, :]
    (_, rel, _), c1 = call(route, eng.rows, S, T, dispatch=False)
    out, c2 = call(route, eng.fold, S, T, [fr.PROD], vals, dispatch=False)
    assert c1 == c2 and out.shape == (1, len(S), len(T))
    assert eq(out[0], rel) and eq(out[0], ref["rel"])
    tiny = np.finfo(np.float64).tiny
    if name.startswith("rel_deep"):
        assert ((out[0] > 0.0) & (out[0] < tiny)).sum() >= 300 and (out[0] == 0.0).sum() >= 2000
    if name.startswith("rel_zero"):
        assert (out[0] == 0.0).mean() >= 0.2
    eng.close()


@pytest.mark.parametrize("form", FORMS)
def test_fold_min_max_and_pairs(route, monkeypatch, form):
    """rel_zero: MIN, MAX and PROD of the reliability column over the block against
    tests/fold_ref.py (a minimum of exactly 0, a maximum of exactly 1), and pair_fold on 200
    pairs, some twice, some self pairs, on rel_zero and on the chain."""
    choose(monkeypatch, form)
    ops = [fr.MIN, fr.MAX, fr.PROD]
    for name in ("rel_zero", "rel_deep"):
        g = rg.get(name)
        S, T = rg.sources(name), np.arange(g.n, dtype=np.int32)
        col = 1.0 - np.asarray(g.packetloss, np.float64)
        vals = np.stack([col, col, col])
        F = fr.FoldRef(g)
        eng = route.RouteEngine(g)
        if name == "rel_zero":
            want, codes = F.rows(S, T, ops, vals)
            out, c = call(route, eng.fold, S, T, ops, vals, dispatch=False)
            assert ((c in codes) if codes else c == route.OK) and fr.same(out, want)
            ok = ~np.isnan(want[0])
            assert (want[0][ok] == 0.0).mean() >= 0.2 and (want[1][ok] == 1.0).sum() >= 100
            assert np.array_equal(want[2][ok] == 0.0, want[0][ok] == 0.0)
        rng = np.random.default_rng(g.n)
        ps = rng.choice(S, size=200).astype(np.int32)
        pt = rng.integers(0, g.n, size=200).astype(np.int32)
        pt[:5] = ps[:5]
        ps, pt = np.concatenate([ps, ps[40:60]]), np.concatenate([pt, pt[40:60]])
        want, codes = F.pairs(ps, pt, ops, vals)
        out, c = call(route, eng.pair_fold, ps, pt, ops, vals, dispatch=False)
        assert ((c in codes) if codes else c == route.OK) and fr.same(out, want)
        ref = rows_reference(name)
        assert eq(out[2], ref["rel"][np.searchsorted(S, ps), pt])
        eng.close()


# ---- link loss -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loss_reference(name):
    """The one-source f64 programmes (every product watched on the graphs of LOSS_BLOCK) and, on
    those graphs, the weighted block in exact fractions."""
    g = rg.get(name)
    S, T = rg.sources(name), np.arange(g.n, dtype=np.int32)
    W = loss_weights(name)
    L = Watched(g) if name in LOSS_BLOCK else lr.LossRef(g)
    at = np.unique(np.linspace(0, len(S) - 1, LOSS_ONE).astype(int)).tolist()
    if name == "rel_vzero":
        dead = rg.vclasses(g)[0]
        at = sorted(set(at) | {int(np.flatnonzero(S == dead[-1])[0])})
    one = [L.block(S[i:i + 1], T, W[i:i + 1]) for i in at]
    block = lr.LossRef(g).block(S, T, W, exact=True) if name in LOSS_BLOCK else None
    return dict(g=g, S=S, T=T, W=W, at=at, one=one, block=block)


def compare(route, got, code, want, exact_bits):
    assert got[4] == want.unrouted
    assert (code in want.codes) if want.codes else code == route.OK, (code, want.codes)
    for k in range(4):
        if exact_bits:
            a = want.arrays()[k]
            bad = np.flatnonzero(got[k] != a)
            assert np.array_equal(got[k], a), (lr.NAMES[k], len(bad), bad[:5].tolist(), got[k][bad[:5]].tolist(),
                                               a[bad[:5]].tolist())
        else:
            assert lr.close(got[k], want.outs()[k], want.R, want.A), (lr.NAMES[k], want.R, want.A)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", LOSS_GRAPHS)
def test_loss(route, monkeypatch, name, form):
    ref = loss_reference(name)
    g, S, T, W = ref["g"], ref["S"], ref["T"], ref["W"]
    choose(monkeypatch, form)
    eng = route.RouteEngine(g)
    tiny = np.finfo(np.float64).tiny
    sub = 0
    for i, want in zip(ref["at"], ref["one"]):
        assert want.A <= 2
        got, code = call(route, eng.loss, S[i:i + 1], T, W[i:i + 1], dispatch=False)
        compare(route, got, code, want, True)
        sub += sum(int(((a > 0.0) & (a < tiny)).sum()) for a in got[:4])
    if name == "rel_deep":
        assert sub >= 8                                            # subnormal packets, bit for bit
    if name == "rel_vzero":                                          # a dead source: all it sends is dropped at once
        dead = rg.vclasses(g)[0]
        i = int(np.flatnonzero(S == dead[-1])[0])
        got, _ = call(route, eng.loss, S[i:i + 1], T, W[i:i + 1], dispatch=False)
        assert not got[0].any() and not got[3].any() and got[2][S[i]] > 0 and np.count_nonzero(got[2]) == 1
    if ref["block"] is not None:
        want = ref["block"]
        assert want.A > 2
        got, code = call(route, eng.loss, S, T, W, dispatch=False)
        compare(route, got, code, want, False)
        # the pair form: the same entries as pairs, in no order
        ps, pt = np.repeat(S, g.n).astype(np.int32), np.tile(T, len(S)).astype(np.int32)
        o = np.random.default_rng(g.n).permutation(len(ps))
        got, code = call(route, eng.pair_loss, ps[o], pt[o], W.reshape(-1)[o], dispatch=False)
        compare(route, got, code, want, False)
    eng.close()


@pytest.mark.parametrize("form", FORMS)
def test_tiny_loss_still_drops(route, monkeypatch, form):
    """rel_tinyloss against its copy without the 2**-60 losses: the same reliabilities, so the same
    packets reach every link and are delivered, bit for bit; the links of loss 2**-60 that carry
    traffic drop a positive number of packets, and nothing in the copy."""
    g = rg.get("rel_tinyloss")
    h = rg.without_loss(g)
    S, T = rg.sources("rel_tinyloss"), np.arange(g.n, dtype=np.int32)
    W = loss_weights("rel_tinyloss")
    choose(monkeypatch, form)
    eg, eh = route.RouteEngine(g), route.RouteEngine(h)
    tiny = g.packetloss == rg.TINY
    loaded = 0
    for i in (0, len(S) // 2, len(S) - 1):
        a, ca = call(route, eg.loss, S[i:i + 1], T, W[i:i + 1], dispatch=False)
        b, cb = call(route, eh.loss, S[i:i + 1], T, W[i:i + 1], dispatch=False)
        assert ca == cb and a[4] == b[4]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2])
        on = tiny & (a[0] > 0.0)
        assert np.all(a[1][on] > 0.0) and np.array_equal(a[1][on], a[0][on] * rg.TINY) and not b[1][tiny].any()
        assert np.array_equal(a[1][~tiny], b[1][~tiny])
        loaded += int(on.sum())
    assert loaded >= 100
    eg.close(); eh.close()


def test_front_end_link_loss(topo, route):
    """Topology.link_loss on rel_zero: packet counters on a few hundred stored pairs against the
    reference over the stored pairs (lower -> higher); dead links pass nothing on."""
    g = rg.get("rel_zero")
    A = np.flatnonzero(has_loop(g))[::3].astype(np.int32)
    t = topo.Topology.from_graph(g)
    t.attach_all(A)
    rng = np.random.default_rng(len(A))
    P = rng.choice(A, size=(300, 2))
    P[:6, 1] = P[:6, 0]
    for (a, b), k in zip(P.tolist(), rng.integers(1, 1000, size=len(P)).tolist()):
        t.add_path_packets(a, b, k)
    ps, pt, pw = [], [], []
    for i, a in enumerate(A.tolist()):
        for b in A[i:].tolist():
            c = t.packet_count(a, b)
            if c:
                ps.append(a); pt.append(b); pw.append(c)
    assert len(ps) > 100
    want = lr.LossRef(g).pairs(ps, pt, pw, dispatch=True, exact=True)
    got = t.link_loss()
    assert got[4] == want.unrouted == 0
    for k in range(4):
        assert lr.close(got[k], want.outs()[k], want.R, want.A), lr.NAMES[k]
    # q = 1.0 drops all of it: exactly so in the fractions, which both outputs are held to above (a
    # link's addends reach the two arrays by atomic adds in an order of their own, so the two
    # doubles may differ in the last place)
    on = np.flatnonzero((g.packetloss == 1.0) & (got[0] > 0.0))
    assert len(on) >= 10 and all(want.edge_drop[e] == want.edge_reach[e] > 0 for e in on.tolist())
    assert np.all(got[1][on] > 0.0)
    assert (got[3] > 0.0).sum() > 0
    t.close()
