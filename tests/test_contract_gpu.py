"""GPU: the output contract of the device-pointer entry points (include/shd_route.h), for every
kernel behind them, on a narrow graph (internet_like(389, 3), the self-loops of a third of the
vertices removed) and a wide-range one (range_graphs "wide_mid"):

  row stride   outputs are written at [i * ld + j], j < nt, and nowhere else: with ld = nt + 1
               and nt + 5 (odd and even strides, rows of both 16-byte parities), from a base
               that is 16-byte aligned and one that is only 8-byte aligned, the columns past nt
               and the guard elements around the buffer keep their canary bit for bit, and the
               nt columns equal the ld == nt result bit for bit
  targets      all vertices, a sorted subset of odd length, an unsorted list with repeats, and
               nt == 1; 11 sources, one repeated, some without a self-loop
  NULL outputs each output alone gives the values of the full call
  failures     t == s without a self-loop: NaN in lat and rel (-1 in hops), the rest of the row
               exact, SHD_ROUTE_ENOEDGE from the next shd_route_sync and none from the one
               after; row_min over the entries that exist, +inf when none does

Every result is also held to the CPU oracle (TIE_MINKEY; neither graph has vertex loss, so
reliability is bit-exact).
"""
import dataclasses

import numpy as np
import pytest

from shadow_amd.graph import complete_graph, internet_like
from tests import range_graphs as rg
from tests.test_range_gpu import SELECTIONS, fw_accepts, has_loop, oracle_rows, row_min_of, select

pytestmark = pytest.mark.gpu

CAN64 = 0x7FF8DEADBEEF0001   # (a NaN with a payload no kernel produces)
CAN32 = 0x5EADBEEF
GUARD = 16                   # elements before and after: 128 / 64 bytes, keeps the base 16-byte aligned
NS = 11


@pytest.fixture(scope="module")
def route():
    from shadow_amd import route as r
    r.load_library()
    return r


@pytest.fixture(autouse=True)
def close_engines(route, monkeypatch):
    """Every context a test makes is closed (its plans first) when the test ends, also when it
    fails half-way: none is left for the collector to finalise during a later test."""
    made = []
    real = route.RouteEngine

    def tracked(*a, **k):
        made.append(real(*a, **k))
        return made[-1]
    monkeypatch.setattr(route, "RouteEngine", tracked)
    yield
    for e in reversed(made):
        e.close()


def narrow():
    g = internet_like(389, 3, seed=33, name="narrow389")
    keep = (g.src != g.dst) | (g.src % 3 != 1)
    return dataclasses.replace(g, src=g.src[keep], dst=g.dst[keep], latency=g.latency[keep],
                               packetloss=g.packetloss[keep], vertex_packetloss=None)


_G = {}


def graph(name):
    if name not in _G:
        _G[name] = narrow() if name == "narrow" else rg.get(name)
    return _G[name]


def source_list(g):
    """11 sources: vertex 0, the highest vertex, four with and four without a self-loop, and
    the first self-loop-free one again."""
    hl = has_loop(g)
    a = [int(v) for v in np.flatnonzero(hl) if v not in (0, g.n - 1)]
    b = [int(v) for v in np.flatnonzero(~hl) if v not in (0, g.n - 1)]
    pick = [0, g.n - 1] + [a[k * len(a) // 4] for k in range(4)] + [b[k * len(b) // 4] for k in range(4)] + [b[0]]
    assert len(pick) == NS
    return np.array(pick, np.int32)


def target_lists(g, S):
    rng = np.random.default_rng(3)
    sub = np.unique(np.concatenate([S[2:7], np.arange(2, g.n, 4)]))
    sub = sub[: len(sub) - 1 + len(sub) % 2]
    uns = np.concatenate([rng.permutation(g.n)[:60], S[[9, 3, 9]], [5, 5]])
    return {"all": np.arange(g.n, dtype=np.int32), "subset": sub.astype(np.int32),
            "unsorted": uns.astype(np.int32), "one": S[6:7].copy()}


_REF = {}


def reference(oracle_mod, gname, tname):
    key = (gname, tname)
    if key not in _REF:
        g = graph(gname)
        S = source_list(g)
        T = target_lists(g, S)[tname]
        assert tname != "subset" or (len(T) % 2 == 1 and np.all(np.diff(T) > 0))
        lat, rel, hops = oracle_rows(oracle_mod, oracle_mod.OracleGraph(g), g, S, T)
        _REF[key] = dict(g=g, S=S, T=T, lat=lat, rel=rel, hops=hops, failed=bool(np.isnan(lat).any()))
    return _REF[key]


class Padded:
    """An ns x ld output carved from a canary-filled device buffer, GUARD elements in from its
    start (+ 8 bytes with `shift`: then the base is 8- but not 16-byte aligned)."""

    def __init__(self, ns, ld, i32=False, shift=0):
        import torch
        self.ns, self.ld = ns, ld
        self.can = CAN32 if i32 else CAN64
        self.off = GUARD + (2 if i32 else 1) * shift
        self.big = torch.full((self.off + ns * ld + GUARD,), self.can, dtype=torch.int32 if i32 else torch.int64,
                              device=torch.device("cuda", 0))
        flat = self.big[self.off: self.off + ns * ld]
        self.t = (flat if i32 else flat.view(torch.float64)).view(ns, ld)
        assert self.t.data_ptr() % 16 == 8 * shift

    def bits(self, nt):
        """The nt written columns as integers, after checking that nothing else changed."""
        b = self.big.cpu().numpy()
        assert np.all(b[: self.off] == self.can) and np.all(b[self.off + self.ns * self.ld:] == self.can)
        body = b[self.off: self.off + self.ns * self.ld].reshape(self.ns, self.ld)
        assert np.all(body[:, nt:] == self.can)
        return body[:, :nt].copy()

    def untouched(self):
        return bool(np.all(self.big.cpu().numpy() == self.can))


def sync_code(route, eng):
    try:
        eng.sync()
        return route.OK
    except route.RouteError as e:
        return e.code


def run(route, eng, launch, S, T, ld, shift=0, outs=(1, 1, 1), i32=False):
    """One launch into padded outputs: (bits of out0, out1, row reduction, sync code).  `outs`
    selects which outputs are passed; the others are left NULL and must stay untouched."""
    import torch
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(np.ascontiguousarray(S, np.int32)).to(dev)
    d_t = torch.from_numpy(np.ascontiguousarray(T, np.int32)).to(dev)
    ns, nt = len(S), len(T)
    a, b, m = Padded(ns, ld, i32, shift), Padded(ns, ld, i32, shift), Padded(ns, 1, i32, shift)
    launch(d_s, d_t, a.t if outs[0] else None, b.t if outs[1] else None, m.t if outs[2] else None, ld)
    code = sync_code(route, eng)
    assert sync_code(route, eng) == route.OK          # reported once
    res = []
    for k, (p, w) in enumerate(zip((a, b, m), (nt, nt, 1))):
        if outs[k]:
            res.append(p.bits(w))
        else:
            assert p.untouched()
            res.append(None)
    return res[0], res[1], res[2], code


def f64(bits):
    return None if bits is None else bits.view(np.float64)


def contract(route, eng, launch, ref, hops=False):
    """The whole contract for one entry point and one (sources, targets) request."""
    S, T = ref["S"], ref["T"]
    nt = len(T)
    a0, b0, m0, c0 = run(route, eng, launch, S, T, nt, i32=hops)
    # values: the oracle's, failed entries NaN / -1, the row reduction over the rest
    assert c0 == (route.ENOEDGE if ref["failed"] else route.OK)
    if hops:
        assert np.array_equal(a0, ref["hops"])
        assert np.array_equal(m0[:, 0], ref["hops"].max(axis=1))
    else:
        assert np.array_equal(f64(a0), ref["lat"], equal_nan=True)
        assert np.array_equal(f64(b0), ref["rel"], equal_nan=True)
        assert np.array_equal(f64(m0)[:, 0], row_min_of(ref["lat"]))
        assert np.array_equal(np.isnan(f64(a0)), np.isnan(f64(b0)))
    # strides and base alignments
    for ld, shift in ((nt + 1, 0), (nt + 1, 1), (nt + 5, 0), (nt + 5, 1), (nt, 1)):
        a, b, m, c = run(route, eng, launch, S, T, ld, shift, i32=hops)
        assert np.array_equal(a, a0) and np.array_equal(m, m0) and c == c0, (ld, shift)
        assert hops or np.array_equal(b, b0), (ld, shift)
    # each output alone
    for outs in ((1, 0), (0, 1)) if hops else ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        o = outs if not hops else (outs[0], 0, outs[1])
        a, b, m, c = run(route, eng, launch, S, T, nt + 1, 1, outs=o, i32=hops)
        assert c == c0
        for got, want in ((a, a0), (b, b0), (m, m0)):
            assert got is None or np.array_equal(got, want), outs


LAUNCHERS = list(SELECTIONS) + ["fw", "plan_auto", "plan_kd", "hops", "hops_kd"]
GRAPHS = ("narrow", "wide_mid")
TARGETS = ("all", "subset", "unsorted", "one")


@pytest.mark.parametrize("tname", TARGETS)
@pytest.mark.parametrize("how", LAUNCHERS)
@pytest.mark.parametrize("gname", GRAPHS)
def test_contract(route, oracle_mod, monkeypatch, gname, how, tname):
    ref = reference(oracle_mod, gname, tname)
    g, S = ref["g"], ref["S"]
    sel = how if how in SELECTIONS else "kd" if how.endswith("_kd") else "auto"
    select(monkeypatch, sel)
    eng = route.RouteEngine(g)
    if how in SELECTIONS:
        def launch(d_s, d_t, lat, rel, mn, ld):
            eng.rows_async(d_s, d_t, lat, rel, mn, dispatch=False, ld=ld)
        contract(route, eng, launch, ref)
    elif how == "fw":
        assert fw_accepts("wide_mid", eng.info, g.n)   # (both graphs: integer, u16, LDS-sized)
        def launch(d_s, d_t, lat, rel, mn, ld):
            eng.fw_table_async()
            eng.fw_rows_async(d_s, d_t, lat, rel, mn, ld=ld)
        contract(route, eng, launch, ref)
    elif how.startswith("plan"):
        plan = eng.plan(S)
        assert plan.info["rows"] == NS
        assert plan.info["seeded"] == int(how == "plan_kd" and gname == "narrow")
        rows = dict(ref)
        for k in ("lat", "rel", "hops"):
            rows[k] = ref[k][plan.positions]
        rows["S"] = S[plan.positions]
        def launch(d_s, d_t, lat, rel, mn, ld):
            plan.rows_async(d_t, lat, rel, mn, dispatch=False, ld=ld)
        contract(route, eng, launch, rows)
        plan.close()
    else:
        def launch(d_s, d_t, hops, _none, mx, ld):
            eng.hops_async(d_s, d_t, hops, mx, dispatch=False, ld=ld)
        contract(route, eng, launch, ref, hops=True)
    eng.close()


def test_kernels_behind_the_contract(route, monkeypatch):
    """The narrow graph takes the compact forms (KB fused rows, KD's packed records, a seeded
    plan), the wide one their fallbacks; both KF forms run on the narrow one."""
    want = {("narrow", "auto"): (2, 1), ("wide_mid", "auto"): (2, 0), ("narrow", "kbfuse0"): (2, 0),
            ("narrow", "kd"): (4, None), ("wide_mid", "kd"): (4, None), ("narrow", "k32"): (1, 0),
            ("wide_mid", "k32"): (1, 0), ("narrow", "f64"): (0, 0), ("narrow", "kf"): (5, 0),
            ("narrow", "kfh"): (5, 1), ("wide_mid", "kf"): (0, 0), ("wide_mid", "kfh"): (0, 0)}
    for (gname, sel), (kernel, reserved) in want.items():
        select(monkeypatch, sel)
        e = route.RouteEngine(graph(gname))
        assert e.info["kernel"] == kernel, (gname, sel)
        assert reserved is None or e.info["reserved"] == reserved, (gname, sel)
        e.close()


@pytest.mark.parametrize("tname", TARGETS)
def test_contract_complete_dispatch(route, oracle_mod, monkeypatch, tname):
    """rows_async with SHD_ROUTE_DISPATCH on a complete graph: direct_rows_kernel."""
    select(monkeypatch, "auto")
    g = complete_graph(67, seed=3)
    eng = route.RouteEngine(g)
    assert eng.info["is_complete"] == 1
    og = oracle_mod.OracleGraph(g)
    S = np.array([0, 66, 5, 17, 31, 32, 33, 64, 65, 1, 5], np.int32)
    T = {"all": np.arange(67), "subset": np.arange(1, 67, 2), "unsorted": np.array([66, 3, 3, 0, 41, 5, 17, 5]),
         "one": np.array([5])}[tname].astype(np.int32)
    lat = np.empty((NS, len(T))); rel = np.empty((NS, len(T)))
    for i, s in enumerate(S):
        for j, t in enumerate(T):
            lat[i, j], rel[i, j] = og.direct(int(s), int(t))
    ref = dict(S=S, T=T, lat=lat, rel=rel, failed=False)
    def launch(d_s, d_t, la, re, mn, ld):
        eng.rows_async(d_s, d_t, la, re, mn, dispatch=True, ld=ld)
    contract(route, eng, launch, ref)
    eng.close()


@pytest.mark.parametrize("how", ["auto", "kd", "kb", "k32", "f64", "kf", "kfh", "fw", "plan_kd", "hops"])
@pytest.mark.parametrize("gname", GRAPHS)
def test_row_of_failures_only(route, monkeypatch, gname, how):
    """tgt = [s] for sources without a self-loop: every entry of the row failed, row_min is
    +inf (hops: row_max -1); the row of a self-looped source beside them is its self entry."""
    import torch
    g = graph(gname)
    hl = has_loop(g)
    s = int(np.flatnonzero(~hl)[3])
    sel = how if how in SELECTIONS else "kd" if how.endswith("_kd") else "auto"
    select(monkeypatch, sel)
    eng = route.RouteEngine(g)
    dev = torch.device("cuda", 0)
    d_s = torch.tensor([s, s], dtype=torch.int32, device=dev)
    lat = torch.zeros((2, 1), dtype=torch.float64, device=dev); rel = torch.zeros_like(lat)
    mn = torch.zeros(2, dtype=torch.float64, device=dev)
    if how == "hops":
        h = torch.zeros((2, 1), dtype=torch.int32, device=dev); mx = torch.zeros(2, dtype=torch.int32, device=dev)
        eng.hops_async(d_s, d_s[:1], h, mx, dispatch=False)
    elif how == "fw":
        eng.fw_table_async()
        eng.fw_rows_async(d_s, d_s[:1], lat, rel, mn)
    elif how == "plan_kd":
        plan = eng.plan(np.array([s, s], np.int32))
        plan.rows_async(d_s[:1], lat, rel, mn, dispatch=False)
    else:
        eng.rows_async(d_s, d_s[:1], lat, rel, mn, dispatch=False)
    with pytest.raises(route.RouteError) as ei:
        eng.sync()
    assert ei.value.code == route.ENOEDGE
    eng.sync()
    if how == "hops":
        assert h.cpu().tolist() == [[-1], [-1]] and mx.cpu().tolist() == [-1, -1]
    else:
        assert np.isnan(lat.cpu().numpy()).all() and np.isnan(rel.cpu().numpy()).all()
        assert mn.cpu().tolist() == [float("inf")] * 2
    eng.close()


def test_host_calls_attach_partial_rows(route, oracle_mod, monkeypatch):
    """RouteEngine.rows() raises on a failed entry; err.partial holds what shd_route_rows
    wrote (every row, NaN at the failed entries, row_min over the rest)."""
    select(monkeypatch, "auto")
    ref = reference(oracle_mod, "wide_mid", "all")
    eng = route.RouteEngine(ref["g"])
    with pytest.raises(route.RouteError) as ei:
        eng.rows(ref["S"], ref["T"], dispatch=False)
    assert ei.value.code == route.ENOEDGE
    lat, rel, mn = ei.value.partial
    assert np.array_equal(lat, ref["lat"], equal_nan=True) and np.array_equal(rel, ref["rel"], equal_nan=True)
    assert np.array_equal(mn, row_min_of(ref["lat"]))
    ok = ref["S"][[0, 2, 3]] if has_loop(ref["g"])[0] else ref["S"][[2, 3]]
    lat, rel, mn = eng.rows(ok, ref["T"], dispatch=False)      # no failure: returned as before
    assert not np.isnan(lat).any()
    eng.close()


# ---- shd_route_tri_payload_async: the input row stride ------------------------------------

@pytest.mark.parametrize("lat16", [True, False])
@pytest.mark.parametrize("gname", GRAPHS)
def test_payload_input_stride(route, oracle_mod, monkeypatch, gname, lat16):
    """Rows with NaN diagonals, stored with ld = na, na + 1 and na + 5 from both base
    alignments, pack to the same payload; LAT16 codes NaN as 0xFFFF, the f64 payload keeps it."""
    import torch
    from shadow_amd.shard import decode_lat16, pack_triangle_host, tri_offsets
    select(monkeypatch, "auto")
    ref = reference(oracle_mod, gname, "subset")
    g, A = ref["g"], ref["T"]
    na = len(A)
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1
    posof = {int(v): k for k, v in enumerate(A)}
    rows = [i for i, s in enumerate(ref["S"]) if int(s) in posof]
    pos = np.array([posof[int(ref["S"][i])] for i in rows], np.int32)
    lat, rel = ref["lat"][rows], ref["rel"][rows]
    assert np.isnan(lat[np.arange(len(pos)), pos]).any() and len(pos) >= 5
    off, tot = tri_offsets(pos, na)
    hl, hr = pack_triangle_host(lat, rel, pos, na, lat16=lat16)
    dev = torch.device("cuda", 0)
    d_pos = torch.from_numpy(pos).to(dev); d_off = torch.from_numpy(off[:-1].copy()).to(dev)
    for ld, shift in ((na, 0), (na + 1, 0), (na + 1, 1), (na + 5, 0), (na + 5, 1), (na, 1)):
        il, ir = Padded(len(pos), ld, shift=shift), Padded(len(pos), ld, shift=shift)
        il.t[:, :na] = torch.from_numpy(lat).to(dev); ir.t[:, :na] = torch.from_numpy(rel).to(dev)
        ol = Padded(1, tot, i32=False, shift=shift) if not lat16 else None
        o16 = torch.full((GUARD + tot + GUARD,), 0x5EAD, dtype=torch.int16, device=dev)
        orr = Padded(1, tot, shift=shift)
        out_l = ol.t if ol is not None else o16[GUARD: GUARD + tot]
        eng.tri_payload_async(il.t, ir.t, d_pos, d_off, na, out_l, orr.t, lat16=lat16, ld=ld)
        assert sync_code(route, eng) == route.OK
        R = orr.bits(tot).view(np.float64)[0]
        assert np.array_equal(R, hr, equal_nan=True)
        if lat16:
            o = o16.cpu().numpy()
            assert np.all(o[:GUARD] == 0x5EAD) and np.all(o[GUARD + tot:] == 0x5EAD)
            L = o[GUARD: GUARD + tot].view(np.uint16)
            assert np.array_equal(L, hl) and np.array_equal(L == 0xFFFF, np.isnan(hr))
            assert np.array_equal(decode_lat16(L), np.concatenate([lat[r, p:] for r, p in enumerate(pos)]), equal_nan=True)
        else:
            L = ol.bits(tot).view(np.float64)[0]
            assert np.array_equal(L, hl, equal_nan=True) and np.array_equal(np.isnan(L), np.isnan(hr))
    eng.close()
