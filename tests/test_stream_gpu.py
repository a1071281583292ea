"""GPU: stream order of every *_async entry point (include/shd_route.h: "enqueued on `stream`;
returns after enqueueing"), on a torch side stream, which does not block against the NULL stream.

  gated calls   tests/stream_order.py: each entry point behind a timed gate, decoys in every
                device input until the gate opens and again after the call's work; a memset, a
                counter reset, a record upload or a kernel the engine left on another stream,
                or an input it read on the host, shows as a wrong row every time
  a chain       rows, hops, loads, planned rows, min_reduce and rows again on one side stream
                behind one gate, one sync at the end
  growth        the hops scratch and the loads' HBM slices freed and reallocated while earlier
                work of the stream is still queued
  a capture     rows + min_reduce (and planned rows + min_reduce) captured into one graph on a
                capture stream, replayed three times over a source list that changes between
                the replays

Every result is compared bit for bit with the CPU oracle under TIE_MINKEY (no graph here has
vertex loss), hops and loads with the references of tests/test_hops_gpu.py and
tests/test_loads_gpu.py.  The decoy's own reference is asserted to differ from the true one in
every output row before anything runs.

Measured on one MI355X (printed by every gated call; torch.cuda._sleep: 2.40 M cycles per ms).
Host wall time of the warm call's enqueue, ms:
  rows_async, every selection, 11 sources                0.007 - 0.011
  rows_async with SHD_ROUTE_DISPATCH                     0.007
  rows_planned_async: neighbour-seeded                   0.017
    landmark-only, its landmark rows and jobs inside     0.023   (SHD_ROUTE_PLAN_REUSE: 0.013)
    refresh MINE + refresh JOBS + rows with reuse        0.025 - 0.028
  hops_async, three chunks (either state form)           0.057 - 0.059
  loads_async, three chunks (either form, with / without ADD)   0.078 - 0.081
  min_reduce_async                                       0.005 - 0.007
  tri_payload_async                                      0.006 - 0.007
  fw_table_async + fw_rows_async (389 vertices)          0.046 - 0.047;  fw_async (60): 0.017
  the chain of six calls                                 0.072 - 0.100
Ten times any of these is far below the floor, so every gate was 20.0 ms, and every gate was
still shut on return at the first try.  No entry point waited for the device in its steady
state; the 58 tests of this file take 1.9 s together.

The deliberate check (once, on a scratch copy): with shd_route_rows_async's
hipMemsetAsync(d_kd_next) moved to the NULL stream, test_gated_rows_from_the_work_queue failed in
all four cases on rows left unwritten (canary), without a fault; with a workgroup per source
(test_gated_rows) the counter decides nothing and the move goes unseen.
"""
import dataclasses

import numpy as np
import pytest

from shadow_amd.graph import complete_graph
from tests import range_graphs as rg
from tests import shape_graphs
from tests import stream_order as so
from tests import test_loads_gpu as tl
from tests.test_contract_gpu import NS, close_engines, reference, route, source_list  # noqa: F401
from tests.test_range_gpu import (SELECTIONS, dispatch_ref, expect_kernel, fw_accepts, has_loop, oracle_rows,
                                  row_min_of, select)

pytestmark = pytest.mark.gpu

ROWS_CASES = ([("narrow", s) for s in SELECTIONS]
              + [("wide_mid", s) for s in SELECTIONS if s == "f64" or expect_kernel("wide_mid", s) != 0]
              + [("dec100", s) for s in ("kf", "kfh")])


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def decoys_of(ref):
    """The decoy source and target lists of a reference over all vertices, after asserting that
    an engine that read either list (or both) early would get every row wrong."""
    S, T, lat, rel = ref["S"], ref["T"], ref["lat"], ref["rel"]
    assert np.array_equal(T, np.arange(len(T)))
    Sd, Td = so.decoy_sources(S), so.decoy_targets(T)
    rows = np.roll(np.arange(len(S)), -1)
    for x in (lat, rel) + ((ref["hops"],) if "hops" in ref else ()):
        assert so.rows_differ(x[rows], x) and so.rows_differ(x[:, Td], x) and so.rows_differ(x[rows][:, Td], x)
    return Sd, Td


def gated_rows(route, eng, ref, launch, label, hops=False, src=True):
    """A rows-shaped call (launch(d_src, d_tgt, out0, out1, row reduction, ld, stream)) behind the
    gate, ld = nt + 1, held to `ref`."""
    S, T = ref["S"], ref["T"]
    ns, nt = len(S), len(T)
    Sd, Td = decoys_of(ref)
    i_s, i_t = so.In(S, Sd), so.In(T, Td)
    a, b, m = so.Out(ns, nt + 1, i32=hops), so.Out(ns, nt + 1, i32=hops), so.Out(ns, 1, i32=hops)
    code = so.gated(route, eng, ([i_s] if src else []) + [i_t], [a, b, m],
                    lambda sh: launch(i_s.t, i_t.t, a.t, b.t, m.t, nt + 1, sh), label)
    assert code == (route.ENOEDGE if ref["failed"] else route.OK)
    if hops:
        assert np.array_equal(a.snap_bits(nt), ref["hops"])
        assert np.array_equal(m.snap_bits(1)[:, 0], ref["hops"].max(axis=1))
        b.snap_bits(0)                                    # (not passed: all canary)
    else:
        assert eq(a.f64(nt), ref["lat"]) and eq(b.f64(nt), ref["rel"])
        assert np.array_equal(m.f64(1)[:, 0], row_min_of(ref["lat"]))


@pytest.mark.parametrize("gname,sel", ROWS_CASES)
def test_gated_rows(route, oracle_mod, monkeypatch, gname, sel):
    ref = reference(oracle_mod, gname, "all")
    assert ref["failed"] and len(ref["S"]) == NS
    select(monkeypatch, sel)
    eng = route.RouteEngine(ref["g"])
    assert sel in ("auto", "f64") or eng.info["kernel"] == {"kd": 4, "kdwalk0": 4, "kb": 2, "kbfuse0": 2, "k32": 1,
                                                             "kf": 5, "kfh": 5}[sel]
    gated_rows(route, eng, ref,
               lambda s, t, la, re, mn, ld, sh: eng.rows_async(s, t, la, re, mn, stream=sh, dispatch=False, ld=ld),
               f"rows_async {gname} {sel}")


@pytest.mark.parametrize("sel", ["kd", "kdwalk0"])
@pytest.mark.parametrize("gname", ["narrow", "wide_mid"])
def test_gated_rows_from_the_work_queue(route, oracle_mod, monkeypatch, gname, sel):
    """KD with fewer workgroups than sources (SHD_ROUTE_KDGRID=4): a workgroup's first row is its
    block index, the other 7 of the 11 come from the context's work-queue counter, which every
    rows call zeroes on the stream first.  (With a workgroup per source, as in test_gated_rows,
    the counter decides nothing.)  This is the case that fails, on rows left unwritten, when
    that memset is moved to the NULL stream."""
    ref = reference(oracle_mod, gname, "all")
    select(monkeypatch, sel)
    monkeypatch.setenv("SHD_ROUTE_KDGRID", "4")
    eng = route.RouteEngine(ref["g"])
    assert eng.info["kernel"] == 4
    gated_rows(route, eng, ref,
               lambda s, t, la, re, mn, ld, sh: eng.rows_async(s, t, la, re, mn, stream=sh, dispatch=False, ld=ld),
               f"rows_async {gname} {sel} KDGRID=4")


def _table_ref(g, S, lat, rel):
    return dict(g=g, S=S, T=np.arange(g.n, dtype=np.int32), lat=lat, rel=rel, failed=bool(np.isnan(lat).any()))


@pytest.mark.parametrize("which", ["complete", "prefer_direct"])
def test_gated_rows_dispatch(route, oracle_mod, monkeypatch, which):
    """SHD_ROUTE_DISPATCH: direct_rows_kernel over the dense tables on a complete graph, the
    generic kernel with the dispatch bits on a prefer-direct one."""
    select(monkeypatch, "auto")
    if which == "complete":
        g = complete_graph(24, seed=3)
        og = oracle_mod.OracleGraph(g)
        S = np.array([0, 23, 5, 17, 11, 12, 13, 22, 21, 1, 5], np.int32)
        lat = np.empty((NS, g.n)); rel = np.empty((NS, g.n))
        for i, s in enumerate(S):
            for t in range(g.n):
                lat[i, t], rel[i, t] = og.direct(int(s), t)
    else:
        g = dataclasses.replace(rg.get("wide_mid"), prefer_direct=True)
        S = source_list(g)
        lat, rel = dispatch_ref(oracle_mod, g, S, np.arange(g.n, dtype=np.int32))
    eng = route.RouteEngine(g)
    assert eng.info["is_complete"] == int(which == "complete")
    gated_rows(route, eng, _table_ref(g, S, lat, rel),
               lambda s, t, la, re, mn, ld, sh: eng.rows_async(s, t, la, re, mn, stream=sh, dispatch=True, ld=ld),
               f"rows_async dispatch {which}")


# ---- planned rows ---------------------------------------------------------------------------

_FULL = {}


def full_ref(oracle_mod, n):
    """sized{n}: the oracle's whole table (every source over every vertex), computed once."""
    if n not in _FULL:
        g = shape_graphs.get(f"sized{n}")
        S = np.arange(g.n, dtype=np.int32)
        lat, rel, hops = oracle_rows(oracle_mod, oracle_mod.OracleGraph(g), g, S, S)
        _FULL[n] = dict(g=g, lat=lat, rel=rel, hops=hops)
    return _FULL[n]


def smallest_plan(route, monkeypatch, form, world=1, rank=0):
    """(engine, plan, n) on the smallest sized* graph whose plan over all its vertices takes the
    form, as plan_info reports it: "neighbour" a host-built plan whose rows seed each other
    (one launch, rows kept in the row store, more than one level; SHD_ROUTE_KDGRID=7, the knob of
    tests/test_seed_gpu.py's kd fixture, leaves more than 1.5 rows per workgroup slot, which keeps
    the landmark-only rule out), "landmark" a device-built landmark-only plan (the landmark rows
    inside every call)."""
    select(monkeypatch, "kd")
    for k in ("SHD_ROUTE_GPUCHOICE", "SHD_ROUTE_PLANDEV", "SHD_ROUTE_LMALL_REV", "SHD_ROUTE_LANDMARKS",
              "SHD_ROUTE_KDGRID", "SHD_ROUTE_LMALL"):
        monkeypatch.delenv(k, raising=False)
    if form == "neighbour":
        monkeypatch.setenv("SHD_ROUTE_KDGRID", "7")
    infos = []
    for n in shape_graphs.SIZES[:9]:
        eng = route.RouteEngine(shape_graphs.get(f"sized{n}"))
        assert eng.info["kernel"] == 4
        plan = eng.plan(np.arange(n, dtype=np.int32)[::-1].copy(), world, rank)
        i = plan.info
        took = (i["seeded"] == 1 and i["launches"] == 1 and i["stored_rows"] > 0 and i["levels"] >= 2) \
            if form == "neighbour" else (i["seeded"] == 1 and i["launches"] >= 3 and plan.landmarks() is not None)
        infos.append((n, i))
        if took:
            print(form, "plan taken at", n, i)
            return eng, plan, n
        plan.close(); eng.close()
    raise AssertionError(f"no sized graph up to {shape_graphs.SIZES[8]} takes a {form} plan: {infos}")


def plan_ref(oracle_mod, n, plan):
    f = full_ref(oracle_mod, n)
    S = np.arange(n, dtype=np.int32)[::-1][plan.positions]
    assert np.array_equal(S, plan.sources)
    lat, rel = f["lat"][S], f["rel"][S]
    return dict(g=f["g"], S=S, T=np.arange(n, dtype=np.int32), lat=lat, rel=rel, failed=bool(np.isnan(lat).any()))


def gated_plan(route, eng, ref, launch, label):
    """Planned rows behind the gate: the targets are the only caller input."""
    T = ref["T"]
    nr, nt = len(ref["S"]), len(T)
    Td = so.decoy_targets(T)
    assert so.rows_differ(ref["lat"][:, Td], ref["lat"]) and so.rows_differ(ref["rel"][:, Td], ref["rel"])
    i_t = so.In(T, Td)
    a, b, m = so.Out(nr, nt + 1), so.Out(nr, nt + 1), so.Out(nr, 1)
    code = so.gated(route, eng, [i_t], [a, b, m], lambda sh: launch(i_t.t, a.t, b.t, m.t, nt + 1, sh), label)
    assert code == (route.ENOEDGE if ref["failed"] else route.OK)
    assert eq(a.f64(nt), ref["lat"]) and eq(b.f64(nt), ref["rel"])
    assert np.array_equal(m.f64(1)[:, 0], row_min_of(ref["lat"]))


@pytest.mark.parametrize("form,reuse", [("neighbour", False), ("landmark", False), ("landmark", True)])
def test_gated_planned_rows(route, oracle_mod, monkeypatch, form, reuse):
    eng, plan, n = smallest_plan(route, monkeypatch, form)
    ref = plan_ref(oracle_mod, n, plan)
    assert ref["failed"]
    gated_plan(route, eng, ref,
               lambda t, la, re, mn, ld, sh: plan.rows_async(t, la, re, mn, stream=sh, dispatch=False, ld=ld, reuse=reuse),
               f"rows_planned_async {form} sized{n} reuse={int(reuse)}")


def test_gated_split_refresh(route, oracle_mod, monkeypatch):
    """The multi-GPU form, world 3: refresh_async(MINE), refresh_async(JOBS), then the rows with
    SHD_ROUTE_PLAN_REUSE, one after the other on the side stream."""
    seen, failed = [], []
    for rank in range(3):
        eng, plan, n = smallest_plan(route, monkeypatch, "landmark", 3, rank)
        def launch(t, la, re, mn, ld, sh):
            plan.refresh_async(sh, route.REFRESH_MINE)
            plan.refresh_async(sh, route.REFRESH_JOBS)
            plan.rows_async(t, la, re, mn, stream=sh, dispatch=False, ld=ld, reuse=True)
        ref = plan_ref(oracle_mod, n, plan)
        gated_plan(route, eng, ref, launch, f"refresh MINE, JOBS, rows reuse, rank {rank}/3")
        failed.append(ref["failed"])
        seen += plan.positions.tolist()
        plan.close(); eng.close()
    assert sorted(seen) == list(range(n)) and True in failed and False in failed


# ---- hops and loads ---------------------------------------------------------------------------

HOLES = "ba60_holes"   # tests/test_loads_gpu.py: ba60 without the self-loops of the odd vertices


def holes_graph():
    """ba60_holes without its vertex loss (paths, hops and loads do not depend on it; the rows'
    reliability is then bit-exact)."""
    return dataclasses.replace(tl._graph(HOLES)[0], vertex_packetloss=None)


_HOLES = {}


def holes_ref(oracle_mod):
    if not _HOLES:
        g = holes_graph()
        S, T = source_list(g), np.arange(g.n, dtype=np.int32)
        lat, rel, hops = oracle_rows(oracle_mod, oracle_mod.OracleGraph(g), g, S, T)
        _HOLES.update(g=g, S=S, T=T, lat=lat, rel=rel, hops=hops, failed=True)
        assert np.isnan(lat).any()
    return _HOLES


def three_chunks(monkeypatch, n):
    """SHD_ROUTE_HOPS_SCRATCH: 4 sources of loads scratch (16 n bytes each), 5 of hops scratch
    (12 n): the 11 sources take three chunks either way."""
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", str(4 * 16 * n))
    assert -(-NS // 4) == 3 and -(-NS // (4 * 16 // 12)) == 3


@pytest.mark.parametrize("lds", [None, "0"])
def test_gated_hops(route, oracle_mod, monkeypatch, lds):
    select(monkeypatch, "auto")
    ref = holes_ref(oracle_mod)
    three_chunks(monkeypatch, ref["g"].n)
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_HOPS_LDS", lds)
    else:
        monkeypatch.delenv("SHD_ROUTE_HOPS_LDS", raising=False)
    eng = route.RouteEngine(ref["g"])
    gated_rows(route, eng, ref,
               lambda s, t, h, _b, mx, ld, sh: eng.hops_async(s, t, h, mx, stream=sh, dispatch=False, ld=ld),
               f"hops_async HOPS_LDS={lds}", hops=True)


def loads_case(route, ref, seed, ld):
    """Weights (row stride ld), base accumulators and the reference of ref's block: the loads
    alone, and what SHD_ROUTE_LOADS_ADD leaves on top of the base."""
    g, S, T = ref["g"], ref["S"], ref["T"]
    rng = np.random.default_rng(seed)
    W = tl.weights(rng, S, T)
    el, tr, un, codes, _ = tl.ref_loads(route, HOLES, S, T, W, False)
    Wp = np.zeros((len(S), ld), np.uint64)
    Wp[:, :len(T)] = W
    base = [rng.integers(1, 1 << 40, size=k).astype(np.uint64) for k in (len(g.src), g.n, 1)]
    return dict(W=Wp, el=el, tr=tr, un=np.uint64(un), codes=codes, base=base)


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("lds", [None, "0"])
def test_gated_loads(route, oracle_mod, monkeypatch, lds, add):
    select(monkeypatch, "auto")
    ref = holes_ref(oracle_mod)
    g, S, T = ref["g"], ref["S"], ref["T"]
    three_chunks(monkeypatch, g.n)
    if lds is not None:
        monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", lds)
    else:
        monkeypatch.delenv("SHD_ROUTE_LOADS_LDS", raising=False)
    nt = len(T)
    c = loads_case(route, ref, 5, nt + 1)
    # the decoys: other sources, permuted targets, other weights -- and other loads
    Sd, Td = decoys_of(ref)
    Wd = np.roll(c["W"][:, :nt], 7, axis=1)
    dl = tl.ref_loads(route, HOLES, Sd, Td, Wd, False)
    assert not np.array_equal(dl[0], c["el"]) and not np.array_equal(dl[1], c["tr"])
    for s, t, w in ((Sd, T, c["W"][:, :nt]), (S, Td, c["W"][:, :nt]), (S, T, Wd)):
        one = tl.ref_loads(route, HOLES, s, t, w, False)
        assert not np.array_equal(one[0], c["el"]) and not np.array_equal(one[1], c["tr"])
    Wdp = np.zeros_like(c["W"]); Wdp[:, :nt] = Wd
    eng = route.RouteEngine(g)
    i_s, i_t, i_w = so.In(S, Sd), so.In(T, Td), so.In(c["W"], Wdp)
    outs = [so.Out(1, k, i64=True) for k in (len(g.src), g.n, 1)]
    accum = [so.In(b[None, :], (b + np.uint64(1))[None, :], into=o.t) for b, o in zip(c["base"], outs)] if add else []
    code = so.gated(route, eng, [i_s, i_t, i_w], outs,
                    lambda sh: eng.loads_async(i_s.t, i_t.t, i_w.t, outs[0].t, outs[1].t, outs[2].t, stream=sh,
                                               dispatch=False, ld=nt + 1, add=add),
                    f"loads_async LOADS_LDS={lds} add={int(add)}", accum=accum)
    assert code in c["codes"] and c["codes"] == {route.ENOEDGE}
    for o, want, b in zip(outs, (c["el"], c["tr"], np.array([c["un"]])), c["base"]):
        got = o.snap_bits(o.ld)[0].view(np.uint64)
        assert np.array_equal(got, want + b if add else want)


# ---- the other async calls --------------------------------------------------------------------

@pytest.mark.parametrize("count", [(1 << 20) - 3, 1 << 20, (1 << 20) + 1])
def test_gated_min_reduce(route, monkeypatch, count):
    """count on both sides of the one-block limit (direct_fw.hpp kMinOneBlock = 2^20): the
    one-launch form, and the memset + many-block form."""
    select(monkeypatch, "auto")
    eng = route.RouteEngine(holes_graph())
    rng = np.random.default_rng(count)
    v = rng.uniform(5.0, 9.0, size=count)
    v[count - 1] = 1.25                                   # the minimum: the last element
    d = rng.uniform(5.0, 9.0, size=count)
    d[0] = 0.5
    assert v.min() == 1.25 and d.min() == 0.5
    i_v = so.In(v, d)
    out = so.Out(1, 1)
    code = so.gated(route, eng, [i_v], [out], lambda sh: eng.min_reduce_async(i_v.t, out.t, stream=sh),
                    f"min_reduce_async {count}")
    assert code == route.OK and out.f64(1)[0, 0] == 1.25


@pytest.mark.parametrize("lat16", [True, False])
def test_gated_tri_payload(route, oracle_mod, monkeypatch, lat16):
    from shadow_amd.shard import pack_triangle_host, tri_offsets
    select(monkeypatch, "auto")
    ref = holes_ref(oracle_mod)
    g, na = ref["g"], ref["g"].n
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1
    pos = np.unique(ref["S"]).astype(np.int32)              # the rows of the sources, by position
    rows = [int(np.flatnonzero(ref["S"] == p)[0]) for p in pos]
    lat, rel = ref["lat"][rows], ref["rel"][rows]
    off, tot = tri_offsets(pos, na)
    hl, hr = pack_triangle_host(lat, rel, pos, na, lat16=lat16)
    # decoys: the rows in another order under a permutation of the positions (the same total)
    perm = np.roll(np.arange(len(pos)), 3)
    pos_d = pos[perm].copy()
    off_d, tot_d = tri_offsets(pos_d, na)
    assert tot_d == tot and not np.array_equal(off_d, off)
    lat_d, rel_d = np.roll(lat, 1, axis=0), np.roll(rel, 1, axis=0)
    for p, o, la, re in ((pos_d, off_d, lat_d, rel_d), (pos_d, off_d, lat, rel), (pos, off, lat_d, rel_d)):
        dl, dr = pack_triangle_host(la, re, p, na, lat16=lat16)
        assert not eq(dl, hl) and not eq(dr, hr)
    ins = [so.In(lat, lat_d), so.In(rel, rel_d), so.In(pos, pos_d), so.In(off[:-1].copy(), off_d[:-1].copy())]
    o_r = so.Out(1, tot)
    o_l = so.Out16(tot) if lat16 else so.Out(1, tot)
    code = so.gated(route, eng, ins, [o_l, o_r],
                    lambda sh: eng.tri_payload_async(ins[0].t, ins[1].t, ins[2].t, ins[3].t, na, o_l.t, o_r.t,
                                                     lat16=lat16, stream=sh, ld=na),
                    f"tri_payload_async lat16={int(lat16)}")
    assert code == route.OK
    assert eq(o_r.f64(tot)[0], hr)
    assert np.array_equal(o_l.u16(), hl) if lat16 else eq(o_l.f64(tot)[0], hl)


@pytest.mark.parametrize("gname", ["narrow", "wide_mid"])
def test_gated_fw_rows(route, oracle_mod, monkeypatch, gname):
    """K4: shd_route_fw_table_async + shd_route_fw_rows_async, the table rebuilt in every call."""
    ref = reference(oracle_mod, gname, "all")
    select(monkeypatch, "auto")
    eng = route.RouteEngine(ref["g"])
    assert fw_accepts("wide_mid", eng.info, ref["g"].n)
    def launch(s, t, la, re, mn, ld, sh):
        eng.fw_table_async(stream=sh)
        eng.fw_rows_async(s, t, la, re, mn, stream=sh, ld=ld)
    gated_rows(route, eng, ref, launch, f"fw_table_async + fw_rows_async {gname}")


def test_gated_fw(route, oracle_mod, monkeypatch):
    """shd_route_fw_async: the caller's n x n matrix is input and output."""
    select(monkeypatch, "auto")
    g = holes_graph()
    n = g.n
    def matrix(bump):
        d = np.full((n, n), np.inf)
        np.fill_diagonal(d, 0.0)
        nl = g.src != g.dst
        a, b, w = g.src[nl], g.dst[nl], g.latency[nl] + bump
        np.minimum.at(d, (a, b), w); np.minimum.at(d, (b, a), w)
        return d
    want, other = oracle_mod.floyd_warshall(matrix(0.0)), oracle_mod.floyd_warshall(matrix(3.0))
    assert so.rows_differ(want, other)
    eng = route.RouteEngine(g)
    out = so.Out(n, n)
    i_d = so.In(matrix(0.0), matrix(3.0), into=out.t)
    code = so.gated(route, eng, [], [out], lambda sh: eng.fw_async(out.t, stream=sh), "fw_async", accum=[i_d])
    assert code == route.OK and np.array_equal(out.f64(n), want)


# ---- a chain on one stream --------------------------------------------------------------------

@pytest.mark.parametrize("sel", ["auto", "kd", "kb", "kf"])
def test_chain_on_one_stream(route, oracle_mod, monkeypatch, sel):
    """rows, hops, loads, planned rows, min_reduce over the planned rows' row_min and rows again
    (other sources, other buffers) on one side stream behind one gate, no host sync in between:
    every output equals its reference and the failed entries are reported by the one sync, once."""
    select(monkeypatch, sel)
    ref = holes_ref(oracle_mod)
    g, S, T = ref["g"], ref["S"], ref["T"]
    ns, nt = len(S), len(T)
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == {"auto": 2, "kd": 4, "kb": 2, "kf": 5}[sel]
    plan = eng.plan(S)
    assert plan.info["rows"] == ns and plan.info["seeded"] == int(sel == "kd")
    pr = plan.positions
    S2 = np.array([int(v) for v in np.flatnonzero(has_loop(g))[:5]], np.int32)      # (no failed entry here)
    lat2, rel2, _ = oracle_rows(oracle_mod, oracle_mod.OracleGraph(g), g, S2, T)
    c = loads_case(route, ref, 9, nt)
    Sd, Td = decoys_of(ref)
    i_s, i_t, i_w = so.In(S, Sd), so.In(T, Td), so.In(c["W"], np.roll(c["W"], 5, axis=1))
    i_s2 = so.In(S2, np.roll(S2, 1))
    la, re, mn = so.Out(ns, nt), so.Out(ns, nt), so.Out(ns, 1)
    hp, mx = so.Out(ns, nt, i32=True), so.Out(ns, 1, i32=True)
    lo = [so.Out(1, k, i64=True) for k in (len(g.src), g.n, 1)]
    pla, pre, pmn, gmin = so.Out(ns, nt), so.Out(ns, nt), so.Out(ns, 1), so.Out(1, 1)
    la2, re2, mn2 = so.Out(5, nt), so.Out(5, nt), so.Out(5, 1)
    def chain(sh):
        eng.rows_async(i_s.t, i_t.t, la.t, re.t, mn.t, stream=sh, dispatch=False)
        eng.hops_async(i_s.t, i_t.t, hp.t, mx.t, stream=sh, dispatch=False)
        eng.loads_async(i_s.t, i_t.t, i_w.t, lo[0].t, lo[1].t, lo[2].t, stream=sh, dispatch=False)
        plan.rows_async(i_t.t, pla.t, pre.t, pmn.t, stream=sh, dispatch=False)
        eng.min_reduce_async(pmn.t, gmin.t, stream=sh)
        eng.rows_async(i_s2.t, i_t.t, la2.t, re2.t, mn2.t, stream=sh, dispatch=False)
    code = so.gated(route, eng, [i_s, i_t, i_w, i_s2], [la, re, mn, hp, mx, pla, pre, pmn, gmin, la2, re2, mn2] + lo,
                    chain, f"chain {sel}")
    assert code == route.ENOEDGE
    assert eq(la.f64(nt), ref["lat"]) and eq(re.f64(nt), ref["rel"])
    assert np.array_equal(mn.f64(1)[:, 0], row_min_of(ref["lat"]))
    assert np.array_equal(hp.snap_bits(nt), ref["hops"]) and np.array_equal(mx.snap_bits(1)[:, 0], ref["hops"].max(axis=1))
    for o, want in zip(lo, (c["el"], c["tr"], np.array([c["un"]]))):
        assert np.array_equal(o.snap_bits(o.ld)[0].view(np.uint64), want)
    assert eq(pla.f64(nt), ref["lat"][pr]) and eq(pre.f64(nt), ref["rel"][pr])
    assert np.array_equal(pmn.f64(1)[:, 0], row_min_of(ref["lat"][pr]))
    assert gmin.f64(1)[0, 0] == row_min_of(ref["lat"]).min()
    assert eq(la2.f64(nt), lat2) and eq(re2.f64(nt), rel2) and np.array_equal(mn2.f64(1)[:, 0], row_min_of(lat2))


def test_scratch_growth_in_stream_order(route, oracle_mod, monkeypatch):
    """hops of 2 sources, hops of 11, then the loads' HBM form with more sources than the slices
    held, enqueued in a row on a side stream of a context whose warm calls used 2 sources: the
    hops scratch and the loads' slices are freed and reallocated while the earlier work is
    still queued, and all three results are right."""
    import torch
    select(monkeypatch, "auto")
    monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    ref = holes_ref(oracle_mod)
    g, S, T = ref["g"], ref["S"], ref["T"]
    ns, nt = len(S), len(T)
    S20 = np.concatenate([S, S[:9]])              # more sources than the 16 slices of the warm call
    eng = route.RouteEngine(g)
    side = torch.cuda.Stream()
    sh = side.cuda_stream
    d_s = torch.from_numpy(S20).to(so.dev()); d_t = torch.from_numpy(T).to(so.dev())
    h2, m2 = so.Out(2, nt, i32=True), so.Out(2, 1, i32=True)
    h11, m11 = so.Out(ns, nt, i32=True), so.Out(ns, 1, i32=True)
    lo = [so.Out(1, k, i64=True) for k in (len(g.src), g.n, 1)]
    # warm: 2 sources through hops and loads under a scratch budget of one source per chunk (the
    # budget is read in every call): the scratch holds one source, the loads' slices are 16
    monkeypatch.setenv("SHD_ROUTE_HOPS_SCRATCH", "1000")
    eng.hops_async(d_s[:2], d_t, h2.t, m2.t, stream=sh, dispatch=False)
    eng.loads_async(d_s[:2], d_t, None, lo[0].t, lo[1].t, lo[2].t, stream=sh, dispatch=False)
    so.sync_code(route, eng, sh)
    monkeypatch.delenv("SHD_ROUTE_HOPS_SCRATCH")
    for o in [h2, m2, h11, m11] + lo:
        o.reset()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(so.GATE_FLOOR_MS * so.cycles_per_ms()))      # (work queued ahead of the growth)
    eng.hops_async(d_s[:2], d_t, h2.t, m2.t, stream=sh, dispatch=False)
    eng.hops_async(d_s[:ns], d_t, h11.t, m11.t, stream=sh, dispatch=False)
    eng.loads_async(d_s, d_t, None, lo[0].t, lo[1].t, lo[2].t, stream=sh, dispatch=False)
    with torch.cuda.stream(side):
        for o in [h2, m2, h11, m11] + lo:
            o.snap.copy_(o.big, non_blocking=True)
    assert so.sync_code(route, eng, sh) == route.ENOEDGE and so.sync_code(route, eng, sh) == route.OK
    assert np.array_equal(h2.snap_bits(nt), ref["hops"][:2]) and np.array_equal(h11.snap_bits(nt), ref["hops"])
    assert np.array_equal(m2.snap_bits(1)[:, 0], ref["hops"][:2].max(axis=1))
    assert np.array_equal(m11.snap_bits(1)[:, 0], ref["hops"].max(axis=1))
    el, tr, un, codes, _ = tl.ref_loads(route, HOLES, S20, T, None, False)
    for o, want in zip(lo, (el, tr, np.array([un], np.uint64))):
        assert np.array_equal(o.snap_bits(o.ld)[0].view(np.uint64), want)


# ---- a captured step --------------------------------------------------------------------------

def source_lists(ref):
    """Three source lists of the same length from the reference's sources: as they are, reversed
    and rotated; every one has a source without a self-loop among the targets."""
    S = ref["S"]
    idx = [np.arange(len(S)), np.arange(len(S))[::-1].copy(), np.roll(np.arange(len(S)), 4)]
    return [(S[i], i) for i in idx]


@pytest.mark.parametrize("sel", list(SELECTIONS))
def test_captured_step(route, oracle_mod, monkeypatch, sel):
    """rows_async + min_reduce_async captured into one graph on its own capture stream (a linear
    chain, no parallel branches), replayed three times; between the replays another source list
    is copied into the same d_src: each replay's rows and minimum are that list's (nothing of
    the inputs is fixed at enqueue time)."""
    import torch
    ref = reference(oracle_mod, "narrow", "all")
    select(monkeypatch, sel)
    eng = route.RouteEngine(ref["g"])
    T = ref["T"]
    ns, nt = len(ref["S"]), len(T)
    d_s = torch.from_numpy(ref["S"]).to(so.dev()); d_t = torch.from_numpy(T).to(so.dev())
    la, re, mn, gm = so.Out(ns, nt + 1), so.Out(ns, nt + 1), so.Out(ns, 1), so.Out(1, 1)
    cs = torch.cuda.Stream()
    def step(sh):
        eng.rows_async(d_s, d_t, la.t, re.t, mn.t, stream=sh, dispatch=False, ld=nt + 1)
        eng.min_reduce_async(mn.t, gm.t, stream=sh)
    step(cs.cuda_stream)                                              # the warm call
    assert so.sync_code(route, eng, cs.cuda_stream) == route.ENOEDGE
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cs):
        step(cs.cuda_stream)
    for S, idx in source_lists(ref):
        for o in (la, re, mn, gm):
            o.reset()
        d_s.copy_(torch.from_numpy(S))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for o in (la, re, mn, gm):
            o.snap.copy_(o.big)
        assert so.sync_code(route, eng) == route.ENOEDGE and so.sync_code(route, eng) == route.OK
        assert eq(la.f64(nt), ref["lat"][idx]) and eq(re.f64(nt), ref["rel"][idx])
        assert np.array_equal(mn.f64(1)[:, 0], row_min_of(ref["lat"][idx]))
        assert gm.f64(1)[0, 0] == row_min_of(ref["lat"]).min()
    del graph


@pytest.mark.parametrize("reuse", [True, False])
def test_captured_planned_step(route, oracle_mod, monkeypatch, reuse):
    """The same for a device-built landmark-only plan's rows, with SHD_ROUTE_PLAN_REUSE and
    without (the landmark rows and job records inside the captured step): what changes between
    the replays is the target list."""
    import torch
    eng, plan, n = smallest_plan(route, monkeypatch, "landmark")
    ref = plan_ref(oracle_mod, n, plan)
    T = ref["T"]
    nr, nt = len(ref["S"]), len(T)
    d_t = torch.from_numpy(T).to(so.dev())
    la, re, mn, gm = so.Out(nr, nt + 1), so.Out(nr, nt + 1), so.Out(nr, 1), so.Out(1, 1)
    cs = torch.cuda.Stream()
    def step(sh):
        plan.rows_async(d_t, la.t, re.t, mn.t, stream=sh, dispatch=False, ld=nt + 1, reuse=reuse)
        eng.min_reduce_async(mn.t, gm.t, stream=sh)
    step(cs.cuda_stream)
    assert so.sync_code(route, eng, cs.cuda_stream) == route.ENOEDGE
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cs):
        step(cs.cuda_stream)
    for Tk in (T, T[::-1].copy(), np.roll(T, 11)):
        for o in (la, re, mn, gm):
            o.reset()
        d_t.copy_(torch.from_numpy(Tk))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for o in (la, re, mn, gm):
            o.snap.copy_(o.big)
        assert so.sync_code(route, eng) == route.ENOEDGE and so.sync_code(route, eng) == route.OK
        assert eq(la.f64(nt), ref["lat"][:, Tk]) and eq(re.f64(nt), ref["rel"][:, Tk])
        assert np.array_equal(mn.f64(1)[:, 0], row_min_of(ref["lat"]))
        assert gm.f64(1)[0, 0] == row_min_of(ref["lat"]).min()
    del graph
    plan.close()
