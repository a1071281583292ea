"""GPU: every rows kernel on the wide-range graphs of tests/range_graphs.py (latencies up to
65534 ms, u16 distances past the sign bit and up to 0xFFFE, tentative sums past 0xFFFF, more
distinct reliabilities than the u8 / u16 tables index, decimal latencies up to k = 65535,
self-loops on a share of the vertices only) against the CPU oracle.

Latency is bit-exact everywhere, and checked a second time against the oracle's plain
Floyd-Warshall of the weight matrix.  Reliability is bit-exact against the oracle's engine tie
rule (TIE_MINKEY) without vertex loss; with vertex loss it is bit-exact where a walk kernel ran
(KB fused rows; KD with at most 254 distinct reliabilities and SHD_ROUTE_KDWALK unset: its
phase-C walks) and within REL_TOL where a level sweep multiplies f_t last (the rule of
test_gpu_parity.py).  The oracle fails a whole row when the source has no self-loop and is
among the targets, so it is asked for the row without that target and the engine must answer
NaN there (and SHD_ROUTE_ENOEDGE at the end).

Kernel selections: the auto choice, each SHD_ROUTE_KERNEL, and the knobs together with the
kernel they belong to (SHD_ROUTE_KFH=1 with kf, SHD_ROUTE_KDWALK=0 with kd, SHD_ROUTE_KBFUSE=0
with kb: alone they change nothing where auto picks another kernel).  A forced kernel that is
not eligible falls back to the generic f64 kernel; expect_kernel states, per graph class, which kernel
`info` must report, so that each of the kernel ids 0, 1, 2, 4, 5 and KFH provably ran on these
graphs.
"""
import dataclasses

import numpy as np
import pytest

from tests import range_graphs as rg

pytestmark = pytest.mark.gpu

REL_TOL = 1e-12
LDS_BUDGET = 160 * 1024

SELECTIONS = {
    "auto": {},
    "kd": {"SHD_ROUTE_KERNEL": "kd"},
    "kb": {"SHD_ROUTE_KERNEL": "kb"},
    "k32": {"SHD_ROUTE_KERNEL": "k32"},
    "f64": {"SHD_ROUTE_KERNEL": "f64"},
    "kf": {"SHD_ROUTE_KERNEL": "kf"},
    "kfh": {"SHD_ROUTE_KERNEL": "kf", "SHD_ROUTE_KFH": "1"},
    "kdwalk0": {"SHD_ROUTE_KERNEL": "kd", "SHD_ROUTE_KDWALK": "0"},
    "kbfuse0": {"SHD_ROUTE_KERNEL": "kb", "SHD_ROUTE_KBFUSE": "0"},
}
_KNOBS = ("SHD_ROUTE_KERNEL", "SHD_ROUTE_KFH", "SHD_ROUTE_KDWALK", "SHD_ROUTE_KBFUSE", "SHD_ROUTE_KFPK",
          "SHD_ROUTE_KDPACK", "SHD_ROUTE_SEED", "SHD_TOPOLOGY_LAT16")

# graph classes by what the engine documents about them
U16 = ("wide_hi", "wide_mid", "wide_vloss", "wide_fewrel", "wide_dir", "dumbbell65534", "path65534",
       "manyrel255", "manyrel257", "front32767", "front32768")   # integer, bound < 65535, LDS-sized
FEWREL = ("wide_fewrel", "dumbbell65534", "path65534", "front32767", "front32768")  # <= 254: KF takes them
KF_ONLY = ("dumbbell65536", "dec1", "dec10", "dec100", "dec1000", "dec100_over")    # no u16 kernel
GRAPHS = U16 + ("manyrel70k",) + KF_ONLY


def expect_kernel(name, sel):
    """info["kernel"] as include/shd_route.h and the eligibility rules of shd_route_create
    document it (0 f64, 1 K32, 2 KB, 4 KD, 5 KF/KFH)."""
    if sel == "f64":
        return 0
    if sel in ("kf", "kfh"):
        return 5 if name in FEWREL + KF_ONLY else 0           # KF gives up above 254 reliabilities
    if name in U16:
        return {"auto": 2, "kb": 2, "kbfuse0": 2, "kd": 4, "kdwalk0": 4, "k32": 1}[sel]
    if name == "manyrel70k":                                   # 70000 reliabilities: no KD; 140000
        return 1 if sel in ("auto", "k32") else 0              # arcs: no KB (they do not fit LDS)
    return 5 if sel == "auto" else 0                           # KF_ONLY: a forced integer kernel -> f64


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


def select(monkeypatch, sel):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SELECTIONS[sel].items():
        monkeypatch.setenv(k, v)


def has_loop(g):
    m = np.zeros(g.n, bool)
    m[g.src[g.src == g.dst]] = True
    return m


def sources(g):
    """Every vertex of a graph up to 400 vertices; else 16: vertex 0, the highest one, and
    vertices with and without a self-loop."""
    if g.n <= 400:
        return np.arange(g.n, dtype=np.int32)
    hl = has_loop(g)
    a, b = np.flatnonzero(hl), np.flatnonzero(~hl)
    pick = [0, g.n - 1] + [int(a[k * len(a) // 7]) for k in range(7)] + [int(b[k * len(b) // 7]) for k in range(7)]
    return np.array(list(dict.fromkeys(pick)), np.int32)


def oracle_rows(oracle_mod, og, g, S, T):
    """(lat, rel, hops) of the sources S over the targets T under TIE_MINKEY, NaN / -1 where
    t == s and s has no self-loop (asked without that target)."""
    hl = has_loop(g)
    T = np.asarray(T, np.int32)
    lat = np.full((len(S), len(T)), np.nan); rel = np.full((len(S), len(T)), np.nan)
    hops = np.full((len(S), len(T)), -1, np.int32)
    for i, s in enumerate(S):
        keep = np.ones(len(T), bool) if hl[s] else T != s
        if keep.any():
            l, r, _, h = og.source_row(int(s), T[keep], oracle_mod.TIE_MINKEY)
            lat[i, keep], rel[i, keep], hops[i, keep] = l, r, h
    return lat, rel, hops


def row_min_of(lat):
    return np.fmin.reduce(lat, axis=1, initial=np.inf)


_REF = {}


def reference(oracle_mod, name):
    """Per graph, computed once: the oracle graph, the sources, their oracle rows over all
    vertices and the Floyd-Warshall latencies of those sources."""
    if name not in _REF:
        g = rg.get(name)
        og = oracle_mod.OracleGraph(g)
        S, T = sources(g), np.arange(g.n, dtype=np.int32)
        lat, rel, _ = oracle_rows(oracle_mod, og, g, S, T)
        d = np.full((g.n, g.n), np.inf)
        np.fill_diagonal(d, 0.0)
        nl = g.src != g.dst
        a, b, w = g.src[nl], g.dst[nl], g.latency[nl]
        np.minimum.at(d, (a, b), w)
        if not g.directed:
            np.minimum.at(d, (b, a), w)
        fw = oracle_mod.floyd_warshall(d)[S]
        _REF[name] = dict(g=g, og=og, S=S, T=T, lat=lat, rel=rel, fw=fw, loops=has_loop(g),
                          nrel=len(np.unique(1.0 - g.packetloss[nl])))
    return _REF[name]


def host_rows(route, eng, S, T, dispatch=False):
    """RouteEngine.rows, with the arrays of a call that ended in a per-entry failure."""
    try:
        return eng.rows(S, T, dispatch=dispatch) + (route.OK,)
    except route.RouteError as e:
        assert e.code == route.ENOEDGE, e
        return e.partial + (e.code,)


def dev_rows(route, eng, S, T, launch=None):
    """One shd_route_rows_async (or `launch`) over fresh device tensors -> host arrays + code."""
    import torch
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(np.ascontiguousarray(S, np.int32)).to(dev)
    d_t = torch.from_numpy(np.ascontiguousarray(T, np.int32)).to(dev)
    lat = torch.empty((len(S), len(T)), dtype=torch.float64, device=dev)
    rel = torch.empty_like(lat)
    mn = torch.empty(len(S), dtype=torch.float64, device=dev)
    if launch is None:
        eng.rows_async(d_s, d_t, lat, rel, mn, dispatch=False)
    else:
        launch(d_s, d_t, lat, rel, mn)
    code = route.OK
    try:
        eng.sync()
    except route.RouteError as e:
        code = e.code
    return lat.cpu().numpy(), rel.cpu().numpy(), mn.cpu().numpy(), code


def walk_kernel(info, sel, nrel):
    """Did a kernel that folds reliability from (1.0 * f_s) * f_t down the path run?"""
    if info["kernel"] == 2:
        return info["reserved"] == 1                       # KB with fused path attributes
    if info["kernel"] == 4:
        return nrel <= 254 and sel != "kdwalk0"            # KD's phase-C walks (rtab slot 254 = 1.0)
    return False


def check_table(ref, lat, rel, mn, code, route, exact_rel=True):
    g, S = ref["g"], ref["S"]
    assert np.array_equal(lat, ref["lat"], equal_nan=True)
    if exact_rel:
        assert np.array_equal(rel, ref["rel"], equal_nan=True)
    else:
        assert np.array_equal(np.isnan(rel), np.isnan(ref["rel"]))
        np.testing.assert_allclose(rel, ref["rel"], rtol=REL_TOL, atol=0)
    assert np.array_equal(mn, row_min_of(ref["lat"]))
    assert code == (route.ENOEDGE if (~ref["loops"][S]).any() else route.OK)
    # the second, independent latency reference: plain Floyd-Warshall of the weight matrix
    off = np.asarray(ref["T"])[None, :] != np.asarray(S)[:, None]
    if np.all(g.latency == np.floor(g.latency)):
        assert np.array_equal(lat[off], ref["fw"][off])
    else:  # fractional sums are no left folds in FW: n roundings of 2^-53 on either side
        np.testing.assert_allclose(lat[off], ref["fw"][off], rtol=REL_TOL, atol=0)


INFO_KEYS = ("kernel", "dist_bound", "lat16", "reserved", "lds_resident", "block")


@pytest.mark.parametrize("sel", list(SELECTIONS))
@pytest.mark.parametrize("name", GRAPHS)
def test_rows(route, oracle_mod, monkeypatch, name, sel):
    """The sources' rows over all vertices (the whole table up to 400 vertices) under one
    kernel selection: the host call, then three launches on the same context."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    select(monkeypatch, sel)
    eng = route.RouteEngine(g)
    info = eng.info
    print(name, sel, {k: info[k] for k in INFO_KEYS})
    assert info["kernel"] == expect_kernel(name, sel)
    u16 = name in U16 + ("manyrel70k",)
    if sel in ("f64", "kf", "kfh"):
        assert info["dist_bound"] == 0 and info["lat16"] == 0   # (the integer stage is skipped)
    else:
        assert (0 < info["dist_bound"] < 65535) == u16 and info["lat16"] == int(u16)
        if not u16:
            assert info["dist_bound"] == 0
    if sel == "kfh" and info["kernel"] == 5:
        assert info["lds_resident"] == 0                         # KFH: the vertex state in HBM
    exact = g.vertex_packetloss is None or walk_kernel(info, sel, ref["nrel"])
    lat, rel, mn, code = host_rows(route, eng, S, T)
    check_table(ref, lat, rel, mn, code, route, exact_rel=exact)
    for _ in range(3):
        l2, r2, m2, c2 = dev_rows(route, eng, S, T)
        assert np.array_equal(l2, lat, equal_nan=True) and np.array_equal(r2, rel, equal_nan=True)
        assert np.array_equal(m2, mn) and c2 == code
    eng.close()


def test_selection_at_the_u16_boundary(route, monkeypatch):
    """bound = ecc_out(0) + ecc_in(0) < 65535 is the u16 rule: 65534 takes the u16 kernels
    (and the end-to-end distance 0xFFFE is stored as such), 65536 none of them."""
    select(monkeypatch, "auto")
    for name, s, t in (("dumbbell65534", 2, 4), ("path65534", 194, 388)):
        e = route.RouteEngine(rg.get(name))
        assert e.info["dist_bound"] == 65534 and e.info["kernel"] in (1, 2, 4) and e.info["lat16"] == 1
        assert host_rows(route, e, [s], [t])[0][0, 0] == 65534.0
        e.close()
    e = route.RouteEngine(rg.get("dumbbell65536"))
    assert e.info["dist_bound"] == 0 and e.info["kernel"] not in (1, 2, 4) and e.info["lat16"] == 0
    assert host_rows(route, e, [2], [4])[0][0, 0] == 65536.0
    with pytest.raises(route.RouteError) as ei:
        e.fw_table_async()
    assert ei.value.code == route.EUNSUPPORTED
    e.close()
    for sel in ("kd", "kb", "k32"):
        select(monkeypatch, sel)
        e = route.RouteEngine(rg.get("dumbbell65536"))
        assert e.info["kernel"] == 0 and e.info["dist_bound"] == 0
        e.close()
    # the reliability tables: KD off past 65535 values, KF off past 254
    select(monkeypatch, "kd")
    e = route.RouteEngine(rg.get("manyrel70k"))
    assert e.info["kernel"] != 4
    e.close()
    select(monkeypatch, "kf")
    for name in ("manyrel70k", "manyrel255", "manyrel257", "wide_mid"):
        e = route.RouteEngine(rg.get(name))
        assert e.info["kernel"] == 0, name
        e.close()
    select(monkeypatch, "kb")
    for name, fused in (("path65534", 1), ("manyrel255", 0), ("wide_mid", 0)):
        e = route.RouteEngine(rg.get(name))   # fused rows: w < 256 and <= 254 reliabilities
        assert e.info["kernel"] == 2 and e.info["reserved"] == fused, name
        e.close()


def fw_accepts(name, info, n):
    a16 = lambda x: (x + 15) & ~15
    return (name in U16 + ("manyrel70k",)
            and a16(8 * n) + a16(2 * n) + a16(4 * (info["dist_bound"] + 2)) <= LDS_BUDGET)


@pytest.mark.parametrize("name", GRAPHS)
def test_fw_rows(route, oracle_mod, monkeypatch, name):
    """K4 (shd_route_fw_table_async + shd_route_fw_rows_async) where fw_prepare accepts the
    graph: integer latencies, bound < 0xFFFF and the rows' LDS state (10 n + 4 (bound + 2)
    bytes) within the budget; EUNSUPPORTED otherwise, every time."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    select(monkeypatch, "auto")
    eng = route.RouteEngine(g)
    if not fw_accepts(name, eng.info, g.n):
        for _ in range(2):
            with pytest.raises(route.RouteError) as ei:
                eng.fw_table_async()
            assert ei.value.code == route.EUNSUPPORTED
        eng.close()
        return
    def launch(d_s, d_t, lat, rel, mn):
        eng.fw_table_async()
        eng.fw_rows_async(d_s, d_t, lat, rel, mn)
    out = [dev_rows(route, eng, S, T, launch) for _ in range(3)]
    # fw_rows folds reliability source-first down the tree and multiplies f_t last
    check_table(ref, *out[0], route, exact_rel=g.vertex_packetloss is None)
    for o in out[1:]:
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(o[:3], out[0][:3])) and o[3] == out[0][3]
    eng.close()


def test_fw_takes_some_wide_graph(route, monkeypatch):
    select(monkeypatch, "auto")
    took = []
    for n in GRAPHS:
        e = route.RouteEngine(rg.get(n))
        if fw_accepts(n, e.info, rg.get(n).n):
            took.append(n)
        e.close()
    assert "wide_mid" in took and "wide_dir" in took and "manyrel70k" in took, took


@pytest.mark.parametrize("sel", ["auto", "kd"])
@pytest.mark.parametrize("name", GRAPHS)
def test_plan_rows(route, oracle_mod, monkeypatch, name, sel):
    """A plan over all the sources (in an order of its own): seeded where the code says so --
    KD selected, undirected, packed records (w < 256 and <= 256 reliabilities), no
    prefer-direct -- and plain rows otherwise; the same table either way."""
    import torch
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    select(monkeypatch, sel)
    eng = route.RouteEngine(g)
    plan = eng.plan(S[::-1].copy())
    nl = g.src != g.dst
    packed = g.latency[nl].max() < 256 and ref["nrel"] <= 256 and bool(np.all(g.latency[nl] == np.floor(g.latency[nl])))
    want = eng.info["kernel"] == 4 and packed and not g.directed and not g.prefer_direct
    print(name, sel, "kernel", eng.info["kernel"], "seeded", plan.info["seeded"], "rows", plan.info["rows"])
    assert plan.info["seeded"] == int(want) and plan.info["rows"] == len(S)
    order = S[::-1][plan.positions]
    inv = np.empty(g.n, np.int64); inv[order] = np.arange(len(order))
    def launch(d_s, d_t, lat, rel, mn):
        plan.rows_async(d_t, lat, rel, mn, dispatch=False)
    out = [dev_rows(route, eng, order, T, launch) for _ in range(3)]
    lat, rel, mn, code = out[0]
    back = inv[S]
    exact = g.vertex_packetloss is None or walk_kernel(eng.info, sel, ref["nrel"])
    check_table(ref, lat[back], rel[back], mn[back], code, route, exact_rel=exact)
    for o in out[1:]:
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(o[:3], out[0][:3])) and o[3] == code
    plan.close(); eng.close()


def test_seeded_plan_ran_on_a_wide_range_graph(route, monkeypatch):
    """The seeded rows (D0 = w(s, u) + d_u, saturating at 0xFFFF) with distances up to 0xFFFE."""
    select(monkeypatch, "kd")
    eng = route.RouteEngine(rg.get("path65534"))
    plan = eng.plan(np.arange(rg.get("path65534").n, dtype=np.int32))
    assert eng.info["kernel"] == 4 and plan.info["seeded"] == 1
    plan.close(); eng.close()


# ---- self, direct and the dispatch --------------------------------------------------------

def dispatch_ref(oracle_mod, g, S, T):
    """topology.c:2019-2031 on a prefer-direct graph: adjacent pairs (a self-loop makes s
    adjacent to itself) take the direct path, the others the source path."""
    og = oracle_mod.OracleGraph(g)
    lat, rel, _ = oracle_rows(oracle_mod, og, g, S, T)
    for i, s in enumerate(S):
        for j, t in enumerate(T):
            if og.get_eid(int(s), int(t)) >= 0:
                lat[i, j], rel[i, j] = og.direct(int(s), int(t))
    return lat, rel


def test_self_and_direct(route, oracle_mod, monkeypatch):
    select(monkeypatch, "auto")
    ref = reference(oracle_mod, "wide_hi")
    g, og = ref["g"], ref["og"]
    eng = route.RouteEngine(g)
    v = np.arange(g.n, dtype=np.int32)
    lat, rel = eng.self_paths(v)
    for k in range(g.n):
        assert (lat[k], rel[k]) == og.self_path(k)
    S = v[::29]
    try:
        dl, dr, dm = eng.direct(S, v)
        code = route.OK
    except route.RouteError as e:
        (dl, dr, dm), code = e.partial, e.code
    assert code == route.ENOEDGE                 # BA(n, 3) is far from complete
    el = np.full(dl.shape, np.nan); er = np.full(dl.shape, np.nan)
    for i, s in enumerate(S):
        for t in range(g.n):
            if og.get_eid(int(s), t) >= 0:
                el[i, t], er[i, t] = og.direct(int(s), t)
    assert np.array_equal(dl, el, equal_nan=True) and np.array_equal(dr, er, equal_nan=True)
    assert np.array_equal(dm, row_min_of(el))
    eng.close()


@pytest.mark.parametrize("n", [389, 8000])
def test_prefer_direct_dispatch(route, oracle_mod, monkeypatch, n):
    """rows(dispatch=True) on a prefer-direct wide graph: the generic kernel with the dispatch
    bits, per-source state in LDS (n = 389) and in HBM (n = 8000)."""
    select(monkeypatch, "auto")
    g = dataclasses.replace(rg.get("wide_mid") if n == 389 else rg.wide(n, 17, rg.WIDE_MID_SCALE), prefer_direct=True)
    eng = route.RouteEngine(g)
    hl = has_loop(g)
    a, b = np.flatnonzero(hl), np.flatnonzero(~hl)
    S = np.array([0, n - 1, a[1], a[len(a) // 2], b[0], b[len(b) // 2]], np.int32)
    T = np.arange(n, dtype=np.int32)
    lat, rel, mn, code = host_rows(route, eng, S, T, dispatch=True)
    el, er = dispatch_ref(oracle_mod, g, S, T)
    assert np.isnan(el).sum() == int((~hl[S]).sum()) and code == route.ENOEDGE
    assert np.array_equal(lat, el, equal_nan=True) and np.array_equal(rel, er, equal_nan=True)
    assert np.array_equal(mn, row_min_of(el))
    if n == 8000:
        monkeypatch.setenv("SHD_ROUTE_KERNEL", "f64")
        assert route.RouteEngine(g).info["lds_resident"] == 0
    eng.close()


# ---- payload, triangle fill, front end ----------------------------------------------------

@pytest.mark.parametrize("lat16", [True, False])
def test_payload(route, oracle_mod, monkeypatch, lat16):
    """shd_route_tri_payload_async over rows with NaN diagonals and latencies past 32768."""
    import torch
    from shadow_amd.shard import decode_lat16, pack_triangle_host, tri_offsets
    select(monkeypatch, "auto")
    ref = reference(oracle_mod, "wide_hi")
    g = ref["g"]
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1
    na = g.n
    pos = np.arange(na - 1, -1, -3, dtype=np.int32)
    lat, rel = ref["lat"][pos], ref["rel"][pos]
    assert np.isnan(lat[np.arange(len(pos)), pos]).any() and np.nanmax(lat) >= 32768
    off, tot = tri_offsets(pos, na)
    dev = torch.device("cuda", 0)
    out_l = torch.empty(tot, dtype=torch.int16 if lat16 else torch.float64, device=dev)
    out_r = torch.empty(tot, dtype=torch.float64, device=dev)
    eng.tri_payload_async(torch.from_numpy(lat).to(dev), torch.from_numpy(rel).to(dev), torch.from_numpy(pos).to(dev),
                          torch.from_numpy(off[:-1].copy()).to(dev), na, out_l, out_r, lat16=lat16)
    eng.sync()
    L, R = out_l.cpu().numpy(), out_r.cpu().numpy()
    hl, hr = pack_triangle_host(lat, rel, pos, na, lat16=lat16)
    want = np.concatenate([lat[r, p:] for r, p in enumerate(pos)])
    if lat16:
        assert np.array_equal(L.view(np.uint16), hl)
        assert np.array_equal(decode_lat16(L), want, equal_nan=True)
        assert (L.view(np.uint16) == 0xFFFF).sum() == np.isnan(want).sum() > 0
    else:
        assert np.array_equal(L, hl, equal_nan=True) and np.array_equal(L, want, equal_nan=True)
    assert np.array_equal(R, hr, equal_nan=True)
    eng.close()


def read_triangle(route, buf, na, lat16):
    """(lat, rel) upper triangles (na x na, NaN below the diagonal) from either fill layout."""
    lat = np.full((na, na), np.nan); rel = np.full((na, na), np.nan)
    raw = buf.array()
    if not lat16:
        o = 0
        for i in range(na):
            seg = raw[2 * o: 2 * (o + na - i)]
            lat[i, i:], rel[i, i:] = seg[0::2], seg[1::2]
            o += na - i
        return lat, rel
    u16 = raw.view(np.uint16)
    for i in range(na):
        e = np.arange(na - i)
        line = route.tri16_lines(na, i) + e // 6
        rel[i, i:] = raw[line * 8 + e % 6]
        x = u16[line * 32 + 24 + e % 6]
        lat[i, i:] = np.where(x == 0xFFFF, np.nan, x.astype(np.float64))
    return lat, rel


@pytest.mark.parametrize("lat16", [False, True])
def test_fill_triangle(route, oracle_mod, monkeypatch, lat16):
    """shd_route_fill_triangle in both layouts over an attached subset of wide_hi with
    vertices of both kinds (the compact layout holds latencies past the sign bit of a u16)."""
    select(monkeypatch, "auto")
    ref = reference(oracle_mod, "wide_hi")
    g = ref["g"]
    A = np.arange(1, g.n, 3, dtype=np.int32)
    assert 0 < ref["loops"][A].sum() < len(A)
    na = len(A)
    eng = route.RouteEngine(g)
    nbytes = 64 * route.tri16_lines(na) if lat16 else 16 * na * (na + 1) // 2
    buf = route.PinnedBuffer(nbytes)
    buf.array()[:] = -7.0
    mn, _ = eng.fill_triangle(A, buf, dispatch=True, lat16=lat16)
    lat, rel = read_triangle(route, buf, na, lat16)
    iu = np.triu_indices(na)
    el, er = ref["lat"][np.ix_(A, A)], ref["rel"][np.ix_(A, A)]
    assert np.array_equal(lat[iu], el[iu], equal_nan=True) and np.array_equal(rel[iu], er[iu], equal_nan=True)
    assert np.nanmax(el[iu]) >= 32768 and np.isnan(el[iu]).sum() == int((~ref["loops"][A]).sum())
    assert mn == np.nanmin(el[iu])
    buf.close(); eng.close()


def front_ref(oracle_mod, g, A):
    """The front end's table over the sorted attached vertices A: the pair {A[i], A[j]}, i <= j,
    holds the Path row i wrote (first writer wins): direct for adjacent pairs of a prefer-direct
    graph, the path to self (topology.c:1545-1653) where the batch could not store (s, s)."""
    og = oracle_mod.OracleGraph(g)
    lat, rel = dispatch_ref(oracle_mod, g, A, A) if g.prefer_direct else oracle_rows(oracle_mod, og, g, A, A)[:2]
    for i, s in enumerate(A):
        if np.isnan(lat[i, i]):
            lat[i, i], rel[i, i] = og.self_path(int(s))
    il = np.tril_indices(len(A), -1)
    lat[il], rel[il] = lat.T[il], rel.T[il]
    return lat, rel


@pytest.mark.parametrize("which", [0, 1])
def test_front_end_compact_rule(route, oracle_mod, monkeypatch, which):
    """The front end takes the compact triangle when 2 * max edge latency < 0xFFFF: at 32767,
    not at 32768 (the engine's info.lat16 is 1 for both)."""
    from shadow_amd import topology
    topology.load_library()
    select(monkeypatch, "auto")
    g = rg.front_pair()[which]
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1 and eng.info["dist_bound"] == 60000
    eng.close()
    A = np.arange(g.n, dtype=np.int32)
    el, er = front_ref(oracle_mod, g, A)
    for sub in (A, A[[1, 2, 3, 4]]):
        t = topology.Topology.from_graph(g)
        t.attach_all(sub)
        lat, rel = t.table(sub)
        na = len(sub)
        compact = t.triangle_bytes() == 64 * route.tri16_lines(na)
        assert compact == (which == 0) and (compact or t.triangle_bytes() == 16 * na * (na + 1) // 2)
        assert np.array_equal(lat, el[np.ix_(sub, sub)]) and np.array_equal(rel, er[np.ix_(sub, sub)])
        assert t.min_path_latency() == el[np.ix_(sub, sub)].min()
        t.close()
    assert el[2, 4] == 59000.0 and el[1, 3] == (32767.0, 32768.0)[which] and el[2, 2] == 30000.0
    # the self-looped vertices alone: the oracle's own eager table is defined there
    loops = np.flatnonzero(has_loop(g)).astype(np.int32)
    tab = oracle_mod.OracleGraph(g).eager_table(loops, prefer_direct=True, tiebreak=oracle_mod.TIE_MINKEY)
    assert np.array_equal(tab["lat"], el[np.ix_(loops, loops)]) and np.array_equal(tab["rel"], er[np.ix_(loops, loops)])
    assert tab["min_latency"] == el[np.ix_(loops, loops)].min()


# ---- decimal latencies under KFH ----------------------------------------------------------

@pytest.mark.parametrize("name,scale", [("dec1", 1), ("dec10", 10), ("dec100", 100), ("dec1000", 1000),
                                        ("dec100_over", 0)])
def test_decimal_packed_arcs(route, oracle_mod, monkeypatch, name, scale):
    """KFH's packed arcs (head | k << 16) pick the decimal scale with every k <= 65535, and
    keep f64 arcs when one arc needs k = 65536; the same rows as SHD_ROUTE_KFPK=0."""
    ref = reference(oracle_mod, name)
    g, S, T = ref["g"], ref["S"], ref["T"]
    select(monkeypatch, "kfh")
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 5 and eng.info["lds_resident"] == 0 and eng.info["reserved"] == scale
    out = host_rows(route, eng, S, T)
    check_table(ref, *out, route)
    monkeypatch.setenv("SHD_ROUTE_KFPK", "0")
    e0 = route.RouteEngine(g)
    assert e0.info["kernel"] == 5 and e0.info["reserved"] == 0
    o0 = host_rows(route, e0, S, T)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(out[:3], o0[:3])) and out[3] == o0[3]
    eng.close(); e0.close()
