"""GPU: more sources than workgroups, for every launch that caps its grid.

Most launches cap their grid and loop `for (i = blockIdx.x; i < ns; i += gridDim.x)`.  A
workgroup's second trip round that loop is where LDS or HBM-slice state left by its first
source shows.  KD and KB have SHD_ROUTE_KDGRID / KBGRID and KF test_kf_many_sources_per_workgroup;
for the launches below the other suites never pass more sources than the cap, so there every
workgroup runs one source.  Sources may repeat in every entry point, so each cap is crossed on
a graph of a few hundred vertices:

  launch (engine.hip; the path calls: path_calls.hpp)   cap             sources here
  fw_rows_kernel                                        2048            2048 + 7
  fw_parent_kernel (SHD_ROUTE_FWP8=0)                   8192            8192 + 7
  fw_parent8_kernel                                     2048 x 8        16384 + 9 (ragged last group)
  hops_depth / loads_tree / ties_dag kernels, LDS       1024 per chunk  1024 + 7
  the same three, HBM slices                            512 slots       1024 + 7
  hops_parent_kernel, the ties in-degree kernel grid.y  65535           65535 + 5
  direct_rows_kernel (dispatch, shd_route_direct)       65535           65535 + 7
  tri_payload_kernel                                    8192 rows       8192 + 7
  generic f64 kernel, HBM state form                    1024 slots      1024 + 7
  KFH                                                   kf.slots        kf.slots + 7

Method: a base list of distinct sources repeated and permuted to cap + r entries; the oracle
(TIE_MINKEY), tests/ties_ref.py or the loads reference below for the distinct sources only,
gathered by index; np.array_equal on every output, row reductions included.  The graphs have
no vertex loss and the listed entries do not fail, so every form is bit-exact.  The calls go
through the device-pointer entry points (the host wrappers would chunk by output size, not
below these caps, but stage through buffers of their own), each test asserts that its cap was
crossed, and where the cap is the context's it is read from tests/select_main.cpp's record.

Out of scope: the caps at 2^20 (K32, the generic kernel's LDS form, path_attr_kernel) and at
4096 x 256 vertices: no topology this engine is built for lists a million sources."""
import functools
import json
import os

import numpy as np
import pytest

from shadow_amd.graph import complete_graph, internet_like
from tests import shape_graphs
from tests import ties_ref as tr
from tests.test_contexts import selection  # noqa: F401  (select_main's record, built once)
from tests.test_contract_gpu import close_engines, route  # noqa: F401
from tests.test_kd_gpu import _graph as kd_graph

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the caps, as engine.hip and path_host.hpp (state_form) state them
FW_ROWS_CAP = 2048
FW_PARENT_CAP = 8192
FW_PARENT8_CAP = 2048 * 8
TREE_LDS_CAP = 1024          # hops_depth / loads_tree / ties_dag, LDS forms
TREE_HBM_SLOTS = 512         # the same, HBM slices: 16 to 512 slots
GRID_Y_CAP = 65535
DIRECT_CAP = 65535
PAYLOAD_CAP = 8192
F64_SLOTS = 1024


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]:
        monkeypatch.delenv(k)


def repeated(base, total, seed):
    """`total` entries of `base` (distinct), as whole permutations one after another; returns
    the list and the index of every entry in base.  Every base entry occurs, and a workgroup's
    second source (entry i + cap) differs from its first (entry i) for most i."""
    base = np.asarray(base, np.int32)
    assert len(np.unique(base)) == len(base) > 1
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.permutation(len(base)) for _ in range(-(-total // len(base)))])[:total]
    return base[idx], idx


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def sync_code(route, eng):
    try:
        eng.sync()
        return route.OK
    except route.RouteError as err:
        return err.code


def rows_async(route, eng, S, T, dispatch=False, launch=None):
    """(lat, rel, row_min) of one rows launch over device buffers, the sync's code checked."""
    import torch
    d = torch.device("cuda", 0)
    lat = torch.full((len(S), len(T)), -7.0, dtype=torch.float64, device=d)
    rel = torch.full_like(lat, -7.0)
    mn = torch.full((len(S),), -7.0, dtype=torch.float64, device=d)
    (launch or eng.rows_async)(dev(S), dev(T), lat, rel, mn, **({} if launch else {"dispatch": dispatch}))
    assert sync_code(route, eng) == route.OK
    return lat.cpu().numpy(), rel.cpu().numpy(), mn.cpu().numpy()


def check_rows(got, ref, idx):
    lat, rel, mn = got
    olat, orel = ref
    assert lat.shape == (len(idx), olat.shape[1])
    assert np.array_equal(lat, olat[idx])
    assert np.array_equal(rel, orel[idx])
    assert np.array_equal(mn, olat.min(axis=1)[idx])


# ---- K4 rows ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def k4_graph(name):
    return {"k130_odd": lambda: complete_graph(130, seed=6), "ba300": lambda: internet_like(300, 3, seed=17)}[name]()


def k4_targets(g):
    """16 unsorted targets, one of them twice."""
    t = np.random.default_rng(g.n).permutation(g.n)[:15]
    return np.concatenate([t[:9], t[3:4], t[9:]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def k4_ref(name):
    from oracle.oracle import OracleGraph, TIE_MINKEY
    g = k4_graph(name)
    lat, rel, _, _ = OracleGraph(g).source_rows(np.arange(g.n, dtype=np.int32), k4_targets(g), TIE_MINKEY)
    for a in (lat, rel):
        a.setflags(write=False)
    return lat, rel


@pytest.mark.parametrize("fwpk", ["1", "0"])
@pytest.mark.parametrize("kernel,ns", [("rows", FW_ROWS_CAP + 7), ("parent", FW_PARENT_CAP + 7),
                                       ("parent8", FW_PARENT8_CAP + 9)])
@pytest.mark.parametrize("name", ["k130_odd", "ba300"])
def test_k4_rows(route, monkeypatch, name, kernel, ns, fwpk):
    """fw_rows_kernel past 2048 sources (its rel row and bucket starts in LDS are per source),
    fw_parent_kernel past 8192 (SHD_ROUTE_FWP8=0), fw_parent8_kernel past 2048 groups of eight
    with a ragged last group; packed and wide in-list keys."""
    g = k4_graph(name)
    assert g.latency.max() <= 255            # the packed keys are eligible; FWPK=0 turns them off
    monkeypatch.setenv("SHD_ROUTE_FWPK", fwpk)
    if kernel == "parent":
        monkeypatch.setenv("SHD_ROUTE_FWP8", "0")
    np_ = (g.n + 63) // 64 * 64
    assert 16 * np_ <= 160 * 1024            # the 8-source parent search is the default form here
    cap = {"rows": FW_ROWS_CAP, "parent": FW_PARENT_CAP, "parent8": FW_PARENT8_CAP}[kernel]
    assert ns > cap and (ns + 7) // 8 * 8 != ns
    S, idx = repeated(np.arange(g.n), ns, ns)
    T = k4_targets(g)
    eng = route.RouteEngine(g)
    eng.fw_table_async()
    got = rows_async(route, eng, S, T, launch=eng.fw_rows_async)
    check_rows(got, k4_ref(name), idx)


# ---- hops, loads and ties: 1024 workgroups (LDS state) or 512 slots (HBM slices) per chunk ----

BASE = 48   # distinct sources


@functools.lru_cache(maxsize=None)
def tree_graph(name):
    return shape_graphs.tiny(6, "all") if name == "path6" else kd_graph(name)


def tree_base(name):
    g = tree_graph(name)
    return np.arange(g.n, dtype=np.int32) if g.n <= BASE else (np.arange(BASE, dtype=np.int32) * (g.n // BASE) + 3)


@functools.lru_cache(maxsize=None)
def hops_ref(name):
    from oracle.oracle import OracleGraph, TIE_MINKEY
    g = tree_graph(name)
    h = OracleGraph(g).source_rows(tree_base(name), np.arange(g.n, dtype=np.int32), TIE_MINKEY)[3]
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def ties_rows(name):
    g = tree_graph(name)
    cnt, lo, hi, codes = tr.TiesRef(g).rows(tree_base(name), np.arange(g.n, dtype=np.int32), False)
    assert not codes
    return cnt, lo, hi


@functools.lru_cache(maxsize=None)
def trees(name):
    """Per base source: (parent edge, parent vertex, vertices in decreasing distance) of the
    oracle's min-key tree, as tests/test_loads_gpu.py takes them."""
    from oracle.oracle import OracleGraph, TIE_MINKEY
    g = tree_graph(name)
    og = OracleGraph(g)
    out = []
    V = np.arange(g.n)
    for s in tree_base(name).tolist():
        dist, par = og.dijkstra(int(s), TIE_MINKEY)
        assert (par >= 0).sum() == g.n - 1           # connected: nothing unrouted
        e = np.maximum(par, 0)
        pv = np.where(g.directed | (g.dst[e] == V), g.src[e], g.dst[e])
        reach = np.flatnonzero(par >= 0)
        out.append((par, pv, reach[np.argsort(-dist[reach], kind="stable")]))
    return out


def loads_ref(name, idx, W):
    """(edge_load, transit) of the rows idx (indices into the base sources) over all vertices as
    targets with the weight rows W: the reference of tests/test_loads_gpu.py (weights onto their
    targets, vertices in decreasing distance, each sum onto its parent edge and parent), all
    rows of one base source at a time.  Every vertex of these graphs has a self-loop, which
    takes the self entry's weight."""
    g = tree_graph(name)
    base = tree_base(name)
    el = np.zeros(len(g.src), np.uint64)
    trn = np.zeros(g.n, np.uint64)
    loop = {int(a): e for e, (a, b) in enumerate(zip(g.src, g.dst)) if a == b}
    for b, (par, pv, order) in enumerate(trees(name)):
        s = int(base[b])
        acc = W[idx == b].astype(np.uint64).copy()      # (rows of this source, n)
        if not len(acc):
            continue
        el[loop[s]] += acc[:, s].sum(dtype=np.uint64)
        acc[:, s] = 0
        own = acc.copy()
        for v in order.tolist():
            a = acc[:, v]
            el[par[v]] += a.sum(dtype=np.uint64)
            if pv[v] != s:
                acc[:, pv[v]] += a
        trn += (acc - own).sum(axis=0, dtype=np.uint64)
    return el, trn


def slots_of(stride):
    """path_host.hpp state_form: the HBM slices take a quarter of the 1 GiB scratch budget, 16 to 512 slots."""
    return max(16, min(TREE_HBM_SLOTS, ((1 << 30) // 4) // stride))


def a16(x):
    return (x + 15) & ~15


def crossed(name, what, lds, ns):
    """The launch's grid is below ns: 1024 workgroups in the LDS form, the slot rule in the
    HBM form (state sizes: path_hops.hpp hp_state_bytes, tests/ties_ref.py layout_total,
    link_loads.hpp's 22 bytes per vertex bounded from above)."""
    n = tree_graph(name).n
    assert ns <= (1 << 30) // (16 * n)                # one chunk (hops 12, loads 16 bytes per vertex)
    if lds:
        assert ns > TREE_LDS_CAP
        return
    stride = {"hops": a16(4 * a16(2 * n)), "ties": a16(tr.layout_total(n, 2)), "loads": a16(32 * n)}[what]
    assert slots_of(stride) == TREE_HBM_SLOTS and ns > 2 * TREE_HBM_SLOTS     # a third source for some


NS_TREE = TREE_LDS_CAP + 7


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_hops(route, monkeypatch, name, lds):
    import torch
    g = tree_graph(name)
    if not lds:
        monkeypatch.setenv("SHD_ROUTE_HOPS_LDS", "0")
    crossed(name, "hops", lds, NS_TREE)
    S, idx = repeated(tree_base(name), NS_TREE, 11)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    h = torch.full((len(S), g.n), -9, dtype=torch.int32, device=d)
    mx = torch.full((len(S),), -9, dtype=torch.int32, device=d)
    eng.hops_async(dev(S), dev(T), h, mx, dispatch=False)
    assert sync_code(route, eng) == route.OK
    want = hops_ref(name)[idx]
    assert np.array_equal(h.cpu().numpy(), want)
    assert np.array_equal(mx.cpu().numpy(), want.max(axis=1))


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_ties(route, monkeypatch, name, lds):
    import torch
    g = tree_graph(name)
    assert tr.fits_lds(g.n)
    if not lds:
        monkeypatch.setenv("SHD_ROUTE_TIES_LDS", "0")
    crossed(name, "ties", lds, NS_TREE)
    S, idx = repeated(tree_base(name), NS_TREE, 12)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    cnt = torch.full((len(S), g.n), -9, dtype=torch.int64, device=d)
    lo = torch.full((len(S), g.n), -9.0, dtype=torch.float64, device=d)
    hi = torch.full_like(lo, -9.0)
    eng.ties_async(dev(S), dev(T), cnt, lo, hi, dispatch=False)
    assert sync_code(route, eng) == route.OK
    wc, wl, wh = ties_rows(name)
    assert np.array_equal(cnt.cpu().numpy().view(np.uint64), wc[idx])
    assert np.array_equal(lo.cpu().numpy(), wl[idx])
    assert np.array_equal(hi.cpu().numpy(), wh[idx])
    if name == "ties":
        assert (wc > 1).any() and (wl < wh).any()     # tied pairs with a spread among them


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_loads(route, monkeypatch, name, lds):
    """A weight matrix, then a second call with other weights and SHD_ROUTE_LOADS_ADD: the u64
    sums are exact, so both are array_equal."""
    import torch
    g = tree_graph(name)
    if not lds:
        monkeypatch.setenv("SHD_ROUTE_LOADS_LDS", "0")
    crossed(name, "loads", lds, NS_TREE)
    S, idx = repeated(tree_base(name), NS_TREE, 13)
    T = np.arange(g.n, dtype=np.int32)
    rng = np.random.default_rng(14)
    W1 = (rng.integers(0, 5, size=(len(S), g.n)) * (rng.random((len(S), g.n)) < 0.3)).astype(np.uint64)
    W1[np.arange(len(S)), rng.integers(0, g.n, size=len(S))] = np.uint64(2 ** 40 + 3)
    W1[len(S) // 2] = 0
    W2 = rng.integers(0, 1000, size=(len(S), g.n)).astype(np.uint64)
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    de = torch.full((len(g.src),), 9, dtype=torch.int64, device=d)
    dt = torch.full((g.n,), 9, dtype=torch.int64, device=d)
    du = torch.full((1,), 9, dtype=torch.int64, device=d)
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    eng.loads_async(dev(S), dev(T), dev(W1), de, dt, du, dispatch=False)
    assert sync_code(route, eng) == route.OK
    e1, t1 = loads_ref(name, idx, W1)
    assert np.array_equal(u64(de), e1) and np.array_equal(u64(dt), t1) and int(u64(du)[0]) == 0
    assert t1.any() and int(e1.sum(dtype=np.uint64)) >= int(W1.sum(dtype=np.uint64))
    eng.loads_async(dev(S), dev(T), dev(W2), de, dt, du, dispatch=False, add=True)
    assert sync_code(route, eng) == route.OK
    e2, t2 = loads_ref(name, idx, W2)
    assert np.array_equal(u64(de), e1 + e2) and np.array_equal(u64(dt), t1 + t2) and int(u64(du)[0]) == 0


def test_hops_and_ties_past_grid_y(route):
    """65535 + 5 sources of a six-vertex path in one chunk: hops_parent_kernel and the ties
    in-degree kernel take the source from blockIdx.y, capped at 65535."""
    import torch
    name = "path6"
    g = tree_graph(name)
    ns = GRID_Y_CAP + 5
    assert ns <= (1 << 30) // (12 * g.n)              # one chunk
    S, idx = repeated(tree_base(name), ns, 15)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    h = torch.full((ns, g.n), -9, dtype=torch.int32, device=d)
    mx = torch.full((ns,), -9, dtype=torch.int32, device=d)
    eng.hops_async(dev(S), dev(T), h, mx, dispatch=False)
    assert sync_code(route, eng) == route.OK
    want = hops_ref(name)[idx]
    assert np.array_equal(h.cpu().numpy(), want) and np.array_equal(mx.cpu().numpy(), want.max(axis=1))
    cnt = torch.full((ns, g.n), -9, dtype=torch.int64, device=d)
    lo = torch.full((ns, g.n), -9.0, dtype=torch.float64, device=d)
    hi = torch.full_like(lo, -9.0)
    eng.ties_async(dev(S), dev(T), cnt, lo, hi, dispatch=False)
    assert sync_code(route, eng) == route.OK
    wc, wl, wh = ties_rows(name)
    assert np.array_equal(cnt.cpu().numpy().view(np.uint64), wc[idx])
    assert np.array_equal(lo.cpu().numpy(), wl[idx]) and np.array_equal(hi.cpu().numpy(), wh[idx])


# ---- direct rows ------------------------------------------------------------------------------

def test_direct_rows(route, oracle_mod):
    """direct_rows_kernel past 65535 sources: rows with dispatch on a complete graph
    (shd_route_rows_async) and the host shd_route_direct, whose one chunk holds them all."""
    g = complete_graph(67, seed=3)
    ns = DIRECT_CAP + 7
    V = np.arange(g.n, dtype=np.int32)
    S, idx = repeated(V, ns, 16)
    T = np.array([66, 3, 40, 3, 0, 17, 65, 21], np.int32)
    assert ns <= (1 << 30) // (8 * len(T))            # shd_route_direct: one chunk
    tab = oracle_mod.OracleGraph(g).eager_table(V)
    assert tab["is_direct"].all()
    ref = (tab["lat"][:, T], tab["rel"][:, T])
    eng = route.RouteEngine(g)
    assert eng.info["is_complete"] == 1
    check_rows(rows_async(route, eng, S, T, dispatch=True), ref, idx)
    check_rows(eng.direct(S, T), ref, idx)


# ---- payload ----------------------------------------------------------------------------------

@pytest.mark.parametrize("lat16", [True, False])
def test_payload(route, lat16):
    """tri_payload_kernel past 8192 rows: 16 attached vertices, every position many times, the
    caller's prefix offsets starting above zero."""
    import torch
    from shadow_amd.shard import pack_triangle_host, tri_offsets
    g = internet_like(300, 2, seed=5)
    na, nrows = 16, PAYLOAD_CAP + 7
    A = np.sort(np.random.default_rng(5).permutation(g.n)[:na]).astype(np.int32)
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1
    lat0, rel0, _ = eng.rows(A, A, dispatch=False)
    pos, _ = repeated(np.arange(na), nrows, 17)
    lat, rel = lat0[pos], rel0[pos]
    off, tot = tri_offsets(pos, na)
    d = torch.device("cuda", 0)
    out_l = torch.full((tot,), -1, dtype=torch.int16 if lat16 else torch.float64, device=d)
    out_r = torch.full((tot,), -1.0, dtype=torch.float64, device=d)
    eng.tri_payload_async(dev(lat), dev(rel), dev(pos), dev(off[:-1] + 12345), na, out_l, out_r, lat16=lat16)
    assert sync_code(route, eng) == route.OK
    hl, hr = pack_triangle_host(lat, rel, pos, na, lat16=lat16)
    L = out_l.cpu().numpy()
    assert np.array_equal(L.view(np.uint16) if lat16 else L, hl)
    assert np.array_equal(out_r.cpu().numpy(), hr)


# ---- the generic f64 kernel with its state in HBM slices ----------------------------------------

def test_generic_f64_hbm_form(route, oracle_mod, monkeypatch, selection):
    """SHD_ROUTE_KERNEL=f64 on the smallest sized(n) of the suite whose state does not fit the
    LDS: 1024 slots, 1024 + 7 sources.  tests/golden/select_info.json records the forced generic
    kernel up to sized4097 only, all LDS-resident, so n comes from select_main's f64.lds over the
    larger sizes and the created context must report lds_resident == 0."""
    env = {"SHD_ROUTE_KERNEL": "f64"}
    with open(os.path.join(GOLD, "select_info.json")) as f:
        info = json.load(f)
    known_lds = max(int(k.split(":")[0][5:]) for k, v in info.items()
                    if k.startswith("sized") and k.endswith(":KERNEL=f64") and v["lds_resident"] == 1)
    n = next(n for n in shape_graphs.SIZES if n > known_lds and selection(f"sized{n}", env)["f64.lds"] == 0)
    assert selection(f"sized{known_lds}", env)["f64.lds"] == 1
    monkeypatch.setenv("SHD_ROUTE_KERNEL", "f64")
    g = shape_graphs.get(f"sized{n}")
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 0 and eng.info["lds_resident"] == 0
    ns = F64_SLOTS + 7
    # (the vertices v % 3 == 1 have no self-loop: targets and sources are kept apart, so no
    # entry fails)
    T = (np.random.default_rng(n).permutation(n // 2)[:16] * 2 + 1).astype(np.int32)
    base = np.arange(24, dtype=np.int32) * 2 * (n // 48)
    assert not np.intersect1d(base, T).size
    S, idx = repeated(base, ns, 18)
    olat, orel, _, _ = oracle_mod.OracleGraph(g).source_rows(base, T, oracle_mod.TIE_MINKEY)
    check_rows(rows_async(route, eng, S, T), (olat, orel), idx)


# ---- KFH ------------------------------------------------------------------------------------

@pytest.mark.parametrize("ring", [None, "64"])
def test_kfh(route, oracle_mod, monkeypatch, selection, ring):
    """KFH (vertex state in HBM slices, one per workgroup slot) with kf.slots + 7 sources, with
    the default ring and a ring of 64 records."""
    from tests import select_cases as sc
    env = {"SHD_ROUTE_KFH": "1"}
    f = selection("frac1024", env)
    assert f["sel"] == 5 and f["kf.h"] == 1 and f["kf.slots"] >= 16
    monkeypatch.setenv("SHD_ROUTE_KFH", "1")
    if ring:
        monkeypatch.setenv("SHD_ROUTE_KFH_RING", ring)
    g = sc.graph("frac1024")
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 5 and eng.info["lds_resident"] == 0
    ns = f["kf.slots"] + 7
    T = (np.random.default_rng(7).permutation(g.n // 2)[:64] * 2 + 1).astype(np.int32)
    base = np.arange(40, dtype=np.int32) * 2 * (g.n // 80)
    assert not np.intersect1d(base, T).size
    S, idx = repeated(base, ns, 19)
    olat, orel, _, _ = oracle_mod.OracleGraph(g).source_rows(base, T, oracle_mod.TIE_MINKEY)
    check_rows(rows_async(route, eng, S, T), (olat, orel), idx)
