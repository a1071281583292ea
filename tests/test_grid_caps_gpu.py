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
  ecmp_dag / fold_tree / loss_tree kernels, LDS         1024 per chunk  1024 + 7
  the same three, HBM slices                            512 slots       1024 + 7
  the same three under dispatch (complete: no state)    1024 per chunk  1024 + 7
  outage_repair_kernel (grid over work units), LDS      1024 units      1031 sources x 1 slab of 3;
                                                                        7 sources x 147 slabs of 1
  the same, HBM slices                                  512 slots       the same 1031 and 1029 units
  the four pair forms (grouped by distinct source)      1024 per chunk  1056 distinct sources
  hops_parent_kernel, the ties in-degree kernel grid.y  65535           65535 + 5
  direct_rows_kernel (dispatch, shd_route_direct)       65535           65535 + 7
  tri_payload_kernel                                    8192 rows       8192 + 7
  generic f64 kernel, HBM state form                    1024 slots      1024 + 7
  KFH                                                   kf.slots        kf.slots + 7

Method: a base list of distinct sources repeated and permuted to cap + r entries; the oracle
(TIE_MINKEY), tests/ties_ref.py or the loads reference below for the distinct sources only,
gathered by index; np.array_equal on every output, row reductions included.  The graphs have
no vertex loss and the listed entries do not fail, so every form is bit-exact.  The folds and
the outages are held the same way (fold_ref, outage_ref; the outage statistics are u64 sums,
linear in the weights, so the reference runs over the distinct sources with each one's rows
added up).  The ECMP loads and the link loss add floating-point terms across sources in no fixed
order: they are held to ecmp_ref and loss_ref over the whole repeated list within the two bounds
those headers derive -- EcmpRef.tol and (R + 4 + A) * 2^-52, R and A counted by the reference for
the very call -- and exactly where all terms are whole numbers below 2^53.  The calls go
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
from tests import ecmp_ref as er
from tests import fold_ref as fr
from tests import loss_ref as lr
from tests import outage_ref as orf
from tests import shape_graphs
from tests import test_hops_gpu as hg
from tests import test_outage as tout
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
    if name in ("k24", "ba80_prefer"):
        return hg._graph(name)[0]
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
    link_loads.hpp's 22 bytes per vertex bounded from above, and the layout_total of ecmp_ref,
    fold_ref, loss_ref and outage_ref).  ns: the sources; the outage kernel's work units."""
    n = tree_graph(name).n
    assert ns <= (1 << 30) // (16 * n)                # one chunk (hops 12, loads 16 bytes per vertex)
    if lds:
        assert ns > TREE_LDS_CAP
        return
    stride = {"hops": a16(4 * a16(2 * n)), "ties": a16(tr.layout_total(n, 2)), "loads": a16(32 * n),
              "ecmp": a16(er.layout_total(n)), "fold": a16(fr.layout_total(n)), "loss": a16(lr.layout_total(n)),
              "outage": a16(orf.layout_total(n))}[what]
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


# ---- ECMP loads, folds, link loss and link outages: the same caps -------------------------------
# (path_calls.hpp launches ecmp_dag_kernel, fold_tree_kernel, loss_tree_kernel and
# outage_repair_kernel through state_form as the three above: 1024 workgroups in the LDS form, the
# slot rule in the HBM form, min(k, 1024) without state under dispatch on a complete graph.)

FAMILY_KNOB = {"ecmp": "SHD_ROUTE_ECMP_LDS", "fold": "SHD_ROUTE_FOLD_LDS", "loss": "SHD_ROUTE_LOSS_LDS",
               "outage": "SHD_ROUTE_OUTAGE_LDS"}
FAMILY_REF = {"ecmp": er, "fold": fr, "loss": lr, "outage": orf}
FOLD_OPS = [fr.SUM, fr.MIN, fr.MAX, fr.PROD]


def form(monkeypatch, name, what, lds, ns):
    """Choose the state form of family `what` and assert that ns crosses its cap in one chunk."""
    assert FAMILY_REF[what].fits_lds(tree_graph(name).n)     # the LDS form unless the knob says off
    if not lds:
        monkeypatch.setenv(FAMILY_KNOB[what], "0")
    crossed(name, what, lds, ns)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def summed(W, idx, k):
    """The weight rows W added up per base source (idx: the base index of every row), modulo 2^64."""
    out = np.zeros((k, W.shape[1]), np.uint64)
    np.add.at(out, idx, W)
    return out


def load_weights(ns, n, seed):
    """A u64 block with zeros, a zero row and one value above 2^40 in every other row, as test_loads has."""
    rng = np.random.default_rng(seed)
    W = (rng.integers(0, 5, size=(ns, n)) * (rng.random((ns, n)) < 0.3)).astype(np.uint64)
    W[np.arange(ns), rng.integers(0, n, size=ns)] = np.uint64(2 ** 40 + 3)
    W[ns // 2] = 0
    return W


# -- folds

@functools.lru_cache(maxsize=None)
def fold_rows(name, dispatch=False):
    """((4, base, n) folds of fold_ref.columns, (base, n) latencies of the rows) of the base sources."""
    g = tree_graph(name)
    F = fr.FoldRef(g)
    T = np.arange(g.n, dtype=np.int32)
    out, codes = F.rows(tree_base(name), T, FOLD_OPS, fr.columns(g), dispatch)
    lat = F.ref.rows(tree_base(name), T, dispatch)[0]
    assert not codes and not np.isnan(out).any() and not np.isnan(lat).any()
    out.setflags(write=False)
    lat.setflags(write=False)
    return out, lat


def run_folds(route, name, dispatch, seed):
    import torch
    g = tree_graph(name)
    S, idx = repeated(tree_base(name), NS_TREE, seed)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    out = torch.full((4, len(S), g.n), -7.0, dtype=torch.float64, device=d)
    eng.fold_async(dev(S), dev(T), FOLD_OPS, dev(fr.columns(g)), out, dispatch=dispatch)
    assert sync_code(route, eng) == route.OK
    want, lat = fold_rows(name, dispatch)
    assert np.array_equal(out.cpu().numpy(), want[:, idx])
    one = torch.full((1, len(S), g.n), -7.0, dtype=torch.float64, device=d)
    eng.fold_async(dev(S), dev(T), [fr.SUM], dev(np.asarray(g.latency, np.float64)), one, dispatch=dispatch)
    assert sync_code(route, eng) == route.OK
    assert np.array_equal(one.cpu().numpy()[0], lat[idx])     # the sum of the latencies is the rows' lat
    return eng


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_folds(route, monkeypatch, name, lds):
    """Four folds in one call: the carried folds of a workgroup's first source must not reach its second."""
    form(monkeypatch, name, "fold", lds, NS_TREE)
    run_folds(route, name, False, 21)


# -- link outages

@functools.lru_cache(maxsize=None)
def outage_ref_of(name):
    return orf.OutageRef(tree_graph(name))


def tree_edge(name, b, where):
    """The parent edge of a vertex of base source b's tree: where = 0.0 the nearest level .. 1.0 the deepest."""
    _, pe, _, _, order = outage_ref_of(name)._tree(int(tree_base(name)[b]))
    return int(pe[order[int(where * (len(order) - 1))]])


def run_outage(route, name, S, W, scn, want, rows):
    """outage_async over canary-filled outputs; want: the reference's Result, whose latencies are
    (scenarios, base sources x n) when rows (the base index of every source row) is given."""
    import torch
    g = tree_graph(name)
    T = np.arange(g.n, dtype=np.int32)
    off, edge = orf.pack([sorted(f) for f in scn])
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    st = torch.full((len(scn), 3), 7, dtype=torch.int64, device=d)
    mx = torch.full((len(scn),), 7.25, dtype=torch.float64, device=d)
    nl = torch.full((len(scn), len(S), g.n), 7.25, dtype=torch.float64, device=d)
    un = torch.full((1,), 7, dtype=torch.int64, device=d)
    eng.outage_async(dev(S), dev(T), dev(W), dev(off), dev(edge), st, mx, nl, un)
    assert sync_code(route, eng) == route.OK
    assert want.codes == frozenset({0}) and want.unrouted == 0 == int(u64(un)[0])
    assert np.array_equal(u64(st), want.stats), (u64(st).tolist(), want.stats.tolist())
    assert np.array_equal(mx.cpu().numpy(), want.max_add)
    wl = want.lat.reshape(len(scn), -1, g.n)
    assert not np.isnan(wl).any()
    assert np.array_equal(nl.cpu().numpy(), wl if rows is None else wl[:, rows])


@functools.lru_cache(maxsize=None)
def outage_sources_case(name):
    """1031 source rows x 3 scenarios.  lat: OutageRef.repair of the base sources, gathered by the
    test; stats: the u64 sums over all 1031 rows, which are linear in the weights modulo 2^64, so
    the same repair with every base source's rows added up gives them (max_add takes no weights,
    and every base source occurs)."""
    g = tree_graph(name)
    base = tree_base(name)
    S, idx = repeated(base, NS_TREE, 22)
    W = load_weights(len(S), g.n, 23)
    a, b, c = tree_edge(name, 0, 0.0), tree_edge(name, 17, 0.5), tree_edge(name, 40, 1.0)
    scn = [[a], sorted({b, c}), [c]]
    want = outage_ref_of(name).repair(*orf.block_entries(base, np.arange(g.n), summed(W, idx, len(base))), scn)
    assert len(np.unique(idx)) == len(base)
    assert want.stats[:, orf.HIT].all() and want.stats[:, orf.SLOWER].any() and want.max_add.max() > 0
    return S, idx, W, scn, want


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_outage_sources(route, monkeypatch, name, lds):
    """One slab of three scenarios per source: every second trip of a workgroup is a new source,
    whose level order is rebuilt over marks that the first one must have left clean."""
    S, idx, W, scn, want = outage_sources_case(name)
    assert orf.units(len(S), len(scn)) == (3, 1, NS_TREE)
    form(monkeypatch, name, "outage", lds, orf.units(len(S), len(scn))[2])
    run_outage(route, name, S, W, scn, want, idx)


@functools.lru_cache(maxsize=None)
def outage_slabs_case(name):
    """7 sources x 147 single-edge scenarios, the edges spread over the tree of the first source."""
    g = tree_graph(name)
    S = tree_base(name)[:7]
    _, pe, _, _, order = outage_ref_of(name)._tree(int(S[0]))
    edges = sorted({int(pe[v]) for v in order})
    scn = [[e] for e in edges[:: len(edges) // 147][:147]]
    W = load_weights(len(S), g.n, 24)
    want = outage_ref_of(name).repair(*orf.block_entries(S, np.arange(g.n), W), scn)
    assert len(scn) == 147 and np.count_nonzero(want.stats[:, orf.HIT]) > 147 // 2 and want.stats[:, orf.SLOWER].any()
    return S, W, scn, want


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_outage_slabs(route, monkeypatch, name, lds):
    """147 slabs of one scenario per source: a workgroup's second unit is another source's slab
    (units 1024 .. 1028 are the last source's, unit b the first's)."""
    S, W, scn, want = outage_slabs_case(name)
    assert orf.units(len(S), len(scn)) == (1, 147, 1029)
    form(monkeypatch, name, "outage", lds, orf.units(len(S), len(scn))[2])
    run_outage(route, name, S, W, scn, want, None)


# -- ECMP loads

@functools.lru_cache(maxsize=None)
def ecmp_case(name, dispatch=False):
    """(S, idx, W, EcmpRef.rows of the whole list in f64, its derived tolerance)."""
    g = tree_graph(name)
    S, idx = repeated(tree_base(name), NS_TREE, 25)
    W = np.random.default_rng(26).integers(0, 1 << 20, size=(len(S), g.n)).astype(np.uint64)
    W[len(S) // 3] = 0
    E = er.EcmpRef(g)
    want = E.rows(S, np.arange(g.n), W, dispatch)
    assert want[2] == 0 and not want[3]
    return S, idx, W, want, E.tol(S, dispatch=dispatch)


def run_ecmp(route, name, dispatch):
    import torch
    g = tree_graph(name)
    S, idx, W, want, rtol = ecmp_case(name, dispatch)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    d = torch.device("cuda", 0)
    de = torch.full((g.m,), 9.5, dtype=torch.float64, device=d)
    dt = torch.full((g.n,), 9.5, dtype=torch.float64, device=d)
    du = torch.full((1,), 9, dtype=torch.int64, device=d)
    eng.ecmp_loads_async(dev(S), dev(T), dev(W), de, dt, du, dispatch=dispatch)
    assert sync_code(route, eng) == route.OK and int(u64(du)[0]) == 0
    assert er.close(de.cpu().numpy(), want[0], rtol) and er.close(dt.cpu().numpy(), want[1], rtol)
    return eng, S, idx, W


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_ecmp(route, monkeypatch, name, lds):
    """Against EcmpRef over the whole list within its derived tolerance; then with the weight of
    every tied entry set to zero, where the ECMP loads are shd_route_loads' converted to f64,
    whole numbers below 2^53 that add exactly in any order."""
    import torch
    form(monkeypatch, name, "ecmp", lds, NS_TREE)
    eng, S, idx, W = run_ecmp(route, name, False)
    g = tree_graph(name)
    T = np.arange(g.n, dtype=np.int32)
    one = ties_rows(name)[0][idx] == 1
    if name == "ties":
        assert np.count_nonzero(~one) > len(S) and W[~one].any()      # tied entries took part in the first run
    W1 = np.where(one, W, np.uint64(0)).astype(np.uint64)
    d = torch.device("cuda", 0)
    de = torch.full((g.m,), 9.5, dtype=torch.float64, device=d)
    dt = torch.full((g.n,), 9.5, dtype=torch.float64, device=d)
    le = torch.full((g.m,), 9, dtype=torch.int64, device=d)
    lt = torch.full((g.n,), 9, dtype=torch.int64, device=d)
    du = [torch.full((1,), 9, dtype=torch.int64, device=d) for _ in range(2)]
    eng.ecmp_loads_async(dev(S), dev(T), dev(W1), de, dt, du[0], dispatch=False)
    eng.loads_async(dev(S), dev(T), dev(W1), le, lt, du[1], dispatch=False)
    assert sync_code(route, eng) == route.OK and int(u64(du[0])[0]) == int(u64(du[1])[0]) == 0
    assert 0 < int(u64(le).max()) < 2 ** 53 and u64(lt).any()
    assert np.array_equal(de.cpu().numpy(), u64(le).astype(np.float64))
    assert np.array_equal(dt.cpu().numpy(), u64(lt).astype(np.float64))


# -- link loss

@functools.lru_cache(maxsize=None)
def loss_case(name, dispatch=False):
    """(S, idx, W1, W2, r1, r2, x1, x2) of a call with the weights W1 and a second one that adds
    the weights W2 on top.  r1, r2: LossRef.block of the whole list in f64, which counts R and A
    of either call (r2 starts from r1's outputs: one more addend wherever those are not zero).
    x1, x2: the exact fractions of either call's own terms.  In exact arithmetic the outputs are
    linear in the weights as long as no u64 sum wraps, so LossRef.block of the base sources with
    each one's rows added up is LossRef.block of the whole list, at a twentieth of the cost."""
    g = tree_graph(name)
    base = tree_base(name)
    T = np.arange(g.n, dtype=np.int32)
    S, idx = repeated(base, NS_TREE, 27)
    W1 = load_weights(len(S), g.n, 28)
    W2 = np.random.default_rng(29).integers(0, 1000, size=(len(S), g.n)).astype(np.uint64)
    L = lr.LossRef(g)
    r1 = L.block(S, T, W1, dispatch)
    r2 = L.block(S, T, W2, dispatch, init=r1.arrays())
    assert int(W1.sum(dtype=np.uint64)) + int(W2.sum(dtype=np.uint64)) < 2 ** 63            # nothing wraps
    x1 = L.block(base, T, summed(W1, idx, len(base)), dispatch, exact=True)
    x2 = L.block(base, T, summed(W2, idx, len(base)), dispatch, exact=True)
    for r, x in ((r1, x1), (r2, x2)):
        assert (r.R, r.unrouted, r.codes, r.routed) == (x.R, 0, set(), x.routed) and r.A > 2
    return S, idx, W1, W2, r1, r2, x1, x2


def loss_outs(g, d):
    import torch
    return ([torch.full((k,), 7.25, dtype=torch.float64, device=d) for k in (g.m, g.m, g.n, g.n)]
            + [torch.full((1,), 7, dtype=torch.int64, device=d)])


def run_loss(route, name, dispatch):
    import torch
    from fractions import Fraction
    g = tree_graph(name)
    S, idx, W1, W2, r1, r2, x1, x2 = loss_case(name, dispatch)
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g)
    outs = loss_outs(g, torch.device("cuda", 0))
    eng.loss_async(dev(S), dev(T), dev(W1), *outs, dispatch=dispatch)
    assert sync_code(route, eng) == route.OK and int(u64(outs[4])[0]) == 0
    got1 = [o.cpu().numpy() for o in outs[:4]]
    for k in range(4):
        assert lr.close(got1[k], x1.outs()[k], r1.R, r1.A), (lr.NAMES[k], r1.R, r1.A)
    assert got1[0].any() and got1[1].any() and got1[3].any()
    # a second call adds other weights on top of what the first one left
    eng.loss_async(dev(S), dev(T), dev(W2), *outs, dispatch=dispatch, add=True)
    assert sync_code(route, eng) == route.OK and int(u64(outs[4])[0]) == 0
    for k in range(4):
        want = [Fraction(a) + b for a, b in zip(got1[k].tolist(), x2.outs()[k])]
        assert lr.close(outs[k].cpu().numpy(), want, r2.R, r2.A), (lr.NAMES[k], r2.R, r2.A)
    return S, W1


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", ["ba400", "ties"])
def test_loss(route, monkeypatch, name, lds):
    """All four outputs within (R + 4 + A) * 2^-52 of the exact fractions, a second call that
    adds, and on a copy of the graph without any loss edge_reach equal to shd_route_loads' edge
    load converted to f64, exactly, with nothing dropped."""
    import dataclasses
    import torch
    form(monkeypatch, name, "loss", lds, NS_TREE)
    S, W = run_loss(route, name, False)
    g = tree_graph(name)
    g0 = dataclasses.replace(g, packetloss=np.zeros(g.m), vertex_packetloss=None, name=g.name + "_zero")
    T = np.arange(g.n, dtype=np.int32)
    eng = route.RouteEngine(g0)
    d = torch.device("cuda", 0)
    outs = loss_outs(g0, d)
    le = torch.full((g.m,), 9, dtype=torch.int64, device=d)
    eng.loss_async(dev(S), dev(T), dev(W), *outs, dispatch=False)
    eng.loads_async(dev(S), dev(T), dev(W), le, None, None, dispatch=False)
    assert sync_code(route, eng) == route.OK and int(u64(outs[4])[0]) == 0
    assert 2 ** 40 < int(u64(le).max()) < 2 ** 53
    assert np.array_equal(outs[0].cpu().numpy(), u64(le).astype(np.float64))
    assert not outs[1].cpu().numpy().any() and not outs[2].cpu().numpy().any()
    assert float(outs[3].cpu().numpy().sum()) == float(int(W.sum(dtype=np.uint64)))


# -- dispatch: a complete graph (no rows launch, no sweep, no state) and a prefer-direct one

RUN = {"ecmp": lambda route, name: run_ecmp(route, name, True),
       "fold": lambda route, name: run_folds(route, name, True, 30),
       "loss": lambda route, name: run_loss(route, name, True)}


@pytest.mark.parametrize("family", ["ecmp", "fold", "loss"])
@pytest.mark.parametrize("name", ["k24", "ba80_prefer"])
def test_dispatch(route, name, family):
    """1031 source rows under SHD_ROUTE_DISPATCH.  k24 is complete: mode 2 of state_form, a grid
    of min(k, 1024) whose workgroups `continue` past the sweep after a lone barrier, also for
    their second source.  ba80_prefer mixes direct and tree entries in every row, in the LDS form."""
    from tests.multi_ref import Ref
    g = tree_graph(name)
    R = Ref(g)
    assert NS_TREE > TREE_LDS_CAP and NS_TREE <= (1 << 30) // (16 * g.n) and FAMILY_REF[family].fits_lds(g.n)
    if name == "k24":
        assert R.complete and len(tree_base(name)) == g.n
    else:
        direct = sum(R.is_direct(int(s), t, True) for s in tree_base(name)[:8] for t in range(g.n) if t != s)
        assert g.prefer_direct and not R.complete and 8 < direct < 4 * g.n
    RUN[family](route, name)


# -- the pair forms: pairs are grouped by distinct source, so the cap takes 1,056 vertices

GRID = "grid"


@functools.lru_cache(maxsize=None)
def grid_pairs():
    """Every vertex of the 1,056-vertex lattice as a source with three random targets (vertex 0's
    first is its neighbour 1, whose one shortest path is their edge), shuffled, weighted."""
    g = tout.graph(GRID)
    rng = np.random.default_rng(31)
    ps = np.repeat(np.arange(g.n, dtype=np.int32), 3)
    pt = ((ps + rng.integers(1, g.n, size=len(ps))) % g.n).astype(np.int32)     # no self pair: a third of the
    pt[0] = 1                                                                    # vertices has no self-loop
    pw = rng.integers(0, 1000, size=len(ps)).astype(np.uint64)
    pw[0], pw[7] = np.uint64(5), np.uint64(2 ** 40 + 3)
    k = rng.permutation(len(ps))
    return ps[k], pt[k], pw[k]


@functools.lru_cache(maxsize=None)
def grid_pair_ref(family):
    g = tout.graph(GRID)
    ps, pt, pw = grid_pairs()
    if family == "fold":
        return fr.FoldRef(g).pairs(ps, pt, FOLD_OPS, fr.columns(g))
    if family == "ecmp":
        E = er.EcmpRef(g)
        mult = int(np.unique(ps.astype(np.int64) * g.n + pt, return_counts=True)[1].max())
        return E.pairs(ps, pt, pw), E.tol(np.unique(ps), mult=mult)
    if family == "loss":
        L = lr.LossRef(g)
        return L.pairs(ps, pt, pw), L.pairs(ps, pt, pw, exact=True)
    O = tout.ref(GRID)
    es = O.ref.path(0, g.n - 1)[1]
    scn = [[int(O.ref.path(0, 1)[1][0])], sorted([int(es[1]), int(es[-2])])]
    return scn, O.repair(ps, pt, pw, scn)


@pytest.mark.parametrize("family", ["ecmp", "fold", "loss", "outage"])
def test_pair_forms(route, family):
    """shd_route_pair_{ecmp_loads,fold,loss,outage} over 1,056 distinct sources in one chunk, all
    in the LDS form: workgroups 0 .. 31 take a second source."""
    g = tout.graph(GRID)
    ps, pt, pw = grid_pairs()
    k = len(np.unique(ps))
    assert k == g.n == 1056 > TREE_LDS_CAP and k <= (1 << 30) // (16 * g.n)
    assert g.n < min(m.lds_max_n() for m in FAMILY_REF.values()) and g.vertex_packetloss is None
    eng = route.RouteEngine(g)
    want = grid_pair_ref(family)
    if family == "fold":
        assert not want[1] and not np.isnan(want[0]).any()
        got = eng.pair_fold(ps, pt, FOLD_OPS, fr.columns(g), dispatch=False)
        assert np.array_equal(got, want[0])
    elif family == "ecmp":
        (we, wt, wu, codes), rtol = want
        ge, gt, gu = eng.pair_ecmp_loads(ps, pt, pw, dispatch=False)
        assert not codes and gu == wu == 0
        assert er.close(ge, we, rtol) and er.close(gt, wt, rtol)
    elif family == "loss":
        f64, exact = want
        got = eng.pair_loss(ps, pt, pw, dispatch=False)
        assert (exact.R, exact.A, exact.unrouted, exact.codes) == (f64.R, f64.A, 0, set()) and got[4] == 0
        for j in range(4):
            assert lr.close(got[j], exact.outs()[j], exact.R, exact.A), (lr.NAMES[j], exact.R, exact.A)
    else:
        scn, w = want
        assert w.codes == frozenset({0}) and w.stats[:, orf.HIT].all() and w.stats[:, orf.SLOWER].any()
        st, mx, nl, un = eng.pair_outage(ps, pt, scn, pw, lat=True)
        assert un == w.unrouted == 0 and np.array_equal(st, w.stats) and np.array_equal(mx, w.max_add)
        assert np.array_equal(nl, w.lat, equal_nan=True) and not np.isnan(w.lat).any()
