"""GPU: several live contexts in one process.  A context sets the dynamic-LDS limit of its
kernel functions (hipFuncAttributeMaxDynamicSharedMemorySize) to its own size when it is created,
or at the first hops / K4 call; the limit belongs to the function, so a second, smaller context
lowers it under the first one's feet.  For every pair of tests/test_contexts.py (checked there,
on the CPU, to ask for amounts a factor of two apart, past 64 KiB where the form gets there):

  rows     create large and small in both orders, then run large, small and large again through
           shd_route_rows_async; the KD pairs also through a device-built landmark-only plan of
           each (kd_plan_rows_kernel: the context's own rows, and the 1024-thread hub rows)
  lazy     A.hops, B.hops, A.hops, and the same for shd_route_fw_table_async +
           shd_route_fw_rows_async: the limit is set at the first call of each context
  closing  the small context is destroyed while the large one has a launch queued behind a
           timed gate; that launch's result is right

Everything equals the CPU oracle (TIE_MINKEY, bit for bit; the sized graphs have no vertex
loss), over the sources of test_range_gpu.sources (16 on the large graphs).  A launch the
runtime refused would come back as SHD_ROUTE_EDEVICE from the call, which raises.
"""
import numpy as np
import pytest

from tests import shape_graphs
from tests import stream_order as so
from tests.test_contexts import KERNEL_OF, PAIRS
from tests.test_contract_gpu import close_engines, route  # noqa: F401
from tests.test_range_gpu import _KNOBS, dev_rows, has_loop, oracle_rows, row_min_of, sources

pytestmark = pytest.mark.gpu

ROWS_PAIRS = [p for p in sorted(PAIRS) if p not in ("hops", "k4")]
_REF = {}


def ref_of(oracle_mod, gname):
    """Per graph, once: the sources, their oracle rows and hop rows over all vertices."""
    if gname not in _REF:
        g = shape_graphs.get(gname)
        assert g.vertex_packetloss is None
        S, T = sources(g), np.arange(g.n, dtype=np.int32)
        lat, rel, hops = oracle_rows(oracle_mod, oracle_mod.OracleGraph(g), g, S, T)
        _REF[gname] = dict(g=g, S=S, T=T, lat=lat, rel=rel, hops=hops, failed=bool((~has_loop(g)[S]).any()))
        assert _REF[gname]["failed"]
    return _REF[gname]


def set_env(monkeypatch, env):
    for k in _KNOBS + ("SHD_ROUTE_KDBLOCK", "SHD_ROUTE_LANDMARKS", "SHD_ROUTE_LMALL", "SHD_ROUTE_HOPS_LDS",
                       "SHD_ROUTE_HOPS_SCRATCH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_pair(route, oracle_mod, monkeypatch, name, order):
    """(large, small) as (engine, reference), created in the given order."""
    env, big, small = PAIRS[name][:3]
    set_env(monkeypatch, env)
    made = {}
    for gname in ((big, small) if order == "large_first" else (small, big)):
        ref = ref_of(oracle_mod, gname)
        made[gname] = (route.RouteEngine(ref["g"]), ref)
    want = KERNEL_OF[name]
    for eng, _ in made.values():
        i = eng.info
        assert "sel" not in want or i["kernel"] == want["sel"]
        for key in ("k32.block", "kd.block", "kf.block"):
            assert key not in want or i["block"] == want[key]
        assert "kb.fused" not in want or i["reserved"] == want["kb.fused"]
        assert "kf.h" not in want or i["lds_resident"] == 1 - want["kf.h"]
    return made[big], made[small]


def check_rows(route, eng, ref, launch=None, rows=None):
    S = ref["S"] if rows is None else ref["S"][rows]
    want_l = ref["lat"] if rows is None else ref["lat"][rows]
    want_r = ref["rel"] if rows is None else ref["rel"][rows]
    lat, rel, mn, code = dev_rows(route, eng, S, ref["T"], launch)
    assert code == route.ENOEDGE
    assert np.array_equal(lat, want_l, equal_nan=True) and np.array_equal(rel, want_r, equal_nan=True)
    assert np.array_equal(mn, row_min_of(want_l))


@pytest.mark.parametrize("order", ["large_first", "small_first"])
@pytest.mark.parametrize("name", ROWS_PAIRS)
def test_rows_of_two_live_contexts(route, oracle_mod, monkeypatch, name, order):
    (A, ra), (B, rb) = make_pair(route, oracle_mod, monkeypatch, name, order)
    for eng, ref in ((A, ra), (B, rb), (A, ra), (B, rb)):
        check_rows(route, eng, ref)
    if not name.startswith("kd"):
        return
    # a device-built landmark-only plan of each: kd_plan_rows_kernel at the context's block size
    # and, with at most 256 landmarks on a 256-thread context, the 1024-thread hub rows
    plans = []
    for eng, ref in ((A, ra), (B, rb)):
        p = eng.plan(ref["S"])
        lm = p.landmarks()
        assert p.info["seeded"] == 1 and p.info["launches"] >= 3 and lm is not None, p.info
        assert (lm["nland"] <= 256) == (name == "kd_hub" or ref["g"].n <= 256)
        plans.append(p)
    for (eng, ref), p in list(zip(((A, ra), (B, rb)), plans)) * 2:
        check_rows(route, eng, ref, lambda d_s, d_t, la, re, mn: p.rows_async(d_t, la, re, mn, dispatch=False),
                   rows=p.positions)
    for p in plans:
        p.close()


def test_lazy_hops_limit(route, oracle_mod, monkeypatch):
    """ensure_hops sets hops_depth_kernel's limit at a context's first hops call: A.hops, B.hops
    (lowers it), A.hops, B.hops."""
    import torch
    (A, ra), (B, rb) = make_pair(route, oracle_mod, monkeypatch, "hops", "large_first")
    for eng, ref in ((A, ra), (B, rb), (A, ra), (B, rb)):
        S, T = ref["S"], ref["T"]
        d_s = torch.from_numpy(S).to(so.dev()); d_t = torch.from_numpy(T).to(so.dev())
        h = torch.full((len(S), len(T)), -7, dtype=torch.int32, device=so.dev())
        mx = torch.full((len(S),), -7, dtype=torch.int32, device=so.dev())
        eng.hops_async(d_s, d_t, h, mx, dispatch=False)
        assert so.sync_code(route, eng) == route.ENOEDGE
        assert np.array_equal(h.cpu().numpy(), ref["hops"]) and np.array_equal(mx.cpu().numpy(), ref["hops"].max(axis=1))


def test_lazy_k4_limits(route, oracle_mod, monkeypatch):
    """fw_prepare sets the limits of fw_rows_kernel, fw_inlist_kernel and the parent kernels at
    a context's first table call: A, B (lowers them), A, B."""
    (A, ra), (B, rb) = make_pair(route, oracle_mod, monkeypatch, "k4", "large_first")
    for eng, ref in ((A, ra), (B, rb), (A, ra), (B, rb)):
        def launch(d_s, d_t, la, re, mn):
            eng.fw_table_async()
            eng.fw_rows_async(d_s, d_t, la, re, mn)
        check_rows(route, eng, ref, launch)


@pytest.mark.parametrize("name", ["kb_fused", "kd_1024", "f64"])
def test_close_small_while_large_is_pending(route, oracle_mod, monkeypatch, name):
    """The small context is destroyed while the large one's rows wait behind a timed gate on a
    side stream: the rows are right."""
    import torch
    (A, ra), (B, rb) = make_pair(route, oracle_mod, monkeypatch, name, "large_first")
    check_rows(route, B, rb)
    S, T = ra["S"], ra["T"]
    d_s = torch.from_numpy(S).to(so.dev()); d_t = torch.from_numpy(T).to(so.dev())
    lat = torch.zeros((len(S), len(T)), dtype=torch.float64, device=so.dev()); rel = torch.zeros_like(lat)
    mn = torch.zeros(len(S), dtype=torch.float64, device=so.dev())
    side = torch.cuda.Stream()
    opened = torch.cuda.Event()
    cpm = so.cycles_per_ms()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(so.GATE_FLOOR_MS * cpm))
        opened.record(side)
    A.rows_async(d_s, d_t, lat, rel, mn, stream=side.cuda_stream, dispatch=False)
    pending = not opened.query()
    B.close()
    assert so.sync_code(route, A, side.cuda_stream) == route.ENOEDGE
    assert pending, "the gate opened before the small context was closed"
    assert np.array_equal(lat.cpu().numpy(), ra["lat"], equal_nan=True)
    assert np.array_equal(rel.cpu().numpy(), ra["rel"], equal_nan=True)
    assert np.array_equal(mn.cpu().numpy(), row_min_of(ra["lat"]))
