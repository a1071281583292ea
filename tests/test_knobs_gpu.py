"""GPU: rows under the knob values no other test sets.

The selection, the planner and the K4 rows read some seventy SHD_ROUTE_* variables: the A/B
switches that performance work flips into defaults.  Behind the values below sit template
instantiations and plans of the seeded launch that are compiled into the product and that no
other test executes (tests/test_knobs.py, on the CPU, keeps the list complete).  Everything is
bit-exact against the oracle (TIE_MINKEY): lat, rel and row_min.

Rows kernels
  SHD_ROUTE_KBTCAP       KB's fused rows with many ragged target chunks (64 and 128 targets)
  SHD_ROUTE_HUB1024=0    the landmark hub rows in the context's own 256-thread block
  SHD_ROUTE_FWRBLK       fw_rows_kernel at 256 and 1024 threads
  SHD_ROUTE_FWP8BLK      fw_parent8_kernel at 256 and 512 threads
  SHD_ROUTE_FWPBLK       fw_parent_kernel at 512 and 1024 threads (SHD_ROUTE_FWP8=0)

Planner (tests/golden/make_plan_jobs.py KNOB_CASES, recorded in plan_jobs.json as well):
LMSEEDS, LMSPREAD, LMALL_SMALL, SEEDALPHA, HOPDEG, SEED_ROOTS, TOPCAP, STORE_SYNC, ROOTCOST,
LMCOST, FLAGAT, each on the graph and rank where it moves the plan.  A plan nobody has run may
be wrong in a way that makes a row wait for a flag nobody sets, so each plan's job records are
validated on the host (tests/plan_check.py) BEFORE its rows are launched; then the rows are held
to the oracle, and the plan's job digest to the default plan's: it must differ, or the case is
listed in INERT with the reason.

SHD_ROUTE_PLAN_THREADS is read when the process-wide planner workers are made: one fresh child
process per value."""
import functools
import json
import os
import queue

import numpy as np
import pytest

from shadow_amd.graph import complete_graph, internet_like
from tests import plan_check
from tests.golden import make_plan_jobs as mk
from tests.test_contract_gpu import close_engines, route  # noqa: F401
from tests.test_seed_gpu import _plan_rows, check_landmark_only_rank

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]:
        monkeypatch.delenv(k)


def check_rows(oracle_mod, g, S, T, got):
    lat, rel, mn = got
    olat, orel, _, _ = oracle_mod.OracleGraph(g).source_rows(S, T, oracle_mod.TIE_MINKEY)
    assert np.array_equal(lat, olat)
    assert np.array_equal(rel, orel)
    assert np.array_equal(mn, olat.min(axis=1))


# ---- KB: the fused rows' target chunks ---------------------------------------------------------

@pytest.mark.parametrize("targets", ["all", "subset65", "tiled3"])
@pytest.mark.parametrize("tcap", ["64", "128"])
@pytest.mark.parametrize("name", ["ba400", "c2"])
def test_kb_target_chunks(route, oracle_mod, monkeypatch, name, tcap, targets):
    """SHD_ROUTE_KBTCAP: the fused rows stage `tcap` targets at a time (default: as many as
    the LDS holds, one chunk when nt <= n), so a row's walks run once per chunk over a ragged
    last one: all targets (400 = 6 x 64 + 16, 2000 = 15 x 128 + 80), 65 unsorted targets with
    duplicates (64 + 1), and every target three times (nt > n).  tests/test_knobs.py holds
    kb.f_tcap to the knob on the CPU."""
    from tests.test_kb_gpu import _graph
    g = _graph(name)
    monkeypatch.setenv("SHD_ROUTE_KBTCAP", tcap)
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 2 and eng.info["reserved"] == 1      # KB, fused
    V = g.targets()
    rng = np.random.default_rng(int(tcap))
    if targets == "all":
        T = V
    elif targets == "subset65":
        t = rng.permutation(V)[:60]
        T = np.concatenate([t[:30], t[5:10], t[30:]]).astype(np.int32)
        assert len(T) == 65 and len(np.unique(T)) == 60
    else:
        T = np.tile(V, 3).astype(np.int32)
    assert len(T) % int(tcap) != 0 and (len(T) > int(tcap) or targets == "subset65")   # ragged; 65 = 64 + 1
    S = V if g.n <= 600 else V[3::41]
    check_rows(oracle_mod, g, S, T, eng.rows(S, T, dispatch=False))


# ---- KD: the landmark hub rows in the context's own block ---------------------------------------

@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1)])
def test_hub_rows_in_the_contexts_block(route, oracle_mod, monkeypatch, world, rank):
    """SHD_ROUTE_HUB1024=0 on a 256-thread KD context: the landmark rows of a landmark-only
    plan run in kd_plan_rows_kernel<256> with the context's queue and bucket width instead of
    the 1024-thread hub form.  The whole statement of test_landmark_only_plans holds.
    (tests/test_knobs.py: kd.hub_block is 0 under the knob and 1024 without.)"""
    monkeypatch.setenv("SHD_ROUTE_KERNEL", "kd")
    monkeypatch.setenv("SHD_ROUTE_HUB1024", "0")
    g = mk.graph("lmonly3000")
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 4 and eng.info["block"] == 256
    pos = check_landmark_only_rank(oracle_mod, monkeypatch, eng, oracle_mod.OracleGraph(g), world, rank)
    assert len(pos) == len(set(pos)) == len(range(rank, g.n, world))


# ---- K4 rows: the block sizes ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def k4_graph(name):
    return {"k130_odd": lambda: complete_graph(130, seed=6), "ba300": lambda: internet_like(300, 3, seed=17)}[name]()


@functools.lru_cache(maxsize=None)
def k4_ref(name):
    from oracle.oracle import OracleGraph, TIE_MINKEY
    g = k4_graph(name)
    V = np.arange(g.n, dtype=np.int32)
    lat, rel, _, _ = OracleGraph(g).source_rows(V, V, TIE_MINKEY)
    return lat, rel


K4_BLOCKS = [("SHD_ROUTE_FWRBLK", "256", False), ("SHD_ROUTE_FWRBLK", "1024", False),
             ("SHD_ROUTE_FWP8BLK", "256", False), ("SHD_ROUTE_FWP8BLK", "512", False),
             ("SHD_ROUTE_FWPBLK", "512", True), ("SHD_ROUTE_FWPBLK", "1024", True)]


@pytest.mark.parametrize("fwpk", ["1", "0"])
@pytest.mark.parametrize("name", ["k130_odd", "ba300"])
def test_k4_block_sizes(route, monkeypatch, name, fwpk):
    """fw_rows_kernel at 256 and 1024 threads, fw_parent8_kernel at 256 and 512, fw_parent_kernel
    (SHD_ROUTE_FWP8=0) at 512 and 1024, under both in-list key forms.  The block sizes are read
    at call time, so one context and one table per graph and key form serve every value; the
    sources are all vertices, in an order that puts a workgroup's eight sources far apart."""
    import torch
    g = k4_graph(name)
    assert g.latency.max() <= 255
    monkeypatch.setenv("SHD_ROUTE_FWPK", fwpk)
    eng = route.RouteEngine(g)
    eng.fw_table_async()
    dev = torch.device("cuda", 0)
    V = np.arange(g.n, dtype=np.int32)
    S = np.random.default_rng(g.n).permutation(V).astype(np.int32)
    d_src, d_tgt = torch.from_numpy(S).to(dev), torch.from_numpy(V).to(dev)
    olat, orel = k4_ref(name)
    for knob, val, one_source in K4_BLOCKS:
        monkeypatch.setenv(knob, val)
        if one_source:
            monkeypatch.setenv("SHD_ROUTE_FWP8", "0")
        lat = torch.full((g.n, g.n), -7.0, dtype=torch.float64, device=dev)
        rel = torch.full_like(lat, -7.0)
        mn = torch.full((g.n,), -7.0, dtype=torch.float64, device=dev)
        eng.fw_rows_async(d_src, d_tgt, lat, rel, mn)
        eng.sync()
        monkeypatch.delenv(knob)
        monkeypatch.delenv("SHD_ROUTE_FWP8", raising=False)
        assert np.array_equal(lat.cpu().numpy(), olat[S]), (knob, val)
        assert np.array_equal(rel.cpu().numpy(), orel[S]), (knob, val)
        assert np.array_equal(mn.cpu().numpy(), olat[S].min(axis=1)), (knob, val)


# ---- the planner ------------------------------------------------------------------------------

def _matrix():
    """id -> (graph, environment, world, rank, knob): the recorded cases of make_plan_jobs.KNOB_CASES
    and, around them, the same values on the other ranks and graphs: ba400 at world 1 and every rank
    of world 3, lmonly3000 at world 1 and world 3 rank 1, roots300."""
    m = {name: mk.KNOB_CASES[name] + (mk.KNOB_OF[name],) for name in mk.KNOB_CASES}

    def add(gname, base, world, rank, knob, value):
        tag = gname + ("" if world == 1 else f"-w{world}r{rank}")
        m.setdefault(f"{tag}-{knob[10:].lower()}{value}", (gname, {**base, knob: value}, world, rank, knob))

    everywhere = (("SHD_ROUTE_LMSEEDS", "1"), ("SHD_ROUTE_LMSEEDS", "2"), ("SHD_ROUTE_SEEDALPHA", "0"),
                  ("SHD_ROUTE_SEEDALPHA", "10"), ("SHD_ROUTE_HOPDEG", "1"), ("SHD_ROUTE_SEED_ROOTS", "0"),
                  ("SHD_ROUTE_SEED_ROOTS", "1"), ("SHD_ROUTE_SEED_ROOTS", "1000000"))
    for world, rank in ((1, 0), (3, 0), (3, 1), (3, 2)):
        for knob, value in everywhere:
            add("ba400", mk.KD7, world, rank, knob, value)
        if world == 3:
            for value in ("1", "64"):
                add("ba400", mk.KD7, world, rank, "SHD_ROUTE_TOPCAP", value)
    add("ba400", mk.KD7, 3, 1, "SHD_ROUTE_STORE_SYNC", "1")
    for world, rank in ((1, 0), (3, 1)):
        for knob, value in (("SHD_ROUTE_LMSEEDS", "1"), ("SHD_ROUTE_LMSEEDS", "2"), ("SHD_ROUTE_LMSPREAD", "0"),
                            ("SHD_ROUTE_LMALL_SMALL", "0")):
            add("lmonly3000", mk.KD, world, rank, knob, value)
    for knob, value in (("SHD_ROUTE_LMSEEDS", "1"), ("SHD_ROUTE_LMSEEDS", "2"), ("SHD_ROUTE_LMSPREAD", "0"),
                        ("SHD_ROUTE_SEED_ROOTS", "0"), ("SHD_ROUTE_ROOTCOST", "50"), ("SHD_ROUTE_LMCOST", "50")):
        add("roots300", mk.KD, 1, 0, knob, value)
    return m


MATRIX = _matrix()

# cases whose job digest equals that of the plan without the knob (same graph, world, rank and
# the rest of the environment), and why
_ONE_START = ("the estimate shortens the only root's row: with one row running and six of the seven slots "
              "free either way, every other row still starts when its seeds' flags are up, in the same order")
_DEVICE_BUILT = ("300 rows on 1024 slots: a landmark-only plan built on the device, every row a landmark-seeded "
                 "root at level 0; no unseeded roots to choose and no list schedule to cost")
INERT = {
    "ba400-store_sync1": "moves the row store's allocation to the planning thread: when, not what",
    "ba400-w3r1-store_sync1": "moves the row store's allocation to the planning thread: when, not what",
    "ba400-rootcost0.1": _ONE_START,
    "ba400-lmcost0.1": _ONE_START,
    "lmonly3000-w3r1-lmall_small0": "1000 rows on 1024 slots: landmark-only by the rows-per-slot rule "
                                    "(SHD_ROUTE_LMALL) whatever the small-graph rule says",
    "roots300-seed_roots0": _DEVICE_BUILT,
    "roots300-rootcost50": _DEVICE_BUILT,
    "roots300-lmcost50": _DEVICE_BUILT,
}


@functools.lru_cache(maxsize=None)
def oracle_table(gname):
    """The oracle's latency table of the graph (every d(s, u) the validation asks for) and its
    reliability table."""
    from oracle.oracle import OracleGraph, TIE_MINKEY
    g = mk.graph(gname)
    V = np.arange(g.n, dtype=np.int32)
    lat, rel, _, _ = OracleGraph(g).source_rows(V, V, TIE_MINKEY)
    for a in (lat, rel):
        a.setflags(write=False)
    return lat, rel


def validated_plan(eng, T, world, rank, D):
    """The plan, its job array and the validation's summary.  A device-built landmark-only plan
    is refreshed first, so that the records read are the ones a reusing rows call launches."""
    plan = eng.plan(T, world, rank)
    lm = plan.landmarks()
    if lm is not None:
        plan.refresh_async()
        eng.sync()
    jobs = plan.jobs()
    assert plan.info["seeded"] == 1 and jobs is not None, plan.info
    summary = plan_check.validate(jobs, T, plan.positions, lambda s: D[s], lm)
    return plan, jobs, summary


@functools.lru_cache(maxsize=None)
def reference_plan(gname, env, world, rank):
    """(job digest, info) of the plan without the knob, built in that environment alone."""
    from shadow_amd import route
    old = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]}
    os.environ.update(dict(env))
    try:
        g = mk.graph(gname)
        eng = route.RouteEngine(g)
        plan = eng.plan(g.targets(), world, rank)
        out = mk.jobs_digest(plan.jobs()), dict(plan.info)
        plan.close()
        eng.close()
    finally:
        for k in dict(env):
            os.environ.pop(k, None)
        os.environ.update(old)
    return out


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_planner_knob(route, monkeypatch, case):
    gname, env, world, rank, knob = MATRIX[case]
    ref_digest, ref_info = reference_plan(gname, tuple(sorted((k, v) for k, v in env.items() if k != knob)), world, rank)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = mk.graph(gname)
    olat, orel = oracle_table(gname)
    eng = route.RouteEngine(g)
    assert eng.info["kernel"] == 4
    T = g.targets()
    # 1, 2: the plan, validated before any of its rows is launched
    plan, jobs, summary = validated_plan(eng, T, world, rank, olat)
    info = dict(plan.info)
    if case == "lmonly3000-lmall_small0":
        # a neighbour-seeded plan on a 256-thread context at n >= 2048, which no default reaches
        assert eng.info["block"] == 256 and g.n >= 2048
        assert info["seeded"] == 1 and info["launches"] != 4 and info["levels"] > 1 and summary["row_seeds"] > 0, info
        assert ref_info["launches"] == 4 and ref_info["levels"] == 1
    if knob == "SHD_ROUTE_LMSEEDS":
        # that many landmark seeds on a row at the most (a landmark slot: one no job writes)
        kept = set(jobs["store"][jobs["store"] >= 0].tolist())
        per_row = [sum(int(q) not in kept for q in j["seed"][:j["nseed"]]) for j in jobs]
        assert max(per_row) == int(env[knob]), max(per_row)
    # 3: the rows
    lat, rel, mn = _plan_rows(eng, plan, T, reuse=plan.landmarks() is not None)
    pos = plan.positions
    assert np.array_equal(lat, olat[pos])
    assert np.array_equal(rel, orel[pos])
    assert np.array_equal(mn, olat[pos].min(axis=1))
    # 4: the knob moved the plan, or is known not to
    digest = mk.jobs_digest(jobs)
    if case in INERT:
        assert digest == ref_digest and info == ref_info, f"{case} moves the plan now: take it out of INERT"
    else:
        assert digest != ref_digest, f"{case} leaves the plan as it is without the knob: it proves nothing here"


def test_knob_cases_cover_every_value():
    """One recorded case per planner knob value of the list, every inert case named."""
    want = {("LMSEEDS", "1"), ("LMSEEDS", "2"), ("LMSPREAD", "0"), ("LMALL_SMALL", "0"), ("SEEDALPHA", "0"),
            ("SEEDALPHA", "10"), ("HOPDEG", "1"), ("HOPDEG", "100000"), ("SEED_ROOTS", "0"), ("SEED_ROOTS", "1"),
            ("SEED_ROOTS", "1000000"), ("TOPCAP", "1"), ("TOPCAP", "64"), ("STORE_SYNC", "1"), ("ROOTCOST", "0.1"),
            ("ROOTCOST", "50"), ("LMCOST", "0.1"), ("LMCOST", "50"), ("FLAGAT", "0"), ("FLAGAT", "1")}
    have = {(mk.KNOB_OF[c][len("SHD_ROUTE_"):], mk.CASES[c][1][mk.KNOB_OF[c]]) for c in mk.KNOB_CASES}
    assert have == want and len(mk.KNOB_CASES) == len(want)
    assert set(mk.KNOB_CASES) <= set(MATRIX) and set(INERT) <= set(MATRIX)
    with open(os.path.join(GOLD, "plan_jobs.json")) as f:
        assert set(mk.KNOB_CASES) <= set(json.load(f))


# ---- SHD_ROUTE_PLAN_THREADS ---------------------------------------------------------------------

def _threads_worker(nth, q):
    import torch
    torch.cuda.init()  # torch's HIP runtime before the engine's (see conftest)
    for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]:
        del os.environ[k]
    os.environ.update(mk.case_env("ba400-hostchoice"))
    os.environ["SHD_ROUTE_PLAN_THREADS"] = str(nth)      # read when the first plan makes the workers
    q.put(mk.record("ba400-hostchoice"))


@pytest.mark.parametrize("nth", [1, 5])
def test_plan_threads(nth):
    """The plan does not depend on the number of planner threads: one (no workers: the planning
    thread makes the seed choices itself) and five, each in a fresh process, reproduce the
    recorded host-choice plan."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_threads_worker, args=(nth, q))
    p.start()
    got = None
    while got is None:
        try:
            got = q.get(timeout=0.5)
        except queue.Empty:
            assert p.is_alive(), f"the child ended with {p.exitcode} and no result"
    p.join(timeout=120)
    assert p.exitcode == 0
    with open(os.path.join(GOLD, "plan_jobs.json")) as f:
        want = json.load(f)["ba400-hostchoice"]
    assert got == want
