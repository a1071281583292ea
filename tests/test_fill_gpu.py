"""GPU: the machinery that takes the rows of shd_route_fill_triangle to the host triangle -- the
two staging buffers and their reuse, the rank shares, the copies cut at the registration
boundaries of lazily pinned memory, the grid-stride loop of the two pack kernels -- at sizes
that run in seconds, through two knobs that shrink the compile-time sizes:

  SHD_ROUTE_FILL_STAGE   pairs per staging buffer (default 32 Mi; never below one row, a multiple of 4)
  SHD_ROUTE_HOST_CHUNK   bytes per chunk of shd_route_host_alloc / _lazy (default 256 MiB; 2 MiB multiples)

The reference is the CPU oracle under TIE_MINKEY over A x A (tests/test_range_gpu.oracle_rows;
dispatch_ref on a prefer-direct graph, as the front end passes SHD_ROUTE_DISPATCH), compared bit
for bit by value (a failed entry is NaN, whatever its payload); buffers of different settings are
compared byte for byte with each other, which also holds the pad slots and pad bytes of the
compact lines; check_pads states what those must be.  No graph of the engine tests here has
vertex loss; the front-end test holds its one graph with vertex loss (ba120_vloss) to the golden
table within REL_TOL, the rule of test_gpu_parity.py for that table, and bit for bit to the same
front end without the knobs.

What each test reaches (chunk counts are computed from the sizes by stage_chunks and asserted):

  test_stage_chunks_and_buffer_reuse  454 to 682 stage chunks (one row each at the top) and 31
      to 69 at 8 na: every staging buffer packed again after its copy, hundreds of times
  test_rank_shares                    world 2 and 3 called directly: one block per rank (KB) and,
      under KD's seeded plan, 352 to 528 one-row pieces per rank; bytes outside the rank's rows
      untouched
  test_rank_without_rows, test_no_vertices, test_tiny_compact_rows
  test_lazy_chunks                    2 MiB registrations: 5 (interleaved) and 3 (compact) chunks,
      rows straddling each boundary, a refused chunk in the middle, memory of neither allocator
  test_more_than_4096_rows_in_a_chunk 4097 rows in one launch of 4096 workgroups
  test_front_end_under_the_knobs      devices=(0, 0) with both knobs at their minimum
"""
import ctypes

import numpy as np
import pytest

from tests import shape_graphs as sg
from tests.test_range_gpu import REL_TOL, dispatch_ref, has_loop, oracle_rows, read_triangle, route  # noqa: F401
from tests.test_shape_gpu import choose

pytestmark = pytest.mark.gpu

CAN64 = 0x7FF8DEADBEEF0001      # (a NaN with a payload no kernel produces)
MIB = 1 << 20
DEFAULT_STAGE = 32 << 20        # pairs (fill_sched.hpp FILL_STAGE_PAIRS)
KNOBS = ("SHD_ROUTE_FILL_STAGE", "SHD_ROUTE_HOST_CHUNK", "SHD_ROUTE_REGFAIL_CHUNK")


@pytest.fixture(autouse=True)
def close_all(route, monkeypatch):
    """Every context and pinned buffer a test makes is closed when the test ends (contexts
    first, their plans before them), also when it fails half-way."""
    engines, buffers = [], []
    real_e, real_b = route.RouteEngine, route.PinnedBuffer

    def engine(*a, **k):
        engines.append(real_e(*a, **k))
        return engines[-1]

    def buffer(*a, **k):
        buffers.append(real_b(*a, **k))
        return buffers[-1]
    monkeypatch.setattr(route, "RouteEngine", engine)
    monkeypatch.setattr(route, "PinnedBuffer", buffer)
    yield
    for e in reversed(engines):
        e.close()
    for b in reversed(buffers):
        b.close()


def knobs(monkeypatch, stage=None, chunk=None, regfail=None, sel="auto"):
    """The kernel choice (tests/test_range_gpu.SELECTIONS), and the fill knobs as given (None: unset)."""
    choose(monkeypatch, sel)
    for k, v in zip(KNOBS, (stage, chunk, regfail)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


# ---- sizes, from include/shd_route.h ---------------------------------------------------------

def row_units(na, lat16):
    """Pairs (interleaved) or 64-byte lines (compact) of each row of the triangle."""
    e = na - np.arange(na, dtype=np.int64)
    return (e + 5) // 6 if lat16 else e


def row_bytes(route, na, lat16):
    """(first byte, byte past the last) of each row, and the triangle's bytes."""
    u = row_units(na, lat16) * (64 if lat16 else 16)
    end = np.cumsum(u)
    nbytes = 64 * route.tri16_lines(na) if lat16 else 16 * (na * (na + 1) // 2)
    assert (int(end[-1]) if na else 0) == nbytes
    return end - u, end, nbytes


def min_stage(na, lat16):
    """The smallest effective SHD_ROUTE_FILL_STAGE: one whole row, in pairs, a multiple of 4."""
    return (max(1, 4 * ((na + 5) // 6) if lat16 else na) + 3) & ~3


def stage_chunks(na, positions, lat16, stage):
    """The stage chunks of the rows `positions` (plan order) under SHD_ROUTE_FILL_STAGE=stage
    (None: unset): rows are taken while they fit the buffer."""
    pairs = DEFAULT_STAGE if stage is None else (max(int(stage), min_stage(na, lat16)) + 3) & ~3
    cap = pairs // 4 if lat16 else pairs
    u = row_units(na, lat16)
    n, acc = 0, 0
    for i in positions:
        if acc and acc + int(u[i]) > cap:
            n, acc = n + 1, 0
        acc += int(u[i])
    return n + (acc > 0)


def owned_mask(route, na, lat16, positions):
    lo, hi, nbytes = row_bytes(route, na, lat16)
    m = np.zeros(nbytes, bool)
    for i in positions:
        m[lo[i]:hi[i]] = True
    return m


def check_pads(raw8, na):
    """The compact layout: bytes 60-63 of every line are zero; the slots past a row's last pair
    hold rel 0.0 and lat 0xFFFF."""
    lines = raw8.reshape(-1, 64)
    assert not lines[:, 60:].any()
    e = na - np.arange(na, dtype=np.int64)
    nl = (e + 5) // 6
    last = np.cumsum(nl) - 1
    used = e - 6 * (nl - 1)
    u16 = lines.view(np.uint16)
    for k in range(1, 6):
        rows = last[used <= k]
        assert not lines[rows, 8 * k: 8 * k + 8].any() and np.all(u16[rows, 24 + k] == 0xFFFF)


# ---- buffers --------------------------------------------------------------------------------

def bytes_of(buf, nbytes):
    """The buffer's bytes as a uint8 view (not a copy)."""
    return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(buf.ptr), np.uint8)


def canary(buf, nbytes):
    bytes_of(buf, nbytes).view(np.uint64)[:] = CAN64


class NumpyBuffer:
    """Memory of neither allocator behind the .ptr / .array() of a PinnedBuffer."""

    def __init__(self, nbytes, content=None):
        self.mem = np.full(nbytes // 8, CAN64, np.uint64)
        self.ptr = self.mem.ctypes.data
        if content is not None:
            self.mem.view(np.uint8)[:] = content

    def array(self):
        return self.mem.view(np.float64)


# ---- the reference --------------------------------------------------------------------------

_REF = {}


def reference(oracle_mod, name, which="all", rows=None):
    """Per (graph, attached list), computed once and never written to: A ("all": every vertex,
    "loops": the self-looped ones, an int k: the first k vertices) and the oracle's (lat, rel)
    over A x A, NaN where the source has no self-loop and is the target.  rows: the oracle is
    asked for these rows of A only (the others stay NaN and must not be compared)."""
    key = (name, which)
    if key not in _REF:
        g = sg.get(name)
        hl = has_loop(g)
        A = (np.arange(g.n) if which == "all" else np.flatnonzero(hl) if which == "loops" else np.arange(which)).astype(np.int32)
        S = A if rows is None else A[rows]
        if g.prefer_direct:
            lat, rel = dispatch_ref(oracle_mod, g, S, A)
        else:
            lat, rel, _ = oracle_rows(oracle_mod, oracle_mod.OracleGraph(g), g, S, A)
        if rows is not None:
            full_l = np.full((len(A), len(A)), np.nan); full_r = np.full((len(A), len(A)), np.nan)
            full_l[rows], full_r[rows] = lat, rel
            lat, rel = full_l, full_r
        lat.setflags(write=False); rel.setflags(write=False)
        _REF[key] = dict(g=g, A=A, na=len(A), lat=lat, rel=rel, noloop=bool((~hl[A]).any()))
    return _REF[key]


def kept_min(lat, positions):
    """The smallest latency among the kept entries (j >= i) of the rows `positions`; +inf if none."""
    v = [lat[i, i:] for i in positions]
    v = np.concatenate(v) if v else np.empty(0)
    v = v[~np.isnan(v)]
    return float(v.min()) if len(v) else float("inf")


def check_rows(route, ref, buf, lat16, positions, tables=None):
    """The rows `positions` of the buffer (tables: its read_triangle, if the caller has it) hold
    the oracle's values, bit for bit."""
    lat, rel = tables or read_triangle(route, buf, ref["na"], lat16)
    for i in positions:
        assert np.array_equal(lat[i, i:], ref["lat"][i, i:], equal_nan=True), i
        assert np.array_equal(rel[i, i:], ref["rel"][i, i:], equal_nan=True), i


def eager_fill(route, eng, ref, lat16):
    """One fill of all rows into a canary-filled eager buffer: (bytes copy, min, code)."""
    _, _, nbytes = row_bytes(route, ref["na"], lat16)
    buf = route.PinnedBuffer(nbytes)
    canary(buf, nbytes)
    mn, _ = eng.fill_triangle(ref["A"], buf, dispatch=True, lat16=lat16)
    out = bytes_of(buf, nbytes).copy()
    buf.close()
    return out, mn, eng.last_fill_code


# ---- a. stage chunks and buffer reuse -------------------------------------------------------

@pytest.mark.parametrize("lat16", [False, True])
@pytest.mark.parametrize("which", ["all", "loops"])
def test_stage_chunks_and_buffer_reuse(route, oracle_mod, monkeypatch, which, lat16):
    """The 32 x 33 grid over every vertex (NaN / 0xFFFF diagonals without a self-loop, ENOEDGE)
    and over its self-looped vertices (OK), SHD_ROUTE_FILL_STAGE at its minimum (one row per
    chunk at the top of the triangle), at 8 na and unset: byte-identical buffers, the unset one
    equal to the oracle."""
    ref = reference(oracle_mod, "grid", which)
    A, na = ref["A"], ref["na"]
    _, _, nbytes = row_bytes(route, na, lat16)
    order = list(range(na))
    knobs(monkeypatch)
    eng = route.RouteEngine(ref["g"])
    assert eng.info["lat16"] == 1
    assert stage_chunks(na, order, lat16, None) == 1
    base, mn, code = eager_fill(route, eng, ref, lat16)
    assert code == (route.ENOEDGE if which == "all" else route.OK) and ref["noloop"] == (which == "all")
    check_rows(route, ref, NumpyBuffer(nbytes, base), lat16, order)
    assert mn == kept_min(ref["lat"], order) == np.nanmin(ref["lat"][np.triu_indices(na)])
    assert np.isnan(ref["lat"][np.triu_indices(na)]).sum() == (na - int(has_loop(ref["g"])[A].sum()))
    if lat16:
        check_pads(base, na)
    for stage in (1, 8 * na):
        n = stage_chunks(na, order, lat16, stage)
        print("grid", which, "lat16", lat16, "stage", stage, "->", n, "chunks")
        assert n >= 5                       # each buffer packed twice at least after its first copy
        if stage == 1:
            assert stage_chunks(na, order[:4], lat16, stage) == 4      # one row per chunk at the top
        knobs(monkeypatch, stage=stage)
        got, mn2, code2 = eager_fill(route, eng, ref, lat16)
        assert np.array_equal(got, base) and mn2 == mn and code2 == code
    knobs(monkeypatch, stage="abc")         # not a number: the default
    got, mn2, code2 = eager_fill(route, eng, ref, lat16)
    assert np.array_equal(got, base) and mn2 == mn and code2 == code


# ---- b. rank shares called directly ---------------------------------------------------------

@pytest.mark.parametrize("stage", [1, None])
@pytest.mark.parametrize("lat16", [False, True])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,sel", [("grid", "auto"), ("grid", "kd"), ("dir_grid", "auto")])
def test_rank_shares(route, oracle_mod, monkeypatch, name, sel, world, lat16, stage):
    """Every rank of world 2 and 3 in turn into one canary-filled eager buffer: after each call
    the rank's rows (plan(A, world, rank).positions) hold the oracle's values, every byte
    outside them is what it was before, and min_out is the minimum over the rank's kept
    entries; at the end the buffer is the world = 1 buffer and the positions cover range(na).
    Under the auto choice (KB on these graphs) a rank's rows are one block of the triangle; under
    KD on the grid the plan is seeded and its partition leaves no two rows of a rank adjacent, so
    every row is a copy piece of its own."""
    ref = reference(oracle_mod, name)
    A, na = ref["A"], ref["na"]
    _, _, nbytes = row_bytes(route, na, lat16)
    knobs(monkeypatch, sel=sel)
    eng = route.RouteEngine(ref["g"])
    base, mn1, code1 = eager_fill(route, eng, ref, lat16)
    knobs(monkeypatch, stage=stage, sel=sel)
    buf = route.PinnedBuffer(nbytes)
    canary(buf, nbytes)
    view = bytes_of(buf, nbytes)
    seen, mins, codes, seeded, runs = [], [], [], [], []
    for rank in range(world):
        plan = eng.plan(A, world, rank)
        pos = [int(p) for p in plan.positions]
        seeded.append(plan.info["seeded"])
        plan.close()
        before = view.copy()
        mn, _ = eng.fill_triangle(A, buf, world=world, rank=rank, dispatch=True, lat16=lat16)
        own = owned_mask(route, na, lat16, pos)
        assert np.array_equal(view[~own], before[~own])
        assert np.array_equal(view[own], base[own])
        check_rows(route, ref, buf, lat16, pos)
        assert mn == kept_min(ref["lat"], pos)
        nan_rows = bool(np.isnan(ref["lat"][pos, pos]).any())
        assert eng.last_fill_code == (route.ENOEDGE if nan_rows else route.OK)
        runs.append(1 + int((np.diff(pos) != 1).sum()) if pos else 0)
        print(name, sel, "world", world, "rank", rank, "rows", len(pos), "seeded", seeded[-1], "chunks",
              stage_chunks(na, pos, lat16, stage), "runs", runs[-1], "ascending", pos == sorted(pos))
        seen += pos; mins.append(mn); codes.append(eng.last_fill_code)
    assert sorted(seen) == list(range(na))
    assert np.array_equal(view, base) and min(mins) == mn1 and min(codes) == code1
    if sel == "kd":                 # a seeded plan: the forest's partition, one copy piece per row here
        assert all(seeded) and min(runs) > na // (2 * world)


def test_rank_without_rows(route, oracle_mod, monkeypatch):
    """tiny3_some over eight ranks: a rank without rows returns OK, writes nothing and gives
    +inf; the others write their rows only."""
    ref = reference(oracle_mod, "tiny3_some")
    A, na = ref["A"], ref["na"]
    knobs(monkeypatch)
    eng = route.RouteEngine(ref["g"])
    for lat16 in (False, True):
        _, _, nbytes = row_bytes(route, na, lat16)
        buf = route.PinnedBuffer(nbytes + 64)
        canary(buf, nbytes + 64)
        view = bytes_of(buf, nbytes + 64)
        seen, empty = [], 0
        for rank in range(8):
            plan = eng.plan(A, 8, rank)
            pos = [int(p) for p in plan.positions]
            plan.close()
            before = view.copy()
            mn, _ = eng.fill_triangle(A, buf, world=8, rank=rank, dispatch=True, lat16=lat16)
            if not pos:
                empty += 1
                assert eng.last_fill_code == route.OK and mn == float("inf") and np.array_equal(view, before)
            else:
                own = np.concatenate([owned_mask(route, na, lat16, pos), np.zeros(64, bool)])
                assert np.array_equal(view[~own], before[~own])
                check_rows(route, ref, buf, lat16, pos)
                assert mn == kept_min(ref["lat"], pos)
            seen += pos
        assert sorted(seen) == list(range(na)) and empty >= 5
        if lat16:
            check_pads(view[:nbytes], na)


def test_no_vertices(route, monkeypatch):
    """na = 0: OK, +inf, nothing written."""
    knobs(monkeypatch)
    eng = route.RouteEngine(sg.get("tiny3_some"))
    buf = route.PinnedBuffer(64)
    canary(buf, 64)
    for lat16 in (False, True):
        for world, rank in ((1, 0), (3, 2)):
            mn, _ = eng.fill_triangle(np.empty(0, np.int32), buf, world=world, rank=rank, lat16=lat16)
            assert eng.last_fill_code == route.OK and mn == float("inf")
    assert np.all(bytes_of(buf, 64).view(np.uint64) == CAN64)


@pytest.mark.parametrize("stage", [1, None])
@pytest.mark.parametrize("lat16", [True, False])
@pytest.mark.parametrize("na", [1, 5, 6, 7])
def test_tiny_compact_rows(route, oracle_mod, monkeypatch, na, lat16, stage):
    """The first 1, 5, 6 and 7 vertices of tiny9_some: in the compact layout a first row whose
    last line is one short, full, and one over; the 64 bytes after the triangle keep their canary."""
    ref = reference(oracle_mod, "tiny9_some", na)
    _, _, nbytes = row_bytes(route, na, lat16)
    knobs(monkeypatch, stage=stage)
    eng = route.RouteEngine(ref["g"])
    buf = route.PinnedBuffer(nbytes + 64)
    canary(buf, nbytes + 64)
    mn, _ = eng.fill_triangle(ref["A"], buf, dispatch=True, lat16=lat16)
    assert eng.last_fill_code == (route.ENOEDGE if ref["noloop"] else route.OK) and ref["noloop"] == (na > 1)
    check_rows(route, ref, buf, lat16, range(na))
    assert mn == kept_min(ref["lat"], range(na))
    view = bytes_of(buf, nbytes + 64)
    assert np.all(view[nbytes:].view(np.uint64) == CAN64)
    assert stage is not None or stage_chunks(na, range(na), lat16, stage) == 1
    if lat16:
        check_pads(view[:nbytes], na)


# ---- c. lazily pinned memory in small chunks -----------------------------------------------

@pytest.mark.parametrize("lat16", [False, True])
@pytest.mark.parametrize("mode", ["plain", "stage", "world3", "world3kd", "regfail", "numpy"])
def test_lazy_chunks(route, oracle_mod, monkeypatch, mode, lat16):
    """SHD_ROUTE_HOST_CHUNK = 2 MiB, the grid over every vertex: the triangle spans 5 chunks
    (3 compact) and rows straddle the boundaries.  Allocated lazily and filled at once, without
    wait(): after wait() the bytes are the eager buffer's (which equals the oracle).  The same
    with the smallest stage, with three ranks in turn (after each, the rows nobody wrote yet
    are all-zero bytes: the workers' first touch; world3kd: under KD, whose seeded plan makes
    every row a piece of its own), with chunk 1 refused registration, and into a plain numpy
    array."""
    ref = reference(oracle_mod, "grid")
    A, na = ref["A"], ref["na"]
    lo, hi, nbytes = row_bytes(route, na, lat16)
    chunk = 2 * MIB
    assert (nbytes + chunk - 1) // chunk >= (3 if lat16 else 4)
    straddle = [i for i in range(na) if lo[i] // chunk != (hi[i] - 1) // chunk]
    assert len(straddle) >= 1 and all(lo[i] % chunk for i in straddle)
    sel = "kd" if mode == "world3kd" else "auto"
    knobs(monkeypatch, sel=sel)
    eng = route.RouteEngine(ref["g"])
    base, mn1, code1 = eager_fill(route, eng, ref, lat16)
    assert code1 == route.ENOEDGE
    check_rows(route, ref, NumpyBuffer(nbytes, base), lat16, range(na))    # the eager buffer against the oracle
    assert mn1 == kept_min(ref["lat"], range(na))
    knobs(monkeypatch, stage=1 if mode == "stage" else None, chunk=chunk, regfail=1 if mode == "regfail" else None, sel=sel)
    if mode == "numpy":
        buf = NumpyBuffer(nbytes)
        mn, _ = eng.fill_triangle(A, buf, dispatch=True, lat16=lat16)
        assert eng.last_fill_code == code1 and mn == mn1
        assert np.array_equal(buf.mem.view(np.uint8), base)
        return
    buf = route.PinnedBuffer(nbytes, lazy=True)
    view = bytes_of(buf, nbytes)
    if mode.startswith("world3"):
        written = np.zeros(nbytes, bool)
        for rank in range(3):
            plan = eng.plan(A, 3, rank)
            pos = [int(p) for p in plan.positions]
            plan.close()
            eng.fill_triangle(A, buf, world=3, rank=rank, dispatch=True, lat16=lat16)     # (rank 0: no wait() before)
            buf.wait()
            written |= owned_mask(route, na, lat16, pos)
            assert not view[~written].any()
            assert np.array_equal(view[written], base[written])
        assert written.all()
    else:
        mn, _ = eng.fill_triangle(A, buf, dispatch=True, lat16=lat16)
        assert eng.last_fill_code == code1 and mn == mn1
        buf.wait()
    assert np.array_equal(view, base)
    assert buf.unpinned() == (chunk if mode == "regfail" else 0)   # (the knob took effect: one 2 MiB chunk)


# ---- d. more than 4096 rows in one stage chunk ----------------------------------------------

@pytest.mark.parametrize("lat16", [False, True])
def test_more_than_4096_rows_in_a_chunk(route, oracle_mod, monkeypatch, lat16):
    """sized4097 over every vertex with the default stage: one chunk of 4097 rows, packed by
    4096 workgroups (row 4096 is the second turn of workgroup 0 in the grid-stride loop).  The
    fill runs whole; the oracle over all of A x A takes 15 s on a CPU, so the comparison is
    kept to every 7th row plus the last 10 (row 4096 among them), all their targets."""
    g = sg.get("sized4097")
    na = g.n
    rows = sorted(set(range(0, na, 7)) | set(range(na - 10, na)))
    ref = reference(oracle_mod, "sized4097", "all", rows=rows)
    assert na > 4096 and stage_chunks(na, range(na), lat16, None) == 1 and 4096 in rows
    _, _, nbytes = row_bytes(route, na, lat16)
    knobs(monkeypatch)
    eng = route.RouteEngine(g)
    assert eng.info["lat16"] == 1
    buf = route.PinnedBuffer(nbytes)
    canary(buf, nbytes)
    mn, _ = eng.fill_triangle(ref["A"], buf, dispatch=True, lat16=lat16)
    assert eng.last_fill_code == route.ENOEDGE
    lat, rel = read_triangle(route, buf, na, lat16)
    check_rows(route, ref, buf, lat16, rows, (lat, rel))
    view = bytes_of(buf, nbytes)
    if lat16:
        check_pads(view, na)
    else:
        assert not np.any(view.view(np.uint64) == CAN64)    # every pair of every row was written
    assert mn == np.nanmin(lat) <= kept_min(ref["lat"], rows)


# ---- e. the front end under the knobs -------------------------------------------------------

@pytest.mark.parametrize("lat16", ["0", "1"])
@pytest.mark.parametrize("name", ["ba100_attached", "ba120_vloss", "dir40"])
def test_front_end_under_the_knobs(route, monkeypatch, name, lat16):
    """Two contexts on one device, SHD_ROUTE_FILL_STAGE at its minimum and 2 MiB host chunks:
    every getter value over all attached pairs equals the golden eager table (as
    test_topology_gpu.test_cache_matches_golden_eager_table holds it; with vertex loss,
    reliability within REL_TOL of it) and the table of the same front end without the knobs."""
    from shadow_amd import topology
    from tests.test_topology_gpu import _small
    topology.load_library()
    g, z, p = _small(name)
    A = z[p + "attached"]
    tabs = []
    for stage, chunk in ((None, None), (1, 2 * MIB)):
        knobs(monkeypatch, stage=stage, chunk=chunk)
        monkeypatch.setenv("SHD_TOPOLOGY_LAT16", lat16)
        t = topology.Topology.from_graph(g, devices=(0, 0))
        t.attach_all(A)
        lat, rel = t.table(A)
        isd = np.array([[t.is_direct(a, b) for b in A] for a in A], bool)
        tabs.append((lat, rel, t.min_path_latency(), isd))
        t.close()
    lat, rel, mn, isd = tabs[1]
    assert np.array_equal(lat, z[p + "lat"])
    uq = z[p + "unique"]
    if g.vertex_packetloss is None:
        assert np.array_equal(rel[uq], z[p + "rel"][uq])
    else:
        np.testing.assert_allclose(rel[uq], z[p + "rel"][uq], rtol=REL_TOL, atol=0)
    assert mn == float(z[p + "min_latency"])
    assert np.array_equal(isd, z[p + "is_direct"])
    assert np.array_equal(lat, tabs[0][0]) and np.array_equal(rel, tabs[0][1]) and mn == tabs[0][2]
