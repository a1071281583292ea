"""ctypes binding of the HIP engine (shadow_amd/libshd_route.so, include/shd_route.h).

This is the same binding a maintainer would add on the reference side (see
INTEGRATION.md); Python is only the test/bench driver.  There is no CPU fallback:
if the HIP library is missing, importing the engine raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .graph import Graph

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SHD_ROUTE_LIB") or os.path.join(_HERE, "libshd_route.so")

OK = 0
EINVAL = -1
ENOMEM = -2
EDEVICE = -3
ENOEDGE = -4
EUNREACH = -5
EUNSUPPORTED = -6
DISPATCH = 0x1
PLAN_REUSE = 0x200  # shd_route.h SHD_ROUTE_PLAN_REUSE
REFRESH_ALL, REFRESH_MINE, REFRESH_JOBS = 0x1, 0x2, 0x4  # SHD_ROUTE_REFRESH_*
PAYLOAD_LAT16 = 0x1
FILL_LAT16 = 0x100
LOADS_ADD = 0x400  # shd_route.h SHD_ROUTE_LOADS_ADD
FOLD_SUM, FOLD_MIN, FOLD_MAX, FOLD_PROD = 0, 1, 2, 3  # SHD_ROUTE_FOLD_*
FOLD_MAX_N = 8
OUTAGE_HIT, OUTAGE_CUT, OUTAGE_SLOWER, OUTAGE_NSTAT = 0, 1, 2, 3  # SHD_ROUTE_OUTAGE_*
REPRICE_HIT, REPRICE_SLOWER, REPRICE_FASTER, REPRICE_NSTAT = 0, 1, 2, 3  # SHD_ROUTE_REPRICE_*
EDIT_HIT, EDIT_CUT, EDIT_SLOWER, EDIT_FASTER, EDIT_NSTAT = 0, 1, 2, 3, 4  # SHD_ROUTE_EDIT_*


class RouteError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: {strerror(code)} ({code})")


class _Graph(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int32), ("n_edges", C.c_int32),
        ("edge_src", C.c_void_p), ("edge_dst", C.c_void_p),
        ("edge_latency", C.c_void_p), ("edge_packetloss", C.c_void_p),
        ("vertex_packetloss", C.c_void_p),
        ("directed", C.c_int32), ("prefer_direct", C.c_int32),
    ]


class _Info(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("n_arcs", C.c_int32),
        ("is_complete", C.c_int32), ("directed", C.c_int32), ("prefer_direct", C.c_int32),
        ("integer_weights", C.c_int32), ("multigraph", C.c_int32), ("device", C.c_int32),
        ("lds_resident", C.c_int32), ("device_bytes", C.c_uint64), ("min_edge_latency", C.c_double),
        ("kernel", C.c_int32), ("dist_bound", C.c_int32), ("block", C.c_int32), ("reserved", C.c_int32),
        ("lat16", C.c_int32),
    ]


# one KDJob (sssp_delta.hpp): a 64-byte record of the planned launch's job array
JOB_DTYPE = np.dtype([("row", "<i4"), ("s", "<i4"), ("store", "<i4"), ("nseed", "<i4"), ("seed", "<i4", 3),
                      ("u", "<i4", 3), ("wr", "<i4", 3), ("rec", "<i4", 3)])
assert JOB_DTYPE.itemsize == 64


class _PlanInfo(C.Structure):
    _fields_ = [
        ("rows", C.c_int32), ("seeded", C.c_int32), ("launches", C.c_int32), ("levels", C.c_int32),
        ("roots", C.c_int32),
        ("helpers", C.c_int32), ("stored_rows", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32),
        ("store_bytes", C.c_uint64), ("delta", C.c_int32), ("pad_", C.c_int32),
    ]


# every symbol include/shd_route.h declares
EXPORTS = (
    "shd_route_create", "shd_route_destroy", "shd_route_get_info", "shd_route_strerror",
    "shd_route_rows", "shd_route_rows_async", "shd_route_sync", "shd_route_direct",
    "shd_route_self", "shd_route_min_reduce_async", "shd_route_fw_async",
    "shd_route_plan_create", "shd_route_plan_destroy", "shd_route_plan_get_info", "shd_route_plan_rows",
    "shd_route_rows_planned_async", "shd_route_fw_table_async", "shd_route_fw_rows_async",
    "shd_route_fill_triangle", "shd_route_host_alloc", "shd_route_host_free", "shd_route_tri_payload_async",
    "shd_route_kd_stats", "shd_route_host_alloc_lazy", "shd_route_host_wait",
    "shd_route_host_unpinned", "shd_route_plan_refresh_async", "shd_route_plan_landmarks",
    "shd_route_plan_bind_store", "shd_route_hops_async", "shd_route_hops", "shd_route_paths",
    "shd_route_plan_jobs", "shd_route_loads_async", "shd_route_loads", "shd_route_pair_loads",
    "shd_route_ties_async", "shd_route_ties",
    "shd_route_ecmp_loads_async", "shd_route_ecmp_loads", "shd_route_pair_ecmp_loads",
    "shd_route_fold_async", "shd_route_fold", "shd_route_pair_fold",
    "shd_route_loss_async", "shd_route_loss", "shd_route_pair_loss",
    "shd_route_outage_async", "shd_route_outage", "shd_route_pair_outage",
    "shd_route_reprice_async", "shd_route_reprice", "shd_route_pair_reprice",
    "shd_route_edit_async", "shd_route_edit", "shd_route_pair_edit",
)

_lib = None


def load_library():
    """Load libshd_route.so (fails loudly if the HIP build is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"HIP engine not built: {LIB_PATH} missing (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P, I32, I64, U32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    L.shd_route_strerror.restype = C.c_char_p
    L.shd_route_strerror.argtypes = [C.c_int]
    L.shd_route_create.restype = C.c_int
    L.shd_route_create.argtypes = [C.POINTER(P), C.POINTER(_Graph), C.c_int]
    L.shd_route_destroy.argtypes = [P]
    L.shd_route_get_info.restype = C.c_int
    L.shd_route_get_info.argtypes = [P, C.POINTER(_Info)]
    L.shd_route_rows.restype = C.c_int
    L.shd_route_rows.argtypes = [P, P, I32, P, I32, U32, P, P, P]
    L.shd_route_rows_async.restype = C.c_int
    L.shd_route_rows_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P]
    L.shd_route_sync.restype = C.c_int
    L.shd_route_sync.argtypes = [P, P]
    L.shd_route_direct.restype = C.c_int
    L.shd_route_direct.argtypes = [P, P, I32, P, I32, P, P, P]
    L.shd_route_self.restype = C.c_int
    L.shd_route_self.argtypes = [P, P, I32, P, P]
    L.shd_route_min_reduce_async.restype = C.c_int
    L.shd_route_min_reduce_async.argtypes = [P, P, I64, P, P]
    L.shd_route_fw_async.restype = C.c_int
    L.shd_route_fw_async.argtypes = [P, P, P]
    L.shd_route_fill_triangle.restype = C.c_int
    L.shd_route_fill_triangle.argtypes = [P, P, I32, I32, I32, U32, P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.shd_route_host_alloc.restype = P
    L.shd_route_host_alloc.argtypes = [C.c_size_t]
    L.shd_route_host_free.argtypes = [P]
    L.shd_route_host_alloc_lazy.restype = P
    L.shd_route_host_alloc_lazy.argtypes = [C.c_size_t]
    L.shd_route_host_wait.restype = C.c_int
    L.shd_route_host_wait.argtypes = [P]
    L.shd_route_host_unpinned.restype = C.c_int64
    L.shd_route_host_unpinned.argtypes = [P]
    L.shd_route_fw_table_async.restype = C.c_int
    L.shd_route_fw_table_async.argtypes = [P, P]
    L.shd_route_fw_rows_async.restype = C.c_int
    L.shd_route_fw_rows_async.argtypes = [P, P, I32, P, I32, I64, P, P, P, P]
    L.shd_route_tri_payload_async.restype = C.c_int
    L.shd_route_tri_payload_async.argtypes = [P, P, P, I64, P, P, I32, I32, U32, P, P, P]
    L.shd_route_plan_create.restype = C.c_int
    L.shd_route_plan_create.argtypes = [P, P, I32, I32, I32, C.POINTER(P)]
    L.shd_route_plan_destroy.argtypes = [P]
    L.shd_route_plan_get_info.restype = C.c_int
    L.shd_route_plan_get_info.argtypes = [P, C.POINTER(_PlanInfo)]
    L.shd_route_plan_rows.restype = C.c_int
    L.shd_route_plan_rows.argtypes = [P, P]
    L.shd_route_rows_planned_async.restype = C.c_int
    L.shd_route_rows_planned_async.argtypes = [P, P, P, I32, I64, U32, P, P, P, P]
    L.shd_route_plan_refresh_async.restype = C.c_int
    L.shd_route_plan_refresh_async.argtypes = [P, P, U32, P]
    L.shd_route_plan_landmarks.restype = C.c_int
    L.shd_route_plan_landmarks.argtypes = [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int64)]
    L.shd_route_plan_bind_store.restype = C.c_int
    L.shd_route_plan_bind_store.argtypes = [P, P, P, P]
    L.shd_route_plan_jobs.restype = C.c_int
    L.shd_route_plan_jobs.argtypes = [P, P, C.POINTER(C.c_int32), P, I64]
    L.shd_route_kd_stats.restype = C.c_int
    L.shd_route_kd_stats.argtypes = [P, P, I32]
    L.shd_route_hops_async.restype = C.c_int
    L.shd_route_hops_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P]
    L.shd_route_hops.restype = C.c_int
    L.shd_route_hops.argtypes = [P, P, I32, P, I32, U32, P, P]
    L.shd_route_paths.restype = C.c_int
    L.shd_route_paths.argtypes = [P, P, P, I64, U32, P, P, P, I64]
    L.shd_route_loads_async.restype = C.c_int
    L.shd_route_loads_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P, P]
    L.shd_route_loads.restype = C.c_int
    L.shd_route_loads.argtypes = [P, P, I32, P, I32, U32, P, P, P, P]
    L.shd_route_pair_loads.restype = C.c_int
    L.shd_route_pair_loads.argtypes = [P, P, P, P, I64, U32, P, P, P]
    L.shd_route_ties_async.restype = C.c_int
    L.shd_route_ties_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P]
    L.shd_route_ties.restype = C.c_int
    L.shd_route_ties.argtypes = [P, P, I32, P, I32, U32, P, P, P]
    L.shd_route_ecmp_loads_async.restype = C.c_int
    L.shd_route_ecmp_loads_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P, P]
    L.shd_route_ecmp_loads.restype = C.c_int
    L.shd_route_ecmp_loads.argtypes = [P, P, I32, P, I32, U32, P, P, P, P]
    L.shd_route_pair_ecmp_loads.restype = C.c_int
    L.shd_route_pair_ecmp_loads.argtypes = [P, P, P, P, I64, U32, P, P, P]
    L.shd_route_loss_async.restype = C.c_int
    L.shd_route_loss_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P, P, P, P]
    L.shd_route_loss.restype = C.c_int
    L.shd_route_loss.argtypes = [P, P, I32, P, I32, U32, P, P, P, P, P, P]
    L.shd_route_pair_loss.restype = C.c_int
    L.shd_route_pair_loss.argtypes = [P, P, P, P, I64, U32, P, P, P, P, P]
    L.shd_route_outage_async.restype = C.c_int
    L.shd_route_outage_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, I32, P, P, P, P, P]
    L.shd_route_outage.restype = C.c_int
    L.shd_route_outage.argtypes = [P, P, I32, P, I32, U32, P, P, P, I32, P, P, P, P]
    L.shd_route_pair_outage.restype = C.c_int
    L.shd_route_pair_outage.argtypes = [P, P, P, P, I64, U32, P, P, I32, P, P, P, P]
    L.shd_route_reprice_async.restype = C.c_int
    L.shd_route_reprice_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P, I32, P, P, P, P, P, P, P]
    L.shd_route_reprice.restype = C.c_int
    L.shd_route_reprice.argtypes = [P, P, I32, P, I32, U32, P, P, P, P, I32, P, P, P, P, P, P]
    L.shd_route_pair_reprice.restype = C.c_int
    L.shd_route_pair_reprice.argtypes = [P, P, P, P, I64, U32, P, P, P, I32, P, P, P, P, P, P]
    L.shd_route_edit_async.restype = C.c_int
    L.shd_route_edit_async.argtypes = [P, P, I32, P, I32, I64, U32, P, P, P, P, P, P, I32, P, P, P, P, P, P, P]
    L.shd_route_edit.restype = C.c_int
    L.shd_route_edit.argtypes = [P, P, I32, P, I32, U32, P, P, P, P, P, P, I32, P, P, P, P, P, P]
    L.shd_route_pair_edit.restype = C.c_int
    L.shd_route_pair_edit.argtypes = [P, P, P, P, I64, U32, P, P, P, P, P, I32, P, P, P, P, P, P]
    L.shd_route_fold_async.restype = C.c_int
    L.shd_route_fold_async.argtypes = [P, P, I32, P, I32, I64, U32, P, I32, P, P, I64, P]
    L.shd_route_fold.restype = C.c_int
    L.shd_route_fold.argtypes = [P, P, I32, P, I32, U32, P, I32, P, P]
    L.shd_route_pair_fold.restype = C.c_int
    L.shd_route_pair_fold.argtypes = [P, P, P, I64, U32, P, I32, P, P]
    _lib = L
    return L


def strerror(code: int) -> str:
    try:
        return load_library().shd_route_strerror(int(code)).decode()
    except RuntimeError:
        return f"error {code}"


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def pack_scenarios(scenarios):
    """(off int64, edge int32) of a list of id arrays or of an (off, edge) tuple of arrays."""
    if isinstance(scenarios, tuple):
        off = np.ascontiguousarray(scenarios[0], np.int64)
        edge = np.ascontiguousarray(scenarios[1], np.int32).reshape(-1)
    else:
        lists = [np.asarray(f, np.int32).reshape(-1) for f in scenarios]
        off = np.zeros(len(lists) + 1, np.int64)
        if lists:
            off[1:] = np.cumsum([len(f) for f in lists])
        edge = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return off, np.ascontiguousarray(edge)


def pack_reprice(scenarios):
    """(off int64, edge int32, lat float64) of a list of scenarios, each a list of (edge id, new
    latency) pairs, or of an (off, edge, lat) tuple of arrays."""
    if isinstance(scenarios, tuple):
        off = np.ascontiguousarray(scenarios[0], np.int64)
        edge = np.ascontiguousarray(scenarios[1], np.int32).reshape(-1)
        lat = np.ascontiguousarray(scenarios[2], np.float64).reshape(-1)
    else:
        lists = [list(f) for f in scenarios]
        off = np.zeros(len(lists) + 1, np.int64)
        if lists:
            off[1:] = np.cumsum([len(f) for f in lists])
        edge = np.array([e for f in lists for e, _ in f], np.int32)
        lat = np.array([w for f in lists for _, w in f], np.float64)
    if len(edge) != len(lat):
        raise ValueError("one new latency per listed edge id")
    return off, edge, lat


def pack_edits(scenarios):
    """(off int64, edge int32, a int32, b int32, lat float64) of a list of scenarios, each a list
    of items -- (edge id, latency) reprices that edge, (edge id, math.inf) removes it, (a, b,
    latency) adds a link between a and b (edge -1) -- or of an (off, edge, a, b, lat) tuple of
    arrays."""
    if isinstance(scenarios, tuple):
        off = np.ascontiguousarray(scenarios[0], np.int64)
        edge, a, b = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in scenarios[1:4])
        lat = np.ascontiguousarray(scenarios[4], np.float64).reshape(-1)
    else:
        lists = [[tuple(it) for it in f] for f in scenarios]
        if any(len(it) not in (2, 3) for f in lists for it in f):
            raise ValueError("an item is (edge id, latency) or (a, b, latency)")
        off = np.zeros(len(lists) + 1, np.int64)
        if lists:
            off[1:] = np.cumsum([len(f) for f in lists])
        items = [it for f in lists for it in f]
        edge = np.array([it[0] if len(it) == 2 else -1 for it in items], np.int32)
        a = np.array([0 if len(it) == 2 else it[0] for it in items], np.int32)
        b = np.array([0 if len(it) == 2 else it[1] for it in items], np.int32)
        lat = np.array([it[-1] for it in items], np.float64)
    if not len(edge) == len(a) == len(b) == len(lat):
        raise ValueError("one id, two ends and one latency per record")
    return off, edge, a, b, lat


def _check(rc, what):
    if rc != OK:
        raise RouteError(rc, what)


class RouteEngine:
    """One routing context on one GPU (one process per GPU)."""

    def __init__(self, g: Graph, device: int = 0):
        L = load_library()
        self.graph = g
        self._arrays = (
            np.ascontiguousarray(g.src, np.int32), np.ascontiguousarray(g.dst, np.int32),
            np.ascontiguousarray(g.latency, np.float64), np.ascontiguousarray(g.packetloss, np.float64),
            None if g.vertex_packetloss is None else np.ascontiguousarray(g.vertex_packetloss, np.float64),
        )
        s, d, lat, loss, vl = self._arrays
        desc = _Graph(int(g.n), len(s), s.ctypes.data, d.ctypes.data, lat.ctypes.data, loss.ctypes.data,
                      None if vl is None else vl.ctypes.data, int(bool(g.directed)), int(bool(g.prefer_direct)))
        h = C.c_void_p()
        _check(L.shd_route_create(C.byref(h), C.byref(desc), int(device)), "shd_route_create")
        self._h = h
        self.device = device
        # plans made on this context (a plan must be destroyed before its context: when both
        # become garbage together, the collector may finalise them in either order)
        import weakref
        self._plans = weakref.WeakSet()
        inf = _Info()
        _check(L.shd_route_get_info(self._h, C.byref(inf)), "shd_route_get_info")
        self.info = {k: getattr(inf, k) for k, _ in _Info._fields_}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            for p in list(getattr(self, "_plans", ())):
                p.close()
            load_library().shd_route_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-pointer API -----------------------------------------------------
    def rows(self, sources, targets, dispatch: bool = True):
        """shd_route_rows: (lat, rel, row_min).  A per-entry failure (a missing self-loop,
        an unreachable target) raises RouteError; ``err.partial`` then holds the arrays,
        every row written and the failed entries NaN."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        lat = np.empty((len(s), len(t))); rel = np.empty((len(s), len(t))); mn = np.empty(len(s))
        rc = load_library().shd_route_rows(self._h, _p(s), len(s), _p(t), len(t),
                                           DISPATCH if dispatch else 0, _p(lat), _p(rel), _p(mn))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_rows")
            err.partial = (lat, rel, mn)
            raise err
        _check(rc, "shd_route_rows")
        return lat, rel, mn

    def direct(self, sources, targets):
        """shd_route_direct: (lat, rel, row_min); a pair without an edge raises RouteError
        with ``err.partial`` = the arrays (that entry NaN), as rows()."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        lat = np.empty((len(s), len(t))); rel = np.empty((len(s), len(t))); mn = np.empty(len(s))
        rc = load_library().shd_route_direct(self._h, _p(s), len(s), _p(t), len(t), _p(lat), _p(rel), _p(mn))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_direct")
            err.partial = (lat, rel, mn)
            raise err
        _check(rc, "shd_route_direct")
        return lat, rel, mn

    def self_paths(self, vertices):
        v = np.ascontiguousarray(vertices, np.int32)
        lat = np.empty(len(v)); rel = np.empty(len(v))
        _check(load_library().shd_route_self(self._h, _p(v), len(v), _p(lat), _p(rel)), "shd_route_self")
        return lat, rel

    def hops(self, sources, targets, dispatch: bool = True):
        """shd_route_hops: (hops, row_max), the hop count of every (source, target) path
        (int32, -1 = failed entry) and each row's maximum.  A missing self-loop or an
        unreachable target raises RouteError; ``err.partial`` then holds the arrays."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        hops = np.empty((len(s), len(t)), np.int32); mx = np.empty(len(s), np.int32)
        rc = load_library().shd_route_hops(self._h, _p(s), len(s), _p(t), len(t),
                                           DISPATCH if dispatch else 0, _p(hops), _p(mx))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_hops")
            err.partial = (hops, mx)
            raise err
        _check(rc, "shd_route_hops")
        return hops, mx

    def ties(self, sources, targets, dispatch: bool = True):
        """shd_route_ties: (count, rel_lo, rel_hi) of every (source, target) entry: the number
        of shortest paths (uint64, saturating at 2^64 - 1) and the smallest and largest
        reliability any of them has.  Failed entries are (0, NaN, NaN); a missing self-loop or
        an unreachable target raises RouteError with ``err.partial`` = the arrays."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        cnt = np.empty((len(s), len(t)), np.uint64)
        lo = np.empty((len(s), len(t))); hi = np.empty((len(s), len(t)))
        rc = load_library().shd_route_ties(self._h, _p(s), len(s), _p(t), len(t),
                                           DISPATCH if dispatch else 0, _p(cnt), _p(lo), _p(hi))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_ties")
            err.partial = (cnt, lo, hi)
            raise err
        _check(rc, "shd_route_ties")
        return cnt, lo, hi

    def paths(self, pair_src, pair_tgt, dispatch: bool = True):
        """shd_route_paths: (off, vert, edge) of the explicit routes of the pairs, in the
        caller's order: vert[off[k]:off[k+1]] = pair k's vertices from source to target
        (empty for a failed pair), its edge ids edge[eoff[k]:eoff[k] + hops] with
        eoff = path_edge_offsets(off).  Makes the sizing call itself.  Failed pairs raise
        RouteError with ``err.partial`` = the arrays."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        if len(s) != len(t):
            raise ValueError("pair_src and pair_tgt differ in length")
        L = load_library()
        flags = DISPATCH if dispatch else 0
        off = np.zeros(len(s) + 1, np.int64)
        rc = L.shd_route_paths(self._h, _p(s), _p(t), len(s), flags, _p(off), None, None, 0)
        if rc != EINVAL or off[-1] <= 0:  # EINVAL with the sizes filled in: the buffers to bring
            if rc in (ENOEDGE, EUNREACH):
                err = RouteError(rc, "shd_route_paths")
                err.partial = (off, np.empty(0, np.int32), np.empty(0, np.int32))
                raise err
            _check(rc, "shd_route_paths")
            return off, np.empty(0, np.int32), np.empty(0, np.int32)
        cap = int(off[-1])
        vert = np.full(cap, -1, np.int32); edge = np.full(cap, -1, np.int32)
        rc = L.shd_route_paths(self._h, _p(s), _p(t), len(s), flags, _p(off), _p(vert), _p(edge), cap)
        edge = edge[: cap - int(np.count_nonzero(np.diff(off)))]
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_paths")
            err.partial = (off, vert, edge)
            raise err
        _check(rc, "shd_route_paths")
        return off, vert, edge

    def _loads_out(self, out):
        if out is not None:
            return out
        return (np.zeros(self.info["n_edges"], np.uint64), np.zeros(self.info["n_vertices"], np.uint64),
                np.zeros(1, np.uint64))

    def loads(self, sources, targets, weights=None, dispatch: bool = True, out=None, add: bool = False):
        """shd_route_loads: (edge_load, transit, unrouted) of the (source, target) block, uint64:
        the weight each edge id carries, the weight through each vertex as an intermediate hop,
        and the summed weight of the failed entries.  weights: (sources, targets) uint64, None =
        1 per entry.  out: the three arrays of an earlier call (unrouted as a 1-element array)
        to write into; add=True (SHD_ROUTE_LOADS_ADD) adds into them.  A missing self-loop or an
        unreachable target raises RouteError; ``err.partial`` then holds the results."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        if w is not None and w.shape != (len(s), len(t)):
            raise ValueError("weights must be (sources, targets)")
        el, tr, un = self._loads_out(out)
        flags = (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0)
        rc = load_library().shd_route_loads(self._h, _p(s), len(s), _p(t), len(t), flags, _p(w), _p(el), _p(tr), _p(un))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_loads")
            err.partial = (el, tr, int(un[0]))
            raise err
        _check(rc, "shd_route_loads")
        return el, tr, int(un[0])

    def pair_loads(self, pair_src, pair_tgt, pair_wt=None, dispatch: bool = True, out=None, add: bool = False):
        """shd_route_pair_loads: as loads() for a list of (source, target, weight) pairs in any
        order, repeats adding up (pair_wt None = 1 each)."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        w = None if pair_wt is None else np.ascontiguousarray(pair_wt, np.uint64)
        if len(s) != len(t) or (w is not None and len(w) != len(s)):
            raise ValueError("pair_src, pair_tgt and pair_wt differ in length")
        el, tr, un = self._loads_out(out)
        flags = (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0)
        rc = load_library().shd_route_pair_loads(self._h, _p(s), _p(t), _p(w), len(s), flags, _p(el), _p(tr), _p(un))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_loads")
            err.partial = (el, tr, int(un[0]))
            raise err
        _check(rc, "shd_route_pair_loads")
        return el, tr, int(un[0])

    def _ecmp_out(self, out):
        if out is not None:
            return out
        return (np.zeros(self.info["n_edges"], np.float64), np.zeros(self.info["n_vertices"], np.float64),
                np.zeros(1, np.uint64))

    def ecmp_loads(self, sources, targets, weights=None, dispatch: bool = True, out=None, add: bool = False):
        """shd_route_ecmp_loads: (edge_load, transit, unrouted) of the (source, target) block as
        loads(), with every entry's weight split evenly over all of its shortest paths:
        edge_load and transit are float64, unrouted stays an exact integer.  weights, out
        (float64, float64 and a 1-element uint64 array) and add as loads().  A missing self-loop
        or an unreachable target raises RouteError; ``err.partial`` then holds the results."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        if w is not None and w.shape != (len(s), len(t)):
            raise ValueError("weights must be (sources, targets)")
        el, tr, un = self._ecmp_out(out)
        flags = (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0)
        rc = load_library().shd_route_ecmp_loads(self._h, _p(s), len(s), _p(t), len(t), flags, _p(w), _p(el), _p(tr),
                                                 _p(un))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_ecmp_loads")
            err.partial = (el, tr, int(un[0]))
            raise err
        _check(rc, "shd_route_ecmp_loads")
        return el, tr, int(un[0])

    def pair_ecmp_loads(self, pair_src, pair_tgt, pair_wt=None, dispatch: bool = True, out=None, add: bool = False):
        """shd_route_pair_ecmp_loads: as ecmp_loads() for a list of (source, target, weight) pairs
        in any order, repeats adding up (pair_wt None = 1 each)."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        w = None if pair_wt is None else np.ascontiguousarray(pair_wt, np.uint64)
        if len(s) != len(t) or (w is not None and len(w) != len(s)):
            raise ValueError("pair_src, pair_tgt and pair_wt differ in length")
        el, tr, un = self._ecmp_out(out)
        flags = (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0)
        rc = load_library().shd_route_pair_ecmp_loads(self._h, _p(s), _p(t), _p(w), len(s), flags, _p(el), _p(tr),
                                                      _p(un))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_ecmp_loads")
            err.partial = (el, tr, int(un[0]))
            raise err
        _check(rc, "shd_route_pair_ecmp_loads")
        return el, tr, int(un[0])

    def _loss_out(self, out):
        if out is not None:
            return out
        m, n = self.info["n_edges"], self.info["n_vertices"]
        return (np.zeros(m, np.float64), np.zeros(m, np.float64), np.zeros(n, np.float64), np.zeros(n, np.float64),
                np.zeros(1, np.uint64))

    def loss(self, sources, targets, weights=None, dispatch: bool = True, out=None, add: bool = False):
        """shd_route_loss: (edge_reach, edge_drop, vertex_drop, delivered, unrouted) of the (source,
        target) block: the expected packets that reach each edge id, that each edge and each
        vertex drops and that arrive at each vertex (float64), and the summed weight of the
        failed entries (an exact integer).  weights as loads().  out: the five arrays of an
        earlier call (unrouted as a 1-element uint64 array), any of them None for an output not
        wanted; add=True (SHD_ROUTE_LOADS_ADD) adds into them.  A missing self-loop or an
        unreachable target raises RouteError; ``err.partial`` then holds the results."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        if w is not None and w.shape != (len(s), len(t)):
            raise ValueError("weights must be (sources, targets)")
        er, ed, vd, dl, un = self._loss_out(out)
        flags = (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0)
        rc = load_library().shd_route_loss(self._h, _p(s), len(s), _p(t), len(t), flags, _p(w), _p(er), _p(ed), _p(vd),
                                           _p(dl), _p(un))
        res = (er, ed, vd, dl, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_loss")
            err.partial = res
            raise err
        _check(rc, "shd_route_loss")
        return res

    def pair_loss(self, pair_src, pair_tgt, pair_wt=None, dispatch: bool = True, out=None, add: bool = False):
        """shd_route_pair_loss: as loss() for a list of (source, target, weight) pairs in any
        order, repeats adding up (pair_wt None = 1 each)."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        w = None if pair_wt is None else np.ascontiguousarray(pair_wt, np.uint64)
        if len(s) != len(t) or (w is not None and len(w) != len(s)):
            raise ValueError("pair_src, pair_tgt and pair_wt differ in length")
        er, ed, vd, dl, un = self._loss_out(out)
        flags = (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0)
        rc = load_library().shd_route_pair_loss(self._h, _p(s), _p(t), _p(w), len(s), flags, _p(er), _p(ed), _p(vd),
                                                _p(dl), _p(un))
        res = (er, ed, vd, dl, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_loss")
            err.partial = res
            raise err
        _check(rc, "shd_route_pair_loss")
        return res

    def _outage_out(self, nscn, entries, lat, out):
        if out is not None:
            return out
        return (np.zeros((nscn, OUTAGE_NSTAT), np.uint64), np.zeros(nscn, np.float64),
                np.full((nscn, *entries), np.nan) if lat else None, np.zeros(1, np.uint64))

    def outage(self, sources, targets, scenarios, weights=None, lat: bool = False, out=None):
        """shd_route_outage: (stats, max_add, lat, unrouted) of the (source, target) block under
        every scenario, each a set of failed edge ids: scenarios is a list of id arrays or an
        (off, edge) tuple of arrays.  stats is uint64 (scenarios, OUTAGE_NSTAT) with the columns
        OUTAGE_HIT, OUTAGE_CUT and OUTAGE_SLOWER, max_add float64 per scenario; lat=True also
        returns the new latencies (scenarios, sources, targets), NaN where cut or failed, else
        None.  Entries are judged without dispatch.  weights as loads().  out: the four arrays
        of an earlier call's shapes (unrouted a 1-element uint64 array), any of them None for an
        output not wanted.  A missing self-loop or an unreachable target in the whole graph raises
        RouteError; ``err.partial`` then holds the results."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        if w is not None and w.shape != (len(s), len(t)):
            raise ValueError("weights must be (sources, targets)")
        off, edge = pack_scenarios(scenarios)
        nscn = len(off) - 1
        st, mx, la, un = self._outage_out(nscn, (len(s), len(t)), lat, out)
        rc = load_library().shd_route_outage(self._h, _p(s), len(s), _p(t), len(t), 0, _p(w), _p(off), _p(edge), nscn,
                                             _p(st), _p(mx), _p(la), _p(un))
        res = (st, mx, la, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_outage")
            err.partial = res
            raise err
        _check(rc, "shd_route_outage")
        return res

    def pair_outage(self, pair_src, pair_tgt, scenarios, pair_wt=None, lat: bool = False, out=None):
        """shd_route_pair_outage: as outage() for a list of (source, target, weight) pairs in any
        order, repeats adding up (pair_wt None = 1 each); lat is (scenarios, pairs) in the
        caller's pair order."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        w = None if pair_wt is None else np.ascontiguousarray(pair_wt, np.uint64)
        if len(s) != len(t) or (w is not None and len(w) != len(s)):
            raise ValueError("pair_src, pair_tgt and pair_wt differ in length")
        off, edge = pack_scenarios(scenarios)
        nscn = len(off) - 1
        st, mx, la, un = self._outage_out(nscn, (len(s),), lat, out)
        rc = load_library().shd_route_pair_outage(self._h, _p(s), _p(t), _p(w), len(s), 0, _p(off), _p(edge), nscn,
                                                  _p(st), _p(mx), _p(la), _p(un))
        res = (st, mx, la, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_outage")
            err.partial = res
            raise err
        _check(rc, "shd_route_pair_outage")
        return res

    def _reprice_out(self, nscn, entries, lat, out):
        if out is not None:
            return out
        return (np.zeros((nscn, REPRICE_NSTAT), np.uint64), np.zeros(nscn, np.float64), np.zeros(nscn, np.float64),
                np.full(nscn, np.inf), np.full((nscn, *entries), np.nan) if lat else None, np.zeros(1, np.uint64))

    def reprice(self, sources, targets, scenarios, weights=None, lat: bool = False, out=None):
        """shd_route_reprice: (stats, max_add, max_gain, min_new, lat, unrouted) of the (source,
        target) block under every scenario, each a list of (edge id, new latency) pairs: scenarios
        is a list of such lists or an (off, edge, lat) tuple of arrays.  stats is uint64
        (scenarios, REPRICE_NSTAT) with the columns REPRICE_HIT, REPRICE_SLOWER and REPRICE_FASTER;
        max_add, max_gain and min_new (the smallest new latency, +inf without a routed entry) are
        float64 per scenario; lat=True also returns the new latencies (scenarios, sources,
        targets), NaN where the entry fails in the graph itself, else None.  Entries are judged
        without dispatch.  weights as loads().  out: the six arrays of an earlier call's shapes
        (unrouted a 1-element uint64 array), any of them None for an output not wanted.  A missing
        self-loop or an unreachable target raises RouteError; ``err.partial`` then holds the
        results."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        if w is not None and w.shape != (len(s), len(t)):
            raise ValueError("weights must be (sources, targets)")
        off, edge, nl = pack_reprice(scenarios)
        nscn = len(off) - 1
        st, mx, mg, mn, la, un = self._reprice_out(nscn, (len(s), len(t)), lat, out)
        rc = load_library().shd_route_reprice(self._h, _p(s), len(s), _p(t), len(t), 0, _p(w), _p(off), _p(edge), _p(nl),
                                              nscn, _p(st), _p(mx), _p(mg), _p(mn), _p(la), _p(un))
        res = (st, mx, mg, mn, la, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_reprice")
            err.partial = res
            raise err
        _check(rc, "shd_route_reprice")
        return res

    def pair_reprice(self, pair_src, pair_tgt, scenarios, pair_wt=None, lat: bool = False, out=None):
        """shd_route_pair_reprice: as reprice() for a list of (source, target, weight) pairs in any
        order, repeats adding up (pair_wt None = 1 each); lat is (scenarios, pairs) in the
        caller's pair order."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        w = None if pair_wt is None else np.ascontiguousarray(pair_wt, np.uint64)
        if len(s) != len(t) or (w is not None and len(w) != len(s)):
            raise ValueError("pair_src, pair_tgt and pair_wt differ in length")
        off, edge, nl = pack_reprice(scenarios)
        nscn = len(off) - 1
        st, mx, mg, mn, la, un = self._reprice_out(nscn, (len(s),), lat, out)
        rc = load_library().shd_route_pair_reprice(self._h, _p(s), _p(t), _p(w), len(s), 0, _p(off), _p(edge), _p(nl),
                                                   nscn, _p(st), _p(mx), _p(mg), _p(mn), _p(la), _p(un))
        res = (st, mx, mg, mn, la, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_reprice")
            err.partial = res
            raise err
        _check(rc, "shd_route_pair_reprice")
        return res

    def _edit_out(self, nscn, entries, lat, out):
        if out is not None:
            return out
        return (np.zeros((nscn, EDIT_NSTAT), np.uint64), np.zeros(nscn, np.float64), np.zeros(nscn, np.float64),
                np.full(nscn, np.inf), np.full((nscn, *entries), np.nan) if lat else None, np.zeros(1, np.uint64))

    def edit(self, sources, targets, scenarios, weights=None, lat: bool = False, out=None):
        """shd_route_edit: (stats, max_add, max_gain, min_new, lat, unrouted) of the (source,
        target) block under every scenario, each a list of items as pack_edits() takes them:
        (edge id, latency) reprices, (edge id, math.inf) removes, (a, b, latency) adds a link.
        stats is uint64 (scenarios, EDIT_NSTAT) with the columns EDIT_HIT, EDIT_CUT, EDIT_SLOWER
        and EDIT_FASTER; the rest as reprice(), lat NaN where the entry is cut or fails in the
        graph itself."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, np.uint64)
        if w is not None and w.shape != (len(s), len(t)):
            raise ValueError("weights must be (sources, targets)")
        off, edge, a, b, nl = pack_edits(scenarios)
        nscn = len(off) - 1
        st, mx, mg, mn, la, un = self._edit_out(nscn, (len(s), len(t)), lat, out)
        rc = load_library().shd_route_edit(self._h, _p(s), len(s), _p(t), len(t), 0, _p(w), _p(off), _p(edge), _p(a),
                                           _p(b), _p(nl), nscn, _p(st), _p(mx), _p(mg), _p(mn), _p(la), _p(un))
        res = (st, mx, mg, mn, la, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_edit")
            err.partial = res
            raise err
        _check(rc, "shd_route_edit")
        return res

    def pair_edit(self, pair_src, pair_tgt, scenarios, pair_wt=None, lat: bool = False, out=None):
        """shd_route_pair_edit: as edit() for a list of (source, target, weight) pairs in any
        order, repeats adding up (pair_wt None = 1 each); lat is (scenarios, pairs) in the
        caller's pair order."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        w = None if pair_wt is None else np.ascontiguousarray(pair_wt, np.uint64)
        if len(s) != len(t) or (w is not None and len(w) != len(s)):
            raise ValueError("pair_src, pair_tgt and pair_wt differ in length")
        off, edge, a, b, nl = pack_edits(scenarios)
        nscn = len(off) - 1
        st, mx, mg, mn, la, un = self._edit_out(nscn, (len(s),), lat, out)
        rc = load_library().shd_route_pair_edit(self._h, _p(s), _p(t), _p(w), len(s), 0, _p(off), _p(edge), _p(a), _p(b),
                                                _p(nl), nscn, _p(st), _p(mx), _p(mg), _p(mn), _p(la), _p(un))
        res = (st, mx, mg, mn, la, None if un is None else int(un[0]))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_edit")
            err.partial = res
            raise err
        _check(rc, "shd_route_pair_edit")
        return res

    def _fold_args(self, ops, values):
        o = np.ascontiguousarray(ops, np.int32).reshape(-1)
        v = np.ascontiguousarray(values, np.float64)
        if v.ndim == 1 and len(o) == 1:
            v = v.reshape(1, -1)
        if v.shape != (len(o), self.info["n_edges"]):
            raise ValueError("values must be (ops, n_edges)")
        return o, v

    def fold(self, sources, targets, ops, values, dispatch: bool = True):
        """shd_route_fold: the array (nf, sources, targets) of the folds ops[k] (FOLD_SUM, FOLD_MIN,
        FOLD_MAX, FOLD_PROD; at most FOLD_MAX_N) of the per-edge values[k] (float64, (nf, n_edges),
        no NaN) along every (source, target) path, each a left fold from the source.  A failed
        entry is NaN in every fold; a missing self-loop or an unreachable target raises
        RouteError with ``err.partial`` = the array."""
        s = np.ascontiguousarray(sources, np.int32)
        t = np.ascontiguousarray(targets, np.int32)
        o, v = self._fold_args(ops, values)
        out = np.empty((len(o), len(s), len(t)))
        rc = load_library().shd_route_fold(self._h, _p(s), len(s), _p(t), len(t), DISPATCH if dispatch else 0,
                                           _p(o), len(o), _p(v), _p(out))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_fold")
            err.partial = out
            raise err
        _check(rc, "shd_route_fold")
        return out

    def pair_fold(self, pair_src, pair_tgt, ops, values, dispatch: bool = True):
        """shd_route_pair_fold: as fold() for a list of (source, target) pairs in any order,
        repeats allowed: the array (nf, pairs) in the caller's pair order."""
        s = np.ascontiguousarray(pair_src, np.int32)
        t = np.ascontiguousarray(pair_tgt, np.int32)
        if len(s) != len(t):
            raise ValueError("pair_src and pair_tgt differ in length")
        o, v = self._fold_args(ops, values)
        out = np.empty((len(o), len(s)))
        rc = load_library().shd_route_pair_fold(self._h, _p(s), _p(t), len(s), DISPATCH if dispatch else 0,
                                                _p(o), len(o), _p(v), _p(out))
        if rc in (ENOEDGE, EUNREACH):
            err = RouteError(rc, "shd_route_pair_fold")
            err.partial = out
            raise err
        _check(rc, "shd_route_pair_fold")
        return out

    # -- device-pointer API (torch tensors as HBM plumbing) --------------------
    def fold_async(self, d_src, d_tgt, ops, d_val, d_out, stream=None, dispatch=True, ld=None, plane=None):
        """shd_route_fold_async over device tensors: int32 sources and targets, float64 values
        (len(ops) x n_edges) and outputs (len(ops) planes of `plane` elements, rows of stride
        ld); ops is a host sequence, read at call time."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        plane = ns * ld if plane is None else int(plane)
        o = np.ascontiguousarray(ops, np.int32).reshape(-1)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_fold_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, DISPATCH if dispatch else 0, _p(o), len(o), ptr(d_val),
            ptr(d_out), plane, C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_fold_async")

    def outage_async(self, d_src, d_tgt, d_wt, d_scn_off, d_scn_edge, d_stats, d_max_add, d_lat, d_unrouted,
                     stream=None, ld=None, flags=0):
        """shd_route_outage_async over device tensors: int32 sources and targets, 64-bit integer
        weights (None = 1 per entry), int64 scenario offsets (scenarios + 1) and int32 edge ids,
        each scenario ascending; 64-bit integer stats (scenarios x OUTAGE_NSTAT), float64
        max_add (scenarios) and lat (scenarios x sources x ld), a 64-bit integer unrouted (1
        element); any output may be None."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        nscn = 0 if d_scn_off is None else int(d_scn_off.numel()) - 1
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_outage_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, int(flags), ptr(d_wt), ptr(d_scn_off), ptr(d_scn_edge), nscn,
            ptr(d_stats), ptr(d_max_add), ptr(d_lat), ptr(d_unrouted), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_outage_async")

    def reprice_async(self, d_src, d_tgt, d_wt, d_scn_off, d_scn_edge, d_scn_lat, d_stats, d_max_add, d_max_gain,
                      d_min_new, d_lat, d_unrouted, stream=None, ld=None, flags=0):
        """shd_route_reprice_async over device tensors: as outage_async(), with float64 new
        latencies beside the edge ids (each scenario strictly ascending in its ids) and float64
        max_gain and min_new (scenarios) beside max_add; any output may be None."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        nscn = 0 if d_scn_off is None else int(d_scn_off.numel()) - 1
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_reprice_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, int(flags), ptr(d_wt), ptr(d_scn_off), ptr(d_scn_edge),
            ptr(d_scn_lat), nscn, ptr(d_stats), ptr(d_max_add), ptr(d_max_gain), ptr(d_min_new), ptr(d_lat),
            ptr(d_unrouted), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_reprice_async")

    def edit_async(self, d_src, d_tgt, d_wt, d_scn_off, d_scn_edge, d_scn_a, d_scn_b, d_scn_lat, d_stats, d_max_add,
                   d_max_gain, d_min_new, d_lat, d_unrouted, stream=None, ld=None, flags=0):
        """shd_route_edit_async over device tensors: as reprice_async(), with the int32 ends of
        the new links beside the edge ids (each scenario its new links, id -1, first and then its
        ids strictly ascending; +inf removes) and stats of EDIT_NSTAT columns; any output may be
        None."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        nscn = 0 if d_scn_off is None else int(d_scn_off.numel()) - 1
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_edit_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, int(flags), ptr(d_wt), ptr(d_scn_off), ptr(d_scn_edge),
            ptr(d_scn_a), ptr(d_scn_b), ptr(d_scn_lat), nscn, ptr(d_stats), ptr(d_max_add), ptr(d_max_gain),
            ptr(d_min_new), ptr(d_lat), ptr(d_unrouted), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_edit_async")

    def loss_async(self, d_src, d_tgt, d_wt, d_edge_reach, d_edge_drop, d_vertex_drop, d_delivered, d_unrouted,
                   stream=None, dispatch=True, ld=None, add=False):
        """shd_route_loss_async over device tensors: int32 sources and targets, 64-bit integer
        weights (None = 1 per entry), float64 edge_reach and edge_drop (n_edges elements),
        vertex_drop and delivered (n_vertices) and a 64-bit integer unrouted (1 element); any
        output may be None."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_loss_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0),
            ptr(d_wt), ptr(d_edge_reach), ptr(d_edge_drop), ptr(d_vertex_drop), ptr(d_delivered), ptr(d_unrouted),
            C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_loss_async")

    def ecmp_loads_async(self, d_src, d_tgt, d_wt, d_edge_load, d_transit, d_unrouted, stream=None, dispatch=True,
                         ld=None, add=False):
        """shd_route_ecmp_loads_async over device tensors: int32 sources and targets, 64-bit
        integer weights (None = 1 per entry), float64 edge loads and transit (n_edges,
        n_vertices elements) and a 64-bit integer unrouted (1 element); any output may be None."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_ecmp_loads_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0),
            ptr(d_wt), ptr(d_edge_load), ptr(d_transit), ptr(d_unrouted), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_ecmp_loads_async")

    def loads_async(self, d_src, d_tgt, d_wt, d_edge_load, d_transit, d_unrouted, stream=None, dispatch=True,
                    ld=None, add=False):
        """shd_route_loads_async over device tensors: int32 sources and targets, 64-bit weights
        (None = 1 per entry) and outputs (n_edges, n_vertices, 1 elements; any may be None; the
        values are unsigned, whatever 64-bit integer dtype carries them)."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_loads_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, (DISPATCH if dispatch else 0) | (LOADS_ADD if add else 0),
            ptr(d_wt), ptr(d_edge_load), ptr(d_transit), ptr(d_unrouted), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_loads_async")

    def hops_async(self, d_src, d_tgt, d_hops, d_rowmax, stream=None, dispatch=True, ld=None):
        """shd_route_hops_async over int32 device tensors (d_hops / d_rowmax may be None)."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_hops_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, DISPATCH if dispatch else 0,
            ptr(d_hops), ptr(d_rowmax), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_hops_async")

    def ties_async(self, d_src, d_tgt, d_count, d_rel_lo, d_rel_hi, stream=None, dispatch=True, ld=None):
        """shd_route_ties_async over device tensors: int32 sources and targets, a 64-bit integer
        tensor for the counts (unsigned values) and float64 bounds; any output may be None."""
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_ties_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, DISPATCH if dispatch else 0,
            ptr(d_count), ptr(d_rel_lo), ptr(d_rel_hi), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_ties_async")

    def rows_async(self, d_src, d_tgt, d_lat, d_rel, d_rowmin, stream=None, dispatch=True, ld=None):
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        rc = load_library().shd_route_rows_async(
            self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, DISPATCH if dispatch else 0,
            ptr(d_lat), ptr(d_rel), ptr(d_rowmin), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_rows_async")

    def sync(self, stream=None):
        _check(load_library().shd_route_sync(self._h, C.c_void_p(stream) if stream else None), "shd_route_sync")

    def min_reduce_async(self, d_vals, d_out, stream=None):
        rc = load_library().shd_route_min_reduce_async(self._h, C.c_void_p(d_vals.data_ptr()), int(d_vals.numel()),
                                                       C.c_void_p(d_out.data_ptr()),
                                                       C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_min_reduce_async")

    def fw_table_async(self, stream=None):
        """K4: the all-pairs u16 table by blocked min-plus Floyd-Warshall (kept on the device)."""
        _check(load_library().shd_route_fw_table_async(self._h, C.c_void_p(stream) if stream else None),
               "shd_route_fw_table_async")

    def fw_rows_async(self, d_src, d_tgt, d_lat, d_rel, d_rowmin, stream=None, ld=None):
        ns, nt = int(d_src.numel()), int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _check(load_library().shd_route_fw_rows_async(self._h, ptr(d_src), ns, ptr(d_tgt), nt, ld, ptr(d_lat),
                                                      ptr(d_rel), ptr(d_rowmin), C.c_void_p(stream) if stream else None),
               "shd_route_fw_rows_async")

    def fill_triangle(self, attached, out, world: int = 1, rank: int = 0, dispatch: bool = True,
                      lat16: bool = False):
        """shd_route_fill_triangle: this rank's rows of the front end's upper-triangle cache
        over the sorted `attached` vertices into `out` (a PinnedBuffer or any object with
        .ptr; 16 * na * (na + 1) / 2 bytes, or 64 * tri16_lines(na) with lat16: the compact
        layout).  Returns (min latency written, seconds); ``self.last_fill_code`` is the
        call's code: OK, or ENOEDGE / EUNREACH when entries failed (they are NaN / 0xFFFF)."""
        A = np.ascontiguousarray(attached, np.int32)
        mn, sec = C.c_double(), C.c_double()
        flags = (DISPATCH if dispatch else 0) | (FILL_LAT16 if lat16 else 0)
        rc = load_library().shd_route_fill_triangle(self._h, _p(A), len(A), int(world), int(rank),
                                                   flags, C.c_void_p(out.ptr),
                                                   C.byref(mn), C.byref(sec))
        self.last_fill_code = rc
        if rc not in (OK, ENOEDGE, EUNREACH):
            raise RouteError(rc, "shd_route_fill_triangle")
        return mn.value, sec.value

    def tri_payload_async(self, d_lat, d_rel, d_pos, d_off, na, out_lat, out_rel, lat16=True, stream=None, ld=None):
        """shd_route_tri_payload_async: the upper-triangle payload of this rank's rows
        (row r = attached position d_pos[r], targets j >= it) at offsets d_off - d_off[0]."""
        nrows = int(d_pos.numel())
        ld = int(d_lat.shape[1]) if ld is None else int(ld)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        _check(load_library().shd_route_tri_payload_async(
            self._h, ptr(d_lat), ptr(d_rel), ld, ptr(d_pos), ptr(d_off), nrows, int(na),
            PAYLOAD_LAT16 if lat16 else 0, ptr(out_lat), ptr(out_rel), C.c_void_p(stream) if stream else None),
            "shd_route_tri_payload_async")

    def kd_stats(self, reset: bool = True):
        """shd_route_kd_stats: the longest KD waits (s_sleep rounds) since the last reset:
        ring space, writer on an unwritten record, slice on an unwritten queue entry."""
        out = np.zeros(4, np.uint64)
        _check(load_library().shd_route_kd_stats(self._h, _p(out), int(reset)), "shd_route_kd_stats")
        return [int(x) for x in out[:3]]

    def plan(self, sources, world: int = 1, rank: int = 0) -> "RoutePlan":
        return RoutePlan(self, sources, world, rank)

    def fw_async(self, d_dist, stream=None):
        _check(load_library().shd_route_fw_async(self._h, C.c_void_p(d_dist.data_ptr()),
                                                 C.c_void_p(stream) if stream else None), "shd_route_fw_async")


class RoutePlan:
    """A seeded plan over a source list (shd_route_plan_*): this rank's output rows, the
    launches that compute them and the device row store.  Keep it for repeated fills."""

    def __init__(self, eng: RouteEngine, sources, world: int = 1, rank: int = 0):
        L = load_library()
        self.eng = eng
        src = np.ascontiguousarray(sources, np.int32)
        h = C.c_void_p()
        _check(L.shd_route_plan_create(eng._h, _p(src), len(src), int(world), int(rank), C.byref(h)),
               "shd_route_plan_create")
        self._h = h
        eng._plans.add(self)
        inf = _PlanInfo()
        _check(L.shd_route_plan_get_info(self._h, C.byref(inf)), "shd_route_plan_get_info")
        self.info = {k: getattr(inf, k) for k, _ in _PlanInfo._fields_ if not k.endswith("_")}
        pos = np.empty(max(1, self.info["rows"]), np.int32)
        _check(L.shd_route_plan_rows(self._h, _p(pos)), "shd_route_plan_rows")
        self.positions = pos[: self.info["rows"]]
        self.sources = src[self.positions]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load_library().shd_route_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows_async(self, d_tgt, d_lat, d_rel, d_rowmin, stream=None, dispatch=True, ld=None, reuse=False):
        """The plan's rows (shd_route_rows_planned_async).  A device-built landmark-only plan
        recomputes its landmark rows and job records first, unless reuse=True
        (SHD_ROUTE_PLAN_REUSE: the last refresh_async's, for timing the rows launch alone)."""
        nt = int(d_tgt.numel())
        ld = nt if ld is None else int(ld)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        flags = (DISPATCH if dispatch else 0) | (PLAN_REUSE if reuse else 0)
        rc = load_library().shd_route_rows_planned_async(
            self.eng._h, self._h, ptr(d_tgt), nt, ld, flags, ptr(d_lat), ptr(d_rel),
            ptr(d_rowmin), C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_rows_planned_async")

    def refresh_async(self, stream=None, what: int = 0):
        """The landmark rows, queue order and job records of a device-built landmark-only
        plan (shd_route_plan_refresh_async; what: REFRESH_ALL / REFRESH_MINE / REFRESH_JOBS,
        0 = all landmark rows + jobs); nothing for other plans."""
        rc = load_library().shd_route_plan_refresh_async(self.eng._h, self._h, int(what),
                                                         C.c_void_p(stream) if stream else None)
        _check(rc, "shd_route_plan_refresh_async")

    def landmarks(self):
        """The landmark store of a device-built landmark-only plan: {nland, first, count,
        row_stride} (this rank's share = slots [first, first + count)), or None."""
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        rc = load_library().shd_route_plan_landmarks(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        if rc == EUNSUPPORTED:
            return None
        _check(rc, "shd_route_plan_landmarks")
        return {"nland": a.value, "first": b.value, "count": c.value, "row_stride": d.value}

    def jobs(self):
        """shd_route_plan_jobs: the job records of a seeded plan in queue order, as a structured
        array (JOB_DTYPE: row, s, store, nseed, seed[3], u[3], wr[3], rec[3]); None for an
        unseeded plan.  Synchronises the device."""
        L = load_library()
        nj = C.c_int32()
        rc = L.shd_route_plan_jobs(self.eng._h, self._h, C.byref(nj), None, 0)
        if rc == EUNSUPPORTED:
            return None
        _check(rc, "shd_route_plan_jobs")
        out = np.zeros(nj.value, JOB_DTYPE)
        _check(L.shd_route_plan_jobs(self.eng._h, self._h, C.byref(nj), _p(out), out.nbytes), "shd_route_plan_jobs")
        return out

    def bind_store(self, d_drow, d_prow):
        """Move the landmark store into caller tensors (int16 / int32, nland x row_stride at
        least), which the plan keeps a reference to."""
        rc = load_library().shd_route_plan_bind_store(self.eng._h, self._h, C.c_void_p(d_drow.data_ptr()),
                                                      C.c_void_p(d_prow.data_ptr()))
        _check(rc, "shd_route_plan_bind_store")
        self._store = (d_drow, d_prow)


def path_edge_offsets(off) -> np.ndarray:
    """Where each pair's edge ids start in shd_route_paths' edge_out, from its off_out:
    off[k] minus the pairs before k that did not fail (each has one edge less than vertices)."""
    off = np.asarray(off, np.int64)
    ok = (np.diff(off) > 0).astype(np.int64)
    return off[:-1] - (np.cumsum(ok) - ok)


def tri16_lines(na: int, i: int | None = None) -> int:
    """shd_route_tri16_line: first 64-byte line of row i of the compact triangle (i = na, the
    default: the line count)."""
    na = int(na)
    i = na if i is None else int(i)
    pad = (i // 6) * 15 + sum((6 - (na - t) % 6) % 6 for t in range(i % 6))
    return (i * na - i * (i - 1) // 2 + pad) // 6


class PinnedBuffer:
    """Pinned host memory (shd_route_host_alloc) viewed as float64.  lazy: pinned in the
    background (shd_route_host_alloc_lazy); hand it to the device only through fill_triangle
    until wait() returns."""

    def __init__(self, nbytes: int, lazy: bool = False):
        self.nbytes = int(nbytes)
        name = "shd_route_host_alloc_lazy" if lazy else "shd_route_host_alloc"
        self.ptr = getattr(load_library(), name)(self.nbytes)
        if not self.ptr:
            raise RouteError(ENOMEM, name)

    def wait(self):
        _check(load_library().shd_route_host_wait(C.c_void_p(self.ptr)), "shd_route_host_wait")

    def unpinned(self) -> int:
        """Bytes of the buffer the runtime refused to register (pageable: still usable)."""
        n = int(load_library().shd_route_host_unpinned(C.c_void_p(self.ptr)))
        if n < 0:
            _check(n, "shd_route_host_unpinned")
        return n

    def array(self):
        buf = (C.c_double * (self.nbytes // 8)).from_address(self.ptr)
        return np.frombuffer(buf, dtype=np.float64)

    def close(self):
        if getattr(self, "ptr", None):
            load_library().shd_route_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
