"""ctypes binding of the C front end (shadow_amd/libshd_topology.so, include/shd_topology.h).

Mirrors Shadow's routing API (reference src/main/routing/topology.h:17-28) keyed by
vertex index: ``Topology.new(path)`` ~ ``topology_new``, ``get_latency`` ~
``topology_getLatency`` (-1 on error), ``get_reliability``, ``is_routable``,
``increment_path_packet_counter``; plus the runahead the cache implies.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from .graph import Graph
from .route import _Graph, load_library as _load_engine

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libshd_topology.so")

EXPORTS = (
    "shd_graphml_load", "shd_graphml_free", "shd_topology_new", "shd_topology_new_from_graph",
    "shd_topology_free", "shd_topology_vertex_count", "shd_topology_find_vertex",
    "shd_topology_attach_vertex", "shd_topology_attached_count", "shd_topology_get_latency",
    "shd_topology_get_reliability", "shd_topology_is_routable",
    "shd_topology_increment_path_packet_counter", "shd_topology_get_path_packet_count",
    "shd_topology_is_direct_path", "shd_topology_min_path_latency", "shd_topology_runahead_ns",
    "shd_topology_fill", "shd_topology_dump_paths", "shd_topology_triangle_bytes",
    "shd_attach_create", "shd_attach_find_vertex", "shd_attach_destroy", "shd_topology_attach",
    "shd_topology_get_path", "shd_topology_format_path", "shd_topology_dump_routes", "shd_topology_route_line",
    "shd_topology_link_loads", "shd_topology_ecmp_link_loads", "shd_topology_dump_link_loads", "shd_topology_link_line",
    "shd_topology_edge_count", "shd_topology_add_path_packets",
    "shd_topology_edge_jitter", "shd_topology_fold_pairs", "shd_topology_link_loss", "shd_topology_link_outage",
    "shd_topology_link_reprice",
    "shd_topology_link_edit",
    "shd_topology_tie_stats", "shd_topology_dump_ties", "shd_topology_tie_line", "shd_topology_tie_summary_line",
)

VATTRS = ("ip", "citycode", "countrycode", "geocode", "type")  # SHD_VATTR_* order
_NEXT_DOUBLE = C.CFUNCTYPE(C.c_double, C.c_void_p)


class _GraphML(C.Structure):
    _fields_ = [("graph", _Graph), ("vertex_ids", C.POINTER(C.c_char_p)),
                ("bandwidth_down", C.POINTER(C.c_double)), ("bandwidth_up", C.POINTER(C.c_double)),
                ("has_vertex_packetloss", C.c_int32), ("has_vertex_str", C.c_int32 * 5),
                ("vertex_str", C.POINTER(C.c_char_p) * 5), ("edge_jitter", C.POINTER(C.c_double))]


class TieStats(C.Structure):
    """shd_tie_stats_t (include/shd_topology.h)."""
    _fields_ = [("pairs", C.c_uint64), ("tied", C.c_uint64), ("sensitive", C.c_uint64), ("saturated", C.c_uint64),
                ("max_spread", C.c_double), ("worst_src", C.c_int32), ("worst_dst", C.c_int32),
                ("worst_count", C.c_uint64), ("worst_lo", C.c_double), ("worst_hi", C.c_double)]


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    _load_engine()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"front end not built: {LIB_PATH} missing (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P, I32, D = C.c_void_p, C.c_int32, C.c_double
    L.shd_graphml_load.restype = C.c_int
    L.shd_graphml_load.argtypes = [C.c_char_p, C.POINTER(_GraphML), C.c_char_p, C.c_size_t]
    L.shd_graphml_free.argtypes = [C.POINTER(_GraphML)]
    L.shd_topology_new.restype = P
    L.shd_topology_new.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int]
    L.shd_topology_new_from_graph.restype = P
    L.shd_topology_new_from_graph.argtypes = [C.POINTER(_Graph), C.POINTER(C.c_int), C.c_int]
    L.shd_topology_free.argtypes = [P]
    L.shd_topology_vertex_count.restype = I32
    L.shd_topology_vertex_count.argtypes = [P]
    L.shd_topology_edge_count.restype = I32
    L.shd_topology_edge_count.argtypes = [P]
    L.shd_topology_find_vertex.restype = I32
    L.shd_topology_find_vertex.argtypes = [P, C.c_char_p]
    L.shd_topology_attach_vertex.restype = C.c_int
    L.shd_topology_attach_vertex.argtypes = [P, I32]
    L.shd_topology_attached_count.restype = I32
    L.shd_topology_attached_count.argtypes = [P]
    for f in ("get_latency", "get_reliability"):
        getattr(L, "shd_topology_" + f).restype = D
        getattr(L, "shd_topology_" + f).argtypes = [P, I32, I32]
    L.shd_topology_is_routable.restype = C.c_int
    L.shd_topology_is_routable.argtypes = [P, I32, I32]
    L.shd_topology_is_direct_path.restype = C.c_int
    L.shd_topology_is_direct_path.argtypes = [P, I32, I32]
    L.shd_topology_increment_path_packet_counter.argtypes = [P, I32, I32]
    L.shd_topology_add_path_packets.argtypes = [P, I32, I32, C.c_uint64]
    L.shd_topology_get_path_packet_count.restype = C.c_uint64
    L.shd_topology_get_path_packet_count.argtypes = [P, I32, I32]
    L.shd_topology_min_path_latency.restype = D
    L.shd_topology_min_path_latency.argtypes = [P]
    L.shd_topology_runahead_ns.restype = C.c_uint64
    L.shd_topology_runahead_ns.argtypes = [P]
    L.shd_topology_fill.restype = C.c_int
    L.shd_topology_fill.argtypes = [P, C.POINTER(D)]
    L.shd_topology_triangle_bytes.restype = C.c_uint64
    L.shd_topology_triangle_bytes.argtypes = [P]
    L.shd_topology_dump_paths.restype = C.c_int
    L.shd_topology_dump_paths.argtypes = [P, P]
    L.shd_topology_get_path.restype = I32
    L.shd_topology_get_path.argtypes = [P, I32, I32, P, P, I32]
    L.shd_topology_format_path.restype = C.c_int
    L.shd_topology_format_path.argtypes = [P, I32, I32, C.c_char_p, C.c_size_t]
    L.shd_topology_dump_routes.restype = C.c_int
    L.shd_topology_dump_routes.argtypes = [P, P]
    L.shd_topology_route_line.restype = C.c_int64
    L.shd_topology_route_line.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), P, P, I32, P, P, D, D, C.c_int]
    L.shd_topology_link_loads.restype = C.c_int
    L.shd_topology_link_loads.argtypes = [P, P, P, C.POINTER(C.c_uint64)]
    L.shd_topology_ecmp_link_loads.restype = C.c_int
    L.shd_topology_ecmp_link_loads.argtypes = [P, P, P, C.POINTER(C.c_uint64)]
    L.shd_topology_link_outage.restype = C.c_int
    L.shd_topology_link_outage.argtypes = [P, P, P, C.c_int32, P, P, C.POINTER(C.c_uint64)]
    L.shd_topology_link_reprice.restype = C.c_int
    L.shd_topology_link_reprice.argtypes = [P, P, P, P, C.c_int32, P, P, P, P, C.POINTER(C.c_uint64)]
    L.shd_topology_link_edit.restype = C.c_int
    L.shd_topology_link_edit.argtypes = [P, P, P, P, P, P, C.c_int32, P, P, P, P, C.POINTER(C.c_uint64)]
    L.shd_topology_link_loss.restype = C.c_int
    L.shd_topology_link_loss.argtypes = [P, P, P, P, P, C.POINTER(C.c_uint64)]
    L.shd_topology_edge_jitter.restype = C.c_int
    L.shd_topology_edge_jitter.argtypes = [P, P]
    L.shd_topology_fold_pairs.restype = C.c_int
    L.shd_topology_fold_pairs.argtypes = [P, I32, P, P, P, C.c_int64, P]
    L.shd_topology_dump_link_loads.restype = C.c_int
    L.shd_topology_dump_link_loads.argtypes = [P, P]
    L.shd_topology_link_line.restype = C.c_int64
    L.shd_topology_link_line.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), P, I32, I32, I32, D, D,
                                         C.c_uint64, C.c_int]
    L.shd_topology_tie_stats.restype = C.c_int
    L.shd_topology_tie_stats.argtypes = [P, C.POINTER(TieStats)]
    L.shd_topology_dump_ties.restype = C.c_int
    L.shd_topology_dump_ties.argtypes = [P, P]
    L.shd_topology_tie_line.restype = C.c_int64
    L.shd_topology_tie_line.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), P, I32, I32, C.c_uint64, D, D,
                                        C.c_int]
    L.shd_topology_tie_summary_line.restype = C.c_int64
    L.shd_topology_tie_summary_line.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(TieStats),
                                                C.c_int]
    S = C.c_char_p
    L.shd_attach_create.restype = C.c_int
    L.shd_attach_create.argtypes = [C.POINTER(P), C.POINTER(_GraphML)]
    L.shd_attach_find_vertex.restype = I32
    L.shd_attach_find_vertex.argtypes = [P, _NEXT_DOUBLE, P, S, S, S, S, S]
    L.shd_attach_destroy.argtypes = [P]
    L.shd_topology_attach.restype = I32
    L.shd_topology_attach.argtypes = [P, _NEXT_DOUBLE, P, S, S, S, S, S, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
    _lib = L
    return L


def load_graphml(path: str) -> Graph:
    """Parse + validate graphml with the C loader (no GPU needed)."""
    L = load_library()
    out = _GraphML()
    err = C.create_string_buffer(512)
    rc = L.shd_graphml_load(path.encode(), C.byref(out), err, 512)
    if rc != 0:
        raise ValueError(err.value.decode() or f"graphml load failed ({rc})")
    try:
        g = out.graph
        n, m = g.n_vertices, g.n_edges
        arr = lambda p, cnt, ct, dt: np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(cnt,)).astype(dt).copy() \
            if cnt else np.zeros(0, dt)
        src = arr(g.edge_src, m, C.c_int32, np.int32)
        dst = arr(g.edge_dst, m, C.c_int32, np.int32)
        lat = arr(g.edge_latency, m, C.c_double, np.float64)
        loss = arr(g.edge_packetloss, m, C.c_double, np.float64)
        vl = arr(g.vertex_packetloss, n, C.c_double, np.float64) if g.vertex_packetloss else None
        ids = [out.vertex_ids[v].decode() for v in range(n)]
        return Graph(n=n, src=src, dst=dst, latency=lat, packetloss=loss, vertex_packetloss=vl,
                     directed=bool(g.directed), prefer_direct=bool(g.prefer_direct), ids=ids,
                     name=os.path.basename(path))
    finally:
        L.shd_graphml_free(C.byref(out))


def _enc(x):
    return None if x is None else x.encode()


class AttachIndex:
    """Host attachment over a graphml file (shd_attach_*, no GPU): the vertex a host
    with these hints joins, as _topology_findAttachmentVertex (topology.c:2245-2366).
    ``next_double`` is called where the reference draws random_nextDouble."""

    def __init__(self, path: str):
        L = load_library()
        self._gml = _GraphML()
        err = C.create_string_buffer(512)
        rc = L.shd_graphml_load(path.encode(), C.byref(self._gml), err, 512)
        if rc != 0:
            raise ValueError(err.value.decode() or f"graphml load failed ({rc})")
        self._h = C.c_void_p()
        rc = L.shd_attach_create(C.byref(self._h), C.byref(self._gml))
        if rc != 0:
            L.shd_graphml_free(C.byref(self._gml))
            raise ValueError(f"shd_attach_create failed ({rc})")
        self.n = self._gml.graph.n_vertices

    def vertex_attrs(self):
        """{name: [value or None per vertex] or None when the key is not declared}."""
        out = {}
        for a, name in enumerate(VATTRS):
            if not self._gml.has_vertex_str[a]:
                out[name] = None
                continue
            col = self._gml.vertex_str[a]
            out[name] = [None if col[v] is None else col[v].decode() for v in range(self.n)]
        return out

    def find(self, next_double=None, ip=None, citycode=None, countrycode=None, geocode=None, type=None) -> int:
        cb = _NEXT_DOUBLE((lambda _ctx: float(next_double()))) if next_double else _NEXT_DOUBLE()
        return int(load_library().shd_attach_find_vertex(self._h, cb, None, _enc(ip), _enc(citycode),
                                                          _enc(countrycode), _enc(geocode), _enc(type)))

    def close(self):
        if getattr(self, "_h", None):
            L = load_library()
            L.shd_attach_destroy(self._h)
            L.shd_graphml_free(C.byref(self._gml))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Topology:
    """topology.h over the GPU engine, vertex-indexed (one object per simulation)."""

    def __init__(self, handle, keep=None):
        if not handle:
            raise RuntimeError("topology creation failed")
        self._h = C.c_void_p(handle)
        self._keep = keep

    @classmethod
    def new(cls, path: str, devices=(0,)):
        L = load_library()
        dv = (C.c_int * len(devices))(*devices)
        return cls(L.shd_topology_new(path.encode(), dv, len(devices)))

    @classmethod
    def from_graph(cls, g: Graph, devices=(0,)):
        L = load_library()
        keep = (np.ascontiguousarray(g.src, np.int32), np.ascontiguousarray(g.dst, np.int32),
                np.ascontiguousarray(g.latency, np.float64), np.ascontiguousarray(g.packetloss, np.float64),
                None if g.vertex_packetloss is None else np.ascontiguousarray(g.vertex_packetloss, np.float64))
        s, d, lat, loss, vl = keep
        desc = _Graph(int(g.n), len(s), s.ctypes.data, d.ctypes.data, lat.ctypes.data, loss.ctypes.data,
                      None if vl is None else vl.ctypes.data, int(bool(g.directed)), int(bool(g.prefer_direct)))
        dv = (C.c_int * len(devices))(*devices)
        return cls(L.shd_topology_new_from_graph(C.byref(desc), dv, len(devices)), keep)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load_library().shd_topology_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def vertex_count(self):
        return load_library().shd_topology_vertex_count(self._h)

    def edge_count(self):
        return load_library().shd_topology_edge_count(self._h)

    def find_vertex(self, graphml_id: str) -> int:
        return load_library().shd_topology_find_vertex(self._h, graphml_id.encode())

    def attach(self, vertex: int):
        rc = load_library().shd_topology_attach_vertex(self._h, int(vertex))
        if rc:
            raise ValueError(f"attach failed ({rc})")

    def attach_host(self, next_double=None, ip=None, citycode=None, countrycode=None, geocode=None, type=None):
        """topology_attach (topology.c:2371-2439): (vertex, bandwidth down, bandwidth up)."""
        cb = _NEXT_DOUBLE((lambda _ctx: float(next_double()))) if next_double else _NEXT_DOUBLE()
        down, up = C.c_uint64(), C.c_uint64()
        v = load_library().shd_topology_attach(self._h, cb, None, _enc(ip), _enc(citycode), _enc(countrycode),
                                               _enc(geocode), _enc(type), C.byref(down), C.byref(up))
        if v < 0:
            raise ValueError("attach failed (topology not loaded from graphml?)")
        return int(v), int(down.value), int(up.value)

    def attached_count(self) -> int:
        return int(load_library().shd_topology_attached_count(self._h))

    def attach_all(self, vertices):
        for v in vertices:
            self.attach(v)

    def fill(self) -> float:
        t = C.c_double()
        rc = load_library().shd_topology_fill(self._h, C.byref(t))
        if rc:
            raise RuntimeError(f"fill failed ({rc})")
        return t.value

    def triangle_bytes(self) -> int:
        """Host bytes of the filled triangle (16 per pair, or the compact u16 layout)."""
        return int(load_library().shd_topology_triangle_bytes(self._h))

    def get_latency(self, s, d) -> float:
        return load_library().shd_topology_get_latency(self._h, int(s), int(d))

    def get_reliability(self, s, d) -> float:
        return load_library().shd_topology_get_reliability(self._h, int(s), int(d))

    def is_routable(self, s, d) -> bool:
        return bool(load_library().shd_topology_is_routable(self._h, int(s), int(d)))

    def is_direct(self, s, d) -> int:
        return load_library().shd_topology_is_direct_path(self._h, int(s), int(d))

    def increment_path_packet_counter(self, s, d):
        load_library().shd_topology_increment_path_packet_counter(self._h, int(s), int(d))

    def add_path_packets(self, s, d, packets: int):
        load_library().shd_topology_add_path_packets(self._h, int(s), int(d), int(packets))

    def packet_count(self, s, d) -> int:
        return int(load_library().shd_topology_get_path_packet_count(self._h, int(s), int(d)))

    def min_path_latency(self) -> float:
        return load_library().shd_topology_min_path_latency(self._h)

    def runahead_ns(self) -> int:
        return int(load_library().shd_topology_runahead_ns(self._h))

    def get_path(self, s, d):
        """shd_topology_get_path: (vert, edge) of the stored Path of {s, d}, from the lower
        attached vertex to the higher; None where the getters return -1."""
        L = load_library()
        cap = max(2, int(L.shd_topology_vertex_count(self._h)) + 1)
        vert = np.empty(cap, np.int32); edge = np.empty(cap, np.int32)
        h = L.shd_topology_get_path(self._h, int(s), int(d), C.c_void_p(vert.ctypes.data),
                                    C.c_void_p(edge.ctypes.data), cap)
        if h < 0:
            return None
        return vert[: h + 1].copy(), edge[:h].copy()

    def format_path(self, s, d):
        """shd_topology_format_path: the reference's "shortest path ..." line of the pair."""
        L = load_library()
        size = 4096
        while True:
            buf = C.create_string_buffer(size)
            k = L.shd_topology_format_path(self._h, int(s), int(d), buf, size)
            if k < 0:
                return None
            if k < size:
                return buf.value.decode()
            size = k + 1

    def _dump(self, name: str, path: str):
        libc = C.CDLL(None)
        libc.fopen.restype = C.c_void_p
        libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        libc.fclose.argtypes = [C.c_void_p]
        fp = libc.fopen(str(path).encode(), b"w")
        if not fp:
            raise OSError(f"cannot open {path}")
        try:
            rc = getattr(load_library(), "shd_topology_" + name)(self._h, fp)
        finally:
            libc.fclose(fp)
        if rc:
            raise RuntimeError(f"{name} failed ({rc})")

    def dump_routes(self, path: str):
        """shd_topology_dump_routes into the file `path`."""
        self._dump("dump_routes", path)

    def link_loads(self):
        """shd_topology_link_loads: (edge_packets, transit_packets, unrouted), the cached Paths'
        packet counters summed per edge id and per intermediate vertex, and the
        packets of self pairs stored as the path to self."""
        L = load_library()
        ep = np.zeros(int(L.shd_topology_edge_count(self._h)), np.uint64)
        tp = np.zeros(int(L.shd_topology_vertex_count(self._h)), np.uint64)
        un = C.c_uint64()
        rc = L.shd_topology_link_loads(self._h, C.c_void_p(ep.ctypes.data), C.c_void_p(tp.ctypes.data), C.byref(un))
        if rc:
            raise RuntimeError(f"link_loads failed ({rc})")
        return ep, tp, int(un.value)

    def ecmp_link_loads(self):
        """shd_topology_ecmp_link_loads: (edge_packets, transit_packets, unrouted) as link_loads(),
        every pair's packets split evenly over all of its shortest paths: float64 totals, an
        exact integer unrouted."""
        L = load_library()
        ep = np.zeros(int(L.shd_topology_edge_count(self._h)), np.float64)
        tp = np.zeros(int(L.shd_topology_vertex_count(self._h)), np.float64)
        un = C.c_uint64()
        rc = L.shd_topology_ecmp_link_loads(self._h, C.c_void_p(ep.ctypes.data), C.c_void_p(tp.ctypes.data),
                                            C.byref(un))
        if rc:
            raise RuntimeError(f"ecmp_link_loads failed ({rc})")
        return ep, tp, int(un.value)

    def link_loss(self):
        """shd_topology_link_loss: (edge_reach, edge_drop, vertex_drop, delivered, unrouted) of the
        cached Paths' packet counters, thinned out by the loss of every link and vertex on the
        route: float64 totals per edge id and per vertex, an exact integer unrouted.  A counter
        holds both directions of its pair; all of it is attributed in the stored orientation."""
        L = load_library()
        m, n = int(L.shd_topology_edge_count(self._h)), int(L.shd_topology_vertex_count(self._h))
        er, ed = np.zeros(m, np.float64), np.zeros(m, np.float64)
        vd, dl = np.zeros(n, np.float64), np.zeros(n, np.float64)
        un = C.c_uint64()
        rc = L.shd_topology_link_loss(self._h, *(C.c_void_p(a.ctypes.data) for a in (er, ed, vd, dl)), C.byref(un))
        if rc:
            raise RuntimeError(f"link_loss failed ({rc})")
        return er, ed, vd, dl, int(un.value)

    def link_outage(self, scenarios):
        """shd_topology_link_outage: (stats, max_add, unrouted) of the cached Paths' packet counters
        under every scenario of failed edge ids (a list of id arrays, or an (off, edge) tuple):
        uint64 stats (scenarios, 3) = the packets hit, cut off and slower, float64 max_add per
        scenario, an exact integer unrouted.  Raises RuntimeError with SHD_ROUTE_EUNSUPPORTED (-6)
        for a topology whose cache dispatches (a complete graph, or prefer-direct)."""
        from .route import pack_scenarios
        L = load_library()
        off, edge = pack_scenarios(scenarios)
        nscn = len(off) - 1
        st, mx = np.zeros((nscn, 3), np.uint64), np.zeros(nscn, np.float64)
        un = C.c_uint64()
        rc = L.shd_topology_link_outage(self._h, C.c_void_p(off.ctypes.data), C.c_void_p(edge.ctypes.data) if len(edge)
                                        else None, nscn, C.c_void_p(st.ctypes.data), C.c_void_p(mx.ctypes.data),
                                        C.byref(un))
        if rc:
            raise RuntimeError(f"link_outage failed ({rc})")
        return st, mx, int(un.value)

    def link_reprice(self, scenarios):
        """shd_topology_link_reprice: (stats, max_add, max_gain, min_new, unrouted) of the cached
        Paths' packet counters under every scenario of (edge id, new latency) pairs (a list of
        such lists, or an (off, edge, lat) tuple): uint64 stats (scenarios, 3) = the packets hit,
        slower and faster, float64 max_add, max_gain and min_new per scenario, an exact integer
        unrouted.  Raises RuntimeError with SHD_ROUTE_EUNSUPPORTED (-6) for a topology whose cache
        dispatches (a complete graph, or prefer-direct)."""
        from .route import pack_reprice
        L = load_library()
        off, edge, nl = pack_reprice(scenarios)
        nscn = len(off) - 1
        st = np.zeros((nscn, 3), np.uint64)
        mx, mg, mn = np.zeros(nscn, np.float64), np.zeros(nscn, np.float64), np.full(nscn, np.inf)
        un = C.c_uint64()
        vp = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
        rc = L.shd_topology_link_reprice(self._h, C.c_void_p(off.ctypes.data), vp(edge), vp(nl), nscn,
                                         C.c_void_p(st.ctypes.data), C.c_void_p(mx.ctypes.data),
                                         C.c_void_p(mg.ctypes.data), C.c_void_p(mn.ctypes.data), C.byref(un))
        if rc:
            raise RuntimeError(f"link_reprice failed ({rc})")
        return st, mx, mg, mn, int(un.value)

    def link_edit(self, scenarios):
        """shd_topology_link_edit: (stats, max_add, max_gain, min_new, unrouted) of the cached
        Paths' packet counters under every scenario of items as route.pack_edits() takes them --
        (edge id, latency) reprices, (edge id, math.inf) removes, (a, b, latency) adds a link --
        or an (off, edge, a, b, lat) tuple: uint64 stats (scenarios, 4) = the packets hit, cut,
        slower and faster, the rest as link_reprice().  Raises RuntimeError with
        SHD_ROUTE_EUNSUPPORTED (-6) for a topology whose cache dispatches."""
        from .route import pack_edits
        L = load_library()
        off, edge, a, b, nl = pack_edits(scenarios)
        nscn = len(off) - 1
        st = np.zeros((nscn, 4), np.uint64)
        mx, mg, mn = np.zeros(nscn, np.float64), np.zeros(nscn, np.float64), np.full(nscn, np.inf)
        un = C.c_uint64()
        vp = lambda x: C.c_void_p(x.ctypes.data) if len(x) else None
        rc = L.shd_topology_link_edit(self._h, C.c_void_p(off.ctypes.data), vp(edge), vp(a), vp(b), vp(nl), nscn,
                                      C.c_void_p(st.ctypes.data), C.c_void_p(mx.ctypes.data),
                                      C.c_void_p(mg.ctypes.data), C.c_void_p(mn.ctypes.data), C.byref(un))
        if rc:
            raise RuntimeError(f"link_edit failed ({rc})")
        return st, mx, mg, mn, int(un.value)

    def edge_jitter(self):
        """shd_topology_edge_jitter: the graphml's jitter edge attribute per edge id (NaN where
        an edge has none), or None for a topology without the key."""
        L = load_library()
        out = np.empty(int(L.shd_topology_edge_count(self._h)), np.float64)
        rc = L.shd_topology_edge_jitter(self._h, C.c_void_p(out.ctypes.data))
        if rc == -6:  # SHD_ROUTE_EUNSUPPORTED
            return None
        if rc:
            raise RuntimeError(f"edge_jitter failed ({rc})")
        return out

    def fold_pairs(self, op, values, src, dst):
        """shd_topology_fold_pairs: the fold `op` (route.FOLD_*) of the per-edge `values` along the
        route of each pair's stored Path, NaN for the pairs the getters reject and for self
        pairs stored as the path to self."""
        L = load_library()
        v = np.ascontiguousarray(values, np.float64)
        s = np.ascontiguousarray(src, np.int32)
        d = np.ascontiguousarray(dst, np.int32)
        if len(v) != int(L.shd_topology_edge_count(self._h)) or len(s) != len(d):
            raise ValueError("values must have one element per edge, src and dst one length")
        out = np.empty(len(s), np.float64)
        rc = L.shd_topology_fold_pairs(self._h, int(op), C.c_void_p(v.ctypes.data), C.c_void_p(s.ctypes.data),
                                       C.c_void_p(d.ctypes.data), len(s), C.c_void_p(out.ctypes.data))
        if rc:
            raise RuntimeError(f"fold_pairs failed ({rc})")
        return out

    def dump_link_loads(self, path: str):
        """shd_topology_dump_link_loads into the file `path`: one line per edge that carried
        packets."""
        self._dump("dump_link_loads", path)

    def tie_stats(self) -> dict:
        """shd_topology_tie_stats over the stored off-diagonal pairs: {pairs, tied, sensitive,
        saturated, max_spread, worst_src, worst_dst, worst_count, worst_lo, worst_hi}."""
        st = TieStats()
        rc = load_library().shd_topology_tie_stats(self._h, C.byref(st))
        if rc:
            raise RuntimeError(f"tie_stats failed ({rc})")
        return {k: getattr(st, k) for k, _ in TieStats._fields_}

    def dump_ties(self, path: str):
        """shd_topology_dump_ties into the file `path`: one line per pair whose reliability
        depends on the tie rule, then the summary line."""
        self._dump("dump_ties", path)

    def table(self, vertices):
        """Dense lookup(i, j) table (lat, rel) for a vertex list, via the public getters."""
        k = len(vertices)
        lat = np.empty((k, k)); rel = np.empty((k, k))
        L = load_library()
        for a, s in enumerate(vertices):
            for b, d in enumerate(vertices):
                lat[a, b] = L.shd_topology_get_latency(self._h, int(s), int(d))
                rel[a, b] = L.shd_topology_get_reliability(self._h, int(s), int(d))
        return lat, rel
