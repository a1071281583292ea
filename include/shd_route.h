/*
 * shd_route.h -- C-ABI of the MI355X-native topology routing engine.
 *
 * This is the boundary that replaces the igraph-backed path computation inside
 * Shadow 1.14's src/main/routing/topology.c (mckerrigan/shadow).  Shadow keeps
 * its public routing API unchanged (topology.h:17-28); its topology.c front end
 * calls this module instead of igraph for every number that ends up in a Path
 * (path.c:13-21: latency, reliability).  Plain C types only; no HIP/torch types
 * in any signature.  One context per GPU; contexts are not re-entrant, and a context
 * (with its plans) runs one rows launch at a time: the launches of shd_route_rows_async
 * and shd_route_rows_planned_async share the context's work-queue counter and
 * per-workgroup scratch, so two of them must not be in flight together (enqueue them
 * on one stream, or synchronise in between).  The path hops calls (shd_route_hops*,
 * shd_route_paths) and the link loads calls (shd_route_loads*, shd_route_pair_loads) run a
 * rows launch inside and fall under the same rule, and so do the tie envelope calls
 * (shd_route_ties*), the ECMP link loads calls (shd_route_ecmp_loads*,
 * shd_route_pair_ecmp_loads), the path fold calls (shd_route_fold*, shd_route_pair_fold),
 * the link loss calls (shd_route_loss*, shd_route_pair_loss), the link outage calls
 * (shd_route_outage*, shd_route_pair_outage), the link repricing calls (shd_route_reprice*,
 * shd_route_pair_reprice) and the link edit calls (shd_route_edit*, shd_route_pair_edit).
 *
 * Several contexts may be alive in one process, on one device or on several, each used as
 * above; creating, using and destroying one never changes what another computes.  (A context
 * sets the dynamic-LDS limit of its kernel functions to its own size when it is created, or at
 * its first hops / ties / K4 call; the limit belongs to the function, so a later, smaller context
 * lowers it.  The ROCm runtime this was tried on (gfx950) does not hold a launch to that
 * attribute -- a launch of up to the 160 KiB the device has goes through whatever the last
 * value was -- and tests/test_contexts_gpu.py keeps pairs of contexts that ask for 3 to over
 * 100 times different amounts, up to the full 160 KiB, alive together for every such kernel.)
 * shd_route_destroy frees device memory, which waits for the device: it may block while other
 * contexts' work is queued, and that work is not disturbed.
 *
 * Stream order of the *_async calls.  Everything such a call does on the device -- its
 * kernels, the zeroing of its counters, flags and outputs, the parking of the error word --
 * is enqueued on the caller's stream, and the call reads its device inputs only there:
 * inputs written by earlier work of the same stream are seen, and calls of one context may be
 * chained on one stream without a host synchronisation (any stream, the non-blocking ones
 * included; tests/test_stream_gpu.py).  In its steady state no *_async call waits for the
 * device.  The calls that may block the host, and when:
 *   first use      shd_route_rows_async with SHD_ROUTE_DISPATCH on a complete graph,
 *                  shd_route_fw_table_async (the dense tables, built on the host and copied);
 *                  the hops, loads, folds, ties and ECMP loads calls (their in-CSR with edge ids; the
 *                  ties and ECMP loads calls also their per-arc reliabilities and out-CSR, the
 *                  ECMP loads calls the out-arcs' edge ids; the loss calls also their per-edge
 *                  and per-vertex loss columns, the outage calls the edges' ends and latencies
 *                  and the self-loop lists, the repricing calls what the outage and the ECMP
 *                  loads calls build, the edit calls what the repricing calls build); all once
 *                  per context
 *   scratch growth a call that needs more scratch than the context holds frees the old block
 *                  (which waits for the device) and allocates: shd_route_rows_async under KB
 *                  without fused path attributes and shd_route_fw_rows_async when ns grows,
 *                  the hops, loads, folds, ties and ECMP loads calls when their source chunk
 *                  grows (the loss, outage and repricing calls follow the loads calls),
 *                  shd_route_loads_async, shd_route_fold_async, shd_route_ties_async,
 *                  shd_route_ecmp_loads_async, shd_route_loss_async, shd_route_outage_async and
 *                  shd_route_reprice_async in their HBM forms when the slices grow (those
 *                  synchronise the stream); shd_route_edit_async follows shd_route_reprice_async
 *                  in both
 * A first call with the largest sizes takes both out of the way.
 * Capture: after such a first call, shd_route_rows_async (every kernel),
 * shd_route_rows_planned_async (with and without SHD_ROUTE_PLAN_REUSE),
 * shd_route_plan_refresh_async and shd_route_min_reduce_async enqueue only kernels and
 * memsets and can be captured into a graph (hipStreamBeginCapture on the stream they are
 * given); inputs are read when the graph runs, so a replay sees what its buffers hold then.
 * A call that would grow scratch or build tables must not be made while capturing; the
 * blocking calls and shd_route_sync are not capturable.
 *
 * Reference interface each entry point replaces (file:line in the reference):
 *   shd_route_create   <- _topology_loadGraph/_topology_checkGraph/_topology_extractEdgeWeights
 *                         (topology.c:371-399, 1187-1246): graph in, validated, resident
 *   shd_route_rows     <- _topology_computeSourcePaths (topology.c:1655-1875) =
 *                         igraph_get_shortest_paths_dijkstra (topology.c:1756) +
 *                         _topology_computePathProperties (topology.c:1407-1523),
 *                         batched over many sources; with SHD_ROUTE_DISPATCH also the
 *                         direct-path dispatch of _topology_getPathEntry (topology.c:2019-2031)
 *                         and _topology_lookupDirectPath (topology.c:1877-1927)
 *   shd_route_hops, shd_route_paths <- the path itself: the vertex sequence igraph returns
 *                         (topology.c:1756) and the per-hop walk that logs it
 *                         (topology.c:1449, 1502-1503, 1829-1844)
 *   shd_route_direct   <- _topology_lookupDirectPath (topology.c:1877-1927) for many pairs
 *   shd_route_self     <- _topology_computeShortestPathToSelf (topology.c:1545-1653)
 *   shd_route_min_reduce <- minimumPathLatency tracking (topology.c:1374-1385)
 *   shd_route_fw       <- (no reference equivalent; dense all-pairs alternative)
 *   shd_route_loads, shd_route_pair_loads <- (no reference equivalent; per-link and
 *                         per-router traffic of the chosen paths)
 *   shd_route_ties     <- (no reference equivalent; how many shortest paths tie and how far
 *                         any tie rule, igraph's heap order included, can move reliability)
 *   shd_route_ecmp_loads, shd_route_pair_ecmp_loads <- (no reference equivalent; per-link and
 *                         per-router traffic split evenly over all tied shortest paths)
 *   shd_route_fold, shd_route_pair_fold <- (no reference equivalent; any per-link quantity
 *                         folded along the chosen paths, e.g. the jitter edge attribute the
 *                         reference validates and drops, topology.c:1105-1114)
 *   shd_route_loss, shd_route_pair_loss <- (no reference equivalent; the reference drops a
 *                         packet with one end-to-end coin flip on the Path's reliability and
 *                         cannot say on which link or router it was lost)
 *   shd_route_outage, shd_route_pair_outage, shd_route_reprice, shd_route_pair_reprice <- (no
 *                         reference equivalent; what-if scenarios that remove links or change
 *                         their latencies)
 *   shd_route_edit, shd_route_pair_edit <- (no reference equivalent; what-if scenarios that
 *                         remove links, change their latencies and add links in one step)
 *
 * Semantics of one (s,t) entry are exactly the Path the reference would cache:
 *   t != s : lat = 0.0 + sum of edge latencies along the chosen shortest path, summed
 *            from s (bit-exact: any relaxation order reaches the same left-fold minimum);
 *            rel = ((1.0*f_s)*f_t) * prod(1 - loss_e) with absent vertex factors skipped.
 *            The engine multiplies f_t last, so rel is bit-exact whenever f_t is absent
 *            or 1.0 and within a few ulp otherwise.
 *   t == s : the batch self-loop entry (path [s]): lat = w_ss, rel = (1.0*f_s)*r_ss;
 *            SHD_ROUTE_ENOEDGE if s has no self-loop (topology.c:1488-1495).
 * Ties between equal-latency paths are broken deterministically: the parent of v is
 * the tight in-arc (u->v) with the smallest (dist[u], u, edge id).  Latency never
 * depends on ties; reliability matches igraph wherever the shortest path is unique.
 */
#ifndef SHD_ROUTE_H
#define SHD_ROUTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes: 0 = success, negative = failure (topology.c maps them to critical()) */
#define SHD_ROUTE_OK 0
#define SHD_ROUTE_EINVAL (-1)       /* bad argument / graph fails topology.c validation */
#define SHD_ROUTE_ENOMEM (-2)       /* host or device allocation failed */
#define SHD_ROUTE_EDEVICE (-3)      /* HIP runtime error */
#define SHD_ROUTE_ENOEDGE (-4)      /* a hop has no edge (missing self-loop; topology.c:1488) */
#define SHD_ROUTE_EUNREACH (-5)     /* a target is unreachable (graph not strongly connected) */
#define SHD_ROUTE_EUNSUPPORTED (-6) /* request outside what this build supports */

/* flags for shd_route_rows */
#define SHD_ROUTE_DISPATCH 0x1u /* apply topology.c:2019 dispatch: complete graph -> direct,
                                   prefer-direct && adjacent -> direct, else source paths */

typedef struct shd_route shd_route_t;

/* A topology as igraph holds it after igraph_read_graph_graphml: vertices and edges
 * numbered in graphml document order.  Arrays are read during shd_route_create only. */
typedef struct shd_graph {
    int32_t n_vertices;
    int32_t n_edges;
    const int32_t* edge_src;          /* [n_edges] */
    const int32_t* edge_dst;          /* [n_edges] */
    const double* edge_latency;       /* [n_edges] ms, > 0        (topology.c:1070); no latency so small
                                       * that a distance could absorb it: see below */
    const double* edge_packetloss;    /* [n_edges] in [0,1]       (topology.c:1090) */
    const double* vertex_packetloss;  /* [n_vertices] or NULL; NaN = absent (topology.c:330-347) */
    int32_t directed;                 /* graphml edgedefault="directed" */
    int32_t prefer_direct;            /* graph attribute preferdirectpaths (topology.c:761-790) */
} shd_graph_t;
/* Absorbed latencies.  Every call takes fl(d[u] + w) > d[u] for granted: an arc u -> v is on a
 * shortest path exactly when d[u] + w == d[v] in f64, and those arcs must form a DAG.  With
 * min_w and max_w the smallest and the largest latency over the edges that are no self-loops,
 * shd_route_create refuses a graph with min_w <= (n_vertices - 1) * max_w * 2^-52 with
 * SHD_ROUTE_EUNSUPPORTED, from its host validation, before it touches the device.  (No distance
 * exceeds (n - 1) max_w (1 + 2^-53)^n, ulp(d) <= d 2^-52, and absorption needs w <= ulp(d) / 2:
 * the factor of two left over covers the rounding growth of the fold.  50,000 vertices with
 * latencies up to 250 ms: latencies of 3e-9 ms and below are refused.) */

typedef struct shd_route_info {
    int32_t n_vertices;
    int32_t n_edges;
    int32_t n_arcs;          /* CSR arcs used by SSSP (self-loops excluded) */
    int32_t is_complete;     /* topology.c:450-552 */
    int32_t directed;
    int32_t prefer_direct;
    int32_t integer_weights; /* every latency integral and path sums exact in u32 */
    int32_t multigraph;      /* parallel edges present (SURVEY hazard H3) */
    int32_t device;
    int32_t lds_resident;    /* per-source state fits the 160 KiB LDS (KF above ~12k vertices: 0, KFH) */
    uint64_t device_bytes;   /* resident graph bytes */
    double min_edge_latency;
    int32_t kernel;          /* SSSP kernel: 0 = generic f64, 1 = integer K32 (LDS keys), 2 = KB/KBF
                              * (8 sources per workgroup, C2-class), 4 = KD (delta-stepping, u16
                              * distances, seeded plans), 5 = KF (f64 delta-stepping in LDS: the
                              * fractional-latency path; with lds_resident 0 its KFH form, vertex
                              * state in HBM, up to 65535 vertices); 3 = K16 in diagnostic builds only */
    int32_t dist_bound;      /* K32: proven bound on every shortest-path latency (ms) */
    int32_t block;           /* threads per workgroup of the SSSP kernel */
    int32_t reserved;        /* KD: bucket width delta; KB: 1 when path attributes are fused; KF:
                              * the packed arcs' decimal scale (latency = k / scale, 4 bytes per
                              * arc; 0 = f64 arcs) */
    int32_t lat16;           /* 1 when every table latency, the self-loop diagonal included, is an
                              * integer below 0xFFFF: the SHD_ROUTE_PAYLOAD_LAT16 eligibility */
} shd_route_info_t;

int shd_route_create(shd_route_t** out, const shd_graph_t* graph, int device);
void shd_route_destroy(shd_route_t* ctx);
int shd_route_get_info(const shd_route_t* ctx, shd_route_info_t* info);
const char* shd_route_strerror(int code);

/* Eager batch of SOURCE(s,.) rows: for i < ns, j < nt,
 *   lat_out[i*nt + j], rel_out[i*nt + j] = Path(src[i] -> tgt[j]);
 *   row_min_out[i] = min_j lat_out[i*nt + j]   (any of the three outputs may be NULL).
 * Host pointers; the call blocks.  SHD_ROUTE_ENOEDGE / SHD_ROUTE_EUNREACH are per-entry
 * failures: every row is still written, the failed entries are NaN (the reference skips
 * storing those targets, topology.c:1812-1870) and the code is returned at the end.
 * row_min_out[i] is the minimum over the entries of row i that did not fail, and +inf when
 * none did. */
int shd_route_rows(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt,
                   int32_t nt, uint32_t flags, double* lat_out, double* rel_out,
                   double* row_min_out);

/* Same, all pointers device pointers (inputs already resident in HBM, outputs written
 * in HBM with row stride ld >= nt); enqueued on `stream` (a hipStream_t, NULL =
 * default stream); returns after enqueueing.  Errors detected on the device are
 * reported by the next shd_route_sync(). */
int shd_route_rows_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns,
                         const int32_t* d_tgt, int32_t nt, int64_t ld, uint32_t flags,
                         double* d_lat, double* d_rel, double* d_row_min, void* stream);

/* Wait for `stream` and return the first device-side error raised since the last sync. */
int shd_route_sync(shd_route_t* ctx, void* stream);

/* ---- path hops: hop counts and explicit routes of the chosen paths ---------------------
 * The path behind every number above, which the reference shows in the line
 * _topology_computeSourcePaths logs per target (topology.c:1449, 1502-1503, 1829-1844).
 * Entries are those of shd_route_rows, same flags:
 *   t != s : hops = the edges on the chosen shortest path (the tie rule above); the path is
 *            hops + 1 vertices from s to t with hops edge ids.
 *   t == s : the batch self entry (topology.c:1471-1499): hops = 1, vertices [s, s], the edge
 *            the self-loop; without a self-loop the entry is -1 and SHD_ROUTE_ENOEDGE.
 *   unreachable t : entry -1 and SHD_ROUTE_EUNREACH.
 * Failed entries never stop the rest from being written; the code is returned at the end
 * (shd_route_hops, shd_route_paths) or by the next shd_route_sync (shd_route_hops_async).
 * With SHD_ROUTE_DISPATCH a complete graph, or prefer-direct with an adjacent pair, gives the
 * one-hop direct path [s, t] (topology.c:1877-1927, 2019-2031) over the edge the direct
 * tables keep, the lowest edge id joining the pair; without the flag always the tree path.
 * On a multigraph (info.multigraph, SURVEY hazard H3) the edge reported for a tree hop is the
 * tie rule's: the lowest edge id among the parallel edges that are tight for that hop, which
 * is the edge the latency came from; the reference's igraph_get_eid may name another one.
 * The hops calls derive everything from the all-vertex latency rows of shd_route_rows_async,
 * so they work with every kernel the context selects, and they use the context's scratch and
 * its rows launch: the "one rows launch at a time" rule at the top of this header covers
 * them too (no rows, planned rows or hops call of the same context in flight together).
 * Scratch: per source of a chunk an f64 distance row and a u32 parent row over all vertices
 * (shd_route_paths: an i32 hop row too), chunks of sources sized to 1 GiB, or to
 * SHD_ROUTE_HOPS_SCRATCH bytes from the environment.  SHD_ROUTE_HOPS_LDS=0 keeps the hop
 * counting's state out of LDS (its large-graph form, for tests).  Diagnostic rate: every
 * call runs the sources' SSSP again. */

/* d_hops[i*ld + j] = hops of src[i] -> tgt[j] (i32, -1 = failed entry), d_row_max[i] = the
 * largest entry of row i; either may be NULL.  Device pointers, as shd_route_rows_async. */
int shd_route_hops_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                         int32_t nt, int64_t ld, uint32_t flags, int32_t* d_hops, int32_t* d_row_max,
                         void* stream);
/* Same with host pointers (row stride nt); blocks. */
int shd_route_hops(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                   uint32_t flags, int32_t* hops_out, int32_t* row_max_out);
/* Explicit routes of npairs (pair_src[k], pair_tgt[k]) pairs, in any order, repeats allowed
 * (grouped by source inside).  Host pointers; blocks.  off_out (npairs + 1 entries):
 * off_out[k] = the element offset of pair k's vertices in vert_out, off_out[k+1] - off_out[k]
 * = its hops + 1, or 0 for a failed pair.  The edge ids of pair k start in edge_out at
 * off_out[k] - (the pairs before k that did not fail), i.e. at off_out[k] - k when none
 * failed.  cap = the elements vert_out and edge_out can each hold: if cap is smaller than
 * off_out[npairs] the call returns SHD_ROUTE_EINVAL with off_out complete and nothing
 * written to vert_out / edge_out, and the caller retries with that size (vert_out NULL and
 * cap 0: the sizing call).  A vertex out of range is SHD_ROUTE_EINVAL for the whole call. */
int shd_route_paths(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, int64_t npairs,
                    uint32_t flags, int64_t* off_out, int32_t* vert_out, int32_t* edge_out, int64_t cap);

/* ---- link loads: per-edge and per-vertex weight of the chosen paths ----------------------
 * No reference equivalent (Shadow 1.14 counts packets per cached Path only, path.c:57-60).
 * Entries are those of shd_route_hops*, same flags; the load of an entry (s, t) with weight
 * w goes where shd_route_paths puts that entry's route:
 *   t != s : w is added to edge_load[e] of every edge id e on the chosen path (the tie rule
 *            above; on a multigraph the lowest tight edge id of each hop, the edge
 *            shd_route_paths reports) and to transit[v] of every intermediate vertex v of the
 *            path, not of s or t.
 *   t == s : w goes on the lowest self-loop edge of s, no transit; without a self-loop the
 *            entry fails with SHD_ROUTE_ENOEDGE.
 *   unreachable t : the entry fails with SHD_ROUTE_EUNREACH.
 * With SHD_ROUTE_DISPATCH a complete graph, or prefer-direct with an adjacent pair, puts w on
 * the direct edge (the lowest edge id joining the pair), no transit.  A failed entry never
 * stops the rest; it fails whatever its weight, and its weight is added to *unrouted.  The
 * code comes back at the end (shd_route_loads, shd_route_pair_loads) or by the next
 * shd_route_sync (shd_route_loads_async).  Repeated targets and repeated pairs add up.  On an
 * undirected graph an edge has one load for both directions.  All sums are u64 integer adds:
 * exact (modulo 2^64) and independent of order.
 * The sums go down each source's shortest-path tree, O(n) per source: the hop depth of every
 * vertex orders the tree into levels, and from the deepest level up every vertex hands its
 * subtree's sum to its parent.  The calls run a rows launch inside (the "one rows launch at a
 * time" rule covers them) and follow the hops calls' scratch: per source of a chunk an f64
 * distance row, a u32 parent row and an i32 hop row over all vertices, chunks sized to
 * SHD_ROUTE_HOPS_SCRATCH (1 GiB).  The per-source sums live in LDS (22 bytes per vertex) or,
 * on larger graphs and with SHD_ROUTE_LOADS_LDS=0, in HBM slices of 16 to 512 workgroup slots
 * within a quarter of that budget.  Diagnostic rate: every call runs the sources' SSSP. */
#define SHD_ROUTE_LOADS_ADD 0x400u /* add into the outputs instead of zeroing them first */
/* Device pointers, as shd_route_hops_async: d_wt[i*ld + j] = the weight of (src[i], tgt[j]),
 * NULL = 1 per entry (how many of the listed pairs route over each link);
 * d_edge_load[n_edges], d_transit[n_vertices], d_unrouted[1]; any output may be NULL. */
int shd_route_loads_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                          int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt,
                          uint64_t* d_edge_load, uint64_t* d_transit, uint64_t* d_unrouted, void* stream);
/* Same with host pointers (row stride nt); blocks.  A vertex out of range is SHD_ROUTE_EINVAL
 * for the whole call, nothing written. */
int shd_route_loads(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                    uint32_t flags, const uint64_t* wt, uint64_t* edge_load_out, uint64_t* transit_out,
                    uint64_t* unrouted_out);
/* The sparse form: npairs (pair_src[k], pair_tgt[k], pair_wt[k]) in any order (pair_wt NULL =
 * 1 each), grouped by source inside as shd_route_paths groups them.  Host pointers; blocks. */
int shd_route_pair_loads(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt,
                         const uint64_t* pair_wt, int64_t npairs, uint32_t flags, uint64_t* edge_load_out,
                         uint64_t* transit_out, uint64_t* unrouted_out);

/* ---- tie envelope: path counts and reliability bounds over tied shortest paths ------------
 * No reference equivalent: the reference keeps the one path igraph's heap pop order leaves it
 * with (topology.c:1756), the engine the one its tie rule above picks.  These calls say what
 * every tie rule could give.  Entries are those of shd_route_hops*, same flags.
 *   A shortest path s -> t (t != s) is a sequence of arcs u -> v over an edge e with
 * d[u] + w_e == d[v] in f64, d the all-vertex latency row of shd_route_rows_async for s (no
 * dispatch, any selected kernel) with d[s] taken as 0.0.  Self-loops are not arcs; parallel
 * tight edges are distinct paths.
 *   t != s : count = the number of such paths, a u64 that saturates at 2^64 - 1 (a saturated
 *            summand keeps the sum saturated); rel_lo / rel_hi = the min / max over those paths
 *            of (1.0*f_s)*r_1*r_2*... folded from the source, then multiplied by f_t last when
 *            the target has a vertex factor; absent factors are skipped.  Computed as
 *            lo[s] = hi[s] = 1.0*f_s, lo[v] = min over the tight in-arcs of lo[u]*r_e (hi: max),
 *            count[v] = the saturating sum of count[u].  Reliabilities are in [0, 1], so
 *            fl(a*r) is monotone in a and the programme's bounds are the exact min and max of
 *            the paths' left folds, bit for bit: the rel of shd_route_rows lies in
 *            [rel_lo, rel_hi] (to the bit where f_t is absent or 1.0, within a few ulp
 *            otherwise) and equals both where count == 1.
 *   t == s : count 1, rel_lo == rel_hi == the batch self entry's reliability (the lowest-id
 *            self-loop, (1.0*f_s)*r_ss); without a self-loop count 0, NaN and SHD_ROUTE_ENOEDGE.
 *   unreachable t : count 0, NaN and SHD_ROUTE_EUNREACH.
 * With SHD_ROUTE_DISPATCH a complete graph, or prefer-direct with an adjacent pair, gives
 * count 1 and both bounds = ((1.0*f_s)*f_t)*r over the lowest edge id joining the pair; on a
 * complete graph no rows launch and no sweep run (a pair without an edge: SHD_ROUTE_ENOEDGE).
 * Failed entries never stop the rest from being written; the code is returned at the end
 * (shd_route_ties) or by the next shd_route_sync (shd_route_ties_async).
 * The calls run a rows launch inside (the "one rows launch at a time" rule covers them) and
 * follow the hops calls' scratch: per source of a chunk an f64 distance row and a u32 row (the
 * tight in-degree of every vertex, in the parent row's place), chunks sized to
 * SHD_ROUTE_HOPS_SCRATCH (1 GiB).  One workgroup per source sweeps the DAG of tight arcs level
 * by level; its state (32 bytes per vertex while n <= 65535, 36 above) lives in LDS or, on
 * larger graphs and with SHD_ROUTE_TIES_LDS=0, in HBM slices of 16 to 512 workgroup slots
 * within a quarter of that budget.  The rounds equal the deepest tied path in hops.
 * Diagnostic rate: every call runs the sources' SSSP. */

/* d_count / d_rel_lo / d_rel_hi[i*ld + j] of src[i] -> tgt[j]; any output may be NULL.  Device
 * pointers, as shd_route_hops_async. */
int shd_route_ties_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                         int32_t nt, int64_t ld, uint32_t flags, uint64_t* d_count, double* d_rel_lo,
                         double* d_rel_hi, void* stream);
/* Same with host pointers (row stride nt); blocks. */
int shd_route_ties(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                   uint32_t flags, uint64_t* count_out, double* rel_lo_out, double* rel_hi_out);

/* ---- ECMP link loads: every entry's weight split evenly over all of its shortest paths ----
 * No reference equivalent.  shd_route_loads* put all of a pair's weight on the one path the tie
 * rule picks; routers with equal-cost multipath spread it over the tied paths.  With weight 1
 * on all pairs the outputs are the edge and vertex betweenness centrality (ordered pairs,
 * endpoints excluded).  Entries are those of shd_route_hops*, same flags; a shortest path is
 * what shd_route_ties defines: a chain of tight arcs, d[u] + w_e == d[v] in f64, over the
 * all-vertex latency row of the source with d[s] taken as 0.0; self-loops are not arcs,
 * parallel tight edges are distinct paths.  sigma_s(v) = the number of shortest paths s -> v as
 * f64: exact below 2^53 and rounded above; it never saturates.
 *   t != s : w is split evenly over the sigma_s(t) shortest paths: every edge id on a path
 *            gets that path's w / sigma_s(t) in edge_load, every intermediate vertex of the path
 *            gets it in transit; the endpoints s and t get none.  Summed per source this is the
 *            programme own[x] = the sum of the weights of the entries with target x,
 *            delta[v] = the sum over the tight out-arcs (v -> x, e) of f_e,
 *            f_e = (sigma[v] / sigma[x]) * (own[x] + delta[x]); edge_load[e] += f_e, and
 *            transit[v] += delta[v] for v != s (Brandes' dependency accumulation).
 *   t == s : w goes on the lowest self-loop edge of s, no transit; without a self-loop the
 *            entry fails with SHD_ROUTE_ENOEDGE.
 *   unreachable t : the entry fails with SHD_ROUTE_EUNREACH.
 * With SHD_ROUTE_DISPATCH a complete graph, or prefer-direct with an adjacent pair, puts the
 * whole w on the direct edge (the lowest edge id joining the pair), no transit; on a complete
 * graph no rows launch and no sweep run.  A failed entry never stops the rest; it fails
 * whatever its weight, and its weight is added to *unrouted, which stays a uint64_t: an exact
 * integer sum (modulo 2^64), as in the loads.  The code comes back at the end
 * (shd_route_ecmp_loads, shd_route_pair_ecmp_loads) or by the next shd_route_sync
 * (shd_route_ecmp_loads_async).  On an undirected graph an edge has one load for both
 * directions.
 *   Weights stay uint64_t (packet counts).  Repeated targets of one source and repeated pairs
 * are summed as integers, modulo 2^64, and that sum is converted to f64 once.  The loads are
 * doubles.  Every quantity of the programme is non-negative and nothing is subtracted
 * (transit is delta, not "sum minus own"), so errors stay relative: an element whose exact
 * value is 0 is exactly 0.  Where every listed pair has exactly one shortest path and the
 * totals are below 2^53 the result equals shd_route_loads converted to double, exactly.
 *   Reproducibility: the programme of one source has a fixed order (tight arcs in the order of
 * the in- and out-CSR: by neighbour, then edge id; lists of more than 32 arcs are summed by a
 * wave in a fixed tree) and is reproducible to the bit.  The sums across sources into the
 * outputs are floating-point atomic adds in the order they arrive: a call with more than two
 * sources is reproducible to rounding, not to the bit.  With R the deepest level of any source
 * of the call, D the largest number of tight in- or out-arcs of a vertex and A = ns * (1 + the
 * largest multiplicity of one pair), every element is within
 * ((R+1)*(2*(R+1)*D + D + 4) + A) * 2^-52 relative of the exact value.
 *   The calls run a rows launch inside (the "one rows launch at a time" rule covers them) and
 * follow the ties calls' scratch: per source of a chunk an f64 distance row and a u32 row (the
 * tight in-degrees), chunks sized to SHD_ROUTE_HOPS_SCRATCH (1 GiB).  One workgroup per source
 * sweeps the DAG of tight arcs forwards, level by level, for sigma, and backwards for delta;
 * its state (34 bytes per vertex while n <= 65535, 36 above) lives in LDS or, on larger graphs
 * and with SHD_ROUTE_ECMP_LDS=0, in HBM slices of 16 to 512 workgroup slots within a quarter of
 * that budget.  Diagnostic rate: every call runs the sources' SSSP.  SHD_ROUTE_LOADS_ADD adds
 * into the outputs instead of zeroing them first. */
/* Device pointers, as shd_route_loads_async: d_wt[i*ld + j] = the weight of (src[i], tgt[j]),
 * NULL = 1 per entry; d_edge_load[n_edges], d_transit[n_vertices] (memory of hipMalloc),
 * d_unrouted[1]; any output may be NULL. */
int shd_route_ecmp_loads_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                               int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt,
                               double* d_edge_load, double* d_transit, uint64_t* d_unrouted, void* stream);
/* Same with host pointers (row stride nt); blocks.  A vertex out of range is SHD_ROUTE_EINVAL
 * for the whole call, nothing written. */
int shd_route_ecmp_loads(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                         uint32_t flags, const uint64_t* wt, double* edge_load_out, double* transit_out,
                         uint64_t* unrouted_out);
/* The sparse form: npairs (pair_src[k], pair_tgt[k], pair_wt[k]) in any order (pair_wt NULL =
 * 1 each), grouped by source inside as shd_route_paths groups them.  Host pointers; blocks. */
int shd_route_pair_ecmp_loads(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt,
                              const uint64_t* pair_wt, int64_t npairs, uint32_t flags, double* edge_load_out,
                              double* transit_out, uint64_t* unrouted_out);

/* ---- path folds: sum, min, max and product of per-edge values along the chosen paths ------
 * No reference equivalent: the reference folds latency and reliability only and drops the
 * graphml's jitter after validating it (topology.c:1105-1114).  A call takes nf folds at once
 * (1 <= nf <= SHD_ROUTE_FOLD_MAX_N) and pays for the sources' trees once: ops[k] is the op of
 * fold k (a host array in all three calls, read at call time), val[k * n_edges + e] the value of
 * edge id e for fold k (on an undirected graph an edge has one value for both directions), and
 * out[k * plane + i * ld + j] fold k of the entry src[i] -> tgt[j].
 *   Entries are those of shd_route_hops*, with the same flags:
 *   t != s : the fold over the edge ids shd_route_paths reports for the entry, taken in order
 *            from the source (on a multigraph each tree hop uses the lowest tight edge id of
 *            that hop).
 *   t == s : the fold over the lowest self-loop edge alone; without a self-loop the entry is NaN
 *            and the code SHD_ROUTE_ENOEDGE.
 *   unreachable t : NaN and SHD_ROUTE_EUNREACH.
 * With SHD_ROUTE_DISPATCH a complete graph, or prefer-direct with an adjacent pair, gives the fold
 * over the one direct edge (the lowest edge id joining the pair); on a complete graph no rows
 * launch and no sweep run, and a pair without an edge is SHD_ROUTE_ENOEDGE.  A failed entry is
 * NaN in every fold and never stops the rest; the code comes back at the end (shd_route_fold,
 * shd_route_pair_fold) or by the next shd_route_sync (shd_route_fold_async).  A vertex out of
 * range is SHD_ROUTE_EINVAL for the whole call; ns == 0 is SHD_ROUTE_OK.
 *   Values: NaN is reserved for failed entries.  The two blocking calls scan val and return
 * SHD_ROUTE_EINVAL, nothing written, if any value is NaN.  shd_route_fold_async does not look:
 * a NaN value there gives unspecified entries on the paths that cross it, never a fault.
 * +inf and -inf are ordinary values.
 *   Exactness: every entry is a deterministic left fold from the source, acc = op(acc, a_e) hop
 * by hop from the op's start value.  There are no atomics on values and nothing is reassociated,
 * so all four ops are reproducible and equal the plain fold in double, bit for bit:
 *   SUM over the edge latencies equals lat of shd_route_rows;
 *   SUM over ones equals the hop count of shd_route_hops;
 *   PROD over 1 - loss equals rel of shd_route_rows on graphs without vertex loss.
 *   The calls run a rows launch inside (the "one rows launch at a time" rule covers them) and
 * follow the hops calls' scratch: per source of a chunk an f64 distance row, a u32 parent row
 * and an i32 hop row, chunks sized to SHD_ROUTE_HOPS_SCRATCH (1 GiB).  One workgroup per source
 * sorts the reached vertices by hop depth once and sweeps the levels top-down once per fold;
 * its state (14 bytes per vertex while n <= 65535, 16 above) lives in LDS or, on larger graphs
 * and with SHD_ROUTE_FOLD_LDS=0, in HBM slices of 16 to 512 workgroup slots within 256 MiB,
 * regrown (which synchronises the stream) when a launch needs more than the context holds.
 * First use blocks only for what the hops calls build.  Diagnostic rate: every call runs the
 * sources' SSSP. */
#define SHD_ROUTE_FOLD_SUM  0   /* acc = acc + a_e, from 0.0 */
#define SHD_ROUTE_FOLD_MIN  1   /* acc = a_e < acc ? a_e : acc, from +inf */
#define SHD_ROUTE_FOLD_MAX  2   /* acc = a_e > acc ? a_e : acc, from -inf */
#define SHD_ROUTE_FOLD_PROD 3   /* acc = acc * a_e, from 1.0 */
#define SHD_ROUTE_FOLD_MAX_N 8  /* folds per call */
/* Device pointers: d_val[nf * n_edges], d_out with ld >= nt and plane >= ns * ld; elements
 * outside the nt entries of a row are never written. */
int shd_route_fold_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                         int64_t ld, uint32_t flags, const int32_t* ops, int32_t nf, const double* d_val,
                         double* d_out, int64_t plane, void* stream);
/* Same with host pointers (ld = nt, plane = ns * nt); blocks. */
int shd_route_fold(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                   uint32_t flags, const int32_t* ops, int32_t nf, const double* val, double* out);
/* The sparse form: out[k * npairs + p] = fold k of (pair_src[p], pair_tgt[p]), in the caller's
 * pair order; the pairs are grouped by source inside as shd_route_pair_loads groups them.  Host
 * pointers; blocks. */
int shd_route_pair_fold(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt, int64_t npairs,
                        uint32_t flags, const int32_t* ops, int32_t nf, const double* val, double* out);

/* ---- link loss: expected packets reaching, dropped by and delivered over the chosen paths ----
 * No reference equivalent: the reference drops a packet with one coin flip on the Path's
 * end-to-end reliability.  These calls spread that loss over the route: how many of the packets
 * shd_route_loads* put on a link are expected to reach it, how many each link and each vertex
 * drops, and how many arrive.  Entries, flags (SHD_ROUTE_DISPATCH, SHD_ROUTE_LOADS_ADD),
 * weights (uint64_t packet counts, NULL = 1 per entry) and the failure rules are those of
 * shd_route_loads*; the route of an entry is the one shd_route_paths reports.
 *   Per element, all f64 and nothing contracted into a fused multiply-add: r_e = the context's
 * reliability of edge id e (1.0f - loss, promoted), q_e = edge_packetloss[e] as given, f_v = the
 * context's vertex factor, p_v = vertex_packetloss[v] as given; a NaN or absent vertex loss
 * means no factor and no vertex drop.  Per source s:
 *   F_s = 1.0*f_s, or 1.0 when f_s is absent.  pre[s] = F_s and pre[v] = pre[parent(v)] * r_e
 *   over the parent arc: the left fold from the source, level by level, as the PROD fold.
 *   own[t] = the u64 sum (modulo 2^64) of the weights of the source's tree-routed entries with
 *   target t (repeated targets are summed as integers first); W_sub(v) = the u64 sum of own over
 *   the subtree of v, the edge load shd_route_loads* give the parent arc.  Each integer is
 *   converted to f64 once.
 *   tree arc u -> v over edge id e, W_sub(v) != 0 : reach = (double)W_sub(v) * pre[u];
 *            edge_reach[e] += reach; edge_drop[e] += reach * q_e.
 *   tree target t, own[t] != 0 : arrive = (double)own[t] * pre[t]; vertex_drop[t] += arrive * p_t
 *            where p_t is present; delivered[t] += arrive * f_t, or arrive where f_t is absent.
 *   direct-dispatched entry (s, t, w) over the lowest edge id e joining the pair :
 *            reach = (double)w * F_s; edge_reach[e] += reach; edge_drop[e] += reach * q_e;
 *            arrive = reach * r_e, then the target's step above.
 *   t == s with the lowest self-loop e : reach = (double)w * F_s; edge_reach[e] += reach;
 *            edge_drop[e] += reach * q_e; delivered[s] += reach * r_e.  No second vertex factor:
 *            the batch self entry's rel is (1.0*f_s)*r_ss.
 *   the source vertex : vertex_drop[s] += (double)W_routed * p_s where p_s is present, W_routed
 *            the u64 sum of the weights of all entries of s that did not fail (tree, direct and
 *            self): one addend per source.
 *   a failed entry (SHD_ROUTE_ENOEDGE, SHD_ROUTE_EUNREACH) adds its weight to *unrouted, a
 *            uint64_t and exact (modulo 2^64), and contributes nowhere else, whatever its weight.
 * On an undirected graph an edge has one edge_reach and one edge_drop for both directions.
 * Nothing is subtracted anywhere and zero weights add nothing, so an element whose exact value
 * is 0 is exactly 0.  On a graph without loss edge_reach equals edge_load of shd_route_loads*
 * converted to double (exactly, below 2^53) and both drops are zero; with unit weights from one
 * source delivered[t] is rel of shd_route_rows on a graph without vertex loss, and rel_lo of
 * shd_route_ties wherever its count is 1.  The code of a failed entry comes back at the
 * end (shd_route_loss, shd_route_pair_loss) or by the next shd_route_sync
 * (shd_route_loss_async); a failed entry never stops the rest.
 *   Reproducibility: the programme of one source has a fixed order and is reproducible to the
 * bit.  The sums across sources into the outputs are f64 atomic adds in the order they arrive,
 * the add the ECMP loads use.  A call in which no element receives more than two addends is
 * bit-equal to the plain f64 programme (the first add onto 0.0 is exact, one more add is one
 * commutative rounding); one source with distinct targets is such a call.  Otherwise, with R
 * the deepest level of any source of the call and A the largest number of addends into one
 * element, every element is within (R + 4 + A) * 2^-52 relative of the exact value
 * (DESIGN.md 4.10).
 *   The calls run a rows launch inside (the "one rows launch at a time" rule covers them) and
 * follow the loads calls' scratch: per source of a chunk an f64 distance row, a u32 parent row
 * and an i32 hop row, chunks sized to SHD_ROUTE_HOPS_SCRATCH (1 GiB).  One workgroup per source
 * sorts the reached vertices by hop depth, carries pre down the levels, sums the weights up them
 * as integers and multiplies the two in one pass; its state (22 bytes per vertex while
 * n <= 65535, 24 above) lives in LDS up to 7,442 vertices or, on larger graphs and with
 * SHD_ROUTE_LOSS_LDS=0, in HBM slices of 16 to 512 workgroup slots within a quarter of that
 * budget, regrown (which synchronises the stream) when a launch needs more than the context
 * holds.  First use blocks for what the hops calls build and for the three loss columns (per
 * edge r_e and q_e, per vertex p_v), once per context.  On a complete graph under
 * SHD_ROUTE_DISPATCH no rows launch and no sweep run.  Diagnostic rate: every call runs the
 * sources' SSSP. */
/* Device pointers, as shd_route_loads_async: d_wt[i*ld + j] = the weight of (src[i], tgt[j]),
 * NULL = 1 per entry; d_edge_reach[n_edges], d_edge_drop[n_edges], d_vertex_drop[n_vertices],
 * d_delivered[n_vertices] (doubles, memory of hipMalloc), d_unrouted[1]; any output may be NULL. */
int shd_route_loss_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                         int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt,
                         double* d_edge_reach, double* d_edge_drop, double* d_vertex_drop,
                         double* d_delivered, uint64_t* d_unrouted, void* stream);
/* Same with host pointers (row stride nt); blocks.  A vertex out of range is SHD_ROUTE_EINVAL
 * for the whole call, nothing written. */
int shd_route_loss(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                   uint32_t flags, const uint64_t* wt, double* edge_reach_out, double* edge_drop_out,
                   double* vertex_drop_out, double* delivered_out, uint64_t* unrouted_out);
/* The sparse form: npairs (pair_src[k], pair_tgt[k], pair_wt[k]) in any order (pair_wt NULL =
 * 1 each), grouped by source inside as shd_route_paths groups them.  Host pointers; blocks. */
int shd_route_pair_loss(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt,
                        const uint64_t* pair_wt, int64_t npairs, uint32_t flags, double* edge_reach_out,
                        double* edge_drop_out, double* vertex_drop_out, double* delivered_out,
                        uint64_t* unrouted_out);

/* ---- link outages: what the entries lose when a set of edges goes down ----
 * No reference equivalent: Shadow 1.14 has no outage model, a user loads another topology.
 * Scenario k is the set F_k = scn_edge[scn_off[k] .. scn_off[k+1]) of edge ids, duplicates
 * allowed; G_k is the context's graph without those edges, the others in their order (an
 * undirected edge loses both arcs, a directed edge its one arc).  A vertex outage is the
 * scenario of the vertex's incident edges.  Every entry (src[i], tgt[j], weight) is judged
 * without dispatch -- tree routes and the batch self entry, as shd_route_rows gives them with
 * flags 0 -- so flags must be 0: SHD_ROUTE_DISPATCH or any other bit is SHD_ROUTE_EINVAL.
 *   old = the entry in G.  An entry that fails in G (SHD_ROUTE_ENOEDGE, SHD_ROUTE_EUNREACH)
 * fails as in the loads calls: its code is raised, its weight goes to *unrouted once (not once
 * per scenario) and it takes part in no scenario.
 *   new = the entry of a context created from G_k: for t != s the shortest latency in G_k (the
 * f64 left fold from the source), for t == s the latency of the lowest self-loop of s not in F_k.
 *   Per scenario, stats[k*SHD_ROUTE_OUTAGE_NSTAT + ...] in u64 adds, exact mod 2^64 and
 * independent of order:
 *     SHD_ROUTE_OUTAGE_HIT     the weight of the entries whose old route, the one shd_route_paths
 *                              reports, uses an edge of F_k (for a self entry: the self-loop);
 *     SHD_ROUTE_OUTAGE_CUT     the weight of the entries without a route in G_k;
 *     SHD_ROUTE_OUTAGE_SLOWER  the weight of the entries routable in both with new > old;
 * max_add[k] = the largest new - old (one f64 subtraction per entry) over the slower entries,
 * 0.0 without any (an entry of weight 0 is an entry too): an exact maximum, independent of
 * order.  lat[(k*ns + i)*ld + j], if asked
 * for, is the new latency, NaN where cut or where the entry failed in G; it is bit-equal to
 * lat of shd_route_rows with flags 0 on a context created from G_k.  An entry that is hit but
 * has a tied alternative keeps its latency and counts in hit only.  Reliability and hops of the
 * new routes are not computed: create a context for the one scenario wanted in full.
 *   nscn == 0 writes only *unrouted; an empty scenario gives zeros and the old latencies.
 *   The calls run a rows launch inside (the "one rows launch at a time" rule covers them) and
 * follow the loads calls' scratch: distance, parent and hop rows per source of a chunk, chunks
 * sized to SHD_ROUTE_HOPS_SCRATCH.  A work unit is one source with a slab of up to 1,024
 * scenarios, the grid covers the units.  A unit sorts the source's tree by hop depth, finds
 * the scenarios that fail a parent arc (or the source's lowest self-loop) and repairs each of
 * them in the marked subtrees alone: seed from the unmarked in-neighbours, then pull sweeps
 * until nothing changes.  The state (17 bytes per vertex while n <= 65535, 21
 * above) lives in LDS up to 9,328 vertices or, on larger graphs and with
 * SHD_ROUTE_OUTAGE_LDS=0, in HBM slices of 16 to 512 workgroup slots within a quarter of
 * that budget, regrown (which synchronises the stream) when a launch needs more.  First use
 * blocks for what the hops calls build and for the edge ends, latencies and self-loop lists,
 * once per context.  Diagnostic rate: every call runs the sources' SSSP. */
#define SHD_ROUTE_OUTAGE_HIT 0
#define SHD_ROUTE_OUTAGE_CUT 1
#define SHD_ROUTE_OUTAGE_SLOWER 2
#define SHD_ROUTE_OUTAGE_NSTAT 3
/* Device pointers, as shd_route_loads_async: d_wt[i*ld + j], NULL = 1 per entry;
 * d_scn_off[nscn + 1] (from 0, rising), d_scn_edge each scenario ascending; d_stats
 * [nscn * SHD_ROUTE_OUTAGE_NSTAT], d_max_add[nscn], d_lat[((int64)k*ns + i)*ld + j],
 * d_unrouted[1]; any output may be NULL.  A validation kernel raises SHD_ROUTE_EINVAL on the
 * error word for an offset, range or order violation (the outputs are then undefined); the
 * main kernel indexes no memory with an unchecked id. */
int shd_route_outage_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                           int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt,
                           const int64_t* d_scn_off, const int32_t* d_scn_edge, int32_t nscn,
                           uint64_t* d_stats, double* d_max_add, double* d_lat, uint64_t* d_unrouted,
                           void* stream);
/* Same with host pointers (row stride nt); blocks.  Scenario ids in any order: each scenario is
 * sorted inside.  An id outside [0, n_edges) or a vertex out of range is SHD_ROUTE_EINVAL for
 * the whole call, nothing written. */
int shd_route_outage(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                     uint32_t flags, const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge,
                     int32_t nscn, uint64_t* stats_out, double* max_add_out, double* lat_out,
                     uint64_t* unrouted_out);
/* The sparse form: npairs (pair_src[p], pair_tgt[p], pair_wt[p]) in any order (pair_wt NULL =
 * 1 each); lat_out[k*npairs + p] in the caller's pair order.  Host pointers; blocks. */
int shd_route_pair_outage(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt,
                          const uint64_t* pair_wt, int64_t npairs, uint32_t flags, const int64_t* scn_off,
                          const int32_t* scn_edge, int32_t nscn, uint64_t* stats_out, double* max_add_out,
                          double* lat_out, uint64_t* unrouted_out);

/* ---- link repricing: what the entries gain or lose when a set of edges gets other latencies ----
 * No reference equivalent: a user of Shadow 1.14 loads another topology.
 * Scenario k is the list of pairs (scn_edge[x], scn_lat[x]) for x in scn_off[k] .. scn_off[k+1));
 * G_k is the context's graph with those edges' latencies replaced: edge order, ends, losses and
 * everything else stay as they are.  An undirected edge changes both arcs, a directed edge its
 * one arc, a self-loop the self entry only.  A new latency must be finite and > 0, anything else
 * is SHD_ROUTE_EINVAL; removal stays with the outage calls.  An id repeated within one scenario
 * is SHD_ROUTE_EINVAL (the async form asks for strictly ascending ids); a new latency equal to
 * the old one is allowed.
 *   Absorbed latencies follow the rule at shd_graph_t: with lo the minimum and hi the maximum
 * over the graph's latencies on edges that are no self-loops and every new latency of the call
 * put on such an edge, lo <= (n_vertices - 1) * hi * 2^-52 makes the whole call
 * SHD_ROUTE_EUNSUPPORTED with nothing computed (the host forms refuse before they launch, the
 * async form raises it on the error word from its check kernel).  The rule is sufficient for
 * every G_k at once and therefore conservative: it may refuse a call none of whose scenarios,
 * taken alone, would be refused as a graph.
 *   Every entry (src[i], tgt[j], weight) is judged without dispatch, as for the outage calls:
 * flags must be 0, SHD_ROUTE_DISPATCH or any other bit is SHD_ROUTE_EINVAL.
 *   old = the entry in G.  An entry that fails in G (SHD_ROUTE_ENOEDGE, SHD_ROUTE_EUNREACH) raises
 * its code, adds its weight to *unrouted once (not once per scenario) and takes part in no
 * scenario.
 *   new = the entry of a context created from G_k: for t != s the shortest latency in G_k (the
 * f64 left fold from the source), for t == s the latency in G_k of the lowest-id self-loop of s.
 * Connectivity does not change, so nothing is ever cut.
 *   Per scenario, stats[k*SHD_ROUTE_REPRICE_NSTAT + ...] in u64 adds, exact mod 2^64 and
 * independent of order:
 *     SHD_ROUTE_REPRICE_HIT     the weight of the entries whose old route, the one shd_route_paths
 *                               reports, uses a listed edge (for a self entry: the lowest self-loop);
 *     SHD_ROUTE_REPRICE_SLOWER  the weight of the entries with new > old;
 *     SHD_ROUTE_REPRICE_FASTER  the weight of the entries with new < old;
 * max_add[k] = the largest new - old over the slower entries and max_gain[k] = the largest
 * old - new over the faster ones (one f64 subtraction per entry, 0.0 without any entry of that
 * kind, a u64 maximum on the bits); min_new[k] = the smallest new latency over the entries that
 * route in G (a u64 minimum on the bits, +inf without any such entry): the runahead window a
 * simulation of G_k would get from these entries.  lat[(k*ns + i)*ld + j], if asked for, is the
 * new latency, NaN where the entry failed in G; it is bit-equal to lat of shd_route_rows with
 * flags 0 on a context created from G_k.  An entry that is hit but keeps its latency counts in
 * hit only.  Reliability and hops of the new routes are not computed.
 *   nscn == 0 writes only *unrouted; an empty scenario gives zero stats and the old latencies,
 * with min_new the old minimum.
 *   The calls run a rows launch inside (the "one rows launch at a time" rule covers them) and
 * follow the outage calls' scratch and work units.  A unit holds the source's old row as its
 * current distances, finds the scenarios that reprice a parent arc or the source's lowest
 * self-loop or lower an edge below the distance gap of its ends (every other scenario leaves the
 * row as it is), marks the subtrees below the listed tree arcs and rebuilds them as an outage
 * does, a listed arc taken at its new latency, then pushes what fell along the out-arcs, round by
 * round, until nothing falls, and puts the touched vertices back.  The state
 * (21.25 bytes per vertex while n <= 65535, 29.25 above) lives in LDS up to 7,456 vertices or, on
 * larger graphs and with SHD_ROUTE_REPRICE_LDS=0, in HBM slices of 16 to 512 workgroup slots
 * within a quarter of SHD_ROUTE_HOPS_SCRATCH, regrown (which synchronises the stream) when a
 * launch needs more.  First use blocks for what the outage and the ECMP loads calls build, once
 * per context.  Diagnostic rate: every call runs the sources' SSSP. */
#define SHD_ROUTE_REPRICE_HIT 0
#define SHD_ROUTE_REPRICE_SLOWER 1
#define SHD_ROUTE_REPRICE_FASTER 2
#define SHD_ROUTE_REPRICE_NSTAT 3
/* Device pointers, as shd_route_outage_async, with d_scn_lat beside d_scn_edge (each scenario
 * strictly ascending in its ids); d_max_gain[nscn] and d_min_new[nscn] beside d_max_add; any
 * output may be NULL.  A validation kernel raises SHD_ROUTE_EINVAL on the error word for an
 * offset, range, order or latency violation and SHD_ROUTE_EUNSUPPORTED for the absorbed-latency
 * rule (the outputs are then undefined); the main kernel indexes no memory with an unchecked
 * id. */
int shd_route_reprice_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                            int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt,
                            const int64_t* d_scn_off, const int32_t* d_scn_edge, const double* d_scn_lat,
                            int32_t nscn, uint64_t* d_stats, double* d_max_add, double* d_max_gain,
                            double* d_min_new, double* d_lat, uint64_t* d_unrouted, void* stream);
/* Same with host pointers (row stride nt); blocks.  Scenario ids in any order: each scenario is
 * sorted by id inside.  An id outside [0, n_edges), a repeated id, a bad latency or a vertex out
 * of range is SHD_ROUTE_EINVAL for the whole call, nothing written. */
int shd_route_reprice(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                      uint32_t flags, const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge,
                      const double* scn_lat, int32_t nscn, uint64_t* stats_out, double* max_add_out,
                      double* max_gain_out, double* min_new_out, double* lat_out, uint64_t* unrouted_out);
/* The sparse form: npairs (pair_src[p], pair_tgt[p], pair_wt[p]) in any order (pair_wt NULL =
 * 1 each); lat_out[k*npairs + p] in the caller's pair order.  Host pointers; blocks. */
int shd_route_pair_reprice(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt,
                           const uint64_t* pair_wt, int64_t npairs, uint32_t flags, const int64_t* scn_off,
                           const int32_t* scn_edge, const double* scn_lat, int32_t nscn, uint64_t* stats_out,
                           double* max_add_out, double* max_gain_out, double* min_new_out, double* lat_out,
                           uint64_t* unrouted_out);

/* ---- link edits: what the entries gain or lose when links are removed, repriced and added ----
 * No reference equivalent: a user of Shadow 1.14 loads another topology.
 * Scenario k is the list of records (scn_edge[x], scn_a[x], scn_b[x], scn_lat[x]) for x in
 * scn_off[k] .. scn_off[k+1)):
 *   scn_edge[x] >= 0 with a finite scn_lat[x] > 0 gives that edge id this latency, as the
 *     repricing calls do;
 *   scn_edge[x] >= 0 with scn_lat[x] == +inf removes that edge, as the outage calls do;
 *     for both, scn_a[x] and scn_b[x] are ignored;
 *   scn_edge[x] == -1 is a new link between scn_a[x] and scn_b[x] at latency scn_lat[x],
 *     undirected or directed as the graph is (a directed graph gets the one arc a -> b); its
 *     latency must be finite and > 0; several new links between the same ends are allowed.
 * G_k is the context's graph with the removed edges taken out and the others in their order,
 * the repriced latencies replaced and the new links appended behind every existing edge in list
 * order, so that their ids lie above every existing id.  Losses play no part: no reliability is
 * computed.
 *   SHD_ROUTE_EINVAL for the whole call, nothing written: an id outside [0, n_edges) other than
 * -1; an id repeated within one scenario; a NaN, zero or negative latency, or +inf on a new link;
 * an end of a new link outside [0, n_vertices); scn_a[x] == scn_b[x] on a new link (a new
 * self-loop could only become the self entry of a vertex whose entry fails in G or whose own
 * loops were all removed; it stays out of scope).
 *   Absorbed latencies follow the rule at shd_graph_t: with lo the minimum and hi the maximum
 * over the graph's latencies on edges that are no self-loops, every finite new latency put on
 * such an edge and every new link's latency, lo <= (n_vertices - 1) * hi * 2^-52 makes the whole
 * call SHD_ROUTE_EUNSUPPORTED with nothing computed, as for the repricing calls (sufficient for
 * every G_k at once and therefore conservative).
 *   Every entry is judged without dispatch: flags must be 0, any bit is SHD_ROUTE_EINVAL.
 *   old = the entry in G.  An entry that fails in G (SHD_ROUTE_ENOEDGE, SHD_ROUTE_EUNREACH) raises
 * its code, adds its weight to *unrouted once and takes part in no scenario.  This is a limit: an
 * entry that fails in G stays out even where a new link of the scenario would route it.
 *   new = the entry of a context created from G_k: for t != s the shortest latency in G_k (the
 * f64 left fold from the source), for t == s the latency in G_k of the lowest-id self-loop of s
 * that is not removed.
 *   Per scenario, stats[k*SHD_ROUTE_EDIT_NSTAT + ...] in u64 adds, exact mod 2^64 and independent
 * of order:
 *     SHD_ROUTE_EDIT_HIT     the weight of the entries whose old route, the one shd_route_paths
 *                            reports, uses a removed or repriced edge (for a self entry: the
 *                            lowest self-loop);
 *     SHD_ROUTE_EDIT_CUT     the weight of the entries with no route in G_k;
 *     SHD_ROUTE_EDIT_SLOWER  the weight of the entries routable in both with new > old;
 *     SHD_ROUTE_EDIT_FASTER  the weight of the entries with new < old;
 * max_add[k] and max_gain[k] as for the repricing calls (u64 maxima on the bits, 0.0 without an
 * entry of the kind); min_new[k] = the smallest new latency over the entries routable in G and in
 * G_k (a u64 minimum on the bits, +inf without one).  lat[(k*ns + i)*ld + j], if asked for, is
 * the new latency, NaN where the entry is cut or failed in G; it is bit-equal to lat of
 * shd_route_rows with flags 0 on a context created from G_k.  An entry whose only change is a
 * tied alternative through a new link keeps its latency and counts nowhere.
 *   nscn == 0 writes only *unrouted; an empty scenario gives zero stats, the old latencies and
 * the old minimum.
 *   The calls run a rows launch inside and follow the repricing calls' scratch, work units and
 * state: the same 21.25 / 29.25 bytes per vertex, in LDS up to 7,456 vertices or, on larger
 * graphs and with SHD_ROUTE_EDIT_LDS=0, in HBM slices.  A unit finds the scenarios that touch a
 * parent arc or the source's lowest self-loop, or lower an edge below the distance gap of its
 * ends, or whose new link does (every other scenario leaves the row as it is), marks the subtrees
 * below the listed tree arcs, rebuilds them with a listed arc at its listed latency and a removed
 * arc left out, then pushes what fell along the out-arcs and along every new link of the
 * scenario, round by round, until a round lowers nothing.  Known limits: a
 * scenario's whole list of new links is relaxed in every round, and the live test and the id
 * searches are the repricing calls'.  Diagnostic rate: every call runs the sources' SSSP. */
#define SHD_ROUTE_EDIT_HIT 0
#define SHD_ROUTE_EDIT_CUT 1
#define SHD_ROUTE_EDIT_SLOWER 2
#define SHD_ROUTE_EDIT_FASTER 3
#define SHD_ROUTE_EDIT_NSTAT 4
/* Device pointers, as shd_route_reprice_async, with d_scn_a and d_scn_b beside d_scn_edge.  Each
 * scenario holds its new links first, in any order, then its ids strictly ascending.  A
 * validation kernel raises SHD_ROUTE_EINVAL on the error word for an offset, id, order, end or
 * latency violation and SHD_ROUTE_EUNSUPPORTED for the absorbed-latency rule (the outputs are
 * then undefined); the main kernel indexes no memory with an unchecked id or end. */
int shd_route_edit_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                         int32_t nt, int64_t ld, uint32_t flags, const uint64_t* d_wt,
                         const int64_t* d_scn_off, const int32_t* d_scn_edge, const int32_t* d_scn_a,
                         const int32_t* d_scn_b, const double* d_scn_lat, int32_t nscn, uint64_t* d_stats,
                         double* d_max_add, double* d_max_gain, double* d_min_new, double* d_lat,
                         uint64_t* d_unrouted, void* stream);
/* Same with host pointers (row stride nt); blocks.  Records in any order: each scenario is sorted
 * inside, new links first in the caller's order, then ids ascending. */
int shd_route_edit(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                   uint32_t flags, const uint64_t* wt, const int64_t* scn_off, const int32_t* scn_edge,
                   const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, int32_t nscn,
                   uint64_t* stats_out, double* max_add_out, double* max_gain_out, double* min_new_out,
                   double* lat_out, uint64_t* unrouted_out);
/* The sparse form: npairs (pair_src[p], pair_tgt[p], pair_wt[p]) in any order (pair_wt NULL =
 * 1 each); lat_out[k*npairs + p] in the caller's pair order.  Host pointers; blocks. */
int shd_route_pair_edit(shd_route_t* ctx, const int32_t* pair_src, const int32_t* pair_tgt,
                        const uint64_t* pair_wt, int64_t npairs, uint32_t flags, const int64_t* scn_off,
                        const int32_t* scn_edge, const int32_t* scn_a, const int32_t* scn_b,
                        const double* scn_lat, int32_t nscn, uint64_t* stats_out, double* max_add_out,
                        double* max_gain_out, double* min_new_out, double* lat_out, uint64_t* unrouted_out);

/* Direct-path pairs (topology.c:1877-1927) for the full src x tgt block. */
int shd_route_direct(shd_route_t* ctx, const int32_t* src, int32_t ns, const int32_t* tgt,
                     int32_t nt, double* lat_out, double* rel_out, double* row_min_out);

/* Self paths (topology.c:1545-1653) for a list of vertices. */
int shd_route_self(shd_route_t* ctx, const int32_t* v, int32_t nv, double* lat_out,
                   double* rel_out);

/* Device-wide min over `count` non-negative doubles (runahead, topology.c:1374-1385).
 * Device pointers; result written to *d_out. */
int shd_route_min_reduce_async(shd_route_t* ctx, const double* d_vals, int64_t count,
                               double* d_out, void* stream);

/* ---- planned (seeded) rows: the eager fill of many sources at once -----------------
 * Replaces the same reference work as shd_route_rows (one SOURCE(s,.) row per source,
 * topology.c:1655-1875), planned over the whole source list.  A row whose source s has
 * a neighbour u among the planned sources may start from u's finished row: distances
 * w(s,u) + d_u(v) are path lengths that already satisfy every arc, so only the vertices
 * that improve on them are expanded, and the rows come out bit-identical to unseeded
 * rows (same distances, same engine tie rule for parents, same source-first products).
 * Up to three seeds per row; a row short of neighbour seeds takes rows two hops away,
 * and the first rows of the launch take landmark rows (the most central vertices' rows,
 * computed on the host when the plan is built).  The plan orders the rows into one
 * launch, where a row waits for its seeds' ready flags, and keeps the seeding rows (u16
 * distances + parent records per vertex) in a device row store.
 * Rows of a multi-GPU job: with world > 1 this rank's output rows are whole subtrees of
 * the seed forest (shd_route_plan_rows gives their positions in the caller's list), the
 * forest's top rows recomputed on every rank as helper rows.  Plans need the KD kernel
 * on an undirected integer-latency topology (else the plan falls back to plain rows);
 * SHD_ROUTE_SEED=0 in the environment disables seeding. */
typedef struct shd_route_plan shd_route_plan_t;

typedef struct shd_route_plan_info {
    int32_t rows;          /* output rows of this rank */
    int32_t seeded;        /* 1 = seeded launches, 0 = plain rows */
    int32_t launches;      /* kernel launches per shd_route_rows_planned_async */
    int32_t levels;        /* depth of the seed forest (longest chain of seeded rows) */
    int32_t roots;         /* rows computed from scratch (no neighbour, two-hop or landmark seed) */
    int32_t helpers;       /* rows computed only to seed others (no output) */
    int32_t stored_rows;   /* rows kept in the row store */
    int32_t world, rank;
    uint64_t store_bytes;  /* device bytes of the row store */
    int32_t delta;         /* the rows' bucket width (ms; at most the context's, info.reserved) */
    int32_t pad_;
} shd_route_plan_info_t;

int shd_route_plan_create(shd_route_t* ctx, const int32_t* src, int32_t ns, int32_t world, int32_t rank,
                          shd_route_plan_t** out);
void shd_route_plan_destroy(shd_route_plan_t* plan);  /* before its context's shd_route_destroy */
int shd_route_plan_get_info(const shd_route_plan_t* plan, shd_route_plan_info_t* info);
/* positions (in the caller's source list) of this rank's output rows, in row order */
int shd_route_plan_rows(const shd_route_plan_t* plan, int32_t* pos_out);
/* this rank's rows of the plan: row r of d_lat / d_rel / d_row_min = source
 * src[pos[r]]; device pointers as shd_route_rows_async.  A landmark-only plan built on the
 * device (256-thread contexts, and ranks with few rows per workgroup slot; info.launches 4)
 * seeds every row from its nearest landmark rows (the highest-degree vertices' exact rows),
 * and this call computes those landmark rows too, on the stream, before the rows: the
 * landmark rows and the job records derived from them (each row's nearest landmarks, its
 * offsets and seed records) are recomputed in every call, so every SSSP behind the table
 * runs inside it; the queue order is the plan's, fixed when it is made.  SHD_ROUTE_PLAN_REUSE skips that and reuses the
 * last computation (the plan's creation, or shd_route_plan_refresh_async), which a caller
 * may run separately to time the rows launch alone; other plans ignore the flag. */
#define SHD_ROUTE_PLAN_REUSE 0x200u
int shd_route_rows_planned_async(shd_route_t* ctx, const shd_route_plan_t* plan, const int32_t* d_tgt,
                                 int32_t nt, int64_t ld, uint32_t flags, double* d_lat, double* d_rel,
                                 double* d_row_min, void* stream);
/* the landmark rows, queue order and job records of a device-built landmark-only plan,
 * enqueued on the stream; SHD_ROUTE_OK and nothing enqueued for other plans.  `what`:
 * SHD_ROUTE_REFRESH_ALL computes every landmark row into the plan's store,
 * SHD_ROUTE_REFRESH_MINE only this rank's share (shd_route_plan_landmarks), and
 * SHD_ROUTE_REFRESH_JOBS derives the job records from the store as it stands; 0 = ALL | JOBS, what shd_route_rows_planned_async runs first without
 * SHD_ROUTE_PLAN_REUSE.  A multi-GPU rank runs MINE, exchanges the store slots with the
 * other ranks (an all-gather of equal shares), then JOBS and the rows with
 * SHD_ROUTE_PLAN_REUSE: each landmark row is computed once per job instead of once per rank.
 * No reference equivalent (Shadow 1.14 has no multi-process path, master.c:414-416). */
#define SHD_ROUTE_REFRESH_ALL 0x1u
#define SHD_ROUTE_REFRESH_MINE 0x2u
#define SHD_ROUTE_REFRESH_JOBS 0x4u
int shd_route_plan_refresh_async(shd_route_t* ctx, const shd_route_plan_t* plan, uint32_t what, void* stream);
/* the landmark store of such a plan: nland rows of row_stride u16 distances (d_drow) and as
 * many u32 parent records (d_prow), slot k = landmark k; this rank's share is the slots
 * [first, first + count).  SHD_ROUTE_EUNSUPPORTED for other plans. */
int shd_route_plan_landmarks(const shd_route_plan_t* plan, int32_t* nland, int32_t* first, int32_t* count,
                             int64_t* row_stride);
/* moves the plan's landmark store into caller memory (nland * row_stride elements each,
 * device, kept alive by the caller for the plan's lifetime), e.g. buffers a collective
 * library can all-gather into; the current contents are copied.  Blocks. */
int shd_route_plan_bind_store(shd_route_t* ctx, shd_route_plan_t* plan, uint16_t* d_drow, uint32_t* d_prow);

/* ---- the eager fill of a dense Path cache ------------------------------------------
 * The front end's cache (shd_topology.h) replaces topology.c's hash of Paths
 * (topology.c:1284-1386) with an upper triangle over the attached vertices A (sorted):
 * pair {A[i], A[j]}, i <= j, holds the Path of row i (first writer wins over both
 * directions under ascending sources, topology.c:1307-1336) as interleaved (lat, rel)
 * doubles at lr_out + 2 * (i * na - i * (i - 1) / 2 + (j - i)).  This fills the rows this
 * rank owns (world/rank: the plan's partition; world 1: all) with one seeded plan: rows
 * on the device, packed into the triangle layout and copied out in 512 MiB chunks on a
 * second stream while the next chunk packs.  lr_out is host memory, pinned for full
 * PCIe rate when it comes from shd_route_host_alloc.  *min_out = the smallest latency
 * written (topology.c:1374-1385), *seconds_out = the wall time (nullable).  Flags as
 * shd_route_rows (SHD_ROUTE_DISPATCH for the topology.c:2019 dispatch).  The rank's rows
 * are held whole in HBM (2 x 8 x rows x na bytes + 2 GiB; C4 on one GPU: 41 GB): a
 * larger request is SHD_ROUTE_ENOMEM (shard it over more devices).
 *
 * SHD_ROUTE_FILL_STAGE in the environment (tests: many stage chunks and reused staging
 * buffers on a small triangle) sets the pairs per staging buffer: unset, empty, not a
 * number or <= 0 keeps the default 32 Mi (512 MiB per buffer); the value in effect is never
 * below one whole row (na pairs; ceil(na / 6) lines in the compact layout) and is rounded
 * up to a multiple of 4, and the two staging allocations and the free-memory guard
 * (2 x table + 4 x 8 x stage pairs + 1 GiB) use it.  The schedule itself -- stage chunks,
 * buffers, copy pieces -- is the pure host function of shadow_amd/csrc/fill_sched.hpp.
 *
 * With SHD_ROUTE_FILL_LAT16 in flags the triangle is the compact layout instead (10.7 B per
 * pair against 16): row i starts a 64-byte line at line shd_route_tri16_line(na, i), and
 * its pairs j >= i go six to a line, pair e = j - i in line row_start + e / 6 at slot
 * e % 6 -- the line holds rel as 6 doubles (bytes 0-47), then lat as 6 u16 (bytes 48-59,
 * 0xFFFF = NaN), 4 pad bytes; a lookup is still one cache line.  Exact only when every
 * latency written is an integer below 0xFFFF (info.lat16, and the caller's direct-path
 * and self-path latencies): else SHD_ROUTE_EUNSUPPORTED.  lr_out then points at
 * 64 * shd_route_tri16_line(na, na) bytes (16-byte aligned). */
#define SHD_ROUTE_FILL_LAT16 0x100u
int shd_route_fill_triangle(shd_route_t* ctx, const int32_t* A, int32_t na, int32_t world, int32_t rank,
                            uint32_t flags, double* lr_out, double* min_out, double* seconds_out);

/* first 64-byte line of row i in the SHD_ROUTE_FILL_LAT16 triangle (i = na: the line count):
 * sum over r < i of ceil((na - r) / 6) */
static inline int64_t shd_route_tri16_line(int32_t na, int32_t i) {
    /* sum of (na - r) over r < i, plus the pads (6 - (na - r) % 6) % 6: period 6, sum 15 */
    int64_t pairs = (int64_t)i * na - (int64_t)i * (i - 1) / 2;
    int64_t pad = (int64_t)(i / 6) * 15;
    for (int32_t t = 0; t < i % 6; t++) pad += (6 - ((na - t) % 6 + 6) % 6) % 6;
    return (pairs + pad) / 6;
}
/* ---- multi-GPU table assembly payload (no reference equivalent: Shadow 1.14 is one
 * process, master.c:414-416).  The Path cache needs each unordered pair once
 * (topology.c:1307-1336: the first writer stores both directions), so the rows a rank
 * sends to the others are their upper triangles: row r of d_lat / d_rel (row stride ld,
 * na targets = the sorted attached list) is the row of attached position d_pos[r] and
 * keeps the targets j >= d_pos[r], packed at element offset d_off[r] - d_off[0] of
 * d_out_lat / d_out_rel (d_off: int64 per row, the caller's prefix sums of na - pos).
 * With SHD_ROUTE_PAYLOAD_LAT16 latencies go out as u16 (exact: integer latencies whose
 * shortest paths are below 65535 ms, proven at create, and integer self-loops below 65535
 * ms -- info.lat16; NaN -> 0xFFFF, which no latency takes; else SHD_ROUTE_EUNSUPPORTED),
 * otherwise as f64; rel always as f64.  C4 over 8 GPUs: 10 B
 * per pair of the triangle instead of 16 B per pair of the square (0.31x the bytes). */
#define SHD_ROUTE_PAYLOAD_LAT16 0x1u
int shd_route_tri_payload_async(shd_route_t* ctx, const double* d_lat, const double* d_rel, int64_t ld,
                                const int32_t* d_pos, const int64_t* d_off, int32_t nrows, int32_t na, uint32_t flags,
                                void* d_out_lat, double* d_out_rel, void* stream);

/* Pinned host memory (NULL on failure), for lr_out above: huge-page-advised anonymous
 * memory first-touched in 256 MiB chunks by background threads.  shd_route_host_alloc
 * returns once the whole buffer is touched and registered with HIP as ONE registration
 * (any copy may span it; hipHostMalloc if the registration fails).
 * shd_route_host_alloc_lazy returns at once and registers each 256 MiB chunk separately:
 * until shd_route_host_wait(p) returns, the memory may be used only as
 * shd_route_fill_triangle's lr_out (no CPU reads or writes: the workers first-touch each
 * chunk), whose copies wait for each chunk they land in -- so the fill's D2H overlaps the
 * pinning of the rest (C4's 13.3 GB triangle) instead of following it.  A caller's own
 * hipMemcpy into lazy memory must not span a 256 MiB chunk boundary (the runtime fails a
 * copy across two registrations).  shd_route_host_wait returns SHD_ROUTE_OK once every
 * chunk is settled, including a chunk the runtime refused to register (it stays pageable:
 * the fill's copies into it still complete, slower); shd_route_host_unpinned(p) waits the
 * same way and returns how many bytes of p stayed pageable (0 = all pinned; for memory not
 * from these allocators, 0).  shd_route_host_free takes either.
 *
 * SHD_ROUTE_HOST_CHUNK in the environment (tests: registration boundaries inside a small
 * triangle) replaces the 256 MiB: bytes per chunk, read when a buffer is allocated, rounded up
 * to a multiple of 2 MiB (the huge page the mapping is aligned to; 2 MiB at least); unset,
 * empty, not a number or <= 0 keeps 256 MiB.  SHD_ROUTE_REGFAIL_CHUNK=k leaves chunk k of a
 * lazy buffer unregistered, as when the runtime refuses it. */
void* shd_route_host_alloc(size_t bytes);
void* shd_route_host_alloc_lazy(size_t bytes);
int shd_route_host_wait(void* p);
int64_t shd_route_host_unpinned(void* p);
void shd_route_host_free(void* p);

/* KD liveness counters since the last reset (no reference equivalent): the longest single
 * wait, in s_sleep rounds, of the delta-stepping kernel's waves on each other -- out[0] a
 * compute wave for space in the parent-record ring, out[1] the writer wave on a reserved
 * record not yet written, out[2] a wave on a work-queue entry not yet written; out[3] 0.  A
 * stall (both sides of the ring spinning to their caps) shows as 2^22; healthy waits are
 * hundreds.  Synchronises the device; reset != 0 zeroes the counters. */
int shd_route_kd_stats(shd_route_t* ctx, uint64_t* out, int32_t reset);

/* A seeded plan's job records, in queue order (diagnostics; no reference equivalent): the
 * launch's job array as the rows kernel reads it, 64 bytes per job -- int32 row, s, store,
 * nseed, seed[3], u[3], wr[3], rec[3] (only the first nseed entries of each array mean
 * anything).  *njobs is always set; out == NULL only asks for it, a buffer of fewer than
 * 64 * *njobs bytes is SHD_ROUTE_EINVAL, an unseeded plan SHD_ROUTE_EUNSUPPORTED.
 * Synchronises the device (a device-built plan's records are those of its last refresh). */
int shd_route_plan_jobs(shd_route_t* ctx, const shd_route_plan_t* plan, int32_t* njobs, void* out,
                        int64_t out_bytes);

/* K4: all-pairs shortest latencies by blocked min-plus
 * Floyd-Warshall over all vertices, u16 on the device (kept in the context).  Integer
 * latencies with every shortest path below 65535 ms, n <= 12000, simple graphs; else
 * SHD_ROUTE_EUNSUPPORTED.  No reference equivalent: Shadow 1.14 never takes shortest
 * paths on a complete graph (topology.c:1321-1323, 2019-2021); this is the dense
 * alternative to per-source SSSP. */
int shd_route_fw_table_async(shd_route_t* ctx, void* stream);

/* SOURCE(s,.) rows (as shd_route_rows_async without dispatch: topology.c:1407-1523)
 * from the resident K4 table: lat from the table, the parent of each vertex by the
 * engine tie rule among its tight in-arcs, rel the source-first product down that
 * tree.  Same entries as shd_route_rows_async bit for bit (integer latencies).  Device
 * pointers; call shd_route_fw_table_async first (same stream or synchronised): without a
 * table SHD_ROUTE_EINVAL, or SHD_ROUTE_EUNSUPPORTED on a graph K4 does not take (a multigraph
 * among them); nothing is written either way. */
int shd_route_fw_rows_async(shd_route_t* ctx, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                            int32_t nt, int64_t ld, double* d_lat, double* d_rel, double* d_row_min,
                            void* stream);

/* Dense all-pairs shortest latencies by blocked min-plus Floyd-Warshall over all
 * vertices: d_dist is n x n (device, row-major).  Bit-exact against Dijkstra only
 * for integer-valued latencies (fl sums of subpaths are not left folds otherwise). */
int shd_route_fw_async(shd_route_t* ctx, double* d_dist, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SHD_ROUTE_H */
