/*
 * shd_topology.h -- C front end with the semantics of Shadow 1.14's
 * src/main/routing/topology.c (mckerrigan/shadow), keyed by vertex index.
 *
 * Shadow's own topology.c keeps its public API (topology.h:17-28) and its
 * Address->vertex map (virtualIP, topology.c:1388-1405); each public function then
 * becomes a one-line call into this module.  Behind it:
 *   - graphml loading with igraph_read_graph_graphml numbering (document order,
 *     missing numeric attribute = NaN) and the validation of topology.c:565-1185;
 *   - the Path cache as dense upper-triangle arrays over the attached vertices,
 *     filled eagerly (ascending sources, first writer wins over both directions,
 *     topology.c:1307-1336) by the HIP engine (include/shd_route.h) on the first
 *     cache miss, optionally sharded over several GPUs;
 *   - minimumPathLatency and the runahead it implies (topology.c:1374-1385,
 *     master.c:148-159).
 * Functions returning int use SHD_ROUTE_* codes; getters return -1 on error like
 * topology_getLatency / topology_getReliability (topology.c:2065-2087).
 */
#ifndef SHD_TOPOLOGY_H
#define SHD_TOPOLOGY_H

#include <stdint.h>
#include <stdio.h>

#include "shd_route.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shd_topology shd_topology_t;

/* graphml -> igraph-numbered arrays (plain or .xz/.gz file).  On success the caller
 * owns *out (release with shd_graphml_free). Validation as topology.c:565-1185;
 * returns SHD_ROUTE_EINVAL with a message in errbuf on failure. */
enum { SHD_VATTR_IP, SHD_VATTR_CITYCODE, SHD_VATTR_COUNTRYCODE, SHD_VATTR_GEOCODE, SHD_VATTR_TYPE, SHD_VATTR_N };
typedef struct shd_graphml {
    shd_graph_t graph;         /* arrays owned by this struct */
    char** vertex_ids;         /* graphml node id of each vertex */
    double* bandwidth_down;    /* vertex attributes Shadow reads at attach time */
    double* bandwidth_up;
    int32_t has_vertex_packetloss;
    /* string vertex attributes ip, citycode, countrycode, geocode, type (SHD_VATTR_*):
     * has = the key is declared for nodes; values as igraph holds them (key default or
     * "" where a node has no <data>); NULL arrays when the key is not declared */
    int32_t has_vertex_str[SHD_VATTR_N];
    char** vertex_str[SHD_VATTR_N];
    /* the jitter edge attribute (topology.c:1105-1114: validated, then unused), per edge id: NULL
     * when no jitter key is declared for edges, NaN where an edge has no value and the key has no
     * default */
    double* edge_jitter;
} shd_graphml_t;
int shd_graphml_load(const char* path, shd_graphml_t* out, char* errbuf, size_t errlen);
void shd_graphml_free(shd_graphml_t* g);

/* topology_new (topology.c:2486-2510): load, validate, make one engine context per
 * device in `devices` (NULL/0 -> device 0).  NULL on failure. */
shd_topology_t* shd_topology_new(const char* graph_path, const int* devices, int ndev);
shd_topology_t* shd_topology_new_from_graph(const shd_graph_t* g, const int* devices, int ndev);
void shd_topology_free(shd_topology_t* top);  /* topology_free (topology.c:2441) */

int32_t shd_topology_vertex_count(const shd_topology_t* top);
int32_t shd_topology_edge_count(const shd_topology_t* top);  /* edge ids are 0 .. count - 1, document order */
int32_t shd_topology_find_vertex(const shd_topology_t* top, const char* graphml_id);

/* topology_attach's effect on routing (topology.c:2371-2439): the vertex joins
 * verticesWithAttachedHosts; detach never shrinks it (topology.c:2437). */
int shd_topology_attach_vertex(shd_topology_t* top, int32_t vertex);
int32_t shd_topology_attached_count(const shd_topology_t* top);

/* Host attachment: _topology_findAttachmentVertex (topology.c:2245-2366) with its
 * per-vertex filter hook (topology.c:2094-2216) and longest-prefix match
 * (topology.c:2218-2243).  The index interns each vertex's parsed IP and case-folded
 * codes once, with posting lists per code and sorted IPs, so a lookup touches only the
 * candidates of the chosen list instead of making 5 igraph string-attribute lookups
 * per vertex.  Hints may be NULL.
 * next_double(ctx) is called exactly where the reference calls
 * random_nextDouble(randomSourcePool) (one draw, only when no longest-prefix match is
 * used), so a caller passing Shadow's Random keeps its stream bit for bit.
 * Returns the vertex index, or -1 (no vertices / bad arguments). */
typedef struct shd_attach shd_attach_t;
typedef double (*shd_next_double_fn)(void* ctx);
int shd_attach_create(shd_attach_t** out, const shd_graphml_t* g);
int32_t shd_attach_find_vertex(const shd_attach_t* a, shd_next_double_fn next_double, void* ctx,
                               const char* ip_hint, const char* citycode_hint, const char* countrycode_hint,
                               const char* geocode_hint, const char* type_hint);
void shd_attach_destroy(shd_attach_t* a);

/* topology_attach (topology.c:2371-2439) for a topology loaded from graphml: pick the
 * vertex as above, attach it, return the vertex (-1 on error) and, when the out
 * pointers are non-NULL, its bandwidths truncated to integers like (guint64) casts. */
int32_t shd_topology_attach(shd_topology_t* top, shd_next_double_fn next_double, void* ctx,
                            const char* ip_hint, const char* citycode_hint, const char* countrycode_hint,
                            const char* geocode_hint, const char* type_hint,
                            uint64_t* bw_down_out, uint64_t* bw_up_out);

/* Public accessors (topology.c:2053-2092); fill the cache on the first miss. */
double shd_topology_get_latency(shd_topology_t* top, int32_t src, int32_t dst);
double shd_topology_get_reliability(shd_topology_t* top, int32_t src, int32_t dst);
int shd_topology_is_routable(shd_topology_t* top, int32_t src, int32_t dst);
void shd_topology_increment_path_packet_counter(shd_topology_t* top, int32_t src, int32_t dst);
/* many packets of one pair at once: the same counter (its u32 word and the spill past 2^32) as
 * that many increments (no reference equivalent) */
void shd_topology_add_path_packets(shd_topology_t* top, int32_t src, int32_t dst, uint64_t packets);
uint64_t shd_topology_get_path_packet_count(shd_topology_t* top, int32_t src, int32_t dst);
int shd_topology_is_direct_path(shd_topology_t* top, int32_t src, int32_t dst);

/* minimumPathLatency over all cached Paths and the runahead it sets (ns). */
double shd_topology_min_path_latency(shd_topology_t* top);
uint64_t shd_topology_runahead_ns(shd_topology_t* top);

/* Explicit eager fill (otherwise done by the first accessor); seconds spent in
 * *elapsed_s (nullable), like shortestPathTotalTime (topology.c:1751-1788). */
int shd_topology_fill(shd_topology_t* top, double* elapsed_s);
/* Host bytes of the current fill's triangle (0 before the first fill): 16 per pair
 * (interleaved lat/rel doubles) or the compact layout of shd_route_fill_triangle
 * (SHD_ROUTE_FILL_LAT16, 64 bytes per six pairs of a row), chosen at creation when every
 * stored latency is an integer below 0xFFFF (env SHD_TOPOLOGY_LAT16=0 keeps the doubles). */
uint64_t shd_topology_triangle_bytes(shd_topology_t* top);

/* _topology_logAllCachedPaths (topology.c:1929-1967): one line per cached Path. */
int shd_topology_dump_paths(shd_topology_t* top, FILE* out);

/* ---- the routes behind the cached Paths ------------------------------------------------
 * What _topology_computeSourcePaths logs for every path it computes (topology.c:1829-1844):
 *   shortest path A<-->B (i<-->j) is L ms with P loss, path: A<--[lat,loss]-->X<--[lat,loss]-->B
 * ("-->" and "--" on directed graphs; names are graphml ids, or decimal vertex indices for
 * shd_topology_new_from_graph topologies, as in shd_topology_dump_paths).  These calls run
 * on engine 0 under the topology lock (shd_route_paths: the sources' SSSP again), compute on
 * demand and cache nothing: diagnostic rate, not per packet.  They change neither the fill
 * nor the cache nor what any accessor above returns. */

/* The route of the stored Path of {src, dst}, in the stored orientation (from the lower
 * attached vertex to the higher, as shd_topology_is_direct_path takes it): hops + 1
 * vertices into vert and hops edge ids into edge when cap >= hops + 1 (else nothing is
 * written).  Returns hops, or -1 as the getters do (not attached, never stored) and for a
 * self pair without a self-loop, whose stored Path is the path to self
 * (topology.c:1545-1653), not a route of the graph's edges. */
int32_t shd_topology_get_path(shd_topology_t* top, int32_t src, int32_t dst, int32_t* vert, int32_t* edge,
                              int32_t cap);
/* The line above for that Path into buf (snprintf-style: at most len - 1 characters and a
 * NUL; returns the full length, -1 on error). */
int shd_topology_format_path(shd_topology_t* top, int32_t src, int32_t dst, char* buf, size_t len);
/* One such line per cached pair that came from source paths, in triangle order (the order
 * of shd_topology_dump_paths): direct-dispatch pairs (topology.c:2019-2031) and self pairs
 * resolved as the path to self are left out.  Routes are fetched a block of source rows at
 * a time. */
int shd_topology_dump_routes(shd_topology_t* top, FILE* out);
/* The formatter alone, a pure host function (route_fmt.c): vert = the nv >= 1 vertices of
 * the path, hop_lat / hop_rel = latency and reliability of its nv - 1 edges, lat / rel =
 * the Path's totals, names = graphml ids indexed by vertex (NULL, or a NULL entry: the
 * decimal index).  The text goes to *buf, a malloc buffer of *cap bytes (NULL / 0 to
 * start) that is grown with realloc and stays the caller's to free; returns its length
 * without the NUL, -1 on a bad argument or allocation failure. */
int64_t shd_topology_route_line(char** buf, size_t* cap, char* const* names, const int32_t* vert, int32_t nv,
                                const double* hop_lat, const double* hop_rel, double lat, double rel,
                                int directed);

/* ---- link loads: the traffic of every link and every router ------------------------------
 * No reference equivalent: Shadow 1.14 counts packets per cached Path (path.c:57-60,
 * shd_topology_dump_paths), not per link.  These calls put every cached pair's packet count
 * on the route of its stored Path (shd_route_pair_loads in shd_route.h).  Like the route
 * calls above they run on engine 0 under the topology lock, compute on demand, cache nothing
 * and change no accessor. */

/* Per-link and per-router packet totals of the cached Paths' counters: every cached pair with
 * a non-zero packet count, in its stored orientation (lower attached vertex -> higher), with
 * the dispatch the cache used.  edge_packets[n_edges] = packets over each edge id,
 * transit_packets[n_vertices] = packets through each vertex as an intermediate hop,
 * *unrouted = packets of self pairs stored as the path to self (no self-loop), which is not
 * a route of the graph's edges; each may be NULL.  Counts past 2^32 stay exact.  Before the
 * first fill every total is zero. */
int shd_topology_link_loads(shd_topology_t* top, uint64_t* edge_packets, uint64_t* transit_packets,
                            uint64_t* unrouted);
/* The same pairs, counters and dispatch with every pair's packets split evenly over all of its
 * shortest paths (shd_route_pair_ecmp_loads: what equal-cost multipath routers would carry), in
 * double; *unrouted stays an exact integer.  Same rules: engine 0, nothing cached, every total
 * zero before the first fill; each output may be NULL. */
int shd_topology_ecmp_link_loads(shd_topology_t* top, double* edge_packets, double* transit_packets,
                                 uint64_t* unrouted);
/* The same pairs, counters, stored orientation and dispatch with the packets thinned out by the
 * loss of every link and vertex on the route (shd_route_pair_loss in shd_route.h), in double:
 * edge_reach[n_edges] = the packets expected to reach each edge id, edge_drop[n_edges] = those it
 * drops, vertex_drop[n_vertices] = those each vertex drops as a source or a target,
 * delivered[n_vertices] = those that arrive; *unrouted stays an exact integer.  A Path's counter
 * holds the packets of both directions of its pair, and all of them are attributed in the
 * stored orientation (lower attached vertex -> higher): the higher vertex's sends count as
 * sent by the lower one, and on a directed graph over the lower -> higher route.  Same rules:
 * engine 0, nothing cached, every total zero before the first fill; each output may be NULL. */
int shd_topology_link_loss(shd_topology_t* top, double* edge_reach, double* edge_drop, double* vertex_drop,
                           double* delivered, uint64_t* unrouted);
/* What the same pairs and counters (stored orientation, the counter as the weight) lose when
 * links go down: scenario k fails the edge ids scn_edge[scn_off[k] .. scn_off[k+1]), in any
 * order (shd_route_pair_outage in shd_route.h).  stats[nscn * SHD_ROUTE_OUTAGE_NSTAT] = per
 * scenario the packets whose route used a failed link, those cut off and those that get
 * slower; max_add[nscn] = the largest added latency; *unrouted = the packets of pairs without a
 * route in the whole graph.  The outage calls judge tree routes only: a topology whose cache
 * dispatches (a complete graph, or prefer-direct) returns SHD_ROUTE_EUNSUPPORTED.  An id outside
 * [0, n_edges) is SHD_ROUTE_EINVAL, nothing written.  Same rules: engine 0 under the lock,
 * nothing cached, every total zero before the first fill; each output may be NULL. */
int shd_topology_link_outage(shd_topology_t* top, const int64_t* scn_off, const int32_t* scn_edge, int32_t nscn,
                             uint64_t* stats, double* max_add, uint64_t* unrouted);
/* What the same pairs and counters gain or lose when links get other latencies: scenario k puts
 * scn_lat[x] on the edge id scn_edge[x] for x in scn_off[k] .. scn_off[k+1]), in any order
 * (shd_route_pair_reprice in shd_route.h).  stats[nscn * SHD_ROUTE_REPRICE_NSTAT] = per scenario
 * the packets whose route used a repriced link, those that get slower and those that get faster;
 * max_add[nscn] and max_gain[nscn] = the largest added and the largest gained latency;
 * min_new[nscn] = the smallest new latency over the counted pairs, the runahead window they would
 * give (+inf without a counted pair); *unrouted = the packets of pairs without a route in the
 * whole graph.  Tree routes only: a topology whose cache dispatches (a complete graph, or
 * prefer-direct) returns SHD_ROUTE_EUNSUPPORTED.  An id outside [0, n_edges), an id repeated in a
 * scenario or a latency that is not finite and > 0 is SHD_ROUTE_EINVAL, nothing written.  Same
 * rules: engine 0 under the lock, nothing cached, stats and maxima zero and min_new +inf before
 * the first fill; each output may be NULL. */
int shd_topology_link_reprice(shd_topology_t* top, const int64_t* scn_off, const int32_t* scn_edge,
                              const double* scn_lat, int32_t nscn, uint64_t* stats, double* max_add,
                              double* max_gain, double* min_new, uint64_t* unrouted);
/* What the same pairs and counters gain or lose when links are removed, repriced and added in one
 * scenario: the records (scn_edge[x], scn_a[x], scn_b[x], scn_lat[x]) of shd_route_pair_edit in
 * shd_route.h, in any order -- an edge id with a finite latency reprices it, with +inf removes it,
 * the id -1 adds a link between scn_a[x] and scn_b[x].  stats[nscn * SHD_ROUTE_EDIT_NSTAT] = per
 * scenario the packets whose route used a removed or repriced link, those that are cut off, those
 * that get slower and those that get faster; max_add, max_gain, min_new and *unrouted as for
 * shd_topology_link_reprice.  The counted pairs are taken in the stored orientation (lower ->
 * higher vertex).  Same rules: a dispatching cache is SHD_ROUTE_EUNSUPPORTED, whatever
 * shd_route_pair_edit refuses as SHD_ROUTE_EINVAL is refused here with nothing written (before the
 * first fill too; a repeated id costs a sort of the scenario's ids), engine 0 under the lock,
 * nothing cached, stats and maxima zero and min_new +inf before the first fill; each output may
 * be NULL.  "Nothing written" covers SHD_ROUTE_EINVAL only: the absorbed-latency refusal
 * (SHD_ROUTE_EUNSUPPORTED) comes from the engine call, which needs counted pairs, and arrives
 * after the outputs were set to zero and +inf, as for shd_topology_link_reprice. */
int shd_topology_link_edit(shd_topology_t* top, const int64_t* scn_off, const int32_t* scn_edge,
                           const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, int32_t nscn,
                           uint64_t* stats, double* max_add, double* max_gain, double* min_new,
                           uint64_t* unrouted);
/* ---- path folds: a per-link quantity along the stored Paths ---------------------------------
 * No reference equivalent (shd_route_pair_fold in shd_route.h).  Like the route calls above
 * these run on engine 0 under the topology lock, compute on demand (diagnostic rate), cache
 * nothing and change no accessor. */

/* The graphml's jitter edge attribute, n_edges doubles in edge-id order (NaN where an edge has no
 * value and the key no default).  SHD_ROUTE_EUNSUPPORTED for a topology whose graphml declares no
 * jitter key for edges, or one made by shd_topology_new_from_graph. */
int shd_topology_edge_jitter(shd_topology_t* top, double* out);
/* out[p] = the fold op (SHD_ROUTE_FOLD_*) of edge_val[n_edges] along the route of the stored Path
 * of {src[p], dst[p]}: the stored orientation (lower attached vertex -> higher) and the dispatch
 * the cache used, exactly as shd_topology_get_path takes them.  Pairs the getters reject (not
 * attached, never stored) and self pairs stored as the path to self give NaN.  A NaN in edge_val
 * is SHD_ROUTE_EINVAL. */
int shd_topology_fold_pairs(shd_topology_t* top, int32_t op, const double* edge_val, const int32_t* src,
                            const int32_t* dst, int64_t npairs, double* out);

/* One line per edge with a non-zero total, in edge-id order:
 *   link A<-->B (i<-->j) edge E is L ms with P loss, N packets
 * ("-->" on directed graphs; A, B = the edge's ends as the graph lists them, named as in the
 * route line). */
int shd_topology_dump_link_loads(shd_topology_t* top, FILE* out);
/* The formatter alone, a pure host function (link_fmt.c): edge id, its ends a and b, its
 * latency (ms) and packet loss, the packet total; names and the growable *buf / *cap as
 * shd_topology_route_line.  Returns the length without the NUL, -1 on a bad argument or
 * allocation failure. */
int64_t shd_topology_link_line(char** buf, size_t* cap, char* const* names, int32_t edge, int32_t a, int32_t b,
                               double latency, double loss, uint64_t packets, int directed);

/* ---- tie envelope: how much of the cached reliabilities hangs on a tie-break ---------------
 * No reference equivalent.  Where several shortest paths tie on latency the reference keeps
 * the one igraph's heap order returns and the engine the one of its own rule; shd_route_ties
 * (shd_route.h) gives, per pair, the number of shortest paths and the smallest and largest
 * reliability any of them has.  These calls run it over the cache's stored off-diagonal pairs:
 * the sorted attached vertices A, pair i < j as source A[i] -> target A[j] (the orientation
 * the first writer stored), with the dispatch the cache used.  Like the link loads they run on
 * engine 0 under the topology lock, in chunks of sources, compute on demand, cache nothing and
 * change no accessor. */
typedef struct shd_tie_stats {
    uint64_t pairs;      /* stored off-diagonal pairs that have a path */
    uint64_t tied;       /* of them: more than one shortest path */
    uint64_t sensitive;  /* of them: rel_lo != rel_hi, the reliability depends on the tie rule */
    uint64_t saturated;  /* of them: the path count reached 2^64 - 1 */
    double max_spread;   /* the largest (rel_hi - rel_lo) / rel_hi; 0 without a sensitive pair */
    int32_t worst_src, worst_dst; /* the pair attaining it, the lowest (src, dst) among equals; -1, -1 */
    uint64_t worst_count;         /* its path count, */
    double worst_lo, worst_hi;    /* and bounds (0 without a sensitive pair) */
} shd_tie_stats_t;
int shd_topology_tie_stats(shd_topology_t* top, shd_tie_stats_t* out);
/* One line per sensitive pair, in (src, dst) order, then the summary line:
 *   tie A<-->B (i<-->j) has N shortest paths, reliability LO to HI, spread S
 *   ties: P pairs, T tied, S sensitive, U saturated, max spread X at (i<-->j) with N paths
 * ("-->" on directed graphs; names as in the route line; %.17g numbers; a saturated count ends
 * in '+'). */
int shd_topology_dump_ties(shd_topology_t* top, FILE* out);
/* The formatters alone, pure host functions (tie_fmt.c); names and the growable *buf / *cap
 * as shd_topology_route_line.  Return the length without the NUL, -1 on a bad argument or
 * allocation failure. */
int64_t shd_topology_tie_line(char** buf, size_t* cap, char* const* names, int32_t a, int32_t b, uint64_t count,
                              double rel_lo, double rel_hi, int directed);
int64_t shd_topology_tie_summary_line(char** buf, size_t* cap, const shd_tie_stats_t* st, int directed);

#ifdef __cplusplus
}
#endif
#endif /* SHD_TOPOLOGY_H */
