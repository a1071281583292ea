/*
 * topology_front.c -- the Path cache and public accessors of Shadow 1.14's
 * src/main/routing/topology.c, rebuilt over the HIP routing engine (shd_route.h).
 *
 * Reference behaviour kept (file:line in mckerrigan/shadow):
 *   - one Path per unordered pair, first writer wins over both directions
 *     (_topology_shouldStorePath, topology.c:1307-1336); lookups probe (s,d) then
 *     (d,s) (topology.c:1987-1990, 2033-2037).  With the fill running over attached
 *     sources in ascending order, the stored orientation of {s,t} is from min(s,t),
 *     so the cache is one upper triangle over the attached vertices.
 *   - dispatch complete / prefer-direct+adjacent -> direct path, else source paths
 *     (topology.c:2019-2031), self entry = batch self-loop hop;
 *   - minimumPathLatency over every stored Path (topology.c:1374-1385) and the
 *     runahead it implies, truncated to whole ms (master.c:148-159, 10 ms default);
 *   - -1 from the getters when a vertex has no attached host (topology.c:1973-1985);
 *   - verticesWithAttachedHosts never shrinks on detach (topology.c:2437).
 * What changes: the cache is dense (|A|(|A|+1)/2 latency + reliability doubles
 * instead of a glib hash of 48-byte Paths), it is filled eagerly at the first miss
 * by batched GPU rows (instead of one serialised igraph Dijkstra per missing source,
 * topology.c:1747-1781), and the fill can shard sources over several GPUs.
 */
#define _GNU_SOURCE
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/shd_topology.h"

typedef struct {
    uint64_t key;    /* triangle index + 1, 0 = empty */
    uint64_t val;
} pcslot;
typedef struct {
    pthread_mutex_t lock;
    pcslot* s;       /* key and count in one slot: one cache miss per probe */
    size_t cap, len;
} __attribute__((aligned(64))) pcmap;  /* one stripe per cache line: no false sharing */

#define PC_STRIPES 64
static inline unsigned pc_stripe(uint64_t key) { return (unsigned)((key * 0xD6E8FEB86659FD93ull) >> 58); }

/* One fill of the Path cache over the attached set of its time.  Published to readers
 * with a release store and never changed or freed while the topology lives: a late
 * attach retires it (readers still holding it stay valid) and the next lookup fills a
 * new one, carrying the packet counters over.  Lookups pay one acquire load. */
typedef struct pcache {
    int32_t na;
    int32_t* A;          /* sorted attached vertices */
    int32_t* cid;        /* vertex -> index in A, -1 = not attached */
    double* lr;          /* (lat, rel) pairs: one cache line serves both getters; or, with
                          * l16, the compact layout of shd_route.h (SHD_ROUTE_FILL_LAT16): six
                          * pairs per 64-byte line, rel f64 x 6 then lat u16 x 6 */
    int l16;
    int64_t* row16;      /* l16: first line of each row (na + 1) */
    uint32_t* cnt;       /* packet counters per pair (calloc: pages commit on first touch);
                          * each 2^32 wrap adds 2^32 to the striped spill map pc */
    double min_lat;
    pcmap pc[PC_STRIPES];  /* spill map for counters past 2^32, striped over locks */
    struct pcache* older;  /* retired fills (freed with the topology) */
} pcache;

struct shd_topology {
    shd_graphml_t gml;   /* owns the arrays when loaded from a file */
    shd_graph_t g;       /* view used by the engine */
    int owns_copy;       /* arrays copied by shd_topology_new_from_graph */
    int ndev;
    shd_route_t** eng;
    int32_t n;
    int complete, directed, prefer_direct;
    int lat16;           /* the fill may use the compact layout: every latency it stores is an
                          * integer below 0xFFFF (engine info.lat16; direct and self paths are
                          * edge latencies or twice one: 2 * max edge latency < 0xFFFF) */
    /* host adjacency for the prefer-direct isDirect flags */
    int32_t* arow;
    int32_t* acol;
    /* attached set */
    uint8_t* attached;
    int32_t nattached;
    /* dense cache over A (sorted attached vertices), upper triangle incl. diagonal */
    pcache* cache;       /* current fill (acquire/release), NULL = fill at the next lookup */
    pcache* retired;     /* the fills a late attach replaced */
    double fill_seconds;
    pthread_mutex_t lock;
    shd_attach_t* at;    /* host attachment index (graphml topologies only) */
};

static inline size_t tri(int32_t na, int32_t i, int32_t j) { /* i <= j */
    return (size_t)i * (size_t)na - ((size_t)i * (size_t)(i - 1)) / 2 + (size_t)(j - i);
}

/* the stored Path of pair (i, j), i <= j: latency (NaN = never stored) and reliability,
 * from the interleaved doubles or from the compact line layout (widened exactly) */
static inline double lat_at(const pcache* c, int32_t i, int32_t j) {
    if (c->l16) {
        const int64_t e = j - i;
        const unsigned char* line = (const unsigned char*)c->lr + 64 * (c->row16[i] + e / 6);
        const uint16_t x = ((const uint16_t*)(line + 48))[e % 6];
        return x == 0xFFFFu ? NAN : (double)x;
    }
    return c->lr[2 * tri(c->na, i, j)];
}
static inline double rel_at(const pcache* c, int32_t i, int32_t j) {
    if (c->l16) {
        const int64_t e = j - i;
        return ((const double*)((const unsigned char*)c->lr + 64 * (c->row16[i] + e / 6)))[e % 6];
    }
    return c->lr[2 * tri(c->na, i, j) + 1];
}
static inline void set_at(pcache* c, int32_t i, int32_t j, double lat, double rel) {
    if (c->l16) {
        const int64_t e = j - i;
        unsigned char* line = (unsigned char*)c->lr + 64 * (c->row16[i] + e / 6);
        ((uint16_t*)(line + 48))[e % 6] = isnan(lat) ? (uint16_t)0xFFFFu : (uint16_t)lat;
        ((double*)line)[e % 6] = rel;
        return;
    }
    c->lr[2 * tri(c->na, i, j)] = lat;
    c->lr[2 * tri(c->na, i, j) + 1] = rel;
}

static int cmp_i32(const void* a, const void* b) {
    int32_t x = *(const int32_t*)a, y = *(const int32_t*)b;
    return (x > y) - (x < y);
}

static void build_adjacency(shd_topology_t* t) {
    const shd_graph_t* g = &t->g;
    int32_t n = g->n_vertices;
    t->arow = calloc((size_t)n + 1, sizeof(int32_t));
    for (int32_t e = 0; e < g->n_edges; e++) {
        t->arow[g->edge_src[e] + 1]++;
        if (!g->directed && g->edge_src[e] != g->edge_dst[e]) t->arow[g->edge_dst[e] + 1]++;
    }
    for (int32_t v = 0; v < n; v++) t->arow[v + 1] += t->arow[v];
    t->acol = malloc(sizeof(int32_t) * ((size_t)t->arow[n] + 1));
    int32_t* fill = malloc(sizeof(int32_t) * ((size_t)n + 1));
    memcpy(fill, t->arow, sizeof(int32_t) * (size_t)n);
    for (int32_t e = 0; e < g->n_edges; e++) {
        int32_t a = g->edge_src[e], b = g->edge_dst[e];
        t->acol[fill[a]++] = b;
        if (!g->directed && a != b) t->acol[fill[b]++] = a;
    }
    free(fill);
    for (int32_t v = 0; v < n; v++) qsort(t->acol + t->arow[v], (size_t)(t->arow[v + 1] - t->arow[v]), sizeof(int32_t), cmp_i32);
}

/* _topology_verticesAreAdjacent (topology.c:1248-1264) via get_eid semantics */
static int adjacent(const shd_topology_t* t, int32_t s, int32_t d) {
    int32_t lo = t->arow[s], hi = t->arow[s + 1];
    while (lo < hi) {
        int32_t mid = (lo + hi) / 2;
        if (t->acol[mid] < d) lo = mid + 1;
        else if (t->acol[mid] > d) hi = mid;
        else return 1;
    }
    return 0;
}

#define FILL_MAX_DEV 64  /* fill worker threads (one per device context) */

static uint64_t* pc_slot(pcmap* m, uint64_t key);

static void pcache_free(pcache* c) {
    while (c) {
        pcache* o = c->older;
        free(c->A); free(c->cid); shd_route_host_free(c->lr); free(c->cnt); free(c->row16);
        for (int k = 0; k < PC_STRIPES; k++) { pthread_mutex_destroy(&c->pc[k].lock); free(c->pc[k].s); }
        free(c);
        c = o;
    }
}

static shd_topology_t* finish_new(shd_topology_t* t, const int* devices, int ndev) {
    t->n = t->g.n_vertices;
    t->ndev = ndev > 0 ? (ndev < FILL_MAX_DEV ? ndev : FILL_MAX_DEV) : 1;
    t->eng = calloc((size_t)t->ndev, sizeof(shd_route_t*));
    for (int d = 0; d < t->ndev; d++) {
        int dev = (devices && ndev > 0) ? devices[d] : 0;
        if (shd_route_create(&t->eng[d], &t->g, dev) != SHD_ROUTE_OK) {
            shd_topology_free(t);
            return NULL;
        }
    }
    shd_route_info_t info;
    shd_route_get_info(t->eng[0], &info);
    t->complete = info.is_complete;
    t->directed = info.directed;
    t->prefer_direct = info.prefer_direct;
    double maxw = 0;
    for (int32_t e = 0; e < t->g.n_edges; e++)
        if (t->g.edge_latency[e] > maxw) maxw = t->g.edge_latency[e];
    const char* e16 = getenv("SHD_TOPOLOGY_LAT16");  /* "0": keep the interleaved doubles (A/B) */
    t->lat16 = info.lat16 && 2.0 * maxw < 65535.0 && !(e16 && atoi(e16) == 0);
    t->attached = calloc((size_t)t->n, 1);
    build_adjacency(t);
    pthread_mutex_init(&t->lock, NULL);
    return t;
}

/* the counter stripes are cache-line aligned: allocate the struct that way */
static shd_topology_t* alloc_top(void) {
    const size_t sz = (sizeof(shd_topology_t) + 63) & ~(size_t)63;
    shd_topology_t* t = aligned_alloc(64, sz);
    if (t) memset(t, 0, sz);
    return t;
}

shd_topology_t* shd_topology_new(const char* graph_path, const int* devices, int ndev) {
    shd_topology_t* t = alloc_top();
    char err[512];
    if (shd_graphml_load(graph_path, &t->gml, err, sizeof(err)) != SHD_ROUTE_OK) {
        fprintf(stderr, "shd_topology_new: %s\n", err);
        free(t);
        return NULL;
    }
    t->g = t->gml.graph;
    if (shd_attach_create(&t->at, &t->gml) != SHD_ROUTE_OK) t->at = NULL;
    return finish_new(t, devices, ndev);
}

shd_topology_t* shd_topology_new_from_graph(const shd_graph_t* g, const int* devices, int ndev) {
    if (!g || g->n_vertices <= 0) return NULL;
    shd_topology_t* t = alloc_top();
    t->owns_copy = 1;
    t->g = *g;
    size_t m = (size_t)g->n_edges, n = (size_t)g->n_vertices;
    int32_t* s = malloc(sizeof(int32_t) * (m + 1));
    int32_t* d = malloc(sizeof(int32_t) * (m + 1));
    double* l = malloc(sizeof(double) * (m + 1));
    double* p = malloc(sizeof(double) * (m + 1));
    memcpy(s, g->edge_src, sizeof(int32_t) * m); memcpy(d, g->edge_dst, sizeof(int32_t) * m);
    memcpy(l, g->edge_latency, sizeof(double) * m); memcpy(p, g->edge_packetloss, sizeof(double) * m);
    t->g.edge_src = s; t->g.edge_dst = d; t->g.edge_latency = l; t->g.edge_packetloss = p;
    if (g->vertex_packetloss) {
        double* vl = malloc(sizeof(double) * n);
        memcpy(vl, g->vertex_packetloss, sizeof(double) * n);
        t->g.vertex_packetloss = vl;
    }
    return finish_new(t, devices, ndev);
}

void shd_topology_free(shd_topology_t* t) {
    if (!t) return;
    if (t->eng) for (int d = 0; d < t->ndev; d++) if (t->eng[d]) shd_route_destroy(t->eng[d]);
    free(t->eng);
    if (t->owns_copy) {
        free((void*)t->g.edge_src); free((void*)t->g.edge_dst); free((void*)t->g.edge_latency);
        free((void*)t->g.edge_packetloss); free((void*)t->g.vertex_packetloss);
    }
    shd_attach_destroy(t->at);
    shd_graphml_free(&t->gml);
    free(t->arow); free(t->acol); free(t->attached);
    pcache_free(t->cache);
    pcache_free(t->retired);
    free(t);
}

int32_t shd_topology_vertex_count(const shd_topology_t* t) { return t ? t->n : -1; }
int32_t shd_topology_edge_count(const shd_topology_t* t) { return t ? t->g.n_edges : -1; }

int32_t shd_topology_find_vertex(const shd_topology_t* t, const char* id) {
    if (!t || !id || !t->gml.vertex_ids) return -1;
    for (int32_t v = 0; v < t->n; v++)
        if (!strcmp(t->gml.vertex_ids[v], id)) return v;
    return -1;
}

int shd_topology_attach_vertex(shd_topology_t* t, int32_t v) {
    if (!t || v < 0 || v >= t->n) return SHD_ROUTE_EINVAL;
    pthread_mutex_lock(&t->lock);
    if (!t->attached[v]) {
        t->attached[v] = 1;
        t->nattached++;
        /* the next lookup refills over the grown attached set (paths do not depend on the
         * target set, so pairs already cached keep their values; their counters move over).
         * Readers still holding the old fill keep a valid one: it is retired, not freed */
        pcache* c = t->cache;
        if (c) {
            __atomic_store_n(&t->cache, (pcache*)NULL, __ATOMIC_RELEASE);
            c->older = t->retired;
            t->retired = c;
        }
    }
    pthread_mutex_unlock(&t->lock);
    return SHD_ROUTE_OK;
}

int32_t shd_topology_attach(shd_topology_t* t, shd_next_double_fn next_double, void* ctx,
                            const char* ip_hint, const char* citycode_hint, const char* countrycode_hint,
                            const char* geocode_hint, const char* type_hint,
                            uint64_t* bw_down_out, uint64_t* bw_up_out) {
    if (!t || !t->at) return -1;
    const int32_t v = shd_attach_find_vertex(t->at, next_double, ctx, ip_hint, citycode_hint, countrycode_hint,
                                             geocode_hint, type_hint);
    if (v < 0 || shd_topology_attach_vertex(t, v) != SHD_ROUTE_OK) return -1;
    /* topology.c:2394-2405: default cluster bandwidths, (guint64) casts */
    if (bw_up_out) *bw_up_out = (uint64_t)t->gml.bandwidth_up[v];
    if (bw_down_out) *bw_down_out = (uint64_t)t->gml.bandwidth_down[v];
    return v;
}

int32_t shd_topology_attached_count(const shd_topology_t* t) { return t ? t->nattached : -1; }

typedef struct {
    shd_topology_t* t;
    pcache* c;
    int dev, nd;
    int rc;
    double min_lat;
} fill_job;

/* One thread per device context: the rows its plan share owns (shd_route_fill_triangle:
 * one seeded plan, rows packed into this triangle and copied out on the device), so the
 * eager fill is one call per device instead of a batch per chunk of sources. */
static void* fill_worker(void* arg) {
    fill_job* job = arg;
    pcache* c = job->c;
    double mn = INFINITY;
    int rc = shd_route_fill_triangle(job->t->eng[job->dev], c->A, c->na, job->nd, job->dev,
                                     SHD_ROUTE_DISPATCH | (c->l16 ? SHD_ROUTE_FILL_LAT16 : 0u), c->lr, &mn, NULL);
    /* ENOEDGE: a self pair without a self-loop; that entry stays NaN, i.e. not stored by
     * the batch, as the reference skips the failed target (topology.c:1488-1495,
     * 1812-1870); fill_locked resolves it below.  EUNREACH (not after the
     * strong-connectivity check at load) leaves the pair unstored */
    if (rc && rc != SHD_ROUTE_ENOEDGE && rc != SHD_ROUTE_EUNREACH) job->rc = rc;
    job->min_lat = mn;
    return NULL;
}

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* counters of the pairs the last retired fill held, moved to fill c (after a late
 * attach every old pair is still a pair: the attached set only grows).  A reader that
 * still holds the retired fill may count into it after this pass has read a pair:
 * packet counts are approximate across a late attach (Shadow attaches every host before
 * the simulation starts, so this does not arise there).  The spill maps are read under
 * their locks, as a concurrent wrap may be growing one: every stripe is locked once for
 * the whole pass (a lock round trip per pair was O(na^2) of them). */
static void carry_counters(pcache* o, pcache* c) {
    for (int k = 0; k < PC_STRIPES; k++) pthread_mutex_lock(&o->pc[k].lock);
    for (int32_t i = 0; i < o->na; i++)
        for (int32_t j = i; j < o->na; j++) {
            const size_t ko = tri(o->na, i, j);
            uint64_t v = __atomic_load_n(&o->cnt[ko], __ATOMIC_RELAXED);
            const pcmap* m = &o->pc[pc_stripe((uint64_t)ko + 1)];
            if (m->cap) {
                size_t h = (((uint64_t)ko + 1) * 0x9E3779B97F4A7C15ull) & (m->cap - 1);
                while (m->s[h].key && m->s[h].key != (uint64_t)ko + 1) h = (h + 1) & (m->cap - 1);
                if (m->s[h].key) v += m->s[h].val;
            }
            if (!v) continue;
            int32_t a = c->cid[o->A[i]], b = c->cid[o->A[j]];
            if (a > b) { int32_t x = a; a = b; b = x; }
            const size_t k = tri(c->na, a, b);
            c->cnt[k] = (uint32_t)v;
            if (v >> 32) {
                pcmap* mm = &c->pc[pc_stripe((uint64_t)k + 1)];
                *pc_slot(mm, (uint64_t)k + 1) = v & ~(uint64_t)UINT32_MAX;
            }
        }
    for (int k = PC_STRIPES - 1; k >= 0; k--) pthread_mutex_unlock(&o->pc[k].lock);
}

static int fill_locked(shd_topology_t* t) {
    if (t->cache) return SHD_ROUTE_OK;
    const double t0 = now_s();
    pcache* c = calloc(1, sizeof(pcache));
    if (!c) return SHD_ROUTE_ENOMEM;
    for (int k = 0; k < PC_STRIPES; k++) pthread_mutex_init(&c->pc[k].lock, NULL);
    c->A = malloc(sizeof(int32_t) * ((size_t)t->nattached + 1));
    c->cid = malloc(sizeof(int32_t) * (size_t)t->n);
    if (!c->A || !c->cid) { pcache_free(c); return SHD_ROUTE_ENOMEM; }
    for (int32_t v = 0; v < t->n; v++) {
        c->cid[v] = -1;
        if (t->attached[v]) { c->cid[v] = c->na; c->A[c->na++] = v; }
    }
    const size_t ntri = (size_t)c->na * ((size_t)c->na + 1) / 2;
    c->l16 = t->lat16;
    size_t bytes = 2 * sizeof(double) * ntri;
    if (c->l16) {
        c->row16 = malloc(sizeof(int64_t) * ((size_t)c->na + 1));
        if (!c->row16) { pcache_free(c); return SHD_ROUTE_ENOMEM; }
        c->row16[0] = 0;
        for (int32_t i = 0; i < c->na; i++) c->row16[i + 1] = c->row16[i] + (c->na - i + 5) / 6;
        bytes = 64 * (size_t)c->row16[c->na];
    }
    /* pinned: the device copies its rows straight into the triangle at full PCIe rate; the
     * chunks are registered in the background while the rows run and the first chunks copy */
    c->lr = shd_route_host_alloc_lazy(bytes ? bytes : 16);
    c->cnt = calloc(ntri ? ntri : 1, sizeof(uint32_t));
    if (!c->lr || !c->cnt) { pcache_free(c); return SHD_ROUTE_ENOMEM; }
    int rc = SHD_ROUTE_OK;
    double mn_fill = INFINITY;
    if (c->na) {
        pthread_t th[FILL_MAX_DEV];
        fill_job jobs[FILL_MAX_DEV];
        int started[FILL_MAX_DEV];
        const int nd = t->ndev;  /* <= FILL_MAX_DEV (finish_new) */
        for (int d = 0; d < nd; d++) {
            jobs[d].t = t; jobs[d].c = c; jobs[d].dev = d; jobs[d].nd = nd; jobs[d].rc = 0;
            jobs[d].min_lat = INFINITY;
            started[d] = pthread_create(&th[d], NULL, fill_worker, &jobs[d]) == 0;
        }
        for (int d = 0; d < nd; d++) {
            if (started[d]) pthread_join(th[d], NULL);
            else fill_worker(&jobs[d]);  /* no thread: this device's rows inline */
            if (jobs[d].rc && !rc) rc = jobs[d].rc;
            if (jobs[d].min_lat < mn_fill) mn_fill = jobs[d].min_lat;
        }
    }
    if (!rc) rc = shd_route_host_wait(c->lr);
    if (rc) { pcache_free(c); return rc; }
    /* (s,s) pairs the batch could not store (no self-loop at s): the reference's next
     * (s,s) lookup misses and computes _topology_computeShortestPathToSelf
     * (topology.c:1674-1676, 1545-1653), i.e. 2*w_min and r_min^2 over s's out-edges */
    {
        int32_t nself = 0;
        int32_t* sv = malloc(sizeof(int32_t) * ((size_t)c->na + 1));
        for (int32_t i = 0; i < c->na; i++)
            if (isnan(lat_at(c, i, i))) sv[nself++] = c->A[i];
        if (nself) {
            double* sl = malloc(sizeof(double) * (size_t)nself);
            double* sr = malloc(sizeof(double) * (size_t)nself);
            rc = shd_route_self(t->eng[0], sv, nself, sl, sr);
            if (rc == SHD_ROUTE_ENOEDGE) rc = SHD_ROUTE_OK;  /* no out-edge: stays unstored */
            for (int32_t q = 0; q < nself && !rc; q++) {
                const int32_t ii = c->cid[sv[q]];
                set_at(c, ii, ii, sl[q], sr[q]);
                if (!isnan(sl[q]) && sl[q] < mn_fill) mn_fill = sl[q];
            }
            free(sl); free(sr);
        }
        free(sv);
        if (rc) { pcache_free(c); return rc; }
    }
    /* minimumPathLatency over every stored Path (topology.c:1374-1385; 0 = unset): the
     * fill's per-device minima over the pairs it wrote, and the self pairs above */
    c->min_lat = mn_fill < INFINITY ? mn_fill : 0;
    if (t->retired) carry_counters(t->retired, c);
    t->fill_seconds += now_s() - t0;
    __atomic_store_n(&t->cache, c, __ATOMIC_RELEASE);
    return SHD_ROUTE_OK;
}

uint64_t shd_topology_triangle_bytes(shd_topology_t* t) {
    const pcache* c = t ? __atomic_load_n(&t->cache, __ATOMIC_ACQUIRE) : NULL;
    if (!c) return 0;
    return c->l16 ? 64 * (uint64_t)c->row16[c->na] : 16 * ((uint64_t)c->na * ((uint64_t)c->na + 1) / 2);
}

int shd_topology_fill(shd_topology_t* t, double* elapsed_s) {
    if (!t) return SHD_ROUTE_EINVAL;
    pthread_mutex_lock(&t->lock);
    int rc = fill_locked(t);
    pthread_mutex_unlock(&t->lock);
    if (elapsed_s) *elapsed_s = t->fill_seconds;
    return rc;
}

/* the published fill, filling it first if needed (NULL on failure) */
static pcache* cache_of(shd_topology_t* t) {
    pcache* c = __atomic_load_n(&t->cache, __ATOMIC_ACQUIRE);
    if (c) return c;
    pthread_mutex_lock(&t->lock);
    const int rc = fill_locked(t);
    c = t->cache;
    pthread_mutex_unlock(&t->lock);
    return rc ? NULL : c;
}

/* _topology_getPathEntry (topology.c:1969-2051) -> index into the triangle of *cp, or -1;
 * *ip <= *jp its attached positions */
static int64_t entry_ij(shd_topology_t* t, int32_t s, int32_t d, pcache** cp, int32_t* ip, int32_t* jp) {
    if (!t || s < 0 || d < 0 || s >= t->n || d >= t->n) return -1;
    pcache* c = cache_of(t);
    if (!c) return -1;
    int32_t i = c->cid[s], j = c->cid[d];
    if (i < 0 || j < 0) return -1;  /* address not connected to the topology */
    if (i > j) { const int32_t x = i; i = j; j = x; }
    *cp = c; *ip = i; *jp = j;
    return isnan(lat_at(c, i, j)) ? -1 : (int64_t)tri(c->na, i, j);  /* never stored (topology.c:2040-2046) */
}
static int64_t entry(shd_topology_t* t, int32_t s, int32_t d, pcache** cp) {
    int32_t i, j;
    return entry_ij(t, s, d, cp, &i, &j);
}

double shd_topology_get_latency(shd_topology_t* t, int32_t s, int32_t d) {
    pcache* c;
    int32_t i, j;
    return entry_ij(t, s, d, &c, &i, &j) < 0 ? -1.0 : lat_at(c, i, j);
}

double shd_topology_get_reliability(shd_topology_t* t, int32_t s, int32_t d) {
    pcache* c;
    int32_t i, j;
    return entry_ij(t, s, d, &c, &i, &j) < 0 ? -1.0 : rel_at(c, i, j);
}

int shd_topology_is_routable(shd_topology_t* t, int32_t s, int32_t d) {
    return shd_topology_get_latency(t, s, d) > -1;  /* topology.c:2089-2092 */
}

int shd_topology_is_direct_path(shd_topology_t* t, int32_t s, int32_t d) {
    pcache* c;
    if (entry(t, s, d, &c) < 0) return -1;
    const int32_t a = s < d ? s : d, b = s < d ? d : s;  /* stored orientation: min -> max */
    return t->complete || (t->prefer_direct && adjacent(t, a, b));
}

static uint64_t* pc_slot(pcmap* m, uint64_t key) {
    if (m->len * 2 + 2 > m->cap) {
        size_t nc = m->cap ? m->cap * 2 : 4096;
        pcslot* ns = calloc(nc, sizeof(pcslot));
        for (size_t i = 0; i < m->cap; i++)
            if (m->s[i].key) {
                size_t j = (m->s[i].key * 0x9E3779B97F4A7C15ull) & (nc - 1);
                while (ns[j].key) j = (j + 1) & (nc - 1);
                ns[j] = m->s[i];
            }
        free(m->s);
        m->s = ns; m->cap = nc;
    }
    size_t j = (key * 0x9E3779B97F4A7C15ull) & (m->cap - 1);
    while (m->s[j].key && m->s[j].key != key) j = (j + 1) & (m->cap - 1);
    if (!m->s[j].key) { m->s[j].key = key; m->len++; }
    return &m->s[j].val;
}

/* read without inserting */
static uint64_t pc_get(pcache* c, uint64_t key) {
    const unsigned st = pc_stripe(key);
    uint64_t v = 0;
    pcmap* m = &c->pc[st];
    pthread_mutex_lock(&m->lock);
    if (m->cap) {
        size_t j = (key * 0x9E3779B97F4A7C15ull) & (m->cap - 1);
        while (m->s[j].key && m->s[j].key != key) j = (j + 1) & (m->cap - 1);
        if (m->s[j].key) v = m->s[j].val;
    }
    pthread_mutex_unlock(&m->lock);
    return v;
}

void shd_topology_increment_path_packet_counter(shd_topology_t* t, int32_t s, int32_t d) {
    pcache* c;
    int64_t k = entry(t, s, d, &c);
    if (k < 0) return;
    /* path_incrementPacketCount (path.c:57-60) without its data race: one relaxed
     * atomic add on the pair's own counter, no lock */
    if (__atomic_fetch_add(&c->cnt[k], 1u, __ATOMIC_RELAXED) != UINT32_MAX) return;
    const uint64_t key = (uint64_t)k + 1;
    const unsigned st = pc_stripe(key);
    pthread_mutex_lock(&c->pc[st].lock);
    *pc_slot(&c->pc[st], key) += 1ull << 32;
    pthread_mutex_unlock(&c->pc[st].lock);
}

void shd_topology_add_path_packets(shd_topology_t* t, int32_t s, int32_t d, uint64_t packets) {
    pcache* c;
    int64_t k = entry(t, s, d, &c);
    if (k < 0 || !packets) return;
    /* the low word on the pair's own counter, a wrap of it and the high word on the spill */
    const uint32_t lo = (uint32_t)packets;
    uint64_t hi = packets >> 32;
    if (lo && (uint64_t)__atomic_fetch_add(&c->cnt[k], lo, __ATOMIC_RELAXED) + lo > UINT32_MAX) hi++;
    if (!hi) return;
    const uint64_t key = (uint64_t)k + 1;
    const unsigned st = pc_stripe(key);
    pthread_mutex_lock(&c->pc[st].lock);
    *pc_slot(&c->pc[st], key) += hi << 32;
    pthread_mutex_unlock(&c->pc[st].lock);
}

uint64_t shd_topology_get_path_packet_count(shd_topology_t* t, int32_t s, int32_t d) {
    pcache* c;
    int64_t k = entry(t, s, d, &c);
    if (k < 0) return 0;
    return pc_get(c, (uint64_t)k + 1) + __atomic_load_n(&c->cnt[k], __ATOMIC_RELAXED);
}

double shd_topology_min_path_latency(shd_topology_t* t) {
    if (!t) return -1;
    pcache* c = cache_of(t);
    return c ? c->min_lat : -1;
}

uint64_t shd_topology_runahead_ns(shd_topology_t* t) {
    double m = shd_topology_min_path_latency(t);
    uint64_t ns = m > 0 ? ((uint64_t)m) * 1000000ull : 0;  /* master.c:153 */
    return ns > 0 ? ns : 10ull * 1000000ull;              /* master.c:138 */
}

/* ---- the routes behind the cached Paths (shd_route_paths on engine 0, nothing cached) ---- */

/* the dispatch of the stored pair a <= b (topology.c:2019-2031), as is_direct_path */
static inline int pair_direct(const shd_topology_t* t, int32_t a, int32_t b) {
    return t->complete || (t->prefer_direct && adjacent(t, a, b));
}

/* route of the stored Path of {s, d}: hops, *vp / *ep malloc'd (hops + 1 vertices, hops
 * edge ids); -1 without a route */
static int32_t route_of(shd_topology_t* t, int32_t s, int32_t d, int32_t** vp, int32_t** ep, pcache** cp,
                        int32_t* ip, int32_t* jp) {
    if (entry_ij(t, s, d, cp, ip, jp) < 0) return -1;
    const int32_t a = s < d ? s : d, b = s < d ? d : s;  /* stored orientation: min -> max */
    const int64_t cap = (int64_t)t->n + 1;               /* a path visits a vertex once ([a, a]: 2) */
    int32_t* vert = malloc(sizeof(int32_t) * (size_t)cap);
    int32_t* edge = malloc(sizeof(int32_t) * (size_t)cap);
    int64_t off[2] = { 0, 0 };
    int rc = SHD_ROUTE_ENOMEM;
    if (vert && edge) {
        pthread_mutex_lock(&t->lock);
        rc = shd_route_paths(t->eng[0], &a, &b, 1, SHD_ROUTE_DISPATCH, off, vert, edge, cap);
        pthread_mutex_unlock(&t->lock);
    }
    if (rc || off[1] < 2) {  /* (ENOEDGE: a self pair without a self-loop) */
        free(vert); free(edge);
        return -1;
    }
    *vp = vert; *ep = edge;
    return (int32_t)(off[1] - 1);
}

int32_t shd_topology_get_path(shd_topology_t* t, int32_t s, int32_t d, int32_t* vert, int32_t* edge, int32_t cap) {
    pcache* c;
    int32_t i, j, *v = NULL, *e = NULL;
    const int32_t h = route_of(t, s, d, &v, &e, &c, &i, &j);
    if (h < 0) return -1;
    if (vert && edge && cap >= h + 1) {
        memcpy(vert, v, sizeof(int32_t) * ((size_t)h + 1));
        memcpy(edge, e, sizeof(int32_t) * (size_t)h);
    }
    free(v); free(e);
    return h;
}

/* the line of one route into the growable *buf; hl / hr: scratch of at least h doubles */
static int64_t line_of(const shd_topology_t* t, const pcache* c, int32_t i, int32_t j, const int32_t* v,
                       const int32_t* e, int32_t h, double* hl, double* hr, char** buf, size_t* cap) {
    for (int32_t q = 0; q < h; q++) {
        hl[q] = t->g.edge_latency[e[q]];
        hr[q] = 1.0f - t->g.edge_packetloss[e[q]];  /* topology.c:437 */
    }
    return shd_topology_route_line(buf, cap, t->gml.vertex_ids, v, h + 1, hl, hr, lat_at(c, i, j), rel_at(c, i, j),
                                   t->directed);
}

int shd_topology_format_path(shd_topology_t* t, int32_t s, int32_t d, char* buf, size_t len) {
    pcache* c;
    int32_t i, j, *v = NULL, *e = NULL;
    const int32_t h = route_of(t, s, d, &v, &e, &c, &i, &j);
    if (h < 0) return -1;
    double* hl = malloc(sizeof(double) * 2 * ((size_t)h + 1));
    char* line = NULL;
    size_t lcap = 0;
    const int64_t k = hl ? line_of(t, c, i, j, v, e, h, hl, hl + h + 1, &line, &lcap) : -1;
    if (k >= 0 && buf && len) {
        const size_t w = (size_t)k < len - 1 ? (size_t)k : len - 1;
        memcpy(buf, line, w);
        buf[w] = 0;
    }
    free(line); free(hl); free(v); free(e);
    return k > 0x7FFFFFFF ? -1 : (int)k;
}

#define ROUTE_BLOCK_PAIRS (1 << 18)  /* pairs per shd_route_paths call of the dump (whole rows) */

int shd_topology_dump_routes(shd_topology_t* t, FILE* out) {
    if (!t || !out) return SHD_ROUTE_EINVAL;
    pcache* c = cache_of(t);
    if (!c) return SHD_ROUTE_EDEVICE;
    int rc = SHD_ROUTE_OK;
    int32_t *ps = NULL, *pt = NULL, *pi = NULL, *pj = NULL, *vert = NULL, *edge = NULL;
    int64_t* off = NULL;
    double* hl = malloc(sizeof(double) * 2 * ((size_t)t->n + 1));
    char* line = NULL;
    size_t lcap = 0, pcap = 0;
    int64_t vcap = 0;
    if (!hl) return SHD_ROUTE_ENOMEM;
    for (int32_t i0 = 0; i0 < c->na && !rc;) {
        /* the pairs of a block of rows that came from source paths */
        size_t np = 0;
        int32_t i1 = i0;
        for (; i1 < c->na && (i1 == i0 || np + (size_t)(c->na - i1) <= ROUTE_BLOCK_PAIRS); i1++) {
            if (np + (size_t)(c->na - i1) > pcap) {
                pcap = 2 * (np + (size_t)(c->na - i1));
                ps = realloc(ps, sizeof(int32_t) * pcap); pt = realloc(pt, sizeof(int32_t) * pcap);
                pi = realloc(pi, sizeof(int32_t) * pcap); pj = realloc(pj, sizeof(int32_t) * pcap);
                off = realloc(off, sizeof(int64_t) * (pcap + 1));
                if (!ps || !pt || !pi || !pj || !off) { rc = SHD_ROUTE_ENOMEM; break; }
            }
            for (int32_t j = i1; j < c->na; j++) {
                const int32_t a = c->A[i1], b = c->A[j];
                if (isnan(lat_at(c, i1, j)) || pair_direct(t, a, b)) continue;
                if (a == b && !adjacent(t, a, a)) continue;  /* the path to self (shd_route_self) */
                ps[np] = a; pt[np] = b; pi[np] = i1; pj[np] = j;
                np++;
            }
        }
        i0 = i1;
        if (rc || !np) continue;
        if (vcap < (int64_t)(8 * np + 64)) {
            vcap = (int64_t)(8 * np + 64);
            vert = realloc(vert, sizeof(int32_t) * (size_t)vcap); edge = realloc(edge, sizeof(int32_t) * (size_t)vcap);
            if (!vert || !edge) { rc = SHD_ROUTE_ENOMEM; break; }
        }
        pthread_mutex_lock(&t->lock);
        int prc = shd_route_paths(t->eng[0], ps, pt, (int64_t)np, 0u, off, vert, edge, vcap);
        if (prc == SHD_ROUTE_EINVAL && off[np] > vcap) {  /* longer routes than guessed: the size is in off */
            vcap = off[np];
            vert = realloc(vert, sizeof(int32_t) * (size_t)vcap); edge = realloc(edge, sizeof(int32_t) * (size_t)vcap);
            prc = (vert && edge) ? shd_route_paths(t->eng[0], ps, pt, (int64_t)np, 0u, off, vert, edge, vcap)
                                 : SHD_ROUTE_ENOMEM;
        }
        pthread_mutex_unlock(&t->lock);
        if (prc && prc != SHD_ROUTE_ENOEDGE && prc != SHD_ROUTE_EUNREACH) { rc = prc; break; }
        int64_t done = 0;  /* routes before k: each has one edge less than vertices */
        for (size_t k = 0; k < np; k++) {
            const int64_t nv = off[k + 1] - off[k];
            if (nv < 2) continue;
            const int64_t len = line_of(t, c, pi[k], pj[k], vert + off[k], edge + (off[k] - done), (int32_t)(nv - 1), hl,
                                        hl + t->n + 1, &line, &lcap);
            done++;
            if (len < 0) { rc = SHD_ROUTE_ENOMEM; break; }
            fwrite(line, 1, (size_t)len, out);
            fputc('\n', out);
        }
    }
    free(ps); free(pt); free(pi); free(pj); free(off); free(vert); free(edge); free(hl); free(line);
    return rc;
}

/* ---- link loads: the cached Paths' packet counters summed per edge and per vertex
 * (shd_route_pair_loads on engine 0, nothing cached) ---- */

/* every cached pair with a non-zero packet count, in its stored orientation (lower attached
 * vertex -> higher); the caller holds t->lock and frees the three lists */
static int counted_pairs(shd_topology_t* t, int32_t** ps_out, int32_t** pt_out, uint64_t** pw_out, size_t* np_out) {
    /* the counters live in the current fill, or between a late attach and the next lookup in
     * the fill it retired; before the first fill there are none */
    pcache* c = t->cache ? t->cache : t->retired;
    int rc = SHD_ROUTE_OK;
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0, pcap = 0;
    if (c) {
        /* the dense u32 counter plus its spill, the stripes locked once for the pass as
         * carry_counters locks them */
        for (int k = 0; k < PC_STRIPES; k++) pthread_mutex_lock(&c->pc[k].lock);
        for (int32_t i = 0; i < c->na && !rc; i++)
            for (int32_t j = i; j < c->na; j++) {
                const size_t k = tri(c->na, i, j);
                uint64_t v = __atomic_load_n(&c->cnt[k], __ATOMIC_RELAXED);
                const pcmap* m = &c->pc[pc_stripe((uint64_t)k + 1)];
                if (m->cap) {
                    size_t h = (((uint64_t)k + 1) * 0x9E3779B97F4A7C15ull) & (m->cap - 1);
                    while (m->s[h].key && m->s[h].key != (uint64_t)k + 1) h = (h + 1) & (m->cap - 1);
                    if (m->s[h].key) v += m->s[h].val;
                }
                if (!v) continue;
                if (np == pcap) {
                    pcap = pcap ? 2 * pcap : 1024;
                    int32_t* s2 = realloc(ps, sizeof(int32_t) * pcap);
                    if (s2) ps = s2;
                    int32_t* t2 = realloc(pt, sizeof(int32_t) * pcap);
                    if (t2) pt = t2;
                    uint64_t* w2 = realloc(pw, sizeof(uint64_t) * pcap);
                    if (w2) pw = w2;
                    if (!s2 || !t2 || !w2) { rc = SHD_ROUTE_ENOMEM; break; }
                }
                ps[np] = c->A[i]; pt[np] = c->A[j]; pw[np] = v;
                np++;
            }
        for (int k = PC_STRIPES - 1; k >= 0; k--) pthread_mutex_unlock(&c->pc[k].lock);
    }
    *ps_out = ps; *pt_out = pt; *pw_out = pw; *np_out = np;
    return rc;
}

int shd_topology_link_loads(shd_topology_t* t, uint64_t* edge_packets, uint64_t* transit_packets, uint64_t* unrouted) {
    if (!t) return SHD_ROUTE_EINVAL;
    if (edge_packets) memset(edge_packets, 0, sizeof(uint64_t) * (size_t)t->g.n_edges);
    if (transit_packets) memset(transit_packets, 0, sizeof(uint64_t) * (size_t)t->n);
    if (unrouted) *unrouted = 0;
    pthread_mutex_lock(&t->lock);
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0;
    int rc = counted_pairs(t, &ps, &pt, &pw, &np);
    if (!rc && np) {
        rc = shd_route_pair_loads(t->eng[0], ps, pt, pw, (int64_t)np, SHD_ROUTE_DISPATCH, edge_packets, transit_packets,
                                  unrouted);
        /* ENOEDGE: a self pair without a self-loop, stored as the path to self; its packets
         * are in *unrouted */
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;
    }
    pthread_mutex_unlock(&t->lock);
    free(ps); free(pt); free(pw);
    return rc;
}

/* the same pairs with every pair's packets split evenly over all of its shortest paths
 * (shd_route_pair_ecmp_loads on engine 0, nothing cached) */
int shd_topology_ecmp_link_loads(shd_topology_t* t, double* edge_packets, double* transit_packets, uint64_t* unrouted) {
    if (!t) return SHD_ROUTE_EINVAL;
    for (int32_t e = 0; edge_packets && e < t->g.n_edges; e++) edge_packets[e] = 0.0;
    for (int32_t v = 0; transit_packets && v < t->n; v++) transit_packets[v] = 0.0;
    if (unrouted) *unrouted = 0;
    pthread_mutex_lock(&t->lock);
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0;
    int rc = counted_pairs(t, &ps, &pt, &pw, &np);
    if (!rc && np) {
        rc = shd_route_pair_ecmp_loads(t->eng[0], ps, pt, pw, (int64_t)np, SHD_ROUTE_DISPATCH, edge_packets,
                                       transit_packets, unrouted);
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;  /* as above */
    }
    pthread_mutex_unlock(&t->lock);
    free(ps); free(pt); free(pw);
    return rc;
}

/* the same pairs and counters thinned out by the loss of every link and vertex on the way
 * (shd_route_pair_loss on engine 0, nothing cached) */
int shd_topology_link_loss(shd_topology_t* t, double* edge_reach, double* edge_drop, double* vertex_drop,
                           double* delivered, uint64_t* unrouted) {
    if (!t) return SHD_ROUTE_EINVAL;
    for (int32_t e = 0; e < t->g.n_edges; e++) {
        if (edge_reach) edge_reach[e] = 0.0;
        if (edge_drop) edge_drop[e] = 0.0;
    }
    for (int32_t v = 0; v < t->n; v++) {
        if (vertex_drop) vertex_drop[v] = 0.0;
        if (delivered) delivered[v] = 0.0;
    }
    if (unrouted) *unrouted = 0;
    pthread_mutex_lock(&t->lock);
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0;
    int rc = counted_pairs(t, &ps, &pt, &pw, &np);
    if (!rc && np) {
        rc = shd_route_pair_loss(t->eng[0], ps, pt, pw, (int64_t)np, SHD_ROUTE_DISPATCH, edge_reach, edge_drop,
                                 vertex_drop, delivered, unrouted);
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;  /* as above */
    }
    pthread_mutex_unlock(&t->lock);
    free(ps); free(pt); free(pw);
    return rc;
}

/* ---- link outages over the stored Paths (shd_route_pair_outage on engine 0, nothing cached) ---- */

int shd_topology_link_outage(shd_topology_t* t, const int64_t* scn_off, const int32_t* scn_edge, int32_t nscn,
                             uint64_t* stats, double* max_add, uint64_t* unrouted) {
    if (!t || nscn < 0 || (nscn && !scn_off)) return SHD_ROUTE_EINVAL;
    if (t->complete || t->prefer_direct) return SHD_ROUTE_EUNSUPPORTED;  /* the cache dispatches */
    if (nscn && (scn_off[0] != 0 || (scn_off[nscn] && !scn_edge))) return SHD_ROUTE_EINVAL;
    for (int32_t k = 0; k < nscn; k++)
        if (scn_off[k + 1] < scn_off[k]) return SHD_ROUTE_EINVAL;
    for (int64_t x = 0; nscn && x < scn_off[nscn]; x++)
        if (scn_edge[x] < 0 || scn_edge[x] >= t->g.n_edges) return SHD_ROUTE_EINVAL;
    for (int64_t k = 0; k < nscn; k++) {
        if (stats)
            for (int q = 0; q < SHD_ROUTE_OUTAGE_NSTAT; q++) stats[k * SHD_ROUTE_OUTAGE_NSTAT + q] = 0;
        if (max_add) max_add[k] = 0.0;
    }
    if (unrouted) *unrouted = 0;
    pthread_mutex_lock(&t->lock);
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0;
    int rc = counted_pairs(t, &ps, &pt, &pw, &np);
    if (!rc && np) {
        rc = shd_route_pair_outage(t->eng[0], ps, pt, pw, (int64_t)np, 0u, scn_off, scn_edge, nscn, stats, max_add,
                                   NULL, unrouted);
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;  /* as above */
    }
    pthread_mutex_unlock(&t->lock);
    free(ps); free(pt); free(pw);
    return rc;
}

/* ---- link repricing over the stored Paths (shd_route_pair_reprice on engine 0, nothing cached) ---- */

int shd_topology_link_reprice(shd_topology_t* t, const int64_t* scn_off, const int32_t* scn_edge,
                              const double* scn_lat, int32_t nscn, uint64_t* stats, double* max_add,
                              double* max_gain, double* min_new, uint64_t* unrouted) {
    if (!t || nscn < 0 || (nscn && !scn_off)) return SHD_ROUTE_EINVAL;
    if (t->complete || t->prefer_direct) return SHD_ROUTE_EUNSUPPORTED;  /* the cache dispatches */
    if (nscn && (scn_off[0] != 0 || (scn_off[nscn] && (!scn_edge || !scn_lat)))) return SHD_ROUTE_EINVAL;
    for (int32_t k = 0; k < nscn; k++)
        if (scn_off[k + 1] < scn_off[k]) return SHD_ROUTE_EINVAL;
    for (int32_t k = 0; k < nscn; k++)
        for (int64_t x = scn_off[k]; x < scn_off[k + 1]; x++) {
            if (scn_edge[x] < 0 || scn_edge[x] >= t->g.n_edges || !(scn_lat[x] > 0.0) || isinf(scn_lat[x]))
                return SHD_ROUTE_EINVAL;
            for (int64_t y = scn_off[k]; y < x; y++)
                if (scn_edge[y] == scn_edge[x]) return SHD_ROUTE_EINVAL;
        }
    for (int64_t k = 0; k < nscn; k++) {
        if (stats)
            for (int q = 0; q < SHD_ROUTE_REPRICE_NSTAT; q++) stats[k * SHD_ROUTE_REPRICE_NSTAT + q] = 0;
        if (max_add) max_add[k] = 0.0;
        if (max_gain) max_gain[k] = 0.0;
        if (min_new) min_new[k] = INFINITY;
    }
    if (unrouted) *unrouted = 0;
    pthread_mutex_lock(&t->lock);
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0;
    int rc = counted_pairs(t, &ps, &pt, &pw, &np);
    if (!rc && np) {
        rc = shd_route_pair_reprice(t->eng[0], ps, pt, pw, (int64_t)np, 0u, scn_off, scn_edge, scn_lat, nscn, stats,
                                    max_add, max_gain, min_new, NULL, unrouted);
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;  /* as above */
    }
    pthread_mutex_unlock(&t->lock);
    free(ps); free(pt); free(pw);
    return rc;
}

/* ---- link edits over the stored Paths (shd_route_pair_edit on engine 0, nothing cached) ---- */

static int edit_id_cmp(const void* a, const void* b) {
    const int32_t x = *(const int32_t*)a, y = *(const int32_t*)b;
    return (x > y) - (x < y);
}

int shd_topology_link_edit(shd_topology_t* t, const int64_t* scn_off, const int32_t* scn_edge, const int32_t* scn_a,
                           const int32_t* scn_b, const double* scn_lat, int32_t nscn, uint64_t* stats,
                           double* max_add, double* max_gain, double* min_new, uint64_t* unrouted) {
    if (!t || nscn < 0 || (nscn && !scn_off)) return SHD_ROUTE_EINVAL;
    if (t->complete || t->prefer_direct) return SHD_ROUTE_EUNSUPPORTED;  /* the cache dispatches */
    if (nscn && (scn_off[0] != 0 || (scn_off[nscn] && (!scn_edge || !scn_lat)))) return SHD_ROUTE_EINVAL;
    int64_t longest = 0;
    for (int32_t k = 0; k < nscn; k++) {
        if (scn_off[k + 1] < scn_off[k]) return SHD_ROUTE_EINVAL;
        if (scn_off[k + 1] - scn_off[k] > longest) longest = scn_off[k + 1] - scn_off[k];
    }
    /* everything that is SHD_ROUTE_EINVAL is judged here, before an output is touched and whether or
     * not a pair is counted yet; a repeated id through a sorted copy of the scenario's ids */
    int32_t* ids = longest > 1 ? malloc(sizeof(int32_t) * (size_t)longest) : NULL;
    if (longest > 1 && !ids) return SHD_ROUTE_ENOMEM;
    int bad = 0;
    for (int32_t k = 0; k < nscn && !bad; k++) {
        int64_t ni = 0;
        for (int64_t x = scn_off[k]; x < scn_off[k + 1] && !bad; x++) {
            if (scn_edge[x] < -1 || scn_edge[x] >= t->g.n_edges || !(scn_lat[x] > 0.0)) bad = 1;
            else if (scn_edge[x] == -1)
                bad = !scn_a || !scn_b || isinf(scn_lat[x]) || scn_a[x] < 0 || scn_a[x] >= t->g.n_vertices ||
                      scn_b[x] < 0 || scn_b[x] >= t->g.n_vertices || scn_a[x] == scn_b[x];
            else if (ids) ids[ni++] = scn_edge[x];
        }
        if (bad || ni < 2) continue;
        qsort(ids, (size_t)ni, sizeof(int32_t), edit_id_cmp);
        for (int64_t y = 1; y < ni && !bad; y++) bad = ids[y] == ids[y - 1];
    }
    free(ids);
    if (bad) return SHD_ROUTE_EINVAL;
    for (int64_t k = 0; k < nscn; k++) {
        if (stats)
            for (int q = 0; q < SHD_ROUTE_EDIT_NSTAT; q++) stats[k * SHD_ROUTE_EDIT_NSTAT + q] = 0;
        if (max_add) max_add[k] = 0.0;
        if (max_gain) max_gain[k] = 0.0;
        if (min_new) min_new[k] = INFINITY;
    }
    if (unrouted) *unrouted = 0;
    pthread_mutex_lock(&t->lock);
    int32_t *ps = NULL, *pt = NULL;
    uint64_t* pw = NULL;
    size_t np = 0;
    int rc = counted_pairs(t, &ps, &pt, &pw, &np);
    if (!rc && np) {
        rc = shd_route_pair_edit(t->eng[0], ps, pt, pw, (int64_t)np, 0u, scn_off, scn_edge, scn_a, scn_b, scn_lat, nscn,
                                 stats, max_add, max_gain, min_new, NULL, unrouted);
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;  /* as above */
    }
    pthread_mutex_unlock(&t->lock);
    free(ps); free(pt); free(pw);
    return rc;
}

/* ---- path folds along the stored Paths (shd_route_pair_fold on engine 0, nothing cached) ---- */

int shd_topology_edge_jitter(shd_topology_t* t, double* out) {
    if (!t || !out) return SHD_ROUTE_EINVAL;
    if (!t->gml.edge_jitter) return SHD_ROUTE_EUNSUPPORTED;
    memcpy(out, t->gml.edge_jitter, sizeof(double) * (size_t)t->g.n_edges);
    return SHD_ROUTE_OK;
}

int shd_topology_fold_pairs(shd_topology_t* t, int32_t op, const double* edge_val, const int32_t* src,
                            const int32_t* dst, int64_t npairs, double* out) {
    if (!t || !edge_val || npairs < 0 || npairs > 0x7FFFFFFF || (npairs && (!src || !dst || !out)))
        return SHD_ROUTE_EINVAL;
    if (op < SHD_ROUTE_FOLD_SUM || op > SHD_ROUTE_FOLD_PROD) return SHD_ROUTE_EINVAL;
    for (int32_t e = 0; e < t->g.n_edges; e++)
        if (isnan(edge_val[e])) return SHD_ROUTE_EINVAL;
    if (!npairs) return SHD_ROUTE_OK;
    /* the stored pairs in their stored orientation (min -> max); the rest stay NaN */
    int32_t* ps = malloc(sizeof(int32_t) * (size_t)npairs);
    int32_t* pt = malloc(sizeof(int32_t) * (size_t)npairs);
    int64_t* at = malloc(sizeof(int64_t) * (size_t)npairs);
    double* val = malloc(sizeof(double) * (size_t)npairs);
    int rc = ps && pt && at && val ? SHD_ROUTE_OK : SHD_ROUTE_ENOMEM;
    int64_t np = 0;
    for (int64_t p = 0; p < npairs && !rc; p++) {
        pcache* c;
        int32_t i, j;
        out[p] = NAN;
        if (entry_ij(t, src[p], dst[p], &c, &i, &j) < 0) continue;
        ps[np] = src[p] < dst[p] ? src[p] : dst[p];
        pt[np] = src[p] < dst[p] ? dst[p] : src[p];
        at[np++] = p;
    }
    if (!rc && np) {
        pthread_mutex_lock(&t->lock);
        rc = shd_route_pair_fold(t->eng[0], ps, pt, np, SHD_ROUTE_DISPATCH, &op, 1, edge_val, val);
        pthread_mutex_unlock(&t->lock);
        /* ENOEDGE: a self pair without a self-loop, stored as the path to self: NaN */
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;
        for (int64_t q = 0; q < np && !rc; q++) out[at[q]] = val[q];
    }
    free(ps); free(pt); free(at); free(val);
    return rc;
}

int shd_topology_dump_link_loads(shd_topology_t* t, FILE* out) {
    if (!t || !out) return SHD_ROUTE_EINVAL;
    const int32_t m = t->g.n_edges;
    uint64_t* ep = malloc(sizeof(uint64_t) * ((size_t)m + 1));
    if (!ep) return SHD_ROUTE_ENOMEM;
    int rc = shd_topology_link_loads(t, ep, NULL, NULL);
    char* line = NULL;
    size_t lcap = 0;
    for (int32_t e = 0; e < m && !rc; e++) {
        if (!ep[e]) continue;
        const int64_t len = shd_topology_link_line(&line, &lcap, t->gml.vertex_ids, e, t->g.edge_src[e], t->g.edge_dst[e],
                                                   t->g.edge_latency[e], t->g.edge_packetloss[e], ep[e], t->directed);
        if (len < 0) { rc = SHD_ROUTE_ENOMEM; break; }
        fwrite(line, 1, (size_t)len, out);
        fputc('\n', out);
    }
    free(line); free(ep);
    return rc;
}

/* ---- tie envelope over the stored off-diagonal pairs (shd_route_ties on engine 0, in chunks
 * of sources, nothing cached); `out`: also one line per sensitive pair ---- */

#define TIE_CHUNK_BYTES ((size_t)64 << 20)  /* count, rel_lo, rel_hi rows per shd_route_ties call */

static int ties_pass(shd_topology_t* t, shd_tie_stats_t* st, FILE* out) {
    memset(st, 0, sizeof *st);
    st->worst_src = st->worst_dst = -1;
    pcache* c = cache_of(t);
    if (!c) return SHD_ROUTE_EDEVICE;
    const int32_t na = c->na;
    if (na < 2) return SHD_ROUTE_OK;
    size_t rows = TIE_CHUNK_BYTES / (24 * (size_t)na);
    if (rows < 1) rows = 1;
    if (rows > (size_t)na) rows = (size_t)na;
    uint64_t* cnt = malloc(sizeof(uint64_t) * rows * (size_t)na);
    double* lo = malloc(sizeof(double) * rows * (size_t)na);
    double* hi = malloc(sizeof(double) * rows * (size_t)na);
    char* line = NULL;
    size_t lcap = 0;
    int rc = (cnt && lo && hi) ? SHD_ROUTE_OK : SHD_ROUTE_ENOMEM;
    for (int32_t i0 = 0; i0 < na - 1 && !rc; i0 += (int32_t)rows) {
        const int32_t k = (int32_t)rows < na - 1 - i0 ? (int32_t)rows : na - 1 - i0;
        pthread_mutex_lock(&t->lock);
        rc = shd_route_ties(t->eng[0], c->A + i0, k, c->A, na, SHD_ROUTE_DISPATCH, cnt, lo, hi);
        pthread_mutex_unlock(&t->lock);
        /* a self pair without a self-loop, an unreachable pair: not among the pairs counted */
        if (rc == SHD_ROUTE_ENOEDGE || rc == SHD_ROUTE_EUNREACH) rc = SHD_ROUTE_OK;
        for (int32_t i = i0; i < i0 + k && !rc; i++)
            for (int32_t j = i + 1; j < na; j++) {
                const size_t q = (size_t)(i - i0) * (size_t)na + (size_t)j;
                if (!cnt[q]) continue;
                st->pairs++;
                if (cnt[q] > 1) st->tied++;
                if (cnt[q] == UINT64_MAX) st->saturated++;
                if (lo[q] == hi[q]) continue;
                st->sensitive++;
                const double spread = (hi[q] - lo[q]) / hi[q];
                if (spread > st->max_spread) {
                    st->max_spread = spread;
                    st->worst_src = c->A[i]; st->worst_dst = c->A[j];
                    st->worst_count = cnt[q]; st->worst_lo = lo[q]; st->worst_hi = hi[q];
                }
                if (!out) continue;
                const int64_t len = shd_topology_tie_line(&line, &lcap, t->gml.vertex_ids, c->A[i], c->A[j], cnt[q], lo[q],
                                                          hi[q], t->directed);
                if (len < 0) { rc = SHD_ROUTE_ENOMEM; break; }
                fwrite(line, 1, (size_t)len, out);
                fputc('\n', out);
            }
    }
    if (!rc && out) {
        const int64_t len = shd_topology_tie_summary_line(&line, &lcap, st, t->directed);
        if (len < 0) rc = SHD_ROUTE_ENOMEM;
        else { fwrite(line, 1, (size_t)len, out); fputc('\n', out); }
    }
    free(cnt); free(lo); free(hi); free(line);
    return rc;
}

int shd_topology_tie_stats(shd_topology_t* t, shd_tie_stats_t* out) {
    if (!t || !out) return SHD_ROUTE_EINVAL;
    return ties_pass(t, out, NULL);
}

int shd_topology_dump_ties(shd_topology_t* t, FILE* out) {
    if (!t || !out) return SHD_ROUTE_EINVAL;
    shd_tie_stats_t st;
    return ties_pass(t, &st, out);
}

int shd_topology_dump_paths(shd_topology_t* t, FILE* out) {
    if (!t || !out) return SHD_ROUTE_EINVAL;
    pcache* c = cache_of(t);
    if (!c) return SHD_ROUTE_EDEVICE;
    for (int32_t i = 0; i < c->na; i++)
        for (int32_t j = i; j < c->na; j++) {
            const size_t k = tri(c->na, i, j);
            const int32_t a = c->A[i], b = c->A[j];
            const char* ia = t->gml.vertex_ids ? t->gml.vertex_ids[a] : NULL;
            const char* ib = t->gml.vertex_ids ? t->gml.vertex_ids[b] : NULL;
            char na_[32], nb_[32];
            if (!ia) { snprintf(na_, sizeof na_, "%d", a); ia = na_; }
            if (!ib) { snprintf(nb_, sizeof nb_, "%d", b); ib = nb_; }
            const uint64_t pc = pc_get(c, (uint64_t)k + 1) + __atomic_load_n(&c->cnt[k], __ATOMIC_RELAXED);
            /* path_toString (path.c:62-74) inside _topology_logAllCachedPathsHelper2 */
            fprintf(out, "Found path %s%s%s in cache: SourceIndex=%d DestinationIndex=%d Latency=%f "
                         "Reliability=%f PacketCount=%llu isDirect=%s\n",
                    ia, t->directed ? "->" : "<->", ib, a, b, lat_at(c, i, j), rel_at(c, i, j), (unsigned long long)pc,
                    (t->complete || (t->prefer_direct && adjacent(t, a, b))) ? "True" : "False");
        }
    return SHD_ROUTE_OK;
}
