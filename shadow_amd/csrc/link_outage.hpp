#pragma once
// Link outages: what the entries of a call lose when a set of edges goes down -- per scenario
// the weight whose route used a failed edge, the weight that is cut off, the weight that gets
// slower and the largest added latency, and optionally every entry's new latency.  No
// reference equivalent (Shadow 1.14 has no outage model; a user would load another topology).
//   A scenario touches a source's tree only below the failed parent arcs: every vertex outside
// those subtrees keeps its tree path, and removing edges shortens nothing, so its distance
// stands bit for bit.  The marked subtrees are repaired in place: each marked vertex is seeded
// from its unmarked in-neighbours' old distances, then pull sweeps over the marked vertices
// run until nothing changes.  Every value a sweep writes is the left fold of a real path of
// the reduced graph, f64 addition is monotone, so the fixpoint is the distance a fresh context
// of the reduced graph computes, whatever order the sweeps read in.
//   No floating-point atomic anywhere: a vertex's distance has one writer, the statistics are
// u64 adds and a u64 max on the bits of a non-negative double.  Built on path_hops.hpp as the
// loads and the loss are: the all-vertex rows, the parent arcs and the hop rows are the inputs.
#include "link_loads.hpp"
#include "outage_layout.hpp"

namespace shd {

struct DevOutage {                      // the per-element columns of a context and the scenarios
    int m, directed;
    const int* __restrict__ ea;         // the ends of every edge id
    const int* __restrict__ eb;
    const double* __restrict__ lat;     // its latency
    const int* __restrict__ srow;       // per vertex its self-loop edge ids, ascending (n + 1 offsets)
    const int* __restrict__ seid;
    const long long* __restrict__ off;  // scenario k = edge[off[k] .. off[k + 1]), ascending ids
    const int* __restrict__ edge;
    int nscn;
};

struct OutageOuts {                     // each nullable
    unsigned long long* stats;          // [nscn * SHD_ROUTE_OUTAGE_NSTAT]
    unsigned long long* max_add;        // [nscn], the bits of a non-negative f64
    double* lat;                        // [k * plane + row-of-the-entry]
    long long plane;
    unsigned long long* unrouted;
};

// is e one of the ascending ids edge[q0 .. q1)
__device__ inline bool ou_failed(const int* __restrict__ edge, long long q0, long long q1, int e) {
    while (q0 < q1) {
        const long long mid = (q0 + q1) >> 1;
        const int x = edge[mid];
        if (x < e) q0 = mid + 1;
        else if (x > e) q1 = mid;
        else return true;
    }
    return false;
}

// the list of scenario k, empty unless it lies within the ids the call handed over
__device__ inline void ou_list(const DevOutage& q, int k, long long* q0, long long* q1) {
    const long long a = q.off[k], b = q.off[k + 1], tot = q.off[q.nscn];
    const bool ok = a >= 0 && a <= b && b <= tot;
    *q0 = ok ? a : 0;
    *q1 = ok ? b : 0;
}

// One thread per scenario: the offsets rise, every id is an edge id, every list ascends.
__global__ void outage_check_kernel(DevOutage q, int* __restrict__ err) {
    const long long tot = q.off[q.nscn];
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < q.nscn; k += gridDim.x * blockDim.x) {
        const long long a = q.off[k], b = q.off[k + 1];
        if (a < 0 || a > b || b > tot || (k == 0 && a != 0)) { raise_err(err, SHD_ROUTE_EINVAL); continue; }
        int prev = -1;
        for (long long x = a; x < b; x++) {
            const int e = q.edge[x];
            if (e < 0 || e >= q.m || e < prev) { raise_err(err, SHD_ROUTE_EINVAL); break; }
            prev = e;
        }
    }
}

// Entries of source i as loads_tree_kernel takes them (the block, or with eoff the sparse
// lists; wt null = 1 per entry), tree routes only.  dist / par / hrow (row stride n): the
// all-vertex latency rows (NaN = unreached; the source's own entry is the batch self entry),
// the parent arcs and the hop rows.  The grid covers the units of U (outage_layout.hpp); a
// workgroup builds the level order when its unit's source changes.  An entry that fails in the
// graph itself raises its code and adds its weight to *unrouted in the source's first slab.
// T = u16 while n <= 65535; state (OutageLayout) in LDS (kLds) or in the slice
// ws + slot * ws_stride.  In HBM the distances, marks and level offsets bypass this CU's L1 as
// link_loads.hpp's sums do; order and aff are written and read with plain accesses on either
// side of a barrier.  lat_row0: the row of source 0's first entry in a plane of o.lat (block
// form: rows of stride ld; sparse form: 0, positions are absolute).
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void outage_repair_kernel(DevHops g, DevOutage q, OutageUnits U,
                                                          const double* __restrict__ dist,
                                                          const uint32_t* __restrict__ par,
                                                          const int* __restrict__ hrow, const int* __restrict__ src,
                                                          int ns, const int* __restrict__ tgt, int nt, long long ld,
                                                          const long long* __restrict__ eoff,
                                                          const unsigned long long* __restrict__ wt, OutageOuts o,
                                                          char* ws, size_t ws_stride, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* wsum = reinterpret_cast<int*>(smem);  // B / 64 <= 16 wave sums
    int* maxd = reinterpret_cast<int*>(smem + 64);
    int* rmin = reinterpret_cast<int*>(smem + 68);
    int* rmax = reinterpret_cast<int*>(smem + 72);
    unsigned* na = reinterpret_cast<unsigned*>(smem + 76);
    int* flag = reinterpret_cast<int*>(smem + 80);
    unsigned* nlive = reinterpret_cast<unsigned*>(smem + 84);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + 88);  // hit, cut, slower, max bits
    uint32_t* live = reinterpret_cast<uint32_t*>(smem + kOuLive);
    uint8_t* lflag = reinterpret_cast<uint8_t*>(smem + kOuFlags);
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    char* base;
    if constexpr (kLds) base = smem + kOuSmall;
    else base = ws + (size_t)blockIdx.x * ws_stride;
    const OutageLayout<T> L = OutageLayout<T>::make(n);
    unsigned long long* dnew = reinterpret_cast<unsigned long long*>(base + L.dnew);
    uint32_t* lvl = reinterpret_cast<uint32_t*>(base + L.lvl);
    T* order = reinterpret_cast<T*>(base + L.order);
    T* aff = reinterpret_cast<T*>(base + L.aff);
    uint8_t* mark = reinterpret_cast<uint8_t*>(base + L.mark);

    int cur = -1;  // the source whose level order the state holds
    int md = 0;
    for (long long unit = blockIdx.x; unit < U.units; unit += gridDim.x) {
        const int i = U.source(unit);
        if (i >= ns) break;
        const int k0 = U.first(unit), k1 = U.last(unit, q.nscn);
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (tid == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        const double* __restrict__ drow = dist + (long long)i * n;
        const uint32_t* __restrict__ prow = par + (long long)i * n;
        const int* __restrict__ hr = hrow + (long long)i * n;
        const long long e0 = eoff ? eoff[i] : 0, e1 = eoff ? eoff[i + 1] : (long long)nt;
        const long long wbase = eoff ? 0 : (long long)i * ld;
        const int se = g.self_eid[s];

        // 1. once per source: the counting sort of the reached vertices by hop depth, no marks
        if (i != cur) {
            cur = i;
            for (int v = tid; v < n; v += B) ld_put<kLds>(&mark[v], (uint8_t)0);
            for (int d = tid; d <= n; d += B) ld_put<kLds>(&lvl[d], 0u);
            if (tid == 0) { *maxd = 0; *na = 0u; }
            __syncthreads();
            int lmax = 0;
            for (int v = tid; v < n; v += B) {
                const int d = hr[v];
                if (v != s && d > 0 && d < n) {
                    (void)ld_add<kLds>(&lvl[d], 1u);
                    lmax = max(lmax, d);
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lmax = max(lmax, __shfl_xor(lmax, d, 64));
            if (lane == 0 && lmax) atomicMax(maxd, lmax);
            __syncthreads();
            md = *maxd;
            // exclusive scan of the level sizes 0 .. md: every thread a contiguous run of levels
            {
                const int per = (md + 1 + B - 1) / B;
                const int a0 = min(tid * per, md + 1), a1 = min(a0 + per, md + 1);
                int sz = 0;
                for (int k = a0; k < a1; k++) sz += (int)ld_get<kLds>(&lvl[k]);
                int incl = sz;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int y = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += y;
                }
                if (lane == 63) wsum[wv] = incl;
                __syncthreads();
                int run = incl - sz;
                for (int k = 0; k < wv; k++) run += wsum[k];
                for (int k = a0; k < a1; k++) {
                    const uint32_t c = ld_get<kLds>(&lvl[k]);
                    ld_put<kLds>(&lvl[k], (uint32_t)run);
                    run += (int)c;
                }
            }
            __syncthreads();
            // place the vertices: lvl[d] moves from the start of level d to its end, the start of d + 1
            for (int v = tid; v < n; v += B) {
                const int d = hr[v];
                if (v != s && d > 0 && d < n) order[ld_add<kLds>(&lvl[d], 1u)] = (T)v;
            }
            __syncthreads();
        }

        // the entries that fail in the graph itself: once per source
        if (k0 == 0) {
            unsigned long long lost = 0;
            for (long long x = e0 + tid; x < e1; x += B) {
                const int t = tgt[x];
                if (t < 0 || t >= n) { raise_err(err, SHD_ROUTE_EINVAL); continue; }
                const unsigned long long w = wt ? wt[wbase + x] : 1ull;
                if (t == s) {
                    if (se < 0) { raise_err(err, SHD_ROUTE_ENOEDGE); lost += w; }
                } else if (hr[t] <= 0 || hr[t] >= n) {
                    raise_err(err, SHD_ROUTE_EUNREACH);
                    lost += w;
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lost += __shfl_xor(lost, d, 64);
            if (lane == 0 && lost && o.unrouted) ld_out(o.unrouted, lost);
        }

        // 2. the slab, one thread per scenario: live where a failed edge is the parent arc of
        // one of its ends or the source's lowest self-loop
        if (tid == 0) *nlive = 0u;
        __syncthreads();
        for (int k = k0 + tid; k < k1; k += B) {
            long long q0, q1;
            ou_list(q, k, &q0, &q1);
            bool lv = false;
            for (long long x = q0; x < q1 && !lv; x++) {
                const int e = q.edge[x];
                if (e < 0 || e >= q.m) continue;
                const int a = q.ea[e], b = q.eb[e];
                if (a == b) { lv = e == se; continue; }
                const uint32_t pb = prow[b];
                lv = pb != HP_NONE && g.eid_in[pb] == e;
                if (!lv && !q.directed) {
                    const uint32_t pa = prow[a];
                    lv = pa != HP_NONE && g.eid_in[pa] == e;
                }
            }
            lflag[k - k0] = lv ? 1 : 0;
            if (lv) live[atomicAdd(nlive, 1u)] = (uint32_t)k;
        }
        __syncthreads();
        const unsigned nl = *nlive;
        // a dead scenario leaves every entry as it was
        if (o.lat && nl < (unsigned)(k1 - k0)) {
            const long long ne = e1 - e0;
            for (long long y = tid; y < ne * (k1 - k0); y += B) {
                const int kk = (int)(y / ne);
                if (lflag[kk]) continue;
                const long long x = e0 + y % ne;
                const int t = tgt[x];
                double v = NAN;
                if (t >= 0 && t < n) {
                    if (t == s) v = se >= 0 ? q.lat[se] : NAN;
                    else if (hr[t] > 0 && hr[t] < n) v = drow[t];
                }
                o.lat[(long long)(k0 + kk) * o.plane + wbase + x] = v;
            }
        }

        // 3. the live scenarios, the whole workgroup on each
        for (unsigned li = 0; li < nl; li++) {
            const int k = (int)live[li];
            long long q0, q1;
            ou_list(q, k, &q0, &q1);
            if (tid == 0) { *rmin = n; *rmax = 0; *flag = 0; }
            if (tid < 4) acc[tid] = 0ull;
            __syncthreads();
            // 3.1 mark: the roots, then top-down from the shallowest one
            for (long long x = q0 + tid; x < q1; x += B) {
                const int e = q.edge[x];
                if (e < 0 || e >= q.m) continue;
                const int a = q.ea[e], b = q.eb[e];
                if (a == b) continue;
                const uint32_t pb = prow[b];
                if (pb != HP_NONE && g.eid_in[pb] == e) {
                    ld_put<kLds>(&mark[b], (uint8_t)1);
                    atomicMin(rmin, hr[b]);
                    atomicMax(rmax, hr[b]);
                }
                if (!q.directed) {
                    const uint32_t pa = prow[a];
                    if (pa != HP_NONE && g.eid_in[pa] == e) {
                        ld_put<kLds>(&mark[a], (uint8_t)1);
                        atomicMin(rmin, hr[a]);
                        atomicMax(rmax, hr[a]);
                    }
                }
            }
            __syncthreads();
            const int d0 = max(*rmin, 1), dr = *rmax;
            unsigned before = 0;
            for (int d = d0; d <= md; d++) {
                const uint32_t beg = ld_get<kLds>(&lvl[d - 1]), end = ld_get<kLds>(&lvl[d]);
                for (uint32_t x = beg + tid; x < end; x += B) {
                    const int v = (int)order[x];
                    bool mk = ld_get<kLds>(&mark[v]) != 0;
                    if (!mk) {
                        const uint32_t arc = prow[v];
                        if (arc != HP_NONE && ld_get<kLds>(&mark[g.col_in[arc]]) != 0) {
                            mk = true;
                            ld_put<kLds>(&mark[v], (uint8_t)1);
                        }
                    }
                    if (mk) aff[atomicAdd(na, 1u)] = (T)v;
                }
                __syncthreads();
                const unsigned now = *na;
                __syncthreads();  // every thread has read the length before the next level appends
                if (d > dr && now == before) break;  // below the deepest root a level without marks ends them
                before = now;
            }
            const unsigned A = *na;
            // 3.2 seed: the best in-arc that stays, from a reached tail outside the subtrees
            for (unsigned x = tid; x < A; x += B) {
                const int v = (int)aff[x];
                double best = INFINITY;
                for (int a = g.row_in[v]; a < g.row_in[v + 1]; a++) {
                    const int u = g.col_in[a];
                    if (ld_get<kLds>(&mark[u]) != 0) continue;
                    const double du = u == s ? 0.0 : drow[u];
                    if (isnan(du)) continue;
                    const double cand = du + g.w_in[a];
                    if (cand < best && !ou_failed(q.edge, q0, q1, g.eid_in[a])) best = cand;
                }
                ld_put<kLds>(&dnew[v], as_u(best));
            }
            __syncthreads();
            // 3.3 repair: pull sweeps over the marked tails until nothing changes
            for (unsigned sweep = 0;; sweep++) {
                bool ch = false;
                for (unsigned x = tid; x < A; x += B) {
                    const int v = (int)aff[x];
                    const double old = as_d(ld_get<kLds>(&dnew[v]));
                    double best = old;
                    for (int a = g.row_in[v]; a < g.row_in[v + 1]; a++) {
                        const int u = g.col_in[a];
                        if (ld_get<kLds>(&mark[u]) == 0) continue;
                        const double cand = as_d(ld_get<kLds>(&dnew[u])) + g.w_in[a];
                        if (cand < best && !ou_failed(q.edge, q0, q1, g.eid_in[a])) best = cand;
                    }
                    if (best < old) {
                        ld_put<kLds>(&dnew[v], as_u(best));
                        ch = true;
                    }
                }
                if (ch) *flag = 1;
                __syncthreads();
                const int again = *flag;
                __syncthreads();
                if (!again) break;
                if (sweep >= A) {  // a cap, never reached: |A| sweeps settle |A| vertices
                    if (tid == 0) raise_err(err, SHD_ROUTE_EDEVICE);
                    break;
                }
                if (tid == 0) *flag = 0;
                __syncthreads();
            }
            // 3.4 the entries, and 3.5 their new latencies
            unsigned long long hit = 0, cut = 0, slow = 0, mx = 0;
            for (long long x = e0 + tid; x < e1; x += B) {
                const int t = tgt[x];
                if (t < 0 || t >= n) continue;
                const unsigned long long w = wt ? wt[wbase + x] : 1ull;
                double nw = NAN;
                if (t == s) {
                    if (se >= 0) {
                        const double old = q.lat[se];
                        nw = old;
                        if (ou_failed(q.edge, q0, q1, se)) {
                            hit += w;
                            nw = NAN;
                            for (int y = q.srow[s]; y < q.srow[s + 1]; y++)
                                if (!ou_failed(q.edge, q0, q1, q.seid[y])) { nw = q.lat[q.seid[y]]; break; }
                            if (isnan(nw)) cut += w;
                            else if (nw > old) { slow += w; mx = max(mx, as_u(nw - old)); }
                        }
                    }
                } else if (hr[t] > 0 && hr[t] < n) {
                    const double old = drow[t];
                    nw = old;
                    if (ld_get<kLds>(&mark[t]) != 0) {
                        hit += w;
                        nw = as_d(ld_get<kLds>(&dnew[t]));
                        if (isinf(nw)) { cut += w; nw = NAN; }
                        else if (nw > old) { slow += w; mx = max(mx, as_u(nw - old)); }
                    }
                }
                if (o.lat) o.lat[(long long)k * o.plane + wbase + x] = nw;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                hit += __shfl_xor(hit, d, 64);
                cut += __shfl_xor(cut, d, 64);
                slow += __shfl_xor(slow, d, 64);
                mx = max(mx, (unsigned long long)__shfl_xor(mx, d, 64));
            }
            if (lane == 0) {
                if (hit) (void)ld_add<true>(&acc[0], hit);
                if (cut) (void)ld_add<true>(&acc[1], cut);
                if (slow) (void)ld_add<true>(&acc[2], slow);
                if (mx) (void)atomicMax(&acc[3], mx);
            }
            // 3.6 unmark
            for (unsigned x = tid; x < A; x += B) ld_put<kLds>(&mark[(int)aff[x]], (uint8_t)0);
            __syncthreads();
            if (tid < SHD_ROUTE_OUTAGE_NSTAT) {
                if (o.stats && acc[tid]) ld_out(o.stats + (long long)k * SHD_ROUTE_OUTAGE_NSTAT + tid, acc[tid]);
            } else if (tid == SHD_ROUTE_OUTAGE_NSTAT) {
                if (o.max_add && acc[3]) (void)atomicMax(o.max_add + k, acc[3]);
                *na = 0u;
            }
            __syncthreads();
        }
        __syncthreads();  // the live list goes to the next unit only when every thread is through
    }
}

}  // namespace shd
