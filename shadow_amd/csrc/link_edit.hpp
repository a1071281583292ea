#pragma once
// Link edits: what the entries of a call gain or lose when a scenario removes edges, gives others
// another latency and adds links that do not exist yet -- per scenario the weight whose route used
// a removed or repriced edge, the weight that is cut off, that gets slower and that gets faster,
// the largest added and gained latency, the smallest new latency, and optionally every entry's
// new latency.  No reference equivalent (a user of Shadow 1.14 would load another topology).
//   The programme is the repricing's (link_reprice.hpp) and rests on the same two
// facts: values >= D_k with d[s] = 0 stay >= D_k under every relaxation with G_k's latencies, and
// values with d[s] = 0 that every arc of G_k has relaxed are <= D_k.  A removed edge is a listed
// arc that G_k does not have: it marks the subtree below it like a repriced tree arc and is then
// skipped wherever an arc is relaxed, never added as +inf.  A new link is an arc outside the CSR:
// every propagation round relaxes every new arc of the scenario, so the round that lowers nothing
// has relaxed them all at the final values.
//   No floating-point atomic anywhere: a push is a u64 min on the bits of a non-negative double,
// the statistics are u64 adds and u64 maxima and minima on such bits.
#include "link_reprice.hpp"
#include "edit_layout.hpp"

namespace shd {

// The scenarios: r.o.off / r.o.edge / r.nlat as the repricing's, with edge -1 = a new link
// between sa[x] and sb[x] at r.nlat[x] and r.nlat[x] == +inf = edge[x] removed.  Every list
// holds its new links first, then its ids strictly ascending.
struct DevEdit {
    DevReprice r;
    const int* __restrict__ sa;
    const int* __restrict__ sb;
};

struct EditOuts {                       // each nullable
    unsigned long long* stats;          // [nscn * SHD_ROUTE_EDIT_NSTAT]
    unsigned long long* max_add;        // [nscn], the bits of a non-negative f64
    unsigned long long* max_gain;       // [nscn], likewise
    unsigned long long* min_new;        // [nscn], likewise; +inf before the first entry
    double* lat;                        // [k * plane + row-of-the-entry]
    long long plane;
    unsigned long long* unrouted;
};

// the first position of edge[q0 .. q1) (new links first, then ascending ids) that holds an id
__device__ inline long long ed_ids(const int* __restrict__ edge, long long q0, long long q1) {
    while (q0 < q1) {
        const long long mid = (q0 + q1) >> 1;
        if (edge[mid] < 0) q0 = mid + 1;
        else q1 = mid;
    }
    return q0;
}

// One thread per scenario: the offsets rise; the new links come first, each with two different
// ends that are vertices and a finite latency > 0; then the ids, each an edge id, strictly
// ascending, with a latency > 0 or +inf; and the lo / hi reduction over the new links and the
// finite latencies put on edges that are no self-loops.
__global__ void edit_check_kernel(DevEdit ed, int n, unsigned long long* __restrict__ lohi, int* __restrict__ err) {
    const DevOutage& q = ed.r.o;
    const long long tot = q.off[q.nscn];
    unsigned long long lo = kInfBits, hi = 0ull;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < q.nscn; k += gridDim.x * blockDim.x) {
        const long long a = q.off[k], b = q.off[k + 1];
        if (a < 0 || a > b || b > tot || (k == 0 && a != 0)) { raise_err(err, SHD_ROUTE_EINVAL); continue; }
        int prev = -1;
        for (long long x = a; x < b; x++) {
            const int e = q.edge[x];
            const double w = ed.r.nlat[x];
            bool ok = w > 0.0;  // false for a NaN
            bool counts = false;
            if (e == -1) {
                const int u = ed.sa[x], v = ed.sb[x];
                ok = ok && prev == -1 && !isinf(w) && u >= 0 && u < n && v >= 0 && v < n && u != v;
                counts = true;
            } else {
                ok = ok && e >= 0 && e < q.m && e > prev;
                if (ok) {
                    prev = e;
                    counts = !isinf(w) && q.ea[e] != q.eb[e];
                }
            }
            if (!ok) { raise_err(err, SHD_ROUTE_EINVAL); break; }
            if (counts) {
                lo = min(lo, as_u(w));
                hi = max(hi, as_u(w));
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, (unsigned long long)__shfl_xor(lo, d, 64));
        hi = max(hi, (unsigned long long)__shfl_xor(hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo != kInfBits) (void)atomicMin(lohi, lo);
        if (hi) (void)atomicMax(lohi + 1, hi);
    }
}

// Entries, rows and units as reprice_kernel takes them.  State (RepriceLayout) in LDS (kLds) or
// in the slice ws + slot * ws_stride, the small header of edit_layout.hpp beside it.
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void edit_kernel(DevHops g, DevEdit ed, OutageUnits U, const double* __restrict__ dist,
                                                 const uint32_t* __restrict__ par, const int* __restrict__ hrow,
                                                 const int* __restrict__ src, int ns, const int* __restrict__ tgt,
                                                 int nt, long long ld, const long long* __restrict__ eoff,
                                                 const unsigned long long* __restrict__ wt, EditOuts o, char* ws,
                                                 size_t ws_stride, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DevReprice& r = ed.r;
    const DevOutage& q = r.o;
    int* wsum = reinterpret_cast<int*>(smem);  // B / 64 <= 16 wave sums
    int* maxd = reinterpret_cast<int*>(smem + 64);
    int* rmin = reinterpret_cast<int*>(smem + 68);
    int* rmax = reinterpret_cast<int*>(smem + 72);
    unsigned* na = reinterpret_cast<unsigned*>(smem + 76);
    int* flag = reinterpret_cast<int*>(smem + 80);
    unsigned* nlive = reinterpret_cast<unsigned*>(smem + 84);
    unsigned* ntch = reinterpret_cast<unsigned*>(smem + 88);
    unsigned* nfr = reinterpret_cast<unsigned*>(smem + 92);  // the lengths of fr0 and fr1
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + kEdAcc);  // hit, cut, slower, faster, add, gain, min
    unsigned long long* oldmin = reinterpret_cast<unsigned long long*>(smem + kEdOldMin);
    uint32_t* live = reinterpret_cast<uint32_t*>(smem + kEdLive);
    uint8_t* lflag = reinterpret_cast<uint8_t*>(smem + kEdFlags);
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    char* base;
    if constexpr (kLds) base = smem + kEdSmall;
    else base = ws + (size_t)blockIdx.x * ws_stride;
    const RepriceLayout<T> L = RepriceLayout<T>::make(n);
    unsigned long long* d = reinterpret_cast<unsigned long long*>(base + L.d);
    uint32_t* lvl = reinterpret_cast<uint32_t*>(base + L.lvl);
    T* order = reinterpret_cast<T*>(base + L.order);
    T* tch = reinterpret_cast<T*>(base + L.tch);
    T* fr0 = reinterpret_cast<T*>(base + L.fr0);
    T* fr1 = reinterpret_cast<T*>(base + L.fr1);
    uint8_t* mark = reinterpret_cast<uint8_t*>(base + L.mark);
    uint32_t* tbit = reinterpret_cast<uint32_t*>(base + L.tbit);
    uint32_t* fbit = reinterpret_cast<uint32_t*>(base + L.fbit);
    const int nwords = (int)reprice_words(n);

    // one relaxation into h: the minimum on the bits, and where the value fell, h into the
    // touched list (the first time; a marked vertex is in it already) and into the frontier
    // `to` of length *nto (once per round)
    auto push = [&](int h, double cand, T* to, unsigned* nto) {
        const unsigned long long cb = as_u(cand);
        if (!(cb < ld_get<kLds>(&d[h]))) return;
        if (!(cb < ld_min<kLds>(&d[h], cb))) return;
        const uint32_t bit = 1u << (h & 31);
        if (ld_get<kLds>(&mark[h]) == 0 && !(ld_or<kLds>(&tbit[h >> 5], bit) & bit)) tch[atomicAdd(ntch, 1u)] = (T)h;
        if (!(ld_or<kLds>(&fbit[h >> 5], bit) & bit)) to[atomicAdd(nto, 1u)] = (T)h;
    };

    int cur = -1;  // the source whose level order and old row the state holds
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
        // the old distance of v as bits: 0 at the source, +inf where unreached
        auto oldbits = [&](int v) -> unsigned long long {
            if (v == s) return 0ull;
            return hr[v] > 0 && hr[v] < n ? as_u(drow[v]) : kInfBits;
        };

        // 0. once per source: the old row, clean marks and bitmaps, the counting sort of the
        // reached vertices by hop depth, the smallest old latency over the entries
        if (i != cur) {
            cur = i;
            for (int v = tid; v < n; v += B) {
                ld_put<kLds>(&mark[v], (uint8_t)0);
                ld_put<kLds>(&d[v], oldbits(v));
            }
            for (int x = tid; x < nwords; x += B) {
                ld_put<kLds>(&tbit[x], 0u);
                ld_put<kLds>(&fbit[x], 0u);
            }
            for (int x = tid; x <= n; x += B) ld_put<kLds>(&lvl[x], 0u);
            if (tid == 0) { *maxd = 0; *na = 0u; *ntch = 0u; *oldmin = kInfBits; }
            __syncthreads();
            int lmax = 0;
            for (int v = tid; v < n; v += B) {
                const int x = hr[v];
                if (v != s && x > 0 && x < n) {
                    (void)ld_add<kLds>(&lvl[x], 1u);
                    lmax = max(lmax, x);
                }
            }
            unsigned long long om = kInfBits;
            for (long long x = e0 + tid; x < e1; x += B) {
                const int t = tgt[x];
                if (t < 0 || t >= n) continue;
                if (t == s) { if (se >= 0) om = min(om, as_u(q.lat[se])); }
                else if (hr[t] > 0 && hr[t] < n) om = min(om, as_u(drow[t]));
            }
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) {
                lmax = max(lmax, __shfl_xor(lmax, x, 64));
                om = min(om, (unsigned long long)__shfl_xor(om, x, 64));
            }
            if (lane == 0 && lmax) atomicMax(maxd, lmax);
            if (lane == 0 && om != kInfBits) (void)atomicMin(oldmin, om);
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
                for (int x = 1; x < 64; x <<= 1) {
                    const int y = __shfl_up(incl, x, 64);
                    if (lane >= x) incl += y;
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
            // place the vertices: lvl[x] moves from the start of level x to its end, the start of x + 1
            for (int v = tid; v < n; v += B) {
                const int x = hr[v];
                if (v != s && x > 0 && x < n) order[ld_add<kLds>(&lvl[x], 1u)] = (T)v;
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
            for (int x = 32; x >= 1; x >>= 1) lost += __shfl_xor(lost, x, 64);
            if (lane == 0 && lost && o.unrouted) ld_out(o.unrouted, lost);
        }

        // 1. the slab, one thread per scenario: live where a listed edge is the parent arc of one
        // of its ends or the source's lowest self-loop, or improves its head at its finite new
        // latency, or a new arc improves its head
        if (tid == 0) *nlive = 0u;
        __syncthreads();
        const unsigned long long om = *oldmin;
        for (int k = k0 + tid; k < k1; k += B) {
            long long q0, q1;
            ou_list(q, k, &q0, &q1);
            bool lv = false;
            for (long long x = q0; x < q1 && !lv; x++) {
                const int e = q.edge[x];
                const double w = r.nlat[x];
                int a, b;
                bool listed = false;
                if (e == -1) {
                    a = ed.sa[x]; b = ed.sb[x];
                    if (a < 0 || a >= n || b < 0 || b >= n || a == b) continue;
                } else {
                    if (e < 0 || e >= q.m) continue;
                    a = q.ea[e]; b = q.eb[e];
                    if (a == b) { lv = e == se; continue; }
                    listed = true;
                }
                const double da = as_d(ld_get<kLds>(&d[a])), db = as_d(ld_get<kLds>(&d[b]));
                if (listed) {
                    const uint32_t pb = prow[b], pa = prow[a];
                    lv = (pb != HP_NONE && g.eid_in[pb] == e) || (!q.directed && pa != HP_NONE && g.eid_in[pa] == e);
                }
                if (!lv && !isinf(w)) lv = da + w < db || (!q.directed && db + w < da);
            }
            lflag[k - k0] = lv ? 1 : 0;
            if (lv) live[atomicAdd(nlive, 1u)] = (uint32_t)k;
            else if (o.min_new && om != kInfBits) (void)atomicMin(o.min_new + k, om);
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

        // the live scenarios, the whole workgroup on each
        for (unsigned li = 0; li < nl; li++) {
            const int k = (int)live[li];
            long long q0, q1;
            ou_list(q, k, &q0, &q1);
            const long long qn = ed_ids(q.edge, q0, q1);  // new links q0 .. qn, listed ids qn .. q1
            // the latency of edge e in G_k: its listed one (+inf: removed), else w
            auto wk = [&](int e, double w) -> double { return rp_weight(q.edge, r.nlat, qn, q1, e, w); };
            // every new arc of the scenario relaxed once
            auto new_arcs = [&](T* to, unsigned* nto) {
                for (long long x = q0 + tid; x < qn; x += B) {
                    const int a = ed.sa[x], b = ed.sb[x];
                    const double w = r.nlat[x];
                    if (q.edge[x] != -1 || a < 0 || a >= n || b < 0 || b >= n || a == b || isinf(w)) continue;
                    push(b, as_d(ld_get<kLds>(&d[a])) + w, to, nto);
                    if (!q.directed) push(a, as_d(ld_get<kLds>(&d[b])) + w, to, nto);
                }
            };
            if (tid == 0) { *rmin = n; *rmax = 0; *flag = 0; nfr[0] = 0u; nfr[1] = 0u; }
            if (tid < kEdNAcc - 1) acc[tid] = 0ull;
            if (tid == kEdNAcc - 1) acc[tid] = kInfBits;
            __syncthreads();
            // 2. mark: the roots, then top-down from the shallowest one
            for (long long x = qn + tid; x < q1; x += B) {
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
            for (int x0 = d0; x0 <= md; x0++) {
                const uint32_t beg = ld_get<kLds>(&lvl[x0 - 1]), end = ld_get<kLds>(&lvl[x0]);
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
                    if (mk) tch[atomicAdd(na, 1u)] = (T)v;
                }
                __syncthreads();
                const unsigned now = *na;
                __syncthreads();  // every thread has read the length before the next level appends
                if (x0 > dr && now == before) break;  // below the deepest root a level without marks ends them
                before = now;
            }
            const unsigned A = *na;
            if (tid == 0) *ntch = A;
            // 3. seed: the best in-arc of G_k from a tail outside the subtrees, at its old
            // distance; a removed arc is no arc of G_k
            for (unsigned x = tid; x < A; x += B) {
                const int v = (int)tch[x];
                double best = INFINITY;
                for (int a = g.row_in[v]; a < g.row_in[v + 1]; a++) {
                    const int u = g.col_in[a];
                    if (ld_get<kLds>(&mark[u]) != 0) continue;
                    const double du = as_d(ld_get<kLds>(&d[u]));
                    if (!(du < best)) continue;
                    const double w = wk(g.eid_in[a], g.w_in[a]);
                    if (isinf(w)) continue;
                    const double cand = du + w;
                    if (cand < best) best = cand;
                }
                // the tails are unmarked, so no thread reads what this one writes
                ld_put<kLds>(&d[v], as_u(best));
            }
            __syncthreads();
            // and pull sweeps over the marked tails until nothing changes
            for (unsigned sweep = 0;; sweep++) {
                bool ch = false;
                for (unsigned x = tid; x < A; x += B) {
                    const int v = (int)tch[x];
                    const double old = as_d(ld_get<kLds>(&d[v]));
                    double best = old;
                    for (int a = g.row_in[v]; a < g.row_in[v + 1]; a++) {
                        const int u = g.col_in[a];
                        if (ld_get<kLds>(&mark[u]) == 0) continue;
                        const double du = as_d(ld_get<kLds>(&d[u]));
                        if (!(du < best)) continue;
                        const double w = wk(g.eid_in[a], g.w_in[a]);
                        if (isinf(w)) continue;
                        const double cand = du + w;
                        if (cand < best) best = cand;
                    }
                    if (best < old) {
                        ld_put<kLds>(&d[v], as_u(best));
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
            // 4. propagate.  The first frontier: the marked vertices that ended below their old
            // distance, and the heads that a listed arc still improves
            for (unsigned x = tid; x < A; x += B) {
                const int v = (int)tch[x];
                if (ld_get<kLds>(&d[v]) < oldbits(v)) {
                    const uint32_t bit = 1u << (v & 31);
                    if (!(ld_or<kLds>(&fbit[v >> 5], bit) & bit)) fr0[atomicAdd(&nfr[0], 1u)] = (T)v;
                }
            }
            for (long long x = qn + tid; x < q1; x += B) {
                const int e = q.edge[x];
                if (e < 0 || e >= q.m) continue;
                const int a = q.ea[e], b = q.eb[e];
                const double w = r.nlat[x];
                if (a == b || isinf(w)) continue;
                push(b, as_d(ld_get<kLds>(&d[a])) + w, fr0, &nfr[0]);
                if (!q.directed) push(a, as_d(ld_get<kLds>(&d[b])) + w, fr0, &nfr[0]);
            }
            __syncthreads();
            // the rounds: every new arc, then every out-arc of the frontier; the round that lowers
            // nothing ends them
            int c = 0;
            for (int round = 0;; round++) {
                const unsigned nf = nfr[c];
                if (round > n) {  // a cap, never reached: every round settles a vertex of G_k's order
                    if (tid == 0) raise_err(err, SHD_ROUTE_EDEVICE);
                    break;
                }
                const T* f = c ? fr1 : fr0;
                T* to = c ? fr0 : fr1;
                // the frontier's bits go, so that a vertex lowered while it is read enters the next one
                for (unsigned x = tid; x < nf; x += B) ld_put<kLds>(&fbit[(int)f[x] >> 5], 0u);
                if (tid == 0) nfr[c ^ 1] = 0u;
                __syncthreads();
                new_arcs(to, &nfr[c ^ 1]);
                if (nf <= 64u) {  // a wave per vertex, its lanes over the out-arcs
                    for (unsigned x = wv; x < nf; x += B / 64) {
                        const int v = (int)f[x];
                        const double dv = as_d(ld_get<kLds>(&d[v]));
                        for (int a = r.row_out[v] + lane; a < r.row_out[v + 1]; a += 64) {
                            const double w = wk(r.eid_out[a], r.w_out[a]);
                            if (!isinf(w)) push(r.head_out[a], dv + w, to, &nfr[c ^ 1]);
                        }
                    }
                } else {
                    for (unsigned x = tid; x < nf; x += B) {
                        const int v = (int)f[x];
                        const double dv = as_d(ld_get<kLds>(&d[v]));
                        for (int a = r.row_out[v]; a < r.row_out[v + 1]; a++) {
                            const double w = wk(r.eid_out[a], r.w_out[a]);
                            if (!isinf(w)) push(r.head_out[a], dv + w, to, &nfr[c ^ 1]);
                        }
                    }
                }
                __syncthreads();
                c ^= 1;
                if (nfr[c] == 0u) break;  // uniform: the next write of this word lies behind two barriers
            }
            __syncthreads();
            // 5. the entries and their new latencies
            unsigned long long hit = 0, cut = 0, slow = 0, fast = 0, mx = 0, mg = 0, mn = kInfBits;
            for (long long x = e0 + tid; x < e1; x += B) {
                const int t = tgt[x];
                if (t < 0 || t >= n) continue;
                const unsigned long long w = wt ? wt[wbase + x] : 1ull;
                double nw = NAN, old = NAN;
                bool routed = false;
                if (t == s) {
                    if (se >= 0) {
                        routed = true;
                        old = q.lat[se];
                        nw = old;
                        if (ou_failed(q.edge, qn, q1, se)) {  // listed: the lowest loop that G_k keeps
                            hit += w;
                            nw = INFINITY;
                            for (int y = q.srow[s]; y < q.srow[s + 1]; y++) {
                                const double lw = wk(q.seid[y], q.lat[q.seid[y]]);
                                if (!isinf(lw)) { nw = lw; break; }
                            }
                        }
                    }
                } else if (hr[t] > 0 && hr[t] < n) {
                    routed = true;
                    old = drow[t];
                    nw = as_d(ld_get<kLds>(&d[t]));
                    if (ld_get<kLds>(&mark[t]) != 0) hit += w;
                }
                if (routed) {
                    if (isinf(nw)) { cut += w; nw = NAN; }
                    else {
                        if (nw > old) { slow += w; mx = max(mx, as_u(nw - old)); }
                        else if (nw < old) { fast += w; mg = max(mg, as_u(old - nw)); }
                        mn = min(mn, as_u(nw));
                    }
                }
                if (o.lat) o.lat[(long long)k * o.plane + wbase + x] = nw;
            }
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) {
                hit += __shfl_xor(hit, x, 64);
                cut += __shfl_xor(cut, x, 64);
                slow += __shfl_xor(slow, x, 64);
                fast += __shfl_xor(fast, x, 64);
                mx = max(mx, (unsigned long long)__shfl_xor(mx, x, 64));
                mg = max(mg, (unsigned long long)__shfl_xor(mg, x, 64));
                mn = min(mn, (unsigned long long)__shfl_xor(mn, x, 64));
            }
            if (lane == 0) {
                if (hit) (void)ld_add<true>(&acc[0], hit);
                if (cut) (void)ld_add<true>(&acc[1], cut);
                if (slow) (void)ld_add<true>(&acc[2], slow);
                if (fast) (void)ld_add<true>(&acc[3], fast);
                if (mx) (void)atomicMax(&acc[4], mx);
                if (mg) (void)atomicMax(&acc[5], mg);
                if (mn != kInfBits) (void)atomicMin(&acc[6], mn);
            }
            // 6. restore: the touched vertices back to the old row, marks and bits cleared, once
            // every thread has read its entries
            __syncthreads();
            const unsigned nt_ = *ntch;
            for (unsigned x = tid; x < nt_; x += B) {
                const int v = (int)tch[x];
                ld_put<kLds>(&d[v], oldbits(v));
                ld_put<kLds>(&mark[v], (uint8_t)0);
                ld_put<kLds>(&tbit[v >> 5], 0u);
                ld_put<kLds>(&fbit[v >> 5], 0u);
            }
            __syncthreads();
            if (tid < SHD_ROUTE_EDIT_NSTAT) {
                if (o.stats && acc[tid]) ld_out(o.stats + (long long)k * SHD_ROUTE_EDIT_NSTAT + tid, acc[tid]);
            } else if (tid == 4) {
                if (o.max_add && acc[4]) (void)atomicMax(o.max_add + k, acc[4]);
            } else if (tid == 5) {
                if (o.max_gain && acc[5]) (void)atomicMax(o.max_gain + k, acc[5]);
            } else if (tid == 6) {
                if (o.min_new && acc[6] != kInfBits) (void)atomicMin(o.min_new + k, acc[6]);
                *na = 0u;
                *ntch = 0u;
            }
            __syncthreads();
        }
        __syncthreads();  // the live list goes to the next unit only when every thread is through
    }
}

}  // namespace shd
