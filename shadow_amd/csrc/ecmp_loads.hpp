#pragma once
// ECMP link loads: the weight of every (source, target) entry split evenly over all of its
// shortest paths (Brandes' dependency accumulation; with weight 1 on all pairs, edge and vertex
// betweenness).  No reference equivalent.  A shortest path is what path_ties.hpp defines: a
// chain of tight arcs over the all-vertex latency row of the source.
//   Per source, with sigma[v] the number of shortest paths s -> v as f64 and own[x] the summed
// weight of the entries with target x:
//   delta[v] = sum over the tight out-arcs (v -> x, e) of f_e,
//   f_e      = (sigma[v] / sigma[x]) * (own[x] + delta[x]),
//   edge_load[e] += f_e,  transit[v] += delta[v] for v != s.
// Every term is non-negative and nothing is subtracted: transit is delta, not "sum minus own".
//   ecmp_dag_kernel sweeps the DAG forwards as ties_dag_kernel does (Kahn levels from {s}, the
// frontier pulls sigma from in-arcs that are all final, then releases its tight out-arcs), but
// appends every frontier to one order list and keeps each level's start.  Then it goes through
// the levels backwards, deepest first: a vertex pulls over its tight out-arcs, whose heads lie
// in deeper levels and are final.  Pulling both ways keeps the state free of floating-point
// atomics; the only ones are the adds into the caller's outputs, one per non-zero flow.
// Built on path_ties.hpp (ties_indeg_kernel, the out-CSR) and the helpers of link_loads.hpp.
#include "ecmp_layout.hpp"
#include "path_ties.hpp"

namespace shd {

static_assert(kEcmpLdsBudget == kLdsBudget, "ecmp_layout.hpp sizes the state for the LDS of common.hpp");

// the outputs: one f64 atomic add to HBM (hipMalloc memory); sums across sources are in the
// order the adds arrive
__device__ inline void ec_out(double* p, double x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Entries of source i as loads_tree_kernel takes them (the block, or with eoff the sparse
// lists); mode as hops_depth_kernel.  dist and rem_in (row stride n): the latency rows and the
// tight in-degrees of ties_indeg_kernel; both null in mode 2.  eid_out: the edge id of every
// arc of the out-CSR of q.  A failed entry raises its code and adds its weight to *unrouted.
// One workgroup per source; T = u16 while n <= 65535; the state in LDS (kLds) or in the slice
// ws + slot * ws_stride, where every access to it is an agent-scope one (the decrements of rem
// and the adds to own run in L2).  edge_load (per edge id), transit (per vertex), unrouted:
// nullable.
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void ecmp_dag_kernel(DevHops g, DevTies q, const int* __restrict__ eid_out,
                                                     const double* __restrict__ dist,
                                                     const uint32_t* __restrict__ rem_in,
                                                     const int* __restrict__ src, int ns,
                                                     const int* __restrict__ tgt, int nt, long long ld,
                                                     const long long* __restrict__ eoff,
                                                     const unsigned long long* __restrict__ wt, int mode,
                                                     double* __restrict__ edge_load, double* __restrict__ transit,
                                                     unsigned long long* __restrict__ unrouted, char* ws,
                                                     size_t ws_stride, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* tail = reinterpret_cast<unsigned*>(smem);  // the length of the order list
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    char* base;
    if constexpr (kLds) base = smem + kEcSmall;
    else base = ws + (size_t)blockIdx.x * ws_stride;
    const EcmpLayout<T> L = EcmpLayout<T>::make(n);
    unsigned long long* sig = reinterpret_cast<unsigned long long*>(base + L.sig);
    unsigned long long* dl = reinterpret_cast<unsigned long long*>(base + L.dl);
    unsigned long long* own = reinterpret_cast<unsigned long long*>(base + L.own);
    uint32_t* rem = reinterpret_cast<uint32_t*>(base + L.rem);
    T* order = reinterpret_cast<T*>(base + L.order);
    uint32_t* lvl = reinterpret_cast<uint32_t*>(base + L.lvl);
    const bool dag = mode != 2;

    for (int i = blockIdx.x; i < ns; i += gridDim.x) {
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (tid == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        const double* __restrict__ drow = dag ? dist + (long long)i * n : nullptr;
        if (dag) {
            // nothing of the source before stays: no vertex is final, no weight, an order of {s}
            const uint32_t* __restrict__ rrow = rem_in + (long long)i * n;
            for (int v = tid; v < n; v += B) {
                ld_put<kLds>(&sig[v], ti_u(v == s ? 1.0 : 0.0));
                ld_put<kLds>(&dl[v], ti_u(0.0));
                ld_put<kLds>(&own[v], 0ull);
                ld_put<kLds>(&rem[v], rrow[v]);
            }
            if (tid == 0) {
                ld_put<kLds>(&order[0], (T)s);
                ld_put<kLds>(&lvl[0], 0u);
                *tail = 1u;
            }
            __syncthreads();
        }

        // the row's weights onto their targets; direct-dispatched, self and failed entries end here
        const long long q0 = eoff ? eoff[i] : 0, q1 = eoff ? eoff[i + 1] : (long long)nt;
        const long long wbase = eoff ? 0 : (long long)i * ld;
        unsigned long long lost = 0;
        for (long long e = q0 + tid; e < q1; e += B) {
            const int t = tgt[e];
            if (t < 0 || t >= n) {
                raise_err(err, SHD_ROUTE_EINVAL);
                continue;
            }
            const unsigned long long w = wt ? wt[wbase + e] : 1ull;
            int a;
            if (t == s) {  // the batch self entry: the lowest self-loop edge, no transit
                const int se = g.self_eid[s];
                if (se < 0) { raise_err(err, SHD_ROUTE_ENOEDGE); lost += w; }
                else if (w && edge_load) ec_out(edge_load + se, (double)w);
            } else if (mode && (a = hp_find(g, t, s)) >= 0) {  // the direct path: the lowest edge id of the pair
                if (w && edge_load) ec_out(edge_load + g.eid_in[a], (double)w);
            } else if (!dag) {
                raise_err(err, SHD_ROUTE_ENOEDGE);
                lost += w;
            } else if (isnan(drow[t])) {
                raise_err(err, SHD_ROUTE_EUNREACH);
                lost += w;
            } else if (w) {
                (void)ld_add<kLds>(&own[t], w);
            }
        }
        if (unrouted) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lost += __shfl_xor(lost, d, 64);
            if (lane == 0 && lost) ld_out(unrouted, lost);
        }
        if (!dag) continue;  // a complete graph under dispatch: no sweep (no barrier below either)

        // ---- forwards: level r is order[beg .. end); the vertices it releases are appended ----
        unsigned beg = 0, end = 1;
        int nlev = 0;
        for (int r = 0; r < n && beg < end; r++) {
            // (a) pull: every tight in-arc of a frontier vertex comes from a final vertex
            if (r > 0) {
                for (unsigned x0 = beg; x0 < end; x0 += B) {
                    const unsigned x = x0 + (unsigned)tid;
                    int v = -1, a0 = 0, a1 = 0;
                    double dv = NAN;
                    if (x < end) {
                        v = (int)ld_get<kLds>(&order[x]);
                        a0 = g.row_in[v];
                        a1 = g.row_in[v + 1];
                        dv = drow[v];
                    }
                    double c = 0.0;
                    const bool wide = v >= 0 && (a1 - a0 > HP_WIDE);
                    if (v >= 0 && !wide) {
                        for (int a = a0; a < a1; a++) {
                            const int u = g.col_in[a];
                            const double du = u == s ? 0.0 : drow[u];
                            if (du + g.w_in[a] == dv) c += ti_d(ld_get<kLds>(&sig[u]));
                        }
                    }
                    unsigned long long m = __ballot(wide);
                    while (m) {
                        const int l = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const int b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64);
                        const double tv = __shfl(dv, l, 64);
                        double wc = 0.0;
                        for (int a = b0 + lane; a < b1; a += 64) {
                            const int u = g.col_in[a];
                            const double du = u == s ? 0.0 : drow[u];
                            if (du + g.w_in[a] == tv) wc += ti_d(ld_get<kLds>(&sig[u]));
                        }
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) wc += __shfl_xor(wc, d, 64);
                        if (lane == l) c = wc;
                    }
                    if (v >= 0) ld_put<kLds>(&sig[v], ti_u(c));
                }
                __syncthreads();
            }
            // (b) release: a tight out-arc takes one from its head's count; the lane that takes
            // the last one appends the head to the order
            for (unsigned x0 = beg; x0 < end; x0 += B) {
                const unsigned x = x0 + (unsigned)tid;
                int u = -1, a0 = 0, a1 = 0;
                double du = NAN;
                if (x < end) {
                    u = (int)ld_get<kLds>(&order[x]);
                    a0 = q.row_out[u];
                    a1 = q.row_out[u + 1];
                    du = u == s ? 0.0 : drow[u];
                }
                const bool wide = u >= 0 && (a1 - a0 > HP_WIDE);
                if (u >= 0 && !wide) {
                    for (int a = a0; a < a1; a++) {
                        const int y = q.head_out[a];
                        if (y != s && du + q.w_out[a] == drow[y] && ld_add<kLds>(&rem[y], 0xFFFFFFFFu) == 1u) {
                            const unsigned at = atomicAdd(tail, 1u);
                            if (at < (unsigned)n) ld_put<kLds>(&order[at], (T)y);
                        }
                    }
                }
                unsigned long long m = __ballot(wide);
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64);
                    const double tu = __shfl(du, l, 64);
                    for (int a = b0 + lane; a < b1; a += 64) {
                        const int y = q.head_out[a];
                        if (y != s && tu + q.w_out[a] == drow[y] && ld_add<kLds>(&rem[y], 0xFFFFFFFFu) == 1u) {
                            const unsigned at = atomicAdd(tail, 1u);
                            if (at < (unsigned)n) ld_put<kLds>(&order[at], (T)y);
                        }
                    }
                }
            }
            __syncthreads();
            // the next append comes after the next round's first barrier: every thread reads the same
            nlev = r + 1;
            beg = end;
            end = min(*tail, (unsigned)n);
            if (tid == 0) ld_put<kLds>(&lvl[nlev], beg);
        }
        // a vertex the rows reached and the sweep never made final
        for (int v = tid; v < n; v += B)
            if (v != s && !isnan(drow[v]) && ti_d(ld_get<kLds>(&sig[v])) == 0.0) raise_err(err, SHD_ROUTE_EDEVICE);
        __syncthreads();

        // ---- backwards, deepest level first: the heads of a vertex's tight out-arcs are final ----
        for (int r = nlev - 1; r >= 0; r--) {
            const unsigned b = ld_get<kLds>(&lvl[r]), e = ld_get<kLds>(&lvl[r + 1]);
            for (unsigned x0 = b; x0 < e; x0 += B) {
                const unsigned x = x0 + (unsigned)tid;
                int v = -1, a0 = 0, a1 = 0;
                double dv = NAN, sv = 0.0;
                if (x < e) {
                    v = (int)ld_get<kLds>(&order[x]);
                    a0 = q.row_out[v];
                    a1 = q.row_out[v + 1];
                    dv = v == s ? 0.0 : drow[v];
                    sv = ti_d(ld_get<kLds>(&sig[v]));
                }
                double dsum = 0.0;
                const bool wide = v >= 0 && (a1 - a0 > HP_WIDE);
                if (v >= 0 && !wide) {
                    for (int a = a0; a < a1; a++) {
                        const int y = q.head_out[a];
                        if (y == s || dv + q.w_out[a] != drow[y]) continue;
                        const double below = (double)ld_get<kLds>(&own[y]) + ti_d(ld_get<kLds>(&dl[y]));
                        const double f = (sv / ti_d(ld_get<kLds>(&sig[y]))) * below;
                        if (f == 0.0) continue;
                        dsum += f;
                        if (edge_load) ec_out(edge_load + eid_out[a], f);
                    }
                }
                unsigned long long m = __ballot(wide);
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64);
                    const double tv = __shfl(dv, l, 64), ts = __shfl(sv, l, 64);
                    double wsum = 0.0;
                    for (int a = b0 + lane; a < b1; a += 64) {
                        const int y = q.head_out[a];
                        if (y == s || tv + q.w_out[a] != drow[y]) continue;
                        const double below = (double)ld_get<kLds>(&own[y]) + ti_d(ld_get<kLds>(&dl[y]));
                        const double f = (ts / ti_d(ld_get<kLds>(&sig[y]))) * below;
                        if (f == 0.0) continue;
                        wsum += f;
                        if (edge_load) ec_out(edge_load + eid_out[a], f);
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) wsum += __shfl_xor(wsum, d, 64);
                    if (lane == l) dsum = wsum;
                }
                if (v >= 0) {
                    ld_put<kLds>(&dl[v], ti_u(dsum));
                    if (v != s && dsum != 0.0 && transit) ec_out(transit + v, dsum);
                }
            }
            __syncthreads();  // after the last level: the state goes to the next source
        }
    }
}

}  // namespace shd
