#pragma once
// Tie envelope: for every (source, target) entry the number of shortest paths and the smallest
// and largest reliability any of them has.  No reference equivalent (the reference takes the
// one path igraph's heap order leaves it with, topology.c:1756).
//   A shortest path is a chain of tight arcs, d[u] + w == d[v] in f64 over the all-vertex
// latency row of the source (d[s] taken as 0.0, as hops_parent_kernel does); self-loops are not
// arcs, parallel tight edges are distinct paths.  The tight arcs form a DAG (w > 0), and
//   count[v] = saturating sum of count[u],  lo[v] = min lo[u] * r_e,  hi[v] = max hi[u] * r_e
// over the tight in-arcs (u -> v, e), from count[s] = 1, lo[s] = hi[s] = 1.0 * f_s.  Reliabilities
// are in [0, 1], so fl(a * r) is monotone in a and the min (max) of the source-first left folds
// over all paths is this min (max) programme, bit for bit.
//   ties_indeg_kernel  counts every vertex's tight in-arcs from the distance row (the u32 row
//                      takes the place of the hops calls' parent row in the scratch),
//   ties_dag_kernel    sweeps the DAG level by level from {s} (Kahn), one workgroup per source:
//                      the frontier pulls its values from in-arcs that are all final, then
//                      releases its tight out-arcs; no floating-point atomics, no order in the
//                      result.  Then it writes the caller's entries (vertex factor of the target
//                      last, self entry, direct dispatch, failures).
// Built on path_hops.hpp (the in-CSR, hp_find) and the access helpers of link_loads.hpp.
#include "link_loads.hpp"
#include "ties_layout.hpp"

namespace shd {

static_assert(kTiesLdsBudget == kLdsBudget, "ties_layout.hpp sizes the state for the LDS of common.hpp");
constexpr unsigned long long TI_SAT = 0xFFFFFFFFFFFFFFFFull;  // a count that no longer fits
// what the sweep reads besides the hops in-CSR (built at the first ties call)
struct DevTies {
    const double* __restrict__ r_in;     // reliability of every in-arc, aligned with DevHops::col_in
    const int* __restrict__ row_out;     // out-CSR offsets (n + 1); self-loops left out, parallel arcs kept
    const int* __restrict__ head_out;    // head x of the arc
    const double* __restrict__ w_out;    // its latency
    const double* __restrict__ vf;       // vertex factors, NaN = absent
    const double* __restrict__ self_r;   // reliability of the lowest self-loop, NaN = none
};

__device__ inline unsigned long long ti_satadd(unsigned long long a, unsigned long long b) {
    const unsigned long long c = a + b;
    return c < a ? TI_SAT : c;
}

// rem[i * rld + v] = the number of tight in-arcs of v under source src[i]; 0 for the source and
// for unreached vertices.  Grid: x over vertex tiles of B, y over sources.
template <int B>
__global__ __launch_bounds__(B) void ties_indeg_kernel(DevHops g, const double* __restrict__ dist, long long dld,
                                                       const int* __restrict__ src, int ns,
                                                       uint32_t* __restrict__ rem, long long rld) {
    const int n = g.n;
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.y; i < ns; i += gridDim.y) {
        const int s = src[i];
        if (s < 0 || s >= n) continue;  // the sweep raises SHD_ROUTE_EINVAL
        const double* __restrict__ drow = dist + (long long)i * dld;
        uint32_t* __restrict__ rrow = rem + (long long)i * rld;
        for (int v0 = blockIdx.x * B; v0 < n; v0 += gridDim.x * B) {
            const int v = v0 + (int)threadIdx.x;
            int a0 = 0, a1 = 0;
            double dv = NAN;
            bool live = v < n && v != s;
            if (live) {
                a0 = g.row_in[v];
                a1 = g.row_in[v + 1];
                dv = drow[v];
                live = !isnan(dv);
            }
            uint32_t cnt = 0;
            const bool wide = live && (a1 - a0 > HP_WIDE);
            if (live && !wide) {
                for (int a = a0; a < a1; a++) {
                    const int u = g.col_in[a];
                    const double du = u == s ? 0.0 : drow[u];
                    if (du + g.w_in[a] == dv) cnt++;
                }
            }
            // hubs: one in-list at a time over the 64 lanes
            unsigned long long m = __ballot(wide);
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64);
                const double tv = __shfl(dv, l, 64);
                int c = 0;
                for (int a = b0 + lane; a < b1; a += 64) {
                    const int u = g.col_in[a];
                    const double du = u == s ? 0.0 : drow[u];
                    if (du + g.w_in[a] == tv) c++;
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
                if (lane == l) cnt = (uint32_t)c;
            }
            if (v < n) rrow[v] = cnt;
        }
    }
}

__device__ inline double ti_d(unsigned long long x) { return __longlong_as_double((long long)x); }
__device__ inline unsigned long long ti_u(double x) { return (unsigned long long)__double_as_longlong(x); }

// count / rel_lo / rel_hi[i * ld + j] of src[i] -> tgt[j]; any output may be null.  dist and rem
// (row stride n): the latency rows and the tight in-degrees of ties_indeg_kernel; both null in
// mode 2.  mode as hops_depth_kernel.  One workgroup per source; T = u16 while n <= 65535; the
// state in LDS (kLds) or in the slice ws + slot * ws_stride, where every access to it is an
// agent-scope one (the decrements of rem run in L2).
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void ties_dag_kernel(DevHops g, DevTies q, const double* __restrict__ dist,
                                                     const uint32_t* __restrict__ rem_in,
                                                     const int* __restrict__ src, int ns,
                                                     const int* __restrict__ tgt, int nt, long long ld, int mode,
                                                     unsigned long long* __restrict__ count_out,
                                                     double* __restrict__ lo_out, double* __restrict__ hi_out,
                                                     char* ws, size_t ws_stride, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* fsz = reinterpret_cast<unsigned*>(smem);  // sizes of the two frontier lists
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    char* base;
    if constexpr (kLds) base = smem + kTiSmall;
    else base = ws + (size_t)blockIdx.x * ws_stride;
    const TiesLayout<T> L = TiesLayout<T>::make(n);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(base + L.cnt);
    unsigned long long* lov = reinterpret_cast<unsigned long long*>(base + L.lo);
    unsigned long long* hiv = reinterpret_cast<unsigned long long*>(base + L.hi);
    uint32_t* rem = reinterpret_cast<uint32_t*>(base + L.rem);
    T* f0 = reinterpret_cast<T*>(base + L.f0);
    T* f1 = reinterpret_cast<T*>(base + L.f1);
    const bool dag = mode != 2;

    for (int i = blockIdx.x; i < ns; i += gridDim.x) {
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (tid == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        const double fs = q.vf[s];
        const double cs = isnan(fs) ? 1.0 : 1.0 * fs;
        const double* __restrict__ drow = dag ? dist + (long long)i * n : nullptr;
        if (dag) {
            // nothing of the source before stays: no vertex is final, no list holds anything
            const uint32_t* __restrict__ rrow = rem_in + (long long)i * n;
            for (int v = tid; v < n; v += B) {
                ld_put<kLds>(&cnt[v], v == s ? 1ull : 0ull);
                ld_put<kLds>(&rem[v], rrow[v]);
            }
            if (tid == 0) {
                ld_put<kLds>(&lov[s], ti_u(cs));
                ld_put<kLds>(&hiv[s], ti_u(cs));
                ld_put<kLds>(&f0[0], (T)s);
                fsz[0] = 1u;
                fsz[1] = 0u;
            }
            __syncthreads();
            int cur = 0;
            for (int round = 0; round <= n; round++) {
                const unsigned nf = fsz[cur];
                if (nf == 0) break;
                T* F = cur ? f1 : f0;
                T* G = cur ? f0 : f1;
                // (a) pull: every tight in-arc of a frontier vertex comes from a final vertex
                if (round > 0) {
                    for (unsigned x0 = 0; x0 < nf; x0 += B) {
                        const unsigned x = x0 + (unsigned)tid;
                        int v = -1, a0 = 0, a1 = 0;
                        double dv = NAN;
                        if (x < nf) {
                            v = (int)ld_get<kLds>(&F[x]);
                            a0 = g.row_in[v];
                            a1 = g.row_in[v + 1];
                            dv = drow[v];
                        }
                        unsigned long long c = 0;
                        double lo = INFINITY, hi = -INFINITY;
                        const bool wide = v >= 0 && (a1 - a0 > HP_WIDE);
                        if (v >= 0 && !wide) {
                            for (int a = a0; a < a1; a++) {
                                const int u = g.col_in[a];
                                const double du = u == s ? 0.0 : drow[u];
                                if (du + g.w_in[a] == dv) {
                                    const double r = q.r_in[a];
                                    c = ti_satadd(c, ld_get<kLds>(&cnt[u]));
                                    lo = fmin(lo, ti_d(ld_get<kLds>(&lov[u])) * r);
                                    hi = fmax(hi, ti_d(ld_get<kLds>(&hiv[u])) * r);
                                }
                            }
                        }
                        unsigned long long m = __ballot(wide);
                        while (m) {
                            const int l = __ffsll((long long)m) - 1;
                            m &= m - 1;
                            const int b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64);
                            const double tv = __shfl(dv, l, 64);
                            unsigned long long wc = 0;
                            double wl = INFINITY, wh = -INFINITY;
                            for (int a = b0 + lane; a < b1; a += 64) {
                                const int u = g.col_in[a];
                                const double du = u == s ? 0.0 : drow[u];
                                if (du + g.w_in[a] == tv) {
                                    const double r = q.r_in[a];
                                    wc = ti_satadd(wc, ld_get<kLds>(&cnt[u]));
                                    wl = fmin(wl, ti_d(ld_get<kLds>(&lov[u])) * r);
                                    wh = fmax(wh, ti_d(ld_get<kLds>(&hiv[u])) * r);
                                }
                            }
#pragma unroll
                            for (int d = 32; d >= 1; d >>= 1) {
                                wc = ti_satadd(wc, __shfl_xor(wc, d, 64));
                                wl = fmin(wl, __shfl_xor(wl, d, 64));
                                wh = fmax(wh, __shfl_xor(wh, d, 64));
                            }
                            if (lane == l) { c = wc; lo = wl; hi = wh; }
                        }
                        if (v >= 0) {
                            ld_put<kLds>(&cnt[v], c);
                            ld_put<kLds>(&lov[v], ti_u(lo));
                            ld_put<kLds>(&hiv[v], ti_u(hi));
                        }
                    }
                    __syncthreads();
                }
                // (b) release: a tight out-arc takes one from its head's count; the lane that
                // takes the last one puts the head on the next frontier
                for (unsigned x0 = 0; x0 < nf; x0 += B) {
                    const unsigned x = x0 + (unsigned)tid;
                    int u = -1, a0 = 0, a1 = 0;
                    double du = NAN;
                    if (x < nf) {
                        u = (int)ld_get<kLds>(&F[x]);
                        a0 = q.row_out[u];
                        a1 = q.row_out[u + 1];
                        du = u == s ? 0.0 : drow[u];
                    }
                    const bool wide = u >= 0 && (a1 - a0 > HP_WIDE);
                    if (u >= 0 && !wide) {
                        for (int a = a0; a < a1; a++) {
                            const int y = q.head_out[a];
                            if (y != s && du + q.w_out[a] == drow[y] &&
                                ld_add<kLds>(&rem[y], 0xFFFFFFFFu) == 1u) {
                                const unsigned at = atomicAdd(&fsz[cur ^ 1], 1u);
                                if (at < (unsigned)n) ld_put<kLds>(&G[at], (T)y);
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
                            if (y != s && tu + q.w_out[a] == drow[y] &&
                                ld_add<kLds>(&rem[y], 0xFFFFFFFFu) == 1u) {
                                const unsigned at = atomicAdd(&fsz[cur ^ 1], 1u);
                                if (at < (unsigned)n) ld_put<kLds>(&G[at], (T)y);
                            }
                        }
                    }
                }
                __syncthreads();
                if (tid == 0) fsz[cur] = 0u;  // appended to again after the next round's first barrier
                cur ^= 1;
            }
        }

        // the caller's entries
        unsigned long long* crow = count_out ? count_out + (long long)i * ld : nullptr;
        double* lrow = lo_out ? lo_out + (long long)i * ld : nullptr;
        double* hrow = hi_out ? hi_out + (long long)i * ld : nullptr;
        for (int j = tid; j < nt; j += B) {
            const int t = tgt[j];
            unsigned long long c = 0;
            double lo = NAN, hi = NAN;
            int a;
            if (t < 0 || t >= n) {
                raise_err(err, SHD_ROUTE_EINVAL);
            } else if (t == s) {  // the batch self entry: the lowest self-loop (topology.c:1471-1499)
                const double r = q.self_r[s];
                if (isnan(r)) raise_err(err, SHD_ROUTE_ENOEDGE);
                else { c = 1; lo = hi = cs * r; }
            } else if (mode && (a = hp_find(g, t, s)) >= 0) {  // the direct path (topology.c:1877-1927)
                const double ft = q.vf[t];
                c = 1;
                lo = hi = (isnan(ft) ? cs : cs * ft) * q.r_in[a];
            } else if (!dag) {
                raise_err(err, SHD_ROUTE_ENOEDGE);
            } else if (isnan(drow[t])) {
                raise_err(err, SHD_ROUTE_EUNREACH);
            } else if ((c = ld_get<kLds>(&cnt[t])) == 0) {
                raise_err(err, SHD_ROUTE_EDEVICE);  // reached by the rows and never final here
            } else {
                const double ft = q.vf[t];
                lo = ti_d(ld_get<kLds>(&lov[t]));
                hi = ti_d(ld_get<kLds>(&hiv[t]));
                if (!isnan(ft)) { lo = lo * ft; hi = hi * ft; }
            }
            if (crow) crow[j] = c;
            if (lrow) lrow[j] = lo;
            if (hrow) hrow[j] = hi;
        }
        __syncthreads();  // the state goes to the next source only when every entry is out
    }
}

}  // namespace shd
