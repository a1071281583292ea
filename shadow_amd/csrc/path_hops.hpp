#pragma once
// Path hops: the chosen shortest path itself -- parent arcs, hop counts and packed explicit
// routes -- derived from finished distance rows.  The reference shows the path in the line
// _topology_computeSourcePaths logs per target (topology.c:1449, 1502, 1829-1844).
//   The engine's tie rule is a function of the distances alone: the parent of v is the tight
// in-arc (u -> v), dist[u] + w == dist[v] in f64 (the left fold the rows take), with the
// smallest (dist[u], u, edge id).  So nothing here reaches into an SSSP kernel: the distance
// row of a source is the all-vertex latency row of shd_route_rows_async, whatever kernel the
// context selected, and
//   hops_parent_kernel   picks every vertex's parent arc from it (a u32 index into the in-CSR
//                        below: tail vertex and graph edge id of the arc),
//   hops_depth_kernel    counts hops by pointer jumping over (parent, hops) pairs, one
//                        workgroup per source, in LDS or in an HBM slice per workgroup slot,
//   hops_pairs_kernel    resolves the hop count of (source, target) pairs (self entry and
//                        direct-path dispatch included),
//   hops_extract_kernel  walks each pair's parent chain back from the target and stores
//                        vertices and edge ids in forward order.
// The in-CSR carries edge ids, rows sorted by (u, eid): within one row the arc index orders
// arcs as (u, eid) does, so the tie key is (dist[u], arc index); self-loops are not arcs.
#include "common.hpp"

namespace shd {

constexpr uint32_t HP_NONE = 0xFFFFFFFFu;  // parent record of the source and of unreached vertices
constexpr int HP_WIDE = 32;                // in-lists longer than this are scanned by the whole wave
constexpr int HP_ROUNDS = 40;              // pointer-jumping rounds (2^32 hops; a cap, never reached)

struct DevHops {
    int n;
    const int* __restrict__ row_in;    // in-CSR offsets (n + 1)
    const int* __restrict__ col_in;    // tail u of the arc
    const int* __restrict__ eid_in;    // graph edge id of the arc
    const double* __restrict__ w_in;   // its latency
    const int* __restrict__ self_eid;  // lowest self-loop edge id of each vertex, -1 = none
};

// first in-arc (lowest edge id) of v whose tail is u, or -1
__device__ inline int hp_find(const DevHops& g, int v, int u) {
    int lo = g.row_in[v], hi = g.row_in[v + 1];
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.col_in[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && g.col_in[lo] == u) ? lo : -1;
}

// The rows launch behind a hops call writes its source's own entry too (the batch self
// entry) and raises SHD_ROUTE_ENOEDGE where there is no self-loop.  That entry is not asked
// for here: the error word is parked before the rows and per-entry codes of the rows are
// dropped after them (the hops kernels raise their own for the caller's entries).
__global__ void hops_err_park_kernel(int* err, int* saved) {
    *saved = *err;
    *err = 0;
}
__global__ void hops_err_unpark_kernel(int* err, const int* saved) {
    const int cur = *err;
    const int keep = (cur == SHD_ROUTE_ENOEDGE || cur == SHD_ROUTE_EUNREACH) ? 0 : cur;
    *err = *saved ? *saved : keep;
}

// par[i * pld + v] = the parent arc of v in the tree of source src[i], HP_NONE for the source
// and for unreached vertices.  Grid: x over vertex tiles of B, y over sources.
template <int B>
__global__ __launch_bounds__(B) void hops_parent_kernel(DevHops g, const double* __restrict__ dist, long long dld,
                                                        const int* __restrict__ src, int ns,
                                                        uint32_t* __restrict__ par, long long pld,
                                                        int* __restrict__ err) {
    const int n = g.n;
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.y; i < ns; i += gridDim.y) {
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (threadIdx.x == 0 && blockIdx.x == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        const double* __restrict__ drow = dist + (long long)i * dld;
        uint32_t* __restrict__ prow = par + (long long)i * pld;
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
            uint32_t best = HP_NONE;
            const bool wide = live && (a1 - a0 > HP_WIDE);
            if (live && !wide) {
                double bd = INFINITY;
                for (int a = a0; a < a1; a++) {  // ascending arc index: '<' keeps the first of equals
                    const int u = g.col_in[a];
                    const double du = u == s ? 0.0 : drow[u];
                    if (du + g.w_in[a] == dv && du < bd) { bd = du; best = (uint32_t)a; }
                }
            }
            // hubs: one in-list at a time over the 64 lanes, then a (dist[u], arc) min-reduce
            unsigned long long m = __ballot(wide);
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64);
                const double tv = __shfl(dv, l, 64);
                double bd = INFINITY;
                uint32_t ba = HP_NONE;
                for (int a = b0 + lane; a < b1; a += 64) {
                    const int u = g.col_in[a];
                    const double du = u == s ? 0.0 : drow[u];
                    if (du + g.w_in[a] == tv && du < bd) { bd = du; ba = (uint32_t)a; }
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const double od = __shfl_xor(bd, d, 64);
                    const uint32_t oa = (uint32_t)__shfl_xor((int)ba, d, 64);
                    if (od < bd || (od == bd && oa < ba)) { bd = od; ba = oa; }
                }
                if (lane == l) best = ba;
            }
            if (v < n) prow[v] = best;
        }
    }
}

// bytes of one source's pointer-jumping state: four arrays of n (parent, hops, twice)
template <typename T>
__host__ __device__ inline size_t hp_state_bytes(int n) { return 4 * a16(sizeof(T) * (size_t)n); }
constexpr size_t kHpSmall = 16;  // flag, row maximum

// hops[i * ld + j] = hop count of src[i] -> tgt[j] and row_max[i] = the row's maximum.
// mode 0: the tree path; 1: prefer-direct, an adjacent pair is the one-hop direct path; 2: a
// complete graph, every pair is (no tree: par may be null).  The self entry is the self-loop
// hop (1) or -1 with SHD_ROUTE_ENOEDGE; an unreached target -1 with SHD_ROUTE_EUNREACH;
// quiet != 0 writes the -1 without raising.  One workgroup per source; T = u16 while
// n <= 65535 (hops <= n - 1), the state in LDS (kLds) or in the slice ws + slot * ws_stride.
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void hops_depth_kernel(DevHops g, const uint32_t* __restrict__ par, long long pld,
                                                       const int* __restrict__ src, int ns,
                                                       const int* __restrict__ tgt, int nt, long long ld, int mode,
                                                       int quiet, int* __restrict__ hops_out,
                                                       int* __restrict__ row_max, char* ws, size_t ws_stride,
                                                       int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* flag = reinterpret_cast<int*>(smem);
    int* rmax = reinterpret_cast<int*>(smem + 4);
    const int n = g.n;
    const int tid = threadIdx.x;
    const size_t an = a16(sizeof(T) * (size_t)n) / sizeof(T);
    T* base;
    if constexpr (kLds) base = reinterpret_cast<T*>(smem + kHpSmall);
    else base = reinterpret_cast<T*>(ws + (size_t)blockIdx.x * ws_stride);

    for (int i = blockIdx.x; i < ns; i += gridDim.x) {
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (tid == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        T* p0 = base;
        T* h0 = base + an;
        T* p1 = base + 2 * an;
        T* h1 = base + 3 * an;
        if (mode != 2) {
            const uint32_t* __restrict__ prow = par + (long long)i * pld;
            // a dead (unreached) vertex points at itself with 0 hops and stays so
            for (int v = tid; v < n; v += B) {
                const uint32_t a = prow[v];
                const bool up = v != s && a != HP_NONE;
                p0[v] = (T)(up ? g.col_in[a] : v);
                h0[v] = (T)(up ? 1 : 0);
            }
            __syncthreads();
            // pointer jumping: (p, h) -> (p[p], h + h[p]) until every live vertex points at s
            for (int round = 0; round < HP_ROUNDS; round++) {
                if (tid == 0) *flag = 0;
                __syncthreads();
                int again = 0;
                for (int v = tid; v < n; v += B) {
                    const T p = p0[v];
                    const T pp = p0[p];
                    p1[v] = pp;
                    h1[v] = (T)(h0[v] + h0[p]);
                    if ((int)pp != s && pp != p) again = 1;
                }
                if (again) *flag = 1;
                __syncthreads();
                again = *flag;
                __syncthreads();
                T* x = p0; p0 = p1; p1 = x;
                x = h0; h0 = h1; h1 = x;
                if (!again) break;
            }
        }
        if (tid == 0) *rmax = -1;
        __syncthreads();
        int lmax = -1;
        int* hrow = hops_out ? hops_out + (long long)i * ld : nullptr;
        for (int j = tid; j < nt; j += B) {
            const int t = tgt[j];
            int hv = -1;
            if (t < 0 || t >= n) {
                raise_err(err, SHD_ROUTE_EINVAL);
            } else if (t == s) {  // the batch self entry: one self-loop hop (topology.c:1471-1499)
                if (g.self_eid[s] >= 0) hv = 1;
                else if (!quiet) raise_err(err, SHD_ROUTE_ENOEDGE);
            } else if (mode && hp_find(g, t, s) >= 0) {
                hv = 1;  // the direct path (topology.c:1877-1927)
            } else if (mode == 2) {
                if (!quiet) raise_err(err, SHD_ROUTE_ENOEDGE);
            } else if ((int)p0[t] != s) {
                if (!quiet) raise_err(err, SHD_ROUTE_EUNREACH);
            } else {
                hv = (int)h0[t];
            }
            if (hrow) hrow[j] = hv;
            lmax = max(lmax, hv);
        }
        if (row_max) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lmax = max(lmax, __shfl_xor(lmax, d, 64));
            if ((tid & 63) == 0) atomicMax(rmax, lmax);
            __syncthreads();
            if (tid == 0) row_max[i] = *rmax;
        }
        __syncthreads();
    }
}

// cnt[k] = hop count of pair k = (src[psi[k]], ptgt[k]), from the all-vertex hop rows
// hrow[i * n + v] of the tree (mode 0 / 1; null in mode 2); -1 and the code for a failed pair.
__global__ __launch_bounds__(256) void hops_pairs_kernel(DevHops g, const int* __restrict__ src,
                                                         const int* __restrict__ psi, const int* __restrict__ ptgt,
                                                         int np, int mode, const int* __restrict__ hrow,
                                                         int* __restrict__ cnt, int* __restrict__ err) {
    const int n = g.n;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < np; k += gridDim.x * blockDim.x) {
        const int i = psi[k];
        const int s = src[i], t = ptgt[k];
        int hv = -1;
        if (s < 0 || s >= n || t < 0 || t >= n) {
            raise_err(err, SHD_ROUTE_EINVAL);
        } else if (t == s) {
            if (g.self_eid[s] >= 0) hv = 1;
            else raise_err(err, SHD_ROUTE_ENOEDGE);
        } else if (mode && hp_find(g, t, s) >= 0) {
            hv = 1;
        } else if (mode == 2) {
            raise_err(err, SHD_ROUTE_ENOEDGE);
        } else {
            hv = hrow[(long long)i * n + t];
            if (hv < 0) raise_err(err, SHD_ROUTE_EUNREACH);
        }
        cnt[k] = hv;
    }
}

// Pair k with cnt[k] = h >= 0: vert[voff[k] .. + h] = the path's vertices from the source to
// the target, edge[eoff[k] .. + h - 1] = the graph edge id of each hop.  The walk goes back
// from the target through the parent rows (the original ones: every arc of the path), each
// hop stored at the slot its distance from the source gives.  One lane per pair.
__global__ __launch_bounds__(256) void hops_extract_kernel(DevHops g, const uint32_t* __restrict__ par, long long pld,
                                                           const int* __restrict__ src,
                                                           const int* __restrict__ psi, const int* __restrict__ ptgt,
                                                           const int* __restrict__ cnt,
                                                           const long long* __restrict__ voff,
                                                           const long long* __restrict__ eoff, int np, int mode,
                                                           int* __restrict__ vert, int* __restrict__ edge,
                                                           int* __restrict__ err) {
    const int n = g.n;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < np; k += gridDim.x * blockDim.x) {
        const int h = cnt[k];
        if (h < 0) continue;
        const int i = psi[k];
        const int s = src[i], t = ptgt[k];
        if (s < 0 || s >= n || t < 0 || t >= n) continue;
        const long long vo = voff[k], eo = eoff[k];
        if (t == s) {
            vert[vo] = s; vert[vo + 1] = s;
            edge[eo] = g.self_eid[s];
            continue;
        }
        if (mode) {
            const int a = hp_find(g, t, s);
            if (a >= 0) {  // the direct path: the lowest edge id joining the pair
                vert[vo] = s; vert[vo + 1] = t;
                edge[eo] = g.eid_in[a];
                continue;
            }
        }
        const uint32_t* __restrict__ prow = par + (long long)i * pld;
        int v = t;
        for (int q = h; q > 0; q--) {
            const uint32_t a = prow[v];
            if (a == HP_NONE) { raise_err(err, SHD_ROUTE_EDEVICE); break; }
            vert[vo + q] = v;
            edge[eo + q - 1] = g.eid_in[a];
            v = g.col_in[a];
        }
        vert[vo] = v;
    }
}

}  // namespace shd
