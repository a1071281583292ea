#pragma once
// Link loads: how much weight the chosen paths put on every edge and through every vertex.
// No reference equivalent (Shadow 1.14 counts packets per cached Path only, path.c:57-60).
//   The load of an entry (s, t) with weight w goes where shd_route_paths puts that entry's
// route: on every edge of the tree path and through its intermediate vertices, on the direct
// edge for a direct-dispatched pair, on the self-loop for t == s.  Summing down the source's
// shortest-path tree makes that O(n) per source instead of one walk per pair: every vertex
// hands the sum of its subtree to its parent once, deepest level first.  Built on
// path_hops.hpp: the parent arcs (hops_parent_kernel) and the all-vertex hop rows
// (hops_depth_kernel) of the sources are the inputs, nothing here reaches into an SSSP kernel.
//   All sums are u64 integer adds (LDS and HBM atomics): exact and independent of order.
#include "path_hops.hpp"

namespace shd {

constexpr size_t kLdSmall = 96;  // wave sums of the block scan (16), the row's deepest level

// bytes of one source's state: subtree sums and own weights (u64 per vertex), the level
// offsets (u32 per hop depth, depths 0 .. n - 1 and one more) and the vertices in level order
template <typename T>
__host__ __device__ inline size_t ld_state_bytes(int n) {
    return 2 * a16(sizeof(unsigned long long) * (size_t)n) + a16(sizeof(uint32_t) * ((size_t)n + 1)) +
           a16(sizeof(T) * (size_t)n);
}

// The state lives in LDS or in an HBM slice.  In HBM the sums and the level offsets take
// atomic adds, which run in L2: every other access to them bypasses this CU's L1 (agent-scope
// relaxed).  The own weights and the order list are written and read with plain accesses on
// either side of a barrier, as the hop counting's HBM state is.
template <bool kLds, typename U>
__device__ inline U ld_get(U* p) {
    if constexpr (kLds) return *p;
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool kLds, typename U>
__device__ inline void ld_put(U* p, U x) {
    if constexpr (kLds) *p = x;
    else __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool kLds, typename U>
__device__ inline U ld_add(U* p, U x) {
    if constexpr (kLds) return __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the outputs: one vector u64 atomic add to HBM, order-independent
__device__ inline void ld_out(unsigned long long* p, unsigned long long x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Entries of source i: the row i of the block (tgt[j], wt[i * ld + j], j < nt), or with eoff
// the sparse form, tgt[q] and wt[q] for eoff[i] <= q < eoff[i + 1]; wt null = 1 per entry.
// par / hrow (row stride n): the parent arcs and the tree hop count of every vertex (-1 =
// unreached; the source's own entry is not read); both null in mode 2.  mode as
// hops_depth_kernel.  A failed entry raises its code and adds its weight to *unrouted.
// One workgroup per source; T = u16 while n <= 65535; state in LDS (kLds) or in the slice
// ws + slot * ws_stride.  edge_load (per edge id), transit (per vertex), unrouted: nullable.
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void loads_tree_kernel(DevHops g, const uint32_t* __restrict__ par,
                                                       const int* __restrict__ hrow, const int* __restrict__ src,
                                                       int ns, const int* __restrict__ tgt, int nt, long long ld,
                                                       const long long* __restrict__ eoff,
                                                       const unsigned long long* __restrict__ wt, int mode,
                                                       unsigned long long* __restrict__ edge_load,
                                                       unsigned long long* __restrict__ transit,
                                                       unsigned long long* __restrict__ unrouted, char* ws,
                                                       size_t ws_stride, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* wsum = reinterpret_cast<int*>(smem);          // B / 64 <= 16 wave sums
    int* maxd = reinterpret_cast<int*>(smem + 64);
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    char* base;
    if constexpr (kLds) base = smem + kLdSmall;
    else base = ws + (size_t)blockIdx.x * ws_stride;
    const size_t a8 = a16(sizeof(unsigned long long) * (size_t)n);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(base);
    unsigned long long* own = reinterpret_cast<unsigned long long*>(base + a8);
    uint32_t* lvl = reinterpret_cast<uint32_t*>(base + 2 * a8);
    T* order = reinterpret_cast<T*>(base + 2 * a8 + a16(sizeof(uint32_t) * ((size_t)n + 1)));
    const bool tree = mode != 2;

    for (int i = blockIdx.x; i < ns; i += gridDim.x) {
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (tid == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        const uint32_t* __restrict__ prow = tree ? par + (long long)i * n : nullptr;
        const int* __restrict__ drow = tree ? hrow + (long long)i * n : nullptr;
        // nothing of the source before stays: sums and level counts start from zero
        if (tree) {
            for (int v = tid; v < n; v += B) ld_put<kLds>(&acc[v], 0ull);
            for (int d = tid; d <= n; d += B) ld_put<kLds>(&lvl[d], 0u);
        }
        if (tid == 0) *maxd = 0;
        __syncthreads();

        // the row's weights onto their targets; direct-dispatched, self and failed entries end here
        const long long q0 = eoff ? eoff[i] : 0, q1 = eoff ? eoff[i + 1] : (long long)nt;
        const long long wbase = eoff ? 0 : (long long)i * ld;
        unsigned long long lost = 0;
        for (long long q = q0 + tid; q < q1; q += B) {
            const int t = tgt[q];
            if (t < 0 || t >= n) {
                raise_err(err, SHD_ROUTE_EINVAL);
                continue;
            }
            const unsigned long long w = wt ? wt[wbase + q] : 1ull;
            int a;
            if (t == s) {  // the batch self entry: the lowest self-loop edge, no transit
                const int e = g.self_eid[s];
                if (e < 0) { raise_err(err, SHD_ROUTE_ENOEDGE); lost += w; }
                else if (w && edge_load) ld_out(edge_load + e, w);
            } else if (mode && (a = hp_find(g, t, s)) >= 0) {  // the direct path: the lowest edge id of the pair
                if (w && edge_load) ld_out(edge_load + g.eid_in[a], w);
            } else if (!tree) {
                raise_err(err, SHD_ROUTE_ENOEDGE);
                lost += w;
            } else if (drow[t] <= 0 || drow[t] >= n) {
                raise_err(err, SHD_ROUTE_EUNREACH);
                lost += w;
            } else if (w) {
                (void)ld_add<kLds>(&acc[t], w);
            }
        }
        if (unrouted) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) lost += __shfl_xor(lost, d, 64);
            if (lane == 0 && lost) ld_out(unrouted, lost);
        }
        if (!tree) continue;  // a complete graph under dispatch: no tree sums (no barrier below either)
        __syncthreads();

        // counting sort of the reached vertices by hop depth: level sizes, the deepest level,
        // and each vertex's own weight kept beside its running sum
        int lmax = 0;
        for (int v = tid; v < n; v += B) {
            own[v] = ld_get<kLds>(&acc[v]);
            const int d = drow[v];
            if (v != s && d > 0 && d < n) {
                (void)ld_add<kLds>(&lvl[d], 1u);
                lmax = max(lmax, d);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) lmax = max(lmax, __shfl_xor(lmax, d, 64));
        if (lane == 0 && lmax) atomicMax(maxd, lmax);
        __syncthreads();
        const int md = *maxd;
        // exclusive scan of the level sizes 0 .. md: every thread a contiguous run of levels
        {
            const int per = (md + 1 + B - 1) / B;
            const int k0 = min(tid * per, md + 1), k1 = min(k0 + per, md + 1);
            int sum = 0;
            for (int k = k0; k < k1; k++) sum += (int)ld_get<kLds>(&lvl[k]);
            int incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            int run = incl - sum;
            for (int k = 0; k < wv; k++) run += wsum[k];
            for (int k = k0; k < k1; k++) {
                const uint32_t c = ld_get<kLds>(&lvl[k]);
                ld_put<kLds>(&lvl[k], (uint32_t)run);
                run += (int)c;
            }
        }
        __syncthreads();
        // place the vertices: lvl[d] moves from the start of level d to its end, the start of d + 1
        for (int v = tid; v < n; v += B) {
            const int d = drow[v];
            if (v != s && d > 0 && d < n) order[ld_add<kLds>(&lvl[d], 1u)] = (T)v;
        }
        __syncthreads();
        // deepest level first: a vertex's sum is final when its level comes up; it goes to the
        // parent's sum, to the parent arc's edge, and what came from below through the vertex
        for (int d = md; d >= 1; d--) {
            const uint32_t beg = ld_get<kLds>(&lvl[d - 1]), end = ld_get<kLds>(&lvl[d]);
            for (uint32_t x = beg + tid; x < end; x += B) {
                const int v = (int)order[x];
                const unsigned long long a = ld_get<kLds>(&acc[v]);
                if (!a) continue;
                const uint32_t arc = prow[v];
                if (arc == HP_NONE) { raise_err(err, SHD_ROUTE_EDEVICE); continue; }
                const int p = g.col_in[arc];
                if (p != s) (void)ld_add<kLds>(&acc[p], a);
                if (edge_load) ld_out(edge_load + g.eid_in[arc], a);
                const unsigned long long through = a - own[v];
                if (through && transit) ld_out(transit + v, through);
            }
            __syncthreads();
        }
    }
}

}  // namespace shd
