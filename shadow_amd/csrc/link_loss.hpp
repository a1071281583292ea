#pragma once
// Link loss: how many of the packets the chosen paths carry reach every edge, how many each
// edge and each vertex drops, and how many arrive.  No reference equivalent (Shadow 1.14 drops
// a packet with one end-to-end coin flip, and counts packets per cached Path only).
//   The packets of an entry (s, t) with weight w go where shd_route_paths puts that entry's
// route, and thin out on the way: what reaches the arc u -> v of the source's shortest-path
// tree is the weight of v's subtree (the integer sum of the link loads, link_loads.hpp) times
// the survival product from the source down to u (the PROD fold of path_fold.hpp over
// 1 - loss).  Both are one sweep of the same tree: the reached vertices are sorted by hop depth
// once, the product goes down level by level (a parent is final when read: the left fold from
// the source, the order the rows fold reliability in), the integer sums come up deepest level
// first, and one pass over the reached vertices multiplies the two.
//   No floating-point atomic touches the state: the sums are u64, the products are written once.
// Only the adds into the outputs are f64 atomics, as the ECMP loads' are.  Built on
// path_hops.hpp as the loads and folds are: the parent arcs and the all-vertex hop rows of the
// sources are the inputs, nothing here reaches into an SSSP kernel.
#include "link_loads.hpp"
#include "loss_layout.hpp"

namespace shd {

struct DevLoss {                       // the per-element columns of a context
    const double* __restrict__ r_e;    // 1.0f - loss of every edge id, the rows' reliability
    const double* __restrict__ q_e;    // the loss of every edge id as given
    const double* __restrict__ vf;     // vertex factors, NaN = absent
    const double* __restrict__ p_v;    // the loss of every vertex as given, NaN = absent
};

struct LossOuts {                      // each nullable
    double* edge_reach;                // per edge id
    double* edge_drop;
    double* vertex_drop;               // per vertex
    double* delivered;
    unsigned long long* unrouted;
};

// the outputs: one f64 atomic add to HBM (hipMalloc memory), the add the ECMP loads use; sums
// across sources are in the order the adds arrive
__device__ inline void lo_out(double* p, double x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what arrives at the target t of an entry: the vertex's own drop, and the rest delivered
__device__ inline void lo_target(const DevLoss& q, const LossOuts& o, int t, double arrive) {
    if (o.vertex_drop) {
        const double pt = q.p_v[t];
        if (!isnan(pt)) lo_out(o.vertex_drop + t, arrive * pt);
    }
    if (o.delivered) {
        const double ft = q.vf[t];
        lo_out(o.delivered + t, isnan(ft) ? arrive : arrive * ft);
    }
}

// what starts over the edge e of a direct-dispatched or self entry
__device__ inline void lo_edge(const DevLoss& q, const LossOuts& o, int e, double reach) {
    if (o.edge_reach) lo_out(o.edge_reach + e, reach);
    if (o.edge_drop) lo_out(o.edge_drop + e, reach * q.q_e[e]);
}

// Entries of source i as loads_tree_kernel takes them (the block, or with eoff the sparse
// lists; wt null = 1 per entry), par / hrow and mode too.  A failed entry raises its code and
// adds its weight to *unrouted, nothing else.  One workgroup per source; T = u16 while
// n <= 65535; state (LossLayout) in LDS (kLds) or in the slice ws + slot * ws_stride.  In HBM
// the sums and the level offsets take atomic adds in L2 and are accessed as link_loads.hpp
// accesses its own; pre and order are written and read with plain accesses on either side of a
// barrier, as path_fold.hpp's values are.
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void loss_tree_kernel(DevHops g, DevLoss q, const uint32_t* __restrict__ par,
                                                      const int* __restrict__ hrow, const int* __restrict__ src,
                                                      int ns, const int* __restrict__ tgt, int nt, long long ld,
                                                      const long long* __restrict__ eoff,
                                                      const unsigned long long* __restrict__ wt, int mode,
                                                      LossOuts o, char* ws, size_t ws_stride,
                                                      int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* wsum = reinterpret_cast<int*>(smem);  // B / 64 <= 16 wave sums
    int* maxd = reinterpret_cast<int*>(smem + 64);
    unsigned long long* rsum = reinterpret_cast<unsigned long long*>(smem + 72);  // the source's routed weight
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const bool tree = mode != 2;
    unsigned long long* sum = nullptr;
    double* pre = nullptr;
    uint32_t* lvl = nullptr;
    T* order = nullptr;
    if (tree) {
        char* base;
        if constexpr (kLds) base = smem + kLoSmall;
        else base = ws + (size_t)blockIdx.x * ws_stride;
        const LossLayout<T> L = LossLayout<T>::make(n);
        sum = reinterpret_cast<unsigned long long*>(base + L.sum);
        pre = reinterpret_cast<double*>(base + L.pre);
        lvl = reinterpret_cast<uint32_t*>(base + L.lvl);
        order = reinterpret_cast<T*>(base + L.order);
    }

    for (int i = blockIdx.x; i < ns; i += gridDim.x) {
        const int s = src[i];
        if (s < 0 || s >= n) {
            if (tid == 0) raise_err(err, SHD_ROUTE_EINVAL);
            continue;
        }
        const uint32_t* __restrict__ prow = tree ? par + (long long)i * n : nullptr;
        const int* __restrict__ drow = tree ? hrow + (long long)i * n : nullptr;
        const double fs = q.vf[s];
        const double Fs = isnan(fs) ? 1.0 : 1.0 * fs;
        // nothing of the slice's source before stays: sums and level counts start from zero
        // (pre and order are written before they are read)
        if (tree) {
            for (int v = tid; v < n; v += B) ld_put<kLds>(&sum[v], 0ull);
            for (int d = tid; d <= n; d += B) ld_put<kLds>(&lvl[d], 0u);
        }
        if (tid == 0) { *maxd = 0; *rsum = 0ull; }
        __syncthreads();

        // 1. the entries: tree entries onto their targets by integer adds; direct-dispatched,
        // self and failed entries end here
        const long long q0 = eoff ? eoff[i] : 0, q1 = eoff ? eoff[i + 1] : (long long)nt;
        const long long wbase = eoff ? 0 : (long long)i * ld;
        unsigned long long lost = 0, routed = 0;
        for (long long x = q0 + tid; x < q1; x += B) {
            const int t = tgt[x];
            if (t < 0 || t >= n) {
                raise_err(err, SHD_ROUTE_EINVAL);
                continue;
            }
            const unsigned long long w = wt ? wt[wbase + x] : 1ull;
            int a;
            if (t == s) {  // the batch self entry: the lowest self-loop edge, no second vertex factor
                const int e = g.self_eid[s];
                if (e < 0) { raise_err(err, SHD_ROUTE_ENOEDGE); lost += w; }
                else if (w) {
                    routed += w;
                    const double reach = (double)w * Fs;
                    lo_edge(q, o, e, reach);
                    if (o.delivered) lo_out(o.delivered + s, reach * q.r_e[e]);
                }
            } else if (mode && (a = hp_find(g, t, s)) >= 0) {  // the direct path: the lowest edge id of the pair
                if (w) {
                    routed += w;
                    const int e = g.eid_in[a];
                    const double reach = (double)w * Fs;
                    lo_edge(q, o, e, reach);
                    lo_target(q, o, t, reach * q.r_e[e]);
                }
            } else if (!tree) {
                raise_err(err, SHD_ROUTE_ENOEDGE);
                lost += w;
            } else if (drow[t] <= 0 || drow[t] >= n) {
                raise_err(err, SHD_ROUTE_EUNREACH);
                lost += w;
            } else if (w) {
                routed += w;
                (void)ld_add<kLds>(&sum[t], w);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lost += __shfl_xor(lost, d, 64);
            routed += __shfl_xor(routed, d, 64);
        }
        if (lane == 0 && lost && o.unrouted) ld_out(o.unrouted, lost);
        if (lane == 0 && routed) (void)ld_add<true>(rsum, routed);  // (in LDS in either state form)
        __syncthreads();
        // the source vertex: one addend for everything it sends
        if (tid == 0 && o.vertex_drop) {
            const unsigned long long wr = *rsum;
            const double ps = q.p_v[s];
            if (wr && !isnan(ps)) lo_out(o.vertex_drop + s, (double)wr * ps);
        }
        if (!tree) {  // a complete graph under dispatch: no sweep
            __syncthreads();  // rsum is read before the next source zeroes it
            continue;
        }

        // 2. counting sort of the reached vertices by hop depth: level sizes and the deepest level
        int lmax = 0;
        for (int v = tid; v < n; v += B) {
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
            int sz = 0;
            for (int k = k0; k < k1; k++) sz += (int)ld_get<kLds>(&lvl[k]);
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
        if (tid == 0) pre[s] = Fs;
        __syncthreads();
        const uint32_t reached = ld_get<kLds>(&lvl[md]);  // the end of the deepest level

        // 3. top-down: the survival product from the source; level d reads level d - 1
        for (int d = 1; d <= md; d++) {
            const uint32_t beg = ld_get<kLds>(&lvl[d - 1]), end = ld_get<kLds>(&lvl[d]);
            for (uint32_t x = beg + tid; x < end; x += B) {
                const int v = (int)order[x];
                const uint32_t arc = prow[v];
                if (arc == HP_NONE) { raise_err(err, SHD_ROUTE_EDEVICE); pre[v] = NAN; continue; }
                pre[v] = pre[g.col_in[arc]] * q.r_e[g.eid_in[arc]];
            }
            __syncthreads();
        }

        // 4. the targets: what arrives of each vertex's own weight
        for (uint32_t x = tid; x < reached; x += B) {
            const int v = (int)order[x];
            const unsigned long long own = ld_get<kLds>(&sum[v]);
            if (own) lo_target(q, o, v, (double)own * pre[v]);
        }
        __syncthreads();

        // 5. bottom-up, deepest level first: a vertex's sum is final when its level comes up and
        // goes to its parent's, so the own weights become the subtree weights in place
        for (int d = md; d >= 2; d--) {
            const uint32_t beg = ld_get<kLds>(&lvl[d - 1]), end = ld_get<kLds>(&lvl[d]);
            for (uint32_t x = beg + tid; x < end; x += B) {
                const int v = (int)order[x];
                const unsigned long long a = ld_get<kLds>(&sum[v]);
                if (!a) continue;
                const uint32_t arc = prow[v];
                if (arc == HP_NONE) continue;  // (raised above)
                (void)ld_add<kLds>(&sum[g.col_in[arc]], a);
            }
            __syncthreads();
        }

        // 6. every reached vertex's parent arc: the subtree's weight times the product down to the parent
        for (uint32_t x = tid; x < reached; x += B) {
            const int v = (int)order[x];
            const unsigned long long a = ld_get<kLds>(&sum[v]);
            if (!a) continue;
            const uint32_t arc = prow[v];
            if (arc == HP_NONE) continue;
            lo_edge(q, o, g.eid_in[arc], (double)a * pre[g.col_in[arc]]);
        }
        __syncthreads();  // the state goes to the next source only when every add has read it
    }
}

}  // namespace shd
