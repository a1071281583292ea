#pragma once
// Path folds: sum, min, max or product of a per-edge value along the chosen path of every
// entry.  No reference equivalent (Shadow 1.14 folds latency and reliability only,
// topology.c:1407-1523, and drops the graphml's jitter after validating it, topology.c:1105-1114).
//   The fold of an entry (s, t) runs over the edge ids shd_route_paths reports for it, in order
// from the source.  Carrying the value down the source's shortest-path tree makes that O(n) per
// source and fold instead of one walk per pair: the reached vertices are sorted by hop depth,
// and level by level every vertex takes its parent's value and applies its parent arc's edge.
// A parent sits one level up, so it is final when read, and the value of a vertex is the left
// fold from the source: the order the rows fold latency in.  No atomics on values, nothing
// reassociated: every entry is reproducible to the bit.  Built on path_hops.hpp as
// link_loads.hpp is: the parent arcs (hops_parent_kernel) and the all-vertex hop rows
// (hops_depth_kernel) of the sources are the inputs, nothing here reaches into an SSSP kernel.
#include "fold_layout.hpp"
#include "link_loads.hpp"

namespace shd {

struct FoldOps {  // the ops of a call, by value (SHD_ROUTE_FOLD_*)
    int op[SHD_ROUTE_FOLD_MAX_N];
};

__device__ inline double fold_identity(int op) {
    return op == SHD_ROUTE_FOLD_SUM ? 0.0 : op == SHD_ROUTE_FOLD_MIN ? INFINITY : op == SHD_ROUTE_FOLD_MAX ? -INFINITY : 1.0;
}

__device__ inline double fold_apply(int op, double acc, double a) {
    switch (op) {
        case SHD_ROUTE_FOLD_SUM: return acc + a;
        case SHD_ROUTE_FOLD_MIN: return a < acc ? a : acc;
        case SHD_ROUTE_FOLD_MAX: return a > acc ? a : acc;
        default: return acc * a;
    }
}

// out[k * plane + x] = fold k of entry x of source i.  Entries: the row i of the block
// (tgt[j], x = i * ld + j, j < nt), or with eoff the sparse form, tgt[q] and x = q for
// eoff[i] <= q < eoff[i + 1].  a[k * m + e] = the value of edge id e for fold k.  par / hrow
// (row stride n): the parent arcs and the tree hop count of every vertex (-1 = unreached; the
// source's own entry is not read); both null in mode 2.  mode as hops_depth_kernel.  A failed
// entry raises its code and is NaN in every fold.  One workgroup per source; T = u16 while
// n <= 65535; state (FoldLayout) in LDS (kLds) or in the slice ws + slot * ws_stride.  In HBM
// the level offsets take atomic adds in L2 and are accessed as link_loads.hpp accesses its own;
// val and order are written and read with plain accesses on either side of a barrier.
template <typename T, bool kLds, int B>
__global__ __launch_bounds__(B) void fold_tree_kernel(DevHops g, const uint32_t* __restrict__ par,
                                                      const int* __restrict__ hrow, const int* __restrict__ src,
                                                      int ns, const int* __restrict__ tgt, int nt, long long ld,
                                                      const long long* __restrict__ eoff, FoldOps ops, int nf,
                                                      const double* __restrict__ a, long long m, int mode,
                                                      double* __restrict__ out, long long plane, char* ws,
                                                      size_t ws_stride, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* wsum = reinterpret_cast<int*>(smem);  // B / 64 <= 16 wave sums
    int* maxd = reinterpret_cast<int*>(smem + 64);
    const int n = g.n;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const bool tree = mode != 2;
    double* val = nullptr;
    uint32_t* lvl = nullptr;
    T* order = nullptr;
    if (tree) {
        char* base;
        if constexpr (kLds) base = smem + kFoSmall;
        else base = ws + (size_t)blockIdx.x * ws_stride;
        const FoldLayout<T> L = FoldLayout<T>::make(n);
        val = reinterpret_cast<double*>(base + L.val);
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
        int md = 0;
        if (tree) {
            // nothing of the slice's source before stays: every value failed, level counts zero
            for (int v = tid; v < n; v += B) val[v] = NAN;
            for (int d = tid; d <= n; d += B) ld_put<kLds>(&lvl[d], 0u);
            if (tid == 0) *maxd = 0;
            __syncthreads();
            // counting sort of the reached vertices by hop depth: level sizes and the deepest level
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
            md = *maxd;
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
        }

        const long long q0 = eoff ? eoff[i] : 0, q1 = eoff ? eoff[i + 1] : (long long)nt;
        const long long obase = eoff ? 0 : (long long)i * ld;
        for (int k = 0; k < nf; k++) {
            const int op = ops.op[k];
            const double id = fold_identity(op);
            const double* __restrict__ ak = a + (long long)k * m;
            if (tree) {
                // top-down: the source holds the identity, level d reads level d - 1
                if (tid == 0) val[s] = id;
                __syncthreads();
                for (int d = 1; d <= md; d++) {
                    const uint32_t beg = ld_get<kLds>(&lvl[d - 1]), end = ld_get<kLds>(&lvl[d]);
                    for (uint32_t x = beg + tid; x < end; x += B) {
                        const int v = (int)order[x];
                        const uint32_t arc = prow[v];
                        if (arc == HP_NONE) { raise_err(err, SHD_ROUTE_EDEVICE); val[v] = NAN; continue; }
                        val[v] = fold_apply(op, val[g.col_in[arc]], ak[g.eid_in[arc]]);
                    }
                    __syncthreads();
                }
            }
            // the caller's entries, coalesced over j; self, direct and failed entries need no tree
            double* __restrict__ ok = out + (long long)k * plane + obase;
            for (long long q = q0 + tid; q < q1; q += B) {
                const int t = tgt[q];
                double x = NAN;
                int code = 0, arc;
                if (t < 0 || t >= n) {
                    code = SHD_ROUTE_EINVAL;
                } else if (t == s) {  // the batch self entry: the lowest self-loop edge alone
                    const int e = g.self_eid[s];
                    if (e < 0) code = SHD_ROUTE_ENOEDGE;
                    else x = fold_apply(op, id, ak[e]);
                } else if (mode && (arc = hp_find(g, t, s)) >= 0) {  // the direct path: the lowest edge id of the pair
                    x = fold_apply(op, id, ak[g.eid_in[arc]]);
                } else if (!tree) {
                    code = SHD_ROUTE_ENOEDGE;
                } else if (drow[t] <= 0 || drow[t] >= n) {
                    code = SHD_ROUTE_EUNREACH;
                } else {
                    x = val[t];
                }
                if (code && k == 0) raise_err(err, code);
                ok[q] = x;
            }
            if (tree) __syncthreads();  // the next fold, or the next source, overwrites val
        }
    }
}

}  // namespace shd
