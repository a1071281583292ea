#pragma once
// edit_host.hpp -- what the host forms of the link edit calls (edit_calls.hpp) decide without a
// device: the scenario records packed and sorted (new links first in the caller's order, then the
// listed ids ascending), everything include/shd_route.h refuses, and the absorbed-latency rule
// over the graph, the finite listed latencies and the new links.  Host code only (no hip* call):
// tests/edit_host_main.cpp runs all of it on the CPU.
#include "host_graph.hpp"

namespace shd {

// the smallest and the largest latency over the edges that are no self-loops (lo > hi: none)
inline void edit_graph_lohi(int m, const int32_t* e_src, const int32_t* e_dst, const double* e_lat, double* lo,
                            double* hi) {
    *lo = INFINITY;
    *hi = 0.0;
    for (int e = 0; e < m; e++)
        if (e_src[e] != e_dst[e]) {
            *lo = std::min(*lo, e_lat[e]);
            *hi = std::max(*hi, e_lat[e]);
        }
}

// the rule of shd_graph_t over a lo and a hi
inline bool edit_absorbed(int n, double lo, double hi) { return hi > 0.0 && lo <= (double)(n - 1) * (hi * 0x1p-52); }

struct EditHostScn {
    std::vector<int64_t> off;
    std::vector<int32_t> edge, a, b;  // edge -1: a new link a - b; else a = b = 0
    std::vector<double> lat;          // +inf on a listed id: removed
    // SHD_ROUTE_EINVAL: an offset that does not rise, an id that is neither -1 nor an edge id or
    // comes twice in a scenario, a latency that is NaN or <= 0, +inf on a new link, an end of a
    // new link outside [0, n) or both ends the same; SHD_ROUTE_EUNSUPPORTED: the absorbed-latency
    // rule from the graph's lo and hi on
    int take(int n, int m, const int32_t* e_src, const int32_t* e_dst, double lo, double hi, const int64_t* scn_off,
             const int32_t* scn_edge, const int32_t* scn_a, const int32_t* scn_b, const double* scn_lat, int32_t nscn) {
        if (nscn < 0 || (nscn && !scn_off)) return SHD_ROUTE_EINVAL;
        off.assign(1, 0);
        if (!nscn) return SHD_ROUTE_OK;
        if (scn_off[0] != 0) return SHD_ROUTE_EINVAL;
        for (int k = 0; k < nscn; k++)
            if (scn_off[k + 1] < scn_off[k]) return SHD_ROUTE_EINVAL;
        const int64_t tot = scn_off[nscn];
        if (tot && (!scn_edge || !scn_lat)) return SHD_ROUTE_EINVAL;
        for (int64_t x = 0; x < tot; x++) {
            const int e = scn_edge[x];
            if (e < -1 || e >= m || !(scn_lat[x] > 0.0)) return SHD_ROUTE_EINVAL;
            if (e == -1) {
                if (!scn_a || !scn_b || std::isinf(scn_lat[x])) return SHD_ROUTE_EINVAL;
                if (scn_a[x] < 0 || scn_a[x] >= n || scn_b[x] < 0 || scn_b[x] >= n || scn_a[x] == scn_b[x])
                    return SHD_ROUTE_EINVAL;
            }
        }
        off.assign(scn_off, scn_off + nscn + 1);
        edge.resize(tot); a.resize(tot); b.resize(tot); lat.resize(tot);
        std::vector<int64_t> idx;
        for (int k = 0; k < nscn; k++) {
            idx.resize(off[k + 1] - off[k]);
            std::iota(idx.begin(), idx.end(), off[k]);
            // -1 sorts before every id and the sort is stable: the new links keep their order
            std::stable_sort(idx.begin(), idx.end(), [&](int64_t p, int64_t q) { return scn_edge[p] < scn_edge[q]; });
            for (size_t y = 0; y < idx.size(); y++) {
                const int64_t x = idx[y];
                if (y && scn_edge[x] >= 0 && scn_edge[x] == scn_edge[idx[y - 1]]) return SHD_ROUTE_EINVAL;
                edge[off[k] + y] = scn_edge[x];
                a[off[k] + y] = scn_edge[x] < 0 ? scn_a[x] : 0;
                b[off[k] + y] = scn_edge[x] < 0 ? scn_b[x] : 0;
                lat[off[k] + y] = scn_lat[x];
            }
        }
        for (int64_t x = 0; x < tot; x++) {
            if (std::isinf(lat[x])) continue;
            if (edge[x] < 0 || e_src[edge[x]] != e_dst[edge[x]]) {
                lo = std::min(lo, lat[x]);
                hi = std::max(hi, lat[x]);
            }
        }
        return edit_absorbed(n, lo, hi) ? SHD_ROUTE_EUNSUPPORTED : SHD_ROUTE_OK;
    }
};

}  // namespace shd
