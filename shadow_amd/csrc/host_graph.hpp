#pragma once
// host_graph.hpp -- the host-side graph of shd_route_create: the arcs of a validated topology as
// out- and in-CSR, and what the pre-pass derives from its edges.  Host code only (no hip* call):
// engine.hip builds the device graph from it and tests/select_main.cpp the selection's input.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/shd_route.h"

namespace shd {

// Build a CSR (rows by `key`, columns by `other`), arcs sorted by (row, col, eid).
inline void build_csr(int n, const std::vector<int32_t>& rows, const std::vector<int32_t>& cols,
                      const std::vector<int32_t>& eids, const double* lat,
                      const std::vector<double>& rel, std::vector<int>& row, std::vector<int>& col,
                      std::vector<double>& w, std::vector<double>& r, std::vector<int>* eid_out = nullptr) {
    const size_t k = rows.size();
    std::vector<size_t> idx(k);
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
        if (rows[a] != rows[b]) return rows[a] < rows[b];
        if (cols[a] != cols[b]) return cols[a] < cols[b];
        return eids[a] < eids[b];
    });
    row.assign(n + 1, 0);
    col.resize(k); w.resize(k); r.resize(k);
    for (size_t q = 0; q < k; q++) {
        size_t a = idx[q];
        row[rows[a] + 1]++;
        col[q] = cols[a];
        w[q] = lat[eids[a]];
        r[q] = rel[eids[a]];
    }
    if (eid_out) {
        eid_out->resize(k);
        for (size_t q = 0; q < k; q++) (*eid_out)[q] = eids[idx[q]];
    }
    for (int v = 0; v < n; v++) row[v + 1] += row[v];
}

// The edges as the rows kernels see them (self-loops excluded: w > 0 never relaxes them).
// An undirected graph's in-CSR is its out-CSR (row_in .. r_in stay empty; in_*() answer both).
struct HostGraph {
    int n = 0, m = 0, nnz = 0;
    int directed = 0, integer_w = 0, multigraph = 0;
    int self16 = 1;  // every self-loop latency (the table's diagonal) is an integer below 0xFFFF
    double min_w = 0, max_w = 0;
    std::vector<double> e_rel;           // 1 - loss per edge (topology.c:437)
    std::vector<double> self_w, self_r;  // the first self-loop of each vertex (NaN: none)
    std::vector<int> loops;              // self-loops per vertex
    std::vector<int> row, col, eid, row_in, col_in;
    std::vector<double> w, r, w_in, r_in;
    const std::vector<int>& in_row() const { return directed ? row_in : row; }
    const std::vector<int>& in_col() const { return directed ? col_in : col; }
    const std::vector<double>& in_w() const { return directed ? w_in : w; }
    const std::vector<double>& in_r() const { return directed ? r_in : r; }

    // g has passed shd_route_create's validation
    static HostGraph make(const shd_graph_t* g) {
        HostGraph h;
        const int n = h.n = g->n_vertices, m = h.m = g->n_edges;
        h.directed = g->directed ? 1 : 0;
        h.e_rel.resize(m);
        for (int e = 0; e < m; e++) h.e_rel[e] = (1.0f - g->edge_packetloss[e]);
        std::vector<int32_t> ar, ac, ae, ir, ic, ie;
        h.self_w.assign(n, NAN); h.self_r.assign(n, NAN);
        h.loops.assign(n, 0);
        h.min_w = m ? INFINITY : 0;
        bool integral = true;
        for (int e = 0; e < m; e++) {
            int a = g->edge_src[e], b = g->edge_dst[e];
            double w = g->edge_latency[e];
            h.max_w = std::max(h.max_w, w);
            h.min_w = std::min(h.min_w, w);
            if (w != std::floor(w) || w > 1048576.0) integral = false;
            if (a == b) {
                if (std::isnan(h.self_w[a])) { h.self_w[a] = w; h.self_r[a] = h.e_rel[e]; }
                h.loops[a]++;
                continue;
            }
            ar.push_back(a); ac.push_back(b); ae.push_back(e);
            if (!h.directed) { ar.push_back(b); ac.push_back(a); ae.push_back(e); }
            else { ir.push_back(b); ic.push_back(a); ie.push_back(e); }
        }
        h.integer_w = integral && (double)n * h.max_w < 2147483647.0;
        for (int v = 0; v < n; v++)
            if (!std::isnan(h.self_w[v]) && !(h.self_w[v] == std::floor(h.self_w[v]) && h.self_w[v] < 65535.0))
                h.self16 = 0;
        build_csr(n, ar, ac, ae, g->edge_latency, h.e_rel, h.row, h.col, h.w, h.r, &h.eid);
        if (h.directed) build_csr(n, ir, ic, ie, g->edge_latency, h.e_rel, h.row_in, h.col_in, h.w_in, h.r_in);
        h.nnz = (int)h.col.size();
        for (int v = 0; v < n && !h.multigraph; v++)
            for (int a = h.row[v] + 1; a < h.row[v + 1]; a++)
                if (h.col[a] == h.col[a - 1]) { h.multigraph = 1; break; }
        for (int v = 0; v < n; v++) if (h.loops[v] > 1) h.multigraph = 1;
        return h;
    }
};

}  // namespace shd
