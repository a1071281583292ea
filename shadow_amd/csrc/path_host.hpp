#pragma once
// path_host.hpp -- what the path calls (hops, link loads, tie envelope, ECMP loads: path_calls.hpp) decide
// without a device: the arcs they upload, the pairs of a call grouped by source, the source
// chunks of the row scratch and the form each per-source state kernel launches in.  Host code
// only (no hip* call): tests/path_host_main.cpp runs all of it on the CPU.
#include <cstdlib>

#include "host_graph.hpp"

namespace shd {

// ---- the arcs ----
// Every edge that is no self-loop as an arc (both ways when undirected, parallel arcs kept), and
// each vertex's first self-loop edge (-1: none).
struct PathArcs {
    std::vector<int32_t> head, tail, eid;
    std::vector<int> self;
    PathArcs(int n, bool directed, const std::vector<int32_t>& src, const std::vector<int32_t>& dst) : self(n, -1) {
        for (int e = 0; e < (int)src.size(); e++) {
            const int a = src[e], b = dst[e];
            if (a == b) {
                if (self[a] < 0) self[a] = e;
                continue;
            }
            head.push_back(b); tail.push_back(a); eid.push_back(e);
            if (!directed) { head.push_back(a); tail.push_back(b); eid.push_back(e); }
        }
    }
};

struct PathCsr {
    std::vector<int> row, col, eid;
    std::vector<double> w, r;
};

// the in-CSR, arcs sorted by (head, tail, edge id): what the first hops call uploads (row, col =
// tails, eid, w) and, in the same order, the reliabilities the first ties call adds (r)
inline PathCsr path_in_csr(int n, const PathArcs& a, const double* lat, const std::vector<double>& rel) {
    PathCsr c;
    build_csr(n, a.head, a.tail, a.eid, lat, rel, c.row, c.col, c.w, c.r, &c.eid);
    return c;
}

// the out-CSR, arcs sorted by (tail, head, edge id): the release pass of the ties (row, col = heads, w)
inline PathCsr path_out_csr(int n, const PathArcs& a, const double* lat, const std::vector<double>& rel) {
    PathCsr c;
    build_csr(n, a.tail, a.head, a.eid, lat, rel, c.row, c.col, c.w, c.r, &c.eid);
    return c;
}

// ---- pairs grouped by source ----
// The pairs of a call in any order, repeats allowed, stably sorted by source: order[g] = the
// caller's pair at grouped position g; us = the distinct sources, first[u] .. first[u + 1] the
// grouped positions of us[u] (first[nu] = np); per grouped pair the index of its source in us
// (gsi), its target (gt) and, when the call has weights, its weight (gw).
struct PairGroups {
    std::vector<int> order;
    std::vector<int32_t> us, gsi, gt;
    std::vector<long long> first;
    std::vector<uint64_t> gw;
};

inline PairGroups group_pairs(const int32_t* src, const int32_t* tgt, const uint64_t* wt, int np) {
    PairGroups p;
    p.order.resize(np);
    std::iota(p.order.begin(), p.order.end(), 0);
    std::stable_sort(p.order.begin(), p.order.end(), [&](int a, int b) { return src[a] < src[b]; });
    p.gsi.resize(np); p.gt.resize(np); p.gw.resize(wt ? np : 0);
    for (int g = 0; g < np; g++) {
        const int32_t s = src[p.order[g]];
        if (p.us.empty() || p.us.back() != s) { p.us.push_back(s); p.first.push_back(g); }
        p.gsi[g] = (int32_t)p.us.size() - 1;
        p.gt[g] = tgt[p.order[g]];
        if (wt) p.gw[g] = wt[p.order[g]];
    }
    p.first.push_back(np);
    return p;
}

// ---- source chunks of the row scratch ----
// Per source a distance row (f64) and a parent or in-degree row (u32) over all vertices, with
// hrow a hop row (i32) too; `chunk` sources at a time fit the budget (one, when not even one
// does).  The planes lie one behind the other: dist at 0, par / rem at par_off, hrow at hrow_off.
struct ScratchChunks {
    int chunk;
    size_t bytes, par_off, hrow_off;
};

inline ScratchChunks scratch_chunks(int n, int count, size_t budget, bool hrow) {
    const size_t per = (size_t)n * (sizeof(double) + sizeof(uint32_t) + (hrow ? sizeof(int32_t) : 0));
    ScratchChunks s;
    s.chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, budget / per));
    s.bytes = per * (size_t)s.chunk;
    s.par_off = sizeof(double) * (size_t)n * (size_t)s.chunk;
    s.hrow_off = (sizeof(double) + sizeof(uint32_t)) * (size_t)n * (size_t)s.chunk;
    return s;
}

// ---- the form of a per-source state kernel ----
// hops_depth_kernel, loads_tree_kernel, fold_tree_kernel, loss_tree_kernel, ties_dag_kernel,
// ecmp_dag_kernel, outage_repair_kernel, reprice_kernel and edit_kernel (k = their work units) keep one source's state per
// workgroup:
// none under dispatch on a complete graph (mode 2: no tree; such a graph has n <= 65535, its
// edge count being an int), else u16 state in LDS while it fits and the knob does not say off,
// else u16 (n <= 65535) or u32 state in HBM slices, one per resident workgroup.
enum StateForm { kStateNone = 0, kStateLds = 1, kStateHbm16 = 2, kStateHbm32 = 3 };

struct StateLaunch {
    int form, grid;
    size_t lds;     // dynamic LDS bytes of the launch
    size_t stride;  // HBM forms: bytes of one slice
    int slots;      //            and how many the call wants at most
};

// an *_LDS knob says off: set, not empty and zero ("" is not off)
inline bool knob_off(const char* e) { return e && *e && atoi(e) == 0; }

// k sources.  small = the LDS bytes beside the state, lds16 = the u16 state's, which must fit
// lds_budget together; stride16 / stride32 = one HBM slice of either width; the slot rule:
// slot_budget / stride slices, 16 at the least and 512 at the most.
inline StateLaunch state_form(int n, int mode, int k, size_t small, size_t lds16, size_t lds_budget, bool off,
                              size_t stride16, size_t stride32, size_t slot_budget) {
    StateLaunch f{kStateNone, std::min(k, 1024), small, 0, 0};
    if (mode == 2) return f;
    if (n <= 65535 && small + lds16 <= lds_budget && !off) {
        f.form = kStateLds;
        f.lds = small + lds16;
        return f;
    }
    f.form = n <= 65535 ? kStateHbm16 : kStateHbm32;
    f.stride = n <= 65535 ? stride16 : stride32;
    f.slots = (int)std::max<size_t>(16, std::min<size_t>(512, slot_budget / f.stride));
    f.grid = std::min(k, f.slots);
    return f;
}

// ---- what a context holds for the path calls (path_calls.hpp builds, uses and frees it) ----
struct PathSlices {  // the workgroup slices of an HBM form, grown on demand
    char* p = nullptr;
    size_t cap = 0;
};

struct PathDev {
    // hops: the in-CSR with edge ids and each vertex's self-loop edge (built at the first hops
    // call), the identity targets and the parked error word of the all-vertex rows
    int hp_ready = 0;
    int* hp_row = nullptr; int* hp_col = nullptr; int* hp_eid = nullptr; double* hp_w = nullptr;
    int* hp_self = nullptr; int* hp_ident = nullptr; int* hp_saved = nullptr;
    // ties: the in-arcs' reliabilities and the out-CSR (built at the first ties call)
    int ti_ready = 0;
    double* ti_r = nullptr; int* ti_row = nullptr; int* ti_head = nullptr; double* ti_w = nullptr;
    int ld_ready = 0;  // loads: the LDS form's dynamic-LDS limit is raised
    // ECMP loads: the edge id of every arc of the ties' out-CSR (built at the first ECMP call)
    int ec_ready = 0;
    int* ec_eid = nullptr;
    PathSlices hp_ws, ld_ws, ti_ws, ec_ws;
    char* buf = nullptr;  // the row scratch (scratch_chunks), grown on demand
    size_t buf_cap = 0;
    PathSlices fo_ws;  // folds: the HBM slices, and
    int fo_ready = 0;  // the LDS form's dynamic-LDS limit is raised
    // link loss: per edge id 1.0f - loss and the loss as given, per vertex the loss as given
    // (NaN = absent), built at the first loss call; and the HBM slices
    int lo_ready = 0;
    double* lo_r = nullptr; double* lo_q = nullptr; double* lo_p = nullptr;
    PathSlices lo_ws;
    // link outages: per edge id its ends and its latency, per vertex its self-loop edge ids
    // (offsets and ids, ascending), built at the first outage call; and the HBM slices
    int ou_ready = 0;
    int* ou_ea = nullptr; int* ou_eb = nullptr; double* ou_lat = nullptr;
    int* ou_srow = nullptr; int* ou_seid = nullptr;
    PathSlices ou_ws;
    // link repricing: the smallest and the largest latency over the edges that are no
    // self-loops (rp_lo > rp_hi: none), the two words its check kernels reduce into, set at the
    // first repricing call; and the HBM slices
    int rp_ready = 0;
    double rp_lo = 0.0, rp_hi = 0.0;
    unsigned long long* rp_lohi = nullptr;
    PathSlices rp_ws;
    // link edits: the dynamic-LDS limit of the LDS form is raised, the two words the check
    // kernel reduces into, set at the first edit call; and the HBM slices
    int ed_ready = 0;
    unsigned long long* ed_lohi = nullptr;
    PathSlices ed_ws;
};

}  // namespace shd
