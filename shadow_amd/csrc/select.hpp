#pragma once
// select.hpp -- which rows kernel a topology gets, and everything that kernel reads, as pure
// host functions: no device call, no context.  Included after the kernel headers, whose layout
// structs and constants decide what fits the LDS.  select_all() runs the stages in order,
//   select_inrows -> select_k32 -> select_attr -> select_kd -> select_kb -> (f64 only) select_kf
// and engine.hip's apply_selection() uploads what they staged.  Each choice lists its staged
// arrays once, in arrays(): the upload, Selection::upload_bytes and tests/select_main.cpp's
// digests all walk that list.  tests/golden/select_info.json pins the decisions.
#include <string>

#include "host_graph.hpp"

namespace shd {

// Workgroup sizes of the templated kernels: f(std::integral_constant<int, B>) for a runtime block
template <typename F>
auto kd_dispatch(int blk, F f) {
    switch (blk) {
        case 1024: return f(std::integral_constant<int, 1024>{});
        case 768: return f(std::integral_constant<int, 768>{});
        case 512: return f(std::integral_constant<int, 512>{});
        default: return f(std::integral_constant<int, 256>{});
    }
}
template <typename F>
auto k32_dispatch(int blk, F f) {
    switch (blk) {
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        default: return f(std::integral_constant<int, 1024>{});
    }
}
// KF: f(block, state in HBM, packed arcs); KFH runs 1024 threads only
template <typename F>
auto kf_dispatch(int blk, bool hbm, bool pk, F f) {
    using T = std::true_type;
    using N = std::false_type;
    if (hbm) return pk ? f(std::integral_constant<int, 1024>{}, T{}, T{}) : f(std::integral_constant<int, 1024>{}, T{}, N{});
    if (blk == 256) return pk ? f(std::integral_constant<int, 256>{}, N{}, T{}) : f(std::integral_constant<int, 256>{}, N{}, N{});
    return pk ? f(std::integral_constant<int, 1024>{}, N{}, T{}) : f(std::integral_constant<int, 1024>{}, N{}, N{});
}

// The creation-time SHD_ROUTE_* knobs (launch-time ones are read where they apply).
struct SelectKnobs {
    struct Int { bool set = false; int v = 0; };
    std::string kernel;   // KERNEL: kd, kb, k32, kf, f64, auto (empty: unset)
    int kdblock = 0;      // KDBLOCK: 256 or 1024 (0: by n)
    Int delta;            // DELTA: KD bucket width (>= 1)
    Int qcap;             // QCAP: caps KD's work queue (>= 64)
    Int kdpack, kdgrid, hub1024, kdwalk;
    Int kbtcap, kbfuse, kbgrid;
    Int kfh, kfpk;
    bool kfdelta_set = false;
    double kfdelta = 0;   // KFDELTA: KF bucket width in ms

    // the integer stages run (f64 and kf leave them out altogether)
    bool integer_stages() const { return kernel != "f64" && kernel != "kf"; }
    bool wants(const char* k) const { return kernel.empty() || kernel == k || kernel == "auto"; }

    static SelectKnobs from_env() {
        SelectKnobs k;
        auto num = [](const char* name) {
            Int x;
            if (const char* e = getenv(name)) { x.set = true; x.v = atoi(e); }
            return x;
        };
        if (const char* e = getenv("SHD_ROUTE_KERNEL")) k.kernel = e;
        const int b = num("SHD_ROUTE_KDBLOCK").v;
        if (b == 256 || b == 1024) k.kdblock = b;  // (512/768: the phase-A ring sizing assumes 256 or 1024)
        k.delta = num("SHD_ROUTE_DELTA"); k.delta.v = std::max(1, k.delta.v);
        k.qcap = num("SHD_ROUTE_QCAP"); k.qcap.v = std::max(64, k.qcap.v);
        k.kdpack = num("SHD_ROUTE_KDPACK");
        k.kdgrid = num("SHD_ROUTE_KDGRID");    // tests cap the grid so that every workgroup runs many sources in turn
        k.hub1024 = num("SHD_ROUTE_HUB1024");
        k.kdwalk = num("SHD_ROUTE_KDWALK");
        k.kbtcap = num("SHD_ROUTE_KBTCAP");
        k.kbfuse = num("SHD_ROUTE_KBFUSE");
        k.kbgrid = num("SHD_ROUTE_KBGRID");    // tests cap the grid so that every workgroup runs several batches in turn
        k.kfh = num("SHD_ROUTE_KFH");          // (tests: KFH on graphs KF takes)
        k.kfpk = num("SHD_ROUTE_KFPK");
        if (const char* e = getenv("SHD_ROUTE_KFDELTA")) { k.kfdelta_set = true; k.kfdelta = atof(e); }
        return k;
    }
};

// What shd_route_create has in host vectors (a view: nothing is copied)
struct SelectInput {
    int n, nnz;
    bool directed, integer_w, multigraph;
    double min_w;
    const std::vector<int>&row, &col, &eid;
    const std::vector<double>&w, &r;
    const std::vector<int>&row_in, &col_in;  // the out-CSR itself when undirected
    const std::vector<double>&w_in, &r_in;
    const std::vector<double>& e_rel;
    explicit SelectInput(const HostGraph& h)
        : n(h.n), nnz(h.nnz), directed(h.directed), integer_w(h.integer_w), multigraph(h.multigraph), min_w(h.min_w),
          row(h.row), col(h.col), eid(h.eid), w(h.w), r(h.r), row_in(h.in_row()), col_in(h.in_col()),
          w_in(h.in_w()), r_in(h.in_r()), e_rel(h.e_rel) {}
};

// ---- shared helpers ---------------------------------------------------------------------------

// Host Dijkstra (exact for integer weights) -> eccentricity of vertex 0.
inline double ecc0(int n, const std::vector<int>& row, const std::vector<int>& col, const std::vector<double>& w) {
    std::vector<double> d(n, INFINITY);
    std::vector<std::pair<double, int>> h;
    d[0] = 0;
    h.push_back({0.0, 0});
    auto cmp = [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first > b.first; };
    while (!h.empty()) {
        std::pop_heap(h.begin(), h.end(), cmp);
        auto [du, u] = h.back();
        h.pop_back();
        if (du > d[u]) continue;
        for (int a = row[u]; a < row[u + 1]; a++) {
            double nd = du + w[a];
            if (nd < d[col[a]]) { d[col[a]] = nd; h.push_back({nd, col[a]}); std::push_heap(h.begin(), h.end(), cmp); }
        }
    }
    double mx = 0;
    for (double x : d) mx = std::max(mx, x);
    return mx;
}

// The distinct values (exact bits) in ascending order of their bit patterns and each element's
// index into that table; ok: at most `cap` distinct values (else the result is cut short).
template <typename Idx>
struct Distinct {
    std::vector<double> tab;
    std::vector<Idx> idx;
    bool ok = true;
};
template <typename Idx>
Distinct<Idx> distinct_bits(const std::vector<double>& values, size_t cap) {
    Distinct<Idx> d;
    d.idx.resize(values.size());
    std::vector<std::pair<uint64_t, int>> keyed(values.size());
    for (size_t a = 0; a < values.size(); a++) {
        std::memcpy(&keyed[a].first, &values[a], 8);
        keyed[a].second = (int)a;
    }
    std::sort(keyed.begin(), keyed.end());
    for (size_t q = 0; q < keyed.size(); q++) {
        if (q == 0 || keyed[q].first != keyed[q - 1].first) {
            if (d.tab.size() == cap) { d.ok = false; return d; }
            double x;
            std::memcpy(&x, &keyed[q].first, 8);
            d.tab.push_back(x);
        }
        d.idx[keyed[q].second] = (Idx)(d.tab.size() - 1);
    }
    return d;
}

// the element at rank size * pct / 100 of w (w is not empty; reordered, so take a copy once and
// ask it for every rank needed)
inline double percentile(std::vector<double>& w, int pct) {
    const size_t k = w.size() * pct / 100;
    std::nth_element(w.begin(), w.begin() + k, w.end());
    return w[k];
}

inline int max_weight(const std::vector<double>& w) {
    int mx = 0;
    for (double x : w) mx = std::max(mx, (int)x);
    return mx;
}

// device bytes of one staged array (an empty one still takes an element)
template <typename T>
size_t upload_size(const std::vector<T>& h) { return sizeof(T) * (h.empty() ? 1 : h.size()); }

// ---- the stages -------------------------------------------------------------------------------

// The in-rows sorted by (-w, u, eid), shared by K32, KB and KD (every out-arc a = (u -> v) appears
// in v's in-row), and the distance bound ecc_out(0) + ecc_in(0).  ok: the u16 kernels' limits hold
// (integer latencies, n, in-degrees, latencies and the bound below 65535, no parallel arcs).
struct InRows {
    bool ok = false;
    int bound = 0;
    std::vector<int> irow, order, src_of;  // offsets (n + 1); out-arc per in-row slot; tail per out-arc
    int* d_irow = nullptr;
    template <typename F> void arrays(F f) { if (ok) f("inrows.irow", irow, d_irow); }
};
inline InRows select_inrows(const SelectInput& in, const SelectKnobs& kn) {
    InRows I;
    const int n = in.n;
    if (!kn.integer_stages()) return I;
    if (!in.integer_w || n > 65535 || in.multigraph) return I;
    for (int a = 0; a < in.nnz; a++) if (in.w[a] > 65535.0) return I;
    std::vector<int> indeg(n, 0);
    for (int a = 0; a < in.nnz; a++) indeg[in.col[a]]++;
    for (int v = 0; v < n; v++) if (indeg[v] > 65535) return I;
    const double bound = ecc0(n, in.row, in.col, in.w) + ecc0(n, in.row_in, in.col_in, in.w_in);
    if (!(bound < 65535.0)) return I;
    I.ok = true;
    I.bound = (int)bound;
    I.irow.assign(n + 1, 0);
    for (int a = 0; a < in.nnz; a++) I.irow[in.col[a] + 1]++;
    for (int v = 0; v < n; v++) I.irow[v + 1] += I.irow[v];
    I.order.resize(in.nnz); I.src_of.resize(in.nnz);
    std::vector<int> fill(I.irow.begin(), I.irow.end() - 1);
    for (int u = 0; u < n; u++)
        for (int a = in.row[u]; a < in.row[u + 1]; a++) { I.src_of[a] = u; I.order[fill[in.col[a]]++] = a; }
    for (int v = 0; v < n; v++)
        std::sort(I.order.begin() + I.irow[v], I.order.begin() + I.irow[v + 1], [&](int x, int y) {
            if (in.w[x] != in.w[y]) return in.w[x] > in.w[y];
            if (I.src_of[x] != I.src_of[y]) return I.src_of[x] < I.src_of[y];
            return in.eid[x] < in.eid[y];
        });
    return I;
}

// K32: out-arc records carrying the slot of the same arc in its head's in-row, and the in-rows'
// tails and reliabilities.  Staged whenever the in-rows are (K2 and KB read them); ok: K32 may run.
struct K32Choice {
    bool staged = false, ok = false;
    int block = 256, bound = 0;
    size_t lds = 0;
    std::vector<ArcRec> arc;
    std::vector<uint16_t> col_in;
    std::vector<double> r_in;
    ArcRec* d_arc = nullptr;
    uint16_t* d_col_in = nullptr;
    double* d_r_in = nullptr;
    template <typename F> void arrays(F f) {
        if (!staged) return;
        f("k32.arc", arc, d_arc); f("k32.col_in", col_in, d_col_in); f("k32.r_in", r_in, d_r_in);
    }
};
inline K32Choice select_k32(const SelectInput& in, const SelectKnobs& kn, const InRows& I) {
    K32Choice k;
    if (!I.ok) return k;
    const int n = in.n;
    const K32Layout L = K32Layout::make(n);
    size_t lds = 0;
    int block = 0;
    for (int b : {256, 512, 1024}) {
        const size_t tot = k32_dispatch(b, [](auto B) { return k32_small_bytes<decltype(B)::value>(); }) + L.total;
        if (tot > kLdsBudget) continue;
        int per_cu = (int)(kLdsBudget / tot);
        if (per_cu * (b / 64) >= 16 || b == 1024) { block = b; lds = tot; break; }
    }
    k.staged = true;
    k.bound = I.bound;
    k.arc.resize(in.nnz); k.col_in.resize(in.nnz); k.r_in.resize(in.nnz);
    for (int v = 0; v < n; v++)
        for (int q = I.irow[v]; q < I.irow[v + 1]; q++) {
            int a = I.order[q];
            k.arc[a].rslot = (uint16_t)(q - I.irow[v]);
            k.col_in[q] = (uint16_t)I.src_of[a];
            k.r_in[q] = in.e_rel[in.eid[a]];
        }
    for (int a = 0; a < in.nnz; a++) {
        k.arc[a].col = (uint16_t)in.col[a];
        k.arc[a].w = (uint16_t)in.w[a];
        k.arc[a].pad = 0;
    }
    if (block && kn.wants("k32")) { k.ok = true; k.block = block; k.lds = lds; }
    return k;
}

// K2 path attributes: relv f64 + parent u16 per vertex in LDS
struct AttrChoice {
    bool ok = false;
    size_t lds = 0;
};
inline AttrChoice select_attr(const SelectInput& in, const InRows& I) {
    AttrChoice a;
    const AttrLayout AL = AttrLayout::make(in.n);
    if (I.ok && AL.total <= kLdsBudget) { a.ok = true; a.lds = AL.total; }
    return a;
}

// KD delta-stepping: bucket width ~ the 15th (22nd) percentile of arc latencies (>= 1), so ~15%
// (22%) of arcs are light; light in-arcs are the tail of each (-w)-sorted in-row
struct KDChoice {
    bool ok = false;
    int block = 1024, slots = 0, delta = 1, qcap = 0;
    size_t lds = 0, stride = 0;
    // the planner's unseeded hub rows on 256-thread contexts (C3): 1024-thread workgroups,
    // one row per CU, cut the latency of that launch (each row is unseeded and alone)
    int hub_block = 0, hub_qcap = 0, hub_delta = 1;
    size_t hub_lds = 0;
    int nlight = 0, nrtab = 1, walk = 0, packed = 0, fused = 0;
    int rone = -1;  // rtab index of exactly 1.0 (-1: none)
    std::vector<int> lrow;        // light in-CSR offsets (n+1)
    std::vector<uint32_t> orec;   // out-arc records v | w << 16 (| ridx << 24 when packed)
    std::vector<uint16_t> oridx;  // rtab index per out-arc
    std::vector<uint32_t> lrec;   // light in-arc records (2 x u32 per arc: u | w << 16, ridx)
    std::vector<double> rtab;     // distinct reliabilities
    int* d_lrow = nullptr;
    uint32_t* d_orec = nullptr;
    uint16_t* d_oridx = nullptr;
    uint32_t* d_lrec = nullptr;
    double* d_rtab = nullptr;
    template <typename F> void arrays(F f) {
        if (!ok) return;
        f("kd.lrow", lrow, d_lrow); f("kd.orec", orec, d_orec); f("kd.oridx", oridx, d_oridx);
        f("kd.lrec", lrec, d_lrec); f("kd.rtab", rtab, d_rtab);
    }
};
inline KDChoice select_kd(const SelectInput& in, const SelectKnobs& kn, const InRows& I, const K32Choice& k32) {
    KDChoice d;
    const int n = in.n;
    if (!I.ok || !kn.wants("kd") || in.nnz == 0) return d;
    // one 1024-thread workgroup per CU when dist fills the LDS; smaller graphs run several
    // 256-thread workgroups (sources) per CU
    const int blk = kn.kdblock ? kn.kdblock : n > 16384 ? 1024 : 256;
    // 1024-thread rows: the 15th percentile (38 on C4; seeded rows expand few vertices
    // per bucket, so fewer, wider buckets pay: C4 57 -> 53 ms from the 6th percentile's
    // 15.  Round-5 sweep, two reps each: 30/35/38-40/50/60 = 41.23-41.55/41.05/
    // 41.04-41.40/41.90/42.92 ms).  256-thread rows (three compute waves) take the
    // 22nd (55 on C3: 1.986 ms; 45/65/80 = 2.004-2.017/1.991/2.012-2.017 ms)
    std::vector<double> ws(in.w);
    const int delta = kn.delta.set ? kn.delta.v : std::max(1, (int)percentile(ws, blk >= 1024 ? 15 : 22));
    const size_t base = kd_dispatch(blk, [&](auto B) { return kd_lds_bytes<decltype(B)::value>(n, 0); });
    if (base + 2 * 512 > kLdsBudget) return d;
    // work queue: the rest of the CU's LDS at one workgroup per CU (large n), else
    // enough for a few workgroups per CU
    int qcap;
    if (blk < 768) {
        // four 256-thread workgroups per CU: the queue takes what is left of a quarter
        const size_t quarter = kLdsBudget / 4;
        qcap = base + 64 + 2 * 512 <= quarter ? (int)std::min<size_t>((size_t)n, (quarter - base - 64) / 2)
                                              : std::min(n, std::max(1024, n / 2));
    } else qcap = (int)std::min<size_t>((size_t)n, (kLdsBudget - base - 64) / 2);
    if (kn.qcap.set) qcap = std::min(qcap, kn.qcap.v);
    // (a multiple of 8, and never 0: with fewer than 8 vertices the rounding left an
    // empty queue, every vertex overflowed back to pending and the bucket loop spun)
    qcap = std::max(8, qcap & ~7);
    const size_t lds = kd_dispatch(blk, [&](auto B) { return kd_lds_bytes<decltype(B)::value>(n, qcap); });
    int maxdeg = 0;
    for (int v = 0; v < n; v++) maxdeg = std::max(maxdeg, in.row[v + 1] - in.row[v]);
    // reliability table: every distinct 1-loss value (exact bits), indexed by u16
    Distinct<uint16_t> rel = distinct_bits<uint16_t>(in.r, 65535);
    if (!(lds <= kLdsBudget && maxdeg <= 65535 && rel.ok)) return d;
    // out-arc records v | w << 16 (| ridx << 24 when packed); light in-CSR records
    // {u | w << 16, ridx}, light = w < delta.  Fused parents (found during the
    // expansion, 32-bit tie keys) need an undirected graph and packed records
    // (w < 256, <= 256 reliabilities); otherwise the in-CSR holds every in-arc and
    // phase B finds every parent.
    bool packed = max_weight(in.w) < 256 && rel.tab.size() <= 256;
    if (kn.kdpack.set) packed = packed && kn.kdpack.v != 0;
    const bool fused = !in.directed && packed;
    d.orec.resize(in.nnz);
    for (int a = 0; a < in.nnz; a++)
        d.orec[a] = (uint32_t)in.col[a] | ((uint32_t)in.w[a] << 16) | (packed ? (uint32_t)rel.idx[a] << 24 : 0u);
    d.lrow.assign(n + 1, 0);
    for (int v = 0; v < n; v++) {
        for (int q = I.irow[v]; q < I.irow[v + 1]; q++) {
            const int a = I.order[q];
            if (fused && (int)in.w[a] >= delta) continue;
            d.lrec.push_back((uint32_t)k32.col_in[q] | ((uint32_t)in.w[a] << 16));
            d.lrec.push_back(rel.idx[a]);
        }
        d.lrow[v + 1] = (int)(d.lrec.size() / 2);
    }
    if (d.lrec.empty()) d.lrec.assign(2, 0u);
    d.ok = true; d.block = blk; d.lds = lds; d.delta = delta; d.qcap = qcap;
    d.packed = packed ? 1 : 0;
    d.fused = fused ? 1 : 0;
    d.nlight = d.lrow[n];
    d.nrtab = std::max<int>(1, (int)rel.tab.size());
    for (int q = 0; q < (int)rel.tab.size(); q++)
        if (rel.tab[q] == 1.0) d.rone = q;
    d.oridx = std::move(rel.idx);
    d.rtab = std::move(rel.tab);
    // 16 waves per CU: 4 per SIMD at <= 128 VGPRs (amdgpu_waves_per_eu(4))
    const int per_cu = std::max(1, std::min((int)(kLdsBudget / lds), 1024 / blk));
    d.slots = 256 * per_cu;
    if (kn.kdgrid.set) d.slots = std::max(1, std::min(d.slots, kn.kdgrid.v));
    d.stride = kd_ws_stride(n);
    if (blk < 1024 && !kn.delta.set && !kn.qcap.set) {
        // hub rows in 1024-thread workgroups: that block's queue and bucket width
        const size_t hb = kd_lds_bytes<1024>(n, 0);
        if (hb + 2 * 512 <= kLdsBudget) {
            const int hq = std::max(8, (int)std::min<size_t>((size_t)n, (kLdsBudget - hb - 64) / 2) & ~7);
            const size_t hl = kd_lds_bytes<1024>(n, hq);
            if (hl <= kLdsBudget) {
                d.hub_block = 1024; d.hub_qcap = hq; d.hub_lds = hl;
                // (the light in-CSR above holds the in-arcs with w < delta, and a
                // row's fused parents are exact only if its bucket width is at most
                // that: the hub rows' 12th percentile never exceeds the context's)
                d.hub_delta = std::min(delta, std::max(1, (int)percentile(ws, 12)));
            }
        }
        if (kn.hub1024.set && kn.hub1024.v == 0) d.hub_block = 0;
    }
    d.walk = kd_dispatch(blk, [&](auto B) { return kd_walk_fits<decltype(B)::value>(n, qcap, d.nrtab); }) ? 1 : 0;
    if (kn.kdwalk.set) d.walk = d.walk && kn.kdwalk.v != 0;
    return d;
}

// KB batched kernel: packed in-arcs (u << 16 | w) in the sorted in-row order, staged whenever the
// in-rows are; segments of <= KB_SEG in-arcs, hub rows split.  fused: sssp_batch_rows_kernel
// (the rows in one kernel: no key rows, no K2).
struct KBChoice {
    bool staged = false, ok = false;
    int nseg = 0, nhub = 0, npart = 0;
    size_t lds = 0;
    int fused = 0, f_nrtab = 0, grid_cap = 0, f_tcap = 0;
    size_t f_lds = 0;
    std::vector<uint32_t> arc;   // in-arcs u << 16 | w
    std::vector<KBSeg> segs;
    std::vector<KBHub> hubs;
    std::vector<uint32_t> farc;  // fused: in-arcs u << 16 | ridx << 8 | w
    std::vector<double> rtab;    // fused: distinct reliabilities
    uint32_t* d_arc = nullptr;
    KBSeg* d_seg = nullptr;
    KBHub* d_hub = nullptr;
    uint32_t* d_farc = nullptr;
    double* d_rtab = nullptr;
    template <typename F> void packed_arrays(F f) { if (staged) f("kb.arc", arc, d_arc); }  // (uploaded ahead of KD's)
    template <typename F> void arrays(F f) {
        if (ok) f("kb.segs", segs, d_seg);
        if (ok && !hubs.empty()) f("kb.hubs", hubs, d_hub);
        if (fused) { f("kb.farc", farc, d_farc); f("kb.rtab", rtab, d_rtab); }
    }
};
inline KBChoice select_kb(const SelectInput& in, const SelectKnobs& kn, const InRows& I, const K32Choice& k32,
                          const AttrChoice& attr) {
    KBChoice b;
    const int n = in.n;
    if (!I.ok) return b;
    b.staged = true;
    b.arc.assign(((size_t)in.nnz + 3) / 4 * 4, 0u);
    for (int q = 0; q < in.nnz; q++) b.arc[q] = ((uint32_t)k32.col_in[q] << 16) | (uint32_t)in.w[I.order[q]];
    if (!attr.ok || !kn.wants("kb")) return b;
    std::vector<KBSeg> segs;
    std::vector<KBHub> hubs;
    int npart = 0;
    for (int v = 0; v < n; v++) {
        const int a0 = I.irow[v], a1 = I.irow[v + 1];
        if (a1 - a0 <= KB_SEG) { segs.push_back({v, a0, a1, -1}); continue; }
        KBHub h{v, npart, 0, 0};
        for (int a = a0; a < a1; a += KB_SEG) segs.push_back({v, a, std::min(a1, a + KB_SEG), npart++});
        h.p1 = npart;
        hubs.push_back(h);
    }
    // equal-length segments side by side: a wave's lanes finish their rows together
    std::stable_sort(segs.begin(), segs.end(),
                     [](const KBSeg& x, const KBSeg& y) { return (x.a1 - x.a0) > (y.a1 - y.a0); });
    // thread t takes segments t, t + KB_BLOCK, ...: a sweep lasts as long as the wave
    // whose lanes' longest segments add up most.  Each block of KB_BLOCK segments may
    // run long->short or short->long over the threads; pick the directions with the
    // smallest such wave time (C2: 29 -> 22 arc steps; the mean is 20)
    {
        const int nb = ((int)segs.size() + KB_BLOCK - 1) / KB_BLOCK;
        constexpr int kWaves = KB_BLOCK / 64;
        auto cost = [&](unsigned dirs) {
            int wt[kWaves] = {0};
            for (int b = 0; b < nb; b++) {
                const int k0 = b * KB_BLOCK, cnt = std::min((int)segs.size() - k0, KB_BLOCK);
                for (int w = 0; w < kWaves; w++) {
                    int mx = 0;
                    for (int l = w * 64; l < std::min(cnt, w * 64 + 64); l++) {
                        const KBSeg& sg = segs[k0 + (((dirs >> b) & 1u) ? cnt - 1 - l : l)];
                        mx = std::max(mx, sg.a1 - sg.a0);
                    }
                    wt[w] += mx;
                }
            }
            return *std::max_element(wt, wt + kWaves);
        };
        unsigned best = 0;
        if (nb <= 12) {
            int bc = cost(0);
            for (unsigned d = 1; d < (1u << nb); d++) {
                const int c2 = cost(d);
                if (c2 < bc) { bc = c2; best = d; }
            }
        }
        for (int b = 0; b < nb; b++)
            if ((best >> b) & 1u) {
                const int k0 = b * KB_BLOCK, cnt = std::min((int)segs.size() - k0, KB_BLOCK);
                std::reverse(segs.begin() + k0, segs.begin() + k0 + cnt);
            }
    }
    const size_t kbl = kKBSmall + KBLayout::make(n, in.nnz, npart).total;
    if (kbl > kLdsBudget) return b;
    b.ok = true; b.lds = kbl; b.nseg = (int)segs.size(); b.nhub = (int)hubs.size(); b.npart = npart;
    // fused rows (no key rows, no K2): records u << 16 | ridx << 8 | w need w < 256 and
    // <= 254 distinct reliabilities; parent records of <= KB_RIT segments per thread
    Distinct<uint8_t> rel = distinct_bits<uint8_t>(k32.r_in, KB_ONE);
    // staged targets: as many as the rest of the LDS holds (one chunk when nt <= n)
    const size_t fb0 = kKBSmall + KBLayout::make(n, in.nnz, npart, true, 0).total;
    int tcap = fb0 < kLdsBudget ? (int)std::min<size_t>((size_t)n, (kLdsBudget - fb0 - 64) / 4) : 0;
    tcap = tcap >= 64 ? (tcap & ~63) : 0;
    const size_t fbl = kKBSmall + KBLayout::make(n, in.nnz, npart, true, tcap).total;
    bool fuse = max_weight(in.w) < 256 && rel.ok && (int)segs.size() <= KB_RIT * KB_BLOCK &&
                (int)hubs.size() <= KB_BLOCK && in.nnz < 0xFFFF && KB_SRC * n <= KB_CV * KB_BLOCK && npart < 0xFFFF &&
                tcap >= 64 && fbl <= kLdsBudget;
    if (kn.kbtcap.set) tcap = std::max(64, std::min(tcap, kn.kbtcap.v) & ~63);
    if (kn.kbfuse.set) fuse = fuse && kn.kbfuse.v != 0;
    if (fuse) {
        b.farc.assign(((size_t)in.nnz + 3) / 4 * 4, 0u);
        for (int q = 0; q < in.nnz; q++)
            b.farc[q] = ((uint32_t)k32.col_in[q] << 16) | ((uint32_t)rel.idx[q] << 8) | (uint32_t)in.w[I.order[q]];
        b.fused = 1; b.f_lds = fbl; b.f_nrtab = (int)rel.tab.size(); b.f_tcap = tcap;
        b.rtab = std::move(rel.tab);
    }
    if (kn.kbgrid.set) b.grid_cap = std::max(1, kn.kbgrid.v);
    b.segs = std::move(segs);
    b.hubs = std::move(hubs);
    return b;
}

// KF (graphs the integer kernels do not take): per in-arc index of its 1 - loss in a table of
// the distinct values, bucket width, block size.  Fits when the per-source LDS state does and
// every thread holds at most 16 vertices in the level passes (n <= 16 B); above that KFH
// (n <= 65535: the ring is u16), one 1024-thread workgroup per CU with its vertex state in an
// HBM slice (C4f: 550 KB per slice).
struct KFChoice {
    bool ok = false;
    int block = 0, slots = 0;
    size_t lds = 0;
    double delta = 1.0;
    int nrtab = 0;
    int h = 0;  // KFH: the per-vertex state in a per-workgroup HBM slice (n > ~12k)
    size_t ws_stride = 0;
    double wscale = 0.0;  // packed arcs (head | k << 16, weight k / wscale), or 0
    bool ipk_own = false;  // directed: the in-arcs are packed on their own (else ipk is opk)
    std::vector<uint8_t> rix;
    std::vector<double> rtab;
    std::vector<uint32_t> opk, ipk;
    uint8_t* d_rix = nullptr;
    double* d_rtab = nullptr;
    uint32_t* d_opk = nullptr;
    uint32_t* d_ipk = nullptr;
    template <typename F> void arrays(F f) {
        if (!ok) return;
        f("kf.rix", rix, d_rix); f("kf.rtab", rtab, d_rtab);
        if (wscale > 0.0) f("kf.opk", opk, d_opk);
        if (wscale > 0.0 && ipk_own) f("kf.ipk", ipk, d_ipk);
    }
};
inline KFChoice select_kf(const SelectInput& in, const SelectKnobs& kn) {
    KFChoice k;
    const int n = in.n;
    if (!kn.wants("kf")) return k;
    if (in.nnz == 0 || n > 65535) return k;
    Distinct<uint8_t> rel = distinct_bits<uint8_t>(in.r_in, 254);  // (255 marks unreachable)
    if (!rel.ok) return k;
    int blk = 0;
    size_t lds = 0;
    bool hbm = false;
    if (n <= 16 * 256 && kf_lds_bytes<256>(n) <= kLdsBudget / 4) { blk = 256; lds = kf_lds_bytes<256>(n); }
    else if (n <= 16 * 1024 && kf_lds_bytes<1024>(n) <= kLdsBudget) { blk = 1024; lds = kf_lds_bytes<1024>(n); }
    else if (n <= 64 * 1024 && kfh_lds_bytes<1024>(n) <= kLdsBudget) { blk = 1024; lds = kfh_lds_bytes<1024>(n); hbm = true; }
    if (kn.kfh.set && kn.kfh.v && n <= 64 * 1024 && kfh_lds_bytes<1024>(n) <= kLdsBudget) {
        blk = 1024; lds = kfh_lds_bytes<1024>(n); hbm = true;
    }
    if (!blk) return k;
    // bucket width: the 40th percentile of arc latencies (KF rounds cost far more than the
    // re-expansions wider buckets bring: C3f 15.0 / 13.4 / 13.1 ms at the 12th / 25th / 50th,
    // C2f 0.60 / 0.55 / 0.57 ms); KFH the 10th, where a re-expansion is HBM traffic (C4f, the
    // width in ms: 15 / 25 / 35 / 50 / 70 / ~100 (40th) / 200: 822 / 815 / 822 / 835 / 842 /
    // 886 / 1061 ms)
    std::vector<double> ws(in.w_in);
    double delta = kn.kfdelta_set ? kn.kfdelta : percentile(ws, hbm ? 10 : 40);
    if (!(delta > 0.0) || std::isinf(delta)) delta = in.min_w > 0 ? in.min_w : 1.0;
    // Packed arcs (KFH): when every latency is a decimal k / scale (scale 1, 10, 100 or 1000)
    // with k < 65536, an arc is one u32, head | k << 16, and the kernel divides k by the scale
    // -- IEEE division of two exact integers is the correctly rounded k / scale, the double the
    // decimal parses to, and each arc is checked here (C4f's latencies have two decimals: 4
    // bytes per arc read instead of 12; C4f 780 -> 764 ms).  The LDS kernels keep f64 arcs:
    // there the division costs more than the bytes (C3f 10.39 -> 10.59, C2f 0.45 -> 0.49 ms)
    double wscale = 0.0;
    if (hbm && !(kn.kfpk.set && kn.kfpk.v == 0)) {
        for (const double sc : {1.0, 10.0, 100.0, 1000.0}) {
            auto fits = [&](const std::vector<double>& ws) {
                for (const double x : ws) {
                    const double k = std::nearbyint(x * sc);
                    if (!(k >= 1.0 && k <= 65535.0) || k / sc != x) return false;
                }
                return true;
            };
            if (fits(in.w) && (in.directed ? fits(in.w_in) : true)) { wscale = sc; break; }
        }
    }
    if (wscale > 0.0) {
        auto pack = [&](const std::vector<int>& cc, const std::vector<double>& ws) {
            std::vector<uint32_t> pk(cc.size());
            for (size_t a = 0; a < cc.size(); a++)
                pk[a] = (uint32_t)cc[a] | ((uint32_t)std::nearbyint(ws[a] * wscale) << 16);
            return pk;
        };
        k.opk = pack(in.col, in.w);
        k.ipk_own = in.directed;
        if (in.directed) k.ipk = pack(in.col_in, in.w_in);
        k.wscale = wscale;
    }
    k.ok = true;
    k.block = blk; k.lds = lds; k.delta = delta; k.nrtab = (int)rel.tab.size();
    k.slots = 256 * std::max(1, std::min((int)(kLdsBudget / lds), 1024 / blk));
    if (hbm) { k.h = 1; k.ws_stride = kfh_ws_stride<1024>(n); }
    k.rix = std::move(rel.idx);
    k.rtab = std::move(rel.tab);
    return k;
}

// The whole decision.  sel: 0 f64, 1 K32, 2 KB+K2, 4 KD, 5 KF (3: the retired K16)
struct Selection {
    InRows inrows;
    K32Choice k32;
    AttrChoice attr;
    KBChoice kb;
    KDChoice kd;
    KFChoice kf;
    int sel = 0;
    uint64_t upload_bytes = 0;  // device bytes of every staged array
    // f(name, host vector, device pointer) for every staged array, in upload order
    template <typename F> void arrays(F f) {
        inrows.arrays(f); k32.arrays(f); kb.packed_arrays(f); kd.arrays(f); kb.arrays(f); kf.arrays(f);
    }
};

// KB (C2-class) wins over KD (C3/C4-class), KD over K32; KF is tried only for what is left to f64.
inline Selection select_all(const SelectInput& in, const SelectKnobs& kn) {
    Selection s;
    s.inrows = select_inrows(in, kn);
    s.k32 = select_k32(in, kn, s.inrows);
    s.attr = select_attr(in, s.inrows);
    s.kd = select_kd(in, kn, s.inrows, s.k32);
    s.kb = select_kb(in, kn, s.inrows, s.k32, s.attr);
    s.sel = s.kb.ok ? 2 : s.kd.ok ? 4 : s.k32.ok ? 1 : 0;
    if (s.sel == 0) {
        s.kf = select_kf(in, kn);
        if (s.kf.ok) s.sel = 5;
    }
    s.arrays([&](const char*, auto& h, auto*&) { s.upload_bytes += upload_size(h); });
    return s;
}

}  // namespace shd
