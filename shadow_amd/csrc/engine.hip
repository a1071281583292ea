// engine.hip -- host side of the routing engine (C-ABI in include/shd_route.h): creation,
// selection, the rows, K4, the fill, host memory and the stats.  The seeded-row planner
// (shd_route_plan_*) is plan.hpp and the path calls (hops, link loads, tie envelope) are
// path_calls.hpp over the host-only stages of path_host.hpp, both included below once their
// prerequisites are defined.
#include "common.hpp"

#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sys/mman.h>

#include <thread>
#include "sssp_f64.hpp"
#include "sssp_f64d.hpp"
#include "sssp_k32.hpp"
#include "sssp_batch.hpp"
#include "path_attr.hpp"
#include "sssp_delta.hpp"
#include "direct_fw.hpp"
#include "fw.hpp"
#include "path_hops.hpp"
#include "link_loads.hpp"
#include "path_ties.hpp"
#include "ecmp_loads.hpp"
#include "path_fold.hpp"
#include "link_loss.hpp"
#include "link_outage.hpp"
#include "link_reprice.hpp"
#include "fill_sched.hpp"
#include "select.hpp"
#include "path_host.hpp"

using namespace shd;

// =============================================================================
// Host side
// =============================================================================
// The planner's host workers: one process-wide set, created with the first context that plans
// (KD) and parked on a condition variable between plans, so a plan does not pay ~15 thread
// creations (~0.5 ms).  run(f) starts f on every worker; wait() returns once all of them have
// returned from it.  A plan that finds the set in use (plans on several devices at once)
// starts its own.
struct HostPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, cv_done;
    std::function<void()> fn;
    uint64_t gen = 0;
    int busy = 0;
    bool stop = false;
    explicit HostPool(int n) {
        for (int i = 0; i < n; i++) th.emplace_back([this] { loop(); });
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                f = fn;
            }
            f();
            std::lock_guard<std::mutex> l(m);
            if (--busy == 0) cv_done.notify_all();
        }
    }
    void run(std::function<void()> f) {
        std::lock_guard<std::mutex> l(m);
        fn = std::move(f);
        busy = (int)th.size();
        gen++;
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> l(m);
        cv_done.wait(l, [&] { return busy == 0; });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> l(m);
            stop = true;
        }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};

struct shd_route {
    int device = 0;
    int n = 0, m = 0, nnz = 0;
    int directed = 0, prefer_direct = 0, complete = 0, integer_w = 0, multigraph = 0;
    int self16 = 1;  // every self-loop latency (the table's diagonal) is an integer below 0xFFFF
    double min_w = 0, max_w = 0;
    // device graph
    int* d_row = nullptr; int* d_col = nullptr; double* d_w = nullptr; double* d_r = nullptr;
    int* d_row_in = nullptr; int* d_col_in = nullptr; double* d_w_in = nullptr; double* d_r_in = nullptr;
    double* d_vf = nullptr; double* d_self_w = nullptr; double* d_self_r = nullptr;
    double* d_W = nullptr; double* d_R = nullptr;  // dense direct tables (complete graphs, lazy)
    int* d_err = nullptr;
    char* d_ws = nullptr; size_t ws_stride = 0; int ws_slots = 0;
    bool lds = false;
    size_t lds_bytes = 0;
    // the rows kernel chosen at creation and what it reads (select.hpp; apply_selection):
    // sel 0 f64, 1 K32 (sssp_k32.hpp), 2 KB (sssp_batch.hpp) + K2 path attributes
    // (path_attr.hpp), 4 KD (sssp_delta.hpp), 5 KF (sssp_f64d.hpp); 3 was the retired K16
    int sel = 0;
    InRows inrows;
    K32Choice k32;
    AttrChoice attr;
    KBChoice kb;
    KDChoice kd;
    KFChoice kf;
    unsigned long long* d_dbg = nullptr;  // SHD_STAMPS builds: per-source phase stamps
    uint32_t* d_keys = nullptr;     // KB key rows scratch (ns x n u32), grown on demand
    size_t keys_cap = 0;
    char* d_kd_ws = nullptr;  // KD: the workgroup slices (kd.stride each, kd.slots of them)
    unsigned long long* d_kd_stats = nullptr;  // KD liveness counters (shd_route_kd_stats)
    int* d_kd_next = nullptr;  // KD source queue counter
    char* d_kf_ws = nullptr;  // KFH: the workgroup slices of the per-vertex state
    int has_vf = 0;  // some vertex has a packet-loss factor (else f_v is absent everywhere)
    int vf_lossy = 0;  // some vertex factor is not exactly 1.0 (else every present f_v is a no-op)
    int* d_fwflag = nullptr;  // K4: per pivot, its closed tile is published (fw_restp_kernel)
    // host copies for seeded planning (shd_route_plan_*): out-CSR, rtab index per arc and
    // the landmark closeness of every vertex (computed on the first plan)
    std::vector<int> h_row, h_col;
    std::vector<double> h_w;
    std::vector<uint16_t> h_ridx;
    std::vector<double> close;
    // landmark rows (planner): the most central vertices' distances and tie-rule parent
    // records computed on the host, uploaded as seed rows for the plan's roots
    std::vector<int> lm_v;
    std::vector<uint16_t> lm_hd;  // landmark l's u16 distance of v at [l * lm_rs + v] (0xFFFF: unreached)
    std::vector<uint32_t> lm_hp;  // and its parent record
    long long lm_rs = 0;
    uint16_t* d_lm_drow = nullptr;  // the landmark rows in the row-store format (device)
    uint32_t* d_lm_prow = nullptr;
    char* d_hub_ws = nullptr;       // the planner's hub-row launch scratch (kept: a free costs a sync)
    size_t hub_ws_bytes = 0;
    // K4 (fw.hpp): u16 all-pairs table + dense u16 weights, Np x Np (Np = n rounded to 64)
    uint16_t* d_fwD = nullptr;
    uint32_t* d_fwinl = nullptr;  // K4 parent search: sorted in-arc keys per vertex (np x np)
    uint16_t* d_fwpos = nullptr;  // and the start index per small threshold (n x FW_X)
    uint32_t* d_fwkey = nullptr;
    uint8_t* d_fwrix = nullptr;  // K4 rows: reliability index of each arc (dense n x n u8)
    double* d_fwrtab = nullptr;  // and the distinct reliabilities (fw_nrtab <= 255; 0: dense R reads)
    int fw_pk = 0;               // K4 in-list keys carry the parent arc's reliability index
    int fw_nrtab = 0;
    size_t fwkey_cap = 0;
    int fw_np = 0, fw_ready = 0;
    PathDev path;  // hops, link loads and tie envelope (path_calls.hpp)
    uint64_t device_bytes = 0;
    // host copies needed for lazy dense build
    std::vector<int32_t> e_src, e_dst;
    std::vector<double> e_lat, e_rel;
    std::vector<double> e_loss, v_loss;  // the losses as given (v_loss NaN = absent): the link loss columns
    std::vector<void*> allocs;
};

namespace {

HostPool* host_pool();  // (plan.hpp; shd_route_create starts the planner's workers)
void path_free(PathDev& p);  // (path_calls.hpp; shd_route_destroy frees the path calls' buffers)

int hip_check(hipError_t e) { return e == hipSuccess ? SHD_ROUTE_OK : SHD_ROUTE_EDEVICE; }

template <typename T>
int upload(shd_route* c, T** dptr, const std::vector<T>& h) {
    size_t bytes = sizeof(T) * (h.empty() ? 1 : h.size());
    if (hipMalloc((void**)dptr, bytes) != hipSuccess) return SHD_ROUTE_ENOMEM;
    c->allocs.push_back(*dptr);
    c->device_bytes += bytes;
    if (!h.empty() && hipMemcpy(*dptr, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

DevGraph dev_graph(const shd_route* c) {
    DevGraph g;
    g.n = c->n; g.prefer_direct = c->prefer_direct;
    g.row = c->d_row; g.col = c->d_col; g.w = c->d_w; g.r = c->d_r;
    g.row_in = c->d_row_in; g.col_in = c->d_col_in; g.w_in = c->d_w_in; g.r_in = c->d_r_in;
    g.vf = c->d_vf; g.self_w = c->d_self_w; g.self_r = c->d_self_r;
    return g;
}

bool strongly_connected(int n, const std::vector<int>& row, const std::vector<int>& col,
                        const std::vector<int>& row_in, const std::vector<int>& col_in) {
    auto reach_all = [&](const std::vector<int>& R, const std::vector<int>& Cc) {
        std::vector<char> seen(n, 0);
        std::vector<int> st{0};
        seen[0] = 1;
        int cnt = 1;
        while (!st.empty()) {
            int u = st.back(); st.pop_back();
            for (int a = R[u]; a < R[u + 1]; a++)
                if (!seen[Cc[a]]) { seen[Cc[a]] = 1; cnt++; st.push_back(Cc[a]); }
        }
        return cnt == n;
    };
    return reach_all(row, col) && reach_all(row_in, col_in);
}

int alloc_ws(shd_route* c) {
    // per-source state in HBM when it cannot live in LDS
    StateLayout L = StateLayout::make(c->n);
    c->ws_stride = a16(L.total) + 256;
    c->ws_slots = 1024;  // 256 CUs x 4 workgroups
    size_t bytes = c->ws_stride * (size_t)c->ws_slots;
    if (hipMalloc((void**)&c->d_ws, bytes) != hipSuccess) return SHD_ROUTE_ENOMEM;
    c->allocs.push_back(c->d_ws);
    return SHD_ROUTE_OK;
}

int ensure_dense(shd_route* c) {
    if (c->d_W) return SHD_ROUTE_OK;
    const size_t nn = (size_t)c->n * c->n;
    std::vector<double> W(nn, NAN), R(nn, NAN);
    // igraph_get_eid on a simple graph returns the unique edge; for parallel edges we
    // keep the lowest edge id (documented deviation, SURVEY hazard H3).
    for (int e = c->m - 1; e >= 0; e--) {
        int a = c->e_src[e], b = c->e_dst[e];
        W[(size_t)a * c->n + b] = c->e_lat[e];
        R[(size_t)a * c->n + b] = c->e_rel[e];
        if (!c->directed) {
            W[(size_t)b * c->n + a] = c->e_lat[e];
            R[(size_t)b * c->n + a] = c->e_rel[e];
        }
    }
    int rc = upload(c, &c->d_W, W);
    if (rc) return rc;
    return upload(c, &c->d_R, R);
}

// Uploads what the selection staged, allocates the chosen kernels' workspaces and counters, raises
// their dynamic-LDS limits, and stores the choice in the context.
int apply_selection(shd_route* c, Selection&& s) {
    int rc = SHD_ROUTE_OK;
    auto up = [&](const char*, auto& h, auto*& d) { if (!rc) rc = upload(c, &d, h); };
    auto lds_attr = [&](const void* fn, size_t lds) {
        return hip_check(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    };
    s.inrows.arrays(up);
    s.k32.arrays(up);
    if (rc) return rc;
    if (s.k32.ok &&
        (rc = lds_attr(k32_dispatch(s.k32.block, [](auto B) { return (const void*)sssp_k32_kernel<decltype(B)::value>; }),
                       s.k32.lds)))
        return rc;
    if (s.attr.ok && (rc = lds_attr((const void*)path_attr_kernel<256>, s.attr.lds))) return rc;
    s.kb.packed_arrays(up);
    if (rc) return rc;
    if (s.kd.ok) {
        s.kd.arrays(up);
        if (rc) return rc;
        if (hipMalloc((void**)&c->d_kd_ws, s.kd.stride * (size_t)s.kd.slots) != hipSuccess) return SHD_ROUTE_ENOMEM;
        c->allocs.push_back(c->d_kd_ws);
        if (hipMalloc((void**)&c->d_kd_next, sizeof(int)) != hipSuccess) return SHD_ROUTE_ENOMEM;
        c->allocs.push_back(c->d_kd_next);
        if (hipMalloc((void**)&c->d_kd_stats, sizeof(unsigned long long) * 4) != hipSuccess ||
            hipMemset(c->d_kd_stats, 0, sizeof(unsigned long long) * 4) != hipSuccess)
            return SHD_ROUTE_ENOMEM;
        c->allocs.push_back(c->d_kd_stats);
        kd_dispatch(s.kd.block, [&](auto B) {
            if (!(rc = lds_attr((const void*)sssp_delta_kernel<decltype(B)::value>, s.kd.lds)))
                rc = lds_attr((const void*)kd_plan_rows_kernel<decltype(B)::value>, s.kd.lds);
            return 0;
        });
        if (rc) return rc;
        // (the hub rows are an extra: without their LDS limit the context's own rows serve)
        if (s.kd.hub_block && lds_attr((const void*)kd_plan_rows_kernel<1024>, s.kd.hub_lds)) {
            s.kd.hub_block = 0; s.kd.hub_qcap = 0; s.kd.hub_lds = 0; s.kd.hub_delta = 1;
        }
    }
    s.kb.arrays(up);
    if (!rc && s.kb.ok) rc = lds_attr((const void*)sssp_batch_kernel, s.kb.lds);
    if (!rc && s.kb.fused) rc = lds_attr((const void*)sssp_batch_rows_kernel, s.kb.f_lds);
    if (rc) return rc;
    if (s.kf.ok) {
        s.kf.arrays(up);
        if (s.kf.wscale > 0.0 && !s.kf.ipk_own) s.kf.d_ipk = s.kf.d_opk;
        if (!rc)
            rc = lds_attr(kf_dispatch(s.kf.block, s.kf.h, s.kf.wscale > 0.0, [](auto B, auto H, auto P) {
                return (const void*)sssp_f64d_kernel<decltype(B)::value, decltype(H)::value, decltype(P)::value>;
            }), s.kf.lds);
        if (rc) return rc;
        if (s.kf.h) {
            if (hipMalloc((void**)&c->d_kf_ws, s.kf.ws_stride * (size_t)s.kf.slots) != hipSuccess) return SHD_ROUTE_ENOMEM;
            c->allocs.push_back(c->d_kf_ws);
        }
    }
    // the staged copies have served, but for the planner's rtab index per arc
    c->h_ridx = std::move(s.kd.oridx);
    s.arrays([](const char*, auto& h, auto*&) { std::remove_reference_t<decltype(h)>().swap(h); });
    s.inrows.order = {}; s.inrows.src_of = {};
    c->sel = s.sel;
    c->inrows = std::move(s.inrows); c->k32 = std::move(s.k32); c->attr = s.attr;
    c->kb = std::move(s.kb); c->kd = std::move(s.kd); c->kf = std::move(s.kf);
    return SHD_ROUTE_OK;
}

DevDelta kd_args(const shd_route* c) {
    DevDelta k;
    k.n = c->n; k.nw = (c->n + 63) / 64; k.bound = c->k32.bound; k.delta = c->kd.delta;
    k.fused = c->kd.fused; k.rc = c->kd.qcap;
    k.row = c->d_row; k.orec = c->kd.d_orec; k.oridx = c->kd.d_oridx;
    k.nnz = c->nnz; k.lrow = c->kd.d_lrow; k.lrec = reinterpret_cast<const uint2*>(c->kd.d_lrec); k.nlight = c->kd.nlight;
    k.rtab = c->kd.d_rtab; k.nrtab = c->kd.nrtab; k.rone = c->kd.rone; k.walk = c->kd.walk; k.packed = c->kd.packed;
    k.vf = c->d_vf; k.self_w = c->d_self_w; k.self_r = c->d_self_r; k.dbg = c->d_dbg; k.dflags = 0;
    // a factor of exactly 1.0 multiplies as a no-op: KD reads vf only where one is not
    k.has_vf = c->vf_lossy;
#ifdef SHD_STAMPS
    if (const char* e = getenv("SHD_ROUTE_DFLAGS")) k.dflags = atoi(e);
#endif
    k.seed_drop = 0;
    if (const char* e = getenv("SHD_ROUTE_SEEDDROP")) k.seed_drop = atoi(e) & ~1;

    k.jobs = nullptr; k.drow = nullptr; k.drow_out = nullptr; k.prow = nullptr; k.rstride = 0; k.evcap = c->n;
    k.done = nullptr;
    // tests shrink the tie-event list to force the unseeded rerun of overflowing rows
    if (const char* e = getenv("SHD_ROUTE_EVCAP")) k.evcap = std::max(0, std::min(c->n, atoi(e)));
    // and cap a chunk of phase A' at a few events, so that small graphs take several chunks
    k.evchunk = 0;
    if (const char* e = getenv("SHD_ROUTE_EVCHUNK")) k.evchunk = std::max(0, atoi(e));
    k.next = nullptr;
    k.stats = c->d_kd_stats;
    return k;
}

// one KD launch of ns sources (k.jobs: planned jobs, else d_src); `next` is zeroed
int kd_launch(shd_route* c, DevDelta k, int* next, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt,
              int64_t ld, double* d_lat, double* d_rel, double* d_row_min, hipStream_t st, bool planner = false,
              char* ws = nullptr, int max_grid = 0, bool hub = false) {
    if (ns <= 0) return SHD_ROUTE_OK;
    k.next = next;
    if (!ws) ws = c->d_kd_ws;
    const int grid = std::min(ns, max_grid > 0 ? std::min(max_grid, c->kd.slots) : c->kd.slots);
    // (hub: the planner's rows in 1024-thread workgroups where the context's are smaller)
    const bool big = hub && planner && c->kd.hub_block > 0;
    size_t lds = c->kd.lds;
    if (big) { k.rc = c->kd.hub_qcap; k.delta = c->kd.hub_delta; lds = c->kd.hub_lds; }
    kd_dispatch(big ? c->kd.hub_block : c->kd.block, [&](auto B) {
        constexpr int b = decltype(B)::value;
        if (planner)
            hipLaunchKernelGGL(kd_plan_rows_kernel<b>, dim3(grid), dim3(b), lds, st, k, d_src, ns, d_tgt,
                               nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err, ws, c->kd.stride);
        else
            hipLaunchKernelGGL(sssp_delta_kernel<b>, dim3(grid), dim3(b), c->kd.lds, st, k, d_src, ns, d_tgt,
                               nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err, ws, c->kd.stride);
        return 0;
    });
    return hip_check(hipGetLastError());
}

DevKB kb_args(const shd_route* c, int ns) {
    DevKB kb;
    kb.n = c->n; kb.nnz = c->nnz; kb.nseg = c->kb.nseg; kb.nhub = c->kb.nhub; kb.npart = c->kb.npart;
    kb.bound = c->k32.bound; kb.arc = c->kb.fused ? c->kb.d_farc : c->kb.d_arc; kb.row_in = c->inrows.d_irow;
    kb.seg = c->kb.d_seg; kb.hub = c->kb.d_hub;
    kb.rtab = c->kb.d_rtab; kb.nrtab = c->kb.f_nrtab; kb.tcap = c->kb.f_tcap;
    kb.vf = c->d_vf; kb.self_w = c->d_self_w; kb.self_r = c->d_self_r;
    kb.dbg = c->d_dbg ? c->d_dbg + (size_t)ns * 8 : nullptr;
    return kb;
}

DevAttr attr_args(const shd_route* c) {
    DevAttr at;
    at.n = c->n; at.row_in = c->inrows.d_irow; at.col_in = c->k32.d_col_in; at.r_in = c->k32.d_r_in;
    at.vf = c->d_vf; at.self_w = c->d_self_w; at.self_r = c->d_self_r;
    at.dbg = c->d_dbg;
    return at;
}

DevK32 k32_args(const shd_route* c) {
    DevK32 k;
    k.n = c->n; k.bound = c->k32.bound; k.row = c->d_row; k.arc = c->k32.d_arc; k.row_in = c->inrows.d_irow;
    k.col_in = c->k32.d_col_in; k.r_in = c->k32.d_r_in; k.vf = c->d_vf; k.self_w = c->d_self_w;
    k.self_r = c->d_self_r;
    k.dbg = c->d_dbg;
    return k;
}

DevF64D kf_args(const shd_route* c) {
    DevF64D k;
    k.n = c->n; k.nw = (c->n + 63) / 64; k.delta = c->kf.delta;
    k.row = c->d_row; k.col = c->d_col; k.w = c->d_w;
    k.row_in = c->d_row_in; k.col_in = c->d_col_in; k.w_in = c->d_w_in;
    k.rix_in = c->kf.d_rix; k.rtab = c->kf.d_rtab; k.nrtab = c->kf.nrtab;
    k.hring = 0;
    if (const char* e = getenv("SHD_ROUTE_KFH_RING")) k.hring = std::max(0, atoi(e));  // (tests: a small ring)
    k.vf = c->d_vf; k.self_w = c->d_self_w; k.self_r = c->d_self_r; k.dbg = c->d_dbg;
    k.opk = c->kf.d_opk; k.ipk = c->kf.d_ipk; k.wscale = c->kf.wscale;
    return k;
}

// the rows of ns sources by KB: the fused kernel, or distances and parents for KB_SRC sources
// per workgroup -> key rows -> K2
int kb_launch(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, int64_t ld, double* d_lat,
              double* d_rel, double* d_row_min, hipStream_t st) {
    const DevKB kb = kb_args(c, ns);
    int gridb = std::min((ns + KB_SRC - 1) / KB_SRC, 1 << 20);
    if (c->kb.grid_cap > 0) gridb = std::min(gridb, c->kb.grid_cap);
    if (c->kb.fused) {
        hipLaunchKernelGGL(sssp_batch_rows_kernel, dim3(gridb), dim3(KB_BLOCK), c->kb.f_lds, st, kb, d_src, ns,
                           c->d_err, d_tgt, nt, (long long)ld, d_lat, d_rel, d_row_min);
        return hip_check(hipGetLastError());
    }
    const size_t need = (size_t)ns * c->n;
    if (need > c->keys_cap) {
        if (c->d_keys) (void)hipFree(c->d_keys);
        c->d_keys = nullptr;
        c->keys_cap = 0;
        if (hipMalloc((void**)&c->d_keys, need * sizeof(uint32_t)) != hipSuccess) return SHD_ROUTE_ENOMEM;
        c->keys_cap = need;
    }
    hipLaunchKernelGGL(sssp_batch_kernel, dim3(gridb), dim3(KB_BLOCK), c->kb.lds, st, kb, d_src, ns,
                       c->d_keys, (long long)c->n, c->d_err);
    int rc = hip_check(hipGetLastError());
    if (rc) return rc;
    const int grida = std::min(ns, 1 << 20);
    hipLaunchKernelGGL(path_attr_kernel<256>, dim3(grida), dim3(256), c->attr.lds, st, attr_args(c), c->d_keys,
                       (long long)c->n, d_src, ns, d_tgt, nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err);
    return hip_check(hipGetLastError());
}

int k32_launch(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, int64_t ld, double* d_lat,
               double* d_rel, double* d_row_min, hipStream_t st) {
    const DevK32 k = k32_args(c);
    const int grid = std::min(ns, 1 << 20);
    k32_dispatch(c->k32.block, [&](auto B) {
        constexpr int b = decltype(B)::value;
        hipLaunchKernelGGL(sssp_k32_kernel<b>, dim3(grid), dim3(b), c->k32.lds, st, k, d_src, ns, d_tgt, nt,
                           (long long)ld, d_lat, d_rel, d_row_min, c->d_err);
        return 0;
    });
    return hip_check(hipGetLastError());
}

int kf_launch(shd_route* c, const int32_t* d_src, int ns, const int32_t* d_tgt, int nt, int64_t ld, double* d_lat,
              double* d_rel, double* d_row_min, hipStream_t st) {
    const DevF64D k = kf_args(c);
    const int grid = std::min(ns, c->kf.slots);
    // (KFH's slices: one per workgroup slot, grid <= kf.slots)
    kf_dispatch(c->kf.block, c->kf.h, c->kf.d_opk != nullptr, [&](auto B, auto H, auto P) {
        constexpr int b = decltype(B)::value;
        constexpr bool h = decltype(H)::value;
        hipLaunchKernelGGL((sssp_f64d_kernel<b, h, decltype(P)::value>), dim3(grid), dim3(b), c->kf.lds, st, k, d_src,
                           ns, d_tgt, nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err, h ? c->d_kf_ws : (char*)nullptr,
                           h ? c->kf.ws_stride : (size_t)0);
        return 0;
    });
    return hip_check(hipGetLastError());
}

int take_err(shd_route* c) {
    int h = 0;
    if (hipMemcpy(&h, c->d_err, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (h) {
        int z = 0;
        if (hipMemcpy(c->d_err, &z, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return SHD_ROUTE_EDEVICE;
    }
    return h;
}

}  // namespace

extern "C" {

const char* shd_route_strerror(int code) {
    switch (code) {
        case SHD_ROUTE_OK: return "success";
        case SHD_ROUTE_EINVAL: return "invalid argument or topology failed validation";
        case SHD_ROUTE_ENOMEM: return "out of memory";
        case SHD_ROUTE_EDEVICE: return "HIP device error";
        case SHD_ROUTE_ENOEDGE: return "path hop without an edge (missing self-loop?)";
        case SHD_ROUTE_EUNREACH: return "target unreachable";
        case SHD_ROUTE_EUNSUPPORTED: return "unsupported request";
        default: return "unknown error";
    }
}

int shd_route_create(shd_route_t** out, const shd_graph_t* g, int device) {
    if (!out || !g) return SHD_ROUTE_EINVAL;
    *out = nullptr;
    const int n = g->n_vertices, m = g->n_edges;
    if (n <= 0 || m < 0 || (m > 0 && (!g->edge_src || !g->edge_dst || !g->edge_latency || !g->edge_packetloss)))
        return SHD_ROUTE_EINVAL;
    // validation as topology.c:1041-1124 (edges) and 811-978 (vertex packetloss)
    double arc_min = INFINITY, arc_max = 0.0;  // over the edges that are relaxed (no self-loops)
    for (int e = 0; e < m; e++) {
        int a = g->edge_src[e], b = g->edge_dst[e];
        double w = g->edge_latency[e], p = g->edge_packetloss[e];
        if (a < 0 || a >= n || b < 0 || b >= n) return SHD_ROUTE_EINVAL;
        if (!(w > 0.0) || std::isinf(w)) return SHD_ROUTE_EINVAL;
        if (!(p >= 0.0 && p <= 1.0)) return SHD_ROUTE_EINVAL;
        if (a != b) { arc_min = std::min(arc_min, w); arc_max = std::max(arc_max, w); }
    }
    if (g->vertex_packetloss)
        for (int v = 0; v < n; v++) {
            double p = g->vertex_packetloss[v];
            if (!std::isnan(p) && !(p >= 0.0 && p <= 1.0)) return SHD_ROUTE_EINVAL;
        }
    // No latency may be absorbed: every kernel and path call takes d[u] + w > d[u] for granted
    // (the tight arcs d[u] + w == d[v] form a DAG, a parent is strictly nearer than its child).
    // A distance is a left fold of at most n - 1 latencies, so no d exceeds (n - 1) max_w times
    // (1 + 2^-53)^n; ulp(d) <= d 2^-52, and fl(d + w) == d needs w <= ulp(d) / 2.  Refusing
    // min_w <= (n - 1) max_w 2^-52 therefore keeps a factor of two, which covers the rounding
    // growth of the fold.  (C4f: 50,000 vertices, latencies up to ~250 ms: refused below 3e-9 ms.)
    if (arc_max > 0.0 && arc_min <= (double)(n - 1) * (arc_max * 0x1p-52)) return SHD_ROUTE_EUNSUPPORTED;
    if (hipSetDevice(device) != hipSuccess) return SHD_ROUTE_EDEVICE;

    shd_route* c = new (std::nothrow) shd_route();
    if (!c) return SHD_ROUTE_ENOMEM;
    c->device = device; c->n = n; c->m = m;
    c->directed = g->directed ? 1 : 0;
    c->prefer_direct = g->prefer_direct ? 1 : 0;
    c->e_src.assign(g->edge_src, g->edge_src + m);
    c->e_dst.assign(g->edge_dst, g->edge_dst + m);
    c->e_lat.assign(g->edge_latency, g->edge_latency + m);
    c->e_loss.assign(g->edge_packetloss, g->edge_packetloss + m);
    c->v_loss.assign(n, NAN);
    if (g->vertex_packetloss) c->v_loss.assign(g->vertex_packetloss, g->vertex_packetloss + n);
    HostGraph h = HostGraph::make(g);
    c->nnz = h.nnz; c->integer_w = h.integer_w; c->multigraph = h.multigraph; c->self16 = h.self16;
    c->min_w = h.min_w; c->max_w = h.max_w;

    // topology.c:738-806: strongly connected, one cluster
    if (!strongly_connected(n, h.row, h.col, h.in_row(), h.in_col())) {
        delete c;
        return SHD_ROUTE_EINVAL;
    }
    // topology.c:450-552 isComplete: OUT-incident count (undirected: loops twice, minus one)
    c->complete = 1;
    for (int v = 0; v < n; v++) {
        long long ecount;
        if (c->directed) ecount = (h.row[v + 1] - h.row[v]) + h.loops[v];
        else ecount = (h.row[v + 1] - h.row[v]) + 2LL * h.loops[v] - (h.loops[v] > 0 ? 1 : 0);
        if (ecount < n) { c->complete = 0; break; }
    }

    std::vector<double> vf(n, NAN);
    if (g->vertex_packetloss)
        for (int v = 0; v < n; v++)
            if (!std::isnan(g->vertex_packetloss[v])) {
                vf[v] = (1.0f - g->vertex_packetloss[v]);
                c->has_vf = 1;
                if (vf[v] != 1.0) c->vf_lossy = 1;
            }

    int rc = SHD_ROUTE_OK;
    if (!rc) rc = upload(c, &c->d_row, h.row);
    if (!rc) rc = upload(c, &c->d_col, h.col);
    if (!rc) rc = upload(c, &c->d_w, h.w);
    if (!rc) rc = upload(c, &c->d_r, h.r);
    if (c->directed) {
        if (!rc) rc = upload(c, &c->d_row_in, h.row_in);
        if (!rc) rc = upload(c, &c->d_col_in, h.col_in);
        if (!rc) rc = upload(c, &c->d_w_in, h.w_in);
        if (!rc) rc = upload(c, &c->d_r_in, h.r_in);
    } else {
        c->d_row_in = c->d_row; c->d_col_in = c->d_col; c->d_w_in = c->d_w; c->d_r_in = c->d_r;
    }
    if (!rc) rc = upload(c, &c->d_vf, vf);
    if (!rc) rc = upload(c, &c->d_self_w, h.self_w);
    if (!rc) rc = upload(c, &c->d_self_r, h.self_r);
    if (!rc) {
        std::vector<int> z(1, 0);
        rc = upload(c, &c->d_err, z);
    }
    StateLayout L = StateLayout::make(n);
    c->lds_bytes = kSmallBytes + L.total;
    c->lds = c->lds_bytes <= kLdsBudget;
    if (!rc) {
        if (c->lds) {
            rc = hip_check(hipFuncSetAttribute((const void*)sssp_rows_kernel<true>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_bytes));
        } else {
            rc = alloc_ws(c);
        }
    }
    if (!rc) rc = apply_selection(c, select_all(SelectInput(h), SelectKnobs::from_env()));
    if (rc) {
        shd_route_destroy(c);
        return rc;
    }
    c->e_rel = std::move(h.e_rel);
    if (c->kd.ok) {  // the planner's host copies
        c->h_row = std::move(h.row); c->h_col = std::move(h.col); c->h_w = std::move(h.w);
    }
    if (c->sel == 4 && c->kd.fused) host_pool();  // the planner's workers, parked until a plan
    *out = c;
    return SHD_ROUTE_OK;
}

void shd_route_destroy(shd_route_t* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->d_keys) (void)hipFree(c->d_keys);
    if (c->d_fwkey) (void)hipFree(c->d_fwkey);
    if (c->d_lm_drow) (void)hipFree(c->d_lm_drow);
    if (c->d_lm_prow) (void)hipFree(c->d_lm_prow);
    if (c->d_hub_ws) (void)hipFree(c->d_hub_ws);
    path_free(c->path);
    for (void* p : c->allocs) (void)hipFree(p);
    delete c;
}

// u16 latency payloads are exact: integer latencies whose shortest paths are proven below
// 0xFFFF and integer self-loops (the diagonal, kept out of the CSR and its bound) below it
static bool lat16_ok(const shd_route* c) {
    return c->integer_w && c->self16 && c->k32.bound > 0 && c->k32.bound < 0xFFFF;
}

int shd_route_get_info(const shd_route_t* c, shd_route_info_t* info) {
    if (!c || !info) return SHD_ROUTE_EINVAL;
    info->n_vertices = c->n;
    info->n_edges = c->m;
    info->n_arcs = c->nnz;
    info->is_complete = c->complete;
    info->directed = c->directed;
    info->prefer_direct = c->prefer_direct;
    info->integer_weights = c->integer_w;
    info->multigraph = c->multigraph;
    info->device = c->device;
    info->lds_resident = ((c->lds || c->sel) && !c->kf.h) ? 1 : 0;  // (KFH: vertex state in HBM)
    info->kernel = c->sel;
    info->dist_bound = c->k32.bound;
    info->block = c->sel == 2 ? KB_BLOCK : c->sel == 3 ? 1024 : c->sel == 4 ? c->kd.block
                : c->sel == 1 ? c->k32.block : c->sel == 5 ? c->kf.block : kBlock;
    info->reserved = c->sel == 4 ? c->kd.delta : c->sel == 2 ? c->kb.fused : c->sel == 5 ? (int)c->kf.wscale : 0;
    info->lat16 = lat16_ok(c) ? 1 : 0;
    info->device_bytes = c->device_bytes;
    info->min_edge_latency = c->min_w;
    return SHD_ROUTE_OK;
}

int shd_route_rows_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt,
                         int32_t nt, int64_t ld, uint32_t flags, double* d_lat, double* d_rel,
                         double* d_row_min, void* stream) {
    if (!c || ns < 0 || nt < 0 || (ns && !d_src) || (nt && !d_tgt) || ld < nt) return SHD_ROUTE_EINVAL;
    if (ns == 0) return SHD_ROUTE_OK;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((flags & SHD_ROUTE_DISPATCH) && c->complete) {
        int rc = ensure_dense(c);
        if (rc) return rc;
        int grid = std::min(ns, 65535);
        hipLaunchKernelGGL(direct_rows_kernel, dim3(grid), dim3(kBlock), 0, st, c->n, c->d_W, c->d_R,
                           c->d_vf, d_src, ns, d_tgt, nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err);
        return hip_check(hipGetLastError());
    }
    const int dispatch = (flags & SHD_ROUTE_DISPATCH) ? 1 : 0;
    if (c->sel && !(dispatch && c->prefer_direct)) {
        switch (c->sel) {
            case 2: return kb_launch(c, d_src, ns, d_tgt, nt, ld, d_lat, d_rel, d_row_min, st);
            case 4:
                if (hipMemsetAsync(c->d_kd_next, 0, sizeof(int), st) != hipSuccess) return SHD_ROUTE_EDEVICE;
                return kd_launch(c, kd_args(c), c->d_kd_next, d_src, ns, d_tgt, nt, ld, d_lat, d_rel, d_row_min, st);
            case 1: return k32_launch(c, d_src, ns, d_tgt, nt, ld, d_lat, d_rel, d_row_min, st);
            case 5: return kf_launch(c, d_src, ns, d_tgt, nt, ld, d_lat, d_rel, d_row_min, st);
        }
    }
    DevGraph g = dev_graph(c);
    if (c->lds) {
        int grid = std::min(ns, 1 << 20);
        hipLaunchKernelGGL(sssp_rows_kernel<true>, dim3(grid), dim3(kBlock), c->lds_bytes, st, g, d_src, ns,
                           d_tgt, nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err, nullptr, (size_t)0,
                           dispatch);
    } else {
        int grid = std::min(ns, c->ws_slots);
        hipLaunchKernelGGL(sssp_rows_kernel<false>, dim3(grid), dim3(kBlock), kSmallBytes, st, g, d_src, ns,
                           d_tgt, nt, (long long)ld, d_lat, d_rel, d_row_min, c->d_err, c->d_ws, c->ws_stride,
                           dispatch);
    }
    return hip_check(hipGetLastError());
}

int shd_route_sync(shd_route_t* c, void* stream) {
    if (!c) return SHD_ROUTE_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return SHD_ROUTE_EDEVICE;
    return take_err(c);
}

}  // extern "C"

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t b) { return hipMalloc(&p, b ? b : 1) == hipSuccess ? SHD_ROUTE_OK : SHD_ROUTE_ENOMEM; }
};
}  // namespace

// hops, link loads and the tie envelope: shd_route_hops*, _paths, _loads*, _pair_loads, _ties*
// (and the stages every blocking call shares, host_rows below among them: SoftCode, host_chunk)
#include "path_calls.hpp"

namespace {

// Host-pointer wrapper: chunks rows so device output stays bounded, copies back.
template <typename Launch>
int host_rows(shd_route* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt, double* lat_out,
              double* rel_out, double* row_min_out, Launch launch) {
    if (!c || ns < 0 || nt < 0 || (ns && !src) || (nt && !tgt)) return SHD_ROUTE_EINVAL;
    if (ns == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t row_bytes = sizeof(double) * (size_t)std::max(nt, 1);
    const int32_t chunk = host_chunk(ns, row_bytes);
    DevBuf dsrc, dtgt, dlat, drel, dmin;
    int rc;
    if ((rc = dsrc.alloc(sizeof(int32_t) * chunk)) || (rc = dtgt.alloc(sizeof(int32_t) * std::max(nt, 1))) ||
        (rc = dlat.alloc(row_bytes * chunk)) || (rc = drel.alloc(row_bytes * chunk)) ||
        (rc = dmin.alloc(sizeof(double) * chunk)))
        return rc;
    if (nt && hipMemcpy(dtgt.p, tgt, sizeof(int32_t) * nt, hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    SoftCode sc;
    for (int32_t i0 = 0; i0 < ns; i0 += chunk) {
        int32_t k = std::min(chunk, ns - i0);
        if (hipMemcpy(dsrc.p, src + i0, sizeof(int32_t) * k, hipMemcpyHostToDevice) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        rc = launch((const int32_t*)dsrc.p, k, (const int32_t*)dtgt.p, (double*)dlat.p, (double*)drel.p,
                    (double*)dmin.p);
        if (rc) return rc;
        // per-entry failures (missing self-loop, unreachable target) leave NaN in those
        // entries only: the rows are still copied out and the code returned at the end
        if ((rc = sc.sync(c))) return rc;
        if (lat_out && hipMemcpy(lat_out + (size_t)i0 * nt, dlat.p, row_bytes * k, hipMemcpyDeviceToHost) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        if (rel_out && hipMemcpy(rel_out + (size_t)i0 * nt, drel.p, row_bytes * k, hipMemcpyDeviceToHost) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
        if (row_min_out && hipMemcpy(row_min_out + i0, dmin.p, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
    }
    return sc.soft;
}
}  // namespace

// the seeded-row planner: its kernels, struct shd_route_plan, shd_route_plan_* and planned_host_rows
#include "plan.hpp"

extern "C" {

int shd_route_rows(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                   uint32_t flags, double* lat_out, double* rel_out, double* row_min_out) {
    // many KD rows (at least one per resident workgroup slot, so the plan's landmark rows,
    // row store and table pay off): one seeded plan over all of them when the whole table
    // fits the device; small batches and any device allocation failure take the chunked rows
    if (c && c->sel == 4 && c->kd.fused && ns >= 2 && ns >= c->kd.slots && nt >= 1 && src && tgt &&
        !((flags & SHD_ROUTE_DISPATCH) && (c->complete || c->prefer_direct))) {
        const int rc = planned_host_rows(c, src, ns, tgt, nt, flags, lat_out, rel_out, row_min_out);
        if (rc != SHD_ROUTE_EUNSUPPORTED) return rc;
    }
    return host_rows(c, src, ns, tgt, nt, lat_out, rel_out, row_min_out,
                     [&](const int32_t* ds, int32_t k, const int32_t* dt, double* dl, double* dr, double* dm) {
                         return shd_route_rows_async(c, ds, k, dt, nt, nt, flags, dl, dr, dm, nullptr);
                     });
}

int shd_route_direct(shd_route_t* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                     double* lat_out, double* rel_out, double* row_min_out) {
    if (!c) return SHD_ROUTE_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    int rc = ensure_dense(c);
    if (rc) return rc;
    return host_rows(c, src, ns, tgt, nt, lat_out, rel_out, row_min_out,
                     [&](const int32_t* ds, int32_t k, const int32_t* dt, double* dl, double* dr, double* dm) {
                         int grid = std::min(k, 65535);
                         hipLaunchKernelGGL(direct_rows_kernel, dim3(grid), dim3(kBlock), 0, nullptr, c->n, c->d_W,
                                            c->d_R, c->d_vf, ds, k, dt, nt, (long long)nt, dl, dr, dm, c->d_err);
                         return hip_check(hipGetLastError());
                     });
}

int shd_route_self(shd_route_t* c, const int32_t* v, int32_t nv, double* lat_out, double* rel_out) {
    if (!c || nv < 0 || (nv && (!v || !lat_out || !rel_out))) return SHD_ROUTE_EINVAL;
    if (nv == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    DevBuf dv, dl, dr;
    int rc;
    if ((rc = dv.alloc(sizeof(int32_t) * nv)) || (rc = dl.alloc(sizeof(double) * nv)) ||
        (rc = dr.alloc(sizeof(double) * nv)))
        return rc;
    if (hipMemcpy(dv.p, v, sizeof(int32_t) * nv, hipMemcpyHostToDevice) != hipSuccess) return SHD_ROUTE_EDEVICE;
    DevGraph g = dev_graph(c);
    hipLaunchKernelGGL(self_kernel, dim3((nv + 255) / 256), dim3(256), 0, nullptr, g, (const int*)dv.p, nv,
                       (double*)dl.p, (double*)dr.p, c->d_err);
    if ((rc = hip_check(hipGetLastError()))) return rc;
    if ((rc = shd_route_sync(c, nullptr))) return rc;
    if (hipMemcpy(lat_out, dl.p, sizeof(double) * nv, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rel_out, dr.p, sizeof(double) * nv, hipMemcpyDeviceToHost) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

int shd_route_min_reduce_async(shd_route_t* c, const double* d_vals, int64_t count, double* d_out, void* stream) {
    if (!c || count < 0 || !d_out || (count && !d_vals)) return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (count <= kMinOneBlock) {  // one launch, no clearing memset
        hipLaunchKernelGGL(min_reduce_block_kernel, dim3(1), dim3(1024), 0, st, d_vals, (long long)count,
                           (unsigned long long*)d_out);
        return hip_check(hipGetLastError());
    }
    if (hipMemsetAsync(d_out, 0xFF, sizeof(double), st) != hipSuccess) return SHD_ROUTE_EDEVICE;
    long long blocks = std::min<long long>((count + kBlock - 1) / kBlock, 2048);
    hipLaunchKernelGGL(min_reduce_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_vals, (long long)count,
                       (unsigned long long*)d_out);
    return hip_check(hipGetLastError());
}

int shd_route_fw_async(shd_route_t* c, double* d_dist, void* stream) {
    if (!c || !d_dist) return SHD_ROUTE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const int n = c->n;
    const int nb = (n + kT - 1) / kT;
    for (int kb = 0; kb < nb; kb++) {
        const int k0 = kb * kT;
        hipLaunchKernelGGL(fw_diag_kernel, dim3(1), dim3(kT * 8), 0, st, d_dist, n, k0);
        if (nb > 1)
            hipLaunchKernelGGL(fw_panel_kernel, dim3(nb - 1, 2), dim3(kT * 8), 0, st, d_dist, n, k0);
        hipLaunchKernelGGL(fw_rest_kernel, dim3(nb, nb), dim3(kT * 8), 0, st, d_dist, n, k0);
    }
    return hip_check(hipGetLastError());
}

}  // extern "C"

// =============================================================================
// K4: blocked min-plus Floyd-Warshall (fw.hpp)
// =============================================================================
namespace {
constexpr int kFwMaxN = 12000;  // fw_rows keeps rel f64 + order u16 per vertex in LDS

// Builds the K4 state once per context: eligibility first (nothing is allocated for an
// ineligible graph, so every call answers EUNSUPPORTED), then the buffers into locals,
// published in the context only when every step has succeeded; the in-list build is
// enqueued on the caller's stream, ahead of the table launches that follow it there.
// K4 takes the graph: integer latencies below the u16 bound, no parallel edges, the rows' and the
// in-list build's LDS state within the budget
bool fw_eligible(const shd_route* c) {
    if (!c->integer_w || c->multigraph || c->n > kFwMaxN || c->k32.bound <= 0 || c->k32.bound >= 0xFFFF)
        return false;
    const size_t lds = a16(sizeof(double) * c->n) + a16(sizeof(uint16_t) * c->n) + a16(sizeof(int) * (c->k32.bound + 2));
    if (lds > kLdsBudget) return false;
    const int np = (c->n + FW_T - 1) / FW_T * FW_T;
    int sp = 1;
    while (sp < np) sp <<= 1;
    return (size_t)4 * sp <= kLdsBudget;
}

int fw_prepare(shd_route* c, hipStream_t st) {
    if (c->d_fwD) return SHD_ROUTE_OK;
    if (!fw_eligible(c)) return SHD_ROUTE_EUNSUPPORTED;
    const size_t lds = a16(sizeof(double) * c->n) + a16(sizeof(uint16_t) * c->n) + a16(sizeof(int) * (c->k32.bound + 2));
    const int np = (c->n + FW_T - 1) / FW_T * FW_T;
    int sp = 1;
    while (sp < np) sp <<= 1;
    int rc = ensure_dense(c);
    if (rc) return rc;
    if ((rc = hip_check(hipFuncSetAttribute((const void*)fw_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds))) ||
        (rc = hip_check(hipFuncSetAttribute((const void*)fw_inlist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(4 * sp)))) ||
        (rc = hip_check(hipFuncSetAttribute((const void*)fw_parent_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(2 * np)))) ||
        (rc = hip_check(hipFuncSetAttribute((const void*)fw_parent_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)(2 * np)))) ||
        ((size_t)16 * np <= kLdsBudget &&
         ((rc = hip_check(hipFuncSetAttribute((const void*)fw_parent8_kernel<true>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 * np)))) ||
          (rc = hip_check(hipFuncSetAttribute((const void*)fw_parent8_kernel<false>,
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 * np)))))))
        return rc;
    const size_t cells = (size_t)np * np;
    uint16_t* D = nullptr;
    uint32_t* inl = nullptr;
    uint16_t* pos = nullptr;
    auto undo = [&](int code) {
        if (D) (void)hipFree(D);
        if (inl) (void)hipFree(inl);
        if (pos) (void)hipFree(pos);
        return code;
    };
    if (hipMalloc((void**)&D, 2 * cells) != hipSuccess || hipMalloc((void**)&inl, 4 * cells) != hipSuccess ||
        hipMalloc((void**)&pos, sizeof(uint16_t) * FW_X * (size_t)c->n) != hipSuccess)
        return undo(SHD_ROUTE_ENOMEM);
    // reliability indices (round 5): every distinct 1 - loss (exact bits), at most 255 of them
    // (C5: 101), as a dense u8 matrix: fw_rows reads a parent arc's index and multiplies the
    // table entry in LDS
    std::vector<uint64_t> rbits;
    for (int e = 0; e < c->m; e++) { uint64_t b; std::memcpy(&b, &c->e_rel[e], 8); rbits.push_back(b); }
    std::sort(rbits.begin(), rbits.end());
    rbits.erase(std::unique(rbits.begin(), rbits.end()), rbits.end());
    uint8_t* rixd = nullptr;
    double* rtd = nullptr;
    int nrt = 0;
    if (rbits.size() <= 255 && !getenv("SHD_ROUTE_FWDENSER")) {
        std::vector<double> rt(rbits.size());
        for (size_t q = 0; q < rbits.size(); q++) std::memcpy(&rt[q], &rbits[q], 8);
        std::vector<uint8_t> rix((size_t)c->n * c->n, 0xFF);
        auto idx = [&](double r) {
            uint64_t b; std::memcpy(&b, &r, 8);
            return (uint8_t)(std::lower_bound(rbits.begin(), rbits.end(), b) - rbits.begin());
        };
        // (the same edge ensure_dense keeps: the lowest edge id of a pair)
        for (int e = c->m - 1; e >= 0; e--) {
            const int a = c->e_src[e], b = c->e_dst[e];
            rix[(size_t)a * c->n + b] = idx(c->e_rel[e]);
            if (!c->directed) rix[(size_t)b * c->n + a] = idx(c->e_rel[e]);
        }
        if (hipMalloc((void**)&rixd, rix.size()) != hipSuccess ||
            hipMalloc((void**)&rtd, sizeof(double) * 256) != hipSuccess ||
            hipMemcpy(rixd, rix.data(), rix.size(), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(rtd, rt.data(), sizeof(double) * rt.size(), hipMemcpyHostToDevice) != hipSuccess) {
            for (void* q : {(void*)rixd, (void*)rtd}) if (q) (void)hipFree(q);
            return undo(SHD_ROUTE_ENOMEM);
        }
        nrt = (int)rt.size();
    }
    // packed in-list keys (the parent arc's reliability index inside the key): every latency
    // <= 255 and the u8 index matrix built above (SHD_ROUTE_FWPK=0: the wide keys)
    const int pk = rixd && c->max_w <= 255.0 && !(getenv("SHD_ROUTE_FWPK") && atoi(getenv("SHD_ROUTE_FWPK")) == 0);
    hipLaunchKernelGGL(fw_inlist_kernel, dim3(c->n), dim3(1024), 4 * sp, st, c->d_W, c->n, np, sp, inl, pos, rixd, pk);
    if ((rc = hip_check(hipGetLastError()))) {
        for (void* q : {(void*)rixd, (void*)rtd}) if (q) (void)hipFree(q);
        return undo(rc);
    }
    // (published only now: a failed step above leaves the context as it was, and a retry
    // builds every table again)
    if (rixd) {
        c->d_fwrix = rixd;
        c->d_fwrtab = rtd;
        c->allocs.push_back(c->d_fwrix);
        c->allocs.push_back(c->d_fwrtab);
        c->fw_nrtab = nrt;
    }
    c->d_fwD = D;
    c->fw_pk = pk;
    c->d_fwinl = inl;
    c->d_fwpos = pos;
    c->allocs.push_back(D);
    c->allocs.push_back(inl);
    c->allocs.push_back(pos);
    c->fw_np = np;
    return SHD_ROUTE_OK;
}
}  // namespace

extern "C" {

int shd_route_fw_table_async(shd_route_t* c, void* stream) {
    if (!c) return SHD_ROUTE_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    int rc = fw_prepare(c, st);
    if (rc) return rc;
    const int np = c->fw_np, nb = np / FW_T;
    const unsigned blocks = (unsigned)(((size_t)np * np + 255) / 256);
    hipLaunchKernelGGL(fw_init_kernel, dim3(blocks), dim3(256), 0, st, c->d_W, c->n, np, c->d_fwD);
    // rest kernel: 64 x 64 tiles with 4 x 4 register blocks and the next pivot's panels fused in
    // (default: one launch per pivot); SHD_ROUTE_FWREST=1 the separate panel + rest launches,
    // 2 the 128 x 128-region rest kernel with 8 x 8 blocks (C5 FW table 3.28 ms against 3.06)
    const char* fwr = getenv("SHD_ROUTE_FWREST");
    const int mode = fwr ? atoi(fwr) : 3;
    if ((mode == 0 || mode == 3) && nb > 1) {
        if (!c->d_fwflag) {
            if (hipMalloc((void**)&c->d_fwflag, sizeof(int) * (size_t)(nb + 1)) != hipSuccess) return SHD_ROUTE_ENOMEM;
            c->allocs.push_back(c->d_fwflag);
        }
        if (hipMemsetAsync(c->d_fwflag, 0, sizeof(int) * (size_t)(nb + 1), st) != hipSuccess) return SHD_ROUTE_EDEVICE;
        hipLaunchKernelGGL(fw_diag_kernel<FW_T>, dim3(1), dim3(256), 0, st, c->d_fwD, np, 0);
        hipLaunchKernelGGL(fw_panel_kernel<FW_T>, dim3(nb - 1, 2), dim3(256), 0, st, c->d_fwD, np, 0);
        int P = 1024;  // mode 3: persistent plain-tile workgroups
        if (const char* e = getenv("SHD_ROUTE_FWP")) P = std::max(1, atoi(e));
        for (int kb = 0; kb < nb; kb++) {
            const int nx = kb + 1 < nb ? 2 : 0;  // the next pivot's panel tiles in row / column kb
            if (mode == 0) {
                hipLaunchKernelGGL(fw_restp_kernel<FW_T>, dim3((nb - 1) * (nb - 1) + nx), dim3(256), 0, st, c->d_fwD, np,
                                   kb, c->d_fwflag, c->d_err);
            } else {
                const int m = kb + 1 < nb ? nb - 2 : nb - 1, pp = std::max(1, std::min(P, m * m));
                const int grid = kb + 1 < nb ? 1 + pp + 2 * m + 2 : pp;
                hipLaunchKernelGGL(fw_restpp_kernel<FW_T>, dim3(grid), dim3(256), 0, st, c->d_fwD, np, kb, c->d_fwflag, pp, c->d_err);
            }
        }
        c->fw_ready = 1;
        return hip_check(hipGetLastError());
    }
    const bool rest1 = mode != 2;
    const int nr = (nb + 1) / 2;
    for (int kb = 0; kb < nb; kb++) {
        // pivot tiles after the first are closed inside the previous fw_rest launch
        if (kb == 0) hipLaunchKernelGGL(fw_diag_kernel<FW_T>, dim3(1), dim3(256), 0, st, c->d_fwD, np, kb);
        if (nb > 1) {
            hipLaunchKernelGGL(fw_panel_kernel<FW_T>, dim3(nb - 1, 2), dim3(256), 0, st, c->d_fwD, np, kb);
            if (rest1)
                hipLaunchKernelGGL(fw_rest_kernel<FW_T>, dim3(nb - 1, nb - 1), dim3(256), 0, st, c->d_fwD, np, kb);
            else
                hipLaunchKernelGGL(fw_rest2_kernel, dim3(nr * nr), dim3(256), 0, st, c->d_fwD, np, kb);
        }
    }
    c->fw_ready = 1;
    return hip_check(hipGetLastError());
}

int shd_route_fw_rows_async(shd_route_t* c, const int32_t* d_src, int32_t ns, const int32_t* d_tgt, int32_t nt,
                            int64_t ld, double* d_lat, double* d_rel, double* d_row_min, void* stream) {
    if (!c || ns < 0 || nt < 0 || (ns && !d_src) || (nt && !d_tgt) || ld < nt) return SHD_ROUTE_EINVAL;
    // (no table: a graph K4 never takes is unsupported; else shd_route_fw_table_async first)
    if (!c->fw_ready) return fw_eligible(c) ? SHD_ROUTE_EINVAL : SHD_ROUTE_EUNSUPPORTED;
    if (ns == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    const int np = c->fw_np;
    const size_t need = (size_t)ns * np;
    if (need > c->fwkey_cap) {
        if (c->d_fwkey) (void)hipFree(c->d_fwkey);
        c->d_fwkey = nullptr;
        c->fwkey_cap = 0;
        if (hipMalloc((void**)&c->d_fwkey, need * sizeof(uint32_t)) != hipSuccess) return SHD_ROUTE_ENOMEM;
        c->fwkey_cap = need;
    }
    // (256-thread workgroups: at fw_parent's 70 VGPRs a CU holds seven of them, against one of
    // 1024 threads: C5 rows 1.02 -> 0.94 ms; SHD_ROUTE_FWPBLK=512 / 1024 for the A/B)
    int pblk = 256;
    if (const char* e = getenv("SHD_ROUTE_FWPBLK")) pblk = atoi(e) == 1024 ? 1024 : atoi(e) == 512 ? 512 : 256;
    // eight sources per workgroup where their interleaved rows fit the LDS (C5 rows 0.62 ->
    // 0.41 ms at 1024 threads, 0.44 at 512, 0.50 at 256; SHD_ROUTE_FWP8=0: one source per
    // workgroup, SHD_ROUTE_FWP8BLK=512 / 256 for the A/B)
    const bool p8 = (size_t)16 * np <= kLdsBudget && !(getenv("SHD_ROUTE_FWP8") && atoi(getenv("SHD_ROUTE_FWP8")) == 0);
    int p8blk = 1024;
    if (const char* e = getenv("SHD_ROUTE_FWP8BLK")) p8blk = atoi(e) == 512 ? 512 : atoi(e) == 256 ? 256 : 1024;
    if (p8 && c->fw_pk)
        hipLaunchKernelGGL(fw_parent8_kernel<true>, dim3(std::min((ns + 7) / 8, 2048)), dim3(p8blk), 16 * np, st, c->d_fwD,
                           c->d_fwinl, c->d_fwpos, c->n, np, d_src, ns, c->d_fwkey);
    else if (p8)
        hipLaunchKernelGGL(fw_parent8_kernel<false>, dim3(std::min((ns + 7) / 8, 2048)), dim3(p8blk), 16 * np, st, c->d_fwD,
                           c->d_fwinl, c->d_fwpos, c->n, np, d_src, ns, c->d_fwkey);
    else if (c->fw_pk)
        hipLaunchKernelGGL(fw_parent_kernel<true>, dim3(std::min(ns, 8192)), dim3(pblk), 2 * np, st, c->d_fwD, c->d_fwinl,
                           c->d_fwpos, c->n, np, d_src, ns, c->d_fwkey);
    else
        hipLaunchKernelGGL(fw_parent_kernel<false>, dim3(std::min(ns, 8192)), dim3(pblk), 2 * np, st, c->d_fwD, c->d_fwinl,
                           c->d_fwpos, c->n, np, d_src, ns, c->d_fwkey);
    FWRowsArgs a;
    a.pk = c->fw_pk;
    a.n = c->n; a.np = np; a.bound = c->k32.bound; a.D = c->d_fwD; a.key = c->d_fwkey; a.R = c->d_R;
    a.rix = c->d_fwrix; a.rtab = c->d_fwrtab; a.nrtab = c->d_fwrix ? c->fw_nrtab : 0;
    a.vf = c->d_vf; a.self_w = c->d_self_w; a.self_r = c->d_self_r;
    const size_t lds = a16(sizeof(double) * c->n) + a16(sizeof(uint16_t) * c->n) + a16(sizeof(int) * (c->k32.bound + 2));
    // (512-thread workgroups since the u16 order list: C5 rows 0.92 -> 0.81 ms against 1024,
    // 0.86 at 256; SHD_ROUTE_FWRBLK=1024 / 256 for the A/B)
    int rblk = 512;
    if (const char* e = getenv("SHD_ROUTE_FWRBLK")) rblk = atoi(e) == 1024 ? 1024 : atoi(e) == 256 ? 256 : 512;
    hipLaunchKernelGGL(fw_rows_kernel, dim3(std::min(ns, 2048)), dim3(rblk), lds, st, a, d_src, ns, d_tgt, nt,
                       (long long)ld, d_lat, d_rel, d_row_min, c->d_err);
    return hip_check(hipGetLastError());
}

}  // extern "C"

// =============================================================================
// Eager fill of the front end's dense upper-triangle Path cache
// =============================================================================
namespace {
// pack rows [r0, r1) of the planned table into the triangle layout: row r (source A[i],
// i = pos[r]) keeps targets j >= i, as interleaved (lat, rel) pairs; one workgroup per
// row; row minima over the kept entries (NaN skipped) into *mn (u64 bits)
__global__ __launch_bounds__(256) void tri_pack_kernel(const double* __restrict__ lat, const double* __restrict__ rel,
                                                       long long ld, const int* __restrict__ pos,
                                                       const long long* __restrict__ off, int r0, int r1, int na,
                                                       double* __restrict__ out, unsigned long long* __restrict__ mn) {
    for (int r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
        const int i = pos[r];
        const double* lr = lat + (long long)r * ld;
        const double* rr = rel + (long long)r * ld;
        double* o = out + 2 * (off[r] - off[r0]);
        double m = INFINITY;
        for (int j = i + threadIdx.x; j < na; j += 256) {
            const double L = lr[j];
            o[2 * (j - i)] = L;
            o[2 * (j - i) + 1] = rr[j];
            if (!isnan(L)) m = fmin(m, L);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = fmin(m, __shfl_xor(m, d, 64));
        if ((threadIdx.x & 63) == 0 && m < INFINITY) atomicMin(mn, as_u(m));
    }
}

// the same into the compact SHD_ROUTE_FILL_LAT16 layout: row r's pairs six to a 64-byte line
// (rel f64 x 6, lat u16 x 6 with NaN -> 0xFFFF, 4 pad bytes) from line loff[r] - loff[r0]
__global__ __launch_bounds__(256) void tri_pack16_kernel(const double* __restrict__ lat, const double* __restrict__ rel,
                                                         long long ld, const int* __restrict__ pos,
                                                         const long long* __restrict__ loff, int r0, int r1, int na,
                                                         uint4* __restrict__ out, unsigned long long* __restrict__ mn) {
    for (int r = r0 + blockIdx.x; r < r1; r += gridDim.x) {
        const int i = pos[r];
        const double* lr = lat + (long long)r * ld;
        const double* rr = rel + (long long)r * ld;
        uint4* o = out + 4 * (loff[r] - loff[r0]);
        const int nl = (na - i + 5) / 6;
        double m = INFINITY;
        for (int l = threadIdx.x; l < nl; l += 256) {
            double R[6];
            uint32_t L16[3] = {0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 6; e++) {
                const int j = i + 6 * l + e;
                const double L = j < na ? lr[j] : NAN;
                R[e] = j < na ? rr[j] : 0.0;
                if (!isnan(L)) m = fmin(m, L);
                const uint32_t x = isnan(L) ? 0xFFFFu : (uint32_t)L;
                L16[e >> 1] |= x << (16 * (e & 1));
            }
            uint4* q = o + 4 * (long long)l;
            q[0] = make_uint4((uint32_t)as_u(R[0]), (uint32_t)(as_u(R[0]) >> 32), (uint32_t)as_u(R[1]), (uint32_t)(as_u(R[1]) >> 32));
            q[1] = make_uint4((uint32_t)as_u(R[2]), (uint32_t)(as_u(R[2]) >> 32), (uint32_t)as_u(R[3]), (uint32_t)(as_u(R[3]) >> 32));
            q[2] = make_uint4((uint32_t)as_u(R[4]), (uint32_t)(as_u(R[4]) >> 32), (uint32_t)as_u(R[5]), (uint32_t)(as_u(R[5]) >> 32));
            q[3] = make_uint4(L16[0], L16[1], L16[2], 0u);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = fmin(m, __shfl_xor(m, d, 64));
        if ((threadIdx.x & 63) == 0 && m < INFINITY) atomicMin(mn, as_u(m));
    }
}

// multi-GPU table assembly payload: row r (caller position pos[r] in the attached list)
// keeps its upper-triangle targets j >= pos[r]; lat goes out as u16 (integer latencies
// below 65535, NaN -> 0xFFFF) or f64, rel as f64, each into its own packed array at
// element offset off[r] - off[0]
template <bool L16>
__global__ __launch_bounds__(256) void tri_payload_kernel(const double* __restrict__ lat, const double* __restrict__ rel,
                                                          long long ld, const int* __restrict__ pos,
                                                          const long long* __restrict__ off, int nrows, int na,
                                                          void* __restrict__ out_lat, double* __restrict__ out_rel) {
    const long long base = off[0];
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int i = pos[r];
        const double* lr = lat + (long long)r * ld;
        const double* rr = rel + (long long)r * ld;
        const long long o = off[r] - base;
        for (int j = i + threadIdx.x; j < na; j += 256) {
            const double L = __builtin_nontemporal_load(lr + j);
            if (L16) {
                const uint16_t x = isnan(L) ? (uint16_t)0xFFFFu : (uint16_t)L;
                static_cast<uint16_t*>(out_lat)[o + (j - i)] = x;
            } else {
                static_cast<double*>(out_lat)[o + (j - i)] = L;
            }
            out_rel[o + (j - i)] = __builtin_nontemporal_load(rr + j);
        }
    }
}
}  // namespace

// Pinned host memory for the fill's triangle (C4: 13.3 GB compact, 20 GB interleaved).
// hipHostMalloc faults and pins 4 KiB pages one by one (3.4 s for 20 GiB on the box);
// anonymous memory advised as transparent huge pages, populated by several threads and
// registered takes ~0.15 s for the same D2H rate (tools/micro/pin_bench.cpp).  It is
// first-touched and registered in 256 MiB chunks by worker threads, lowest chunk first, so
// that the fill's copies (shd_route_fill_triangle waits for each chunk it copies into)
// overlap the pinning of the chunks after them instead of waiting for the whole triangle.
// On the box (tools/micro/pin_overlap.cpp, 8 GiB): 16-thread first-touch 136 GB/s against
// 30 GB/s for MADV_POPULATE_WRITE, registering touched pages 0.5 GB/ms, and a D2H runs at
// its full 57 GB/s while other threads touch and register.  (A copy must not span two
// registrations: the runtime fails it.)  hipHostMalloc stays the fallback.
namespace {
struct HostMap {
    char* base = nullptr;  // the mapping (munmap)
    size_t maplen = 0;
    char* p = nullptr;     // the caller's pointer (2 MiB aligned)
    size_t len = 0;
    // (SHD_ROUTE_HOST_CHUNK, read at each allocation: registration boundaries inside a small
    // triangle -- the fill tests)
    size_t chunk = shd::fill_host_chunk(getenv("SHD_ROUTE_HOST_CHUNK"));
    int nchunk = 0;
    std::unique_ptr<std::atomic<int>[]> state;  // per chunk: 0 pending, 1 registered, 2 not registered
    bool whole = false;    // eager form: chunks are only first-touched (state 1 = touched), then
                           // the whole range is registered once, so any copy may span it
    bool whole_reg = false;
    std::atomic<int> next{0};
    std::atomic<bool> stop{false};
    int fail_chunk = getenv("SHD_ROUTE_REGFAIL_CHUNK") ? atoi(getenv("SHD_ROUTE_REGFAIL_CHUNK")) : -1;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::thread> th;
    // wait until every chunk overlapping [off, off + n) is settled (registered or failed)
    void wait_range(size_t off, size_t n) {
        if (!n) return;
        const int c0 = (int)(off / chunk), c1 = (int)std::min<size_t>((off + n - 1) / chunk, nchunk - 1);
        auto settled = [&] {
            for (int k = c0; k <= c1; k++)
                if (state[k].load(std::memory_order_acquire) == 0) return false;
            return true;
        };
        if (settled()) return;
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, settled);
    }
    void worker() {
        for (int k; !stop.load(std::memory_order_relaxed) && (k = next.fetch_add(1)) < nchunk;) {
            char* a = p + (size_t)k * chunk;
            const size_t n = std::min(chunk, len - (size_t)k * chunk);
            for (size_t o = 0; o < n; o += 4096) a[o] = 0;  // (nothing else touches a pending chunk)
            // (SHD_ROUTE_REGFAIL_CHUNK=k: chunk k is left unregistered, as when the runtime
            // refuses it -- the non-fatal path's test)
            const bool ok = whole || (k != fail_chunk && hipHostRegister(a, n, hipHostRegisterPortable) == hipSuccess);
            {
                std::lock_guard<std::mutex> lk(mu);
                state[k].store(ok ? 1 : 2, std::memory_order_release);
            }
            cv.notify_all();
        }
    }
    ~HostMap() {
        stop = true;
        for (auto& t : th) t.join();
        if (whole) {
            if (whole_reg) (void)hipHostUnregister(p);
        } else {
            for (int k = 0; k < nchunk; k++)
                if (state[k].load() == 1) (void)hipHostUnregister(p + (size_t)k * chunk);
        }
        if (base) munmap(base, maplen);
    }
};
std::mutex g_host_mu;
std::map<char*, std::shared_ptr<HostMap>> g_host_maps;  // by the caller's pointer

std::shared_ptr<HostMap> host_map_of(const void* q) {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_maps.upper_bound((char*)q);
    if (it == g_host_maps.begin()) return nullptr;
    --it;
    return (const char*)q < it->first + it->second->len ? it->second : nullptr;
}

void* host_alloc(size_t bytes, bool lazy) {
    if (!bytes) bytes = 1;
    const size_t huge = (size_t)2 << 20;
    const size_t len = (bytes + huge - 1) & ~(huge - 1);
    auto m = std::make_shared<HostMap>();
    void* b = mmap(nullptr, len + huge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (b != MAP_FAILED) {
        m->base = (char*)b;
        m->maplen = len + huge;
        m->p = (char*)(((uintptr_t)b + huge - 1) & ~(uintptr_t)(huge - 1));  // whole huge pages
        m->len = len;
        (void)madvise(m->p, len, MADV_HUGEPAGE);
        m->nchunk = (int)((len + m->chunk - 1) / m->chunk);
        m->state.reset(new std::atomic<int>[m->nchunk]());
        m->whole = !lazy;
        const int nth = std::min(m->nchunk, 12);
        for (int t = 0; t < nth; t++) m->th.emplace_back([mp = m.get()] { mp->worker(); });
        bool ok = true;
        if (!lazy) {
            // touched in parallel, then one registration (a caller's single large copy into
            // the buffer must not span two registrations); on failure, hipHostMalloc below
            m->wait_range(0, len);
            m->whole_reg = ok = hipHostRegister(m->p, len, hipHostRegisterPortable) == hipSuccess;
        }
        if (ok) {
            std::lock_guard<std::mutex> lk(g_host_mu);
            g_host_maps[m->p] = m;
            return m->p;
        }
        m.reset();  // (joins the touch workers and unmaps)
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr;
    return p;
}
}  // namespace

extern "C" {

int shd_route_tri_payload_async(shd_route_t* c, const double* d_lat, const double* d_rel, int64_t ld,
                                const int32_t* d_pos, const int64_t* d_off, int32_t nrows, int32_t na, uint32_t flags,
                                void* d_out_lat, double* d_out_rel, void* stream) {
    if (!c || nrows < 0 || na < 0 || ld < na || (nrows && (!d_lat || !d_rel || !d_pos || !d_off || !d_out_lat || !d_out_rel)))
        return SHD_ROUTE_EINVAL;
    const bool l16 = (flags & SHD_ROUTE_PAYLOAD_LAT16) != 0;
    if (l16 && !lat16_ok(c)) return SHD_ROUTE_EUNSUPPORTED;
    if (nrows == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(std::min(nrows, 8192));
    if (l16)
        hipLaunchKernelGGL(tri_payload_kernel<true>, grid, dim3(256), 0, st, d_lat, d_rel, (long long)ld, d_pos,
                           (const long long*)d_off, nrows, na, d_out_lat, d_out_rel);
    else
        hipLaunchKernelGGL(tri_payload_kernel<false>, grid, dim3(256), 0, st, d_lat, d_rel, (long long)ld, d_pos,
                           (const long long*)d_off, nrows, na, d_out_lat, d_out_rel);
    return hip_check(hipGetLastError());
}

void* shd_route_host_alloc(size_t bytes) { return host_alloc(bytes, false); }

void* shd_route_host_alloc_lazy(size_t bytes) { return host_alloc(bytes, true); }

int shd_route_host_wait(void* p) {
    if (!p) return SHD_ROUTE_EINVAL;
    auto m = host_map_of(p);
    if (!m) return SHD_ROUTE_OK;
    m->wait_range(0, m->len);
    // a chunk the runtime refused to register stays pageable: copies into it still work
    // (slower) and the data is complete, so this is not an error; shd_route_host_unpinned
    // counts such chunks
    return SHD_ROUTE_OK;
}

int64_t shd_route_host_unpinned(void* p) {
    if (!p) return SHD_ROUTE_EINVAL;
    auto m = host_map_of(p);
    if (!m) return 0;
    m->wait_range(0, m->len);
    if (m->whole) return m->whole_reg ? 0 : (int64_t)m->len;
    int64_t bytes = 0;
    for (int k = 0; k < m->nchunk; k++)
        if (m->state[k].load(std::memory_order_acquire) == 2)
            bytes += (int64_t)std::min(m->chunk, m->len - (size_t)k * m->chunk);
    return bytes;
}

void shd_route_host_free(void* p) {
    if (!p) return;
    std::shared_ptr<HostMap> m;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_maps.find((char*)p);
        if (it != g_host_maps.end()) { m = std::move(it->second); g_host_maps.erase(it); }
    }
    if (!m) (void)hipHostFree(p);
    // (else the last reference -- a fill still copying holds one -- joins, unregisters, unmaps)
}

int shd_route_fill_triangle(shd_route_t* c, const int32_t* A, int32_t na, int32_t world, int32_t rank, uint32_t flags,
                            double* lr_out, double* min_out, double* seconds_out) {
    if (!c || na < 0 || (na && (!A || !lr_out)) || world < 1 || rank < 0 || rank >= world) return SHD_ROUTE_EINVAL;
    if (min_out) *min_out = INFINITY;
    const bool l16 = (flags & SHD_ROUTE_FILL_LAT16) != 0;
    // u16 latencies are exact for the source paths (info.lat16) and, with the dispatch, for
    // the direct paths it writes (edge latencies)
    if (l16 && !(lat16_ok(c) && (!(flags & SHD_ROUTE_DISPATCH) || !(c->complete || c->prefer_direct) ||
                                 c->max_w < 65535.0)))
        return SHD_ROUTE_EUNSUPPORTED;
    flags &= ~SHD_ROUTE_FILL_LAT16;
    if (na == 0) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    auto t0 = std::chrono::steady_clock::now();
    shd_route_plan_t* P = nullptr;
    int rc = shd_route_plan_create(c, A, na, world, rank, &P);
    if (rc) return rc;
    std::unique_ptr<shd_route_plan, void (*)(shd_route_plan*)> guard(P, shd_route_plan_destroy);
    const int nr = (int)P->row_pos.size();
    if (nr == 0) return SHD_ROUTE_OK;
    // the schedule (fill_sched.hpp): stage chunks of plan rows, their copy pieces cut at the
    // chunk boundaries of shd_route_host_alloc's memory (a copy waits for the chunks it lands
    // in to be pinned, and never spans two: each is its own registration), and the packed
    // offset of each row in pairs, or in 64-byte lines for the compact layout
    std::vector<int> posv(P->row_pos.begin(), P->row_pos.end());
    const std::shared_ptr<HostMap> hm = host_map_of(lr_out);
    const size_t host_off = hm ? (size_t)((char*)lr_out - hm->p) : 0;
    // (SHD_ROUTE_FILL_STAGE: the pairs per staging buffer, for tests with many stage chunks)
    const size_t stage_pairs = (size_t)shd::fill_stage_pairs(getenv("SHD_ROUTE_FILL_STAGE"), na, l16);
    const shd::FillSchedule sched = shd::fill_schedule(na, posv.data(), nr, l16, shd::fill_stage_units((long long)stage_pairs, l16),
                                                       hm ? hm->chunk : 0, host_off);
    const size_t table = sizeof(double) * (size_t)nr * (size_t)na;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (2 * table + 4 * stage_pairs * 8 + ((size_t)1 << 30) > fr) return SHD_ROUTE_ENOMEM;
    DevBuf dtgt, dlat, drel, dpos, doff, dstage[2], dmn;
    if ((rc = dtgt.alloc(sizeof(int32_t) * na)) || (rc = dlat.alloc(table)) || (rc = drel.alloc(table)) ||
        (rc = dpos.alloc(sizeof(int) * nr)) || (rc = doff.alloc(sizeof(long long) * (nr + 1))) ||
        (rc = dstage[0].alloc(16 * stage_pairs)) || (rc = dstage[1].alloc(16 * stage_pairs)) ||
        (rc = dmn.alloc(sizeof(unsigned long long))))
        return rc;
    hipStream_t cs = nullptr, xs = nullptr;
    if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&xs, hipStreamNonBlocking) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    bool ok = hipMemcpy(dtgt.p, A, sizeof(int32_t) * na, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dpos.p, posv.data(), sizeof(int) * nr, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(doff.p, sched.pk.data(), sizeof(long long) * (nr + 1), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemsetAsync(dmn.p, 0xFF, sizeof(unsigned long long), cs) == hipSuccess;
    // (the plan was made just now: its landmark rows, if any, are current)
    if (ok) rc = shd_route_rows_planned_async(c, P, (const int32_t*)dtgt.p, na, na, flags | SHD_ROUTE_PLAN_REUSE, (double*)dlat.p,
                                              (double*)drel.p, nullptr, cs);
    else rc = SHD_ROUTE_EDEVICE;
    // pack chunks of rows on the compute stream, copy them out on the copy stream; with
    // rows in triangle order (one rank) a chunk is one contiguous range of the cache
    hipEvent_t packed[2], copied[2];
    for (int b = 0; b < 2; b++) { (void)hipEventCreateWithFlags(&packed[b], hipEventDisableTiming); (void)hipEventCreateWithFlags(&copied[b], hipEventDisableTiming); }
    bool first[2] = {true, true};
    for (size_t k = 0; k < sched.chunks.size() && !rc; k++) {
        const shd::FillChunk& ch = sched.chunks[k];
        const int r0 = ch.r0, r1 = ch.r1, buf = ch.buf;
        // (a row longer than a stage buffer cannot happen: the stage holds one row at least)
        if (!first[buf] && hipStreamWaitEvent(cs, copied[buf], 0) != hipSuccess) { rc = SHD_ROUTE_EDEVICE; break; }
        first[buf] = false;
        if (l16)
            hipLaunchKernelGGL(tri_pack16_kernel, dim3(std::min(r1 - r0, 4096)), dim3(256), 0, cs, (const double*)dlat.p,
                               (const double*)drel.p, (long long)na, (const int*)dpos.p, (const long long*)doff.p, r0, r1,
                               na, (uint4*)dstage[buf].p, (unsigned long long*)dmn.p);
        else
            hipLaunchKernelGGL(tri_pack_kernel, dim3(std::min(r1 - r0, 4096)), dim3(256), 0, cs, (const double*)dlat.p,
                               (const double*)drel.p, (long long)na, (const int*)dpos.p, (const long long*)doff.p, r0, r1,
                               na, (double*)dstage[buf].p, (unsigned long long*)dmn.p);
        if (hipGetLastError() != hipSuccess || hipEventRecord(packed[buf], cs) != hipSuccess ||
            hipStreamWaitEvent(xs, packed[buf], 0) != hipSuccess) { rc = SHD_ROUTE_EDEVICE; break; }
        // copy: consecutive rows with consecutive triangle offsets go out in one piece
        for (int q = ch.p0; q < ch.p1; q++) {
            const shd::FillPiece& pc = sched.pieces[q];
            if (hm) hm->wait_range(host_off + (size_t)pc.dst, (size_t)pc.bytes);
            if (hipMemcpyAsync((char*)lr_out + pc.dst, (const char*)dstage[buf].p + pc.src, (size_t)pc.bytes,
                               hipMemcpyDeviceToHost, xs) != hipSuccess) {
                rc = SHD_ROUTE_EDEVICE;
                break;
            }
        }
        if (hipEventRecord(copied[buf], xs) != hipSuccess) rc = SHD_ROUTE_EDEVICE;
    }
    if (hipStreamSynchronize(cs) != hipSuccess || hipStreamSynchronize(xs) != hipSuccess) rc = rc ? rc : SHD_ROUTE_EDEVICE;
    for (int b = 0; b < 2; b++) { (void)hipEventDestroy(packed[b]); (void)hipEventDestroy(copied[b]); }
    (void)hipStreamDestroy(cs); (void)hipStreamDestroy(xs);
    if (rc) return rc;
    const int soft = take_err(c);
    if (soft && soft != SHD_ROUTE_ENOEDGE && soft != SHD_ROUTE_EUNREACH) return soft;
    unsigned long long mb = 0;
    if (hipMemcpy(&mb, dmn.p, sizeof(mb), hipMemcpyDeviceToHost) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (min_out) {
        double m;
        std::memcpy(&m, &mb, sizeof(m));
        *min_out = mb == ~0ull ? INFINITY : m;
    }
    if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return soft;
}

}  // extern "C"

extern "C" int shd_route_kd_stats(shd_route_t* c, uint64_t* out, int reset) {
    if (!c || !out) return SHD_ROUTE_EINVAL;
    for (int q = 0; q < 4; q++) out[q] = 0;
    if (!c->d_kd_stats) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (hipMemcpy(out, c->d_kd_stats, sizeof(uint64_t) * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    if (reset && hipMemset(c->d_kd_stats, 0, sizeof(uint64_t) * 4) != hipSuccess) return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

#ifdef SHD_STAMPS
// Diagnostic builds only (not part of include/shd_route.h): per-source phase stamps.
extern "C" int shd_route_debug_buffer(shd_route_t* c, void* d_buf) {
    if (!c) return SHD_ROUTE_EINVAL;
    c->d_dbg = (unsigned long long*)d_buf;
    return SHD_ROUTE_OK;
}
#endif

// The link edit calls and their kernels (link_edit.hpp) stand behind everything else of the code
// object, so that no kernel the other calls share moves.
#include "link_edit.hpp"
#include "edit_calls.hpp"
