// select_main.cpp -- the kernel selection of shd_route_create on the host alone (tests/test_select.py).
//
//   select_main GRAPH     GRAPH: `n m directed`, one `src dst latency loss` line per edge, then the
//                         n vertex losses (nan: absent)
//
// Builds the host graph as shd_route_create does, runs select_all() under the SHD_ROUTE_* knobs
// of the environment and prints one line: the graph's scalars, every scalar of every choice,
// upload_bytes and a 64-bit FNV-1a digest of each staged array.  It opens no device and launches
// nothing; the test builds it with the address and undefined-behaviour sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../shadow_amd/csrc/common.hpp"
#include "../shadow_amd/csrc/sssp_f64.hpp"
#include "../shadow_amd/csrc/sssp_f64d.hpp"
#include "../shadow_amd/csrc/sssp_k32.hpp"
#include "../shadow_amd/csrc/sssp_batch.hpp"
#include "../shadow_amd/csrc/path_attr.hpp"
#include "../shadow_amd/csrc/sssp_delta.hpp"
#include "../shadow_amd/csrc/select.hpp"

using namespace shd;

static void num(const char* k, long long v) { printf(" %s=%lld", k, v); }
static void real(const char* k, double v) { printf(" %s=%.17g", k, v); }

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: select_main GRAPH\n"); return 2; }
    int n = 0, m = 0, directed = 0;
    if (fscanf(f, "%d %d %d", &n, &m, &directed) != 3 || n <= 0 || m < 0) return 2;
    std::vector<int32_t> src(m), dst(m);
    std::vector<double> lat(m), loss(m), vloss(n);
    for (int e = 0; e < m; e++)
        if (fscanf(f, "%d %d %lf %lf", &src[e], &dst[e], &lat[e], &loss[e]) != 4 || src[e] < 0 || src[e] >= n ||
            dst[e] < 0 || dst[e] >= n)
            return 2;
    for (int v = 0; v < n; v++) if (fscanf(f, "%lf", &vloss[v]) != 1) return 2;
    fclose(f);
    shd_graph_t g{};
    g.n_vertices = n; g.n_edges = m; g.directed = directed;
    g.edge_src = src.data(); g.edge_dst = dst.data(); g.edge_latency = lat.data(); g.edge_packetloss = loss.data();
    g.vertex_packetloss = vloss.data();

    const HostGraph h = HostGraph::make(&g);
    Selection s = select_all(SelectInput(h), SelectKnobs::from_env());

    printf("select");
    num("n", h.n); num("nnz", h.nnz); num("directed", h.directed); num("integer_w", h.integer_w);
    num("multigraph", h.multigraph); num("self16", h.self16); real("min_w", h.min_w);
    num("f64.lds", kSmallBytes + StateLayout::make(n).total <= kLdsBudget); num("f64.block", kBlock);
    num("f64.bytes", (long long)(kSmallBytes + StateLayout::make(n).total));
    num("sel", s.sel); num("upload_bytes", (long long)s.upload_bytes);
    num("inrows.ok", s.inrows.ok); num("inrows.bound", s.inrows.bound);
    num("k32.staged", s.k32.staged); num("k32.ok", s.k32.ok); num("k32.block", s.k32.block);
    num("k32.bound", s.k32.bound); num("k32.lds", (long long)s.k32.lds);
    num("attr.ok", s.attr.ok); num("attr.lds", (long long)s.attr.lds);
    num("kb.staged", s.kb.staged); num("kb.ok", s.kb.ok); num("kb.block", KB_BLOCK); num("kb.nseg", s.kb.nseg);
    num("kb.nhub", s.kb.nhub); num("kb.npart", s.kb.npart); num("kb.lds", (long long)s.kb.lds);
    num("kb.fused", s.kb.fused); num("kb.f_nrtab", s.kb.f_nrtab); num("kb.grid_cap", s.kb.grid_cap);
    num("kb.f_tcap", s.kb.f_tcap); num("kb.f_lds", (long long)s.kb.f_lds);
    num("kd.ok", s.kd.ok); num("kd.block", s.kd.block); num("kd.slots", s.kd.slots); num("kd.delta", s.kd.delta);
    num("kd.qcap", s.kd.qcap); num("kd.lds", (long long)s.kd.lds); num("kd.stride", (long long)s.kd.stride);
    num("kd.hub_block", s.kd.hub_block); num("kd.hub_qcap", s.kd.hub_qcap); num("kd.hub_delta", s.kd.hub_delta);
    num("kd.hub_lds", (long long)s.kd.hub_lds); num("kd.nlight", s.kd.nlight); num("kd.nrtab", s.kd.nrtab);
    num("kd.walk", s.kd.walk); num("kd.packed", s.kd.packed); num("kd.fused", s.kd.fused); num("kd.rone", s.kd.rone);
    num("kf.ok", s.kf.ok); num("kf.block", s.kf.block); num("kf.slots", s.kf.slots); num("kf.lds", (long long)s.kf.lds);
    real("kf.delta", s.kf.delta); num("kf.nrtab", s.kf.nrtab); num("kf.h", s.kf.h);
    num("kf.ws_stride", (long long)s.kf.ws_stride); real("kf.wscale", s.kf.wscale); num("kf.ipk_own", s.kf.ipk_own);
    s.arrays([](const char* name, auto& v, auto*&) {
        uint64_t d = 1469598103934665603ull;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
        for (size_t i = 0; i < sizeof(v[0]) * v.size(); i++) d = (d ^ p[i]) * 1099511628211ull;
        printf(" %s[%zu]=%016" PRIx64, name, v.size(), d);
    });
    printf("\n");
    return 0;
}
