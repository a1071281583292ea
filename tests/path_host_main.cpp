// path_host_main.cpp -- the host stages of the path calls on the host alone (tests/test_path_host.py).
//
//   path_host_main arcs GRAPH      GRAPH in select_main's format: `n m directed`, one `src dst latency
//                                  loss` line per edge (the vertex losses behind them are not read).
//                                  Prints what the first hops call and the first ties call upload.
//   path_host_main pairs PAIRS     PAIRS: `np weighted`, then one `src tgt [weight]` line per pair.
//                                  Prints the pairs grouped by source.
//   path_host_main chunks N COUNT BUDGET HROW
//   path_host_main form FAMILY MODE K SLOT_BUDGET N...
//                                  FAMILY hops, loads or ties: the launch form of its state kernel at each
//                                  vertex count N (one line each), sized by the kernel header's own
//                                  formulas, under the family's SHD_ROUTE_*_LDS knob of the environment.
//
// One `name: values` line per array.  It opens no device and launches nothing; the test builds it
// with the address and undefined-behaviour sanitizers.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../shadow_amd/csrc/common.hpp"
#include "../shadow_amd/csrc/path_hops.hpp"
#include "../shadow_amd/csrc/link_loads.hpp"
#include "../shadow_amd/csrc/ties_layout.hpp"
#include "../shadow_amd/csrc/path_host.hpp"

using namespace shd;

template <typename V>
static void line(const char* name, const V& v) {
    printf("%s:", name);
    for (auto x : v) {
        if constexpr (std::is_floating_point<typename V::value_type>::value) printf(" %.17g", (double)x);
        else printf(" %lld", (long long)x);
    }
    printf("\n");
}

static int arcs(const char* path) {
    FILE* f = fopen(path, "r");
    int n = 0, m = 0, directed = 0;
    if (!f || fscanf(f, "%d %d %d", &n, &m, &directed) != 3 || n <= 0 || m < 0) return 2;
    std::vector<int32_t> src(m), dst(m);
    std::vector<double> lat(m), rel(m);
    for (int e = 0; e < m; e++) {
        double loss;
        if (fscanf(f, "%d %d %lf %lf", &src[e], &dst[e], &lat[e], &loss) != 4 || src[e] < 0 || src[e] >= n ||
            dst[e] < 0 || dst[e] >= n)
            return 2;
        rel[e] = 1.0f - loss;  // as HostGraph::make
    }
    fclose(f);
    const PathArcs a(n, directed != 0, src, dst);
    const PathCsr in = path_in_csr(n, a, lat.data(), rel), out = path_out_csr(n, a, lat.data(), rel);
    line("self", a.self);
    line("in.row", in.row); line("in.col", in.col); line("in.eid", in.eid); line("in.w", in.w); line("in.r", in.r);
    line("out.row", out.row); line("out.col", out.col); line("out.eid", out.eid); line("out.w", out.w);
    return 0;
}

static int pairs(const char* path) {
    FILE* f = fopen(path, "r");
    int np = 0, weighted = 0;
    if (!f || fscanf(f, "%d %d", &np, &weighted) != 2 || np < 0) return 2;
    std::vector<int32_t> src(np), tgt(np);
    std::vector<uint64_t> wt(np);
    for (int k = 0; k < np; k++)
        if (fscanf(f, "%d %d", &src[k], &tgt[k]) != 2 || (weighted && fscanf(f, "%" SCNu64, &wt[k]) != 1)) return 2;
    fclose(f);
    const PairGroups p = group_pairs(src.data(), tgt.data(), weighted ? wt.data() : nullptr, np);
    line("order", p.order); line("us", p.us); line("first", p.first); line("gsi", p.gsi); line("gt", p.gt);
    line("gw", p.gw);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "arcs")) return arcs(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "pairs")) return pairs(argv[2]);
    if (argc == 6 && !strcmp(argv[1], "chunks")) {
        const ScratchChunks s = scratch_chunks(atoi(argv[2]), atoi(argv[3]), strtoull(argv[4], nullptr, 10), atoi(argv[5]) != 0);
        printf("chunk=%d bytes=%zu par_off=%zu hrow_off=%zu\n", s.chunk, s.bytes, s.par_off, s.hrow_off);
        return 0;
    }
    for (int q = 6; argc >= 7 && !strcmp(argv[1], "form") && q < argc; q++) {
        const int n = atoi(argv[q]), mode = atoi(argv[3]), k = atoi(argv[4]);
        const size_t slot_budget = strtoull(argv[5], nullptr, 10);
        StateLaunch f;
        if (!strcmp(argv[2], "hops"))
            f = state_form(n, mode, k, kHpSmall, hp_state_bytes<uint16_t>(n), kLdsBudget,
                           knob_off(getenv("SHD_ROUTE_HOPS_LDS")), a16(hp_state_bytes<uint16_t>(n)),
                           a16(hp_state_bytes<uint32_t>(n)), slot_budget);
        else if (!strcmp(argv[2], "loads"))
            f = state_form(n, mode, k, kLdSmall, ld_state_bytes<uint16_t>(n), kLdsBudget,
                           knob_off(getenv("SHD_ROUTE_LOADS_LDS")), a16(ld_state_bytes<uint16_t>(n)),
                           a16(ld_state_bytes<uint32_t>(n)), slot_budget);
        else if (!strcmp(argv[2], "ties"))
            f = state_form(n, mode, k, kTiSmall, TiesLayout<uint16_t>::make(n).total, kTiesLdsBudget,
                           knob_off(getenv("SHD_ROUTE_TIES_LDS")), a16(TiesLayout<uint16_t>::make(n).total),
                           a16(TiesLayout<uint32_t>::make(n).total), slot_budget);
        else
            return 2;
        printf("form=%d grid=%d lds=%zu stride=%zu slots=%d\n", f.form, f.grid, f.lds, f.stride, f.slots);
        if (q + 1 == argc) return 0;
    }
    fprintf(stderr, "usage: path_host_main arcs GRAPH | pairs PAIRS | chunks N COUNT BUDGET HROW | "
                    "form FAMILY MODE K SLOT_BUDGET N...\n");
    return 2;
}
