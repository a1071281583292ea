// Stand-alone reader of shadow_amd/csrc/edit_host.hpp and edit_layout.hpp for tests/test_edit.py
// (no device, no HIP).  Without arguments: the line "acc nacc oldmin live small reprice_small" of
// the small LDS header.  With the five arguments off edge a b lat (comma-separated columns, "-" =
// empty) one call's scenario records on the graph below go through EditHostScn::take: the line
// "rc", and for SHD_ROUTE_OK behind it the number of records and every record "edge a b lat" in
// the order the device gets them.
//   The graph: 6 vertices, the edges 0-1, 1-2, 2-3, 3-4, 4-5 at latencies 1 .. 5 and as edge 5 the
// self-loop 2-2 at 9.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../shadow_amd/csrc/edit_host.hpp"
#include "../shadow_amd/csrc/edit_layout.hpp"

template <typename V, typename F>
static std::vector<V> column(const char* s, F parse) {
    std::vector<V> out;
    if (!std::strcmp(s, "-")) return out;
    std::string t(s);
    size_t p = 0;
    while (p <= t.size()) {
        size_t q = t.find(',', p);
        if (q == std::string::npos) q = t.size();
        out.push_back(parse(t.substr(p, q - p).c_str()));
        p = q + 1;
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc == 1) {
        std::printf("%zu %d %zu %zu %zu %zu\n", shd::kEdAcc, shd::kEdNAcc, shd::kEdOldMin, shd::kEdLive, shd::kEdSmall,
                    shd::kRpSmall);
        return 0;
    }
    if (argc != 6) return 2;
    const std::vector<int32_t> e_src{0, 1, 2, 3, 4, 2}, e_dst{1, 2, 3, 4, 5, 2};
    const std::vector<double> e_lat{1, 2, 3, 4, 5, 9};
    const int n = 6, m = 6;
    const auto off = column<int64_t>(argv[1], [](const char* x) { return (int64_t)std::atoll(x); });
    const auto edge = column<int32_t>(argv[2], [](const char* x) { return (int32_t)std::atoi(x); });
    const auto a = column<int32_t>(argv[3], [](const char* x) { return (int32_t)std::atoi(x); });
    const auto b = column<int32_t>(argv[4], [](const char* x) { return (int32_t)std::atoi(x); });
    const auto lat = column<double>(argv[5], [](const char* x) { return std::strtod(x, nullptr); });
    if (off.empty() || edge.size() != lat.size() || a.size() != lat.size() || b.size() != lat.size()) return 2;
    double lo, hi;
    shd::edit_graph_lohi(m, e_src.data(), e_dst.data(), e_lat.data(), &lo, &hi);
    if (lo != 1.0 || hi != 5.0) return 3;  // the self-loop's 9 takes no part
    shd::EditHostScn h;
    // exact-size heap copies: a read past a column's end is the sanitizer's to see
    const int rc = h.take(n, m, e_src.data(), e_dst.data(), lo, hi, off.data(), edge.empty() ? nullptr : edge.data(),
                          a.empty() ? nullptr : a.data(), b.empty() ? nullptr : b.data(),
                          lat.empty() ? nullptr : lat.data(), (int32_t)off.size() - 1);
    std::printf("%d", rc);
    if (rc == SHD_ROUTE_OK) {
        std::printf(" %zu", h.edge.size());
        if (h.off.size() != off.size() || h.a.size() != h.edge.size() || h.lat.size() != h.edge.size()) return 4;
        for (size_t x = 0; x < h.edge.size(); x++) std::printf(" %d %d %d %.17g", h.edge[x], h.a[x], h.b[x], h.lat[x]);
    }
    std::printf("\n");
    return 0;
}
