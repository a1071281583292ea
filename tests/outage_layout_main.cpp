// Stand-alone reader of shadow_amd/csrc/outage_layout.hpp and of path_host.hpp's state_form for
// tests/test_outage.py (no device, no HIP).  First the line "budget small slab_max units"; then
// for every n on the command line one line "n dnew16 lvl16 order16 aff16 mark16 total16 dnew32
// ... total32 fits" followed by state_form's (form grid lds stride slots) for 1,000 units within
// 256 MiB of slices, with the LDS knob unset and then set; then, behind the word "units", for
// every KxQ one line "k q slab nslab units ok", ok = 1 when walking every unit meets every
// (source, scenario) exactly once and no slab is longer than the limit.  Every section of the u16
// and the u32 layout is also written end to end into a buffer of exactly `total` bytes, so that
// a section that overlaps the next or runs past the end shows under the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../shadow_amd/csrc/outage_layout.hpp"
#include "../shadow_amd/csrc/path_host.hpp"

template <typename T>
static bool fill(int n) {
    const shd::OutageLayout<T> L = shd::OutageLayout<T>::make(n);
    std::vector<unsigned char> buf(L.total, 0);
    const size_t at[5] = {L.dnew, L.lvl, L.order, L.aff, L.mark};
    const size_t len[5] = {8 * (size_t)n, 4 * ((size_t)n + 1), sizeof(T) * (size_t)n, sizeof(T) * (size_t)n, (size_t)n};
    for (int k = 0; k < 5; k++) {
        if (at[k] % 16) return false;
        for (size_t b = 0; b < len[k]; b++) {
            if (buf[at[k] + b]) return false;  // two sections share a byte
            buf[at[k] + b] = (unsigned char)(k + 1);
        }
    }
    return L.total % 16 == 0;
}

template <typename T>
static void show(int n) {
    const shd::OutageLayout<T> L = shd::OutageLayout<T>::make(n);
    std::printf(" %zu %zu %zu %zu %zu %zu", L.dnew, L.lvl, L.order, L.aff, L.mark, L.total);
}

static void form(int n, bool off) {
    const size_t t16 = shd::OutageLayout<uint16_t>::make(n).total, t32 = shd::OutageLayout<uint32_t>::make(n).total;
    const shd::StateLaunch f = shd::state_form(n, 0, 1000, shd::kOuSmall, t16, shd::kOutageLdsBudget, off,
                                               shd::outage_a16(t16), shd::outage_a16(t32), (size_t)1 << 28);
    std::printf(" %d %d %zu %zu %d", f.form, f.grid, f.lds, f.stride, f.slots);
}

static bool walk(int k, int q, const shd::OutageUnits& U) {
    std::vector<unsigned char> met((size_t)k * (size_t)(q > 0 ? q : 1), 0);
    std::vector<unsigned char> judged(k, 0);  // the source's first slab judges its failed entries
    for (long long x = 0; x < U.units; x++) {
        const int i = U.source(x), k0 = U.first(x), k1 = U.last(x, q);
        if (i < 0 || i >= k || k0 < 0 || k1 > (q > 0 ? q : 0) || k1 - k0 > shd::kOuSlabMax || k1 - k0 > U.slab) return false;
        if (k0 == 0) judged[i]++;
        for (int s = k0; s < k1; s++) met[(size_t)i * q + s]++;
    }
    for (int i = 0; i < k; i++)
        if (judged[i] != 1) return false;
    if (q > 0)
        for (unsigned char m : met)
            if (m != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    std::printf("%zu %zu %d %d\n", shd::kOutageLdsBudget, shd::kOuSmall, shd::kOuSlabMax, shd::kOuUnits);
    int a = 1;
    for (; a < argc && std::strcmp(argv[a], "units"); a++) {
        const int n = std::atoi(argv[a]);
        if (!fill<uint16_t>(n) || !fill<uint32_t>(n)) {
            std::fprintf(stderr, "sections of n = %d overlap or are misaligned\n", n);
            return 1;
        }
        std::printf("%d", n);
        show<uint16_t>(n);
        show<uint32_t>(n);
        std::printf(" %d", shd::outage_fits_lds(n) ? 1 : 0);
        form(n, false);
        form(n, true);
        std::printf("\n");
    }
    for (a++; a < argc; a++) {
        int k = 0, q = 0;
        if (std::sscanf(argv[a], "%dx%d", &k, &q) != 2) return 2;
        const shd::OutageUnits U = shd::OutageUnits::make(k, q);
        std::printf("%d %d %d %d %lld %d\n", k, q, U.slab, U.nslab, U.units, walk(k, q, U) ? 1 : 0);
    }
    return 0;
}
