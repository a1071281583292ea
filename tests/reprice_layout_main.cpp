// Stand-alone reader of shadow_amd/csrc/reprice_layout.hpp and of path_host.hpp's state_form for
// tests/test_reprice.py (no device, no HIP).  First the line "budget small slab_max units"; then
// for every n on the command line one line "n d16 lvl16 order16 tch16 fr0_16 fr1_16 mark16 tbit16
// fbit16 total16 d32 ... total32 fits" followed by state_form's (form grid lds stride slots) for
// 1,000 units within 256 MiB of slices, with the LDS knob unset and then set; then, behind the
// word "units", for every KxQ one line "k q slab nslab units" (the outage calls' units, which the
// repricing calls take as they are).  Every section of the u16 and the u32 layout is also
// written end to end into a buffer of exactly `total` bytes, so that a section that overlaps the
// next or runs past the end shows under the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../shadow_amd/csrc/reprice_layout.hpp"
#include "../shadow_amd/csrc/path_host.hpp"

template <typename T>
static bool fill(int n) {
    const shd::RepriceLayout<T> L = shd::RepriceLayout<T>::make(n);
    std::vector<unsigned char> buf(L.total, 0);
    const size_t w = 4 * shd::reprice_words(n), t = sizeof(T) * (size_t)n;
    const size_t at[9] = {L.d, L.lvl, L.order, L.tch, L.fr0, L.fr1, L.mark, L.tbit, L.fbit};
    const size_t len[9] = {8 * (size_t)n, 4 * ((size_t)n + 1), t, t, t, t, (size_t)n, w, w};
    for (int k = 0; k < 9; k++) {
        if (at[k] % 16) return false;
        for (size_t b = 0; b < len[k]; b++) {
            if (buf[at[k] + b]) return false;  // two sections share a byte
            buf[at[k] + b] = (unsigned char)(k + 1);
        }
    }
    return L.total % 16 == 0 && 32 * shd::reprice_words(n) >= (size_t)n;
}

template <typename T>
static void show(int n) {
    const shd::RepriceLayout<T> L = shd::RepriceLayout<T>::make(n);
    std::printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", L.d, L.lvl, L.order, L.tch, L.fr0, L.fr1, L.mark, L.tbit,
                L.fbit, L.total);
}

static void form(int n, bool off) {
    const size_t t16 = shd::RepriceLayout<uint16_t>::make(n).total, t32 = shd::RepriceLayout<uint32_t>::make(n).total;
    const shd::StateLaunch f = shd::state_form(n, 0, 1000, shd::kRpSmall, t16, shd::kOutageLdsBudget, off,
                                               shd::outage_a16(t16), shd::outage_a16(t32), (size_t)1 << 28);
    std::printf(" %d %d %zu %zu %d", f.form, f.grid, f.lds, f.stride, f.slots);
}

int main(int argc, char** argv) {
    std::printf("%zu %zu %d %d\n", shd::kOutageLdsBudget, shd::kRpSmall, shd::kOuSlabMax, shd::kOuUnits);
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
        std::printf(" %d", shd::reprice_fits_lds(n) ? 1 : 0);
        form(n, false);
        form(n, true);
        std::printf("\n");
    }
    for (a++; a < argc; a++) {
        int k = 0, q = 0;
        if (std::sscanf(argv[a], "%dx%d", &k, &q) != 2) return 2;
        const shd::OutageUnits U = shd::OutageUnits::make(k, q);
        std::printf("%d %d %d %d %lld\n", k, q, U.slab, U.nslab, U.units);
    }
    return 0;
}
