// Stand-alone reader of shadow_amd/csrc/ecmp_layout.hpp for tests/test_ecmp.py (no device, no
// HIP): for every n on the command line one line "n total16 total32 fits", and first the
// budget line "budget small", so that tests/ecmp_ref.py's mirror of the layout is held to it.
// Every section of the u16 and the u32 layout is also written end to end into a buffer of
// exactly `total` bytes, so that a section that overlaps the next or runs past the end shows
// under the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../shadow_amd/csrc/ecmp_layout.hpp"

template <typename T>
static bool fill(int n) {
    const shd::EcmpLayout<T> L = shd::EcmpLayout<T>::make(n);
    std::vector<unsigned char> buf(L.total, 0);
    const size_t at[6] = {L.sig, L.dl, L.own, L.rem, L.order, L.lvl};
    const size_t len[6] = {8 * (size_t)n, 8 * (size_t)n, 8 * (size_t)n, 4 * (size_t)n, sizeof(T) * (size_t)n,
                           4 * ((size_t)n + 1)};
    for (int k = 0; k < 6; k++) {
        if (at[k] % 16) return false;
        for (size_t b = 0; b < len[k]; b++) {
            if (buf[at[k] + b]) return false;  // two sections share a byte
            buf[at[k] + b] = (unsigned char)(k + 1);
        }
    }
    return true;
}

int main(int argc, char** argv) {
    std::printf("%zu %zu\n", shd::kEcmpLdsBudget, shd::kEcSmall);
    for (int k = 1; k < argc; k++) {
        const int n = std::atoi(argv[k]);
        if (!fill<uint16_t>(n) || !fill<uint32_t>(n)) {
            std::fprintf(stderr, "sections of n = %d overlap or are misaligned\n", n);
            return 1;
        }
        std::printf("%d %zu %zu %d\n", n, shd::EcmpLayout<uint16_t>::make(n).total,
                    shd::EcmpLayout<uint32_t>::make(n).total, shd::ecmp_fits_lds(n) ? 1 : 0);
    }
    return 0;
}
