// Stand-alone reader of shadow_amd/csrc/loss_layout.hpp for tests/test_loss.py (no device, no
// HIP): first the budget line "budget small", then for every n on the command line one line
// "n sum16 pre16 lvl16 order16 total16 sum32 pre32 lvl32 order32 total32 fits", so that
// tests/loss_ref.py's mirror of the layout is held to it.  Every section of the u16 and the u32
// layout is also written end to end into a buffer of exactly `total` bytes, so that a section
// that overlaps the next or runs past the end shows under the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../shadow_amd/csrc/loss_layout.hpp"

template <typename T>
static bool fill(int n) {
    const shd::LossLayout<T> L = shd::LossLayout<T>::make(n);
    std::vector<unsigned char> buf(L.total, 0);
    const size_t at[4] = {L.sum, L.pre, L.lvl, L.order};
    const size_t len[4] = {8 * (size_t)n, 8 * (size_t)n, 4 * ((size_t)n + 1), sizeof(T) * (size_t)n};
    for (int k = 0; k < 4; k++) {
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
    const shd::LossLayout<T> L = shd::LossLayout<T>::make(n);
    std::printf(" %zu %zu %zu %zu %zu", L.sum, L.pre, L.lvl, L.order, L.total);
}

int main(int argc, char** argv) {
    std::printf("%zu %zu\n", shd::kLossLdsBudget, shd::kLoSmall);
    for (int k = 1; k < argc; k++) {
        const int n = std::atoi(argv[k]);
        if (!fill<uint16_t>(n) || !fill<uint32_t>(n)) {
            std::fprintf(stderr, "sections of n = %d overlap or are misaligned\n", n);
            return 1;
        }
        std::printf("%d", n);
        show<uint16_t>(n);
        show<uint32_t>(n);
        std::printf(" %d\n", shd::loss_fits_lds(n) ? 1 : 0);
    }
    return 0;
}
