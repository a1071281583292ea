// Stand-alone reader of shadow_amd/csrc/ties_layout.hpp for tests/test_ties.py (no device, no
// HIP): for every n on the command line one line "n total16 total32 fits", and first the
// budget line "budget small", so that tests/ties_ref.py's mirror of the layout is held to it.
#include <cstdio>
#include <cstdlib>

#include "../shadow_amd/csrc/ties_layout.hpp"

int main(int argc, char** argv) {
    std::printf("%zu %zu\n", shd::kTiesLdsBudget, shd::kTiSmall);
    for (int k = 1; k < argc; k++) {
        const int n = std::atoi(argv[k]);
        std::printf("%d %zu %zu %d\n", n, shd::TiesLayout<uint16_t>::make(n).total,
                    shd::TiesLayout<uint32_t>::make(n).total, shd::ties_fits_lds(n) ? 1 : 0);
    }
    return 0;
}
