#pragma once
// The per-source state of the path folds' sweep (path_fold.hpp) as plain C++: the kernel, the
// launcher and tests/fold_layout_main.cpp (no device, no HIP) all size it from here.
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SHD_FOLD_HD __host__ __device__
#else
#define SHD_FOLD_HD
#endif

namespace shd {

constexpr size_t kFoldLdsBudget = 160 * 1024;  // gfx950 LDS per CU (common.hpp's kLdsBudget)
constexpr size_t kFoSmall = 96;                // beside the state: wave sums of the block scan (16), the deepest level

SHD_FOLD_HD inline size_t fold_a16(size_t x) { return (x + 15) & ~size_t(15); }

// One source's state: per vertex the fold carried from the source (f64, reused fold after
// fold), the start of every level of the order list (u32; hop depths 0 .. n - 1 and the end)
// and the reached vertices sorted by hop depth (T: u16 while n <= 65535, u32 above).
template <typename T>
struct FoldLayout {
    size_t val, lvl, order, total;
    SHD_FOLD_HD static FoldLayout make(int n) {
        FoldLayout L;
        size_t o = 0;
        L.val = o;   o += fold_a16(sizeof(double) * (size_t)n);
        L.lvl = o;   o += fold_a16(sizeof(uint32_t) * ((size_t)n + 1));
        L.order = o; o += fold_a16(sizeof(T) * (size_t)n);
        L.total = o;
        return L;
    }
};

// the state lives in LDS while this holds
inline bool fold_fits_lds(int n) {
    return n <= 65535 && kFoSmall + FoldLayout<uint16_t>::make(n).total <= kFoldLdsBudget;
}

}  // namespace shd
