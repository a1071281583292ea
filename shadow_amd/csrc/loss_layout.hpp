#pragma once
// The per-source state of the link loss sweep (link_loss.hpp) as plain C++: the kernel, the
// launcher and tests/loss_layout_main.cpp (no device, no HIP) all size it from here.
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SHD_LOSS_HD __host__ __device__
#else
#define SHD_LOSS_HD
#endif

namespace shd {

constexpr size_t kLossLdsBudget = 160 * 1024;  // gfx950 LDS per CU (common.hpp's kLdsBudget)
// beside the state: wave sums of the block scan (16 x 4 bytes), the deepest level (at 64) and
// the source's routed weight (u64 at 72)
constexpr size_t kLoSmall = 96;

SHD_LOSS_HD inline size_t loss_a16(size_t x) { return (x + 15) & ~size_t(15); }

// One source's state, 22 bytes per vertex while n <= 65535 and 24 above: per vertex the u64
// weight of the entries that end there, which becomes the subtree's weight in place once the
// targets' step has read it (sum); the survival product from the source (pre, f64); the start
// of every level of the order list (u32; hop depths 0 .. n - 1 and the end); and the reached
// vertices sorted by hop depth (T: u16 while n <= 65535, u32 above).
// The LDS form holds while kLoSmall + total <= kLossLdsBudget: n <= 7442.
template <typename T>
struct LossLayout {
    size_t sum, pre, lvl, order, total;
    SHD_LOSS_HD static LossLayout make(int n) {
        LossLayout L;
        size_t o = 0;
        L.sum = o;   o += loss_a16(sizeof(unsigned long long) * (size_t)n);
        L.pre = o;   o += loss_a16(sizeof(double) * (size_t)n);
        L.lvl = o;   o += loss_a16(sizeof(uint32_t) * ((size_t)n + 1));
        L.order = o; o += loss_a16(sizeof(T) * (size_t)n);
        L.total = o;
        return L;
    }
};

// the state lives in LDS while this holds
inline bool loss_fits_lds(int n) {
    return n <= 65535 && kLoSmall + LossLayout<uint16_t>::make(n).total <= kLossLdsBudget;
}

}  // namespace shd
