#pragma once
// The per-source state of the tie envelope's sweep (path_ties.hpp) as plain C++: the kernel,
// the launcher and tests/ties_layout_main.cpp (no device, no HIP) all size it from here.
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SHD_TIES_HD __host__ __device__
#else
#define SHD_TIES_HD
#endif

namespace shd {

constexpr size_t kTiesLdsBudget = 160 * 1024;  // gfx950 LDS per CU (common.hpp's kLdsBudget)
constexpr size_t kTiSmall = 16;                // beside the state: the two frontier sizes

SHD_TIES_HD inline size_t ties_a16(size_t x) { return (x + 15) & ~size_t(15); }

// One source's state: per vertex the path count, the bounds (f64 bits), the tight in-arcs not
// yet released, and two frontier lists of T (u16 while n <= 65535, u32 above).
template <typename T>
struct TiesLayout {
    size_t cnt, lo, hi, rem, f0, f1, total;
    SHD_TIES_HD static TiesLayout make(int n) {
        TiesLayout L;
        size_t o = 0;
        L.cnt = o; o += ties_a16(sizeof(unsigned long long) * (size_t)n);
        L.lo = o;  o += ties_a16(sizeof(unsigned long long) * (size_t)n);
        L.hi = o;  o += ties_a16(sizeof(unsigned long long) * (size_t)n);
        L.rem = o; o += ties_a16(sizeof(uint32_t) * (size_t)n);
        L.f0 = o;  o += ties_a16(sizeof(T) * (size_t)n);
        L.f1 = o;  o += ties_a16(sizeof(T) * (size_t)n);
        L.total = o;
        return L;
    }
};

// the state lives in LDS while this holds
inline bool ties_fits_lds(int n) {
    return n <= 65535 && kTiSmall + TiesLayout<uint16_t>::make(n).total <= kTiesLdsBudget;
}

}  // namespace shd
