#pragma once
// The per-source state of the ECMP link loads' sweep (ecmp_loads.hpp) as plain C++: the kernel,
// the launcher and tests/ecmp_layout_main.cpp (no device, no HIP) all size it from here.
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SHD_ECMP_HD __host__ __device__
#else
#define SHD_ECMP_HD
#endif

namespace shd {

constexpr size_t kEcmpLdsBudget = 160 * 1024;  // gfx950 LDS per CU (common.hpp's kLdsBudget)
constexpr size_t kEcSmall = 16;                // beside the state: the length of the order list

SHD_ECMP_HD inline size_t ecmp_a16(size_t x) { return (x + 15) & ~size_t(15); }

// One source's state: per vertex the path count sigma and the dependency delta (f64 bits), the
// summed weight of its own entries (u64), the tight in-arcs not yet released (u32), the
// vertices in the order the forward sweep finalised them (T: u16 while n <= 65535, u32 above)
// and the start of every level in that list (u32; n levels at the most, and the end).
template <typename T>
struct EcmpLayout {
    size_t sig, dl, own, rem, order, lvl, total;
    SHD_ECMP_HD static EcmpLayout make(int n) {
        EcmpLayout L;
        size_t o = 0;
        L.sig = o;   o += ecmp_a16(sizeof(unsigned long long) * (size_t)n);
        L.dl = o;    o += ecmp_a16(sizeof(unsigned long long) * (size_t)n);
        L.own = o;   o += ecmp_a16(sizeof(unsigned long long) * (size_t)n);
        L.rem = o;   o += ecmp_a16(sizeof(uint32_t) * (size_t)n);
        L.order = o; o += ecmp_a16(sizeof(T) * (size_t)n);
        L.lvl = o;   o += ecmp_a16(sizeof(uint32_t) * ((size_t)n + 1));
        L.total = o;
        return L;
    }
};

// the state lives in LDS while this holds
inline bool ecmp_fits_lds(int n) {
    return n <= 65535 && kEcSmall + EcmpLayout<uint16_t>::make(n).total <= kEcmpLdsBudget;
}

}  // namespace shd
