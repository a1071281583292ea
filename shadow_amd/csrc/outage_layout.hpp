#pragma once
// The per-workgroup state of the link outage repair (link_outage.hpp) and its unit arithmetic
// as plain C++: the kernel, the launcher and tests/outage_layout_main.cpp (no device, no HIP)
// all size it from here.
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SHD_OUT_HD __host__ __device__
#else
#define SHD_OUT_HD
#endif

namespace shd {

constexpr size_t kOutageLdsBudget = 160 * 1024;  // gfx950 LDS per CU (common.hpp's kLdsBudget)
constexpr int kOuSlabMax = 1024;                 // scenarios of one work unit at the most
constexpr int kOuUnits = 1024;                   // units a launch aims at, while the scenarios allow
// Beside the state: wave sums of the block scan (16 x 4 bytes), then as i32 the deepest level
// (64), the shallowest and the deepest root (68, 72), the length of the affected list (76), the
// changed flag (80) and the number of live scenarios (84); as u64 the workgroup's hit, cut and
// slower sums (88, 96, 104) and the bits of its largest added latency (112); the live list
// (u32 per scenario of the slab, from 128) and the live flags (u8 each, behind it).
constexpr size_t kOuLive = 128;
constexpr size_t kOuFlags = kOuLive + sizeof(uint32_t) * kOuSlabMax;
constexpr size_t kOuSmall = kOuFlags + kOuSlabMax;

SHD_OUT_HD inline size_t outage_a16(size_t x) { return (x + 15) & ~size_t(15); }

// One workgroup's state, 17 bytes per vertex while n <= 65535 and 21 above: per vertex the
// repaired distance as the bits of an f64 (dnew; read only where marked), the mark (u8), the
// start of every level of the order list (u32; hop depths 0 .. n - 1 and the end), the reached
// vertices sorted by hop depth (order) and the marked ones in the order they were met
// (aff; T: u16 while n <= 65535, u32 above).
// The LDS form holds while kOuSmall + total <= kOutageLdsBudget: n <= 9328.
template <typename T>
struct OutageLayout {
    size_t dnew, lvl, order, aff, mark, total;
    SHD_OUT_HD static OutageLayout make(int n) {
        OutageLayout L;
        size_t o = 0;
        L.dnew = o;  o += outage_a16(sizeof(unsigned long long) * (size_t)n);
        L.lvl = o;   o += outage_a16(sizeof(uint32_t) * ((size_t)n + 1));
        L.order = o; o += outage_a16(sizeof(T) * (size_t)n);
        L.aff = o;   o += outage_a16(sizeof(T) * (size_t)n);
        L.mark = o;  o += outage_a16((size_t)n);
        L.total = o;
        return L;
    }
};

// the state lives in LDS while this holds
inline bool outage_fits_lds(int n) {
    return n <= 65535 && kOuSmall + OutageLayout<uint16_t>::make(n).total <= kOutageLdsBudget;
}

// A work unit is one source with a slab of scenarios: k sources x nslab slabs of `slab`
// scenarios each (the last one shorter).  The slabs are as long as kOuSlabMax allows while the
// launch still has kOuUnits units; a call without scenarios keeps one empty slab per source,
// which judges the entries that fail in the graph itself.
struct OutageUnits {
    int slab, nslab;
    long long units;
    SHD_OUT_HD static OutageUnits make(int k, int nscn) {
        OutageUnits u;
        const int per = nscn <= 0 ? 1 : (kOuUnits + k - 1) / (k > 0 ? k : 1);  // slabs wanted per source
        int slab = nscn <= 0 ? 1 : (nscn + per - 1) / per;
        if (slab < 1) slab = 1;
        if (slab > kOuSlabMax) slab = kOuSlabMax;
        u.slab = slab;
        u.nslab = nscn <= 0 ? 1 : (nscn + slab - 1) / slab;
        u.units = (long long)k * u.nslab;
        return u;
    }
    // unit x = source x / nslab and scenarios k0 .. k1 of slab x % nslab
    SHD_OUT_HD int source(long long x) const { return (int)(x / nslab); }
    SHD_OUT_HD int first(long long x) const { return (int)(x % nslab) * slab; }
    SHD_OUT_HD int last(long long x, int nscn) const {
        const long long e = (long long)first(x) + slab;
        return e < nscn ? (int)e : (nscn < 0 ? 0 : nscn);
    }
};

}  // namespace shd
