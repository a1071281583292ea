#pragma once
// The per-workgroup state of the link repricing (link_reprice.hpp) as plain C++: the kernel, the
// launcher and tests/reprice_layout_main.cpp (no device, no HIP) all size it from here.  It is
// the outage state (outage_layout.hpp, whose units, slab limit and budget it takes as they are)
// with the distance of every vertex instead of the marked ones alone, the two frontier lists of
// the propagation and the two bitmaps that keep a vertex from entering a list twice.
#include "outage_layout.hpp"

namespace shd {

// Beside the state: wave sums of the block scan (16 x 4 bytes), then as u32 / i32 the deepest
// level (64), the shallowest and the deepest root (68, 72), the number of marked vertices (76),
// the changed flag (80), the number of live scenarios (84), the length of the touched list (88)
// and of the two frontier lists (92, 96); as u64 the workgroup's hit, slower and faster sums
// (104, 112, 120), the bits of its largest added and gained latency (128, 136) and of its
// smallest new latency (144), and the bits of the source's smallest old latency (152); the live
// list (u32 per scenario of the slab, from 192) and the live flags (u8 each, behind it).
constexpr size_t kRpAcc = 104;
constexpr size_t kRpOldMin = 152;
constexpr size_t kRpLive = 192;
constexpr size_t kRpFlags = kRpLive + sizeof(uint32_t) * kOuSlabMax;
constexpr size_t kRpSmall = kRpFlags + kOuSlabMax;

SHD_OUT_HD inline size_t reprice_words(int n) { return ((size_t)n + 31) / 32; }

// One workgroup's state, 21.25 bytes per vertex while n <= 65535 and 29.25 above: per vertex its
// current distance as the bits of an f64 (d: the old row between two scenarios), the mark (u8),
// the start of every level of the order list (u32; hop depths 0 .. n - 1 and the end), the
// reached vertices sorted by hop depth (order), the touched vertices (tch: the marked ones in the
// order they were met, then every other vertex whose distance fell), the frontier of the round
// and the one it builds (fr0, fr1; T: u16 while n <= 65535, u32 above), and one bit per vertex
// for "in the touched list though unmarked" (tbit) and "in the frontier being built" (fbit), in
// u32 words because LDS has no byte atomics.
// The LDS form holds while kRpSmall + total <= kOutageLdsBudget: n <= 7456.
template <typename T>
struct RepriceLayout {
    size_t d, lvl, order, tch, fr0, fr1, mark, tbit, fbit, total;
    SHD_OUT_HD static RepriceLayout make(int n) {
        RepriceLayout L;
        size_t o = 0;
        L.d = o;     o += outage_a16(sizeof(unsigned long long) * (size_t)n);
        L.lvl = o;   o += outage_a16(sizeof(uint32_t) * ((size_t)n + 1));
        L.order = o; o += outage_a16(sizeof(T) * (size_t)n);
        L.tch = o;   o += outage_a16(sizeof(T) * (size_t)n);
        L.fr0 = o;   o += outage_a16(sizeof(T) * (size_t)n);
        L.fr1 = o;   o += outage_a16(sizeof(T) * (size_t)n);
        L.mark = o;  o += outage_a16((size_t)n);
        L.tbit = o;  o += outage_a16(sizeof(uint32_t) * reprice_words(n));
        L.fbit = o;  o += outage_a16(sizeof(uint32_t) * reprice_words(n));
        L.total = o;
        return L;
    }
};

// the state lives in LDS while this holds
inline bool reprice_fits_lds(int n) {
    return n <= 65535 && kRpSmall + RepriceLayout<uint16_t>::make(n).total <= kOutageLdsBudget;
}

}  // namespace shd
