#pragma once
// The small LDS header of the link edits (link_edit.hpp) as plain C++: the per-vertex state is the
// repricing's (RepriceLayout, reprice_layout.hpp, taken as it is, and with it the LDS limit of
// 7,456 vertices); only the workgroup's accumulators differ, a scenario having one statistic more.
#include "reprice_layout.hpp"

namespace shd {

// As reprice_layout.hpp's header up to the frontier lengths (92, 96); then as u64 the workgroup's
// hit, cut, slower and faster sums (104 .. 135), the bits of its largest added and gained latency
// (136, 144) and of its smallest new latency (152), and the bits of the source's smallest old
// latency (160); the live list and the live flags where the repricing has them.
constexpr size_t kEdAcc = 104;
constexpr int kEdNAcc = 7;
constexpr size_t kEdOldMin = kEdAcc + sizeof(unsigned long long) * kEdNAcc;
constexpr size_t kEdLive = kRpLive;
constexpr size_t kEdFlags = kRpFlags;
constexpr size_t kEdSmall = kRpSmall;
static_assert(kEdAcc % 8 == 0 && kEdOldMin + sizeof(unsigned long long) <= kEdLive,
              "the accumulators end before the live list");

}  // namespace shd
