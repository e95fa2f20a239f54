// clip_rule.h — the argument checks of soft clipping (include/scrooge_amd.h: SOFT CLIPPING) that the handle setting, the device
// entry point, the chunk pipeline and the host function (scrg_io.cpp, which sees nothing of HIP) share.
#pragma once

#include <algorithm>
#include <cstdint>

namespace scrg_host {

// match in 1..255, mismatch, gap_open and gap_extend in 0..255
inline bool clip_costs_ok(const int32_t* c) { return c[0] >= 1 && c[0] <= 255 && c[1] >= 0 && c[1] <= 255 && c[2] >= 0 && c[2] <= 255 && c[3] >= 0 && c[3] <= 255; }
// the scores of alignments of up to `bases` bases of read and text together fit 32 bits
inline bool clip_scores_fit(const int32_t* c, uint64_t bases)
{
    const uint64_t worst = (uint64_t)std::max(std::max(c[0], c[1]), c[2] + c[3]);
    return bases < (1ull << 31) && bases * worst < (1ull << 31);
}

}  // namespace scrg_host
