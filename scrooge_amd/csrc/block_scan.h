// block_scan.h — the workgroup scan that the reduce-then-scan passes share: the pileup's finish (pileup_kernels.hip) and the
// compaction of the pileup sites (site_kernels.hip).  Both sum per tile, let ONE workgroup turn the tile sums into what lies in
// front of every tile, and finish per tile; no workgroup waits for another inside a kernel.
#pragma once

#include "run_walk.h"

namespace scrg {

constexpr uint32_t SCAN_THREADS = 1024;

// the inclusive scan of one value per thread over a workgroup of SCAN_THREADS; *total: the sum of all of them
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t v, uint32_t* wave_tot, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t in = wave_scan_incl(v, lane);
    __syncthreads();                              // (the array may still be read from the round before)
    if (lane == 63u) wave_tot[wave] = in;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SCAN_THREADS / 64u; w++) {
        const uint32_t x = wave_tot[w];
        if (w < wave) before += x;
        all += x;
    }
    *total = all;
    return in + before;
}

// one workgroup of SCAN_THREADS: s[0 .. n) becomes what lies in front of every element (mod 2^32), SCAN_THREADS of them per round
// with a carry; every thread returns the sum of all.  wave_tot: SCAN_THREADS / 64 words of LDS.
__device__ __forceinline__ uint32_t block_scan_excl_in_place(uint32_t* __restrict__ s, uint64_t n, uint32_t* wave_tot)
{
    uint32_t carry = 0;
    for (uint64_t base = 0; base < n; base += SCAN_THREADS) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < n ? s[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_scan_incl(v, wave_tot, &total);
        if (i < n) s[i] = carry + incl - v;
        carry += total;
    }
    return carry;
}

}  // namespace scrg
