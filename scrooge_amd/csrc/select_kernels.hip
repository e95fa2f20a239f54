// select_kernels.hip — best-candidate selection (SCRG_OUT_BEST, scrg_select_best): of every group of consecutive pairs with the
// same key (a read's candidates), the eligible pair (status != over the edit limit) with the smallest edit distance stays as
// it is, ties to the lowest index; every other eligible pair loses its runs (count 0) and gets LANE_STATUS_NOT_BEST.
// 16 bytes read and at most 9 written per pair, twice: the cost is the two launches, not the traffic.
//
// One lane per pair, one wavefront per 64 pairs.  A lane's value is (edit distance << 32) | index, so that the minimum of a
// group is its winner and names it.  Inside a wavefront a segmented min-scan over the lanes (6 shuffle steps) gives every
// "piece" (the part of a group that lies in this wavefront) its minimum.  A group of any size may run over wavefronts and
// workgroups: select_summary_kernel leaves three words per wavefront — whether a group starts in it, the minimum of its
// leading piece (the lanes before the first start) and of its trailing piece (from the last start on) — and
// select_mark_kernel, which repeats the cheap in-wavefront part, completes its leading piece by walking back over the
// summaries, 64 wavefronts per step, to the wavefront the group starts in, and its trailing piece by walking forward to the
// wavefront the next group starts in.  No atomics, no initialised scratch, and the same result in any schedule.
#include "genasm_kernels.h"
#include "host_path.h"

namespace scrg {

namespace {

constexpr uint64_t SEL_NONE = ~0ull;
constexpr uint32_t SEL_HAS_START = 1u, SEL_LANE0_START = 2u;

__device__ __forceinline__ uint64_t sel_shfl(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t sel_shfl_up(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t sel_wave_min(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

struct SelLane {
    uint64_t mine;       // this pair's value; SEL_NONE: not eligible (or past the end)
    uint64_t piece;      // minimum of the piece this lane is in
    uint64_t starts;     // lanes at which a group starts (lanes past the end count as starts of their own)
    bool leading;        // no start at or before this lane: the piece continues a group of an earlier wavefront
    bool trailing;       // no start after this lane: the group may go on in the next wavefront
};

__device__ __forceinline__ SelLane sel_wave(uint64_t n, uint64_t i, uint32_t lane, const uint32_t* __restrict__ key, uint32_t key_mask,
                                            const int64_t* __restrict__ ed, const uint32_t* __restrict__ status)
{
    SelLane s;
    bool start = true;
    s.mine = SEL_NONE;
    if (i < n) {
        start = i == 0 || ((key[i - 1] ^ key[i]) & key_mask) != 0u;
        if (status[i] != (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT) s.mine = ((uint64_t)(uint32_t)ed[i] << 32) | (uint32_t)i;
    }
    s.starts = __ballot(start);
    const uint64_t upto = (2ull << lane) - 1ull;                  // lanes 0..lane (lane 63: all)
    const uint64_t below = s.starts & upto, above = s.starts & ~upto;
    s.leading = below == 0;
    s.trailing = above == 0;
    const uint32_t seg_first = below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
    const uint32_t seg_last = above ? (uint32_t)__builtin_ctzll(above) - 1u : 63u;
    uint64_t v = s.mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = sel_shfl_up(v, d);
        if (lane >= seg_first + (uint32_t)d && o < v) v = o;
    }
    s.piece = sel_shfl(v, (int)seg_last);
    return s;
}

}  // namespace

// summaries: [lead: n_waves x 8 | trail: n_waves x 8 | flags: n_waves x 4]
__global__ __launch_bounds__(256) void select_summary_kernel(uint64_t n, const uint32_t* __restrict__ key, uint32_t key_mask,
                                                             const int64_t* __restrict__ ed, const uint32_t* __restrict__ status,
                                                             uint64_t n_waves, uint64_t* __restrict__ lead, uint64_t* __restrict__ trail,
                                                             uint32_t* __restrict__ flags)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, w = i >> 6;
    if (w >= n_waves) return;
    const SelLane s = sel_wave(n, i, lane, key, key_mask, ed, status);
    if (lane == 0) {
        lead[w] = s.leading ? s.piece : SEL_NONE;
        flags[w] = (s.starts ? SEL_HAS_START : 0u) | ((s.starts & 1ull) ? SEL_LANE0_START : 0u);
    }
    if (lane == 63) trail[w] = s.piece;
}

__global__ __launch_bounds__(256) void select_mark_kernel(uint64_t n, const uint32_t* __restrict__ key, uint32_t key_mask,
                                                          const int64_t* __restrict__ ed, uint32_t* __restrict__ status,
                                                          uint32_t* __restrict__ n_runs, uint8_t* __restrict__ is_best, uint64_t n_waves,
                                                          const uint64_t* __restrict__ lead, const uint64_t* __restrict__ trail,
                                                          const uint32_t* __restrict__ flags)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, w = i >> 6;
    if (w >= n_waves) return;
    const SelLane s = sel_wave(n, i, lane, key, key_mask, ed, status);
    // the rest of the group the leading piece belongs to: the trailing pieces of the wavefronts before this one, back to the
    // one the group starts in (wavefront 0 starts a group at its lane 0, so the walk ends)
    uint64_t back = SEL_NONE, fwd = SEL_NONE;
    if (!(s.starts & 1ull)) {
        for (uint64_t done = 0; done < w; done += 64) {
            const bool valid = done + lane < w;
            const uint64_t j = valid ? w - 1 - done - lane : 0;
            const uint64_t stop = __ballot(valid && (flags[j] & SEL_HAS_START));
            const uint32_t last = stop ? (uint32_t)__builtin_ctzll(stop) : 63u;
            back = min(back, sel_wave_min(valid && lane <= last ? trail[j] : SEL_NONE));
            if (stop) break;
        }
    }
    // and of the group the trailing piece belongs to: the leading pieces of the wavefronts after this one, up to the first
    // one in which a group starts (its leading piece is empty if that is at its lane 0)
    for (uint64_t base = w + 1; base < n_waves; base += 64) {
        const uint64_t j = base + lane;
        const bool valid = j < n_waves;
        const uint64_t stop = __ballot(valid && (flags[j] & SEL_HAS_START));
        const uint32_t last = stop ? (uint32_t)__builtin_ctzll(stop) : 63u;
        fwd = min(fwd, sel_wave_min(valid && lane <= last ? lead[j] : SEL_NONE));
        if (stop) break;
    }
    if (i >= n) return;
    uint64_t best = s.piece;
    if (s.leading) best = min(best, back);
    if (s.trailing) best = min(best, fwd);
    const bool eligible = s.mine != SEL_NONE, winner = eligible && s.mine == best;
    if (eligible && !winner) {
        n_runs[i] = 0u;
        status[i] = (uint32_t)LANE_STATUS_NOT_BEST;
    }
    if (is_best) is_best[i] = winner ? 1 : 0;
}

size_t select_scratch_bytes(uint64_t n) { return (size_t)((n + 63) / 64) * 20 + 64; }

hipError_t launch_select_best(uint64_t n, const uint32_t* key, uint32_t key_mask, const int64_t* ed, uint32_t* status, uint32_t* n_runs,
                              uint8_t* is_best, void* scratch, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint64_t n_waves = (n + 63) / 64;
    uint64_t* const lead = static_cast<uint64_t*>(scratch);
    uint64_t* const trail = lead + n_waves;
    uint32_t* const flags = reinterpret_cast<uint32_t*>(trail + n_waves);
    const dim3 grid((unsigned)((n_waves + 3) / 4)), block(256);
    hipLaunchKernelGGL(select_summary_kernel, grid, block, 0, s, n, key, key_mask, ed, (const uint32_t*)status, n_waves, lead, trail, flags);
    hipLaunchKernelGGL(select_mark_kernel, grid, block, 0, s, n, key, key_mask, ed, status, n_runs, is_best, n_waves, (const uint64_t*)lead,
                       (const uint64_t*)trail, (const uint32_t*)flags);
    return hipGetLastError();
}

}  // namespace scrg
