// run_walk.h — what the per-pair output passes share: the CIGAR text (host_path_kernels.hip), the difference strings
// (diff_kernels.hip) and the alignment report (report_kernels.hip) all walk every pair's list of runs once per kernel.
//
// Pairs are taken 64 at a time by a wavefront (for_each_group).  A pair of up to WALK_LANE_MAX_RUNS runs is walked serially by
// its own lane; the longer pairs of the group get the whole wavefront one after the other, in tiles of WALK_TILE_RUNS runs,
// WALK_LANE_RUNS per lane (load_tile): the text and read positions in front of a lane's runs come from wavefront scans, the
// operation of the run before from the lane before, and all three are carried from tile to tile.  A batch of few pairs lets
// `split` wavefronts share a group (group_grid): each takes every split-th long pair of it.
//
// A pass supplies: the record a lane loads for its pair (it has the run count as `cnt`), the serial walk of one pair, the
// wavefront walk of one pair, and what it does per run; the geometry, the hand-out of the long pairs, the run loading, the
// scans, the base codes and the staged copy of a tile's bytes come from here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "genasm_kernels.h"
#include "host_path.h"
#include "launch_grid.h"

namespace scrg {

// the thresholds the tests name (tests/test_diff_strings.py, test_pair_report_gpu.py, test_cigar_text_gpu.py walk both neighbours
// of each; tests/test_walk_geometry_gpu.py lays them into batches of every `split` and of more than one trip of the group loop,
// tests/test_walk_geometry.py holds the sizes of those batches to launch_grid.h)
constexpr uint32_t WALK_LANE_MAX_RUNS = 24;       // up to this many runs: one pair per lane; more: one wavefront per pair
constexpr uint32_t WALK_LANE_RUNS = 8;            // runs per lane and tile
constexpr uint32_t WALK_TILE_RUNS = 64 * WALK_LANE_RUNS;       // 512

// (the grid of these kernels — group_grid: workgroups of four wavefronts, `split` wavefronts per group of 64 pairs — is in
// launch_grid.h)

// ---------------------------------------------------------------------------------------------------------------
// wavefront helpers
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= (uint32_t)d) v += u;
    }
    return v;
}
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// a tile's bytes, which the lanes have written to LDS, leave as contiguous bytes
__device__ __forceinline__ void flush_tile(uint8_t* dst, const uint8_t* tile, uint32_t bytes, uint32_t lane)
{
    wave_sync();
    for (uint32_t b = lane; b < bytes; b += 64) dst[b] = tile[b];
    wave_sync();
}

// ---------------------------------------------------------------------------------------------------------------
// The group driver.  Rec: what a lane holds of its pair for the time of a group, value-initialised; Rec::cnt is the pair's run
// count (0: nothing for the wavefront form).
//   load(rec, p, sub)            the lane's own pair p < n
//   on_lane(rec, p)              the serial walk of p (cnt <= WALK_LANE_MAX_RUNS), by the first wavefront of a group only
//   on_wave(rec, g0, q, lane)    all 64 lanes: the walk of pair g0 + q, which is lane q's — rec is still the lane's OWN record,
//                                what the wavefront needs of lane q's it takes by __shfl or loads again
//   after(rec, lane)             all 64 lanes, once per group
// ---------------------------------------------------------------------------------------------------------------
template <class Rec, class Load, class OnLane, class OnWave, class After>
__device__ __forceinline__ void for_each_group(uint64_t n, uint32_t split, Load load, OnLane on_lane, OnWave on_wave, After after)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave_all = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t wave = wave_all / split, n_waves = (((uint64_t)gridDim.x * blockDim.x) >> 6) / split;
    const uint32_t sub = (uint32_t)(wave_all % split);
    if (wave >= n_waves) return;                       // (the grid is rounded up to whole workgroups)
    for (uint64_t g0 = wave * 64; g0 < n; g0 += n_waves * 64) {
        const uint64_t mine = g0 + lane;
        Rec rec{};
        if (mine < n) load(rec, mine, sub);
        const bool big_me = rec.cnt > WALK_LANE_MAX_RUNS;
        if (mine < n && sub == 0 && !big_me) on_lane(rec, mine);
        uint64_t big = __ballot(big_me);
        for (uint32_t ord = 0; big != 0; ord++) {
            const uint32_t q = (uint32_t)__builtin_ctzll(big);
            big &= big - 1;
            if (ord % split != sub) continue;
            on_wave(rec, g0, q, lane);
        }
        after(rec, lane);
    }
}
struct NothingAfter {
    template <class Rec> __device__ __forceinline__ void operator()(const Rec&, uint32_t) const {}
};

// ---------------------------------------------------------------------------------------------------------------
// a pair's runs and sequences
// ---------------------------------------------------------------------------------------------------------------
// Pair p's runs: runs[src + k], k < cnt.  (Stride 6: the slices as scrg_align_device left them — the offsets are the
// descriptors' cigar_off, the count is capped at cigar_cap.)
__device__ __forceinline__ void run_slice(const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs, uint64_t p,
                                          uint64_t& cnt, uint64_t& src)
{
    cnt = n_runs[p];
    src = run_off[p * run_off_stride];
    if (run_off_stride == 6) cnt = cnt > run_off[p * 6 + 1] ? run_off[p * 6 + 1] : cnt;
}

struct PairSeq {                  // where a pair's bases are, and how many (the strand bits taken out of the offsets)
    const uint64_t* seq;
    uint64_t text_off, read_off;
    uint64_t text_len, read_len;
    uint32_t text_stride, read_stride;
    bool text_rev, read_rev;
};
__device__ __forceinline__ PairSeq pair_seq(const PairRuns& a, const scrg_pair_desc& pd)
{
    PairSeq s;
    s.seq = a.seq;
    s.text_off = pd.text_off & ~SCRG_TEXT_REVCOMP;
    s.text_len = pd.text_len;
    s.text_rev = (pd.text_off & SCRG_TEXT_REVCOMP) != 0;
    s.read_off = pd.read_off & ~SCRG_READ_REVCOMP;
    s.read_len = pd.read_len;
    s.read_rev = (pd.read_off & SCRG_READ_REVCOMP) != 0;
    s.text_stride = a.text_stride;
    s.read_stride = a.read_stride;
    return s;
}

// base k of a sequence with offset `off` and word stride s: word off / 32 + ((off % 32 + k) / 32) * s, bit (off + k) % 32 of each plane
__device__ __forceinline__ uint32_t base_code(const uint64_t* __restrict__ seq, uint64_t off, uint32_t stride, uint64_t k)
{
    const uint64_t pos = (off & 31ull) + k;
    const uint64_t w = seq[(off >> 5) + (pos >> 5) * stride];
    const uint32_t b = (uint32_t)pos & 31u;
    return (uint32_t)((w >> b) & 1ull) | ((uint32_t)((w >> (32u + b)) & 1ull) << 1);
}
// character k of the sequence AS ALIGNED: of a reversed sequence of `len` bases the complement of base len - 1 - k (A0 C1 G2 T3)
__device__ __forceinline__ uint32_t code_aligned(const uint64_t* __restrict__ seq, uint64_t off, uint32_t stride, uint64_t len, bool rev, uint64_t k)
{
    const uint32_t c = base_code(seq, off, stride, rev ? len - 1ull - k : k);
    return rev ? 3u - c : c;
}
__device__ __forceinline__ uint32_t text_code(const PairSeq& s, uint64_t t) { return code_aligned(s.seq, s.text_off, s.text_stride, s.text_len, s.text_rev, t); }
__device__ __forceinline__ uint32_t read_code(const PairSeq& s, uint64_t q) { return code_aligned(s.seq, s.read_off, s.read_stride, s.read_len, s.read_rev, q); }

// ---------------------------------------------------------------------------------------------------------------
// The tile step of the wavefront form: tile t0 / WALK_TILE_RUNS of a pair, lane L holds its runs 8 L .. 8 L + 7.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool run_ok(uint32_t run)
{
    const uint32_t op = run >> 8;
    return (run & 0xffu) != 0u && (op == '=' || op == 'X' || op == 'I' || op == 'D');
}

// my eight runs of the tile (the dense array is only 2-byte aligned: plain loads; 0 past the pair's last run); returns how many
// of them the pair has — r[0 .. mine).  (For a pass that needs no positions; load_tile loads and sums in one loop.)
__device__ __forceinline__ uint32_t load_lane_runs(const uint16_t* __restrict__ s, uint64_t cnt, uint64_t t0, uint32_t lane, uint32_t (&r)[WALK_LANE_RUNS])
{
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
        const uint64_t idx = t0 + WALK_LANE_RUNS * lane + k;
        r[k] = idx < cnt ? s[idx] : 0u;
        if (idx < cnt) mine = k + 1;
    }
    return mine;
}

struct WalkPos {
    uint64_t t, q;                // text and read positions
    uint32_t prev;                // the operation of the run before (0: none)
};
struct RunTile {
    uint32_t r[WALK_LANE_RUNS];   // my runs
    uint32_t mine;                // r[0 .. mine) exist
    WalkPos at;                   // in front of my first run
    uint32_t end_t, end_q, end_op;        // what the whole tile consumes, its last operation (wavefront-uniform)
};
// the carry of the next tile
__device__ __forceinline__ void move_past(WalkPos& carry, const RunTile& x)
{
    carry.t += x.end_t;
    carry.q += x.end_q;
    carry.prev = x.end_op;
}
// `carry`: the state after the tiles so far.  per_run(run): the pass's own look at every run of mine, in order, in the one loop
// that loads and sums them; it may replace the run.  A run that is no run (a zero count, another operation) consumes nothing:
// whoever meets one gives the pair up, and behind it `at`, `end_*` and the carry are of no interest and not specified.
template <class PerRun>
__device__ __forceinline__ RunTile load_tile(const uint16_t* __restrict__ s, uint64_t cnt, uint64_t t0, uint32_t lane, const WalkPos& carry, PerRun per_run)
{
    RunTile x;
    x.mine = 0;
    uint32_t sum_t = 0, sum_q = 0, last_op = 0;
    // (the dense array is only 2-byte aligned: plain loads)
#pragma unroll
    for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
        const uint64_t idx = t0 + WALK_LANE_RUNS * lane + k;
        x.r[k] = idx < cnt ? s[idx] : 0u;
        if (idx >= cnt) continue;
        x.mine = k + 1;
        per_run(x.r[k]);
        const uint32_t c = x.r[k] & 0xffu, op = x.r[k] >> 8;
        if (op == '=' || op == 'X' || op == 'D') sum_t += c;
        if (op == '=' || op == 'X' || op == 'I') sum_q += c;
        last_op = op;
    }
    uint32_t in_t = sum_t, in_q = sum_q;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t vt = (uint32_t)__shfl_up((int)in_t, d, 64), vq = (uint32_t)__shfl_up((int)in_q, d, 64);
        if (lane >= (uint32_t)d) {
            in_t += vt;
            in_q += vq;
        }
    }
    // exclusive: what the lanes before me leave
    x.at.t = carry.t + (in_t - sum_t);
    x.at.q = carry.q + (in_q - sum_q);
    x.at.prev = (uint32_t)__shfl_up((int)last_op, 1, 64);
    if (lane == 0) x.at.prev = carry.prev;
    // the tile's state after its last lane
    const uint32_t runs_here = (uint32_t)(cnt - t0 < WALK_TILE_RUNS ? cnt - t0 : WALK_TILE_RUNS);
    x.end_t = (uint32_t)__shfl((int)in_t, 63, 64);
    x.end_q = (uint32_t)__shfl((int)in_q, 63, 64);
    x.end_op = (uint32_t)__shfl((int)last_op, (int)((runs_here - 1u) / WALK_LANE_RUNS), 64);
    return x;
}

}  // namespace scrg
