// pileup_kernels.hip — the pileup (include/scrooge_amd.h: PILEUP): what the alignments of a batch say at every position of a
// target — '=' columns, 'X' columns by read base, 'D' columns and insertion events — summed over pairs into seven planes of
// target_len + 1 counters (scrg_pileup_add), and the pass that turns the two planes kept in edge form into counts
// (scrg_pileup_finish).  The first pass over run_walk.h that sums over pairs instead of writing per pair.
//
// pileup_add_kernel: one pair per lane up to WALK_LANE_MAX_RUNS runs, one wavefront per pair above that in tiles of 512 runs, eight
// per lane; the text and read positions in front of a lane's runs and the operation of the run before come from the shared tile
// step, so every lane decides alone whether its run begins or ends a stretch and whether its 'I' run is a new insertion, at the
// lane seam and the tile seam alike (pileup_rule.h, shared with the host twin).  The text is never read; the read only under 'X'.
//
// MATCH and DEL are kept in EDGE FORM while pairs are added: +1 at the first position of a stretch of '=' (or 'D') columns, -1
// (0xffffffff: sums wrap mod 2^32) one past its last, both clamped to target_len.  Directly adjacent runs of one operation — the
// 29= 21= of a window seam — are one stretch: the edges between them would cancel and are not issued.  A 10 kb read then costs
// two atomics per stretch instead of one per base; 'X' columns and insertion events are single adds.  All adds are plain device-scope
// atomicAdd on uint32_t whose result is not used.  (Edge form against one add per column has not been measured on this chip.)
//
// pileup_finish: the inclusive prefix sum of planes 0 and 5 mod 2^32, reduce-then-scan in three launches — per-tile sums, ONE
// workgroup per plane that scans the tile sums in a loop with a carry (any length, no recursion), per-tile scan plus offset.  No
// workgroup waits for another inside a kernel.  Every +1 has its -1 at or before slot target_len, so that slot ends as 0.
#include "block_scan.h"
#include "genasm_kernels.h"
#include "host_path.h"
#include "pileup_rule.h"
#include "run_walk.h"

namespace scrg {

struct PileArgs {
    PairRuns pr;
    const uint32_t* status;       // may be null
    const uint64_t* start;        // [n] target_start
    uint64_t len;                 // target_len: planes of len + 1 words
    uint32_t* acc;                // [PILE_PLANES][len + 1]
    uint32_t* outside;            // may be null: += pairs with a column or an insertion outside the target
    uint32_t* counted;            // may be null: += pairs that were counted
};

struct PilePair {                 // a pair as the kernel takes it
    uint64_t cnt, src;            // runs (0: not counted), first run
    uint64_t start;
    PairSeq sq;
    uint32_t counted, outside;    // (its lane) what the pair adds to the two counters
};

__device__ __forceinline__ void load_pair(PilePair& d, const PileArgs& a, uint64_t p, uint32_t sub)
{
    run_slice(a.pr.run_off, a.pr.run_off_stride, a.pr.n_runs, p, d.cnt, d.src);
    d.sq = pair_seq(a.pr, a.pr.pairs[p]);
    d.start = a.start[p];
    const uint32_t st = a.status ? a.status[p] : (uint32_t)LANE_STATUS_DONE;
    // (a flagged read in a call that does not honour the flag: its bases are not where the flag says — nothing of it is counted)
    if (st != LANE_STATUS_DONE || (d.sq.read_rev && !a.pr.stranded)) d.cnt = 0;
    d.counted = d.cnt != 0 && sub == 0;
    d.outside = 0;
}

// the only writes of the pass: position `pos` <= len of a plane
__device__ __forceinline__ void pile_add(const PileArgs& a, uint32_t plane, uint64_t pos, uint32_t v)
{
    atomicAdd(a.acc + (uint64_t)plane * (a.len + 1ull) + pos, v);
}
__device__ __forceinline__ void pile_edge(const PileArgs& a, uint32_t plane, uint64_t g, uint32_t v)
{
    pile_add(a, plane, g < a.len ? g : a.len, v);
}

// one run with text position t and read position q in front of it, behind a run of `prev`; returns whether something of it lies
// outside the target.  (A run that is no run: a zero count adds nothing or edges that cancel, another operation nothing.)
__device__ __forceinline__ bool pile_run(const PileArgs& a, const PilePair& d, uint32_t run, uint32_t prev, uint64_t t, uint64_t q)
{
    const uint32_t c = run & 0xffu, op = run >> 8;
    const uint64_t g = pile_pos(d.start, t);
    if (pile_closes(op, prev)) pile_edge(a, pile_stretch_plane(prev), g, 0xffffffffu);
    if (pile_opens(op, prev)) pile_edge(a, pile_stretch_plane(op), g, 1u);
    if (pile_stretch_op(op)) return pile_columns_outside(g, c, a.len);
    if (op == 'X') {
        for (uint32_t k = 0; k < c; k++) {
            if (g >= a.len || a.len - g <= k || q + k >= d.sq.read_len) break;
            pile_add(a, PILE_BASE + read_code(d.sq, q + k), g + k, 1u);
        }
        return pile_columns_outside(g, c, a.len);
    }
    if (pile_ins_event(op, prev)) {
        if (pile_ins_outside(g, a.len)) return true;
        pile_add(a, PILE_INS, g, 1u);
    }
    return false;
}
// behind the pair's last run
__device__ __forceinline__ void pile_end(const PileArgs& a, const PilePair& d, uint32_t prev, uint64_t t)
{
    if (pile_closes(0u, prev)) pile_edge(a, pile_stretch_plane(prev), pile_pos(d.start, t), 0xffffffffu);
}
// what a run consumes, as the tile step sums it (run_walk.h: load_tile)
__device__ __forceinline__ void step_past(uint32_t run, uint64_t& t, uint64_t& q, uint32_t& prev)
{
    const uint32_t c = run & 0xffu, op = run >> 8;
    if (op == '=' || op == 'X' || op == 'D') t += c;
    if (op == '=' || op == 'X' || op == 'I') q += c;
    prev = op;
}

// one pair per lane: a serial walk
__device__ __forceinline__ bool walk_lane(const PileArgs& a, const PilePair& d)
{
    const uint16_t* const s = a.pr.runs + d.src;
    uint64_t t = 0, q = 0;
    uint32_t prev = 0;
    bool outside = false;
    for (uint64_t k = 0; k < d.cnt; k++) {
        const uint32_t run = s[k];
        outside |= pile_run(a, d, run, prev, t, q);
        step_past(run, t, q, prev);
    }
    pile_end(a, d, prev, t);
    return outside;
}

// one wavefront per pair: tiles of 512 runs, eight per lane.  All 64 lanes call it with the same pair and all return its flag.
__device__ __forceinline__ bool walk_wave(const PileArgs& a, const PilePair& d, uint32_t lane)
{
    const uint16_t* const s = a.pr.runs + d.src;
    WalkPos carry{};                              // the state after the tiles so far (wavefront-uniform)
    bool outside = false;
    for (uint64_t t0 = 0; t0 < d.cnt; t0 += WALK_TILE_RUNS) {
        const RunTile x = load_tile(s, d.cnt, t0, lane, carry, [](uint32_t&) {});
        uint64_t t = x.at.t, q = x.at.q;
        uint32_t prev = x.at.prev;
#pragma unroll
        for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
            if (k >= x.mine) continue;
            outside |= pile_run(a, d, x.r[k], prev, t, q);
            step_past(x.r[k], t, q, prev);
        }
        move_past(carry, x);
    }
    if (lane == 0) pile_end(a, d, carry.prev, carry.t);
    return __ballot(outside) != 0ull;
}

__global__ __launch_bounds__(256) void pileup_add_kernel(PileArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    for_each_group<PilePair>(
        a.pr.n, split, [&](PilePair& me, uint64_t p, uint32_t sub) { load_pair(me, a, p, sub); },
        [&](PilePair& me, uint64_t) {
            if (me.cnt) me.outside = walk_lane(a, me);
        },
        [&](PilePair& me, uint64_t g0, uint32_t q, uint32_t lane) {
            PilePair dq;
            load_pair(dq, a, g0 + q, 0u);
            const bool outside = walk_wave(a, dq, lane);
            if (lane == q) me.outside = outside;
        },
        [&](const PilePair& me, uint32_t lane) {
            const uint32_t n_out = (uint32_t)__popcll(__ballot(me.outside != 0u)), n_cnt = (uint32_t)__popcll(__ballot(me.counted != 0u));
            if (a.outside && n_out && lane == 0) atomicAdd(a.outside, n_out);
            if (a.counted && n_cnt && lane == 0) atomicAdd(a.counted, n_cnt);
        });
}

hipError_t launch_pileup_add(const PairRuns& pr, const uint32_t* status, const uint64_t* target_start, uint64_t target_len, uint32_t* acc,
                             uint32_t* outside, uint32_t* counted, int n_cus, hipStream_t s)
{
    if (pr.n == 0) return hipSuccess;
    PileArgs a{};
    a.pr = pr;
    a.status = status;
    a.start = target_start;
    a.len = target_len;
    a.acc = acc;
    a.outside = outside;
    a.counted = counted;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(pr.n, n_cus, &split);
    hipLaunchKernelGGL(pileup_add_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// pileup_finish: edge form -> counts for planes 0 and 5
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t SCAN_PER_THREAD = 4, SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD;      // 4096 positions per workgroup

__device__ __forceinline__ uint32_t scan_plane(uint32_t y) { return y ? PILE_DEL : PILE_MATCH; }

// 1: the sum of every tile of both planes -> sums[y * n_tiles + tile]
__global__ __launch_bounds__(SCAN_THREADS) void pileup_tile_sums_kernel(const uint32_t* __restrict__ acc, uint64_t n, uint64_t n_tiles, uint32_t* __restrict__ sums)
{
    __shared__ uint32_t wave_tot[SCAN_THREADS / 64u];
    const uint32_t* const src = acc + (uint64_t)scan_plane(blockIdx.y) * n;
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_PER_THREAD;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER_THREAD; k++)
        if (i0 + k < n) v += src[i0 + k];
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0u) wave_tot[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < SCAN_THREADS / 64u; w++) all += wave_tot[w];
        sums[(uint64_t)blockIdx.y * n_tiles + blockIdx.x] = all;
    }
}

// 2: one workgroup per plane: the tile sums become what lies in front of every tile, SCAN_THREADS of them per round with a carry
__global__ __launch_bounds__(SCAN_THREADS) void pileup_scan_sums_kernel(uint32_t* __restrict__ sums, uint64_t n_tiles)
{
    __shared__ uint32_t wave_tot[SCAN_THREADS / 64u];
    block_scan_excl_in_place(sums + (uint64_t)blockIdx.x * n_tiles, n_tiles, wave_tot);
}

// 3: every tile's inclusive scan plus what lies in front of it.  (dst may be src: a workgroup has read its tile before it writes.)
__global__ __launch_bounds__(SCAN_THREADS) void pileup_tile_scan_kernel(const uint32_t* acc, uint64_t n, uint64_t n_tiles, const uint32_t* __restrict__ sums,
                                                                         uint32_t* counts)
{
    __shared__ uint32_t wave_tot[SCAN_THREADS / 64u];
    const uint32_t* const src = acc + (uint64_t)scan_plane(blockIdx.y) * n;
    uint32_t* const dst = counts + (uint64_t)scan_plane(blockIdx.y) * n;
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_PER_THREAD;
    uint32_t x[SCAN_PER_THREAD];
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER_THREAD; k++) {
        x[k] = i0 + k < n ? src[i0 + k] : 0u;
        v += x[k];
    }
    uint32_t total;
    uint32_t run = block_scan_incl(v, wave_tot, &total) - v + sums[(uint64_t)blockIdx.y * n_tiles + blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < SCAN_PER_THREAD; k++) {
        run += x[k];
        if (i0 + k < n) dst[i0 + k] = run;
    }
}

size_t pileup_finish_scratch_bytes(uint64_t target_len)
{
    const uint64_t n_tiles = (target_len + 1ull + SCAN_TILE - 1ull) / SCAN_TILE;
    return (size_t)(2ull * n_tiles * sizeof(uint32_t));
}

hipError_t launch_pileup_finish(uint64_t target_len, const uint32_t* acc, uint32_t* counts, void* scratch, hipStream_t s)
{
    const uint64_t n = target_len + 1ull, n_tiles = (n + SCAN_TILE - 1ull) / SCAN_TILE;
    if (n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
    if (counts != acc) {                          // the planes that are counts already: A, C, G, T side by side, INS
        hipError_t e = hipMemcpyAsync(counts + PILE_BASE * n, acc + PILE_BASE * n, 4ull * n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(counts + PILE_INS * n, acc + PILE_INS * n, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    uint32_t* const sums = static_cast<uint32_t*>(scratch);
    hipLaunchKernelGGL(pileup_tile_sums_kernel, dim3((unsigned)n_tiles, 2), dim3(SCAN_THREADS), 0, s, acc, n, n_tiles, sums);
    hipLaunchKernelGGL(pileup_scan_sums_kernel, dim3(2), dim3(SCAN_THREADS), 0, s, sums, n_tiles);
    hipLaunchKernelGGL(pileup_tile_scan_kernel, dim3((unsigned)n_tiles, 2), dim3(SCAN_THREADS), 0, s, acc, n, n_tiles, sums, counts);
    return hipGetLastError();
}

}  // namespace scrg
