// clip_kernels.hip — soft clipping (scrg_pair_clip, include/scrooge_amd.h: SOFT CLIPPING): per pair the stretch of whole runs, from
// an '=' run to an '=' run, with the best affine score — where it lies in the read and in the text, which runs it is, its score and
// its edits.  One pass over the finished runs on run_walk.h: one pair per lane up to WALK_LANE_MAX_RUNS runs, one wavefront per pair
// above that in tiles of 512 runs, eight per lane.  No sequence is read: the score of a stretch is a function of the runs alone.
//
// With P_k the prefix score in front of run k, the stretch i .. j scores P_{j+1} - P_i.  For every end j the start is the earliest
// '=' run i <= j with the least P_i; the result is the latest j of the best score.  In the wavefront form a lane knows P in front
// of its own eight runs from a scan of the lanes' sums (the gap-open term of a lane's first run from the operation of the run
// before: RunTile::at.prev), the best start at or before each of its runs from a prefix minimum over (P_i, i) keys — the earliest
// wins a tie, the tiles before through the carry — and the tile's best end from a maximum over (score, j) keys, the latest
// winning.  Only the indices travel through the scans: where a chosen start or end lies in the read and the text is walked again
// by the lane that holds it and broadcast, three times per tile at the most.
//
// Apply mode is a second launch (apply_kernel): the wavefronts that share a group of a small batch (`split`) each tell the group's
// long pairs from its short ones by the run counts, so nothing may rewrite a count while the walk is in flight.  The walk marks the
// record of a pair it looked at and kept nothing of (CLIP_KEEPS_NOTHING in first_run), the second launch makes the kept stretch the
// pair's alignment — the count, the offset, the capacity behind a descriptor's offset — and clears the mark.
#include "genasm_kernels.h"
#include "host_path.h"
#include "run_walk.h"

namespace scrg {

constexpr uint32_t CLIP_KEEPS_NOTHING = 0xffffffffu;      // (between the two launches of apply mode only)

struct ClipCosts {
    int32_t match, mismatch, gap_open, gap_extend;
};
struct ClipArgs {
    uint64_t n;
    const uint16_t* runs;
    const uint64_t* run_off;
    uint64_t run_off_stride;
    const uint32_t* n_runs;
    const uint32_t* status;       // may be null
    ClipCosts costs;
    uint32_t mark;                // apply mode: first_run of a walked pair that keeps nothing
    scrg_pair_clip* clip;
};

struct ClipPair {                 // a pair as the kernel takes it
    uint64_t cnt, src;            // runs, first run
    bool walked;                  // its status says it has an alignment
};
__device__ __forceinline__ void load_pair(ClipPair& d, const ClipArgs& a, uint64_t p)
{
    run_slice(a.run_off, a.run_off_stride, a.n_runs, p, d.cnt, d.src);
    d.walked = !a.status || a.status[p] == (uint32_t)LANE_STATUS_DONE;
    if (!d.walked) d.cnt = 0;
}

// what run k adds to the prefix score (prev: the operation of the run before, 0: none)
__device__ __forceinline__ int32_t run_weight(const ClipCosts& c, uint32_t run, uint32_t prev)
{
    const int32_t n = (int32_t)(run & 0xffu);
    const uint32_t op = run >> 8;
    if (op == '=') return c.match * n;
    if (op == 'X') return -c.mismatch * n;
    return -(c.gap_extend * n + (prev == 'I' || prev == 'D' ? 0 : c.gap_open));
}

struct Cut {                      // in front of a run: text and read position, bases under X, I, D so far
    uint32_t t, q, e;
};
__device__ __forceinline__ void move_cut(Cut& c, uint32_t run)
{
    const uint32_t n = run & 0xffu, op = run >> 8;
    if (op != 'I') c.t += n;
    if (op != 'D') c.q += n;
    if (op != '=') c.e += n;
}

__device__ __forceinline__ scrg_pair_clip keeps_nothing(uint32_t mark)
{
    scrg_pair_clip r{};
    r.first_run = mark;
    return r;
}
__device__ __forceinline__ scrg_pair_clip kept(int32_t score, uint32_t i, uint32_t j, const Cut& from, const Cut& to)
{
    scrg_pair_clip r;
    r.read_start = from.q;
    r.read_end = to.q;
    r.text_start = from.t;
    r.text_end = to.t;
    r.first_run = i;
    r.n_runs = j - i + 1u;
    r.score = score;
    r.n_edits = to.e - from.e;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
// one pair per lane: a serial walk
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ scrg_pair_clip walk_lane(const ClipPair& d, const ClipArgs& a)
{
    if (!d.walked) return keeps_nothing(0u);
    const uint16_t* const s = a.runs + d.src;
    Cut at{0u, 0u, 0u}, low_at{}, from{}, to{};
    int32_t P = 0, low = INT32_MAX, best = 0;             // the prefix score, the least in front of an '=' run, the best stretch
    uint32_t low_run = 0, best_i = 0, best_j = 0, prev = 0;
    for (uint64_t k = 0; k < d.cnt; k++) {
        const uint32_t run = s[k], op = run >> 8;
        if (!run_ok(run)) return keeps_nothing(0u);
        if (op == '=' && P < low) {                       // (the earliest of equal starts stays)
            low = P;
            low_run = (uint32_t)k;
            low_at = at;
        }
        P += run_weight(a.costs, run, prev);
        move_cut(at, run);
        prev = op;
        if (op == '=' && P - low >= best) {               // (the latest of equal ends wins)
            best = P - low;
            best_i = low_run;
            best_j = (uint32_t)k;
            from = low_at;
            to = at;
        }
    }
    return best > 0 ? kept(best, best_i, best_j, from, to) : keeps_nothing(a.mark);
}

// ---------------------------------------------------------------------------------------------------------------
// one wavefront per pair: tiles of 512 runs, eight per lane.  All 64 lanes call it with the same pair (which is walked) and all
// return its record.
// ---------------------------------------------------------------------------------------------------------------
// (P_i, i) of a start, ordered by the score and then by the run; none: all ones
__device__ __forceinline__ uint64_t start_key(int32_t P, uint32_t run) { return ((uint64_t)((uint32_t)P ^ 0x80000000u) << 32) | run; }
__device__ __forceinline__ int32_t start_score(uint64_t key) { return (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u); }
constexpr uint64_t NO_START = ~0ull;

__device__ __forceinline__ uint64_t wave_scan_min(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = __shfl_up((unsigned long long)v, d, 64);
        if (lane >= (uint32_t)d && u < v) v = u;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t u = __shfl_xor((unsigned long long)v, d, 64);
        if (u > v) v = u;
    }
    return v;
}
// the cut in front of run `k` (0 .. 8: 8 = behind the last) of lane `owner`, in all lanes
__device__ __forceinline__ Cut cut_of(const RunTile& x, uint32_t e0, uint32_t k, uint32_t owner)
{
    Cut c{(uint32_t)x.at.t, (uint32_t)x.at.q, e0};
#pragma unroll
    for (uint32_t m = 0; m < WALK_LANE_RUNS; m++) {
        if (m < k && m < x.mine) move_cut(c, x.r[m]);
    }
    c.t = (uint32_t)__shfl((int)c.t, (int)owner, 64);
    c.q = (uint32_t)__shfl((int)c.q, (int)owner, 64);
    c.e = (uint32_t)__shfl((int)c.e, (int)owner, 64);
    return c;
}

__device__ __forceinline__ scrg_pair_clip walk_wave(const ClipPair& d, const ClipArgs& a, uint32_t lane)
{
    const uint16_t* const s = a.runs + d.src;
    // the state after the tiles so far (wavefront-uniform): positions and last operation, prefix score, edits, the least start
    // and where it lies, the best stretch
    WalkPos carry{};
    int32_t carry_P = 0;
    uint32_t carry_e = 0;
    uint64_t low_key = NO_START, best_key = 0;            // best: score << 32 | j, 0: none yet
    uint32_t best_i = 0;
    Cut low_at{}, from{}, to{};
    for (uint64_t t0 = 0; t0 < d.cnt; t0 += WALK_TILE_RUNS) {
        bool bad = false;
        const RunTile x = load_tile(s, d.cnt, t0, lane, carry, [&](uint32_t& run) { bad |= !run_ok(run); });
        if (__ballot(bad)) return keeps_nothing(0u);      // (a run that is no run: the pair is given up)
        const uint32_t run0 = (uint32_t)t0 + WALK_LANE_RUNS * lane;
        // my runs' weights, and what my runs add to the score and to the edits
        int32_t w[WALK_LANE_RUNS], lane_w = 0;
        uint32_t lane_e = 0, prev = x.at.prev;
#pragma unroll
        for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
            w[k] = 0;
            if (k >= x.mine) continue;
            w[k] = run_weight(a.costs, x.r[k], prev);
            lane_w += w[k];
            prev = x.r[k] >> 8;
            if (prev != '=') lane_e += x.r[k] & 0xffu;
        }
        const uint32_t in_w = wave_scan_incl((uint32_t)lane_w, lane), in_e = wave_scan_incl(lane_e, lane);
        const int32_t P0 = carry_P + (int32_t)(in_w - (uint32_t)lane_w);      // in front of my first run
        const uint32_t e0 = carry_e + (in_e - lane_e);
        // the least start among my runs; the least at or before the lane before me, the tiles before included
        uint64_t mine_low = NO_START;
        int32_t P = P0;
#pragma unroll
        for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
            if (k < x.mine && (x.r[k] >> 8) == '=') {
                const uint64_t key = start_key(P, run0 + k);
                if (key < mine_low) mine_low = key;
            }
            P += w[k];
        }
        const uint64_t in_low = wave_scan_min(mine_low, lane);
        uint64_t cur = __shfl_up((unsigned long long)in_low, 1, 64);
        if (lane == 0 || low_key < cur) cur = low_key;
        // my best end: score << 32 | j, and its start
        uint64_t mine_best = 0;
        uint32_t mine_i = 0;
        P = P0;
#pragma unroll
        for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
            const bool match = k < x.mine && (x.r[k] >> 8) == '=';
            if (match) {
                const uint64_t key = start_key(P, run0 + k);
                if (key < cur) cur = key;
            }
            P += w[k];
            if (match) {
                const uint64_t key = ((uint64_t)(uint32_t)(P - start_score(cur)) << 32) | (run0 + k);
                if (key > mine_best) {
                    mine_best = key;
                    mine_i = (uint32_t)cur;
                }
            }
        }
        // the tile's: a later end of the same score has the greater key, in the tile and against the tiles before
        const uint64_t tile_best = wave_max(mine_best);
        if (tile_best > best_key) {
            const uint32_t j = (uint32_t)tile_best - (uint32_t)t0;
            const uint32_t i = (uint32_t)__shfl((int)mine_i, (int)(j / WALK_LANE_RUNS), 64);
            to = cut_of(x, e0, j % WALK_LANE_RUNS + 1u, j / WALK_LANE_RUNS);
            from = i >= (uint32_t)t0 ? cut_of(x, e0, (i - (uint32_t)t0) % WALK_LANE_RUNS, (i - (uint32_t)t0) / WALK_LANE_RUNS) : low_at;
            best_key = tile_best;
            best_i = i;
        }
        const uint64_t tile_low = __shfl((unsigned long long)in_low, 63, 64);
        if (tile_low < low_key) {
            const uint32_t i = (uint32_t)tile_low - (uint32_t)t0;
            low_at = cut_of(x, e0, i % WALK_LANE_RUNS, i / WALK_LANE_RUNS);
            low_key = tile_low;
        }
        carry_P += (int32_t)(uint32_t)__shfl((int)in_w, 63, 64);
        carry_e += (uint32_t)__shfl((int)in_e, 63, 64);
        move_past(carry, x);
    }
    return best_key ? kept((int32_t)(best_key >> 32), best_i, (uint32_t)best_key, from, to) : keeps_nothing(a.mark);
}

__device__ __forceinline__ void store_clip(scrg_pair_clip* dst, const scrg_pair_clip& r)
{
    // (a record is 32 bytes, the array 4-byte aligned as far as the interface says: eight dword stores)
    uint32_t* const o = reinterpret_cast<uint32_t*>(dst);
    o[0] = r.read_start;
    o[1] = r.read_end;
    o[2] = r.text_start;
    o[3] = r.text_end;
    o[4] = r.first_run;
    o[5] = r.n_runs;
    o[6] = (uint32_t)r.score;
    o[7] = r.n_edits;
}

__global__ __launch_bounds__(256) void clip_kernel(ClipArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    for_each_group<ClipPair>(
        a.n, split, [&](ClipPair& me, uint64_t p, uint32_t) { load_pair(me, a, p); },
        [&](ClipPair& me, uint64_t p) { store_clip(a.clip + p, walk_lane(me, a)); },
        [&](ClipPair&, uint64_t g0, uint32_t q, uint32_t lane) {
            ClipPair dq;
            load_pair(dq, a, g0 + q);
            const scrg_pair_clip r = walk_wave(dq, a, lane);
            if (lane == q) store_clip(a.clip + g0 + q, r);
        },
        NothingAfter{});
}

// apply mode's second launch, one pair per thread: the kept stretch becomes the pair's alignment
__global__ __launch_bounds__(256) void clip_apply_kernel(uint64_t n, uint64_t* run_off, uint64_t run_off_stride, uint32_t* n_runs, scrg_pair_clip* clip)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t* const rec = reinterpret_cast<uint32_t*>(clip + p);
    const uint32_t first = rec[4], count = rec[5];
    if (count) {
        n_runs[p] = count;
        run_off[p * run_off_stride] += first;
        if (run_off_stride == 6) run_off[p * 6 + 1] -= first;         // (the capacity behind a descriptor's offset)
    } else if (first == CLIP_KEEPS_NOTHING) {
        n_runs[p] = 0;
        rec[4] = 0;
    }
}

hipError_t launch_clip(uint64_t n, const uint16_t* runs, uint64_t* run_off, uint64_t run_off_stride, uint32_t* n_runs, const uint32_t* status,
                       const int32_t* costs, bool apply, scrg_pair_clip* clip, int n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    ClipArgs a{};
    a.n = n;
    a.runs = runs;
    a.run_off = run_off;
    a.run_off_stride = run_off_stride;
    a.n_runs = n_runs;
    a.status = status;
    a.costs = ClipCosts{costs[0], costs[1], costs[2], costs[3]};
    a.mark = apply ? CLIP_KEEPS_NOTHING : 0u;
    a.clip = clip;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(n, n_cus, &split);
    hipLaunchKernelGGL(clip_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    if (apply) hipLaunchKernelGGL(clip_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, run_off, run_off_stride, n_runs, clip);
    return hipGetLastError();
}

}  // namespace scrg
