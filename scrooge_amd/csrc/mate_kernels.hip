// mate_kernels.hip — paired-end selection (scrg_align_mapping_paired, scrg_select_mates): reads 2m and 2m+1 are mate pair m, and of
// their candidates the proper combination (opposite strands, the right distance apart: mate_rule.h) of least joint cost wins
// unless the two single bests beat it by more than the penalty; every other eligible candidate loses its runs (count 0) and gets
// LANE_STATUS_NOT_BEST, exactly as best-candidate mode leaves its losers (select_kernels.hip).
//
// A TEAM of G lanes (4, 8, 16, 32 or 64, one value per launch) serves one mate pair, so a wavefront serves 64 / G of them — four
// at the common 4 x 4 candidates.  The team's lanes stride over the n_a x n_b combinations and over each side's candidates, every
// lane keeping the two smallest (cost << 32 | index) it saw and their number; a butterfly over the team's lanes merges them (the
// merge is associative and commutative), after which every lane of the team holds the same three results, decides alike, and the
// lanes share the walk that clears the losers.  No atomics, no LDS in the selection, nothing crosses a wavefront: a mate pair of
// any size is one team's loop.  Teams past n_mates and lanes past their pair's work carry neutral values through the butterflies,
// which all 64 lanes execute together.
#include <algorithm>

#include "genasm_kernels.h"
#include "host_path.h"
#include "mate_rule.h"

namespace scrg {

namespace {

// lane ^ D of a 32-bit value.  D <= 8 stays inside a row of 16 lanes: DPP, no LDS crossbar.  gfx9 has quad permutes and row
// mirrors, no xor mask: D = 4 and 8 use the (half) row mirror, lane 7 - l or 15 - l, which differs from lane l ^ D only in WHICH
// lane of the other group of D it reads — and after the steps below D every lane of a group of D holds the same value.
template <int D> __device__ __forceinline__ uint32_t mate_xor32(uint32_t v)
{
    if constexpr (D == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);        // quad_perm:[1,0,3,2]
    else if constexpr (D == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm:[2,3,0,1]
    else if constexpr (D == 4) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    else if constexpr (D == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror
    else return (uint32_t)__shfl_xor((int)v, D, 64);
}
template <int D> __device__ __forceinline__ uint64_t mate_xor64(uint64_t v)
{
    return ((uint64_t)mate_xor32<D>((uint32_t)(v >> 32)) << 32) | mate_xor32<D>((uint32_t)v);
}
template <int D> __device__ __forceinline__ void mate_step(uint32_t team, MateMin2& x, MateMin2& a, MateMin2& b)
{
    if (team <= (uint32_t)D) return;             // (uniform: the team size is the launch's)
    x = mate_min2_merge(x, MateMin2{mate_xor64<D>(x.m1), mate_xor64<D>(x.m2), mate_xor32<D>(x.count)});
    a = mate_min2_merge(a, MateMin2{mate_xor64<D>(a.m1), mate_xor64<D>(a.m2), 0u});
    b = mate_min2_merge(b, MateMin2{mate_xor64<D>(b.m1), mate_xor64<D>(b.m2), 0u});
}

struct MateArgs {
    MateRule rule;
    uint64_t n_mates;
    const uint64_t* first;        // [2 n_mates + 1]
    const uint64_t* start;
    const uint32_t* read_len;
    const uint8_t* reverse;       // may be null: all forward
    const int64_t* ed;
    uint32_t* status;
    uint32_t* n_runs;
    uint8_t* is_best;             // may be null
    scrg_mate_record* records;
    const uint32_t* team_word;    // null: `team`; else the team size mate_team_kernel left
    uint32_t team;
};

}  // namespace

// The team size for a batch whose candidate counts only the device knows (scrg_select_mates): the smallest of 4 .. 64 that is at
// least the largest min(n_a x n_b, 64).  *team_word starts at 0 (a memset in front); every wavefront adds its own with one atomic
// max.  24 bytes read per mate pair, two of three from the neighbour's lines.
__global__ __launch_bounds__(256) void mate_team_kernel(uint64_t n_mates, const uint64_t* __restrict__ first, uint32_t* __restrict__ team_word)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    uint32_t most = 1;
    for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < n_mates; m += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t f0 = first[2 * m], f1 = first[2 * m + 1], f2 = first[2 * m + 2];
        const uint64_t n_a = f1 - f0, n_b = f2 - f1;
        const uint64_t comb = n_a >= 64 || n_b >= 64 ? (n_a && n_b ? 64 : 0) : n_a * n_b;
        most = max(most, (uint32_t)min(comb, (uint64_t)64));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, d, 64));
    if ((threadIdx.x & 63u) == 0) {
        uint32_t team = 4;
        while (team < most) team <<= 1;
        atomicMax(team_word, team);
    }
}

__global__ __launch_bounds__(256) void mate_select_kernel(const MateArgs k)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    const uint32_t team = k.team_word ? *k.team_word : k.team;
    const uint32_t lane = threadIdx.x & 63u, t = lane & (team - 1u);
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t per_wave = 64u / team;
    if (wave * per_wave >= k.n_mates) return;                     // (a whole wavefront: launches sized for teams of 64 have spare ones)
    const uint64_t m = wave * per_wave + lane / team;
    const bool live = m < k.n_mates;
    uint64_t fa = 0, fb = 0, n_a = 0, n_b = 0;
    if (live) {
        fa = k.first[2 * m];
        fb = k.first[2 * m + 1];
        const uint64_t end = k.first[2 * m + 2];
        if (fa <= fb && fb <= end) {                              // (offsets that run backwards name no candidates: nothing is read)
            n_a = fb - fa;
            n_b = end - fb;
        }
    }
    // (a pair with 2^32 combinations or more has no index for them: it is served unpaired, as the header says)
    const uint64_t n_comb = n_a && n_b && n_a <= 0xffffffffull / n_b ? n_a * n_b : 0;
    const uint64_t len_a = n_a ? k.read_len[fa] : 0, len_b = n_b ? k.read_len[fb] : 0;
    MateMin2 x = mate_min2_none(), a = mate_min2_none(), b = mate_min2_none();
    for (uint64_t c = t; c < n_comb; c += team) {
        const uint64_t i = fa + (uint32_t)c / (uint32_t)n_b, j = fb + (uint32_t)c % (uint32_t)n_b;
        if (k.status[i] == (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT || k.status[j] == (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT) continue;
        const uint32_t r_i = k.reverse ? (k.reverse[i] != 0) : 0u, r_j = k.reverse ? (k.reverse[j] != 0) : 0u;
        if (mate_proper(k.rule, k.start[i], r_i, len_a, k.start[j], r_j, len_b))
            mate_min2_push(x, mate_value((uint64_t)mate_ed(k.ed[i]) + mate_ed(k.ed[j]), (uint32_t)c));
    }
    for (uint64_t c = t; c < n_a + n_b; c += team) {
        const uint64_t p = fa + c;
        if (k.status[p] == (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT) continue;
        if (c < n_a) mate_min2_push(a, mate_value(mate_ed(k.ed[p]), (uint32_t)c));
        else mate_min2_push(b, mate_value(mate_ed(k.ed[p]), (uint32_t)(c - n_a)));
    }
    // the butterfly: all 64 lanes, whatever they had to do above
    mate_step<1>(team, x, a, b);
    mate_step<2>(team, x, a, b);
    mate_step<4>(team, x, a, b);
    mate_step<8>(team, x, a, b);
    mate_step<16>(team, x, a, b);
    mate_step<32>(team, x, a, b);
    if (!live) return;
    const MateVerdict v = mate_decide(k.rule, x, a, b, (uint32_t)n_b);
    const uint64_t w_a = v.i != MATE_NONE ? fa + v.i : MATE_NONE, w_b = v.j != MATE_NONE ? fb + v.j : MATE_NONE;
    if (t == 0) {
        scrg_mate_record r;
        r.winner[0] = w_a;
        r.winner[1] = w_b;
        r.cost = v.cost;
        r.second_cost = v.second_cost;
        r.span = w_a != MATE_NONE && w_b != MATE_NONE ? mate_span32(mate_span(k.start[w_a], len_a, k.start[w_b], len_b)) : 0u;
        r.n_proper = v.n_proper;
        r.flags = v.flags;
        r.reserved = 0;
        k.records[m] = r;
    }
    // the losers lose their runs (every load of a status above has been consumed by the butterfly: this team's lanes are one wavefront's)
    for (uint64_t c = t; c < n_a + n_b; c += team) {
        const uint64_t p = fa + c;
        const bool eligible = k.status[p] != (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT, winner = p == w_a || p == w_b;
        if (eligible && !winner) {
            k.n_runs[p] = 0u;
            k.status[p] = (uint32_t)LANE_STATUS_NOT_BEST;
        }
        if (k.is_best) k.is_best[p] = winner ? 1 : 0;
    }
}

uint32_t mate_team_size(uint64_t most_combinations)
{
    uint32_t team = 4;
    while (team < 64 && team < most_combinations) team <<= 1;
    return team;
}

hipError_t launch_select_mates(const scrg_mate_rule& rule, uint32_t team, uint32_t* team_word, uint64_t n_mates, const uint64_t* first,
                               const uint64_t* start, const uint32_t* read_len, const uint8_t* reverse, const int64_t* ed, uint32_t* status,
                               uint32_t* n_runs, uint8_t* is_best, scrg_mate_record* records, hipStream_t s)
{
    if (n_mates == 0) return hipSuccess;
    if (team_word) {
        const hipError_t e = hipMemsetAsync(team_word, 0, sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(mate_team_kernel, dim3((unsigned)std::min<uint64_t>(1024, (n_mates + 255) / 256)), dim3(256), 0, s, n_mates, first, team_word);
        team = 64;                    // (the grid: enough wavefronts for any team size; those past the work leave at once)
    }
    MateArgs k;
    k.rule = MateRule{rule.min_span, rule.max_span, rule.orientation, rule.unpaired_penalty};
    k.n_mates = n_mates;
    k.first = first;
    k.start = start;
    k.read_len = read_len;
    k.reverse = reverse;
    k.ed = ed;
    k.status = status;
    k.n_runs = n_runs;
    k.is_best = is_best;
    k.records = records;
    k.team_word = team_word;
    k.team = team;
    const uint64_t per_wave = 64u / team, n_waves = (n_mates + per_wave - 1) / per_wave;
    hipLaunchKernelGGL(mate_select_kernel, dim3((unsigned)((n_waves + 3) / 4)), dim3(256), 0, s, k);
    return hipGetLastError();      // (of either launch: a team pass that could not be launched is reported here too)
}

}  // namespace scrg
