// mapq_rule.h — the per-read candidate summary and the mapping quality made from it (include/scrooge_amd.h: READ SUMMARY AND
// MAPPING QUALITY) that the kernel (mapq_kernels.hip) and the host twin (scrg_read_summary_from_distances, scrg_io.cpp, which sees
// nothing of HIP) share: what a partial summary of some of a read's candidates is, how two of them merge, what MAPQ the merged one
// earns, and the 32-byte record it becomes.  A mate pair's (cost, second_cost, TIED) fits mapq_of() as (best_ed, second_ed, n_tied).
//
// The constants of the default rule (10 per edit of distance to the second placement, at most 60, 0 at an edit rate of 25 %) are a
// HEURISTIC, as every mapper's MAPQ is: defaults of a rule the caller can set, validated against no truth set — not a claim that
// a read with MAPQ q is misplaced with probability 10^(-q/10).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SCRG_MAPQ_HD __host__ __device__
#else
#define SCRG_MAPQ_HD
#endif

namespace scrg {

constexpr uint32_t MAPQ_HAS_WINNER = 1, MAPQ_TIED = 2, MAPQ_HAS_SECOND = 4, MAPQ_KEPT = 8;          // SCRG_MAPQ_HAS_WINNER ...
constexpr uint64_t MAPQ_NONE = ~0ull;              // no winner (as a best value and as a record's winner)
constexpr uint32_t MAPQ_NO_ED = 0xffffffffu;       // no distance: second_ed without a second, both distances without a winner
constexpr uint32_t MAPQ_LANE_READ = 16;            // candidates up to which one lane serves a read (mapq_kernels.hip)

struct MapqRule {                 // scrg_mapq_rule, valid (mapq_rule_valid)
    uint32_t per_edit, max_q, zero_per_mille, min_keep_q;
};
SCRG_MAPQ_HD inline MapqRule mapq_rule_default() { return MapqRule{10u, 60u, 250u, 0u}; }

SCRG_MAPQ_HD inline bool mapq_rule_valid(uint32_t per_edit, uint32_t max_q, uint32_t zero_per_mille, uint32_t min_keep_q, uint32_t reserved)
{
    return per_edit <= 255u && max_q <= 254u && zero_per_mille >= 1u && zero_per_mille <= 1000u && min_keep_q <= 254u && reserved == 0u;
}

// An edit distance as the summary counts it: 32 bits (a read is shorter than 2^31 bases), as best-candidate mode takes it.
SCRG_MAPQ_HD inline uint32_t mapq_ed(int64_t ed) { return (uint32_t)ed; }

// A partial summary: some of one read's ELIGIBLE candidates.  best = (edit distance << 32) | pair index — the minimum is the winner
// and names it, ties to the lowest index (best-candidate mode's value); n_tied: candidates seen at best's distance; second_ed: the
// smallest distance seen strictly above best's; n_eligible: candidates seen.  Neutral: mapq_part_none().
struct MapqPart {
    uint64_t best;
    uint32_t n_tied, second_ed, n_eligible;
};
SCRG_MAPQ_HD inline MapqPart mapq_part_none() { return MapqPart{MAPQ_NONE, 0u, MAPQ_NO_ED, 0u}; }
SCRG_MAPQ_HD inline MapqPart mapq_part_one(uint32_t ed, uint32_t index) { return MapqPart{((uint64_t)ed << 32) | index, 1u, MAPQ_NO_ED, 1u}; }

// THE merge, associative and commutative (so lanes and hosts may merge in any order): the smaller best; n_tied adds only the sides
// that stand at the smaller distance; second_ed is the least of the two seconds and, where the two distances differ, the larger
// one.  (The neutral part's distance reads MAPQ_NO_ED, which is what "no second" is, and it brings no ties: no special case.)
SCRG_MAPQ_HD inline MapqPart mapq_merge(const MapqPart& a, const MapqPart& b)
{
    const uint32_t ea = (uint32_t)(a.best >> 32), eb = (uint32_t)(b.best >> 32);
    MapqPart r;
    r.best = a.best < b.best ? a.best : b.best;
    r.n_tied = (ea <= eb ? a.n_tied : 0u) + (eb <= ea ? b.n_tied : 0u);
    uint32_t s = a.second_ed < b.second_ed ? a.second_ed : b.second_ed;
    const uint32_t larger = ea < eb ? eb : ea;
    if (ea != eb && larger < s) s = larger;
    r.second_ed = s;
    r.n_eligible = a.n_eligible + b.n_eligible;
    return r;
}

// MAPQ of a read of length L.  64-bit arithmetic, divisions floor: max_q * 1000 * best_ed < 2^50, zero_per_mille * L < 2^42.
SCRG_MAPQ_HD inline uint32_t mapq_of(const MapqRule& k, uint64_t L, bool has_winner, uint32_t n_tied, uint32_t best_ed, uint32_t second_ed)
{
    if (!has_winner || n_tied > 1u) return 0u;
    const uint64_t max_q = k.max_q;
    uint64_t cap = max_q;
    if (L != 0) {
        const uint64_t off = max_q * 1000ull * best_ed / ((uint64_t)k.zero_per_mille * L);
        cap = max_q - (off < max_q ? off : max_q);
    }
    if (second_ed == MAPQ_NO_ED) return (uint32_t)cap;
    const uint64_t gap = (uint64_t)k.per_edit * (uint64_t)(second_ed - best_ed);
    const uint64_t by_gap = gap < max_q ? gap : max_q;
    return (uint32_t)(cap < by_gap ? cap : by_gap);
}

// The record of a read whose candidates are all in `p`, as the eight dwords of scrg_read_summary (little endian):
// [winner lo, winner hi, best_ed, second_ed, n_tied, n_eligible, n_candidates, mapq | flags << 8 | reserved << 16].
struct MapqWords {
    uint32_t w[8];
};
SCRG_MAPQ_HD inline MapqWords mapq_record(const MapqRule& k, const MapqPart& p, uint64_t L, uint32_t n_candidates)
{
    const bool won = p.best != MAPQ_NONE;
    const uint32_t best_ed = won ? (uint32_t)(p.best >> 32) : MAPQ_NO_ED, second_ed = won ? p.second_ed : MAPQ_NO_ED;
    const uint32_t q = mapq_of(k, L, won, p.n_tied, best_ed, second_ed);
    const uint32_t flags = (won ? MAPQ_HAS_WINNER : 0u) | (won && p.n_tied > 1u ? MAPQ_TIED : 0u) | (second_ed != MAPQ_NO_ED ? MAPQ_HAS_SECOND : 0u) |
                           (won && q >= k.min_keep_q ? MAPQ_KEPT : 0u);
    MapqWords r;
    r.w[0] = won ? (uint32_t)p.best : 0xffffffffu;
    r.w[1] = won ? 0u : 0xffffffffu;
    r.w[2] = best_ed;
    r.w[3] = second_ed;
    r.w[4] = won ? p.n_tied : 0u;
    r.w[5] = p.n_eligible;
    r.w[6] = n_candidates;
    r.w[7] = q | (flags << 8);
    return r;
}
SCRG_MAPQ_HD inline bool mapq_words_kept(const MapqWords& r) { return ((r.w[7] >> 8) & MAPQ_KEPT) != 0u; }

// What d_keep_status holds for a pair: its status, except that a finished pair (status 0) that is not the winner of a KEPT read reads
// `not_best` (LANE_STATUS_NOT_BEST / SCRG_PAIR_NOT_BEST).
SCRG_MAPQ_HD inline uint32_t mapq_keep_status(uint32_t status, bool kept_winner, uint32_t not_best) { return status == 0u && !kept_winner ? not_best : status; }

}  // namespace scrg
