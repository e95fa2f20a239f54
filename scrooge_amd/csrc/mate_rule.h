// mate_rule.h — the rule of paired-end selection (include/scrooge_amd.h: MATE PAIRS) that the kernel (mate_kernels.hip) and the host
// twin (scrg_mates_from_distances, scrg_io.cpp, which sees nothing of HIP) share: is a combination of an A and a B candidate
// proper, how two running "two smallest" are merged, and what a mate pair's record is once the smallest are known.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SCRG_MATE_HD __host__ __device__
#else
#define SCRG_MATE_HD
#endif

namespace scrg {

constexpr uint32_t MATES_FR = 0, MATES_RF = 1, MATES_FF = 2, MATES_ANY = 3;                        // SCRG_MATES_FR ...
constexpr uint32_t MATES_PROPER = 1, MATES_HAS_A = 2, MATES_HAS_B = 4, MATES_TIED = 8;             // SCRG_MATES_PROPER ...
constexpr uint64_t MATE_NONE = ~0ull;

struct MateRule {                 // scrg_mate_rule, valid (mate_rule_valid)
    uint64_t min_span, max_span;
    uint32_t orientation, unpaired_penalty;
};

SCRG_MATE_HD inline bool mate_rule_valid(uint64_t min_span, uint64_t max_span, uint32_t orientation, uint32_t reserved0, uint32_t reserved1)
{
    return min_span <= max_span && orientation <= MATES_ANY && reserved0 == 0u && reserved1 == 0u;
}

// An edit distance as the rule counts it: 32 bits (a read is shorter than 2^31 bases), as best-candidate mode takes it.
SCRG_MATE_HD inline uint32_t mate_ed(int64_t ed) { return (uint32_t)ed; }

// What a candidate or a combination is ranked by: (cost << 32) | index — the minimum is the winner and names it, ties go to the
// lowest index; a combination's index is i * n_b + j, so "lowest i, then lowest j" is the same order.
SCRG_MATE_HD inline uint64_t mate_value(uint64_t cost, uint32_t index)
{
    return ((cost < 0xfffffffeull ? cost : 0xfffffffeull) << 32) | index;      // (below MATE_NONE whatever the index)
}

// The two smallest values seen and how many were seen.  Neutral: {MATE_NONE, MATE_NONE, 0}; merging is associative and commutative
// (the values of one mate pair are distinct: each names its index), so lanes may merge in any order.
struct MateMin2 {
    uint64_t m1, m2;
    uint32_t count;
};
SCRG_MATE_HD inline MateMin2 mate_min2_none() { return MateMin2{MATE_NONE, MATE_NONE, 0u}; }
SCRG_MATE_HD inline void mate_min2_push(MateMin2& a, uint64_t v)
{
    if (v < a.m1) {
        a.m2 = a.m1;
        a.m1 = v;
    } else if (v < a.m2) {
        a.m2 = v;
    }
    a.count++;
}
SCRG_MATE_HD inline MateMin2 mate_min2_merge(const MateMin2& a, const MateMin2& b)
{
    MateMin2 r;
    r.m1 = a.m1 < b.m1 ? a.m1 : b.m1;
    const uint64_t hi = a.m1 < b.m1 ? b.m1 : a.m1, lo2 = a.m2 < b.m2 ? a.m2 : b.m2;
    r.m2 = hi < lo2 ? hi : lo2;
    r.count = a.count + b.count;
    return r;
}

// span of an A candidate at s_a (read length len_a) and a B candidate at s_b: outermost end minus outermost start, from starts and
// read lengths only (start + length stays below 2^64: starts are genome positions)
SCRG_MATE_HD inline uint64_t mate_span(uint64_t s_a, uint64_t len_a, uint64_t s_b, uint64_t len_b)
{
    const uint64_t e_a = s_a + len_a, e_b = s_b + len_b;
    return (e_a > e_b ? e_a : e_b) - (s_a < s_b ? s_a : s_b);
}

SCRG_MATE_HD inline bool mate_oriented(uint32_t orientation, uint64_t s_a, uint32_t r_a, uint64_t s_b, uint32_t r_b)
{
    if (orientation == MATES_ANY) return true;
    if (orientation == MATES_FF) return r_a == r_b;
    if (r_a == r_b) return false;
    const uint64_t s_fwd = r_a ? s_b : s_a, s_rev = r_a ? s_a : s_b;
    return orientation == MATES_FR ? s_fwd <= s_rev : s_rev <= s_fwd;
}

SCRG_MATE_HD inline bool mate_proper(const MateRule& k, uint64_t s_a, uint32_t r_a, uint64_t len_a, uint64_t s_b, uint32_t r_b, uint64_t len_b)
{
    const uint64_t span = mate_span(s_a, len_a, s_b, len_b);
    return mate_oriented(k.orientation, s_a, r_a, s_b, r_b) && k.min_span <= span && span <= k.max_span;
}

// The decision, from the merged smallest: pairs = the proper combinations (index i * n_b + j), a and b = each side's eligible
// candidates (index within the side).  i and j: the winners within their sides, MATE_NONE: none.  (span is the caller's to fill.)
struct MateVerdict {
    uint64_t i, j;
    uint32_t cost, second_cost;
    uint16_t n_proper;
    uint8_t flags;
};
SCRG_MATE_HD inline MateVerdict mate_decide(const MateRule& k, const MateMin2& pairs, const MateMin2& a, const MateMin2& b, uint32_t n_b)
{
    MateVerdict v;
    v.n_proper = (uint16_t)(pairs.count < 65535u ? pairs.count : 65535u);
    v.second_cost = 0xffffffffu;
    // (a proper combination exists only where both sides have an eligible candidate)
    const bool proper = pairs.m1 != MATE_NONE && (pairs.m1 >> 32) <= (a.m1 >> 32) + (b.m1 >> 32) + (uint64_t)k.unpaired_penalty;
    if (proper) {
        const uint32_t c = (uint32_t)pairs.m1;
        v.i = c / n_b;
        v.j = c % n_b;
        v.cost = (uint32_t)(pairs.m1 >> 32);
        if (pairs.m2 != MATE_NONE) v.second_cost = (uint32_t)(pairs.m2 >> 32);
        v.flags = (uint8_t)(MATES_PROPER | MATES_HAS_A | MATES_HAS_B | (pairs.m2 != MATE_NONE && v.second_cost == v.cost ? MATES_TIED : 0u));
        return v;
    }
    const bool has_a = a.m1 != MATE_NONE, has_b = b.m1 != MATE_NONE;
    v.i = has_a ? (uint64_t)(uint32_t)a.m1 : MATE_NONE;
    v.j = has_b ? (uint64_t)(uint32_t)b.m1 : MATE_NONE;
    const uint64_t cost = (has_a ? a.m1 >> 32 : 0ull) + (has_b ? b.m1 >> 32 : 0ull);
    v.cost = (uint32_t)(cost < 0xffffffffull ? cost : 0xffffffffull);
    const bool tied = (a.m2 != MATE_NONE && (a.m2 >> 32) == (a.m1 >> 32)) || (b.m2 != MATE_NONE && (b.m2 >> 32) == (b.m1 >> 32));
    v.flags = (uint8_t)((has_a ? MATES_HAS_A : 0u) | (has_b ? MATES_HAS_B : 0u) | (tied ? MATES_TIED : 0u));
    return v;
}

SCRG_MATE_HD inline uint32_t mate_span32(uint64_t span) { return (uint32_t)(span < 0xffffffffull ? span : 0xffffffffull); }

}  // namespace scrg
