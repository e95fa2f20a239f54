// seed_rule.h — the rule of seeding (include/scrooge_amd.h: SEEDING) that the kernels (seed_kernels.hip) and the host twin
// (scrg_candidates_from_genome, scrg_io.cpp, which sees nothing of HIP) share: the ranges of a rule, the key of k bases taken from
// the planar 2-bit packing, the words a hit, a cluster and a candidate are sorted and compared by, and where a cluster starts.
// Every quantity is a count or a minimum over a set: nothing here depends on the order in which hits are met.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SCRG_SEED_HD __host__ __device__
#else
#define SCRG_SEED_HD
#endif

namespace scrg {

struct SeedRule {                 // scrg_seed_rule, valid (seed_rule_valid), hit_budget_mb resolved
    uint32_t k, stride, max_occ, band, min_hits, max_candidates, strands, hit_budget_mb;
};

constexpr uint32_t SEED_DEFAULT_BUDGET_MB = 256;
constexpr uint64_t SEED_MAX_GENOME = 0xffffffffull;          // positions are 32-bit: genome_len <= 2^32 - 1
constexpr uint64_t SEED_MAX_ENTRIES = 0x7fffffffull;         // index entries are counted in 31 bits (the sort's item count)
constexpr uint64_t SEED_MAX_READ = 0x3fffffffull;            // a read is shorter than 2^30 bases: its (strand, r) of both strands count in 31 bits

SCRG_SEED_HD inline bool seed_rule_valid(uint32_t k, uint32_t stride, uint32_t max_occ, uint32_t band, uint32_t min_hits, uint32_t max_candidates,
                                         uint32_t strands)
{
    return k >= 8u && k <= 16u && stride >= 1u && stride <= 64u && max_occ >= 1u && max_occ <= 65535u && band <= 65535u && min_hits >= 1u &&
           max_candidates >= 1u && max_candidates <= 64u && (strands == 1u || strands == 3u);
}

// index entries of a genome: the p with p % stride == 0 and p + k <= genome_len
SCRG_SEED_HD inline uint64_t seed_index_entries(uint64_t genome_len, uint32_t k, uint32_t stride)
{
    return genome_len >= k ? (genome_len - k) / stride + 1u : 0u;
}

// the r of a read on one strand: [0, L - k]
SCRG_SEED_HD inline uint64_t seed_read_positions(uint64_t read_len, uint32_t k) { return read_len >= k ? read_len - k + 1u : 0u; }

// bit i of x (i < 16) to bit 2 i
SCRG_SEED_HD inline uint32_t seed_spread16(uint32_t x)
{
    x &= 0xffffu;
    x = (x | (x << 8)) & 0x00ff00ffu;
    x = (x | (x << 4)) & 0x0f0f0f0fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

SCRG_SEED_HD inline uint32_t seed_brev32(uint32_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse32(x);                    // (v_bfrev_b32 on the device)
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

// The planes of 16 bases from base `at` of a sequence packed planar (one uint64 per 32 bases: bit j of the low dword = bit 0 of base
// j's code, of the high dword = bit 1; A0 C1 G2 T3), words `w0` = word at / 32 and `w1` = the one behind it: base at + i at bit i.
SCRG_SEED_HD inline void seed_planes16(uint64_t w0, uint64_t w1, uint32_t at, uint32_t& lo, uint32_t& hi)
{
    const uint32_t b = at & 31u;
    lo = (uint32_t)(((w1 << 32) | (w0 & 0xffffffffull)) >> b) & 0xffffu;
    hi = (uint32_t)(((w1 & 0xffffffff00000000ull) | (w0 >> 32)) >> b) & 0xffffu;
}

// The key of the k bases whose planes are lo and hi (base i at bit i): sum of code[i] 4^(k-1-i).
SCRG_SEED_HD inline uint32_t seed_key_forward(uint32_t lo, uint32_t hi, uint32_t k)
{
    const uint32_t rl = seed_brev32(lo) >> (32u - k), rh = seed_brev32(hi) >> (32u - k);
    return seed_spread16(rl) | (seed_spread16(rh) << 1);
}

// The key of the reverse complement of those k bases: its base i is the complement (3 - code) of base k-1-i, so base j of the
// forward window lands at weight 4^j — no reversal, both planes inverted.
SCRG_SEED_HD inline uint32_t seed_key_revcomp(uint32_t lo, uint32_t hi, uint32_t k)
{
    const uint32_t m = (1u << k) - 1u;
    return seed_spread16(~lo & m) | (seed_spread16(~hi & m) << 1);
}

// Sampling (scrg_ctx_set_seed_sampling): smer = 0 takes every key; 3 .. k - 1 takes the closed syncmers of s-mers.
SCRG_SEED_HD inline bool seed_smer_valid(uint32_t smer, uint32_t k) { return smer == 0u || (smer >= 3u && smer < k); }

// An s-mer's order word: a bijection on 32-bit words, so that only equal s-mers tie.
SCRG_SEED_HD inline uint32_t seed_smer_order(uint32_t v)
{
    const uint32_t m = v * 0x9E3779B1u;
    return m ^ (m >> 15);
}

// Is `key` (k bases, base 0 at the top; smer valid for k) selected?  Its s-mer j, j in [0, k - s], is the s bases from base j; the
// key is selected iff the least order word among them is that of the first s-mer or of the last (a tie at either end counts).  It
// depends on the key alone: not on its neighbours, not on the strand it was read from.
SCRG_SEED_HD inline bool seed_key_selected(uint32_t key, uint32_t k, uint32_t smer)
{
    if (smer == 0u) return true;
    const uint32_t mask = (1u << (2u * smer)) - 1u;      // (smer <= 15)
    const uint32_t first = seed_smer_order((key >> (2u * (k - smer))) & mask), last = seed_smer_order(key & mask);
    uint32_t inner = 0xffffffffu;
    for (uint32_t j = 1; j < k - smer; j++) {
        const uint32_t h = seed_smer_order((key >> (2u * (k - smer - j))) & mask);
        inner = h < inner ? h : inner;
    }
    return (first < last ? first : last) <= inner;
}

// On strand 1 position r of R' (the reverse complement) covers the forward read's bases [L - k - r, L - r).
SCRG_SEED_HD inline uint32_t seed_window_at(uint32_t read_len, uint32_t k, uint32_t strand, uint32_t r)
{
    return strand ? read_len - k - r : r;
}

// A hit's sort word: (read in chunk, strand, d + 2^32) — d = p - r lies in (-2^30, 2^32), so d + 2^32 fills 33 bits.
constexpr uint32_t SEED_D_BITS = 33, SEED_READ_SHIFT = 34;
constexpr uint64_t SEED_D_BIAS = 1ull << 32, SEED_D_MASK = (1ull << 33) - 1u;
constexpr uint64_t SEED_MAX_CHUNK_READS = 1ull << 30;
SCRG_SEED_HD inline uint64_t seed_hit_word(uint64_t read_in_chunk, uint32_t strand, uint32_t p, uint32_t r)
{
    return (read_in_chunk << SEED_READ_SHIFT) | ((uint64_t)strand << SEED_D_BITS) | ((uint64_t)p + SEED_D_BIAS - r);
}
SCRG_SEED_HD inline uint64_t seed_hit_group(uint64_t word) { return word >> SEED_D_BITS; }            // (read in chunk, strand)
SCRG_SEED_HD inline uint64_t seed_hit_read(uint64_t word) { return word >> SEED_READ_SHIFT; }
SCRG_SEED_HD inline uint32_t seed_hit_strand(uint64_t word) { return (uint32_t)(word >> SEED_D_BITS) & 1u; }
SCRG_SEED_HD inline uint64_t seed_hit_dbias(uint64_t word) { return word & SEED_D_MASK; }

// does the hit `word` (sorted after `prev`) begin a cluster?
SCRG_SEED_HD inline bool seed_is_head(uint64_t prev, uint64_t word, uint32_t band)
{
    return seed_hit_group(prev) != seed_hit_group(word) || seed_hit_dbias(word) - seed_hit_dbias(prev) > band;
}

// What a cluster's hits are reduced by: (r, d + 2^32) as one word — the minimum is the hit with the least r, ties to the least d.
SCRG_SEED_HD inline uint64_t seed_anchor_word(uint32_t r, uint64_t dbias) { return ((uint64_t)r << SEED_D_BITS) | dbias; }
SCRG_SEED_HD inline uint32_t seed_anchor_start(uint64_t anchor)             // max(0, d*)
{
    const uint64_t dbias = anchor & SEED_D_MASK;
    return dbias > SEED_D_BIAS ? (uint32_t)(dbias - SEED_D_BIAS) : 0u;
}

// What a read's clusters are ranked by: votes descending, start ascending, strand ascending; the SMALLEST word is the best.
// (Two clusters of one read can share all three — both clamped to start 0 — and are then the same candidate twice: `nth`, the
// cluster's number within its read, only keeps the words distinct so that a selection by "the next larger word" finds both.)
struct SeedRank {
    uint64_t hi, lo;
};
SCRG_SEED_HD inline SeedRank seed_rank(uint32_t votes, uint32_t start, uint32_t strand, uint32_t nth)
{
    return SeedRank{((uint64_t)(0xffffffffu - votes) << 32) | start, ((uint64_t)strand << 32) | nth};
}
SCRG_SEED_HD inline bool seed_rank_less(const SeedRank& a, const SeedRank& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
SCRG_SEED_HD inline uint32_t seed_rank_votes(const SeedRank& a) { return 0xffffffffu - (uint32_t)(a.hi >> 32); }
SCRG_SEED_HD inline uint32_t seed_rank_start(const SeedRank& a) { return (uint32_t)a.hi; }
SCRG_SEED_HD inline uint32_t seed_rank_strand(const SeedRank& a) { return (uint32_t)(a.lo >> 32) & 1u; }

}  // namespace scrg
