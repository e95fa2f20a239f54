// Host build of scrooge_amd/csrc/seed_rule.h (g++): C entry points over the words a hit, a cluster and a candidate are sorted and
// compared by, for tests/test_seed_big.py.
#include <stdint.h>
#include "seed_rule.h"

using namespace scrg;

extern "C" {

uint64_t sw_hit_word(uint64_t read_in_chunk, uint32_t strand, uint32_t p, uint32_t r) { return seed_hit_word(read_in_chunk, strand, p, r); }
uint64_t sw_hit_group(uint64_t word) { return seed_hit_group(word); }
uint64_t sw_hit_read(uint64_t word) { return seed_hit_read(word); }
uint32_t sw_hit_strand(uint64_t word) { return seed_hit_strand(word); }
uint64_t sw_hit_dbias(uint64_t word) { return seed_hit_dbias(word); }
int sw_is_head(uint64_t prev, uint64_t word, uint32_t band) { return seed_is_head(prev, word, band) ? 1 : 0; }

uint64_t sw_anchor_word(uint32_t r, uint64_t dbias) { return seed_anchor_word(r, dbias); }
uint32_t sw_anchor_start(uint64_t anchor) { return seed_anchor_start(anchor); }

// out: hi, lo
void sw_rank(uint32_t votes, uint32_t start, uint32_t strand, uint32_t nth, uint64_t* out)
{
    const SeedRank x = seed_rank(votes, start, strand, nth);
    out[0] = x.hi;
    out[1] = x.lo;
}
int sw_rank_less(const uint64_t* a, const uint64_t* b) { return seed_rank_less(SeedRank{a[0], a[1]}, SeedRank{b[0], b[1]}) ? 1 : 0; }
uint32_t sw_rank_votes(const uint64_t* a) { return seed_rank_votes(SeedRank{a[0], a[1]}); }
uint32_t sw_rank_start(const uint64_t* a) { return seed_rank_start(SeedRank{a[0], a[1]}); }
uint32_t sw_rank_strand(const uint64_t* a) { return seed_rank_strand(SeedRank{a[0], a[1]}); }

uint64_t sw_index_entries(uint64_t genome_len, uint32_t k, uint32_t stride) { return seed_index_entries(genome_len, k, stride); }
}
