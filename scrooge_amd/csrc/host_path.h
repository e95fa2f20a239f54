// host_path.h — launch interface of host_path_kernels.hip (the pipelined host-pointer path, scrg_host.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "genasm_kernels.h"

namespace scrg {

// ---------------------------------------------------------------------------------------------------------------
// What a chunk of n pairs looks like in memory: the ONE statement of the formats the host (scrg_host.cpp) and the kernels share.
// ---------------------------------------------------------------------------------------------------------------
// The per-pair upload: [read_len 4n | text_len (pairwise) or row word (mapping) 4n | pad to 16 | start 8n (mapping) |
// key 4n (own_key: best-candidate mode where the row does not name the read)]
struct MetaLayout {
    size_t o_read_len, o_text_len, o_start, o_key, bytes;
    SCRG_HD MetaLayout(uint64_t n, bool mapping, bool own_key)
        : o_read_len(0), o_text_len(4 * n), o_start((8 * n + 15) & ~(size_t)15), o_key(o_start + 8 * n),
          bytes(n * (mapping ? 16 : 8) + (own_key ? 4 * n : 0) + 64) {}
};
// a mapping pair's row word: the read row of the pair, bit 31 = the read's reverse complement is aligned (one pair per lane),
// bit 30 = a leftward candidate (scrg_align_mapping_directed): its text is the reverse complement of the genome prefix that ends
// at its start, i.e. text_off = 0 | SCRG_TEXT_REVCOMP, text_len = start.  (Bit 31 is then the READ'S flag as the kernel takes
// it — the candidate's strand XOR leftward: what is aligned is the reverse complement of the read as the candidate names it.)
constexpr uint32_t ROW_REVERSE = 0x80000000u;
constexpr uint32_t ROW_LEFTWARD = 0x40000000u;
constexpr uint32_t ROW_INDEX_MASK = ~(ROW_REVERSE | ROW_LEFTWARD);

// A chunk's per-pair results on the device: [ed 8n | status 4n (+pad) | run_off 8n | text_off 8n] (what the kernels write and
// read), and what of them crosses PCIe, the "wire": [ed 4n | run count and flags 4n | text length 4n] at o_wire
// (wire_totals_kernel) — the offsets are made again on the host from the counts (scrg_host.cpp, stage 3).
// Distance-only mode: [ed 8n | status 4n | text_end 4n] is all a chunk produces, and it comes back as it is.
struct PerPairLayout {
    size_t o_st, o_ro, o_to, o_wire, bytes, wire_bytes, o_tend, distance_bytes;
    SCRG_HD explicit PerPairLayout(uint64_t n)
        : o_st(8 * n), o_ro((8 * n + 4 * n + 15) & ~(size_t)15), o_to(o_ro + 8 * n), o_wire((o_to + 8 * n + 255) & ~(size_t)255), bytes(o_wire + 12 * n),
          wire_bytes(12 * n), o_tend(12 * n), distance_bytes(16 * n) {}
    SCRG_HD size_t host_runs() const { return (wire_bytes + 256 + 4095) & ~(size_t)4095; }      // staging area: [wire | runs (then the text)]
};

// The wire's run-count word: the count in 29 bits; bit 31 = the slice overflowed, bit 30 = over the edit limit (no runs, "" —
// which is no failure of the call; it wins over bit 31), bit 29 = not the best candidate of its read (SCRG_OUT_BEST: no runs,
// "" either, and only ever set alone; a slice of such a pair that overflowed is of no interest any more).
// (Only best-candidate mode checks that a slice's capacity fits the 29 bits.  Without it, a count of 2^29 runs or more — a single
// read of 2^28 bases with pathological runs — is taken for flags and ends in stage 3's "sizes do not add up" internal error.)
constexpr uint32_t WIRE_OVERFLOW = 0x80000000u, WIRE_OVER_LIMIT = 0x40000000u, WIRE_NOT_BEST = 0x20000000u;
constexpr uint32_t WIRE_COUNT_MASK = 0x1fffffffu;
SCRG_HD inline uint32_t wire_count_word(uint32_t count, uint32_t lane_status)
{
    return count | (lane_status == LANE_STATUS_OVER_EDIT_LIMIT ? WIRE_OVER_LIMIT : lane_status == LANE_STATUS_NOT_BEST ? WIRE_NOT_BEST : lane_status ? WIRE_OVERFLOW : 0u);
}
SCRG_HD inline uint32_t wire_pair_status(uint32_t word)
{
    return (word & WIRE_OVER_LIMIT) ? (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT : (word & WIRE_NOT_BEST) ? (uint32_t)SCRG_PAIR_NOT_BEST
           : (word & WIRE_OVERFLOW) ? (uint32_t)SCRG_ERR_CIGAR_OVERFLOW : (uint32_t)SCRG_OK;
}
SCRG_HD inline bool wire_overflowed(uint32_t word) { return (word & ~WIRE_COUNT_MASK) == WIRE_OVERFLOW; }
// a per-pair status as the kernels leave it (LaneStatus) -> what the host entry points report
SCRG_HD inline uint32_t public_status(uint32_t lane_status)
{
    return lane_status == LANE_STATUS_OVER_EDIT_LIMIT ? (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT : lane_status == LANE_STATUS_NOT_BEST ? (uint32_t)SCRG_PAIR_NOT_BEST
           : lane_status ? (uint32_t)SCRG_ERR_CIGAR_OVERFLOW : (uint32_t)SCRG_OK;
}

struct HostDescArgs {
    uint64_t n;                   // pairs of the chunk
    scrg_pair_desc* desc;         // out
    const uint32_t* read_len;     // [n]
    const uint32_t* text_len;     // [n]   pairwise                                                  (the four: MetaLayout)
    const uint64_t* start;        // [n]   mapping: start_in_reference; null = pairwise
    const uint32_t* row;          // [n]   mapping: the pair's row word (ROW_REVERSE | ROW_LEFTWARD | row); null = row i
    uint64_t genome_len;
    uint64_t read_base, read_words;   // first word and words per row of the read region (lane-interleaved groups of 64 rows)
    uint64_t text_base, text_words;   // the same for the texts (pairwise)
    uint64_t cap;                 // runs per slice, a multiple of 16
    uint32_t linear;              // 1: rows are contiguous (word stride 1: the GenASM-row kernels); 0: lane-interleaved groups of 64 rows
};

hipError_t launch_build_desc(const HostDescArgs& a, hipStream_t s);
size_t host_scan_temp_bytes(uint64_t n);
// (wire: what goes back to the host, PerPairLayout)
hipError_t launch_result_layout(uint64_t n, const scrg_pair_desc* pairs, const uint16_t* runs, const uint32_t* n_runs, const int64_t* ed,
                                const uint32_t* status, uint64_t* cnt64, uint64_t* len64, uint64_t* run_off, uint64_t* text_off,
                                uint64_t* totals, uint32_t* wire, void* temp, size_t temp_bytes, int want_text, int32_t form, int n_cus,
                                hipStream_t s);
hipError_t launch_render_text(uint64_t n, const uint16_t* dense, const uint64_t* run_off, const uint64_t* cnt64, const uint64_t* text_off,
                              uint8_t* text, int32_t form, int n_cus, hipStream_t s);
// (form: SCRG_CIGAR_WINDOWED, _MERGED or _M (scrooge_amd.h, CIGAR FORMS): both take the same one for a chunk; no form's text of a pair
// is longer than the windowed one, which is what the buffers are sized for)

// ---- the CIGAR text of runs on device buffers in any form (scrg_cigar_text_lengths, scrg_cigar_text_render): runs as for PairRuns
// below; len[p] includes the NUL; the render pass takes it as an input and checks it, with the segment, before it writes.
hipError_t launch_cigar_text_lengths(uint64_t n, const uint16_t* runs, const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs,
                                     int32_t form, uint64_t* len, int n_cus, hipStream_t s);
hipError_t launch_cigar_text_render(uint64_t n, const uint16_t* runs, const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs,
                                    int32_t form, const uint64_t* len, const uint64_t* off, uint8_t* text, uint64_t capacity, uint32_t* bad,
                                    int n_cus, hipStream_t s);

// ---- what the passes over finished alignments take (diff_kernels.hip, report_kernels.hip; run_walk.h): n pairs, their packed
// sequences, descriptors and runs.  Pair p's runs: runs[run_off[p * run_off_stride] + k], k < n_runs[p] (stride 6:
// &pairs[0].cigar_off, the count capped at cigar_cap).
struct PairRuns {
    uint64_t n;
    const uint64_t* seq;
    const scrg_pair_desc* pairs;
    const uint16_t* runs;
    const uint64_t* run_off;
    uint64_t run_off_stride;      // 1 or 6
    const uint32_t* n_runs;
    uint32_t text_stride, read_stride;        // words between a sequence's words (scrg_params, at least 1)
    uint32_t stranded;            // SCRG_READ_REVCOMP is honoured
};

// ---- diff_kernels.hip: difference strings (MD / cs) of every pair from its runs and the packed sequences (scrg_diff_lengths,
// scrg_diff_render; stage 2 of the host path).  len[p] includes the NUL; the render pass takes it as an input.
hipError_t launch_diff_lengths(const PairRuns& pr, int32_t kind, uint64_t* len, int n_cus, hipStream_t s);
hipError_t launch_diff_render(const PairRuns& pr, int32_t kind, const uint64_t* len, const uint64_t* off, uint8_t* text, uint64_t capacity,
                              uint32_t* bad, int n_cus, hipStream_t s);
// out[0 .. n] = exclusive prefix sums of len[0 .. n), out[n] = their total (temp: host_scan_temp_bytes(n + 1); len[n] is written)
hipError_t launch_diff_offsets(uint64_t n, uint64_t* len, uint64_t* off, void* temp, size_t temp_bytes, hipStream_t s);

// ---- report_kernels.hip: the alignment report (scrg_report_device; stage 1 of the host path, after the selection).  Runs as for
// the difference strings; status (may be null) as the align kernels and the selection leave it; *fail (may be null) += the pairs
// whose verdict is neither 0 nor 7.  per_base: the one-base-at-a-time build of the same kernel (the A/B of bench_report.py).
hipError_t launch_report(const PairRuns& pr, const int64_t* ed, const uint32_t* status, uint32_t text_strands, scrg_pair_report* report,
                         uint32_t* fail, bool per_base, int n_cus, hipStream_t s);

// ---- pileup_kernels.hip: the pileup (scrg_pileup_add, scrg_pileup_finish; stage 1 of the host path, where the report runs).
// Runs as for the report; status (may be null) as the align kernels and the selection leave it: only status 0 is counted.
// acc: [7][target_len + 1] words, MATCH and DEL in edge form; *outside (may be null) += the pairs with a column or an insertion
// outside the target, *counted (may be null) += the pairs that were counted.  The text is never read.
hipError_t launch_pileup_add(const PairRuns& pr, const uint32_t* status, const uint64_t* target_start, uint64_t target_len, uint32_t* acc,
                             uint32_t* outside, uint32_t* counted, int n_cus, hipStream_t s);
// edge form -> counts (planes 0 and 5 summed, the others copied unless counts == acc); scratch: pileup_finish_scratch_bytes(target_len),
// 4-byte aligned, need not be initialised
size_t pileup_finish_scratch_bytes(uint64_t target_len);
hipError_t launch_pileup_finish(uint64_t target_len, const uint32_t* acc, uint32_t* counts, void* scratch, hipStream_t s);

// ---- site_kernels.hip: the pileup sites (scrg_pileup_sites_mark, scrg_pileup_sites_write).  counts: [7][target_len + 1] in counts
// form, only read; seq, genome_off: the target's bases, linear 2-bit packing.  scratch: site_scratch_bytes(target_len), 8-byte aligned,
// need not be initialised; mark leaves in it what write reads, the (valid) rule included.  target_len < 2^32 - 1.
size_t site_scratch_bytes(uint64_t target_len);
hipError_t launch_site_mark(uint64_t target_len, const uint32_t* counts, const uint64_t* seq, uint64_t genome_off, const scrg_site_rule& rule, void* scratch,
                            uint64_t* n_sites, hipStream_t s);
hipError_t launch_site_write(uint64_t target_len, const uint32_t* counts, const uint64_t* seq, uint64_t genome_off, void* scratch, uint64_t cap, scrg_site* sites,
                             hipStream_t s);

// ---- clip_kernels.hip: soft clipping (scrg_clip_device; stage 1 of the host path, after the selection and before the result
// layout).  Runs by offset and stride as for PairRuns; status (may be null) as the align kernels and the selection leave it;
// costs: match, mismatch, gap_open, gap_extend.  apply: a second launch makes the kept stretch the pair's alignment — n_runs,
// run_off and (stride 6) the capacity behind it are written.
hipError_t launch_clip(uint64_t n, const uint16_t* runs, uint64_t* run_off, uint64_t run_off_stride, uint32_t* n_runs, const uint32_t* status,
                       const int32_t* costs, bool apply, scrg_pair_clip* clip, int n_cus, hipStream_t s);

// ---- select_kernels.hip: best-candidate selection (SCRG_OUT_BEST of the host path, scrg_select_best)
size_t select_scratch_bytes(uint64_t n);
// Groups are runs of consecutive pairs with equal (key & key_mask).  Losers: n_runs = 0, status = LANE_STATUS_NOT_BEST;
// is_best (may be null) 1/0 per pair.  `scratch`: select_scratch_bytes(n), 8-byte aligned, need not be initialised.  n < 2^32.
hipError_t launch_select_best(uint64_t n, const uint32_t* key, uint32_t key_mask, const int64_t* ed, uint32_t* status, uint32_t* n_runs,
                              uint8_t* is_best, void* scratch, hipStream_t s);

// ---- mate_kernels.hip: paired-end selection (scrg_align_mapping_paired of the host path, scrg_select_mates; the rule: mate_rule.h)
// Reads 2m and 2m+1 are mate pair m; first[r] (2 n_mates + 1 of them, non-decreasing) is the index of read r's first pair: a read's
// candidates are consecutive, and so are a mate pair's two reads.  start, read_len, reverse (may be null: all forward), ed, status
// and n_runs are per pair.  Losers as launch_select_best leaves them; is_best (may be null) 1/0 per pair; records[m]: winner[] are
// indices into these arrays.  A team of `team` lanes (4 .. 64, mate_team_size of the batch's largest n_a x n_b) serves a mate pair;
// team_word not null: the team size is found on the device first and left there (`team` is not looked at).  rule: valid.
uint32_t mate_team_size(uint64_t most_combinations);
hipError_t launch_select_mates(const scrg_mate_rule& rule, uint32_t team, uint32_t* team_word, uint64_t n_mates, const uint64_t* first,
                               const uint64_t* start, const uint32_t* read_len, const uint8_t* reverse, const int64_t* ed, uint32_t* status,
                               uint32_t* n_runs, uint8_t* is_best, scrg_mate_record* records, hipStream_t s);

// ---- mapq_kernels.hip: the per-read candidate summary and its MAPQ (the host calls' read summary, scrg_read_summary; the rule: mapq_rule.h)
// first[r] (n_reads + 1 of them, non-decreasing, at most n_pairs) is the index of read r's first pair; read_len, ed and status are per
// pair and only read.  out[r]: read r's record, winner as an index into these arrays.  keep_status (may be null, not `status`): the
// statuses with every done pair that is not the winner of a KEPT read as LANE_STATUS_NOT_BEST.  rule: valid.
hipError_t launch_read_summary(const scrg_mapq_rule& rule, uint64_t n_reads, uint64_t n_pairs, const uint64_t* first, const uint32_t* read_len,
                               const int64_t* ed, const uint32_t* status, scrg_read_record* out, uint32_t* keep_status, hipStream_t s);

// ---- seed_kernels.hip: seeding (scrg_genome_index, scrg_find_candidates; the rule: seed_rule.h)
// The index as a lookup sees it: n_entries (key, pos) sorted by key, and buckets[b] = the first entry whose key >> shift is at least
// b, b in [0, 2^(2k - shift)].
struct SeedIndexView {
    const uint32_t* keys;
    const uint32_t* pos;
    const uint32_t* buckets;
    uint32_t shift, k, max_occ, band, min_hits, max_candidates;
    uint32_t smer;                    // the sampling the index was built with (seed_rule.h: seed_key_selected); 0: every key
};
// A call's reads on the device: packed planar, read i from word word[i] on, ceil(len / 32) words and one of padding; lane_off[i]
// (n_reads + 1 of them) = the (strand, r) of all reads before i: n_strands * max(0, len - k + 1) each.
struct SeedReadsView {
    const uint64_t* seq;
    const uint64_t* word;
    const uint32_t* len;
    const uint64_t* lane_off;
    uint32_t n_strands;
};
// One chunk of whole reads [read0, read0 + n_reads), at most 2^22 of them: its lanes (lane_base = lane_off[read0]; below 2^31), its
// hits (n_hits, known from launch_seed_totals; below 2^31) and the buffers they go through.
struct SeedChunk {
    uint64_t read0, n_reads, lane_base, n_lanes, n_hits;
    uint64_t *cnt, *off;              // [n_lanes + 1] both
    uint64_t *word_tmp, *word;        // [n_hits]: the hits' words as emitted and sorted
    uint32_t *r_tmp, *r;              // [n_hits]
    uint32_t *head, *cluster;         // [n_hits]
    uint32_t* first;                  // [n_hits + 1]
    uint64_t* anchor;                 // [n_hits]
    uint32_t *out_n, *out_start, *out_votes;      // [n_reads], [n_reads * max_candidates] twice
    uint8_t* out_strand;              // [n_reads * max_candidates]
    void* temp;                       // seed_chunk_temp_bytes(n_lanes, n_hits, n_reads)
    size_t temp_bytes;
};
uint32_t seed_bucket_bits(uint64_t n_entries, uint32_t k);
size_t seed_index_sort_temp_bytes(uint64_t n_entries, uint32_t k);
// genome: planar, stride 1, a word of padding behind its last; buckets: 2^bucket_bits + 1 words; cluster[n_hits - 1] of a chunk is
// its number of clusters
// smer == 0: n_entries = the considered positions, one entry each.  smer > 0: launch_seed_select_count first — block_cnt and
// block_base hold seed_select_blocks(n_positions) + 1 words each, temp seed_select_temp_bytes(n_positions); block_base's last word
// is then the number of entries, which the caller reads back to size keys, pos and the sort's space — and launch_seed_index with
// that n_entries, the same n_positions and block_base.
uint64_t seed_select_blocks(uint64_t n_positions);
size_t seed_select_temp_bytes(uint64_t n_positions);
hipError_t launch_seed_select_count(const uint64_t* genome, uint64_t n_positions, uint32_t k, uint32_t stride, uint32_t smer, uint32_t* block_cnt,
                                    uint32_t* block_base, void* temp, size_t temp_bytes, hipStream_t s);
hipError_t launch_seed_index(const uint64_t* genome, uint64_t n_entries, uint32_t k, uint32_t stride, uint32_t* keys_tmp, uint32_t* pos_tmp, uint32_t* keys,
                             uint32_t* pos, uint32_t bucket_bits, uint32_t* buckets, void* temp, size_t temp_bytes, hipStream_t s, uint32_t smer = 0,
                             uint64_t n_positions = 0, const uint32_t* block_base = nullptr);
// read_lookups[read]: the (strand, r) of the read whose key the index's sampling selects (all of them at smer 0)
hipError_t launch_seed_totals(const SeedIndexView& ix, const SeedReadsView& rd, uint64_t read0, uint64_t n_reads, uint64_t* read_hits, uint32_t* read_over,
                              uint32_t* read_lookups, hipStream_t s);
size_t seed_chunk_temp_bytes(uint64_t n_lanes, uint64_t n_hits, uint64_t n_reads);
hipError_t launch_seed_chunk(const SeedIndexView& ix, const SeedReadsView& rd, const SeedChunk& ch, hipStream_t s);

}  // namespace scrg
