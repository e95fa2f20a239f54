/*
 * scrooge_amd_io.h — the callers and data formats either side of the hot path
 * (SURVEY.md §8f): the reference's read-mapping front door and its result checks.
 *
 *   read_genome / read_fasta                  src/util.cpp:45-108
 *   read_fastq                                src/util.cpp:110-155
 *   read_maf / read_paf                       src/util.cpp:175-276
 *   left_extend_locations, get_global_seeds   src/util.cpp:284-301
 *   read_fastq_and_seed_locations             src/util.cpp:303-336
 *   the perf-test preparation (strand filter, length cap, inflation, sort)
 *                                             src/tests.cu:346-377
 *   get_alignment_score (affine re-scoring)   src/cpu_baseline.cpp:694-725
 *   validateCigarString                       src/tests.cu:27-169
 *
 * Host-side C++ behind a C ABI, in the same shared library as the aligner.
 * Beyond the reference: reverse-strand candidates can be aligned (the read is
 * reverse-complemented while staging) instead of dropped, and results can be
 * written as PAF with a cg:Z: tag or as SAM.
 */
#ifndef SCROOGE_AMD_IO_H
#define SCROOGE_AMD_IO_H

#include "scrooge_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SCRG_ERR_IO = 16,          /* file missing / unreadable                         */
    SCRG_ERR_FORMAT = 17       /* seed names an unknown read or chromosome, bad line */
};

typedef struct scrg_job scrg_job;   /* genome + reads + candidate locations */

typedef struct scrg_job_options {
    int32_t reverse_strand;    /* 0: drop '-' candidates (reference, src/tests.cu:346-355);
                                  1: align the reverse-complemented read against them        */
    int32_t sort_by_length;    /* 1: order reads longest first (src/tests.cu:375-377)        */
    int32_t inflation;         /* >1: replicate the read set (src/tests.cu:366-372)          */
    int32_t left_extend;       /* 1: left_extend_locations() before use (src/util.cpp:284)   */
    int64_t read_length_cap;   /* >=0: truncate reads (src/tests.cu:360-364); -1: off        */
} scrg_job_options;

void scrg_job_options_default(scrg_job_options *o);

/* Loads FASTA + FASTQ + seeds (.maf or .paf).  err (may be NULL) receives a message. */
scrg_status scrg_job_load(const char *genome_fasta, const char *reads_fastq, const char *seeds_path,
                          const scrg_job_options *opt, scrg_job **out, char *err, size_t err_len);
void scrg_job_free(scrg_job *job);

/* Sizes: reads, (read, candidate) pairs, genome bases, chromosomes. */
void scrg_job_counts(const scrg_job *job, uint64_t *n_reads, uint64_t *n_pairs, uint64_t *genome_len,
                     uint64_t *n_chromosomes);
/* Borrowed views in the shape scrg_align_mapping() takes; cand_reverse[k] != 0 marks a
 * reverse-strand candidate (its cand_start is on the forward genome). */
void scrg_job_arrays(const scrg_job *job, const char **genome, const char *const **reads,
                     const uint64_t **read_lens, const uint64_t **cand_offsets, const uint64_t **cand_start,
                     const uint8_t **cand_reverse);
const char *scrg_job_read_name(const scrg_job *job, uint64_t read);
/* chromosome name and 0-based start inside it for pair k */
const char *scrg_job_pair_chromosome(const scrg_job *job, uint64_t pair, uint64_t *start_in_chromosome,
                                     uint64_t *chromosome_len);

/* scrg_align_mapping() with a per-candidate strand flag (NULL = all forward). */
scrg_status scrg_align_mapping_stranded(scrg_ctx *ctx, const scrg_params *params,
                                        const char *genome, uint64_t genome_len,
                                        uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                        const uint64_t *cand_offsets, const uint64_t *cand_start,
                                        const uint8_t *cand_reverse, scrg_result **out);
/* Convenience: align every pair of a loaded job. */
scrg_status scrg_job_align(scrg_ctx *ctx, const scrg_params *params, const scrg_job *job, scrg_result **out);

/* SEEDING without another mapper's file (scrooge_amd.h, SEEDING).
 * scrg_candidates_from_genome: the candidates of n_reads reads on the host (no GPU, no handle) — the same rule text
 * (csrc/seed_rule.h) with an index of its own, made for the call: what the device result is held to.  rule == NULL: the defaults;
 * hit_budget_mb means nothing here.  The result is library-owned (scrg_candidates_free).  SCRG_ERR_BAD_BASE for a base outside
 * ACGTacgt in the genome or a read.
 * scrg_candidates_from_genome_sampled: the same with sampling (smer as scrg_ctx_set_seed_sampling: 0, or 3 .. k - 1; anything
 * else SCRG_ERR_INVALID_ARG); scrg_candidates_from_genome is this function at smer = 0.  n_entries (the index's entries) and
 * n_lookups (the selected (read, strand, r)) may be NULL.
 * scrg_job_load_unseeded: scrg_job_load without a seeds file — a job with no pairs (scrg_job_load with a NULL seeds path stays
 * SCRG_ERR_INVALID_ARG).  options as there; reverse_strand and left_extend have nothing to act on.
 * scrg_job_seed: makes the job's genome resident on the handle, indexes it, finds the reads' candidates on the GPU and installs
 * them as the job's pairs, both strands as the rule has them; scrg_job_align, scrg_job_align_paired and every writer then work
 * unchanged. */
scrg_status scrg_candidates_from_genome(const scrg_seed_rule *rule_or_NULL_for_defaults, const char *genome, uint64_t genome_len,
                                        uint64_t n_reads, const char *const *reads, const uint64_t *read_lens, scrg_candidates **out);
scrg_status scrg_candidates_from_genome_sampled(const scrg_seed_rule *rule_or_NULL_for_defaults, uint32_t smer, const char *genome,
                                                uint64_t genome_len, uint64_t n_reads, const char *const *reads,
                                                const uint64_t *read_lens, scrg_candidates **out, uint64_t *n_entries,
                                                uint64_t *n_lookups);
scrg_status scrg_job_load_unseeded(const char *genome_fasta, const char *reads_fastq, const scrg_job_options *opt, scrg_job **out,
                                   char *err, size_t err_len);
scrg_status scrg_job_seed(scrg_ctx *ctx, const scrg_seed_rule *rule_or_NULL_for_defaults, scrg_job *job);

/* One line per pair.  format 0: PAF (12 columns + NM:i + cg:Z:), 1: SAM, 2: TSV — read name, read length, strand, chromosome,
 * target start, target end, edit distance — for the pairs PAF writes (best-candidate mode: the winners; pairs over the edit
 * limit left out).  Target end = start + text_end of a distance-only result (SCRG_OUT_DISTANCE), else start + the text its runs
 * consume.  A distance-only result can be written as TSV only: formats 0 and 1 return SCRG_ERR_INVALID_ARG for it. */
scrg_status scrg_job_write(const scrg_job *job, const scrg_result *res, const char *path, int format);

/* scrg_job_write's lines with the pairs' difference strings appended (scrooge_amd.h, DIFFERENCE STRINGS; `diff` as
 * scrg_ctx_take_diff handed it over after the call that made `res`): "\tMD:Z:..." or "\tcs:Z:..." according to diff->kind, at
 * the end of the PAF and SAM records of pairs that have an alignment — an unmapped SAM record gets no tag.  diff == NULL is
 * scrg_job_write exactly.  Format 2 (TSV) with a diff, or a diff of another pair count, is SCRG_ERR_INVALID_ARG. */
scrg_status scrg_job_write_diff(const scrg_job *job, const scrg_result *res, const scrg_diff *diff, const char *path, int format);

/* scrg_job_write_diff's lines with the alignment report's tags appended (scrooge_amd.h, ALIGNMENT REPORT; `report` as
 * scrg_ctx_take_report handed it over after the call that made `res`): "\tAS:i:<score>\tde:f:<%.4f>" at the end of the PAF and SAM
 * records of pairs that have an alignment (after the difference string, if any).  The score is scrg_report_score with
 * costs = {match, mismatch, gap open, gap extend} (NULL: 2, 4, 4, 2, the reference baseline's default);
 * de = (n_mismatch + n_indel) / (n_match + n_mismatch + n_indel), the gap-compressed divergence, 0 when the denominator is 0.  PAF's
 * columns 10 and 11 (matches, alignment columns) and the target end come from the record instead of a walk over the runs: the same
 * numbers.  A record whose counts do not cover its runs (scrg_report_score refuses it) gets no tags, and its columns come from the
 * runs.  report == NULL is scrg_job_write_diff exactly; diff may be NULL.  Format 2 (TSV) with a report, or a report of another
 * pair count, is SCRG_ERR_INVALID_ARG. */
scrg_status scrg_job_write_report(const scrg_job *job, const scrg_result *res, const scrg_diff *diff, const scrg_report *report,
                                  const int64_t costs[4], const char *path, int format);

/* scrg_job_write's records for a result of clipped alignments (scrooge_amd.h, SOFT CLIPPING; `clip` as scrg_ctx_take_clip handed it
 * over after the call that made `res`, whose runs and text are those of the kept stretches).
 *   SAM: the CIGAR is "<read_start>S", the pair's text, "<read_len - read_end>S" (a clip of length 0 is left out), POS is moved by
 *        text_start, and the tags are NM:i:<n_edits> — the edits of the kept stretch, not the full alignment's distance — and
 *        AS:i:<score>.  A pair of which nothing is kept is written unmapped, as a pair over the edit limit is.
 *   PAF: query start and end and target start and end come from the record — the query interval on the read's FORWARD strand, as
 *        PAF wants it: [read_len - read_end, read_len - read_start) for a minus-strand candidate — the match and column counts from
 *        the kept runs; NM:i:<n_edits>, cg:Z: and AS:i:<score>.  A pair of which nothing is kept is left out.
 * clip == NULL is scrg_job_write exactly.  Format 2 (TSV) with a clip, or a clip of another pair count, is SCRG_ERR_INVALID_ARG. */
scrg_status scrg_job_write_clipped(const scrg_job *job, const scrg_result *res, const scrg_clip *clip, const char *path, int format);

/* The clip record of ONE pair's runs on the host (no GPU, no handle), by the rule of scrooge_amd.h (SOFT CLIPPING): what the device
 * pass writes, stated apart from it — for callers with joined anchored results and for the CPU tests.  costs: match, mismatch,
 * gap_open, gap_extend (NULL: 2, 4, 4, 2).  A list with a zero count or an operation other than = X I D is not looked at: SCRG_OK and
 * an all-zero record.  SCRG_ERR_INVALID_ARG: a NULL it needs, costs out of range, 2^32 runs and more, or runs that consume so many
 * bases that (read + text) * max(match, mismatch, gap_open + gap_extend) reaches 2^31. */
scrg_status scrg_clip_from_runs(const scrg_run *runs, uint64_t n_runs, const int32_t costs[4], scrg_pair_clip *out);

/* ONE alignment added to a pileup on the host (no GPU, no handle), by the rule of scrooge_amd.h (PILEUP): what the device pass sums,
 * stated apart from it — for callers with joined anchored results and for the CPU tests.  counts: [7][target_len + 1] in COUNTS
 * form (what scrg_pileup_finish and scrg_ctx_take_pileup give; not the edge form of a device accumulator), added to.
 * read_aligned: ASCII, the read AS ALIGNED (of a reverse-strand candidate the reverse complement), either case; only bases under
 * 'X' are looked at.  *out_of_range (may be NULL) is incremented if a column or an insertion lay outside the target.  It validates
 * first: SCRG_ERR_INVALID_ARG, and nothing added, for a NULL it needs, a zero count, an operation other than = X I D, a read
 * shorter than the runs consume, or a base under 'X' other than ACGTacgt. */
scrg_status scrg_pileup_from_runs(const scrg_run *runs, uint64_t n_runs, const char *read_aligned, uint64_t read_len,
                                  uint64_t target_start, uint64_t target_len, uint32_t *counts, uint64_t *out_of_range);

/* A pileup (`pileup` as scrg_ctx_take_pileup handed it over after calls on this job's genome) as a TSV: a header line, then one row
 * per genome position whose depth — match + A + C + G + T + del — is at least max(min_depth, 1):
 *   chrom  pos (1-based)  ref  depth  match  A  C  G  T  del  ins
 * chromosome (its name up to the first blank) and position as scrg_job_write has them for a candidate's start; ins counts the
 * insertions in front of the position.  A pileup whose target_len is not the job's genome length is SCRG_ERR_INVALID_ARG. */
scrg_status scrg_job_write_pileup(const scrg_job *job, const scrg_pileup *pileup, const char *path, uint64_t min_depth);

/* The sites of a pileup on the host (no GPU, no handle), by the rule of scrooge_amd.h (PILEUP SITES) — the text the device passes
 * compile, site_rule.h — for callers who have the counts on the host already and for the CPU tests.  counts: [7][target_len + 1]
 * in COUNTS form; genome_ascii: the target's target_len bases, either case.  out: up to cap records in ascending pos; *n_sites
 * (may be NULL) is the number of sites either way.  out == NULL only counts.  cap < the number of sites is
 * SCRG_ERR_CIGAR_OVERFLOW, and nothing is written to out.  A genome base outside ACGTacgt is SCRG_ERR_BAD_BASE;
 * SCRG_ERR_INVALID_ARG: a rule that is refused, target_len >= 2^32 - 1, a NULL that is needed. */
scrg_status scrg_pileup_sites_from_counts(const uint32_t *counts, uint64_t target_len, const char *genome_ascii,
                                          const scrg_site_rule *rule, scrg_site *out, uint64_t cap, uint64_t *n_sites);

/* Paired-end mapping of a loaded job (scrooge_amd.h, MATE PAIRS): the job's reads 2m and 2m+1 are mates — an interleaved FASTQ —,
 * its genome is made resident on the handle (scrg_genome_set) and scrg_align_mapping_paired runs on it; rule, *mates and *out as
 * there.  An odd number of reads is SCRG_ERR_FORMAT, and *mates and *out stay NULL. */
scrg_status scrg_job_align_paired(scrg_ctx *ctx, const scrg_params *params, const scrg_job *job, const scrg_mate_rule *rule,
                                  scrg_mates **mates, scrg_result **out);

/* A paired result as a file (`res` and `mates` as scrg_job_align_paired made them).  format 1, SAM: one record per read, as
 * best-candidate mode's — the winner of its side, or an unmapped record — with the pair's columns:
 *   FLAG  0x1; 0x40 for read 2m, 0x80 for read 2m+1; 0x2 from SCRG_MATES_PROPER, CLEARED where the two winners lie on different
 *         chromosomes (the rule sees the job's one concatenated coordinate); 0x4 / 0x8 this read / its mate has no winner; 0x10 /
 *         0x20 this read's / its mate's winner is a reverse-strand candidate;
 *   RNEXT, PNEXT  the mate's winner: "=" on the same chromosome, else its name, and its 1-based start; "*" and 0 without one.  (An
 *         unmapped read keeps RNAME "*" and POS 0 and names its mate's chromosome in RNEXT);
 *   TLEN  from the two winners' CIGARs: the leftmost start to the rightmost end (start + the text bases the alignment consumed),
 *         positive for the mate that starts leftmost — equal starts: read 2m —, negative for the other; 0 when a mate has no
 *         winner or lies on another chromosome;
 *   MAPQ  0 with SCRG_MATES_TIED, 255 otherwise; NM:i: the winner's edit distance.
 * format 0, PAF: the winners only, as best-candidate mode writes them (tp:A:P).  SCRG_ERR_INVALID_ARG: another format, a
 * distance-only result, records that are not this job's (their number, a winner that is no pair of its read). */
scrg_status scrg_job_write_paired(const scrg_job *job, const scrg_result *res, const scrg_mates *mates, const char *path, int format);

/* The choice of ONE mate pair on the host (no GPU, no handle), by the rule of scrooge_amd.h (MATE PAIRS) — the text the device pass
 * compiles, mate_rule.h — for callers who have the distances on the host already and for the CPU tests.  Side A has n_a candidates
 * (start_a, rev_a — may be NULL: all forward —, ed_a, status_a — a result's pair_status; may be NULL: all eligible — and the read's
 * length len_a), side B likewise.  *record: winner[0] / winner[1] are indices into side A's / side B's arrays (UINT64_MAX: none);
 * is_best_a / is_best_b (may be NULL) get 1/0 per candidate.  rule == NULL is the default (FR, any span, penalty 0).
 * SCRG_ERR_INVALID_ARG, and nothing written: a rule that is refused, n_a x n_b >= 2^32, a NULL that is needed. */
scrg_status scrg_mates_from_distances(const scrg_mate_rule *rule,
                                      uint64_t n_a, const uint64_t *start_a, const uint8_t *rev_a, const int64_t *ed_a,
                                      const uint32_t *status_a, uint64_t len_a,
                                      uint64_t n_b, const uint64_t *start_b, const uint8_t *rev_b, const int64_t *ed_b,
                                      const uint32_t *status_b, uint64_t len_b,
                                      scrg_mate_record *record, uint8_t *is_best_a, uint8_t *is_best_b);

/* The read summaries and MAPQs on the host (no GPU, no handle), by the rule of scrooge_amd.h (READ SUMMARY AND MAPPING QUALITY) —
 * the text the device pass compiles, mapq_rule.h, applied read by read and candidate by candidate — for callers who have the
 * distances on the host already and for the CPU tests.  The arguments are scrg_read_summary's on host memory: first[r]
 * (n_reads + 1 entries, non-decreasing) is the index of read r's first pair; read_len (the pair's read's length), edit_distance
 * and pair_status (a result's, in its codes: SCRG_PAIR_OVER_EDIT_LIMIT is not eligible; may be NULL: all eligible) are per pair; out[r] is read r's record, winner as an index into these
 * arrays; keep_status (may be NULL; needs pair_status) is pair_status with every status-0 pair that is not the winner of a KEPT read
 * as SCRG_PAIR_NOT_BEST.  rule == NULL is the default.  SCRG_ERR_INVALID_ARG, and nothing written: a rule that is refused,
 * offsets that run backwards or reach 2^32, a NULL that is needed. */
scrg_status scrg_read_summary_from_distances(const scrg_mapq_rule *rule, uint64_t n_reads, const uint64_t *first,
                                             const uint32_t *read_len, const int64_t *edit_distance, const uint32_t *pair_status,
                                             scrg_read_record *out, uint32_t *keep_status);

/* The merge of two partial summaries of one read (mapq_rule.h: mapq_merge, the function the kernel's lanes call), for bindings and
 * for the tests that hold it associative and commutative.  A part is four words: best = (edit distance << 32) | pair index
 * (UINT64_MAX: no eligible candidate seen), n_tied, second_ed (UINT32_MAX: none), n_eligible.  out may be a or b. */
scrg_status scrg_read_summary_merge(const uint64_t a[4], const uint64_t b[4], uint64_t out[4]);

/* scrg_job_write_report's lines with the mapping quality in them (`summary` as scrg_ctx_take_read_summary handed it over after
 * the call that made `res`, a result of best-candidate mode): SAM column 5 of a read's winner record and PAF column 12 are
 * summary->reads[r].mapq instead of 0 / 255; an unmapped SAM record keeps 0.  diff, report and costs as there (any may be NULL).
 * summary == NULL is scrg_job_write_report exactly, byte for byte.  SCRG_ERR_INVALID_ARG: a summary whose n_reads is not the job's,
 * a result that is not best-candidate mode's for these summaries (a read with two pairs that are neither SCRG_PAIR_NOT_BEST nor
 * over the limit, a winner other than the summary's), format 2 (TSV). */
scrg_status scrg_job_write_mapq(const scrg_job *job, const scrg_result *res, const scrg_diff *diff, const scrg_report *report,
                                const int64_t costs[4], const scrg_read_summaries *summary, const char *path, int format);

/* Sites (`sites` as scrg_ctx_take_pileup_sites handed them over, or made by scrg_pileup_sites_from_counts, of this job's genome)
 * as a TSV: a header line, then one row per site:
 *   chrom  pos (1-based)  ref  depth  match  A  C  G  T  del  ins  alt  call  flags
 * the first eleven columns as scrg_job_write_pileup has them; alt and call are A C G T, * for deleted, . for none; flags is the
 * decimal SCRG_SITE_F_* word.  Sites whose target_len is not the job's genome length, or a pos outside it, are
 * SCRG_ERR_INVALID_ARG. */
scrg_status scrg_job_write_sites(const scrg_job *job, const scrg_pileup_sites *sites, const char *path);

/* The difference string of ONE pair on the host (no GPU, no handle), by the rules of scrooge_amd.h (DIFFERENCE STRINGS): for
 * callers with joined anchored results, whose strings the device does not make, and for the CPU tests.  text / read: ASCII, the
 * read AS ALIGNED (either case; MD is written in upper, cs in lower case); only the bases the runs name are looked at.
 * *len = the string's length incl. its NUL.  buf == NULL only measures; otherwise the string goes to buf if cap >= *len, else
 * SCRG_ERR_CIGAR_OVERFLOW and buf is not written.  SCRG_ERR_INVALID_ARG: another kind, a zero count, an operation other than
 * = X I D, or runs that consume more text or more read than there is. */
scrg_status scrg_diff_from_runs(int32_t kind, const char *text, uint64_t text_len, const char *read, uint64_t read_len,
                                const scrg_run *runs, uint64_t n_runs, char *buf, uint64_t cap, uint64_t *len);

/* The CIGAR text of ONE pair's runs on the host (no GPU, no handle) in a form of scrooge_amd.h (CIGAR FORMS): SCRG_CIGAR_WINDOWED,
 * SCRG_CIGAR_MERGED or SCRG_CIGAR_M — what the device kernels write, stated apart from them; scrg_align_mapping_anchored renders its
 * joined runs with it.  *len = the string's length incl. its NUL.  buf == NULL only measures; otherwise the string goes to buf if
 * cap >= *len, else SCRG_ERR_CIGAR_OVERFLOW and buf is not written.  SCRG_ERR_INVALID_ARG: another form, a zero count, or an
 * operation other than = X I D. */
scrg_status scrg_cigar_from_runs(int32_t form, const scrg_run *runs, uint64_t n_runs, char *buf, uint64_t cap, uint64_t *len);

/* The alignment report of ONE pair on the host (no GPU, no handle), by the rules of scrooge_amd.h (ALIGNMENT REPORT), on ASCII: for
 * callers with joined anchored results and for the CPU tests.  text / read: the sequences AS ALIGNED, either case.  A finding is
 * not an error: SCRG_OK with out->verdict set; SCRG_ERR_INVALID_ARG only for a NULL it needs or 2^32 runs and more. */
scrg_status scrg_report_from_runs(const char *text, uint64_t text_len, const char *read, uint64_t read_len,
                                  const scrg_run *runs, uint64_t n_runs, int64_t edit_distance, scrg_pair_report *out);
/* match * n_match - mismatch * n_mismatch - open * n_gap_open - extend * (n_ins + n_del): scrg_affine_score of the pair's CIGAR,
 * without the CIGAR.  SCRG_ERR_INVALID_ARG for a record whose counts do not cover its runs (a verdict other than 0, 6 and the 3 met
 * after the last run). */
scrg_status scrg_report_score(const scrg_pair_report *report, int64_t match_bonus, int64_t mismatch_cost,
                              int64_t gap_open_cost, int64_t gap_extend_cost, int64_t *score);

/* Affine re-scoring of a CIGAR exactly as get_alignment_score (src/cpu_baseline.cpp:694-725):
 * +match per '=', -mismatch per 'X', -(open + extend*len) per maximal I/D stretch
 * (consecutive I and D runs share one opening). */
scrg_status scrg_affine_score(const char *cigar, int64_t match_bonus, int64_t mismatch_cost,
                              int64_t gap_open_cost, int64_t gap_extend_cost, int64_t *score);

/* validateCigarString (src/tests.cu:27-169).  Returns SCRG_OK, or SCRG_ERR_FORMAT and a
 * reason code in *why: 1 malformed, 2 zero-length run, 3 read not consumed exactly,
 * 4 runs past the text, 5 '='/'X' disagrees with the sequences, 6 edit count != edit_distance. */
scrg_status scrg_validate_alignment(const char *text, uint64_t text_len, const char *read, uint64_t read_len,
                                    const char *cigar, int64_t edit_distance, int32_t *why);

#ifdef __cplusplus
}
#endif
#endif
