/*
 * scrooge_amd.h — C ABI of the MI355X-native GenASM/Scrooge aligner.
 *
 * This is the drop-in boundary for Scrooge's GPU library surface
 * (reference: src/genasm_gpu.hpp:5-10, implemented in src/genasm_gpu.cu:890-1065):
 *
 *   genasm_gpu::align_all(vector<string>& texts, vector<string>& queries, long long* ns)
 *       -> scrg_align_pairs()
 *   genasm_gpu::align_all(Genome_t&, vector<Read_t>&, long long* ns)
 *       -> scrg_align_mapping()
 *   __global__ genasm_gpu::ascii_to_twobit_strings(count, lens, ascii, twobit)
 *       -> scrg_ascii_to_twobit()          (same byte layout, src/genasm_gpu.cu:631-685; the kernel itself, with the
 *                                           reference's signature, is in include/compat/genasm_gpu.hpp for hipcc-compiled
 *                                           callers: both are made of include/scrooge_amd_device.hpp)
 *   genasm_gpu::enabled_algorithm_log
 *       -> scrg_set_log() / scrg_get_log()
 *
 * include/scrooge_amd.hpp rebuilds the reference's C++ signatures on top of
 * these entry points.  Everything here is plain pointers and sizes; the
 * library owns no torch/STL types at the boundary.  Unlike the reference
 * (exit()/assert on every error) every entry point returns a
 * status code.
 *
 * Algorithm contract: results (edit distance and CIGAR) are bit-identical to
 * the reference CPU path src/genasm_cpu.cpp:178-438 at the same W and O with
 * K = W; CIGAR runs are flushed per window and never merged across windows
 * (src/genasm_cpu.cpp:304-305, 400-403).
 */
#ifndef SCROOGE_AMD_H
#define SCROOGE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t scrg_status;
enum {
    SCRG_OK = 0,
    SCRG_ERR_INVALID_ARG = 1,   /* null pointer, W/O out of range, ...              */
    SCRG_ERR_BAD_BASE = 2,      /* non-ACGT/acgt input (reference: assert, genasm_cpu.cpp:487-489) */
    SCRG_ERR_NO_DEVICE = 3,     /* no usable gfx950 device / HIP runtime failure at init */
    SCRG_ERR_HIP = 4,           /* a HIP call failed; see scrg_last_error()         */
    SCRG_ERR_OOM = 5,           /* host or device allocation failed                 */
    SCRG_ERR_CIGAR_OVERFLOW = 6, /* a pair produced more runs than its arena slice  */
    SCRG_PAIR_OVER_EDIT_LIMIT = 7, /* pair status only (scrg_result.pair_status): the pair went over the handle's
                                     edit limit (scrg_ctx_set_edit_limit) and has no alignment; not an error */
    SCRG_PAIR_NOT_BEST = 8        /* pair status only: best-candidate mode (SCRG_OUT_BEST) — the pair was aligned in full, its
                                     edit distance is delivered, but another candidate of its read won; not an error */
};

/* Tunables.  Zero-initialise and call scrg_params_default(). */
typedef struct scrg_params {
    int32_t W;               /* window length, 2..256; reference default 64 (genasm_cpu.cpp:7).
                                W > 64 uses multi-word vectors (src/bitvector.hpp:45-48)           */
    int32_t O;               /* window overlap, 0 <= O < W and W-O <= 255 (a run count is one byte: W = 256 with O = 0 is
                                SCRG_ERR_INVALID_ARG; O = 0 needs lanes_per_pair = 1); reference default 33 (genasm_cpu.cpp:9).
                                W <= 64 with W-O <= 31 (e.g. the defaults) keeps the traceback table in 62 registers;
                                32 <= W-O <= 63 with W <= 128 in 128 registers, built in two halves of 32 columns;
                                beyond that the table rows are 128 to 256 bits wide and kept in HBM                */
    int32_t lanes_per_pair;  /* 1 = one pair per lane, 64 pairs per wavefront (the default for every W);
                                64 = one pair per wavefront (lane = text column); 4/8/16/32 pack 64/lanes
                                pairs into one wavefront (GenASM rows; for W > 64 only 32 and 64 exist).
                                0 = default                                                          */
    int32_t lds_rows;        /* rows of the R table kept in LDS per pair (rest spills to HBM);
                                0 = default                                                        */
    int32_t waves_per_cu;    /* persistent wavefronts launched per CU; 0 = default (as many as fit, at most one per 64
                                pairs).  A batch of MIXED read lengths issued longest first balances better with
                                fewer wavefronts than groups of 64 pairs — the work queue then hands the short pairs
                                at the end of the order to the lanes that finish first: 4 (one per SIMD) is +12 % on
                                100 k pairs of 2 .. 20 kb (bench.py other_configs); equal lengths: leave 0           */
    int32_t sort_by_length;  /* host entry points: issue pairs longest-read-first (the reference's
                                callers do this themselves, src/tests.cu:375-377); results keep
                                input order either way.  Default 1                                 */
    int32_t text_stride_words; /* device-pointer entry points: distance, in 64-bit words, between consecutive
                                words of one text in d_seq.  0 or 1 = contiguous; 64 = the lane-interleaved
                                layout of scrg_pack_planar_groups() (see there).  Only lanes_per_pair = 1
                                accepts a stride other than 1                                        */
    int32_t read_stride_words; /* the same for the reads                                             */
    int32_t outputs;         /* host entry points: what the result holds — SCRG_OUT_ALL (0, default): runs and text;
                                SCRG_OUT_TEXT: the CIGAR text only (runs stays empty, run_offset all zero);
                                SCRG_OUT_RUNS: the runs only (cigar_text stays empty, cigar_offset all zero).
                                What is not asked for does not cross PCIe.
                                | SCRG_OUT_BEST (4; mapping calls only, see scrg_result): of every read's candidates only
                                the best keeps its runs and text — chosen on the device, before anything is compacted,
                                rendered or transferred.
                                SCRG_OUT_DISTANCE (16; every host entry point, see scrg_result): distance-only mode — edit
                                distance, status and text end of every pair, no runs and no text: nothing is written,
                                compacted, rendered or transferred for them, and no CIGAR storage exists on the device.  A
                                flag that excludes 1 and 2 and combines with SCRG_OUT_BEST (20).
                                Valid values: 0, 1, 2, 4, 5, 6, 16, 20                                                */
    int32_t reserved[2];     /* must be 0: the shipped library rejects every bit of both with SCRG_ERR_INVALID_ARG, so an
                                uninitialised struct cannot silently change anything.  (Other BUILDS of the same sources
                                give them a meaning — the test build, -DSCRG_SELECT, selects between formulations that give
                                identical results; profiling builds add counters and ablations: see scrg_debug_stats.)   */
    int32_t stranded;        /* device-pointer entry points (ABI 7): 1 = bit 63 of scrg_pair_desc.read_off (SCRG_READ_REVCOMP) marks
                                a pair whose read is aligned as its REVERSE COMPLEMENT, taken from the one packed copy of the read
                                (a read-mapping candidate on the minus strand; the reference drops those, src/tests.cu:346-355).
                                Served by the one-pair-per-lane kernels (lanes_per_pair = 1, the default, at every W and O);
                                SCRG_ERR_INVALID_ARG for the GenASM-row mappings.  0 (default): bit 63 must be clear      */
} scrg_params;
#define SCRG_READ_REVCOMP (1ull << 63)

enum { SCRG_OUT_ALL = 0, SCRG_OUT_TEXT = 1, SCRG_OUT_RUNS = 2, SCRG_OUT_BEST = 4 /* a flag, OR-ed onto one of the three */,
       SCRG_OUT_DISTANCE = 16 /* a flag: alone, or with SCRG_OUT_BEST */ };

void scrg_params_default(scrg_params *p);
/* Fills in every 0 ("default") field for the given W/O and validates; the values a launch will use. */
scrg_status scrg_params_resolve(const scrg_params *in, scrg_params *out);

/* One CIGAR run, layout-compatible with the reference's CigarEntry_t
 * (src/util.hpp:43-46). */
typedef struct scrg_run {
    uint8_t count;
    char    op;     /* one of '=', 'X', 'I', 'D' */
} scrg_run;

/* Per-device handle: owns a HIP stream, the work counter and scratch.  One
 * handle may be used by one thread at a time; separate handles are independent
 * (the reference's GPU path is not re-entrant at all, genasm_gpu.cu:582). */
typedef struct scrg_ctx scrg_ctx;

scrg_status scrg_ctx_create(int device, scrg_ctx **out);
void        scrg_ctx_destroy(scrg_ctx *ctx);
/* Enqueue on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the handle's own.  NULL is a valid value: the device's default (null) stream.
 * scrg_ctx_use_own_stream() goes back to the handle's private stream. */
scrg_status scrg_ctx_set_stream(scrg_ctx *ctx, void *hip_stream);
scrg_status scrg_ctx_use_own_stream(scrg_ctx *ctx);

/* EDIT LIMIT: "only alignments with at most k edits" (Edlib's k, KSW2's z-drop).  For a pair with read length L the limit is
 *     lim = min(max_edits, floor(per_mille * L / 1000))
 * where a part that is off drops out of the min; with both off (the default) there is none.  A pair is over the limit exactly
 * when its full edit distance exceeds lim.  The kernels check after every window: the running sum of the windows' edits
 * (what the reference adds up, genasm_cpu.cpp:432) never goes down, so the pair is retired at the FIRST window end where the
 * sum exceeds lim — its remaining windows are not computed and its lane takes the next pair at once.  Such a pair reports
 *     status SCRG_PAIR_OVER_EDIT_LIMIT (host entry points; 2 in d_pair_status of the device-pointer ones),
 *     edit distance = that running sum (> lim, and <= the full distance), no runs: n_runs 0, CIGAR text "", and with
 *     edit-stream output d_stream_len 0 and d_n_runs 0
 * (also when its last window both finishes the read and crosses the limit).  A pair within the limit is bit for bit what it is
 * without one.  The setting belongs to the handle and applies to every align call on it: scrg_align_device,
 * scrg_align_device_edits, scrg_align_device_distance, scrg_align_pairs, scrg_align_mapping[_stranded|_resident] and scrg_job_align; the _multi calls
 * have no handle and align without a limit.  With a limit set, lanes_per_pair != 1 (the GenASM-row mappings) is
 * SCRG_ERR_INVALID_ARG.  Over-limit pairs do not make a call fail (strict bindings do not raise for them).
 *   max_edits < 0: none (0 is a limit: only exact matches);  per_mille 0: none, 1..1000 otherwise (else SCRG_ERR_INVALID_ARG) */
scrg_status scrg_ctx_set_edit_limit(scrg_ctx *ctx, int64_t max_edits, int32_t per_mille);
scrg_status scrg_ctx_get_edit_limit(const scrg_ctx *ctx, int64_t *max_edits, int32_t *per_mille);    /* -1 / 0: off */
/* The per-pair arithmetic above on the host (no handle, no GPU): *limit = lim for a read of read_len bases, -1 = no limit.
 * SCRG_ERR_INVALID_ARG for a per_mille outside 0..1000 or a NULL limit. */
scrg_status scrg_edit_limit_for(int64_t max_edits, int32_t per_mille, uint64_t read_len, int64_t *limit);

/* TEXT STRANDS: "align against the reverse complement of this stretch", from the ONE packed copy of the text (what extending
 * LEFTWARDS from a seed needs: aligning a read so that it ends at a genome position and grows to the left is aligning its
 * reverse complement against the reverse complement of the genome prefix).  With the setting enabled, bit 63 of
 * scrg_pair_desc.text_off (SCRG_TEXT_REVCOMP) marks such a pair: text_off (the bit cleared) and text_len still name a FORWARD
 * stretch of d_seq, and character k of the text the pair is aligned against is the complement of base
 * text_off + text_len - 1 - k.  A flagged pair reads no word below the first word of its stretch (text_off = 0, the genome's
 * beginning, is the normal case) and nothing past what a forward pair may read (SCRG_SEQ_PAD_WORDS[_STRIDED]); of a stretch
 * longer than 2^32 - 1 bases the LAST 2^32 - 1 are the reachable ones.  It composes per pair with SCRG_READ_REVCOMP, in every
 * one-pair-per-lane kernel, at every W and O, both sequence layouts and all three output modes.  The setting belongs to the
 * handle and applies to every align call on it (scrg_align_device, _edits, _distance and the host calls); with it enabled,
 * lanes_per_pair != 1 (the GenASM-row mappings) is SCRG_ERR_INVALID_ARG in all of them.  (The host calls write their pairs'
 * descriptors themselves — the bit is set for leftward candidates only, scrg_align_mapping_directed —, so for them the
 * setting changes nothing but that rejection.)  Disabled (the default): bit 63 is not looked at,
 * and nothing changes for anybody.  New entry points only: SCRG_ABI_VERSION stays. */
#define SCRG_TEXT_REVCOMP (1ull << 63)
scrg_status scrg_ctx_set_text_strands(scrg_ctx *ctx, int enabled);   /* default 0 */
scrg_status scrg_ctx_get_text_strands(const scrg_ctx *ctx, int *enabled);
/* The kernels' text load on the host (no GPU, no handle; the address arithmetic is the same code, compiled for the host): the
 * planes of the window of W characters at character ref_idx of the text (text_off — bit 63 honoured —, text_len), from a planar
 * array of n_words words whose words of one sequence are stride_words apart (0 = 1).  lo / hi: (W + 63) / 64 words each, bit k
 * of word w = the low / high code bit of text character ref_idx + 64 w + k; only the bits of characters inside the text
 * (fewer than min(W, text_len - ref_idx)) are defined.  *first_word / *last_word (may be NULL): the lowest and highest word
 * index the load touched (~0 and 0 if it touched none: a window past the text).  SCRG_ERR_INVALID_ARG if it would touch a
 * word at or past n_words — nothing is read then —, for W outside 1..256 or ref_idx > min(text_len, 2^32 - 1). */
scrg_status scrg_text_window_planes(const uint64_t *planar, uint64_t n_words, uint64_t text_off, uint64_t text_len,
                                    uint64_t ref_idx, int32_t W, uint64_t stride_words, uint64_t *lo, uint64_t *hi,
                                    uint64_t *first_word, uint64_t *last_word);

/* DIFFERENCE STRINGS: SAM's MD:Z: (SCRG_DIFF_MD, upper case) or PAF's short cs:Z: (SCRG_DIFF_CS, lower case) of every pair, made
 * on the device from the pair's runs and the two packed sequences, next to the CIGAR text.  A pair's alignment is its runs in
 * order, as the result holds them (never merged across windows: "29=21=" has MD "50"); t and q are the positions in the text and
 * in the read AS ALIGNED (a minus-strand pair's read is its reverse complement; text bases are the forward text's).
 *   MD  a number, then one item and a number for every mismatched base and every maximal stretch of deleted bases.  The item of
 *       an 'X' base is the text base; the item of a stretch of directly adjacent 'D' runs is '^' and its text bases; each number
 *       is the count of '=' bases since the previous item (or the start).  Insertions are not written: they neither add to a
 *       number nor reset it.  The string begins and ends with a number, which may be 0:  4=1X2=1D2= -> "4A2^T2".
 *   cs  ":n" for a maximal stretch of n '=' bases (adjacent '=' runs merge; no ":0"), "*tq" per 'X' base (text base, read base),
 *       "+bases" per maximal stretch of adjacent 'I' runs (read bases), "-bases" per maximal stretch of adjacent 'D' runs (text
 *       bases):  4=1X2=1D2= -> ":4*at:2-t:2".
 * A pair without runs (an empty read, over the edit limit, not its read's best) has "" in both kinds; a pair whose slice
 * overflowed has the string of the runs its result holds.  Strings are NUL-terminated and a pair's length includes the NUL, as for cigar_text.
 *
 * The setting belongs to the handle, as the edit limit does: with a kind set, scrg_align_pairs, scrg_align_mapping[_stranded|
 * _resident], scrg_job_align and scrg_align_mapping_directed without a leftward candidate also render every pair's string in
 * the chunk pipeline, bring the strings back and keep them on the handle, in the caller's order whatever the chunking and
 * sort_by_length.  scrg_ctx_take_diff hands them over ONCE (release with scrg_diff_free); a second take, or a take after a call
 * that failed, is SCRG_ERR_INVALID_ARG with *out = NULL, and the next align call discards strings nobody took.  It works with
 * outputs 0, 1, 2 and | SCRG_OUT_BEST (losers: ""), and with an edit limit (pairs over it: ""); what `outputs` sends back is
 * unchanged.  While a kind is set, SCRG_OUT_DISTANCE, leftward candidates, scrg_align_mapping_anchored and lanes_per_pair != 1
 * are SCRG_ERR_INVALID_ARG (joined pairs: scrg_diff_from_runs, scrooge_amd_io.h).  The _multi calls have no handle and are not
 * served.  Off (the default): nothing changes for anybody.  New entry points only: SCRG_ABI_VERSION stays. */
enum { SCRG_DIFF_OFF = 0, SCRG_DIFF_MD = 1, SCRG_DIFF_CS = 2 };
typedef struct scrg_diff {
    uint64_t  n_pairs;
    int32_t   kind;           /* SCRG_DIFF_MD or SCRG_DIFF_CS                             */
    uint64_t *offset;         /* [n_pairs+1] into text (each string NUL-terminated)      */
    char     *text;
} scrg_diff;
scrg_status scrg_ctx_set_diff(scrg_ctx *ctx, int32_t kind);          /* default SCRG_DIFF_OFF */
scrg_status scrg_ctx_get_diff(const scrg_ctx *ctx, int32_t *kind);
scrg_status scrg_ctx_take_diff(scrg_ctx *ctx, scrg_diff **out);
void        scrg_diff_free(scrg_diff *d);

/* CIGAR FORMS: the form in which a pair's CIGAR TEXT is written.  The runs of a result are what the windows of the alignment left:
 * flushed at every window end and never merged ("29=21=31=..." is a normal alignment, "31I13I16=2I2I" a normal answer).  The text
 * may be written in a form that the rest of a tool chain expects instead; the runs themselves are never touched.
 *   SCRG_CIGAR_WINDOWED  (the default) "%d%c" per run: the text exactly as the reference writes it.
 *   SCRG_CIGAR_MERGED    adjacent equal operations merged, as the SAM specification recommends:   29=21= -> 50=
 *   SCRG_CIGAR_M         as MERGED, with '=' and 'X' both written 'M':                       4=1X2=1D2= -> 7M1D2M
 * The class of a run is its operation (= X I D) under MERGED; under M, '=' and 'X' have class 'M' and 'I' and 'D' keep theirs.  The
 * text of a pair is, for every maximal stretch of directly adjacent runs of one class, the decimal sum of their counts (held in 64
 * bits, no leading zeros) and the class letter; a stretch may span any number of windows.  A pair without runs has "".  Strings are
 * NUL-terminated and a pair's length includes the NUL, as for the windowed text.
 * LENGTH INVARIANT: a pair's merged or M text is never longer than its windowed text (the digits of a sum are no more than the
 * digits of its terms together, and every run joined saves a letter), so every capacity derived from run counts holds in every form.
 *
 * The setting belongs to the handle.  It applies to every call that renders text in the chunk pipeline — scrg_align_pairs,
 * scrg_align_mapping[_stranded|_resident|_directed], scrg_job_align — whatever the kernel family, outputs (1, 2, | SCRG_OUT_BEST),
 * edit limit, strands, chunking and sort_by_length, and to the text scrg_align_mapping_anchored makes from the joined runs (an
 * identical read is then one "L=" across the seam).  Pairs without runs keep "".  With SCRG_OUT_RUNS or SCRG_OUT_DISTANCE there is
 * no text and the setting has no effect; it is no error.  What stays as it is: the result's runs, run_offset, edit_distance and
 * pair_status — so under MERGED and M, cigar_text and cigar_offset are no longer the runs printed one by one.  Whoever needs the
 * window ends (the edit-stream encoders) takes the runs.  The _multi calls have no handle and are not served.  Any other value is
 * SCRG_ERR_INVALID_ARG.  New entry points only: SCRG_ABI_VERSION stays. */
enum { SCRG_CIGAR_WINDOWED = 0, SCRG_CIGAR_MERGED = 1, SCRG_CIGAR_M = 2 };
scrg_status scrg_ctx_set_cigar_form(scrg_ctx *ctx, int32_t form);    /* default SCRG_CIGAR_WINDOWED */
scrg_status scrg_ctx_get_cigar_form(const scrg_ctx *ctx, int32_t *form);

/* ALIGNMENT REPORT: per pair, what almost every caller walks the runs for again on the host — the bases under each operation,
 * the gap openings an affine score charges, the indel stretches a gap-compressed divergence counts — and a VERDICT: is this list
 * of runs an alignment of these two sequences with this edit distance.  Made on the device in one pass over the finished runs,
 * the two packed sequences and the edit distance (report_kernels.hip); no align kernel is touched.
 *
 * The walk.  The verdict is defined on the runs, in order, exactly as scrg_validate_alignment (scrooge_amd_io.h) walks the
 * rendered text; t and q are the positions in the text and in the read AS ALIGNED (a SCRG_READ_REVCOMP read is its reverse
 * complement, a SCRG_TEXT_REVCOMP text the reverse complement of its stretch — leftward texts ARE served).  Per run: count 0 -> 2
 * (checked before the operation); an operation other than = X I D -> 1; '=' / 'X': past the read -> 3, then past the text -> 4,
 * then any base whose equality disagrees with the operation -> 5; 'I': past the read -> 3; 'D': past the text -> 4.  After the
 * last run: read not consumed exactly -> 3, then n_mismatch + n_ins + n_del != edit distance -> 6.  The first failure in run
 * order wins.  Bases are compared as 2-bit codes (case-blind, as the host check is).
 * The six counts cover ALL of the pair's runs when the verdict is 0, 6, or the 3 met after the last run (a slice that overflowed
 * holds a truncated alignment: that 3, at bad_run = cigar_cap, with the counts of what it holds); they are all 0 otherwise.
 * A pair without an alignment (over the edit limit, not its read's best) has verdict SCRG_REPORT_NO_ALIGNMENT and zeros; an empty
 * read with status OK and no runs has verdict 0.  A pair whose read_off carries SCRG_READ_REVCOMP without params.stranded, or
 * whose text_off carries SCRG_TEXT_REVCOMP without text strands enabled on the handle, has verdict 1 at bad_run 0, and none of
 * its bases is read. */
typedef struct scrg_pair_report {          /* 32 bytes */
    uint32_t n_match, n_mismatch, n_ins, n_del;  /* bases under '=', 'X', 'I', 'D' */
    uint32_t n_gap_open;  /* maximal stretches of directly adjacent I/D runs; I and D share one: the openings scrg_affine_score charges */
    uint32_t n_indel;     /* maximal stretches of directly adjacent runs of the SAME op I or D: what cs writes as one '+' / '-' item */
    uint32_t verdict;     /* 0 ok; 1..6 = scrg_validate_alignment's *why; 7 = SCRG_REPORT_NO_ALIGNMENT */
    uint32_t bad_run;     /* the run at which verdict 1,2,3,4,5 was met; n_runs for "read not consumed" met after the last run and for 6; 0 for 0 and 7 */
} scrg_pair_report;
enum { SCRG_REPORT_NO_ALIGNMENT = 7 };
/* The setting belongs to the handle, as the difference-string kind does: enabled, scrg_align_pairs, scrg_align_mapping[_stranded|
 * _resident], scrg_job_align and scrg_align_mapping_directed — leftward candidates included — also make every pair's record in the
 * chunk pipeline, after best-candidate selection (a loser has SCRG_REPORT_NO_ALIGNMENT), bring the records back (32 bytes per pair)
 * and keep them on the handle, in the caller's order whatever the chunking, sort_by_length and outputs (0, 1, 2, | SCRG_OUT_BEST;
 * what `outputs` returns is unchanged).  scrg_ctx_take_report hands them over ONCE (release with scrg_report_free); a second take,
 * or a take after a call that failed, is SCRG_ERR_INVALID_ARG with *out = NULL, and the next align call discards a report nobody
 * took.  n_failed = the pairs whose verdict is neither 0 nor SCRG_REPORT_NO_ALIGNMENT.  It may be set together with a
 * difference-string kind (whose refusal of leftward candidates then still holds).  While it is set, SCRG_OUT_DISTANCE,
 * scrg_align_mapping_anchored (joined pairs: scrg_report_from_runs, scrooge_amd_io.h) and lanes_per_pair != 1 are
 * SCRG_ERR_INVALID_ARG.  The _multi calls have no handle and are not served.  Off (the default): nothing changes for anybody.
 * New entry points only: SCRG_ABI_VERSION stays. */
typedef struct scrg_report {
    uint64_t          n_pairs;
    scrg_pair_report *pairs;      /* [n_pairs] */
    uint64_t          n_failed;
} scrg_report;
scrg_status scrg_ctx_set_report(scrg_ctx *ctx, int enabled);           /* default 0 */
scrg_status scrg_ctx_get_report(const scrg_ctx *ctx, int *enabled);
scrg_status scrg_ctx_take_report(scrg_ctx *ctx, scrg_report **out);
void        scrg_report_free(scrg_report *r);

/* SOFT CLIPPING: every alignment is end to end in the read, whatever the read's ends look like; a read with an adapter remnant, a
 * chimeric tail or a poor end comes back with a tail of X / I / D noise.  The clip pass keeps, per pair, the stretch of its runs
 * with the best affine score, as minimap2, BWA and every SAM consumer expect it — on the device, in one pass over the finished
 * runs (clip_kernels.hip); no sequence is read and no align kernel is touched.
 *
 * THE RULE (the kernel, scrg_clip_from_runs of scrooge_amd_io.h and the tests' model implement this one).  Costs are
 * {match, mismatch, gap_open, gap_extend}: match in 1..255, the others in 0..255; the default is 2, 4, 4, 2, as for
 * scrg_job_write_report.  For a pair with runs r_0 .. r_{n-1} (count c_k) the prefix score is P_0 = 0, P_{k+1} = P_k + w_k with
 *   w_k = +match * c_k                         for '='
 *   w_k = -mismatch * c_k                      for 'X'
 *   w_k = -gap_extend * c_k                    for 'I' / 'D', and a further -gap_open when k = 0 or r_{k-1} is neither 'I' nor 'D'
 * (directly adjacent I and D runs share one gap opening, exactly as scrg_affine_score and n_gap_open have it).  A kept stretch is
 * a range of WHOLE runs i <= j with op(r_i) = op(r_j) = '='; its score is P_{j+1} - P_i, which is scrg_affine_score of the
 * sub-CIGAR because it begins and ends on '='.  (Inside an '=' run the prefix score only rises, so the best stretch of bases is
 * always a stretch of whole runs.)  The result is the stretch of the greatest score; among stretches of equal score the greatest j
 * wins, then the least i — for each j the earliest i <= j of the least P_i, then the latest j of the greatest score.
 * A pair without an '=' run keeps nothing: n_runs = 0 and an all-zero record.  A pair is NOT LOOKED AT — an all-zero record, and
 * apply mode leaves it as it is — if its status is not OK (over the edit limit, not its read's best, a slice that overflowed) or
 * if one of its runs is no run (a zero count, an operation other than = X I D).  Verdicts are the report's job, not this pass's.
 * Scores are summed in 32 bits: (longest read + longest text) * max(match, mismatch, gap_open + gap_extend) must stay below 2^31;
 * the host entry points refuse a call that does not (SCRG_ERR_INVALID_ARG) before anything is launched. */
typedef struct scrg_pair_clip {      /* 32 bytes */
    uint32_t read_start, read_end;   /* kept read interval [start, end), read AS ALIGNED */
    uint32_t text_start, text_end;   /* kept text interval, text AS ALIGNED */
    uint32_t first_run, n_runs;      /* the kept runs: first_run .. first_run + n_runs - 1; 0 runs: nothing kept */
    int32_t  score;                  /* affine score of the kept stretch; 0 when nothing is kept */
    uint32_t n_edits;                /* bases under X, I, D inside the kept stretch */
} scrg_pair_clip;
/* The setting belongs to the handle, as the report does: enabled (costs NULL: the default), scrg_align_pairs, scrg_align_mapping
 * [_stranded|_resident|_directed] — leftward candidates included — and scrg_job_align run the pass in the chunk pipeline, after
 * best-candidate selection and before the results are laid out, and make the kept stretch the pair's alignment: the result's runs,
 * run_offset, cigar_text and cigar_offset are those of the KEPT stretch, in whatever CIGAR form is set.  edit_distance and
 * pair_status stay what they are — edit_distance is the distance of the FULL end-to-end alignment, not of the kept stretch, whose
 * edits are in the record (n_edits).  The records come back 32 bytes per pair and are kept on the handle, in the caller's order
 * whatever the chunking and sort_by_length.  scrg_ctx_take_clip hands them over ONCE (release with scrg_clip_free); a second take,
 * or a take after a call that failed, is SCRG_ERR_INVALID_ARG with *out = NULL, and the next align call discards records nobody
 * took.  It works with outputs 0, 1, 2 and | SCRG_OUT_BEST and with an edit limit.  While it is set, these are
 * SCRG_ERR_INVALID_ARG for now: SCRG_OUT_DISTANCE (no runs), lanes_per_pair != 1, scrg_align_mapping_anchored, a difference-string
 * kind (its positions would start at 0, not at the kept stretch) and the alignment report (its counts would describe another
 * alignment than the one returned).  The _multi calls have no handle and are not served.  Off (the default): nothing changes for
 * anybody.  New entry points only: SCRG_ABI_VERSION stays. */
typedef struct scrg_clip {
    uint64_t        n_pairs;
    scrg_pair_clip *pairs;        /* [n_pairs] */
    int32_t         costs[4];     /* match, mismatch, gap_open, gap_extend the records were made with */
} scrg_clip;
scrg_status scrg_ctx_set_clip(scrg_ctx *ctx, int enabled, const int32_t costs[4]);     /* default 0; costs NULL: 2, 4, 4, 2 */
scrg_status scrg_ctx_get_clip(const scrg_ctx *ctx, int *enabled, int32_t costs[4]);    /* either may be NULL */
scrg_status scrg_ctx_take_clip(scrg_ctx *ctx, scrg_clip **out);
void        scrg_clip_free(scrg_clip *c);

/* PILEUP: what the alignments of a batch say at every position of a target — how many reads agree with it, which bases disagree,
 * how many delete it, how many insert something in front of it — summed over pairs on the device (pileup_kernels.hip), so that a
 * consumer who asks for coverage and variants need not bring every CIGAR to the host and walk it there.
 *
 * THE RULE (the kernel, scrg_pileup_from_runs of scrooge_amd_io.h and the tests' model implement this one).  A target is a
 * coordinate space of target_len positions (for the host calls: the genome).  The counts are uint32_t counts[7][target_len + 1],
 * plane-major, plane stride target_len + 1:
 *   plane 0     SCRG_PILE_MATCH               '=' columns at the position
 *   planes 1-4  SCRG_PILE_A, _C, _G, _T       'X' columns whose read base AS ALIGNED is that base (of a SCRG_READ_REVCOMP read the
 *                                             complement, as the align kernels take it)
 *   plane 5     SCRG_PILE_DEL                 'D' columns at the position
 *   plane 6     SCRG_PILE_INS                 insertion events in front of the position
 * A pair p is counted if its status is 0 (or there is no status array) and it has runs.  Its runs are walked with t (text
 * consumed) and q (read consumed) from 0 and g = target_start[p] + t:
 *   c=   MATCH[g .. g + c) += 1
 *   cX   for k < c: plane[1 + read_aligned[q + k]][g + k] += 1
 *   cD   DEL[g .. g + c) += 1
 *   cI   if the run before it is not 'I': INS[g] += 1 — directly adjacent I runs, such as the 2I2I a window seam leaves, are ONE
 *        insertion; its position is that of the next text column and may be target_len: that is what the extra slot is for.
 * A column at a position >= target_len is not counted, nor is an insertion at a position > target_len; a pair that had any such
 * column or insertion is counted once in an out-of-range counter.  Nothing is ever written outside the 7 * (target_len + 1) words.
 * The text is never read.  A pair that holds a run that is no run (a zero count, an operation other than = X I D) contributes
 * nothing outside [target_start, target_start + 255 * n_runs); what it contributes inside is not specified.  Sums wrap mod 2^32.
 * Slot target_len of planes 0-5 is 0.  Texts are forward only.
 *
 * The setting belongs to the handle, as the report does.  While it is on, scrg_align_mapping [_stranded|_resident] and
 * scrg_job_align add every OK pair of every chunk — in stage 1 of the chunk pipeline, after best-candidate selection, where the
 * report runs, at the candidate's start in the genome — to an accumulator the handle keeps on the device: 28 bytes per genome base,
 * allocated and zeroed on first use.  The accumulator sums over chunks, issue orders and SUCCESSIVE CALLS (the first handle state
 * that outlives a call).  scrg_ctx_take_pileup finishes it, copies it to the host, hands it over ONCE (release with
 * scrg_pileup_free) and leaves the accumulator empty; a take with nothing accumulated since the last one is SCRG_ERR_INVALID_ARG
 * with *out = NULL.  It works with outputs 0, 1, 2 and | SCRG_OUT_BEST (only the winners pile up), an edit limit, difference
 * strings, the report and every CIGAR form; the call's own result is byte for byte what it is with the setting off.  While it is
 * on, these are SCRG_ERR_INVALID_ARG: scrg_align_pairs (no target), SCRG_OUT_DISTANCE, lanes_per_pair != 1, a directed call that has
 * a leftward candidate, scrg_align_mapping_anchored, clipping (the kept stretch's positions are a later change) and a genome whose
 * length differs from the accumulator's (take the pileup first).  A call that fails with anything other than
 * SCRG_ERR_CIGAR_OVERFLOW discards the accumulator.  The _multi calls have no handle and are not served.  Off (the default):
 * nothing changes for anybody and no device memory is held.  New entry points only: SCRG_ABI_VERSION stays. */
#define SCRG_PILE_MATCH  0
#define SCRG_PILE_A      1
#define SCRG_PILE_C      2
#define SCRG_PILE_G      3
#define SCRG_PILE_T      4
#define SCRG_PILE_DEL    5
#define SCRG_PILE_INS    6
#define SCRG_PILE_PLANES 7
typedef struct scrg_pileup {
    uint64_t  target_len;         /* the genome's length */
    uint64_t  n_alignments;       /* pairs counted since the last take */
    uint64_t  n_out_of_range;     /* of them: pairs with a column or an insertion outside the target */
    uint32_t *counts;             /* [7][target_len + 1] */
} scrg_pileup;
scrg_status scrg_ctx_set_pileup(scrg_ctx *ctx, int enabled);           /* default 0; 0 also discards and releases the accumulator */
scrg_status scrg_ctx_get_pileup(const scrg_ctx *ctx, int *enabled);
scrg_status scrg_ctx_take_pileup(scrg_ctx *ctx, scrg_pileup **out);
void        scrg_pileup_free(scrg_pileup *p);

/* PILEUP SITES: of a pileup, the positions that matter — where reads disagree with the target, or where insertions pile up —
 * picked by a rule and compacted on the device (site_kernels.hip) into 40-byte records in position order, so that a consumer
 * brings down the sites and not 28 bytes per genome base.
 *
 * THE RULE (the kernels, scrg_pileup_sites_from_counts of scrooge_amd_io.h and the tests' model implement this one; the first two
 * compile one text, site_rule.h).  It is applied at every position g < target_len.  SLOT target_len IS NEVER A SITE: it holds only
 * the insertions behind the last base.  c[0..6] are the position's SCRG_PILE_* counts, r its reference code (0..3 = A C G T); all
 * arithmetic is 64-bit, because the counts are sums mod 2^32 and may each be near 2^32:
 *   depth  = c0 + c1 + c2 + c3 + c4 + c5
 *   n[b]   = c[1 + b] + (b == r ? c0 : 0) for b in 0..3, n[4] = c5        (allele codes: SCRG_SITE_DEL = 4 is "deleted")
 *   nonref = depth - n[r]
 *   alt    = the b != r in 0..4 with the largest n[b], ties to the smallest b; SCRG_SITE_NONE if nonref == 0
 *   call   = alt if n[alt] > n[r], else r                                  (a tie keeps the reference)
 *   passes(x) = x >= min_alt && x * 1000 >= min_alt_per_mille * depth
 *   the position is a site iff depth >= min_depth && (passes(nonref) || passes(c6))
 *   flags: SCRG_SITE_F_NONREF iff nonref > 0 && passes(nonref); SCRG_SITE_F_INS iff c6 > 0 && passes(c6); SCRG_SITE_F_CALL iff
 *   call != r.
 * With min_alt = 0 and min_alt_per_mille = 0 every position of at least min_depth is a site: the compacted coverage of a sparsely
 * covered genome.  Sites come out in ascending pos.  A rule with min_depth = 0, min_alt_per_mille > 1000 or reserved != 0 is
 * SCRG_ERR_INVALID_ARG.  Site offsets are 32-bit: target_len >= 2^32 - 1 is SCRG_ERR_INVALID_ARG for the site calls (only).
 *
 * scrg_ctx_take_pileup_sites is the other way to take a handle's accumulator (PILEUP, above): it finishes the accumulator in place,
 * marks, reads the number of sites (8 bytes), allocates, writes, and copies down 40 * n_sites bytes and the two counters; then the
 * accumulator is empty, exactly as after scrg_ctx_take_pileup — a take, handed over ONCE (release with scrg_pileup_sites_free), and
 * SCRG_ERR_INVALID_ARG with *out = NULL when nothing was accumulated since the last take.  The reference bases are those of the
 * handle's RESIDENT genome (what the mapping calls or scrg_genome_set left on the device): if none is resident, or its length is
 * not the accumulator's, the call is SCRG_ERR_INVALID_ARG and the accumulator is KEPT (scrg_ctx_take_pileup still serves it).
 * Replacing the genome by another of EQUAL length between the calls and the take is the caller's error: the counts are then judged
 * against bases they were not made from, and nothing can notice.  New entry points only: SCRG_ABI_VERSION stays. */
typedef struct scrg_site_rule {
    uint32_t min_depth;          /* >= 1 */
    uint32_t min_alt;            /* observations that must disagree; 0: none need to */
    uint32_t min_alt_per_mille;  /* 0..1000: ... and this share of the depth */
    uint32_t reserved;           /* 0 */
} scrg_site_rule;
typedef struct scrg_site {       /* 40 bytes */
    uint64_t pos;                /* 0-based target position */
    uint32_t counts[7];          /* the position's SCRG_PILE_* counts */
    uint8_t  ref, alt, call, flags;
} scrg_site;
#define SCRG_SITE_DEL   4        /* allele codes: 0..3 = A C G T, 4 = deleted */
#define SCRG_SITE_NONE  255
#define SCRG_SITE_F_NONREF 1
#define SCRG_SITE_F_INS    2
#define SCRG_SITE_F_CALL   4
typedef struct scrg_pileup_sites {
    uint64_t   target_len;       /* the genome's length */
    uint64_t   n_alignments;     /* pairs counted since the last take */
    uint64_t   n_out_of_range;   /* of them: pairs with a column or an insertion outside the target */
    uint64_t   n_sites;
    scrg_site_rule rule;
    scrg_site *sites;            /* [n_sites], ascending pos */
} scrg_pileup_sites;
scrg_status scrg_ctx_take_pileup_sites(scrg_ctx *ctx, const scrg_site_rule *rule, scrg_pileup_sites **out);
void        scrg_pileup_sites_free(scrg_pileup_sites *s);

/* A HIP stream (hipStream_t) of the given priority: -1 high, 0 normal, 1 low.  Streams of different
 * priorities never share a hardware queue, which is what lets launches of two handles overlap
 * (INTEGRATION.md §4b); streams of one priority may be multiplexed onto one queue. */
scrg_status scrg_stream_create(int device, int priority, void **stream);
scrg_status scrg_stream_destroy(void *stream);
const char *scrg_last_error(const scrg_ctx *ctx);
const char *scrg_status_string(scrg_status s);
/* mirrors genasm_gpu::enabled_algorithm_log (src/genasm_gpu.hpp:6) */
void        scrg_set_log(int enabled);
int         scrg_get_log(void);
int         scrg_device_count(void);
/* How this library was built: 0 for the shipped build; SCRG_BUILD_SELECT for the test build, whose scrg_params.reserved[0]
 * selects between formulations that give identical results (-DSCRG_SELECT); SCRG_BUILD_STATS if the kernels also carry their
 * profiling counters and scheduling switches (-DSCRG_STATS), SCRG_BUILD_ABLATE if also the ablation switches
 * (-DSCRG_ABLATE: results wrong by design).  See scrg_debug_stats. */
enum { SCRG_BUILD_STATS = 1, SCRG_BUILD_ABLATE = 2, SCRG_BUILD_SELECT = 4 };
int         scrg_build_flags(void);
/* The version of THIS interface.  It goes up whenever an entry point changes its arguments under the same name (version 5:
 * scrg_decode_edit_stream takes the capacity of its output array; version 6: scrg_encode_edit_stream and
 * scrg_runs_to_edit_stream take the parameters, and the edit stream itself carries the window ends) — such a change still links against code compiled with the
 * older header and would shift every later argument; version 8: scrg_result has grown by text_end, which scrg_job_write reads from a
 * result the caller may have built).  scrg_abi_version() is what the loaded library was built with; a binding
 * compares it with the SCRG_ABI_VERSION it was compiled against before anything else (include/scrooge_amd.hpp throws,
 * scrooge_amd/api.py raises). */
#define SCRG_ABI_VERSION 8
int         scrg_abi_version(void);

/* ---------------------------------------------------------------------------
 * Host-pointer entry points (the drop-in path).
 * ------------------------------------------------------------------------- */

/* Library-owned result of one batch; release with scrg_result_free(). */
typedef struct scrg_result {
    uint64_t  n_pairs;
    int64_t  *edit_distance;  /* [n_pairs]                                              */
    uint32_t *pair_status;    /* [n_pairs] SCRG_OK, SCRG_ERR_CIGAR_OVERFLOW, SCRG_PAIR_OVER_EDIT_LIMIT (the
                                 handle's edit limit: no runs, CIGAR "", edit distance > the limit), or
                                 SCRG_PAIR_NOT_BEST (best-candidate mode, below: no runs, CIGAR "") */
    uint64_t *run_offset;     /* [n_pairs+1] into runs                                   */
    scrg_run *runs;           /* all runs, pair after pair                               */
    uint64_t *cigar_offset;   /* [n_pairs+1] into cigar_text (each CIGAR NUL-terminated) */
    char     *cigar_text;     /* "%d%c" rendering, as genasm_cpu.cpp:387-403 — the runs printed one by one under
                                 SCRG_CIGAR_WINDOWED, the default; stretches of runs in the other forms (CIGAR FORMS) */
    int64_t   kernel_ns;      /* align kernel only (reference: core_algorithm_ns): the sum over
                                 the launches of the call's chunks, which overlap         */
    int64_t   pack_ns;        /* host threads: ASCII -> 2 bits per base into pinned memory */
    int64_t   total_ns;       /* whole call                                              */
    uint64_t *text_end;       /* [n_pairs] distance-only mode (SCRG_OUT_DISTANCE): the text characters the pair's alignment
                                 consumed — the sum of the '=', 'X' and 'D' counts of the CIGAR that was not written; 0 for a
                                 pair over the edit limit and for SCRG_PAIR_NOT_BEST.  NULL in every other mode */
} scrg_result;

/* (The large arrays are recycled by the library: up to 2 GB of them are kept for the next call of similar size
 * instead of being returned to the allocator, so that a stream of batches does not fault fresh pages every time.
 * scrg_result_pool_trim() returns the parked arrays to the allocator; destroying the last handle does the same.
 * Recycled arrays are NOT zeroed: every element a result publishes is written by the call that publishes it.) */
void scrg_result_free(scrg_result *r);
void scrg_result_pool_trim(void);

/* Best-candidate mode (scrg_params.outputs | SCRG_OUT_BEST; the mapping calls — scrg_align_mapping, _stranded, _resident,
 * _multi, scrg_job_align — which know which pairs belong to one read; SCRG_ERR_INVALID_ARG on the pairwise calls and on
 * scrg_host_plan).  For one read with candidates c0 < c1 < ... in the caller's order:
 *   - eligible: every pair that is not over the handle's edit limit.  A pair whose runs overflowed its slice is eligible
 *     (its edit distance is valid);
 *   - the winner: the eligible pair with the smallest edit distance, ties to the lowest candidate index.  A read without
 *     candidates, or without an eligible one, has no winner;
 *   - the winner is returned exactly as without the mode: edit distance, status (SCRG_OK, or SCRG_ERR_CIGAR_OVERFLOW, with
 *     which the call returns SCRG_ERR_CIGAR_OVERFLOW as ever), runs and CIGAR text, bit for bit;
 *   - every other eligible pair: its full edit distance, status SCRG_PAIR_NOT_BEST, no runs
 *     (run_offset[p] == run_offset[p+1]) and CIGAR "".  (A loser's slice that overflowed is of no interest any more: its
 *     status is SCRG_PAIR_NOT_BEST too and does not make the call fail);
 *   - pairs over the edit limit: as without the mode (SCRG_PAIR_OVER_EDIT_LIMIT, the running sum, no runs, "").
 * So at most one pair per read carries runs and text, and every pair's edit distance still arrives (12 bytes per pair cross
 * PCIe): enough for a second-best distance or a tie count.  The result does not depend on how the call is cut into chunks,
 * on sort_by_length, on the number of devices or on timing: chunks are cut at read boundaries in this mode
 * (scrg_host_plan_mapping).  Reads of 2^28 bases or more are rejected in this mode. */

/* Distance-only mode (scrg_params.outputs = SCRG_OUT_DISTANCE, every host entry point; lanes_per_pair = 1, the default —
 * SCRG_ERR_INVALID_ARG for the GenASM-row mappings): "how many edits, and where in the text does the alignment end" (Edlib's
 * default task, KSW2's score-only flag, WFA's score scope).  edit_distance and pair_status are what they are without the
 * flag (no pair can overflow: SCRG_OK, or SCRG_PAIR_OVER_EDIT_LIMIT with the running sum), text_end is filled, run_offset and
 * cigar_offset hold n_pairs + 1 zeros and there are no runs and no text.  The call is cut into the same chunks as without the
 * flag (scrg_host_plan[_mapping] accept it and return the same cuts); 16 bytes per pair cross PCIe on the way back.
 * With SCRG_OUT_BEST (20; mapping calls): the rule above unchanged — the winner has SCRG_OK and its text_end, every other
 * eligible pair SCRG_PAIR_NOT_BEST, its distance and text_end 0. */

/* MATE PAIRS (scrg_align_mapping_paired, scrg_select_mates; scrg_mates_from_distances of scrooge_amd_io.h is the same rule on the
 * host).  Reads 2m and 2m+1 are mate pair m, side A and side B.  A candidate has a start s on the forward genome (cand_start), a
 * strand r (cand_reverse: 0 forward, 1 reverse complement), its read's length L and an edit distance ed (counted in 32 bits, as
 * best-candidate mode counts it); it is eligible when it is not over the edit limit (an overflowed slice stays eligible).  For an
 * eligible A candidate i and an eligible B candidate j:
 *   span(i,j) = max(s_i + L_A, s_j + L_B) - min(s_i, s_j): from starts and read lengths only — not from the text an alignment
 *               consumed, which does not exist in distance-only mode and is not known before the CIGAR is; an insert-size window is
 *               wide against the few bases an alignment's end may differ from start + L;
 *   orientation: FR: r_i != r_j and the forward one's start <= the reverse one's; RF: r_i != r_j and the reverse one's start <= the
 *               forward one's (equal starts satisfy both); FF: r_i == r_j; ANY: always;
 *   (i,j) is proper when the orientation holds and min_span <= span <= max_span; cost(i,j) = ed_i + ed_j (saturated at 2^32 - 2);
 *   (i*,j*) is the proper combination of least cost, ties to the lowest i, then the lowest j; a* and b* are each side's winner by
 *   best-candidate mode's rule (smallest ed, ties to the lowest index).
 * The mate pair is proper exactly when a proper combination exists and cost(i*,j*) <= ed(a*) + ed(b*) + unpaired_penalty; its
 * winners are then i* and j*, otherwise a* and b* (either absent when its side has no eligible candidate).  Winners, losers and
 * pairs over the limit are returned exactly as best-candidate mode returns them (above). */
enum { SCRG_MATES_FR = 0, SCRG_MATES_RF = 1, SCRG_MATES_FF = 2, SCRG_MATES_ANY = 3 };
enum { SCRG_MATES_PROPER = 1, SCRG_MATES_HAS_A = 2, SCRG_MATES_HAS_B = 4, SCRG_MATES_TIED = 8 };
typedef struct scrg_mate_rule {
    uint64_t min_span, max_span;   /* inclusive bounds on the span; min_span <= max_span */
    uint32_t orientation;          /* SCRG_MATES_FR (default), _RF, _FF, _ANY */
    uint32_t unpaired_penalty;     /* edits a proper combination may cost more than the two single bests */
    uint32_t reserved[2];          /* must be 0 */
} scrg_mate_rule;
typedef struct scrg_mate_record {  /* 32 bytes, one per mate pair */
    uint64_t winner[2];     /* pair index of side A's / B's winner; UINT64_MAX: none */
    uint32_t cost;          /* sum of the winners' edit distances (one of them if the other is absent; 0 if both are) */
    uint32_t second_cost;   /* proper: least cost among the OTHER proper combinations; UINT32_MAX: none, or not proper */
    uint32_t span;          /* span of the winners when both exist, saturated to UINT32_MAX; else 0 */
    uint16_t n_proper;      /* proper combinations, saturated to 65535 */
    uint8_t  flags;         /* SCRG_MATES_PROPER | _HAS_A | _HAS_B | _TIED.  TIED on a proper pair: second_cost == cost; on an
                               unpaired result: a side's winner shares its distance with another eligible candidate of that side */
    uint8_t  reserved;
} scrg_mate_record;

typedef struct scrg_mates {        /* library-owned: scrg_mates_free */
    uint64_t n_mates;
    scrg_mate_record *records;     /* [n_mates]; winner[] are the caller's pair indices (as the result's arrays) */
} scrg_mates;
void scrg_mates_free(scrg_mates *mates);

/* Paired-end read mapping against the resident genome (scrg_genome_set): scrg_align_mapping_resident in best-candidate mode —
 * the call implies SCRG_OUT_BEST; params.outputs 0, 1, 2 or SCRG_OUT_DISTANCE, with or without the flag — except that the winners
 * of reads 2m and 2m+1 are chosen together by the rule above, on the GPU, between the align kernel and the compaction.
 * n_reads must be even; rule == NULL is FR, span 0 .. UINT64_MAX, penalty 0; SCRG_ERR_INVALID_ARG for an odd n_reads,
 * min_span > max_span, orientation > 3, a non-zero reserved word, or a mate pair with n_a x n_b >= 2^32 — and *mates and *out stay
 * NULL.  Everything best-candidate mode works with works here through the same statuses: the edit limit, distance-only mode, CIGAR
 * forms, the report, clipping and the pileup (only the winners pile up).  *mates holds one record per mate pair, winner[] as the
 * caller's pair indices; a mate pair without candidates has no winners, cost 0 and flags 0.  The result does not depend on
 * chunking, sort_by_length or timing: the issue order sorts MATE PAIRS (stable, by the longer mate's length), and a chunk cut that
 * would fall inside a mate pair moves forward to the next mate pair's first pair (scrg_host_plan_mates).  A status of
 * SCRG_ERR_CIGAR_OVERFLOW delivers both, as ever. */
scrg_status scrg_align_mapping_paired(scrg_ctx *ctx, const scrg_params *params,
                                      uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                      const uint64_t *cand_offsets, const uint64_t *cand_start,
                                      const uint8_t *cand_reverse, const scrg_mate_rule *rule,
                                      scrg_mates **mates, scrg_result **out);

/* READ SUMMARY AND MAPPING QUALITY (scrg_ctx_set_read_summary, scrg_read_summary; scrg_read_summary_from_distances of
 * scrooge_amd_io.h is the same rule on the host).  Best-candidate mode picks a read's winner; this says how much the winner deserves
 * to be believed.  Eligibility and the winner are exactly best-candidate mode's (above): eligible = not over the edit limit (an
 * overflowed slice stays eligible), the winner = the smallest 32-bit edit distance, ties to the lowest index.  Of one read:
 *   best_ed      the winner's distance;
 *   n_tied       eligible candidates at best_ed, the winner included;
 *   second_ed    the smallest eligible distance strictly above best_ed; UINT32_MAX: none;
 *   n_eligible   eligible candidates;          n_candidates   all candidates of the read.
 * MAPQ, with L the read's length, all arithmetic in 64 bits and every division floored:
 *   no winner: 0;   n_tied > 1: 0;   otherwise
 *   cap = max_q - min(max_q, max_q * 1000 * best_ed / (zero_per_mille * L))           (L == 0: cap = max_q)
 *   no second: q = cap;   otherwise q = min(cap, min(max_q, per_edit * (second_ed - best_ed))).
 * At the defaults (10, 60, 250): L 150, best 0, no second: 60; best 0, second 1: 10; best 3, second 5: 20 (cap 56); best 38: 0;
 * L 10000, best 1000, no second: 36.  The constants are a HEURISTIC, as every mapper's MAPQ is — defaults of a rule the caller
 * sets, validated against no truth set, and no claim about error probabilities.  A read is KEPT when it has a winner and
 * mapq >= min_keep_q: with the handle's pileup on and min_keep_q > 0, only the winners of kept reads pile up. */
enum { SCRG_MAPQ_HAS_WINNER = 1, SCRG_MAPQ_TIED = 2, SCRG_MAPQ_HAS_SECOND = 4, SCRG_MAPQ_KEPT = 8 };
typedef struct scrg_mapq_rule {    /* 16 bytes; anything outside the ranges is SCRG_ERR_INVALID_ARG */
    uint32_t per_edit;             /* 0 .. 255, default 10: MAPQ per edit between the best and the second distance */
    uint32_t max_q;                /* 0 .. 254, default 60 (255 is SAM's "not available") */
    uint16_t zero_per_mille;       /* 1 .. 1000, default 250: the edit rate, in edits per 1000 read bases, at which the cap reaches 0 */
    uint16_t min_keep_q;           /* 0 .. 254, default 0: the MAPQ from which a read is KEPT */
    uint32_t reserved;             /* must be 0 */
} scrg_mapq_rule;
/* (The record is `struct scrg_read_summary`; scrg_read_summary without the keyword is the device entry point below, so the
 * typedef has a name of its own.) */
typedef struct scrg_read_summary { /* 32 bytes, one per read */
    uint64_t winner;               /* pair index of the winner; UINT64_MAX: none */
    uint32_t best_ed, second_ed;   /* UINT32_MAX both without a winner; second_ed UINT32_MAX: no second */
    uint32_t n_tied, n_eligible, n_candidates;
    uint8_t  mapq;
    uint8_t  flags;                /* SCRG_MAPQ_HAS_WINNER | _TIED (n_tied > 1) | _HAS_SECOND | _KEPT */
    uint16_t reserved;
} scrg_read_record;
typedef struct scrg_read_summaries {   /* library-owned: scrg_read_summaries_free */
    uint64_t n_reads;
    scrg_read_record *reads;       /* [n_reads], the caller's read order; winner as the caller's pair index (as the result's arrays) */
    scrg_mapq_rule rule;           /* the rule they were made by */
} scrg_read_summaries;
void scrg_read_summaries_free(scrg_read_summaries *s);

/* The handle's setting: every mapping call in best-candidate mode (SCRG_OUT_BEST; scrg_align_mapping, _stranded, _resident,
 * _directed, scrg_job_align) also makes one record per read, on the GPU right behind the selection, and keeps them until
 * scrg_ctx_take_read_summary or the next align call.  rule == NULL: the defaults.  The call's result is byte for byte what it is
 * with the setting off; 8 bytes per read go up and 32 come back.  It composes with the edit limit, both strands,
 * SCRG_OUT_DISTANCE | SCRG_OUT_BEST, every CIGAR form, difference strings, the report and clipping.  SCRG_ERR_INVALID_ARG, and nothing
 * to take: a call without SCRG_OUT_BEST (chunks are cut at read boundaries only in that mode, so every read is whole inside one
 * chunk), the pairwise calls, scrg_align_mapping_paired (a mate pair's winners are chosen together: scrg_mate_record has cost and
 * second_cost), scrg_align_mapping_anchored, and min_keep_q > 0 without the handle's pileup on.  With the pileup on and
 * min_keep_q > 0 only the winners of KEPT reads are summed (n_alignments counts them); everything else of the call still sees every
 * winner.  The _multi calls have no handle and no setting.  New entry points only: SCRG_ABI_VERSION stays. */
scrg_status scrg_ctx_set_read_summary(scrg_ctx *ctx, const scrg_mapq_rule *rule_or_NULL_for_defaults, int enabled);
scrg_status scrg_ctx_get_read_summary(const scrg_ctx *ctx, scrg_mapq_rule *rule, int *enabled);   /* either may be NULL */
scrg_status scrg_ctx_take_read_summary(scrg_ctx *ctx, scrg_read_summaries **out);

/* Unstructured pairwise alignment: queries[i] is consumed completely against a
 * prefix of texts[i] (reference: genasm_gpu.cu:982-1065; returns all n results,
 * unlike the CPU overload's double increment at genasm_cpu.cpp:600-605). */
scrg_status scrg_align_pairs(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                             const char *const *texts, const uint64_t *text_lens,
                             const char *const *queries, const uint64_t *query_lens,
                             scrg_result **out);

/* Read-mapping alignment: read r is aligned against the genome suffix starting
 * at cand_start[c] for every c in [cand_offsets[r], cand_offsets[r+1])
 * (reference: genasm_gpu.cu:890-980 / genasm_cpu.cpp:495-555, :512-514 for the
 * suffix semantics).  Genome and reads are packed and stored once.  Results are
 * in read-major, candidate-minor order. */
scrg_status scrg_align_mapping(scrg_ctx *ctx, const scrg_params *params,
                               const char *genome, uint64_t genome_len,
                               uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                               const uint64_t *cand_offsets, const uint64_t *cand_start,
                               scrg_result **out);

/* Many read batches against one reference: scrg_genome_set() packs the genome ONCE (host threads), transfers it and
 * keeps it in the handle's HBM; scrg_align_mapping_resident() then aligns batches against it without touching
 * the genome again (scrg_align_mapping stages its genome on every call, as the reference re-converts it,
 * genasm_cpu.cpp:508 — and leaves it resident afterwards).  cand_reverse may be NULL (all forward) or hold one 0/1 per
 * candidate (1 = align the reverse complement of the read, as scrg_align_mapping_stranded in scrooge_amd_io.h).  The
 * genome stays resident until another one is set or scrg_genome_clear() is called; pairwise calls on the same handle do
 * not disturb it. */
scrg_status scrg_genome_set(scrg_ctx *ctx, const char *genome, uint64_t genome_len);
void        scrg_genome_clear(scrg_ctx *ctx);
scrg_status scrg_align_mapping_resident(scrg_ctx *ctx, const scrg_params *params,
                                        uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                        const uint64_t *cand_offsets, const uint64_t *cand_start,
                                        const uint8_t *cand_reverse, scrg_result **out);

/* SEEDING: every read's candidate locations, found on the GPU from a k-mer index of the resident genome (scrg_genome_index,
 * scrg_find_candidates; scrg_candidates_from_genome of scrooge_amd_io.h is the same rule on the host).  The rule, stated once
 * (csrc/seed_rule.h is its text for kernels and host alike):
 *   key      of k bases: sum of code[i] * 4^(k-1-i), A0 C1 G2 T3.
 *   index    one entry (key, p) for every p with p % stride == 0 and p + k <= genome_len, over the resident genome as ONE string
 *            (the job's concatenated coordinate; a k-mer across a chromosome seam is indexed like any other), sorted by key.
 *   hits     of a read on a strand — R' is the read (strand 0) or its reverse complement (strand 1), L its length: for every r in
 *            [0, L - k] and every index entry (key(R', r), p) whose key has at most max_occ entries, a hit (d = p - r, r); d is
 *            signed.  L < k: no hits.
 *   clusters per read and strand: the hits sorted by d; a new cluster begins where d[i] - d[i-1] > band.  votes = its number of
 *            hits; start = max(0, d*) of its hit (r*, d*) with the least r, ties to the least d (the earliest base of the read that
 *            hit says best where base 0 belongs: indel drift grows along the read).
 *   candidates of a read: the clusters of both strands with votes >= min_hits, ordered by votes descending, then start ascending,
 *            then strand ascending; the first max_candidates of them, in that order — the best-voted candidate has the lowest
 *            index, which is what best-candidate mode's tie rule prefers.  A reverse candidate means what cand_reverse means: align
 *            the read's reverse complement at start.
 *   sampling (scrg_ctx_set_seed_sampling; off by default) takes the same subset of k-mers on genome and reads: the closed syncmers
 *            of s-mers, smer = s in 3 .. k - 1; s = 0 is the rule above, bit for bit.  The s-mer j of a key, j in [0, k - s], is
 *            v_j = (key >> 2 (k - s - j)) & (4^s - 1); its order word is h(v) = m ^ (m >> 15) with m = v * 0x9E3779B1 mod 2^32, a
 *            bijection on 32-bit words, so only equal s-mers tie.  The key is SELECTED iff min_j h(v_j) is attained at j = 0 or at
 *            j = k - s; a tie at either end counts (an all-A k-mer is selected).  Then
 *              index   one entry per p with p % stride == 0, p + k <= genome_len AND key(genome, p) selected;
 *              hits    only the (strand, r) whose key(R', r) is selected are looked up: an unselected key contributes nothing and
 *                      is not counted in n_keys_over_max_occ; a selected one counts as a lookup even when it is over max_occ;
 *              clusters, votes, anchors, ranks and candidates are unchanged.
 *            Selection depends on the key alone — not on neighbours, a window or the strand (strand 1 tests the key of R'; the
 *            index holds forward genome k-mers only) — so every conserved k-mer that is an index entry is also looked up.
 *            s = k - 1 selects every key (two s-mers: the minimum is at an end).  At stride 1 any k - s consecutive positions
 *            hold a selected one (the least s-mer they cover is the first s-mer of one of them or the last of one), and on
 *            random sequence about 2 / (k - s + 1) of the keys are selected.
 * Every quantity is a count or a minimum over a set: the result depends on no sort's stability, on no chunking, on no schedule.
 * It is a HEURISTIC of this library's own (the project it is modelled on reads another mapper's output and has no seeding): exact
 * k-mers at a fixed stride, optionally sampled as closed syncmers, no chaining, and a recall that was measured on random genomes
 * with independent errors only. */
typedef struct scrg_seed_rule {     /* 32 bytes; anything outside the ranges is SCRG_ERR_INVALID_ARG */
    uint32_t k;                     /* 8 .. 16, default 13: bases per k-mer (the key has 2k bits, 32 at k = 16) */
    uint32_t stride;                /* 1 .. 64, default 4: the genome positions p with p % stride == 0 are indexed */
    uint32_t max_occ;               /* 1 .. 65535, default 64: a key with more index entries contributes nothing */
    uint32_t band;                  /* 0 .. 65535, default 32: largest gap between neighbouring diagonals of one cluster */
    uint32_t min_hits;              /* >= 1, default 2 */
    uint32_t max_candidates;        /* 1 .. 64, default 4: per read, both strands together */
    uint32_t strands;               /* 1: forward only; 3 (default): both */
    uint32_t hit_budget_mb;         /* 0: the default (256); device memory for the hits of one chunk of reads (see scrg_find_candidates) */
} scrg_seed_rule;
void        scrg_seed_rule_default(scrg_seed_rule *rule);
/* The one statement of the ranges and of the two limits on the genome: genome_len < 2^32 (positions are 32-bit) and at most
 * 2^31 - 1 index entries, (genome_len - k) / stride + 1 (they are counted in 31 bits: a genome of 2^31 + k - 1 bases and more
 * needs a stride of 2 or more).  Pure host code. */
scrg_status scrg_seed_rule_check(const scrg_seed_rule *rule, uint64_t genome_len);

/* The index of the handle's resident genome (scrg_genome_set first), built on the GPU and kept on the handle; it replaces an
 * earlier one.  rule == NULL: the defaults.  It holds positions, never pointers, and goes with the genome it was made of:
 * scrg_genome_set, scrg_genome_clear and every mapping call that stages a genome of its own drop it. */
scrg_status scrg_genome_index(scrg_ctx *ctx, const scrg_seed_rule *rule_or_NULL_for_defaults);
void        scrg_genome_index_clear(scrg_ctx *ctx);   /* (also gives back the device buffers scrg_find_candidates keeps between calls) */
/* SCRG_ERR_INVALID_ARG without an index; every out pointer may be NULL.  device_bytes: entries and bucket table. */
scrg_status scrg_genome_index_info(scrg_ctx *ctx, scrg_seed_rule *rule, uint64_t *n_entries, uint64_t *device_bytes);
/* Sampling (SEEDING above).  smer: 0 (off, the default) or 3 .. 15, anything else SCRG_ERR_INVALID_ARG.  The setting is read by
 * scrg_genome_index (and so by scrg_job_seed): smer >= rule.k is SCRG_ERR_INVALID_ARG there and leaves no index.  The index
 * records the smer it was built with and scrg_find_candidates uses the index's: changing the setting afterwards changes nothing
 * until the next build.  With sampling the build counts the selected positions first (one count per workgroup, no array per
 * position) and brings their total home in one synchronisation; an index of zero entries over a non-empty genome is possible and
 * behaves like that of a genome shorter than k: no read has a candidate. */
scrg_status scrg_ctx_set_seed_sampling(scrg_ctx *ctx, uint32_t smer);
/* smer: that of the current index; n_positions: the positions it considered, (genome_len - k) / stride + 1 (n_entries of
 * scrg_genome_index_info is how many of them it holds); last_n_lookups: the selected (read, strand, r) of the handle's last
 * successful scrg_find_candidates (0 before one).  SCRG_ERR_INVALID_ARG without an index; every out pointer may be NULL. */
scrg_status scrg_seed_sampling_info(scrg_ctx *ctx, uint32_t *smer, uint64_t *n_positions, uint64_t *last_n_lookups);
/* The predicate on the host, pure: 1 if the key of k bases (its low 2k bits) is selected at smer, 0 if not or if k is outside
 * 8 .. 16 or smer is neither 0 nor in 3 .. k - 1. */
int         scrg_seed_key_selected(uint32_t key, uint32_t k, uint32_t smer);

typedef struct scrg_candidates {    /* library-owned: scrg_candidates_free */
    uint64_t n_reads;
    uint64_t *cand_offsets;         /* [n_reads + 1]; read r's candidates are [cand_offsets[r], cand_offsets[r + 1]) */
    uint64_t *cand_start;
    uint8_t  *cand_reverse;
    uint32_t *cand_votes;
    uint64_t n_hits;                /* hits of all reads */
    uint64_t n_clusters;            /* clusters of all reads, whatever their votes */
    uint64_t n_keys_over_max_occ;   /* (read, strand, r) whose key has more than max_occ entries */
    scrg_seed_rule rule;            /* the rule they were made by */
} scrg_candidates;
void scrg_candidates_free(scrg_candidates *c);
/* The candidates of n_reads reads against the handle's index.  cand_offsets, cand_start and cand_reverse go into
 * scrg_align_mapping_resident, _paired and _directed as they are.  The reads go up once, packed; their hits are made, sorted and
 * clustered on the GPU in chunks of whole reads whose hits fit hit_budget_mb (a read with more hits than that gets a chunk of
 * its own) — the result is the same for every budget.  The budget counts the hits alone, at 48 bytes each; a chunk also holds 16
 * bytes per (strand, r) of its reads, of which it may have four per budgeted hit (1.33 times the budget), and the sort's
 * temporary space (about 12 bytes a hit): up to about 2.6 times the budget in all, beside the call's packed reads (a quarter byte
 * per base) and 20 bytes per read, kept on the handle between calls until scrg_genome_index_clear or the index is dropped.
 * SCRG_ERR_INVALID_ARG without an index or for a read of 2^30 bases or more,
 * SCRG_ERR_BAD_BASE for a base outside ACGTacgt; n_reads == 0: SCRG_OK and an empty result. */
scrg_status scrg_find_candidates(scrg_ctx *ctx, uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                 scrg_candidates **out);

/* Candidates with a DIRECTION, against the resident genome (scrg_genome_set).  cand_leftward may be NULL (or all zero): the call
 * is then exactly scrg_align_mapping_resident.  A leftward candidate c (cand_leftward[c] != 0): let R' be the read as the
 * candidate names it — its reverse complement if cand_reverse[c], the read itself otherwise.  The result is what the reference
 * produces for text = reverse complement of genome[0, cand_start[c]) and read = reverse complement of R': R' is aligned so that
 * it ENDS at cand_start[c] and grows to the left.  So
 *   - cand_start[c] is the exclusive right end, 0 <= cand_start <= genome_len; 0 is an empty text (all insertions);
 *   - runs and CIGAR text come in the order the kernel produced them: from the anchor outwards, i.e. right to left on the genome;
 *   - text_end (distance-only mode) = the genome bases consumed to the left of cand_start.
 * The genome is read backwards from its one packed copy (text strands, above: the call switches the setting on for its launches);
 * no reverse-complemented genome exists anywhere.  Edit limit, SCRG_OUT_BEST, SCRG_OUT_DISTANCE, sort_by_length and chunking
 * work as in the resident call.  With any leftward candidate, lanes_per_pair != 1 is SCRG_ERR_INVALID_ARG. */
scrg_status scrg_align_mapping_directed(scrg_ctx *ctx, const scrg_params *params,
                                        uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                        const uint64_t *cand_offsets, const uint64_t *cand_start,
                                        const uint8_t *cand_reverse, const uint8_t *cand_leftward, scrg_result **out);

/* ANCHORED alignment: both sides of a seed, joined.  Candidate p of read r has an anchor: position anchor_read[p] (ra, 0 ..
 * read_len, counted in R' — the read as the candidate's strand names it) matches genome position anchor_genome[p] (ga, 0 ..
 * genome_len).  R'[0, ra) is aligned leftwards so that it ends at ga, R'[ra, L) rightwards from ga, both halves as sub-pairs of
 * ONE scrg_align_mapping_directed call (the halves are pointers into the caller's reads: nothing is copied on the host; each
 * half is packed as a read of its own).  Per pair the result holds
 *   - edit_distance = left + right;
 *   - runs = the left half's runs in REVERSED order, then the right half's: left to right on the genome.  Nothing is merged at
 *     the seam (runs are never merged across windows; the seam is one more window end) — and the left half's windows end where
 *     they ended growing leftwards;
 *   - cigar_text rendered from the joined runs ("%d%c", or in the handle's form: CIGAR FORMS);
 *   - pair_status SCRG_ERR_CIGAR_OVERFLOW if either half overflowed (the call then returns it, as ever), else SCRG_OK;
 *   - text_start[p] (may be NULL) = ga - the genome bases the left half consumed: the alignment covers
 *     genome[text_start, text_start + consumed);
 *   - text_end (distance-only mode) = the genome bases both halves consumed.
 * params.outputs: 0, 1, 2 and SCRG_OUT_DISTANCE.  SCRG_OUT_BEST, or a handle with an edit limit set, is SCRG_ERR_INVALID_ARG (a
 * limit per half is not a limit per read), as are lanes_per_pair != 1 and an anchor out of range.  cand_reverse may be NULL. */
scrg_status scrg_align_mapping_anchored(scrg_ctx *ctx, const scrg_params *params,
                                        uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                        const uint64_t *cand_offsets, const uint64_t *anchor_genome, const uint64_t *anchor_read,
                                        const uint8_t *cand_reverse, uint64_t *text_start, scrg_result **out);
/* The join of one pair on the host (no GPU, no handle): runs = left[n_left-1 .. 0], then right[0 .. n_right-1]; *left_text (may
 * be NULL) = the text characters the left half consumed (its '=', 'X' and 'D' counts).  *n_runs = n_left + n_right either way;
 * SCRG_ERR_CIGAR_OVERFLOW if runs_cap is smaller (runs may be NULL with runs_cap 0 to ask), SCRG_ERR_INVALID_ARG for an
 * operation other than = X I D. */
scrg_status scrg_join_anchored_runs(const scrg_run *left, uint64_t n_left, const scrg_run *right, uint64_t n_right,
                                    scrg_run *runs, uint64_t runs_cap, uint64_t *n_runs, uint64_t *left_text);

/* Several GPUs, one call, one process (the reference is single-GPU: GPU_ID 0, src/genasm_gpu.cu:67).  The batch is cut
 * into chunks in issue order (longest read first) and chunk k goes to devices[k mod n_devices]; every device has its own
 * host thread, streams and buffers, brings its chunks' results back itself (no inter-GPU traffic) and the result is
 * assembled in caller order exactly as by the single-device calls.  A device may be listed more than once (more chunks
 * in flight on it).  No handle: per-device state is created on first use and kept for later calls —
 * scrg_multi_release() frees it.  The mapping call stages the genome on every listed device.  Errors: status code and
 * scrg_multi_last_error() (per thread).  There is no handle, so no edit limit: these calls align every pair in full. */
scrg_status scrg_align_pairs_multi(const int32_t *devices, int32_t n_devices, const scrg_params *params, uint64_t n_pairs,
                                   const char *const *texts, const uint64_t *text_lens,
                                   const char *const *queries, const uint64_t *query_lens,
                                   scrg_result **out);
scrg_status scrg_align_mapping_multi(const int32_t *devices, int32_t n_devices, const scrg_params *params,
                                     const char *genome, uint64_t genome_len,
                                     uint64_t n_reads, const char *const *reads, const uint64_t *read_lens,
                                     const uint64_t *cand_offsets, const uint64_t *cand_start,
                                     const uint8_t *cand_reverse, scrg_result **out);
/* How a host call with these sequence lengths is cut up (no GPU involved): issue_order[k] = caller index of the k-th
 * pair issued (longest read first, stable — src/tests.cu:375-377; NULL to skip), chunk_first[0 .. *n_chunks] = issue index of
 * every chunk's first pair (chunk_cap entries available; NULL to skip).  Chunk k is processed by devices[k mod n_devices];
 * chunks are whole groups of 64 pairs except the last.  text_lens may be NULL. */
scrg_status scrg_host_plan(const scrg_params *params, int32_t n_devices, uint64_t n_pairs, const uint64_t *text_lens,
                           const uint64_t *read_lens, uint32_t *issue_order, uint64_t *chunk_first, uint64_t chunk_cap,
                           uint64_t *n_chunks);
/* The same for a mapping batch: pair p belongs to the read r with cand_offsets[r] <= p < cand_offsets[r+1] and has that
 * read's length.  Without SCRG_OUT_BEST the cuts are those of the call (scrg_host_plan's for the same per-pair read lengths,
 * as long as no chunk of mixed lengths reaches the 32 MB of packed sequence a chunk may hold); with it, every cut that
 * would fall inside a read's candidates is moved forward to the first pair of the next read, so that a chunk holds whole
 * reads (its last group of 64 pairs is then a partial one, as the call's last may be) — exactly the cuts such a call makes. */
scrg_status scrg_host_plan_mapping(const scrg_params *params, int32_t n_devices, uint64_t n_reads, const uint64_t *read_lens,
                                   const uint64_t *cand_offsets, uint32_t *issue_order, uint64_t *chunk_first,
                                   uint64_t chunk_cap, uint64_t *n_chunks);
/* The same for scrg_align_mapping_paired (n_reads even, else SCRG_ERR_INVALID_ARG): the issue order sorts mate pairs — stable, by
 * the longer mate's length, so that a mate pair's pairs stay adjacent and in the caller's order — and every cut that would fall
 * inside a mate pair is moved forward to the next mate pair's first pair: exactly the cuts such a call makes. */
scrg_status scrg_host_plan_mates(const scrg_params *params, int32_t n_devices, uint64_t n_reads, const uint64_t *read_lens,
                                 const uint64_t *cand_offsets, uint32_t *issue_order, uint64_t *chunk_first,
                                 uint64_t chunk_cap, uint64_t *n_chunks);
void        scrg_multi_release(void);
const char *scrg_multi_last_error(void);

/* ---------------------------------------------------------------------------
 * Device-pointer entry points (inputs/outputs already resident in HBM; this is
 * what bench.py times).  All pointers below are device pointers valid on the
 * handle's device; work is enqueued on the handle's stream and NOT synchronised.
 * ------------------------------------------------------------------------- */

/* Sequence storage used by the align kernel: "planar 2-bit" — one uint64_t per
 * 32 bases; bit k of the low word is bit 0 of base k's code, bit k of the high
 * word is bit 1 (A=0 C=1 G=2 T=3, genasm_cpu.cpp:87-90).  Sequence arrays need
 * SCRG_SEQ_PAD_WORDS readable words past the last base. */
#define SCRG_SEQ_PAD_WORDS 4

/* ASCII -> planar.  d_ascii holds n_words*32 bytes; bytes equal to 0 are
 * padding and encode as A.  *d_bad_count is incremented for every other
 * non-ACGTacgt byte. */
scrg_status scrg_pack_planar(scrg_ctx *ctx, const char *d_ascii, uint64_t n_words,
                             uint64_t *d_planar, uint32_t *d_bad_count);

/* ASCII -> planar in the LANE-INTERLEAVED layout the one-pair-per-lane kernel reads best.  d_ascii holds
 * n_rows rows of words_per_row*32 bytes each (zero padded, every sequence starting at a multiple of 32
 * bytes within its row).  Rows are taken in groups of 64 (the pairs one wavefront aligns side by side):
 * word w of row r is stored at d_planar[((r / 64) * words_per_row + w) * 64 + r % 64], so the 64 lanes of a
 * wavefront, which walk their sequences at the same pace, read 512 contiguous bytes per load instead of 64
 * separate cache lines.  A sequence that starts at byte 32*k of row r has
 *     offset_in_bases = 32 * (((r / 64) * words_per_row + k) * 64 + r % 64)
 * and a word stride of 64 (scrg_params.text_stride_words / read_stride_words).  d_planar needs
 * ceil(n_rows / 64) * 64 * words_per_row words plus SCRG_SEQ_PAD_WORDS_STRIDED(64) readable words of padding. */
scrg_status scrg_pack_planar_groups(scrg_ctx *ctx, const char *d_ascii, uint64_t n_rows, uint64_t words_per_row,
                                    uint64_t *d_planar, uint32_t *d_bad_count);
/* The same packing of ONE sequence on the host, with the packer the host entry points use on their threads (AVX2 or scalar
 * code, chosen at run time; no GPU, no handle): word w of the sequence goes to planar[w * stride_words] (stride 0 = 1), the
 * words past the sequence up to n_words are zeroed.  SCRG_ERR_BAD_BASE if a byte is not one of ACGTacgt (the reference asserts,
 * src/genasm_cpu.cpp:487-489).  A caller that stages its own device arrays can use it; the CPU tests hold it to the layout above. */
scrg_status scrg_pack_planar_host(const char *ascii, uint64_t n_bases, uint64_t *planar, uint64_t stride_words, uint64_t n_words);
#define SCRG_SEQ_PAD_WORDS_STRIDED(stride) (2 * (stride) + 2)

/* One alignment problem.  Offsets are in bases from the start of d_seq: base k of a sequence with offset
 * `off` and word stride s lives in word (off / 32) + ((off % 32 + k) / 32) * s, bit (off + k) % 32 of each
 * plane (a strided sequence therefore starts at a multiple of 32). */
typedef struct scrg_pair_desc {
    uint64_t text_off;    /* (| SCRG_TEXT_REVCOMP on a handle with text strands enabled: the reverse complement of the stretch is the text) */
    uint64_t text_len;
    uint64_t read_off;    /* (| SCRG_READ_REVCOMP with scrg_params.stranded: the read's reverse complement is aligned) */
    uint64_t read_len;
    uint64_t cigar_off;   /* first run of this pair's slice, in scrg_run units; multiple of 16 */
    uint64_t cigar_cap;   /* slice capacity in runs; multiple of 16 (runs leave the GPU in
                             aligned 32-byte pieces), d_runs itself 32-byte aligned */
} scrg_pair_desc;

/* Aligns n_pairs problems.  Outputs: d_edit_distance[n], d_n_runs[n],
 * d_pair_status[n], runs in d_runs at each pair's slice.  d_pair_status[p]: 0 done, 1 its runs did not fit its slice,
 * 2 over the handle's edit limit (scrg_ctx_set_edit_limit: d_n_runs[p] = 0, d_edit_distance[p] = the running sum of edits
 * at the window where it went over; the host entry points report SCRG_PAIR_OVER_EDIT_LIMIT). */
scrg_status scrg_align_device(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                              const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                              scrg_run *d_runs, int64_t *d_edit_distance,
                              uint32_t *d_n_runs, uint32_t *d_pair_status);

/* The same alignment delivered as EDIT STREAMS (format below, "Edit stream") straight from the align kernel: pair p's
 * stream goes to its slice — bytes [2 * cigar_off, 2 * cigar_off + 2 * cigar_cap) of d_streams, i.e. the very slice
 * scrg_align_device would fill with runs, so descriptors and buffers can be shared —, d_stream_len[p] is its length
 * in bytes (the bytes up to the next multiple of 4 are zero), d_pair_status[p] is 1 if it did not fit, 2 if it went over the
 * handle's edit limit (stream length 0, d_n_runs[p] 0: drop such pairs by status before decoding) (a stream is
 * never longer than edit distance + number of windows + read_len / 63 bytes; a slice sized like the reference's,
 * cigar_cap = 2 x read length runs, always fits).  The kernel does less
 * work than for runs (it visits edits, not run boundaries) and writes a third of the bytes.
 * scrg_compact_runs with d_n_runs[p] = (d_stream_len[p] + 3) / 4 * 2 and even d_dense_offset gathers the slices.
 * d_n_runs may be NULL; otherwise d_n_runs[p] = the number of runs of the same alignment (what scrg_align_device
 * reports): sent along with the streams it lets the receiver lay out the decoded runs by a prefix sum and restore them
 * with ONE scrg_decode_edit_stream pass (no counting pass).
 * One-pair-per-lane kernels only: lanes_per_pair = 1 (the default for every W and O); SCRG_ERR_INVALID_ARG for the
 * GenASM-row mappings (use scrg_align_device + scrg_encode_edit_stream there).  d_streams 32-byte aligned. */
scrg_status scrg_align_device_edits(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                                    const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                                    uint8_t *d_streams, int64_t *d_edit_distance,
                                    uint32_t *d_stream_len, uint32_t *d_pair_status, uint32_t *d_n_runs);

/* Gathers every pair's runs from its slice into one dense array:
 * d_dense[d_dense_offset[p] + k] = d_runs[d_pairs[p].cigar_off + k]. */
scrg_status scrg_compact_runs(scrg_ctx *ctx, uint64_t n_pairs, const scrg_pair_desc *d_pairs,
                              const scrg_run *d_runs, const uint32_t *d_n_runs,
                              const uint64_t *d_dense_offset, scrg_run *d_dense);

/* The same gather into ONE BYTE per run — op in bits 7..6 (0 '=', 1 'X', 2 'I', 3 'D'), count in bits 5..0 — for
 * transfers (the RCCL gather of CIGARs to one GPU moves half the bytes).  A run never spans windows, so its count
 * is at most W-O; valid for W-O <= 63, i.e. every W <= 64 (SCRG_ERR_INVALID_ARG otherwise).  d_dense_offset is in
 * runs (= bytes).  scrg_unpack_runs restores scrg_run pairs bit for bit; both buffers 4-byte aligned. */
scrg_status scrg_compact_runs_packed(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                                     const scrg_pair_desc *d_pairs, const scrg_run *d_runs, const uint32_t *d_n_runs,
                                     const uint64_t *d_dense_offset, uint8_t *d_packed);
scrg_status scrg_unpack_runs(scrg_ctx *ctx, uint64_t n_runs, const uint8_t *d_packed, scrg_run *d_runs);

/* Distance-only alignment on device buffers (the kernels' third output mode): d_edit_distance[p], d_pair_status[p] (0, or 2 =
 * over the handle's edit limit: the running sum as the distance) and — d_text_end may be NULL — d_text_end[p] = the text
 * characters the alignment consumed (0 over the limit).  No run or stream buffer exists: the second traceback pass, the
 * staging ring and every store into a slice are not part of these kernels, and cigar_off / cigar_cap of the descriptors are
 * not looked at.  Enqueued on the handle's stream and not synchronised, like scrg_align_device; scrg_last_kernel_ms times
 * it; params as there (W, O, strides, stranded, waves_per_cu; params.outputs is not looked at), lanes_per_pair = 1 only.
 * scrg_query_launch with params.outputs = SCRG_OUT_DISTANCE reports this launch's geometry.  For scrg_select_best afterwards
 * pass a zero-filled d_n_runs. */
scrg_status scrg_align_device_distance(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                                       const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                                       int64_t *d_edit_distance, uint32_t *d_text_end, uint32_t *d_pair_status);

/* Best-candidate selection on the device, for callers that run their own pipeline (what SCRG_OUT_BEST does inside the host
 * entry points).  Groups are runs of consecutive pairs with equal d_group_key (the read's number, say; any uint32), of any
 * size.  In every group the pair with the smallest d_edit_distance among those whose d_pair_status is not 2 (over the edit
 * limit) wins, ties to the lowest index.  For every other pair that is not status 2: d_n_runs[p] = 0 and
 * d_pair_status[p] = 3 (eligible, not best; 0, 1 and 2 keep their meaning).  Winners and status-2 pairs are left alone.
 * d_is_best (may be NULL) gets 1/0 per pair.  Enqueued on the handle's stream, not synchronised, like scrg_compact_runs;
 * n_pairs < 2^32.  After it, scrg_compact_runs / scrg_compact_runs_packed with offsets made from the new d_n_runs gather
 * the winners' runs only.  Works after scrg_align_device, and after scrg_align_device_edits, where d_n_runs is the
 * d_stream_len array of that call (a loser's stream length becomes 0).  A new entry
 * point changes no existing one, so SCRG_ABI_VERSION stays. */
scrg_status scrg_select_best(scrg_ctx *ctx, uint64_t n_pairs, const uint32_t *d_group_key, const int64_t *d_edit_distance,
                             uint32_t *d_pair_status, uint32_t *d_n_runs, uint8_t *d_is_best);

/* Paired-end selection on the device, for callers that run their own pipeline (the rule: MATE PAIRS, above): it goes where
 * scrg_select_best goes, between the align launch and the compaction.  Reads 2m and 2m+1 are mate pair m: d_first[r] (2 n_mates + 1
 * entries, non-decreasing) is the index of read r's first pair in the per-pair arrays, so a read's candidates are consecutive and
 * a mate pair's two reads adjacent.  d_start, d_read_len (the pair's read's length), d_reverse (may be NULL: all forward),
 * d_edit_distance and d_pair_status (as an align call left it: 2 = over the edit limit, not eligible) are per pair.  Every
 * eligible pair that is not one of its mate pair's winners gets d_n_runs[p] = 0 and d_pair_status[p] = 3, exactly as
 * scrg_select_best leaves a loser; winners and status-2 pairs are left alone; d_is_best (may be NULL) gets 1/0 per pair;
 * d_records[m].winner[] are indices into these arrays.  Enqueued on the handle's stream and not synchronised: the candidate counts
 * are the device's to know, so a pass over d_first picks the team size (the lanes that share a mate pair, 4 .. 64) before the
 * selection kernel, whose grid is sized for teams of 64 (scrg_select_mates_team avoids both).  A mate pair with
 * n_a x n_b >= 2^32 is served as if it had no proper combination.  After scrg_align_device_distance pass a zero-filled d_n_runs.
 * An invalid rule is SCRG_ERR_INVALID_ARG; rule == NULL is the default (FR, any span, penalty 0). */
scrg_status scrg_select_mates(scrg_ctx *ctx, const scrg_mate_rule *rule, uint64_t n_mates, const uint64_t *d_first,
                              const uint64_t *d_start, const uint32_t *d_read_len, const uint8_t *d_reverse,
                              const int64_t *d_edit_distance, uint32_t *d_pair_status, uint32_t *d_n_runs, uint8_t *d_is_best,
                              scrg_mate_record *d_records);
/* The same for a caller that knows its candidate counts: team = 4, 8, 16, 32 or 64, at least the batch's largest
 * min(n_a x n_b, 64) (a smaller team is still correct: its lanes loop longer) — one launch with an exact grid, no pass over d_first.
 * team = 0 is scrg_select_mates; any other value is SCRG_ERR_INVALID_ARG. */
scrg_status scrg_select_mates_team(scrg_ctx *ctx, const scrg_mate_rule *rule, uint32_t team, uint64_t n_mates, const uint64_t *d_first,
                                   const uint64_t *d_start, const uint32_t *d_read_len, const uint8_t *d_reverse,
                                   const int64_t *d_edit_distance, uint32_t *d_pair_status, uint32_t *d_n_runs, uint8_t *d_is_best,
                                   scrg_mate_record *d_records);

/* The per-read summary and MAPQ on the device, for callers that run their own pipeline (the rule: READ SUMMARY AND MAPPING
 * QUALITY, above): it goes where scrg_select_best goes, after it or before it with the same records — it reads the distances and
 * the over-limit status (2) only, and a loser's status 3 is as eligible as the 0 it was.  d_first[r] (n_reads + 1 entries,
 * non-decreasing, at most n_pairs) is the index of read r's first pair: a read's candidates are consecutive, as for
 * scrg_select_mates; offsets that run backwards or past n_pairs name no candidates.  d_read_len (the pair's read's length),
 * d_edit_distance and d_pair_status are per pair and are not written.  d_out[r] is read r's record, winner as an index into these
 * arrays.  d_keep_status (may be NULL; n_pairs words, not d_pair_status itself) becomes a copy of d_pair_status in which every
 * status-0 pair that is not the winner of a KEPT read reads 3 — what scrg_pileup_add takes to sum the confidently placed reads
 * only; pairs that belong to no read are not written.  One launch: a lane serves a read of up to 16 candidates, a wavefront the
 * longer ones.  Enqueued on the handle's stream and not synchronised; n_pairs and n_reads below 2^32.  rule == NULL: the defaults;
 * an invalid rule or a NULL it needs is SCRG_ERR_INVALID_ARG; n_reads == 0 is SCRG_OK and launches nothing. */
scrg_status scrg_read_summary(scrg_ctx *ctx, const scrg_mapq_rule *rule, uint64_t n_reads, uint64_t n_pairs, const uint64_t *d_first,
                              const uint32_t *d_read_len, const int64_t *d_edit_distance, const uint32_t *d_pair_status,
                              scrg_read_record *d_out, uint32_t *d_keep_status);

/* Difference strings on device buffers (DIFFERENCE STRINGS, above), for callers that run their own pipeline: a length pass, the
 * caller's prefix sum, a render pass.  Both are enqueued on the handle's stream and not synchronised.
 *   Pair p's runs are d_runs[d_run_offset[p * run_offset_stride] + k] for k < d_n_runs[p]: stride 1 = a plain array (the dense
 *   runs after scrg_compact_runs); stride 6 = &d_pairs[0].cigar_off, the slices as scrg_align_device left them — d_n_runs[p] is
 *   then capped at cigar_cap.  Bases are fetched from d_seq as the descriptors name them (scrg_pair_desc: offset and word stride,
 *   params.text_stride_words / read_stride_words, any text_off % 32 in the contiguous layout); with params.stranded a pair with
 *   SCRG_READ_REVCOMP has the read as aligned — base k = the complement of packed base read_len - 1 - k.
 *   scrg_diff_lengths: d_diff_len[p] = the length of pair p's string incl. its NUL.
 *   scrg_diff_render : the string goes to d_diff_text + d_diff_offset[p]; d_diff_len is what the length pass wrote.  Offsets and
 *   lengths may come off a wire: a pair whose segment [d_diff_offset[p], + d_diff_len[p]) does not lie inside [0, diff_capacity),
 *   or whose d_diff_len[p] is not the length of its string, is counted in *d_bad_count and nothing of it is written.
 * A pair whose runs consume more text or more read than its descriptor holds, whose runs hold an operation other than = X I D or
 * a zero count, whose text_off carries SCRG_TEXT_REVCOMP (a leftward text would need its strings on the other strand) or whose
 * read_off carries SCRG_READ_REVCOMP without params.stranded, gets "" (length 1) in both passes, and the render pass counts it in
 * *d_bad_count.  No base outside a pair's sequences is read.  kind: SCRG_DIFF_MD or SCRG_DIFF_CS. */
scrg_status scrg_diff_lengths(scrg_ctx *ctx, const scrg_params *params, int32_t kind, uint64_t n_pairs,
                              const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                              const scrg_run *d_runs, const uint64_t *d_run_offset, uint64_t run_offset_stride,
                              const uint32_t *d_n_runs, uint64_t *d_diff_len);
scrg_status scrg_diff_render(scrg_ctx *ctx, const scrg_params *params, int32_t kind, uint64_t n_pairs,
                             const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                             const scrg_run *d_runs, const uint64_t *d_run_offset, uint64_t run_offset_stride,
                             const uint32_t *d_n_runs, const uint64_t *d_diff_len, const uint64_t *d_diff_offset,
                             char *d_diff_text, uint64_t diff_capacity, uint32_t *d_bad_count);

/* The CIGAR text on device buffers in any form (CIGAR FORMS, above), for callers that run their own pipeline: a length pass, the
 * caller's prefix sum, a render pass, shaped like scrg_diff_lengths / scrg_diff_render without the sequences.  Both are enqueued on
 * the handle's stream and not synchronised; the handle's own form setting plays no part.  Runs by offset and stride as there
 * (stride 1: dense runs; stride 6: &d_pairs[0].cigar_off, the slices, d_n_runs[p] capped at cigar_cap).
 *   scrg_cigar_text_lengths: d_text_len[p] = the length of pair p's text incl. its NUL.
 *   scrg_cigar_text_render : the text goes to d_text + d_text_offset[p].  In every form, a pair whose segment [d_text_offset[p],
 *   + d_text_len[p]) does not lie inside [0, text_capacity), or whose d_text_len[p] is not the length of its string, is counted in
 *   *d_bad_count and nothing of it is written.
 * Under SCRG_CIGAR_MERGED and SCRG_CIGAR_M a pair whose runs hold a zero count or an operation other than = X I D gets "" (length
 * 1) in both passes, and the render pass counts it.  SCRG_CIGAR_WINDOWED prints what the runs hold, as the pipeline always has. */
scrg_status scrg_cigar_text_lengths(scrg_ctx *ctx, int32_t form, uint64_t n_pairs, const scrg_run *d_runs,
                                    const uint64_t *d_run_offset, uint64_t run_offset_stride, const uint32_t *d_n_runs,
                                    uint64_t *d_text_len);
scrg_status scrg_cigar_text_render(scrg_ctx *ctx, int32_t form, uint64_t n_pairs, const scrg_run *d_runs,
                                   const uint64_t *d_run_offset, uint64_t run_offset_stride, const uint32_t *d_n_runs,
                                   const uint64_t *d_text_len, const uint64_t *d_text_offset, char *d_text,
                                   uint64_t text_capacity, uint32_t *d_bad_count);

/* The alignment report on device buffers (ALIGNMENT REPORT, above), for callers that run their own pipeline: one pass, enqueued
 * on the handle's stream and not synchronised.  Runs, offsets and counts as for scrg_diff_lengths (stride 1: dense runs; stride 6:
 * &d_pairs[0].cigar_off, the slices, d_n_runs[p] capped at cigar_cap); sequences as the descriptors and params name them (both
 * layouts, any text_off % 32 in the contiguous one; params.stranded for SCRG_READ_REVCOMP, the handle's text strands for
 * SCRG_TEXT_REVCOMP).  d_pair_status (may be NULL: every pair has an alignment) is what an align call or scrg_select_best left:
 * 2 and 3 have no alignment.  d_report[p] is written for every p < n_pairs; *d_fail_count (may be NULL) is incremented by the
 * number of pairs whose verdict is neither 0 nor SCRG_REPORT_NO_ALIGNMENT.  The base check compares 32 bases per step and reads
 * only words that hold a base of the pair's own sequences. */
scrg_status scrg_report_device(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                               const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                               const scrg_run *d_runs, const uint64_t *d_run_offset, uint64_t run_offset_stride,
                               const uint32_t *d_n_runs, const int64_t *d_edit_distance,
                               const uint32_t *d_pair_status, scrg_pair_report *d_report, uint32_t *d_fail_count);

/* The clip pass on device buffers (SOFT CLIPPING, above), for callers that run their own pipeline: enqueued on the handle's stream
 * and not synchronised.  Runs, offsets and counts as for scrg_report_device (stride 1: dense runs; stride 6: &d_pairs[0].cigar_off,
 * the slices, d_n_runs[p] capped at cigar_cap); no sequence is read.  d_pair_status (may be NULL: every pair is OK) is what an
 * align call or scrg_select_best left: a pair whose status is not 0 is not looked at.  costs: match, mismatch, gap_open, gap_extend
 * (NULL: 2, 4, 4, 2); the caller keeps (longest read + longest text) * max(match, mismatch, gap_open + gap_extend) below 2^31.
 * d_clip[p] is written for every p < n_pairs.  apply != 0: the kept stretch also becomes the pair's alignment for everything
 * downstream (compaction, the wire, the text in every CIGAR form) — d_n_runs[p] = the kept count, d_run_offset[p * stride] +=
 * first_run and, with stride 6, the capacity word behind it, d_run_offset[p * 6 + 1], -= first_run; a pair that was looked at and
 * has no '=' run gets d_n_runs[p] = 0; a pair that was not looked at is not modified.  The runs themselves are never written.
 * (Apply mode is a second, element-wise launch behind the pass.)  params: NULL or valid parameters; they play no part yet. */
scrg_status scrg_clip_device(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs, const scrg_run *d_runs,
                             uint64_t *d_run_offset, uint64_t run_offset_stride, uint32_t *d_n_runs,
                             const uint32_t *d_pair_status, const int32_t costs[4], int apply, scrg_pair_clip *d_clip);

/* The pileup on device buffers (PILEUP, above), for callers that run their own pipeline: both enqueued on the handle's stream and
 * not synchronised.
 * scrg_pileup_add: every counted pair of the batch is added to d_acc, [7][target_len + 1] words that the caller zeroed before the
 *   first add.  Runs, offsets and counts as for scrg_report_device (stride 1: dense runs; stride 6: &d_pairs[0].cigar_off, the
 *   slices, d_n_runs[p] capped at cigar_cap); params gives the sequence strides and `stranded` (a read flagged SCRG_READ_REVCOMP in
 *   a call that is not stranded is not counted).  Of the sequences only read bases under 'X' are read, and none past read_len.
 *   d_pair_status (may be NULL: every pair is OK) is what an align call or scrg_select_best left.  d_target_start[p]: where text
 *   column 0 of pair p lies in the target.  *d_out_of_range (may be NULL) is incremented by the number of pairs with a column or an
 *   insertion outside the target.  With the handle's text strands on the call is SCRG_ERR_INVALID_ARG.  Between adds d_acc holds
 *   planes 0 and 5 in EDGE FORM (+1 where a stretch of columns begins, -1 mod 2^32 one past its end): adds of several batches, from
 *   several streams at once, sum; it is not a result until it is finished.
 * scrg_pileup_finish: d_counts = the counts of d_acc (the prefix sums of planes 0 and 5 mod 2^32; the other planes copied).
 *   d_counts may equal d_acc (it may not overlap it otherwise); after an in-place finish the buffer takes no further adds.  The
 *   scratch (8 bytes per 4096 positions) belongs to the handle, as scrg_select_best's does. */
scrg_status scrg_pileup_add(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                            const uint64_t *d_seq, const scrg_pair_desc *d_pairs,
                            const scrg_run *d_runs, const uint64_t *d_run_offset, uint64_t run_offset_stride,
                            const uint32_t *d_n_runs, const uint32_t *d_pair_status,
                            const uint64_t *d_target_start, uint64_t target_len,
                            uint32_t *d_acc, uint32_t *d_out_of_range);
scrg_status scrg_pileup_finish(scrg_ctx *ctx, uint64_t target_len, const uint32_t *d_acc, uint32_t *d_counts);

/* The pileup sites on device buffers (PILEUP SITES, above): both enqueued on the handle's stream and not synchronised.
 * d_counts: [7][target_len + 1] in COUNTS form (what scrg_pileup_finish gives; it may be an accumulator finished in place); it is
 *   only read.  d_seq, genome_off: the target's bases in the library's linear 2-bit packing (32 bases per word, what
 *   scrg_pack_planar with stride 1 and scrg_genome_set leave), base 0 of the target at base genome_off of d_seq, any offset.
 * d_scratch: scrg_pileup_sites_scratch_bytes(target_len) bytes of the CALLER's, 8-byte aligned, need not be initialised: 16 bytes,
 *   and 516 per 4096 positions (a bitmap of the sites and a count per tile).  Two calls share no hidden handle state.
 * scrg_pileup_sites_mark: evaluates the rule at every position; *d_n_sites = the number of sites; the scratch then holds what
 *   scrg_pileup_sites_write needs (the rule included).  Nothing else is written.
 * scrg_pileup_sites_write: d_sites[k] = site k, in ascending pos, for k < min(*d_n_sites, cap) — records of index >= cap are not
 *   stored: the caller compares cap with *d_n_sites.  It takes the same target_len, d_counts, d_seq and genome_off as the mark whose
 *   scratch it reads.  (d_sites may be NULL if cap is 0.)
 * SCRG_ERR_INVALID_ARG: a rule that is refused, target_len >= 2^32 - 1, a NULL that is needed, a scratch that is not 8-byte aligned. */
size_t      scrg_pileup_sites_scratch_bytes(uint64_t target_len);
scrg_status scrg_pileup_sites_mark(scrg_ctx *ctx, uint64_t target_len, const uint32_t *d_counts, const uint64_t *d_seq,
                                   uint64_t genome_off, const scrg_site_rule *rule, void *d_scratch, uint64_t *d_n_sites);
scrg_status scrg_pileup_sites_write(scrg_ctx *ctx, uint64_t target_len, const uint32_t *d_counts, const uint64_t *d_seq,
                                    uint64_t genome_off, void *d_scratch, uint64_t cap, scrg_site *d_sites);

/* ---- Edit stream: the compact transfer format for CIGARs (multi-GPU gather, D2H) ----
 * The runs of a pair carry the alignment operations AND the places where a window ended (runs are flushed per window,
 * genasm_cpu.cpp:304-305, 400-403).  One byte per EDIT and one per WINDOW carries both (format version 2, ABI 6):
 *     byte = op << 6 | len     op 1 'X', 2 'I', 3 'D': `len` matches, then that edit;
 *                              op 0, len <= 62        : `len` matches, then the window ends (every window of a pair has
 *                                                       its END byte, the last one too);
 *                              op 0, len == 63 (0x3F) : 63 matches and nothing else (only W-O > 63 has such stretches)
 * in alignment order.  Canonical form: P matches before an edit or a window end = P / 63 bytes 0x3F, then the byte with
 * len = P % 63.  A 10 kb read at 10 % error and W-O = 31 is ~1.3 KB (2140 runs = 4.3 KB as scrg_run, 2.1 KB packed).
 * Valid for every W (run counts are <= W-O <= 255).  (Version 1 — ABI <= 5 — sent the edits only and the receiver replayed
 * the window loop: a quarter fewer bytes, three times the decoding work.)
 *
 * scrg_encode_edit_stream: for every pair, the stream of its runs (as scrg_align_device left them in d_runs; W-O of
 *   `params` places the window ends).
 *   Streams are placed in d_stream back to back in no particular order, each starting at a multiple of 4:
 *   d_stream_off[p] (bytes; ~0 if the pair did not fit into stream_cap) and d_stream_len[p] say where.
 *   d_total[0] = bytes of d_stream used (the amount to transfer), d_total[1] = pairs that did not fit.
 *   stream_cap >= sum over the pairs of (edit distance + 2 * (read_len + edit distance) / (W-O) + read_len / 63 + 8) always
 *   suffices (the read_len / 63 term is the 0x3F bytes, one per 63 matches in a row: only W-O > 63 has any).
 * scrg_decode_edit_stream: the inverse (streams of 64 bytes and more on average: one pair per wavefront, four stream bytes per
 *   lane side by side, runs staged in LDS and stored in aligned 16-byte units; shorter ones: one pair per lane, streams read in
 *   aligned 16-byte blocks, runs written in aligned 64-byte pieces — the same runs either way; the launch follows
 *   stream_bytes / n_pairs, the kernel then looks at a sample of d_stream_len itself, so a buffer sized for the worst case
 *   costs nothing).  d_stream holds stream_bytes bytes (16-byte aligned, readable up to the next
 *   multiple of 16): a pair whose stream is not inside [0, stream_bytes) — offsets and lengths may come off a wire —
 *   is counted as bad, never read.  Read lengths are taken from d_read_len[p * read_len_stride] (stride 1: a plain
 *   array; 6: &d_pairs[0].read_len; 0: one length for all).  `params` is not looked at beyond its validity (the window
 *   ends are in the stream).
 *   With d_dense == NULL it only counts: d_n_runs[p] = runs of pair p.  Otherwise d_n_runs[p] is an input, the size
 *   of pair p's segment at d_dense + d_dense_offset[p] (d_dense 16-byte aligned, room for dense_capacity runs), and the
 *   runs are written there — bit for bit the runs the align kernel produced.  Counts and offsets
 *   may come off a wire like the streams: a pair whose segment [d_dense_offset[p], + d_n_runs[p]) does not lie inside
 *   [0, dense_capacity) is counted as bad and nothing of it is written.  (scrg_align_device_edits can deliver the
 *   run counts along with the streams, so that the receiver sizes the dense array by a prefix sum and decodes in ONE
 *   pass.)  *d_bad_count is incremented for every pair whose stream is not an alignment of a read of that length
 *   (it does not end with a window end, places another number of read characters, holds a run longer than 255),
 *   or whose run count differs from d_n_runs[p]. */
scrg_status scrg_encode_edit_stream(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                                    const scrg_pair_desc *d_pairs,
                                    const scrg_run *d_runs, const uint32_t *d_n_runs,
                                    uint8_t *d_stream, uint64_t stream_cap,
                                    uint64_t *d_stream_off, uint32_t *d_stream_len, uint64_t *d_total);
scrg_status scrg_decode_edit_stream(scrg_ctx *ctx, const scrg_params *params, uint64_t n_pairs,
                                    const uint8_t *d_stream, uint64_t stream_bytes,
                                    const uint64_t *d_stream_off, const uint32_t *d_stream_len,
                                    const uint64_t *d_read_len, uint64_t read_len_stride,
                                    const uint64_t *d_dense_offset, scrg_run *d_dense, uint64_t dense_capacity,
                                    uint32_t *d_n_runs, uint32_t *d_bad_count);
/* The same two conversions for ONE pair on the host (no GPU, no handle): what a receiver without a GPU, or a
 * test, uses.  scrg_edit_stream_to_runs returns SCRG_ERR_INVALID_ARG for a malformed stream — it also checks that
 * every window ends where the reference's window loop of W/O ends it (genasm_cpu.cpp:307-310) — and
 * SCRG_ERR_CIGAR_OVERFLOW if runs_cap is too small (*n_runs is the number needed either way; runs may be NULL
 * with runs_cap 0 to ask for it).  scrg_runs_to_edit_stream likewise with stream_cap / *n_bytes; it replays the
 * window loop of W/O to place the window ends (SCRG_ERR_INVALID_ARG for an operation other than = X I D). */
scrg_status scrg_edit_stream_to_runs(const scrg_params *params, uint64_t read_len,
                                     const uint8_t *stream, uint64_t n_bytes,
                                     scrg_run *runs, uint64_t runs_cap, uint64_t *n_runs);
scrg_status scrg_runs_to_edit_stream(const scrg_params *params, const scrg_run *runs, uint64_t n_runs,
                                     uint8_t *stream, uint64_t stream_cap, uint64_t *n_bytes);
/* scrg_edit_stream_to_runs through the state machine the device decoder runs in every lane (same code, compiled for the
 * host): same arguments, same runs; like the device it does not look at the window geometry.  Lets a host without a
 * GPU — and the CPU tests — check that form too. */
scrg_status scrg_edit_stream_to_runs_lane(const scrg_params *params, uint64_t read_len,
                                          const uint8_t *stream, uint64_t n_bytes,
                                          scrg_run *runs, uint64_t runs_cap, uint64_t *n_runs);

/* Reference-layout 2-bit packer, mirrors the exported kernel
 * genasm_gpu::ascii_to_twobit_strings (src/genasm_gpu.cu:631-685): 4 bases per
 * byte, first base in bits 7..6, last byte zero-padded.  Each string occupies
 * ceil(len/4) bytes at d_twobit + d_twobit_off[s]. */
scrg_status scrg_ascii_to_twobit(scrg_ctx *ctx, uint64_t count, const uint64_t *d_lens,
                                 const uint64_t *d_ascii_off, const char *d_ascii,
                                 const uint64_t *d_twobit_off, uint8_t *d_twobit,
                                 uint32_t *d_bad_count);

/* Launch geometry for params on this device (for the bench's roofline line): persistent wavefronts, pairs per
 * wavefront, LDS bytes per wavefront.  It describes the kernel a launch that FILLS the GPU takes.  One exception is
 * decided per launch, by its size: with the default table (W <= 64, W-O <= 31, runs output) and waves_per_cu left at 0, a
 * launch of at most one wavefront per SIMD (n_pairs <= 64 x 4 x CUs) runs as workgroups of 512 threads — four producer and
 * four consumer wavefronts, 58 432 bytes of LDS per workgroup, two workgroups per CU.  A caller that sizes co-resident
 * work from these numbers sets waves_per_cu explicitly: the launch then has exactly the geometry reported here. */
scrg_status scrg_query_launch(scrg_ctx *ctx, const scrg_params *params,
                              int32_t *n_waves, int32_t *pairs_per_wave, int32_t *lds_bytes,
                              int32_t *n_cus);

/* Times the most recent scrg_align_device launch with HIP events recorded on
 * the launch stream (milliseconds); blocks until that launch finished. */
scrg_status scrg_last_kernel_ms(scrg_ctx *ctx, float *ms);

/* scrg_params.reserved[] in the SHIPPED library: both must be 0; scrg_params_resolve() and every entry point REJECT anything
 * else, and none of the code below exists in the shipped kernels or in the shipped kernel selection.
 *
 * Test build only (-DSCRG_SELECT: ab_libs/lib_select.so, scrooge_amd.build_library("select"); scrg_build_flags() tells):
 * reserved[0] selects between formulations that give identical results, for the parity tests that compare them —
 * 32 (lanes_per_pair = 8: GenASM rows only, no diagonal-major path), 256 (32 <= W-O <= 127: the kernel that keeps the
 * window table in HBM instead of the one that keeps it in registers), 512 / 1024 (W <= 64, W-O <= 31, runs output: always /
 * never the variant of the default kernel that splits a window's work over two wavefronts; by default a launch that cannot
 * put two wavefronts on every SIMD takes it), 4096 / 8192 (genasm_lane_kernel: never sweep the window table's 32-row band /
 * sweep it in every eligible round, without the back-off), 16384 (scrg_report_device: the base check one base at a time instead of
 * 32 per step).
 *
 * Profiling builds only (scripts/ab.sh; they include the selections above): with -DSCRG_STATS the align kernels accumulate
 * twelve counters per launch when reserved[1] != 0, read back by scrg_debug_stats (blocks on the stream):
 *   lanes_per_pair = 1 (genasm_lane_kernel): [0] window rounds (one window of each of a wavefront's 64 pairs),
 *     (above bit 32: rounds eligible for the band table that the back-off left to the full table),
 *     [1] rounds that took a short-window variant (bits 0..20; 21..41: rounds that swept the band table, 42..62: those of
 *     them redone on the full table), [2..6] shader cycles summed over wavefronts: traceback pass 1,
 *     queue/fetch, window setup, table, traceback (both passes + CIGAR flush), [7] wavefront life times and
 *     [8..11] latest start, 2^62 - earliest start, latest end, 2^62 - earliest end on the 100 MHz wall clock.
 *   lanes_per_pair >= 4 (genasm_align_kernel): {window rounds, DC sweep steps, TB macro-steps, shader cycles for
 *     fetch / window setup / DC / TB / TB loop, rounds on the diagonal-major path, rounds that fell back from it,
 *     DC / TB cycles of the diagonal-major rounds (not included in the former)};
 * and reserved[0] also accepts the scheduling switches 1 (one pair per lane: no wavefront priority rotation) and
 * 64 / 128 (workgroups of one / two wavefronts instead of four).  With -DSCRG_ABLATE also 2, 4, 8, 16 (skip the table,
 * a traceback pass, the stores: results wrong by design).  None of this code exists in the shipped kernels; there
 * scrg_debug_stats returns SCRG_ERR_INVALID_ARG. */
scrg_status scrg_debug_stats(scrg_ctx *ctx, uint64_t out[12]);

#ifdef __cplusplus
}
#endif
#endif /* SCROOGE_AMD_H */
