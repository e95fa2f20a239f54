// genasm_kernels.h — launch interface between the C-ABI host code
// (scrg_api.cpp) and the gfx950 kernels (genasm_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/scrooge_amd.h"

namespace scrg {

// rows of the HBM spill area per pair slot: K+1 = 65 rows of R can exist, plus
// the rows lanes ahead of the slot leader run past the final row
constexpr int SPILL_ROWS = 72;
// (genasm_kernel_multiword.hip, 64 < W <= 256, sizes its spill area as W+1 rows of stored_row_dwords())

struct AlignArgs {
    const uint64_t* seq;          // planar 2-bit words
    const scrg_pair_desc* pairs;
    uint16_t* runs;               // scrg_run as count | op << 8
    int64_t* ed;
    union {                       // (one kernel argument: the struct is what it was before LANE_OUT_NONE existed, and so are the kernels of the other modes)
        uint32_t* n_runs;
        uint32_t* text_end;       // LANE_OUT_NONE, which has no runs to count; may be null: the text characters a pair's alignment consumed (its final ref_idx)
    };
    uint32_t* status;
    uint32_t* run_count;          // edit-stream output only, may be null: the number of runs the same alignment has (what
                                  //   scrg_align_device would report in n_runs), so that a receiver can size the decoded array
    uint32_t* counter;            // work queue head, zeroed before launch
    uint32_t* spill;              // grid * slots * SPILL_ROWS * 32 words
    uint32_t n_pairs;
    int32_t W;
    int32_t tb_limit;             // W - O
    int32_t lds_rows;
    uint32_t text_stride;         // words between consecutive words of a text / a read in seq (1 = contiguous;
    uint32_t read_stride;         //   64 = lane-interleaved groups, scrg_pack_planar_groups; lane kernel only)
    uint64_t* stats;              // profiling builds (-DSCRG_STATS) only: counters, may be null; never read by the shipped kernels
    int32_t debug;                // params.reserved[0] (always 0 in the shipped build): see SCRG_SEL / SCRG_SW / SCRG_ABL below
    uint32_t stranded;            // params.stranded: bit 63 of a pair's read_off = align the read's reverse complement (the one-pair-per-lane kernels)
    uint32_t max_edits;           // the handle's edit limit (scrg_ctx_set_edit_limit; one-pair-per-lane kernels): 0xffffffff = none
    uint32_t per_mille;           //   and its part per read base, 0 = none (lane_common.h: pair_edit_limit)
    uint32_t text_rev;            // the handle's text-strand setting (scrg_ctx_set_text_strands; one-pair-per-lane kernels): bit 63 of a pair's
                                  //   text_off = align against the reverse complement of the stretch (text_revcomp.h); 0: the bit is not looked at
};
// What the one-pair-per-lane kernels deliver for a pair, besides its edit distance and status:
//   RUNS   runs (scrg_run) in the pair's slice, their number in n_runs                                  (scrg_align_device)
//   EDITS  an edit stream in the pair's slice, its bytes in n_runs, the runs' number in run_count       (scrg_align_device_edits)
//   NONE   text_end alone: a round is fetch -> set-up -> table -> traceback pass 1.  The second pass, the staging ring, the
//          insertion-run lengths and every store into a slice are not compiled in; runs, n_runs, run_count and the
//          descriptors' cigar_off / cigar_cap are not looked at; status is 0 or LANE_STATUS_OVER_EDIT_LIMIT (scrg_align_device_distance)
enum LaneOutput : int { LANE_OUT_RUNS = 0, LANE_OUT_EDITS = 1, LANE_OUT_NONE = 2 };
// f(std::integral_constant<int, OUT>{}) for the OUT that `out` names: how a launcher picks its kernel's LaneOutput template argument
template <typename F> inline void with_lane_output(LaneOutput out, F&& f)
{
    if (out == LANE_OUT_NONE) f(std::integral_constant<int, LANE_OUT_NONE>{});
    else if (out == LANE_OUT_EDITS) f(std::integral_constant<int, LANE_OUT_EDITS>{});
    else f(std::integral_constant<int, LANE_OUT_RUNS>{});
}
// d_pair_status.  OVERFLOW: the pair's output did not fit its slice.  OVER_EDIT_LIMIT: retired because its running sum of edits
// went over its limit (lane_common.h: abandon_pair).  NOT_BEST: eligible (not over the limit) but not the best candidate of its
// group (select_kernels.hip; never written by an align kernel).  The host entry points report them as SCRG_ERR_CIGAR_OVERFLOW,
// SCRG_PAIR_OVER_EDIT_LIMIT and SCRG_PAIR_NOT_BEST (host_path.h: public_status).
enum LaneStatus : uint32_t { LANE_STATUS_DONE = 0, LANE_STATUS_OVERFLOW = 1, LANE_STATUS_OVER_EDIT_LIMIT = 2, LANE_STATUS_NOT_BEST = 3 };

// scrg_params.reserved[0] / reserved[1].  The SHIPPED library accepts neither: scrg_params_resolve() rejects every bit.
// Everything they can do is experiment and test plumbing and exists only in other builds of the same sources (scripts/ab.sh;
// scrooge_amd.build_library(variant=...) for the test build):
//   -DSCRG_SELECT  the test build (ab_libs/lib_select.so): reserved[0] selects between formulations that give IDENTICAL results,
//                  which the parity tests compare — 32 (lanes_per_pair = 8: no diagonal-major path), 256 (the kernel with the
//                  window table in HBM where one that keeps it in registers would serve), 512 / 1024 (the default kernel as two
//                  wavefronts per 64 pairs / as one, whatever the launch size), 4096 / 8192 (the default kernel's window table never /
//                  in every eligible round swept as a 32-row band first: genasm_lane_kernel.hip, lane_window_table_band), 16384 (the
//                  alignment report's base check one base at a time: report_kernels.hip, PER_BASE);
//   -DSCRG_STATS   (implies SELECT) the kernels' counters (reserved[1] != 0 -> scrg_debug_stats: window rounds, shader cycles
//                  per part, wavefront life times) and the scheduling switches 1 (one pair per lane: no wavefront priority
//                  rotation), 64 / 128 (workgroups of one / two wavefronts) — results intact;
//   -DSCRG_ABLATE  (implies STATS) the ablation switches 2, 4, 8, 16 and 1 for the GenASM-row kernel: skip the table, the
//                  runs, the walk, the stores — results are WRONG by design (bench.py --ablate).
// In the shipped build SCRG_TIMING / SCRG_SW / SCRG_ABL / SCRG_SEL are compile-time false: no counter, no clock read, no exit
// atomic and no switch test is left in the kernels or in the kernel selection.
#if defined(SCRG_ABLATE) && !defined(SCRG_STATS)
#define SCRG_STATS 1
#endif
#if defined(SCRG_STATS) && !defined(SCRG_SELECT)
#define SCRG_SELECT 1
#endif
constexpr int32_t SCRG_SWITCH_NO_DIAG = 32;       // lanes_per_pair = 8: GenASM rows only (no diagonal-major path)
constexpr int32_t SCRG_SWITCH_MW_TABLE = 256;     // genasm_lane_mw_kernel (table in HBM) where genasm_lane_wide_kernel / genasm_lane_parts_kernel (table in registers) would serve
constexpr int32_t SCRG_SWITCH_SPLIT = 512;        // W <= 64, W-O <= 31, runs output: genasm_lane_split_kernel (a window's work on two wavefronts) whatever the launch size
constexpr int32_t SCRG_SWITCH_NO_SPLIT = 1024;    // ... genasm_lane_kernel whatever the launch size (default: by launch size, scrg_api.cpp)
constexpr int32_t SCRG_SWITCH_NO_BAND = 4096;     // genasm_lane_kernel: never sweep the window table's 32-row band (every round on the full table)
constexpr int32_t SCRG_SWITCH_BAND_ALWAYS = 8192; // ... sweep it in every eligible round: no back-off
constexpr int32_t SCRG_SWITCH_REPORT_PER_BASE = 16384; // scrg_report_device: the base check one base at a time (report_kernels.hip, PER_BASE) instead of 32 per step
constexpr int32_t SCRG_SAFE_SWITCHES = SCRG_SWITCH_NO_DIAG | SCRG_SWITCH_MW_TABLE | SCRG_SWITCH_SPLIT | SCRG_SWITCH_NO_SPLIT | SCRG_SWITCH_NO_BAND | SCRG_SWITCH_BAND_ALWAYS |
                                       SCRG_SWITCH_REPORT_PER_BASE;
#ifdef SCRG_SELECT
#define SCRG_SEL(flags, bit) (((flags) & (bit)) != 0)
constexpr bool SCRG_HAVE_SELECT = true;
#else
#define SCRG_SEL(flags, bit) false
constexpr bool SCRG_HAVE_SELECT = false;
#endif
#ifdef SCRG_STATS
#define SCRG_TIMING(args) ((args).stats != nullptr)
#define SCRG_SW(args, bit) (((args).debug & (bit)) != 0)
constexpr bool SCRG_HAVE_STATS = true;
#else
#define SCRG_TIMING(args) false
#define SCRG_SW(args, bit) false
constexpr bool SCRG_HAVE_STATS = false;
#endif
#ifdef SCRG_ABLATE
#define SCRG_ABL(args, bit) (((args).debug & (bit)) != 0)
constexpr int32_t SCRG_ALLOWED_SWITCHES = 0x1ff | SCRG_SAFE_SWITCHES;
#elif defined(SCRG_STATS)
#define SCRG_ABL(args, bit) false
constexpr int32_t SCRG_ALLOWED_SWITCHES = SCRG_SAFE_SWITCHES | 1 | 64 | 128;
#elif defined(SCRG_SELECT)
#define SCRG_ABL(args, bit) false
constexpr int32_t SCRG_ALLOWED_SWITCHES = SCRG_SAFE_SWITCHES;
#else
#define SCRG_ABL(args, bit) false
constexpr int32_t SCRG_ALLOWED_SWITCHES = 0;
#endif

#ifdef __HIPCC__
#define SCRG_HD __host__ __device__
#else
#define SCRG_HD
#endif

hipError_t launch_align(int lanes_per_pair, const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s);
hipError_t launch_align_multiword(int lanes_per_pair, const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s);
// lanes_per_pair = 1: one pair per lane, 64 pairs per wavefront (genasm_lane_kernel.hip; W <= 64, W-O <= 31)
// (out: LaneOutput above)
hipError_t launch_align_lane(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out = LANE_OUT_RUNS);
// LDS per wavefront: the CIGAR staging ring (32 runs + 1 dword), a window's insertion-run lengths, the Eq table and the "no match"
// word, per lane; LANE_OUT_NONE: the Eq table and the "no match" word alone
SCRG_HD inline unsigned lane_lds_bytes(LaneOutput out = LANE_OUT_RUNS) { return 64u * ((out == LANE_OUT_NONE ? 0u : 68u + 36u) + 32u + 8u); }
// the same alignment (runs output) with a window's work split over a producer and a consumer wavefront (genasm_lane_kernel.hip:
// genasm_lane_split_kernel): for launches that cannot fill the SIMDs.  grid counts producer wavefronts; 8 resident per CU.
hipError_t launch_align_lane_split(const AlignArgs& a, int grid, hipStream_t s);
constexpr int LANE_SPLIT_PRODUCERS_PER_CU = 8;

// dwords of one stored row of R (the part the traceback can reach):
//   W <= 64: the high dword of columns 0..31, or whole entries of all 64 columns when W-O > 31;
//   W  > 64: words 0..SW-1 of columns 0..64*SW-1 with SW = (W-O)/64 + 1.
// genasm_lane_mw_kernel (W-O > 31 or W > 64): LDS per wavefront = CIGAR ring + one length byte for each of the W-O columns
// (LANE_OUT_NONE: none at all); its table — two rows of (W-O)/64 + 1 64-bit words for each of the W-O columns, for 64 lanes — is a slab of HBM
SCRG_HD inline unsigned lane_mw_len_bytes(int tb_limit) { return (((unsigned)tb_limit + 3u) & ~3u) + 4u; }
SCRG_HD inline unsigned lane_mw_lds_bytes(int tb_limit, LaneOutput out = LANE_OUT_RUNS) { return out == LANE_OUT_NONE ? 0u : 64u * (68u + lane_mw_len_bytes(tb_limit)); }
SCRG_HD inline size_t lane_mw_table_bytes(int tb_limit) { return (size_t)tb_limit * 2u * ((unsigned)tb_limit / 64u + 1u) * 64u * 8u; }
hipError_t launch_align_lane_mw(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out = LANE_OUT_RUNS);
// genasm_lane_wide_kernel (one pair per lane, W <= 128, 32 <= W-O <= 63): the table in registers, built in two halves.
// LDS per wavefront and lane: CIGAR ring, 32 insertion-run lengths (neither with LANE_OUT_NONE), the window's Eq words for the
// four bases and "no match".
SCRG_HD inline bool lane_wide_serves(int W, int tb_limit) { return W <= 128 && tb_limit >= 32 && tb_limit <= 63; }
SCRG_HD inline unsigned lane_wide_lds_bytes(int W, LaneOutput out = LANE_OUT_RUNS) { return 64u * ((out == LANE_OUT_NONE ? 0u : 68u + 36u) + (W <= 64 ? 40u : 80u)); }
hipError_t launch_align_lane_wide(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out = LANE_OUT_RUNS);
// genasm_lane_parts_kernel (one pair per lane, W <= 256, 64 <= W-O <= 127 — or W > 128 with any W-O <= 63 —: two-word table rows): the table in registers, built
// in parts of 16 columns from checkpoints of the difference vectors.  LDS per wavefront and lane: CIGAR ring, 16 insertion-run
// lengths (neither with LANE_OUT_NONE), the window's Eq words for the four bases and "no match" (NW words each, slots of 16 or 32 bytes), the window's text.
// HBM per wavefront: 8 checkpoints of 4 NW dwords per lane.
// (Round 5: also W > 128 with W-O <= 63 — 1 to 4 parts, rows in the first word only — which the two-halves kernel, W <= 128, does
// not reach; genasm_lane_mw_kernel is left with W-O >= 128: table rows of three and four words.)
SCRG_HD inline bool lane_parts_serves(int W, int tb_limit)
{
    return W > 64 && W <= 256 && ((tb_limit >= 64 && tb_limit <= 127) || (W > 128 && tb_limit >= 1 && tb_limit <= 63));      // (W = 64, O = 0: genasm_lane_mw_kernel)
}
SCRG_HD inline unsigned lane_parts_lds_bytes(int W, LaneOutput out = LANE_OUT_RUNS)
{
    const unsigned nw = ((unsigned)W + 63u) / 64u, slot = nw == 2u ? 16u : 32u;
    return 64u * ((out == LANE_OUT_NONE ? 0u : 68u + 20u) + 5u * slot + 16u * nw);
}
SCRG_HD inline size_t lane_parts_checkpoint_bytes(int W) { return (size_t)8u * 4u * (((unsigned)W + 63u) / 64u) * 64u * 4u; }
hipError_t launch_align_lane_parts(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out = LANE_OUT_RUNS);

SCRG_HD inline unsigned stored_row_dwords(int W, int tb_limit)
{
    if (W <= 64) return tb_limit > 31 ? 128u : 32u;
    const unsigned sw = (unsigned)tb_limit / 64u + 1u;
    return 64u * sw * sw * 2u;
}

// dwords of LDS per pair slot for the table R: lds_rows stored rows + 1 (slots land on distinct banks).
// The G = 8 kernel's diagonal-major path (W = 64, W-O <= 31) keeps 16 rows in its own compacted
// layout — 8 rows x 32 diagonals, 8 rows x 16, 4 dwords where idle lanes park their stores — and needs
// 397 dwords whatever lds_rows says.
constexpr unsigned DIAG_WIDE_ROWS = 8;                    // rows 0..7: all 32 diagonals, 32 dwords each
constexpr unsigned DIAG_LATE_BASE = 128;                  // rows r >= 8: diagonal x at 128 + 16 r + x (x = 8..23), i.e. from dword 264
constexpr unsigned DIAG_PARK_DWORD = 392;                 // lanes without a late diagonal park their four stores here
constexpr unsigned DIAG_SLOT_DWORDS = DIAG_PARK_DWORD + 4 + 1;     // 397
SCRG_HD inline unsigned slot_stride_dwords(int W, int tb_limit, int lanes_per_pair, int lds_rows)
{
    unsigned s = (unsigned)lds_rows * stored_row_dwords(W, tb_limit) + 1u;
    if (W == 64 && lanes_per_pair == 8 && tb_limit <= 31 && s < DIAG_SLOT_DWORDS) s = DIAG_SLOT_DWORDS;
    return s;
}

// ---- which kernel serves a launch, and what the host needs to launch it: the ONE statement of the choice on the library's side
// (tests/plane_inputs.py: kernel_class and the README state it independently)
enum AlignForm : int {
    FORM_ROWS,          // GenASM rows, lanes_per_pair >= 4, W <= 64          (genasm_kernels.hip)
    FORM_ROWS_MW,       // GenASM rows, lanes_per_pair 32 | 64, W > 64        (genasm_kernel_multiword.hip)
    FORM_LANE,          // one pair per lane from here on: W <= 64, W-O <= 31 (genasm_lane_kernel.hip; its split form is chosen by launch size, scrg_api.cpp)
    FORM_LANE_WIDE,     // lane_wide_serves                                   (genasm_lane_wide_kernel.hip)
    FORM_LANE_PARTS,    // lane_parts_serves                                  (genasm_lane_parts_kernel.hip)
    FORM_LANE_MW,       // the rest, W = 64 with O = 0 included               (genasm_lane_mw_kernel.hip)
};
// mw_table: SCRG_SEL(reserved[0], SCRG_SWITCH_MW_TABLE) — the constant false in the shipped build
SCRG_HD inline AlignForm align_form(int W, int tb_limit, int lanes_per_pair, bool mw_table)
{
    if (lanes_per_pair != 1) return W <= 64 ? FORM_ROWS : FORM_ROWS_MW;
    if (!mw_table && lane_wide_serves(W, tb_limit)) return FORM_LANE_WIDE;
    if (!mw_table && lane_parts_serves(W, tb_limit)) return FORM_LANE_PARTS;
    return W > 64 || tb_limit > 31 ? FORM_LANE_MW : FORM_LANE;
}
struct LaunchPlan {
    AlignForm form;
    size_t lds_bytes;                // LDS per wavefront
    int default_waves_per_cu;        // where scrg_params.waves_per_cu is 0
    size_t spill_bytes;              // HBM scratch (the handle's spill area) per wavefront ...
    int spill_group;                 // ... of whole groups of this many wavefronts
    int pairs_per_wave;
    size_t spill_for(int n_waves) const { return (size_t)((n_waves + spill_group - 1) / spill_group * spill_group) * spill_bytes; }
};
// p: resolved (W, O, lanes_per_pair and lds_rows are looked at)
SCRG_HD inline LaunchPlan launch_plan(const scrg_params& p, LaneOutput out, AlignForm form)
{
    const int T = p.W - p.O;
    LaunchPlan l{form, 0, 16, 0, 1, 64 / p.lanes_per_pair};
    switch (form) {
    case FORM_LANE:             // (the table in registers: nothing spills)
        l.lds_bytes = lane_lds_bytes(out);
        break;
    case FORM_LANE_WIDE:        // its table takes 128 registers: two wavefronts per SIMD
        l.lds_bytes = lane_wide_lds_bytes(p.W, out);
        l.default_waves_per_cu = 8;
        break;
    case FORM_LANE_PARTS:       // its checkpoints: one slab of HBM per wavefront (workgroups of four); up to 256 VGPRs
        l.lds_bytes = lane_parts_lds_bytes(p.W, out);
        l.default_waves_per_cu = 8;
        l.spill_bytes = lane_parts_checkpoint_bytes(p.W);
        l.spill_group = 4;
        break;
    case FORM_LANE_MW:          // its window tables: one slab of HBM per wavefront.  (W = 64, O = 0 keeps 16 wavefronts per CU: one-word vectors)
        l.lds_bytes = lane_mw_lds_bytes(T, out);
        l.default_waves_per_cu = p.W > 64 ? 8 : 16;
        l.spill_bytes = lane_mw_table_bytes(T);
        break;
    case FORM_ROWS:
    case FORM_ROWS_MW:
        // per slot: CIGAR staging ring (16 dwords) + 1 scratch dword + R rows (+1 dword against bank conflicts); 8 dwords of
        // padding at the end (the traceback's speculative lanes read a little past a row).  A row is 32 DENT dwords, or 64
        // whole entries when W-O > 31 (the kernel's WIDE variant); see stored_row_dwords() for W > 64.
        l.lds_bytes = ((size_t)l.pairs_per_wave * (17 + (size_t)slot_stride_dwords(p.W, T, p.lanes_per_pair, p.lds_rows)) + 8) * sizeof(uint32_t);
        // 11 and 12 wavefronts per CU align equally fast (the kernel is issue-bound); 11 leaves VGPRs and LDS on
        // every CU for kernels of other streams (RCCL's gather in bench.py --gpus N).  The LDS footprint caps it.
        l.default_waves_per_cu = 11;
        l.spill_bytes = (size_t)l.pairs_per_wave * (p.W > 64 ? (size_t)p.W + 1 : (size_t)SPILL_ROWS) * stored_row_dwords(p.W, T) * sizeof(uint32_t);
        break;
    }
    return l;
}

hipError_t launch_pack_planar(const char* d_ascii, uint64_t n_words, uint64_t* d_planar, uint32_t* d_bad,
                              int n_cus, hipStream_t s);
hipError_t launch_pack_planar_groups(const char* d_ascii, uint64_t n_rows, uint64_t words_per_row, uint64_t* d_planar,
                                     uint32_t* d_bad, int n_cus, hipStream_t s);
hipError_t launch_ascii_to_twobit(uint64_t count, const uint64_t* d_lens, const uint64_t* d_ascii_off,
                                  const char* d_ascii, const uint64_t* d_twobit_off, uint8_t* d_twobit,
                                  uint32_t* d_bad, uint64_t max_len, hipStream_t s);
hipError_t launch_compact_runs(uint64_t n_pairs, const scrg_pair_desc* d_pairs, const uint16_t* d_runs,
                               const uint32_t* d_n_runs, const uint64_t* d_dense_off, uint16_t* d_dense,
                               int n_cus, hipStream_t s);

hipError_t launch_compact_runs_packed(uint64_t n_pairs, const scrg_pair_desc* d_pairs, const uint16_t* d_runs,
                                      const uint32_t* d_n_runs, const uint64_t* d_dense_off, uint8_t* d_dense,
                                      int n_cus, hipStream_t s);
hipError_t launch_unpack_runs(uint64_t n_runs, const uint8_t* d_packed, uint16_t* d_runs, int n_cus, hipStream_t s);

}  // namespace scrg
