// genasm_lane_parts_kernel.hip — the lane-per-pair aligner for 64 <= W-O <= 127 (W <= 256; and W > 128 with W-O <= 63): the formulation of
// genasm_lane_kernel.hip (every lane aligns its own pair; the window's table holds the differences of the edit-distance
// matrix behind the GenASM bitvectors, src/genasm_cpu.cpp:210-409 — see the header of that file for why this gives the
// reference's edit distance and CIGAR bit for bit) with multi-word vectors (NW = ceil(W/64) words of 64 pattern rows,
// word 0 the most significant; src/bitvector.hpp:45-48, 124-139) for the reference's large-window sweep points
// (scripts/profile.py:180-185: W = 160 ... 256 with O = W/2 + 1), where a window's traceback may consume up to 127
// characters: a table row is two 64-bit words, W-O columns of two such rows are 8 (W-O) dwords = 4 KB per lane — thirty
// times the registers of a wavefront.  genasm_lane_mw_kernel.hip keeps that table in HBM (0.5 MB written and read back per
// wavefront and window: 3.4 TB/s with the VALU idle half of the time).
//
// Here the table exists only in PARTS of 16 columns, all held in the same 128 registers.  The recurrence runs from the
// last text column down, the walk from column 0 up, so:
//   1. ONE sweep over all W columns (a run-time loop over chunks of 16 columns, the 16 unrolled) keeps the table of
//      columns 0..15 and, on its way, leaves a CHECKPOINT — the difference vectors Pv, Mv in front of a chunk, 4 NW
//      dwords per lane — for each of the chunks 1 .. ceil((W-O)/16) - 1 in a slab of HBM (word-interleaved over the
//      lanes: 512 contiguous bytes per store; 7 x 64 bytes per lane and window at W = 256 instead of 2 x 4 KB);
//   2. the walk consumes part 0; then, part by part, the chunk's 16 columns are swept AGAIN from their checkpoint,
//      this time keeping the table, and the walk goes on from where it stood.
// W + (W-O) - 16 swept columns per window instead of W, no table traffic, no data-dependent slow path.  Chunks that lie
// past the end of every lane's text are skipped (a column past the end leaves the vectors as they are).
//
// Shared with genasm_lane_wide_kernel.hip, in lane_multiword.h: the pair state and claim loop, the window set-up, one column
// of the recurrence, and the second pass.  Here: the checkpoints, the one-word walk modes, and the text in LDS.
//
// Each part ends with its own second pass (masks -> runs or edit-stream bytes: part_events, part_runs / part_edits, 16 columns
// at a time; with LANE_OUT_NONE part_events alone: the part's edits and text columns); a run that crosses from one part into the next is ONE run of the window (the reference merges within a
// window, src/genasm_cpu.cpp:372-404), as with the wide kernel's two halves.
// tests/proto/lane_proto.c (lane_align_codes_mw) restates the multi-word arithmetic; tests/test_gpu_parity.py holds this
// kernel against the CPU checker, the table-in-HBM kernel and the reference-built fixtures at W/O = 192/97, 200/50,
// 256/129, 128/20.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "lane_multiword.h"

namespace scrg {

namespace {

constexpr int PT_COLS = 16;                      // columns per part / chunk
constexpr uint32_t PT_RING_BYTES = 68;           // 32 runs + one dword: lanes land on distinct LDS banks
constexpr uint32_t PT_SCRATCH_BYTES = 20;        // insertion-run length of each column of a part, one byte each (+ bank skew)
constexpr int PT_EQ_AHEAD = 2;                   // Eq words are read from LDS this many columns ahead of their use

// the 64 bits of the 128-bit row {w0 (rows 0..63, row r at bit 63-r), w1 (rows 64..127)} from row s on (s < 128), zeros after the row's end
__device__ __forceinline__ uint64_t pt_from_row(uint64_t w0, uint64_t w1, uint32_t s)
{
    const bool far = s >= 64u;
    const uint64_t hi = far ? w1 : w0, lo = far ? 0ull : w1;
    const uint32_t b = s & 63u;
    return shl64(hi, b) | shr64(lo >> 1, 63u - b);
}

// One chunk: its 16 columns, 15 .. 0 (descending).  xe / xo hold the chunk's text characters, two bits each, next to each
// other (xe: bits c, c + 1 = lo, hi bit of every EVEN column c; xo: bits c - 1, c of every ODD column c — see
// genasm_lane_kernel.hip), so that the LDS address of a column's Eq words is one shift and one v_bitop3.
// STORE: the columns go to tab[c] = {~(V1 | stop), V0 | stop}, rows 0..127 (words 0 and 1 of the vectors).
// SHORT: some lane's text ends inside the chunk: columns c >= nrel read the Eq words "no character matches", which leave
// the vectors as they are (the boundary column D[n][j] = m-j, genasm_cpu.cpp:239-245).
template <int NW, bool STORE, bool SHORT>
__device__ __forceinline__ void pt_sweep16(LaneVec<NW>& st, const uint32_t xe, const uint32_t xo, const int32_t nrel, const uint2 (&stop)[2],
                                           uint64_t (&tab)[PT_COLS][2][2], const uint32_t eq_b, const uint32_t nomatch_b)
{
    constexpr int SLOT_SHIFT = NW == 2 ? 4 : 5;                      // a base's NW words: 16 or 32 bytes (NW = 3: padded)
    auto eq_addr = [&](int c) -> uint32_t {
        const uint32_t x = (c & 1) ? xo : xe;
        const int f = (c & 1) ? c - 1 : c;                                      // the field's low bit; it goes to bit SLOT_SHIFT
        const uint32_t u = f >= SLOT_SHIFT ? x >> (f - SLOT_SHIFT) : x << (SLOT_SHIFT - f);
        const uint32_t a = bitop3<TT_ANDOR>(u, 3u << SLOT_SHIFT, eq_b);
        return (!SHORT || c < nrel) ? a : nomatch_b;
    };
    uint2 eqw[PT_EQ_AHEAD][NW];
#pragma unroll
    for (int k = 0; k < PT_EQ_AHEAD; k++) {
        const uint32_t ad = eq_addr(PT_COLS - 1 - k);
#pragma unroll
        for (int q = 0; q < NW; q++) eqw[k][q] = lds_read64(ad + 8u * q);
    }
#pragma unroll
    for (int c = PT_COLS - 1; c >= 0; c--) {
        uint2 eq[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) eq[q] = eqw[(PT_COLS - 1 - c) % PT_EQ_AHEAD][q];
        if (c - PT_EQ_AHEAD >= 0) {
            const uint32_t ad = eq_addr(c - PT_EQ_AHEAD);
#pragma unroll
            for (int q = 0; q < NW; q++) eqw[(PT_COLS - 1 - c) % PT_EQ_AHEAD][q] = lds_read64(ad + 8u * q);
        }
        const LaneColumn<NW> col = sweep_column<NW>(st, eq);
        if (STORE) {
#pragma unroll
            for (int r = 0; r < 2; r++) {
                table_words<NW>(st, col, r, stop[r], tab[c][0][r], tab[c][1][r]);
            }
        }
    }
}

}  // namespace

// Workgroups are four independent wavefronts (as genasm_lane_kernel); two workgroups per CU: a part's 128 table registers
// leave room for two wavefronts per SIMD.  OUT: LaneOutput (genasm_kernels.h).
template <int NW, int OUT>
__global__ __launch_bounds__(256, 2) void genasm_lane_parts_kernel(AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    char* const lds_b = reinterpret_cast<char*>(lds);
    uint8_t* const lds8 = reinterpret_cast<uint8_t*>(lds);
    constexpr uint32_t SLOT = NW == 2 ? 16u : 32u;                 // bytes of one base's Eq words (NW = 3: padded to 32)
    constexpr uint32_t EQ_BYTES = 4u * SLOT, NOMATCH_BYTES = SLOT, TEXT_BYTES = 16u * NW;     // per lane
    constexpr bool EDITS = OUT == LANE_OUT_EDITS, NONE = OUT == LANE_OUT_NONE;
    constexpr uint32_t STAGE_BYTES = NONE ? 0u : PT_RING_BYTES + PT_SCRATCH_BYTES;      // (NONE: no ring, no insertion-run lengths)
    constexpr uint32_t WAVE_LDS = 64u * (STAGE_BYTES + EQ_BYTES + NOMATCH_BYTES + TEXT_BYTES);
    constexpr uint32_t CP_DWORDS = 4u * NW;                        // a checkpoint: Pv and Mv, 2 NW dwords each

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_b = (threadIdx.x >> 6) * WAVE_LDS;
    const uint32_t ring_b = wave_b + lane * PT_RING_BYTES;
    const uint32_t scr_b = wave_b + 64u * PT_RING_BYTES + lane * PT_SCRATCH_BYTES;
    // (LDS ADDRESSES; the Eq tables start at a multiple of 4 SLOT: nothing static precedes the dynamic LDS, and the ring
    // and scratch areas of a wavefront are 64 x 88 bytes = a multiple of 128, as is a wavefront's whole share)
    const uint32_t eq_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds_b + wave_b + 64u * STAGE_BYTES;
    const uint32_t eq_b = eq_base + lane * EQ_BYTES;
    const uint32_t nomatch_b = eq_base + 64u * EQ_BYTES + lane * NOMATCH_BYTES;
    const uint32_t text_b = eq_base + 64u * (EQ_BYTES + NOMATCH_BYTES) + lane * TEXT_BYTES;       // xe / xo of dword d at text_b + 8 d
    const uint32_t swz = NW == 2 ? (lane >> 2) & 3u : (lane >> 1) & 3u;     // lanes that share LDS banks use different slots for the same base
    const uint32_t W = (uint32_t)a.W;
    const uint32_t TBL = (uint32_t)a.tb_limit;                     // W - O: 64..127, or 1..63 with W > 128
    const uint32_t P = (TBL + (uint32_t)PT_COLS - 1u) / (uint32_t)PT_COLS;     // parts, 1..8
    const int32_t ktop = (int32_t)((W + (uint32_t)PT_COLS - 1u) / (uint32_t)PT_COLS) - 1;      // the first chunk of the sweep
    // my wavefront's checkpoints: dword d of checkpoint k at ((k * CP_DWORDS + d) * 64 + lane)
    uint32_t* const cps = a.spill + ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 8u * CP_DWORDS * 64u + lane;

    bool rev = false;                  // my pair's strand (lane_multiword.h)
    bool trev = false;                 // my pair's text is the reverse complement of its stretch (lane_multiword.h)
    LaneWork lp;                       // my pair (lane_multiword.h)
    const LaneLds ll = {lds, ring_b, scr_b};
    uint32_t st_rounds = 0;

    // write out every piece that consists of finished runs only (the run at index nr may still grow)
    auto flush_pieces = [&]() {
        if constexpr (!NONE) for (;;) {
            const bool need = lp.has_pair && (EDITS ? lp.pos - lp.flushed >= 32u : lp.nr - (int32_t)lp.flushed >= 16);
            if (!wave_any(need)) break;
            if (need) write_piece<EDITS>(a, lds, ring_b, lp.cigar_off, lp.cigar_cap, lp.flushed);
        }
    };

    auto save_checkpoint = [&](uint32_t k, const LaneVec<NW>& st) {
        uint32_t* const dst = cps + (uint64_t)k * CP_DWORDS * 64u;
#pragma unroll
        for (int q = 0; q < NW; q++) {
            dst[(4 * q + 0) * 64] = st.pv[q].x;
            dst[(4 * q + 1) * 64] = st.pv[q].y;
            dst[(4 * q + 2) * 64] = st.mv[q].x;
            dst[(4 * q + 3) * 64] = st.mv[q].y;
        }
    };
    auto load_checkpoint = [&](uint32_t k, LaneVec<NW>& st) {
        const uint32_t* const src = cps + (uint64_t)k * CP_DWORDS * 64u;
#pragma unroll
        for (int q = 0; q < NW; q++) {
            st.pv[q] = make_uint2(src[(4 * q + 0) * 64], src[(4 * q + 1) * 64]);
            st.mv[q] = make_uint2(src[(4 * q + 2) * 64], src[(4 * q + 3) * 64]);
        }
    };

    uint32_t rot = hw_wave_slot();     // priority rotation (lane_common.h): one step per round
    for (;;) {
        if (!SCRG_SW(a, 1)) rotate_priority(rot++);
        if (!next_pairs<OUT>(a, lds, ring_b, lane, lp, rev, trev)) break;
        const bool has_pair = lp.has_pair;

        // ---------------- window setup ----------------
        const LaneWindow ext = window_extent(lp, W, TBL);
        const uint32_t n = ext.n, jlim = ext.jlim;
        uint2 stop[2];                                                        // the stop row (bit 63 - jlim % 64 of word jlim / 64)
        {
            const uint64_t sb = 0x8000000000000000ull >> (jlim & 63u);
            const uint64_t s0 = jlim < 64u ? sb : 0ull, s1 = jlim < 64u ? 0ull : sb;
            stop[0] = make_uint2((uint32_t)s0, (uint32_t)(s0 >> 32));
            stop[1] = make_uint2((uint32_t)s1, (uint32_t)(s1 >> 32));
        }
        LaneVec<NW> st;                  // the boundary column: D[n][j] = m-j, every vertical step is +1
        {
            uint32_t tl[2 * NW], th[2 * NW];
            window_setup<NW, SLOT>(a, lp, rev, trev, ext, eq_b, nomatch_b, swz, st, tl, th);
            // the text, slot swizzle folded in, its two planes interleaved (genasm_lane_kernel.hip), to LDS: a chunk reads its 16 columns from there
#pragma unroll
            for (int q = 0; q < 2 * NW; q++) {
                const uint32_t l = tl[q], h = th[q];
                lds_write64(text_b + 8u * q, make_uint2(bitop3<TT_BFI>(l, h << 1, 0x55555555u), bitop3<TT_BFI>(h, l >> 1, 0xaaaaaaaau)));
            }
        }

        uint64_t tab[PT_COLS][2][2];
        // one chunk of the sweep: the variant by what the wavefront's lanes need (uniform)
        auto sweep_chunk = [&](int32_t k, auto store_tag) {
            constexpr bool STORE = decltype(store_tag)::value;
            const int32_t nrel = (int32_t)n - (int32_t)PT_COLS * k;               // columns c < nrel of the chunk are text
            if (!wave_any(has_pair && nrel > 0)) {                                     // past the end of every lane's text: the vectors stay
                if (STORE) {                                                        // (its table: "insertion in every row", what the sweep would give)
                    LaneVec<NW> keep = st;
                    pt_sweep16<NW, true, true>(keep, 0u, 0u, nrel, stop, tab, eq_b, nomatch_b);
                }
                return;
            }
            const uint2 xx = lds_read64(text_b + 8u * (uint32_t)(k >> 1));
            const uint32_t sh = (uint32_t)(k & 1) * 16u;
            const uint32_t xe = xx.x >> sh, xo = xx.y >> sh;
            if (wave_any(has_pair && nrel < PT_COLS)) pt_sweep16<NW, STORE, true>(st, xe, xo, nrel, stop, tab, eq_b, nomatch_b);
            else pt_sweep16<NW, STORE, false>(st, xe, xo, nrel, stop, tab, eq_b, nomatch_b);
        };
        // ---------------- the sweep over all the columns: checkpoints, and the table of part 0 ----------------
#pragma unroll 1
        for (int32_t k = ktop; k >= 1; k--) {
            if ((uint32_t)k < P) save_checkpoint((uint32_t)k, st);                  // the vectors in front of chunk k
            sweep_chunk(k, std::false_type{});
        }
        sweep_chunk(0, std::true_type{});
        // the next part's checkpoint is asked for as soon as the vectors are free, so that the walk hides the round trip — where
        // the registers allow: with four-word vectors the 16 dwords in flight across the walk would spill (20-26 registers)
        constexpr bool PREFETCH = NW <= 3;
        if (PREFETCH && P > 1u) load_checkpoint(1u, st);

        // ---------------- the parts: (table,) walk, runs ----------------
        uint32_t j = 0;                                    // pattern row of the walk
        uint32_t last_dx = 0;                              // (part_events)
        bool alive = has_pair;                             // still walking after the previous part
#pragma unroll 1
        for (uint32_t part = 0; part < P; part++) {
            const uint32_t ncols = min((uint32_t)PT_COLS, TBL - (uint32_t)PT_COLS * part);
            if (part != 0u) {
                if (!wave_any(alive)) break;
                if (!PREFETCH) load_checkpoint(part, st);
                sweep_chunk((int32_t)part, std::true_type{});           // (st: the checkpoint in front of this chunk)
                if (PREFETCH && part + 1u < P) load_checkpoint(part + 1u, st);
            }
            // pass 1 (see genasm_lane_kernel): the walk through this part's columns.  A table row is 128 bits (rows 0..63 in word 0,
            // 64..127 in word 1), and reading it at an arbitrary row costs a funnel of two 64-bit shifts and two selects per word:
            // ~45 instructions per column.  But the walk of part k is near row 16 k in EVERY lane, so most parts stay inside one
            // word for the whole wavefront: then a row access is ONE 64-bit shift (~16 instructions per column).
            //   MODE 1: every lane that holds a pair starts the part at a row <= 40 — walk on word 0 alone.  Rows past 63 then read
            //           as "insertion", so a lane that really leaves the word ends the part at a row > 63: the part is walked
            //           again on the full rows (rare: more than 7 insertions in 16 columns).
            //   MODE 2: every lane that holds a pair is at a row >= 64 (it can only go up) — walk on word 1 alone.
            //   MODE 0: the full 128-bit rows.
            const uint32_t j0 = j;
            uint32_t nDm = 0, Xm = 0, nIm = 0;
            const uint64_t stop0 = ((uint64_t)stop[0].y << 32) | stop[0].x, stop1 = ((uint64_t)stop[1].y << 32) | stop[1].x;
            auto walk_part = [&](auto mode_tag) {
                constexpr int MODE = decltype(mode_tag)::value;
                nDm = Xm = nIm = 0;
                j = j0;
                if constexpr (MODE == 0) {
#pragma unroll
                    for (int s = 0; s < PT_COLS; s++) {
                        if ((uint32_t)s >= ncols) continue;                 // (uniform)
                        // not (insertion), or the stop row, from row j on: the run of insertions is its leading zeros (the stop bit ends it)
                        const uint64_t x0 = tab[s][0][0] | ~tab[s][1][0] | stop0, x1 = tab[s][0][1] | ~tab[s][1][1] | stop1;
                        const uint64_t top = pt_from_row(x0, x1, j);
                        const uint64_t nxt = j < 64u ? shl64(x1, j) : 0ull;      // the 64 rows after those (only if the run is that long)
                        const uint32_t ni = (top != 0ull) ? clz64(top) : 64u + clz64(nxt);
                        if constexpr (!NONE) lds8[scr_b + s] = (uint8_t)ni;
                        nIm = __builtin_amdgcn_alignbit(nIm, (uint32_t)(top >> 32), 31);
                        j += ni;
                        const uint32_t nt1 = (uint32_t)(pt_from_row(tab[s][0][0], tab[s][0][1], j) >> 32);     // sign: not a deletion
                        const uint32_t t0 = (uint32_t)(pt_from_row(tab[s][1][0], tab[s][1][1], j) >> 32);      // sign: substitution
                        nDm = __builtin_amdgcn_alignbit(nDm, nt1, 31);
                        Xm = __builtin_amdgcn_alignbit(Xm, t0, 31);
                        j -= neg_mask(nt1);                                 // j += sign bit of nt1: a deletion (or the stop row) keeps j
                    }
                } else {
                    constexpr int WD = MODE - 1;                            // the word the whole wavefront stays in
                    const uint64_t stopw = WD == 0 ? stop0 : stop1;
                    uint32_t jr = j - 64u * (uint32_t)WD;                   // row inside that word
#pragma unroll
                    for (int s = 0; s < PT_COLS; s++) {
                        if ((uint32_t)s >= ncols) continue;                 // (uniform)
                        const uint64_t x = tab[s][0][WD] | ~tab[s][1][WD] | stopw;
                        const uint64_t top = shl64(x, jr);               // (rows past the word: zeros = "insertion": see MODE 1 above)
                        // leading zeros, 64 for 0: the run of insertions
                        const uint32_t ni = min(ffbh_u32((uint32_t)(top >> 32)), min(ffbh_u32((uint32_t)top), 32u) + 32u);
                        if constexpr (!NONE) lds8[scr_b + s] = (uint8_t)ni;
                        nIm = __builtin_amdgcn_alignbit(nIm, (uint32_t)(top >> 32), 31);
                        jr += ni;
                        const uint32_t nt1 = (uint32_t)(shl64(tab[s][0][WD], jr) >> 32);      // sign: not a deletion
                        const uint32_t t0 = (uint32_t)(shl64(tab[s][1][WD], jr) >> 32);       // sign: substitution
                        nDm = __builtin_amdgcn_alignbit(nDm, nt1, 31);
                        Xm = __builtin_amdgcn_alignbit(Xm, t0, 31);
                        jr -= neg_mask(nt1);
                    }
                    j = jr + 64u * (uint32_t)WD;
                }
            };
            if (TBL <= 63u) {                                   // (W > 128 with a small W-O: no walk ever reaches row 64 — jlim <= W-O)
                walk_part(std::integral_constant<int, 1>{});
            } else if (!wave_any(has_pair && j0 < 64u)) {
                walk_part(std::integral_constant<int, 2>{});
            } else if (!wave_any(has_pair && j0 > 40u)) {
                walk_part(std::integral_constant<int, 1>{});
                if (wave_any(has_pair && j > 63u)) walk_part(std::integral_constant<int, 0>{});       // some lane left word 0: once more, on the full rows
            } else {
                walk_part(std::integral_constant<int, 0>{});
            }
            // pass 2 (lane_multiword.h).  A run that crosses from one part into the next is one run: see part_runs.
            // (live: a lane without a pair — the one-word walks read it garbage)
            const PartEvents ev = part_events<PT_COLS>(lp, has_pair, part == 0u, ncols, nDm, Xm, nIm, j - j0, last_dx, alive);
            // between two checks of the ring, EDITS: <= 4 x 5 new bytes + 4 speculative ones: the 64-byte ring cannot wrap;
            // runs: <= 12 new runs + 1 speculative slot: the 32-run ring cannot wrap
            if constexpr (EDITS) part_edits<PT_COLS, true, 2>(a, ll, ev, lp, flush_pieces);
            else if constexpr (!NONE) part_runs<PT_COLS, 3>(ll, ev, lp, flush_pieces);
            else (void)ev;
        }
        lp.read_idx += j;
        if constexpr (EDITS) {
            window_end_bytes<true>(ll, lp);
            flush_pieces();
        }
        st_rounds++;
    }
    if (SCRG_TIMING(a) && lane == 0) atomicAdd((unsigned long long*)&a.stats[0], (unsigned long long)st_rounds);
}

template <int NW> static void launch_parts(const AlignArgs& a, dim3 g, dim3 b, size_t lds, hipStream_t s, LaneOutput out)
{
    with_lane_output(out, [&](auto o) { hipLaunchKernelGGL((genasm_lane_parts_kernel<NW, decltype(o)::value>), g, b, lds, s, a); });
}

hipError_t launch_align_lane_parts(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out)
{
    // grid counts wavefronts, lds_bytes is per wavefront
    const dim3 g((grid + 3) / 4), b(256);
    const int nw = (a.W + 63) / 64;
    if (nw == 2) launch_parts<2>(a, g, b, 4 * lds_bytes, s, out);
    else if (nw == 3) launch_parts<3>(a, g, b, 4 * lds_bytes, s, out);
    else if (nw == 4) launch_parts<4>(a, g, b, 4 * lds_bytes, s, out);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace scrg
