// genasm_lane_wide_kernel.hip — the lane-per-pair aligner for 32 <= W-O <= 63 and W <= 128: the formulation of
// genasm_lane_kernel.hip (every lane aligns its own pair; the window's table holds the differences of the
// edit-distance matrix behind the GenASM bitvectors, src/genasm_cpu.cpp:210-409 — see the header of that file for why
// this gives the reference's edit distance and CIGAR bit for bit), for windows whose traceback may consume up to 63
// characters: a table row is one 64-bit word (rows 0 .. W-O <= 63; for W > 64 that is word 0 of the two-word vectors,
// src/bitvector.hpp:45-48), and W-O columns of two such rows are 4 (W-O) dwords — twice the registers of a wavefront.
//
// The table is therefore built in TWO HALVES of 32 columns, both held in the same 128 registers: the sweep over the
// text columns runs from the last column down (the recurrence only goes that way) and keeps columns 0..31, the walk
// consumes them, then the sweep is REPEATED from the top down to column 32, keeping columns 32..W-O-1, and the walk
// goes on from where it stood.  Recomputing 32 columns of difference vectors (21 instructions each for one word)
// replaces 2 x 16 bytes per lane and column of table traffic through HBM (genasm_lane_mw_kernel.hip, which this kernel
// replaces for these W/O: 3 TB/s at the reference's W=64/O=2 sweep point) and there is no data-dependent slow path.
// For W > 64 the columns 127..64 are common to both sweeps: their result (Pv, Mv: 8 dwords) is kept and both halves
// start from it.
//
// Shared with genasm_lane_parts_kernel.hip, in lane_multiword.h: the pair state and claim loop, the window set-up, one column
// of the recurrence, and the second pass.  Here: the two halves, and the prologue sweep for W > 64.
//
// Each half ends with its own second pass (masks -> runs or edit-stream bytes: part_events, part_runs / part_edits; with
// LANE_OUT_NONE part_events alone: the half's edits and text columns).
// A run that crosses from column 31 to column 32 is ONE run of the window (the reference merges within a window,
// src/genasm_cpu.cpp:372-404, and starts a new run at every window): the second half does not force a run start at its
// first column when the step there continues the first half's last run, and adds its length to that run, which is
// still in the staging ring (the last committed run never leaves before the next one is committed).
//
// tests/proto/lane_proto.c (lane_align_codes_mw, RW = 1) restates the arithmetic; tests/test_gpu_parity.py holds the
// kernel against the CPU checker and the reference-built fixtures at W/O = 64/2, 64/16, 64/32, 128/65, 96/49, ...

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_multiword.h"

namespace scrg {

namespace {

#ifndef WD_BLOCKS_PER_CU
#define WD_BLOCKS_PER_CU 2
#endif
constexpr int WD_HALF = 32;                      // columns per half
constexpr uint32_t WD_RING_BYTES = 68;           // 32 runs + one dword: lanes land on distinct LDS banks
constexpr uint32_t WD_SCRATCH_BYTES = 36;        // insertion-run length of each column of a half, one byte each (+ bank skew)
constexpr int WD_EQ_AHEAD = 8;                   // Eq words are read from LDS this many columns ahead of their use

// Per-lane constants of a window's sweeps.
template <int NW> struct WdWindow {
    uint32_t tl[2 * NW], th[2 * NW];     // text planes (swizzled for the Eq slots): dword d holds columns 32 d .. 32 d + 31
    uint32_t n;                          // text columns of the window
    uint2 stop;                          // the stop row (bit 63 - jlim), as two dwords
};

// Columns HI .. LO (descending) of the window's table; the columns >= STORE (at most 32 of them: STORE .. STORE + 31)
// go to tab[column - STORE] as {~(V1 | stop), V0 | stop}; STORE < 0: nothing is kept.
// SHORT_N as in genasm_lane_kernel: columns >= n read the Eq word "no character matches".
// SHORT_N: 0 every lane has its text column; 1 columns >= n read "no character matches", selected by compare + v_cndmask; 2 the same
// selected by arithmetic (subtract, smear the sign, v_bitop3: 5 counted cycles per column instead of 15 — a v_cndmask on VCC issues at
// a seventh of the rate, profiles/r03_valu_issue_rates.txt — but the compiler keeps the masks: 248 registers for one-word vectors;
// the edit-stream variant and two-word vectors, which have none to spare, would spill and take form 1)
template <int NW, int SHORT_N, int HI, int LO, int STORE>
__device__ __forceinline__ void wd_sweep(LaneVec<NW>& st, const WdWindow<NW>& w, uint64_t (&tab)[WD_HALF][2],
                                         const uint32_t eq_b, const uint32_t nomatch_b)
{
    // (the planes pass through an opaque copy: the address arithmetic of the 64 columns must not be shared between the
    // sweeps of a window — kept alive across the walk it would take 64 registers)
    uint32_t wtl[2 * NW], wth[2 * NW];
#pragma unroll
    for (int q = 0; q < 2 * NW; q++) {
        wtl[q] = w.tl[q];
        wth[q] = w.th[q];
        asm volatile("" : "+v"(wtl[q]), "+v"(wth[q]));
    }
    // the two planes interleaved (genasm_lane_kernel.hip): xe: bits b, b + 1 = lo, hi bit of every EVEN column b of the dword; xo:
    // bits b - 1, b of every ODD column b — a column's address is then one shift and one v_bitop3 (2 instructions instead of 4)
    uint32_t xe[2 * NW], xo[2 * NW];
#pragma unroll
    for (int q = 0; q < 2 * NW; q++) {
        if (32 * q > HI || 32 * q + 31 < LO) continue;
        xe[q] = bitop3<TT_BFI>(wtl[q], wth[q] << 1, 0x55555555u);
        xo[q] = bitop3<TT_BFI>(wth[q], wtl[q] >> 1, 0xaaaaaaaau);
    }
    auto eq_addr = [&](int i) -> uint32_t {
        constexpr int SH = NW == 1 ? 3 : 4;                                  // a base's NW words: 8 or 16 bytes
        const int b = i & 31;
        const uint32_t x = (b & 1) ? xo[i >> 5] : xe[i >> 5];
        const int f = (b & 1) ? b - 1 : b;                                  // the field's low bit; it goes to bit SH
        const uint32_t u = f >= SH ? x >> (f - SH) : x << (SH - f);
        const uint32_t a = bitop3<TT_ANDOR>(u, 3u << SH, eq_b);
        if (SHORT_N == 0) return a;
        if (SHORT_N == 2) return bitop3<TT_BFI>(a, nomatch_b, neg_mask((uint32_t)i - w.n));
        return (uint32_t)i < w.n ? a : nomatch_b;
    };
    uint2 eqw[WD_EQ_AHEAD][NW];
#pragma unroll
    for (int k = 0; k < WD_EQ_AHEAD; k++) {
        if (HI - k < LO) continue;
        const uint32_t ad = eq_addr(HI - k);
#pragma unroll
        for (int q = 0; q < NW; q++) eqw[k][q] = lds_read64(ad + 8u * q);
    }
#pragma unroll
    for (int i = HI; i >= LO; i--) {
        uint2 eq[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) eq[q] = eqw[(HI - i) % WD_EQ_AHEAD][q];
        if (i - WD_EQ_AHEAD >= LO) {
            const uint32_t ad = eq_addr(i - WD_EQ_AHEAD);
#pragma unroll
            for (int q = 0; q < NW; q++) eqw[(HI - i) % WD_EQ_AHEAD][q] = lds_read64(ad + 8u * q);
        }
        const LaneColumn<NW> col = sweep_column<NW>(st, eq);
        if (STORE >= 0 && i >= STORE && i < STORE + WD_HALF) {
            table_words<NW>(st, col, 0, w.stop, tab[i - STORE][0], tab[i - STORE][1]);
        }
    }
}

}  // namespace

// Workgroups are four independent wavefronts (as genasm_lane_kernel); two workgroups per CU: the table's 128 registers
// leave room for two wavefronts per SIMD.  OUT: LaneOutput (genasm_kernels.h).
template <int NW, int OUT>
__global__ __launch_bounds__(256, WD_BLOCKS_PER_CU) void genasm_lane_wide_kernel(AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    char* const lds_b = reinterpret_cast<char*>(lds);
    uint8_t* const lds8 = reinterpret_cast<uint8_t*>(lds);
    constexpr bool EDITS = OUT == LANE_OUT_EDITS, NONE = OUT == LANE_OUT_NONE;
    constexpr uint32_t EQ_BYTES = 32u * NW, NOMATCH_BYTES = 8u * NW;
    constexpr uint32_t STAGE_BYTES = NONE ? 0u : WD_RING_BYTES + WD_SCRATCH_BYTES;      // (NONE: no ring, no insertion-run lengths)
    constexpr uint32_t WAVE_LDS = 64u * (STAGE_BYTES + EQ_BYTES + NOMATCH_BYTES);

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_b = (threadIdx.x >> 6) * WAVE_LDS;
    const uint32_t ring_b = wave_b + lane * WD_RING_BYTES;
    const uint32_t scr_b = wave_b + 64u * WD_RING_BYTES + lane * WD_SCRATCH_BYTES;
    // (LDS ADDRESSES, multiples of 8 NW: nothing static precedes the dynamic LDS)
    const uint32_t eq_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds_b + wave_b + 64u * STAGE_BYTES;
    const uint32_t eq_b = eq_base + lane * EQ_BYTES;
    const uint32_t nomatch_b = eq_base + 64u * EQ_BYTES + lane * NOMATCH_BYTES;
    const uint32_t swz = NW == 1 ? (lane >> 3) & 3u : (lane >> 2) & 3u;     // lanes that share LDS banks use different slots for the same base
    const uint32_t W = (uint32_t)a.W;
    const uint32_t TBL = (uint32_t)a.tb_limit;         // W - O, 32..63
    const uint32_t HB = TBL - (uint32_t)WD_HALF;       // columns of the second half, 0..31

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

    uint32_t rot = hw_wave_slot();     // priority rotation (lane_common.h): one step per round
    for (;;) {
        if (!SCRG_SW(a, 1)) rotate_priority(rot++);
        if (!next_pairs<OUT>(a, lds, ring_b, lane, lp, rev, trev)) break;
        const bool has_pair = lp.has_pair;

        // ---------------- window setup ----------------
        const LaneWindow ext = window_extent(lp, W, TBL);
        const uint32_t n = ext.n;
        const uint64_t stop64 = 0x8000000000000000ull >> ext.jlim;
        WdWindow<NW> win;
        win.n = n;
        win.stop = make_uint2((uint32_t)stop64, (uint32_t)(stop64 >> 32));
        LaneVec<NW> st0;                 // the vectors in front of column 63: the boundary column (W <= 64) or the result of columns 127..64
        window_setup<NW, 8u * NW>(a, lp, rev, trev, ext, eq_b, nomatch_b, swz, st0, win.tl, win.th);
        // short_n: some lane's text ends inside the columns 0..63; short_pro (W > 64): ... inside the columns 64 .. the
        // first column of the prologue sweep
        const bool short_n = wave_any(has_pair && n < 64u);
        const bool short_pro = NW == 2 && wave_any(has_pair && n != ((W + 15u) & ~15u));
        uint64_t tab[WD_HALF][2];
        if constexpr (NW == 2) {
            // columns 64 .. W-1, common to both halves.  (A column past the end of the text leaves the boundary vectors as
            // they are — Eq = "no match" gives Xh = ~valid, Ph = Mh = 0 — so the sweep starts at the first column a
            // window of W characters can have, rounded up to 16.)
            if (W <= 80u) {
                if (short_pro) wd_sweep<NW, ((EDITS || NW == 2) ? 1 : 2), 79, 64, -1>(st0, win, tab, eq_b, nomatch_b);
                else wd_sweep<NW, 0, 79, 64, -1>(st0, win, tab, eq_b, nomatch_b);
            } else if (W <= 96u) {
                if (short_pro) wd_sweep<NW, ((EDITS || NW == 2) ? 1 : 2), 95, 64, -1>(st0, win, tab, eq_b, nomatch_b);
                else wd_sweep<NW, 0, 95, 64, -1>(st0, win, tab, eq_b, nomatch_b);
            } else if (W <= 112u) {
                if (short_pro) wd_sweep<NW, ((EDITS || NW == 2) ? 1 : 2), 111, 64, -1>(st0, win, tab, eq_b, nomatch_b);
                else wd_sweep<NW, 0, 111, 64, -1>(st0, win, tab, eq_b, nomatch_b);
            } else {
                if (short_pro) wd_sweep<NW, ((EDITS || NW == 2) ? 1 : 2), 127, 64, -1>(st0, win, tab, eq_b, nomatch_b);
                else wd_sweep<NW, 0, 127, 64, -1>(st0, win, tab, eq_b, nomatch_b);
            }
        }

        // ---------------- the two halves: table, walk, runs ----------------
        uint32_t j = 0;                                    // pattern row of the walk
        uint32_t last_dx = 0;                              // (part_events)
        bool alive = has_pair;                             // still walking after the first half
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            const uint32_t ncols = half == 0 ? (uint32_t)WD_HALF : HB;
            if (half == 1 && (HB == 0u || !wave_any(alive))) break;
            {
                LaneVec<NW> st = st0;
                if (half == 0) {
                    if (short_n) wd_sweep<NW, ((EDITS || NW == 2) ? 1 : 2), 63, 0, 0>(st, win, tab, eq_b, nomatch_b);
                    else wd_sweep<NW, 0, 63, 0, 0>(st, win, tab, eq_b, nomatch_b);
                } else {
                    if (short_n) wd_sweep<NW, ((EDITS || NW == 2) ? 1 : 2), 63, WD_HALF, WD_HALF>(st, win, tab, eq_b, nomatch_b);
                    else wd_sweep<NW, 0, 63, WD_HALF, WD_HALF>(st, win, tab, eq_b, nomatch_b);
                }
            }
            // pass 1 (see genasm_lane_kernel): the walk through this half's columns, on 64-bit rows
            const uint32_t j0 = j;
            uint32_t nDm = 0, Xm = 0, nIm = 0;
#pragma unroll
            for (int s = 0; s < WD_HALF; s++) {
                if ((uint32_t)s >= ncols) continue;                 // (uniform)
                const uint32_t xl = bitop3<TT_NIV>((uint32_t)tab[s][0], (uint32_t)tab[s][1], win.stop.x);
                const uint32_t xu = bitop3<TT_NIV>((uint32_t)(tab[s][0] >> 32), (uint32_t)(tab[s][1] >> 32), win.stop.y);
                const uint64_t x = shl64(((uint64_t)xu << 32) | xl, j);      // not (insertion), or the stop row, from row j on
                const uint32_t ni = min(ffbh_u32((uint32_t)(x >> 32)), ffbh_u32((uint32_t)x) + 32u);     // (the stop bit makes x non-zero)
                if constexpr (!NONE) lds8[scr_b + s] = (uint8_t)ni;
                nIm = __builtin_amdgcn_alignbit(nIm, (uint32_t)(x >> 32), 31);
                j += ni;
                const uint32_t nt1 = (uint32_t)(shl64(tab[s][0], j) >> 32);     // sign: not a deletion
                const uint32_t t0 = (uint32_t)(shl64(tab[s][1], j) >> 32);      // sign: substitution
                nDm = __builtin_amdgcn_alignbit(nDm, nt1, 31);
                Xm = __builtin_amdgcn_alignbit(Xm, t0, 31);
                j -= neg_mask(nt1);                                 // j += sign bit of nt1: a deletion (or the stop row) keeps j
            }
            // pass 2 (lane_multiword.h).  A run that crosses from column 31 to column 32 is one run: see part_runs.
            const PartEvents ev = part_events<WD_HALF>(lp, true, half == 0, ncols, nDm, Xm, nIm, j - j0, last_dx, alive);
            // between two checks of the ring, EDITS: <= 4 x 4 new bytes + 3 speculative ones (+ 2 of a window end): the 64-byte
            // ring cannot wrap; runs: <= 12 new runs + 1 speculative slot: the 32-run ring cannot wrap
            if constexpr (EDITS) part_edits<WD_HALF, false, 2>(a, ll, ev, lp, flush_pieces);
            else if constexpr (!NONE) part_runs<WD_HALF, 3>(ll, ev, lp, flush_pieces);
            else (void)ev;
        }
        lp.read_idx += j;
        if constexpr (EDITS) {
            window_end_bytes<false>(ll, lp);
            flush_pieces();
        }
        st_rounds++;
    }
    if (SCRG_TIMING(a) && lane == 0) atomicAdd((unsigned long long*)&a.stats[0], (unsigned long long)st_rounds);
}

hipError_t launch_align_lane_wide(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out)
{
    // grid counts wavefronts, lds_bytes is per wavefront
    const dim3 g((grid + 3) / 4), b(256);
    if (a.W <= 64) with_lane_output(out, [&](auto o) { hipLaunchKernelGGL((genasm_lane_wide_kernel<1, decltype(o)::value>), g, b, 4 * lds_bytes, s, a); });
    else with_lane_output(out, [&](auto o) { hipLaunchKernelGGL((genasm_lane_wide_kernel<2, decltype(o)::value>), g, b, 4 * lds_bytes, s, a); });
    return hipGetLastError();
}

}  // namespace scrg
