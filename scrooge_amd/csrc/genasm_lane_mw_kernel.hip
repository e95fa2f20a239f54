// genasm_lane_mw_kernel.hip — the lane-per-pair aligner for W > 64 (64 < W <= 256): the formulation of
// genasm_lane_kernel.hip — every lane aligns its own pair, the window's table holds the DIFFERENCES of the
// edit-distance matrix behind the GenASM bitvectors (see the header of that file for why this gives the reference's
// edit distance and CIGAR bit for bit, src/genasm_cpu.cpp:210-409; multi-word entries: src/bitvector.hpp:45-48) — with
// multi-word vectors: a pattern vector has NW = ceil(W/64) words (word 0 the most significant: bit 63-k of word w
// belongs to pattern character 64 w + k), and as the traceback only looks at rows j <= W-O, a table row keeps the
// top RW = (W-O)/64 + 1 words.  One text column — all W pattern rows, every distance at once — is ~10 NW 64-bit
// operations, there is no loop over the distance, and a window's cost does not depend on its distance; the GenASM-row
// kernel this replaces as the default for W > 64 (genasm_kernel_multiword.hip) sweeps W+1 distance rows.
//
// The table (two RW-word rows for each of the W-O columns: 1 to 16 KB per lane) lives in HBM, one slab per wavefront,
// word-interleaved over the lanes so that a store or load of the wavefront is 512 contiguous bytes; the first
// traceback pass reads it back four to sixteen columns at a time.  LDS holds the CIGAR staging ring and the insertion-run
// lengths only.  Written with plain 64-bit operations (this is the knob-sweep configuration, scripts/profile.py:180-185,
// not the tuned one); tests/proto/lane_proto.c (lane_align_codes_mw) restates the arithmetic and is checked against
// the reference algorithm on the CPU (tests/test_lane_proto.py).
// The pair state and the retire / claim loop are the ones of the wide and parts kernels (lane_multiword.h); the passes here
// work on Row<RW> rows (row_ops.h) and are this kernel's own.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_multiword.h"
#include "row_ops.h"

namespace scrg {

namespace {

constexpr uint32_t MW_RING_BYTES = 68;             // 32 runs + one dword per lane (bank skew)

}  // namespace

// EDITS = true (scrg_align_device_edits): the alignment leaves as an edit stream (edit_stream.h: one byte per edit
// carrying the number of matches before it) instead of runs; see genasm_lane_kernel<true>.
// OUT: LaneOutput (genasm_kernels.h).  LANE_OUT_NONE: the table and the first pass alone — no LDS at all.
template <int NW, int RW, int OUT>
__global__ __launch_bounds__(64) void genasm_lane_mw_kernel(AlignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    char* const lds_b = reinterpret_cast<char*>(lds);
    uint8_t* const lds8 = reinterpret_cast<uint8_t*>(lds);

    constexpr bool EDITS = OUT == LANE_OUT_EDITS, NONE = OUT == LANE_OUT_NONE;
    const uint32_t lane = threadIdx.x;
    const uint32_t W = (uint32_t)a.W;
    const uint32_t TBL = (uint32_t)a.tb_limit;         // W - O: 64 (RW - 1) <= TBL < 64 RW
    const uint32_t ring_b = lane * MW_RING_BYTES;
    const uint32_t len_b = 64u * MW_RING_BYTES + lane * lane_mw_len_bytes(a.tb_limit);
    // my wavefront's slab of the table: word ((column * 2 + which) * RW + r) * 64 + lane
    uint64_t* const tab = reinterpret_cast<uint64_t*>(a.spill) + (uint64_t)blockIdx.x * (uint64_t)TBL * 2u * RW * 64u + lane;

    bool rev = false;                  // my pair's strand (lane_multiword.h)
    bool trev = false;                 // my pair's text is the reverse complement of its stretch (lane_multiword.h)
    LaneWork lp;                       // my pair, and below the round's retire / claim loop (lane_multiword.h)

    auto write_piece = [&]() {
        if constexpr (!NONE) scrg::write_piece<EDITS>(a, lds, ring_b, lp.cigar_off, lp.cigar_cap, lp.flushed);
    };
    auto flush_pieces = [&]() {
        for (;;) {
            const bool need = lp.has_pair && lp.nr + 1 - (int32_t)lp.flushed >= 16;
            if (!wave_any(need)) break;
            if (need) write_piece();
        }
    };
    auto push_run = [&](uint32_t op, uint32_t count) {
        lp.nr++;
        *reinterpret_cast<uint16_t*>(lds_b + ring_b + (((uint32_t)lp.nr & 31u) << 1)) = (uint16_t)(count | (op << 8));
    };
    auto emit = [&](uint32_t b) {          // EDITS: one byte of the stream; whole pieces leave at once
        lds8[ring_b + (lp.pos & 63u)] = (uint8_t)b;
        lp.pos++;
        if (lp.pos - lp.flushed >= 32u) write_piece();
    };

    for (;;) {
        // (EDITS: emit writes every whole piece at once, so fewer than 32 bytes are staged: retire_pair needs no loop for them)
        if (!next_pairs<OUT, !EDITS>(a, lds, ring_b, lane, lp, rev, trev)) break;

        // ---------------- window setup (genasm_cpu.cpp:417-420) ----------------
        const uint32_t n = (lp.has_pair && lp.ref_idx < lp.text_len) ? min(W, lp.text_len - lp.ref_idx) : 0u;
        const uint32_t m = lp.has_pair ? min(W, lp.read_len - lp.read_idx) : 1u;      // >= 1 for live pairs
        uint64_t tlo[NW], thi[NW], rlo[NW], rhi[NW], valid[NW];
        const bool wave_trev = a.text_rev && wave_any(lp.has_pair && trev);   // (uniform) texts taken as the reverse complement of their stretch
#pragma unroll
        for (int w = 0; w < NW; w++) {
            Planes t = {0, 0}, p = {0, 0};
            if (lp.has_pair && !trev && 64u * (uint32_t)w < n) t = load_window_strided(a.seq, lp.text_off, lp.ref_idx + 64u * (uint32_t)w, a.text_stride);
            if (wave_trev) {                                  // (a reversed lane loads its words once, here)
                if (lp.has_pair && trev && 64u * (uint32_t)w < n) t = text_revcomp_word(a.seq, lp.text_off, lp.text_len, lp.ref_idx, (uint32_t)w, a.text_stride);
            }
            if (lp.has_pair && 64u * (uint32_t)w < m) p = load_window_strided(a.seq, lp.read_off, lp.read_idx + 64u * (uint32_t)w, a.read_stride);
            tlo[w] = t.lo;
            thi[w] = t.hi;
            rlo[w] = brev64(p.lo);                       // reversed: bit 63-k <-> pattern character 64 w + k
            rhi[w] = brev64(p.hi);
            if (a.stranded && wave_any(lp.has_pair && rev)) {  // (uniform)
                const Planes rv = revcomp_pattern_word(a.seq, lp.read_off, lp.read_len, lp.has_pair ? lp.read_idx : lp.read_len, (uint32_t)w, a.read_stride);
                if (lp.has_pair && rev) { rlo[w] = rv.lo; rhi[w] = rv.hi; }
            }
            const uint32_t lo = 64u * (uint32_t)w;
            valid[w] = m >= lo + 64u ? ~0ull : (m <= lo ? 0ull : ~0ull << (64u - (m - lo)));
        }
        const uint32_t jlim = lp.has_pair ? min(m, TBL) : 0u;          // the walk ends when j gets here (:301, :310)
        const Row<RW> stop = row_bit<RW>(jlim);

        // ---------------- the window's table (genasm_cpu.cpp:210-288 in difference form) ----------------
        // The bits below the pattern are neutral (Eq = 1, Pv = Mv = 0); columns past the end of the text take the Eq
        // word "no character matches", which leaves the boundary column D[n][j] = m-j as it is and yields "insertion
        // in every row".  Column i < W-O keeps ~(V1 | stop) and V0 | stop (V1 = Pv' | Ph, V0 = Pv' | ~(Ph | Xh)).
        {
            uint64_t pv[NW], mv[NW];
#pragma unroll
            for (int w = 0; w < NW; w++) { pv[w] = valid[w]; mv[w] = 0; }
#pragma unroll
            for (int wi = NW - 1; wi >= 0; wi--) {
                for (int b = 63; b >= 0; b--) {
                    const uint32_t i = 64u * (uint32_t)wi + (uint32_t)b;
                    if (i >= W) continue;                             // (uniform)
                    const uint64_t sl = 0ull - ((tlo[wi] >> b) & 1ull), sh = 0ull - ((thi[wi] >> b) & 1ull);
                    const bool in_text = i < n;
                    uint64_t xv[NW], xh[NW], ph[NW], mh[NW];
                    uint64_t carry = 0;
#pragma unroll
                    for (int w = NW - 1; w >= 0; w--) {              // the add: carries run from the last word to word 0
                        const uint64_t eq = (in_text ? ~((rlo[w] ^ sl) | (rhi[w] ^ sh)) : 0ull) | ~valid[w];
                        xv[w] = eq | mv[w];
                        const uint64_t t = eq & pv[w];
                        const uint64_t s1 = t + pv[w];
                        const uint64_t s2 = s1 + carry;
                        carry = (uint64_t)(s1 < t) | (uint64_t)(s2 < s1);
                        xh[w] = (s2 ^ pv[w]) | eq;
                        ph[w] = mv[w] | ~(xh[w] | pv[w]);
                        mh[w] = pv[w] & xh[w];
                    }
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const uint64_t ph1 = (ph[w] << 1) | (w + 1 < NW ? ph[w + 1] >> 63 : 0ull);    // row 0 of the matrix is all
                        const uint64_t mh1 = (mh[w] << 1) | (w + 1 < NW ? mh[w + 1] >> 63 : 0ull);    // zeros: 0 comes in
                        pv[w] = mh1 | ~(xv[w] | ph1);
                        mv[w] = ph1 & xv[w];
                    }
                    if (i < TBL) {
#pragma unroll
                        for (int r = 0; r < RW; r++) {
                            // (O = 0 at W = 64, 128, 256: the stop row W is the first bit of a word the vectors do not have —
                            // RW = NW + 1 — which holds nothing but that bit)
                            const uint64_t pvr = r < NW ? pv[r < NW ? r : 0] : 0ull, phr = r < NW ? ph[r < NW ? r : 0] : 0ull, xhr = r < NW ? xh[r < NW ? r : 0] : ~0ull;
                            tab[((uint64_t)(i * 2u) * RW + r) * 64u] = ~((pvr | phr) | stop.w[r]);
                            tab[((uint64_t)(i * 2u + 1u) * RW + r) * 64u] = (pvr | ~(phr | xhr)) | stop.w[r];
                        }
                    }
                }
            }
        }

        // ---------------- traceback (genasm_cpu.cpp:290-409): the two passes of genasm_lane_kernel on RW-word rows ----------------
        {
            uint32_t j = 0;
            Row<RW> nDm = row_zero<RW>(), Xm = row_zero<RW>(), nIm = row_zero<RW>();
            constexpr int CH = RW == 1 ? 16 : (RW == 2 ? 8 : 4);    // columns in flight: the loads do not depend on the walk
            for (uint32_t i0 = 0; i0 < TBL; i0 += CH) {
                Row<RW> nv1[CH], v0[CH];
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const uint32_t i = min(i0 + (uint32_t)q, TBL - 1u);
#pragma unroll
                    for (int r = 0; r < RW; r++) {
                        nv1[q].w[r] = tab[((uint64_t)(i * 2u) * RW + r) * 64u];
                        v0[q].w[r] = tab[((uint64_t)(i * 2u + 1u) * RW + r) * 64u];
                    }
                }
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const uint32_t i = i0 + (uint32_t)q;
                    if (i >= TBL) continue;                          // (uniform)
                    Row<RW> x;
#pragma unroll
                    for (int r = 0; r < RW; r++) x.w[r] = nv1[q].w[r] | ~v0[q].w[r] | stop.w[r];   // not (insertion), or the stop row
                    x = row_shl<RW>(x, j);
                    const uint32_t ni = row_clz<RW>(x);             // (the stop bit makes x non-zero)
                    if constexpr (!NONE) lds8[len_b + i] = (uint8_t)ni;
                    nIm = row_shl1_in<RW>(nIm, x.w[0] >> 63);
                    j += ni;
                    const Row<RW> nt1 = row_shl<RW>(nv1[q], j), t0 = row_shl<RW>(v0[q], j);    // top bits: not a deletion, substitution
                    nDm = row_shl1_in<RW>(nDm, nt1.w[0] >> 63);
                    Xm = row_shl1_in<RW>(Xm, t0.w[0] >> 63);
                    j += (uint32_t)(nt1.w[0] >> 63);                 // a deletion (or the stop row) keeps j
                }
            }
            // column i -> bit i from the top; a finished lane reads "deletion and substitution" (the stop row)
            const uint32_t nsh = 64u * RW - TBL;
            Row<RW> Draw = row_shl<RW>(nDm, nsh), Im;
            const Row<RW> Xraw = row_shl<RW>(Xm, nsh);
#pragma unroll
            for (int r = 0; r < RW; r++) { Draw.w[r] = ~Draw.w[r]; Im.w[r] = ~nIm.w[r]; }
            Im = row_shl<RW>(Im, nsh);
            const Row<RW> lim = row_bit<RW>(TBL);
            Row<RW> dead;
#pragma unroll
            for (int r = 0; r < RW; r++) dead.w[r] = (Draw.w[r] & Xraw.w[r]) | lim.w[r];
            const uint32_t ti = row_clz<RW>(dead);
            const Row<RW> A = row_top<RW>(ti);
            Row<RW> D, X, B, E;
#pragma unroll
            for (int r = 0; r < RW; r++) { D.w[r] = Draw.w[r] & A.w[r]; X.w[r] = Xraw.w[r] & A.w[r]; }
            const Row<RW> D1 = row_shr1<RW>(D), X1 = row_shr1<RW>(X);
#pragma unroll
            for (int r = 0; r < RW; r++) {
                B.w[r] = ((D.w[r] ^ D1.w[r]) | (X.w[r] ^ X1.w[r]) | Im.w[r] | (r == 0 ? TOP : 0ull)) & A.w[r];
                E.w[r] = B.w[r] | Im.w[r];
            }
            lp.edits += j - ti + 2u * row_pop<RW>(D) + row_pop<RW>(X);
            lp.ref_idx += ti;
            lp.read_idx += j;

            if constexpr (NONE) {
                // (the window's edits and advance are all that is asked for)
            } else if constexpr (EDITS) {
                // the columns that hold an edit: an insertion run (before the column's step), then a deletion or a
                // substitution; mbase + c = matches pending when column c is reached
                Row<RW> Ev;
#pragma unroll
                for (int r = 0; r < RW; r++) Ev.w[r] = D.w[r] | X.w[r] | Im.w[r];
                lp.nr += (int32_t)(row_pop<RW>(B) + row_pop<RW>(Im));       // the runs this window has in the other output format
                while (wave_any(row_any<RW>(Ev))) {
                    if (row_any<RW>(Ev)) {
                        const uint32_t c = row_clz<RW>(Ev);
                        const Row<RW> bit = row_bit<RW>(c);
#pragma unroll
                        for (int r = 0; r < RW; r++) Ev.w[r] &= ~bit.w[r];
                        uint32_t t = lp.mbase + c;
                        if (row_test<RW>(Im, c)) {
                            const uint32_t ni = lds8[len_b + c];
                            for (; t >= 63u; t -= 63u) emit(0x3Fu);          // (edit_stream.h: 63 matches and nothing else)
                            emit(0x80u | t);
                            for (uint32_t q = 1; q < ni; q++) emit(0x80u);
                            t = 0;
                            lp.mbase = 0u - c;
                        }
                        const bool isD = row_test<RW>(D, c), isX = row_test<RW>(X, c);
                        if (isD || isX) {
                            for (; t >= 63u; t -= 63u) emit(0x3Fu);
                            emit((isX ? 0x40u : 0xC0u) | t);
                            lp.mbase = ~c;
                        }
                    }
                }
                // the window ends: the matches since its last edit, then the mark (every window of a pair, the last one too)
                if (wave_any(lp.has_pair)) {
                    if (lp.has_pair) {
                        uint32_t t = lp.mbase + ti;
                        for (; t >= 63u; t -= 63u) emit(0x3Fu);
                        emit(t);
                    }
                }
                lp.mbase = 0;
            } else
            while (wave_any(row_any<RW>(E))) {
                if (row_any<RW>(E)) {
                    const uint32_t c = row_clz<RW>(E);
                    if (row_test<RW>(Im, c)) push_run((uint32_t)'I', lds8[len_b + c]);
                    const Row<RW> bit = row_bit<RW>(c);
#pragma unroll
                    for (int r = 0; r < RW; r++) E.w[r] &= ~bit.w[r];
                    const uint32_t nx = min(row_clz<RW>(E), ti);     // the next event or the end of the walk
                    if (row_test<RW>(B, c))
                        push_run(row_test<RW>(D, c) ? (uint32_t)'D' : (row_test<RW>(X, c) ? (uint32_t)'X' : (uint32_t)'='), nx - c);
                }
                flush_pieces();                                         // at most two new runs per iteration
            }
        }
    }
}

template <int NW, int RW> static hipError_t launch_mw(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out)
{
    with_lane_output(out, [&](auto o) { hipLaunchKernelGGL((genasm_lane_mw_kernel<NW, RW, decltype(o)::value>), dim3(grid), dim3(64), lds_bytes, s, a); });
    return hipGetLastError();
}

hipError_t launch_align_lane_mw(const AlignArgs& a, int grid, size_t lds_bytes, hipStream_t s, LaneOutput out)
{
    const int nw = a.W <= 64 ? 1 : (a.W <= 128 ? 2 : 4), rw = a.tb_limit / 64 + 1;
    if (nw == 1 && rw == 1) return launch_mw<1, 1>(a, grid, lds_bytes, s, out);
    if (nw == 1 && rw == 2) return launch_mw<1, 2>(a, grid, lds_bytes, s, out);       // (W = 64, O = 0: the stop bit is row 64)
    if (nw == 2 && rw == 3) return launch_mw<2, 3>(a, grid, lds_bytes, s, out);       // (W = 128, O = 0)
    if (nw == 2 && rw == 1) return launch_mw<2, 1>(a, grid, lds_bytes, s, out);
    if (nw == 2 && rw == 2) return launch_mw<2, 2>(a, grid, lds_bytes, s, out);
    if (nw == 4 && rw == 1) return launch_mw<4, 1>(a, grid, lds_bytes, s, out);
    if (nw == 4 && rw == 2) return launch_mw<4, 2>(a, grid, lds_bytes, s, out);
    if (nw == 4 && rw == 3) return launch_mw<4, 3>(a, grid, lds_bytes, s, out);
    if (nw == 4 && rw == 4) return launch_mw<4, 4>(a, grid, lds_bytes, s, out);
    return hipErrorInvalidValue;
}

}  // namespace scrg
