// lane_multiword.h — what the lane-per-pair kernels for the non-default window settings share on top of lane_common.h:
//   * a lane's pair state and the round's retire / claim loop (genasm_lane_wide_kernel.hip, genasm_lane_parts_kernel.hip,
//     genasm_lane_mw_kernel.hip);
//   * for the two kernels that keep a part of the table in registers (wide: two halves of 32 columns, parts: parts of 16):
//     the window set-up (pattern -> Eq words in LDS, boundary column, swizzled text planes), one column of the recurrence
//     on NW-word vectors, and a part's second pass — pass 1's masks -> events -> runs or edit-stream bytes, and the
//     window-end bytes of the edit stream.
// All of it takes the kernels' output mode (genasm_kernels.h: LaneOutput); with LANE_OUT_NONE the second pass is not called at all.
// What differs stays in the kernels: which columns are swept and what is stored, how far ahead the Eq words are read, how a
// short text is selected, the walk (pass 1), and WHEN the staging ring is written out (flush_pieces, the trip counts).
// genasm_lane_kernel.hip keeps its own copies of all of this (one-word, 32-bit code): its register assignment is sensitive
// to such edits and bench.py ties its roofline figures to that file's hash.
#pragma once

#include "lane_common.h"

namespace scrg {

// ---------------- a lane's pair, and the round's retire / claim loop ----------------
// (The pair's strand — rev: its read is aligned as its reverse complement, genasm_device.h: revcomp_pattern_word — and its text's
// — trev: lane_common.h: text_revcomp_word — are `bool`s of the kernel next to this struct: as a member it is kept as a byte in a VGPR instead of a lane mask in SGPRs, and
// genasm_lane_parts_kernel<3, true>, at 256 VGPRs, then needs 12 bytes of scratch.)
struct LaneWork {
    bool has_pair = false;
    uint32_t pair = 0;
    uint64_t text_off = 0, read_off = 0, cigar_off = 0;
    uint32_t text_len = 0, read_len = 0, cigar_cap = 0;
    uint32_t ref_idx = 0, read_idx = 0, edits = 0;
    uint32_t lim = 0xffffffffu;        // my pair's edit limit (lane_common.h: pair_edit_limit)
    int32_t nr = -1;                   // index of the last committed run; n_runs = nr + 1
    uint32_t flushed = 0;              // runs below this index are in HBM (a multiple of 16); EDITS: bytes, a multiple of 32
    uint32_t pos = 0;                  // EDITS: bytes of the pair's stream so far
    uint32_t mbase = 0;                // EDITS: matches pending at column c of the current part (mw: window) = mbase + c
    bool queue_empty = false;          // wave-uniform
};

// Retire finished pairs, fetch new ones (genasm_cpu.cpp:440-460).  False: no lane of the wavefront has a pair, and the queue
// is empty.  PIECES: see retire_pair.  OUT: LaneOutput; LANE_OUT_NONE: nothing of the ring or of the pair's slice is touched (lds and
// ring_b are not used), and the state of the second pass (cigar_off ... mbase) stays as it was constructed.
template <int OUT, bool PIECES = true>
__device__ __forceinline__ bool next_pairs(const AlignArgs& a, const uint32_t* lds, uint32_t ring_b, uint32_t lane, LaneWork& w, bool& rev, bool& trev)
{
    for (;;) {
        const bool over = w.has_pair && w.edits > w.lim;             // (over the limit wins over a read that is done)
        const bool fin = over || (w.has_pair && w.read_idx >= w.read_len);
        if (wave_any(fin)) {
            constexpr bool EDITS = OUT == LANE_OUT_EDITS;
            if (over) abandon_pair<OUT>(a, w.pair, w.edits);
            else if constexpr (OUT == LANE_OUT_NONE) { if (fin) retire_pair_distance(a, w.pair, w.edits, w.ref_idx); }
            else if (fin) retire_pair<EDITS, PIECES>(a, lds, ring_b, w.pair, w.cigar_off, w.cigar_cap, w.flushed, EDITS ? w.pos : (uint32_t)(w.nr + 1), w.nr, w.edits);
            w.has_pair = w.has_pair && !fin;
        }
        const bool want = !w.has_pair && !w.queue_empty;
        if (!wave_any(want)) break;
        const uint32_t idx = claim_pairs(a, lane, want);
        const bool got = want && idx < a.n_pairs;
        if (wave_any(want && idx >= a.n_pairs)) w.queue_empty = true;
        if (got) {
            const LanePair p = unpack_pair(a, idx);
            w.pair = idx;
            w.text_off = p.text_off;
            w.read_off = p.read_off;
            rev = p.rev;
            trev = p.trev;
            w.text_len = p.text_len;
            w.read_len = p.read_len;
            w.lim = pair_edit_limit(a, p.read_len);
            if constexpr (OUT == LANE_OUT_NONE) {
                w.ref_idx = w.read_idx = w.edits = 0;
            } else {
                w.cigar_off = p.cigar_off;
                w.cigar_cap = p.cigar_cap;
                w.ref_idx = w.read_idx = w.edits = w.flushed = w.pos = w.mbase = 0;
                w.nr = -1;
            }
            w.has_pair = true;
        }
    }
    return wave_any(w.has_pair);
}

// ---------------- window set-up ----------------
// The difference vectors between two text columns: NW 64-bit words, word 0 the most significant (bit 63-k of word w
// belongs to pattern character 64 w + k), each as two dwords (.x low, .y high).
template <int NW> struct LaneVec {
    uint2 pv[NW], mv[NW];
};

// `count` characters starting at character k of a sequence -> planes, one dword per 32 columns (only the words that
// hold one of those characters are read: nothing past the end of the sequence)
template <int NW>
__device__ __forceinline__ void load_planes(const uint64_t* __restrict__ seq, uint64_t off, uint32_t k, uint32_t count, uint32_t stride,
                                            uint32_t (&lo)[2 * NW], uint32_t (&hi)[2 * NW])
{
    uint32_t s;
    const uint64_t w0 = window_first_word(off, k, stride, s);
    uint64_t v[2 * NW + 1];
#pragma unroll
    for (int q = 0; q <= 2 * NW; q++) v[q] = 32u * (uint32_t)q < s + count ? seq[w0 + (uint64_t)q * stride] : 0ull;
#pragma unroll
    for (int q = 0; q < 2 * NW; q++) {
        lo[q] = __builtin_amdgcn_alignbit((uint32_t)v[q + 1], (uint32_t)v[q], s);
        hi[q] = __builtin_amdgcn_alignbit((uint32_t)(v[q + 1] >> 32), (uint32_t)(v[q] >> 32), s);
    }
}

// A window's extent (genasm_cpu.cpp:417-420).  tbl = W - O.
struct LaneWindow {
    uint32_t n;        // text columns
    uint32_t m;        // pattern rows; >= 1 for live pairs
    uint32_t jlim;     // the walk ends when j gets here (:301, :310): the stop row
};
__device__ __forceinline__ LaneWindow window_extent(const LaneWork& w, uint32_t W, uint32_t tbl)
{
    LaneWindow x;
    x.n = (w.has_pair && w.ref_idx < w.text_len) ? min(W, w.text_len - w.ref_idx) : 0u;
    x.m = w.has_pair ? min(W, w.read_len - w.read_idx) : 1u;
    x.jlim = w.has_pair ? min(x.m, tbl) : 0u;
    return x;
}

// The window's pattern -> the four Eq words (one per base, NW words each) in my LDS table at eq_b, the word "no character
// matches" at nomatch_b, and the boundary column in st; the window's text -> the planes tl / th.  A base's words are SLOT
// bytes apart; lanes that share LDS banks use different slots for the same base (swz, 0..3): the slot of base b is
// b ^ swz, and the swizzle is folded into the text planes, which are what a sweep makes its Eq addresses from.
template <int NW, uint32_t SLOT>
__device__ __forceinline__ void window_setup(const AlignArgs& a, const LaneWork& w, bool rev, bool trev, const LaneWindow& win, uint32_t eq_b,
                                             uint32_t nomatch_b, uint32_t swz, LaneVec<NW>& st, uint32_t (&tl)[2 * NW], uint32_t (&th)[2 * NW])
{
    uint32_t plo[2 * NW], phi[2 * NW];
#pragma unroll
    for (int q = 0; q < 2 * NW; q++) { plo[q] = phi[q] = tl[q] = th[q] = 0; }
    if (w.has_pair) {
        if (!trev) load_planes<NW>(a.seq, w.text_off, w.ref_idx, win.n, a.text_stride, tl, th);      // (a reversed lane loads its words once, below)
        load_planes<NW>(a.seq, w.read_off, w.read_idx, win.m, a.read_stride, plo, phi);
    }
    if (a.text_rev && wave_any(w.has_pair && trev)) {          // (uniform) texts taken as the reverse complement of their stretch
#pragma unroll
        for (int q = 0; q < NW; q++) {
            if (w.has_pair && trev && 64u * (uint32_t)q < win.n) {
                const Planes tv = text_revcomp_word(a.seq, w.text_off, w.text_len, w.ref_idx, (uint32_t)q, a.text_stride);
                tl[2 * q] = (uint32_t)tv.lo; tl[2 * q + 1] = (uint32_t)(tv.lo >> 32);
                th[2 * q] = (uint32_t)tv.hi; th[2 * q + 1] = (uint32_t)(tv.hi >> 32);
            }
        }
    }
    // the reversed pattern, LEFT-aligned over the NW words: bit 63-k of word w <-> pattern[64 w + k]; below the
    // pattern Eq = 1, Pv = Mv = 0 (no carry starts there, 0 comes in at its lowest bit)
    const uint32_t x = eq_b | (swz * SLOT);
    const uint32_t m = win.m;
#pragma unroll
    for (int q = 0; q < NW; q++) {
        // word q: characters 64 q .. 64 q + 63 = plane dwords 2q (-> high dword, reversed) and 2q + 1 (-> low dword)
        uint32_t rl1 = __builtin_bitreverse32(plo[2 * q]), rl0 = __builtin_bitreverse32(plo[2 * q + 1]);
        uint32_t rh1 = __builtin_bitreverse32(phi[2 * q]), rh0 = __builtin_bitreverse32(phi[2 * q + 1]);
        if (a.stranded && wave_any(w.has_pair && rev)) {       // (uniform) minus-strand pairs: the word comes reversed from the read's forward copy
            const Planes rv = revcomp_pattern_word(a.seq, w.read_off, w.read_len, w.has_pair ? w.read_idx : w.read_len, (uint32_t)q, a.read_stride);
            if (w.has_pair && rev) {
                rl1 = (uint32_t)(rv.lo >> 32); rl0 = (uint32_t)rv.lo;
                rh1 = (uint32_t)(rv.hi >> 32); rh0 = (uint32_t)rv.hi;
            }
        }
        const uint32_t lo_chars = 64u * (uint32_t)q;
        const uint64_t valid = m >= lo_chars + 64u ? ~0ull : (m <= lo_chars ? 0ull : ~0ull << (64u - (m - lo_chars)));
        const uint32_t iv0 = ~(uint32_t)valid, iv1 = ~(uint32_t)(valid >> 32);
        lds_write64((x ^ (0u * SLOT)) + 8u * q, make_uint2(~(rl0 | rh0) | iv0, ~(rl1 | rh1) | iv1));
        lds_write64((x ^ (1u * SLOT)) + 8u * q, make_uint2((rl0 & ~rh0) | iv0, (rl1 & ~rh1) | iv1));
        lds_write64((x ^ (2u * SLOT)) + 8u * q, make_uint2((~rl0 & rh0) | iv0, (~rl1 & rh1) | iv1));
        lds_write64((x ^ (3u * SLOT)) + 8u * q, make_uint2((rl0 & rh0) | iv0, (rl1 & rh1) | iv1));
        lds_write64(nomatch_b + 8u * q, make_uint2(iv0, iv1));
        st.pv[q] = make_uint2((uint32_t)valid, (uint32_t)(valid >> 32));       // D[n][j] = m-j: every vertical step is +1
        st.mv[q] = make_uint2(0u, 0u);
    }
    // the slot swizzle folded into the text planes
    const uint32_t swl = 0u - (swz & 1u), swh = 0u - (swz >> 1);
#pragma unroll
    for (int q = 0; q < 2 * NW; q++) { tl[q] ^= swl; th[q] ^= swh; }
}

// ---------------- one column of the recurrence ----------------
// a + b over 2 NW dwords, least significant first (word NW-1 low dword ... word 0 high dword): one carry chain
template <int NW> __device__ __forceinline__ void add_chain(const uint32_t (&a)[2 * NW], const uint32_t (&b)[2 * NW], uint32_t (&s)[2 * NW])
{
    if constexpr (NW == 1) {
        const uint64_t sum = add64(((uint64_t)a[1] << 32) | a[0], ((uint64_t)b[1] << 32) | b[0]);
        s[0] = (uint32_t)sum;
        s[1] = (uint32_t)(sum >> 32);
    } else if constexpr (NW == 2) {
        asm("v_add_co_u32 %0, vcc, %4, %8\n\t"
            "v_addc_co_u32 %1, vcc, %5, %9, vcc\n\t"
            "v_addc_co_u32 %2, vcc, %6, %10, vcc\n\t"
            "v_addc_co_u32 %3, vcc, %7, %11, vcc"
            : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3])
            : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3])
            : "vcc");
    } else if constexpr (NW == 3) {
        asm("v_add_co_u32 %0, vcc, %6, %12\n\t"
            "v_addc_co_u32 %1, vcc, %7, %13, vcc\n\t"
            "v_addc_co_u32 %2, vcc, %8, %14, vcc\n\t"
            "v_addc_co_u32 %3, vcc, %9, %15, vcc\n\t"
            "v_addc_co_u32 %4, vcc, %10, %16, vcc\n\t"
            "v_addc_co_u32 %5, vcc, %11, %17, vcc"
            : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3]), "=&v"(s[4]), "=&v"(s[5])
            : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5])
            : "vcc");
    } else {
        asm("v_add_co_u32 %0, vcc, %8, %16\n\t"
            "v_addc_co_u32 %1, vcc, %9, %17, vcc\n\t"
            "v_addc_co_u32 %2, vcc, %10, %18, vcc\n\t"
            "v_addc_co_u32 %3, vcc, %11, %19, vcc\n\t"
            "v_addc_co_u32 %4, vcc, %12, %20, vcc\n\t"
            "v_addc_co_u32 %5, vcc, %13, %21, vcc\n\t"
            "v_addc_co_u32 %6, vcc, %14, %22, vcc\n\t"
            "v_addc_co_u32 %7, vcc, %15, %23, vcc"
            : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3]), "=&v"(s[4]), "=&v"(s[5]), "=&v"(s[6]), "=&v"(s[7])
            : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]),
              "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(b[4]), "v"(b[5]), "v"(b[6]), "v"(b[7])
            : "vcc");
    }
}

// What a column's table words need besides the vectors in front of it.
template <int NW> struct LaneColumn {
    uint2 xh[NW], ph[NW];
};

// One text column: st (the vectors behind it, Pv / Mv) -> the vectors in front of it; eq: the Eq words of its character.
template <int NW> __device__ __forceinline__ LaneColumn<NW> sweep_column(LaneVec<NW>& st, const uint2 (&eq)[NW])
{
    LaneColumn<NW> col;
    uint2 xv[NW], mh[NW];
    {   // the add (Eq & Pv) + Pv: carries run from the last word to word 0
        uint32_t aa[2 * NW], bb[2 * NW], ss[2 * NW];
#pragma unroll
        for (int q = 0; q < NW; q++) {                       // dword 2 k, 2 k + 1 of the chain = word NW-1-k
            aa[2 * q] = eq[NW - 1 - q].x & st.pv[NW - 1 - q].x;
            aa[2 * q + 1] = eq[NW - 1 - q].y & st.pv[NW - 1 - q].y;
            bb[2 * q] = st.pv[NW - 1 - q].x;
            bb[2 * q + 1] = st.pv[NW - 1 - q].y;
        }
        add_chain<NW>(aa, bb, ss);
#pragma unroll
        for (int q = 0; q < NW; q++) {
            col.xh[NW - 1 - q].x = bitop3<TT_XH>(ss[2 * q], st.pv[NW - 1 - q].x, eq[NW - 1 - q].x);
            col.xh[NW - 1 - q].y = bitop3<TT_XH>(ss[2 * q + 1], st.pv[NW - 1 - q].y, eq[NW - 1 - q].y);
        }
    }
#pragma unroll
    for (int q = 0; q < NW; q++) {
        xv[q].x = eq[q].x | st.mv[q].x;
        xv[q].y = eq[q].y | st.mv[q].y;
        col.ph[q].x = bitop3<TT_PH>(st.mv[q].x, col.xh[q].x, st.pv[q].x);
        col.ph[q].y = bitop3<TT_PH>(st.mv[q].y, col.xh[q].y, st.pv[q].y);
        mh[q].x = st.pv[q].x & col.xh[q].x;
        mh[q].y = st.pv[q].y & col.xh[q].y;
    }
    // << 1 over all the words: row 0 of the matrix is all zeros, 0 comes in at the bottom
    uint2 phs[NW], mhs[NW];
    {
        const uint64_t p = shl1(((uint64_t)col.ph[NW - 1].y << 32) | col.ph[NW - 1].x), m = shl1(((uint64_t)mh[NW - 1].y << 32) | mh[NW - 1].x);
        phs[NW - 1] = make_uint2((uint32_t)p, (uint32_t)(p >> 32));
        mhs[NW - 1] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
#pragma unroll
    for (int q = NW - 2; q >= 0; q--) {
        phs[q].x = __builtin_amdgcn_alignbit(col.ph[q].x, col.ph[q + 1].y, 31);
        phs[q].y = __builtin_amdgcn_alignbit(col.ph[q].y, col.ph[q].x, 31);
        mhs[q].x = __builtin_amdgcn_alignbit(mh[q].x, mh[q + 1].y, 31);
        mhs[q].y = __builtin_amdgcn_alignbit(mh[q].y, mh[q].x, 31);
    }
#pragma unroll
    for (int q = 0; q < NW; q++) {
        st.pv[q].x = bitop3<TT_PVN>(mhs[q].x, xv[q].x, phs[q].x);
        st.pv[q].y = bitop3<TT_PVN>(mhs[q].y, xv[q].y, phs[q].y);
        st.mv[q].x = phs[q].x & xv[q].x;
        st.mv[q].y = phs[q].y & xv[q].y;
    }
    return col;
}

// Word r of the column's two table rows, {~(V1 | stop), V0 | stop} (V1 = Pv' | Ph, V0 = Pv' | ~(Ph | Xh)); st: the vectors
// sweep_column left, stop: word r of the stop row.
template <int NW>
__device__ __forceinline__ void table_words(const LaneVec<NW>& st, const LaneColumn<NW>& col, int r, uint2 stop, uint64_t& nv1, uint64_t& v0)
{
    nv1 = ((uint64_t)bitop3<TT_NOR3>(st.pv[r].y, col.ph[r].y, stop.y) << 32) | bitop3<TT_NOR3>(st.pv[r].x, col.ph[r].x, stop.x);
    v0 = ((uint64_t)(bitop3<TT_V0>(st.pv[r].y, col.ph[r].y, col.xh[r].y) | stop.y) << 32) | (bitop3<TT_V0>(st.pv[r].x, col.ph[r].x, col.xh[r].x) | stop.x);
}

// ---------------- a part's second pass: masks -> events -> runs or edit-stream bytes ----------------
// A lane's staging areas in LDS: its ring (32 runs, or 64 bytes of the edit stream) and, one byte per column of a part, the
// insertion-run lengths pass 1 left.
struct LaneLds {
    uint32_t* lds;
    uint32_t ring_b, scr_b;            // byte offsets
    __device__ __forceinline__ char* bytes() const { return reinterpret_cast<char*>(lds); }
    __device__ __forceinline__ uint8_t* u8() const { return reinterpret_cast<uint8_t*>(lds); }
};

// The events of a part of COLS columns (32 or 16): column s <-> bit 31-s.
struct PartEvents {
    uint32_t ti;           // the lane was alive in the part's first ti columns
    uint32_t D, X, Im;     // deletion / substitution at the column, insertion run in front of it
    uint32_t B;            // a D / X / = run starts here
    uint32_t cont;         // bit 31: the first step continues the previous part's last run
};

// From pass 1's masks (one bit shifted in per column: nDm not a deletion, Xm substitution, nIm no insertion run; `steps`
// pattern rows consumed) to the part's events; counts its edits and text columns.  live = false: the lane's masks are
// garbage (a lane without a pair after a one-word walk), it has no events.  A part after the window's first one whose first
// step continues the previous part's last run starts no run at its column 0 (last_dx: D and X bits of the previous part's
// last column — bit 1, bit 0 — if the lane was alive to its end, else 4; alive: still walking after this part).
template <int COLS>
__device__ __forceinline__ PartEvents part_events(LaneWork& w, bool live, bool first, uint32_t ncols, uint32_t nDm, uint32_t Xm, uint32_t nIm,
                                                  uint32_t steps, uint32_t& last_dx, bool& alive)
{
    PartEvents e;
    // the lane was alive in the ti columns before the first "deletion and substitution" (the stop row)
    const uint32_t nsh = 32u - ncols;
    const uint32_t Draw = ~(nDm << nsh), Xraw = Xm << nsh;
    e.ti = live ? min(ffbh_u32(Draw & Xraw), ncols) : 0u;
    const uint32_t A = ~(uint32_t)shr64(0xffffffffull, e.ti);      // the top ti bits (ti = 0..32)
    e.D = Draw & A;
    e.X = Xraw & A;
    e.Im = ~nIm << nsh;
    e.B = ((e.D ^ (e.D >> 1)) | (e.X ^ (e.X >> 1)) | e.Im | 0x80000000u) & A;
    w.edits += steps - e.ti + 2u * (uint32_t)__builtin_popcount(e.D) + (uint32_t)__builtin_popcount(e.X);
    w.ref_idx += e.ti;
    e.cont = 0;
    if (!first) {
        const uint32_t first_dx = ((e.D >> 31) << 1) | (e.X >> 31);
        e.cont = (e.ti != 0u && (e.Im >> 31) == 0u && first_dx == last_dx) ? 0x80000000u : 0u;
        e.B &= ~e.cont;
    }
    constexpr uint32_t LAST = 32u - (uint32_t)COLS;                 // the bit of column COLS - 1
    last_dx = e.ti == (uint32_t)COLS ? ((((e.D >> LAST) & 1u) << 1) | ((e.X >> LAST) & 1u)) : 4u;
    alive = w.has_pair && e.ti == (uint32_t)COLS;
    return e;
}

// Pass 2, runs (genasm_lane_kernel<false>).  Every run goes to the slot after the last committed one; only committing moves
// on.  A run that crosses from one part into the next is ONE run of the window (the reference merges within a window,
// src/genasm_cpu.cpp:372-404): the steps up to the first event of a part that continues (e.cont) are added to the run
// committed last, which is still in the ring.  flush(): the kernel's flush_pieces, called every TRIPS x 2 events — the kernel
// states the ring bound that TRIPS keeps.
template <int COLS, uint32_t TRIPS, class Flush>
__device__ __forceinline__ void part_runs(const LaneLds& l, const PartEvents& e, LaneWork& w, Flush&& flush)
{
    char* const lds_b = l.bytes();
    const uint8_t* const lds8 = l.u8();
    uint32_t E = e.B | e.Im;
    uint32_t c = ffbh_u32(E);
    if (e.cont) {        // the steps up to the first event belong to the run committed last
        uint16_t* const prev = reinterpret_cast<uint16_t*>(lds_b + l.ring_b + ((2u * (uint32_t)w.nr) & 62u));
        *prev = (uint16_t)(*prev + min(c, e.ti));
    }
    uint32_t ni = lds8[l.scr_b + (c & (uint32_t)(COLS - 1))];
    uint32_t nr2 = 2u * (uint32_t)w.nr;          // byte offset of the last committed run
    // (a lane that has no event left has c = 0xffffffff; a part has a column 31 - c & 31, unlike genasm_lane_kernel's
    // windows, so its mask bits are taken with a field width of 0: nothing is committed)
    auto event = [&]() {
        const uint32_t sh = 31u - c;
        const uint32_t bit = 0x80000000u >> (c & 31u);
        const uint32_t live = ~c >> 31;
        *reinterpret_cast<uint16_t*>(lds_b + l.ring_b + ((nr2 + 2u) & 62u)) = (uint16_t)(((uint32_t)'I' << 8) | ni);
        nr2 += 2u * __builtin_amdgcn_ubfe(e.Im, sh, live);
        E = bitop3<TT_ANDN>(E, bit, bit);
        const uint32_t nx = ffbh_u32(E);
        ni = lds8[l.scr_b + (nx & (uint32_t)(COLS - 1))];
        const uint32_t len = min(nx, e.ti) - c;                       // up to the next event or the end of the walk
        const uint32_t rw = (((uint32_t)'=' << 8) + len) + __builtin_amdgcn_ubfe(e.D, sh, live) * (7u << 8) + __builtin_amdgcn_ubfe(e.X, sh, live) * (27u << 8);
        *reinterpret_cast<uint16_t*>(lds_b + l.ring_b + ((nr2 + 2u) & 62u)) = (uint16_t)rw;
        nr2 += 2u * __builtin_amdgcn_ubfe(e.B, sh, live);
        c = nx;
    };
    uint32_t trips = 0;
    while (wave_any(E != 0u)) {
        event();
        event();
        if (++trips == TRIPS) {
            trips = 0;
            w.nr = (int32_t)nr2 >> 1;
            flush();
        }
    }
    w.nr = (int32_t)nr2 >> 1;
    flush();
}

// Pass 2, edit stream (genasm_lane_kernel<true>): the columns that hold an edit.  Only those are visited: an insertion run
// (before the column's step), then a deletion or substitution.  w.mbase + c = matches pending when column c is reached (the
// window's own: its END byte follows the last part, window_end_bytes); an insertion at c leaves none at c (mbase = -c), a
// deletion / substitution none at c + 1.  Every byte goes to the slot after the last committed one; only committing moves
// on.  Three insertions are handled in line, longer runs on a side path.  (A lane that has no event left has c = 0xffffffff
// and takes its mask bits with a field width of 0.)
// LONG: 63 or more matches may be pending (W-O > 63, at most 126): the edit byte is then owed one or two bytes 0x3F (63
// matches each) first, one of them in line.  Without it fewer than 63 are ever pending where a byte is committed.
// flush(): as in part_runs.
template <int COLS, bool LONG, uint32_t TRIPS, class Flush>
__device__ __forceinline__ void part_edits(const AlignArgs& a, const LaneLds& l, const PartEvents& e, LaneWork& w, Flush&& flush)
{
    uint8_t* const lds8 = l.u8();
    uint32_t E = e.D | e.X | e.Im;
    w.nr += (int32_t)(__builtin_popcount(e.B) + __builtin_popcount(e.Im));       // the runs this part has in the other output format
    uint32_t c = ffbh_u32(E);
    uint32_t ni = lds8[l.scr_b + (c & (uint32_t)(COLS - 1))];
    const uint32_t DX = e.D | e.X;
    auto put = [&](uint32_t at, uint32_t b) { lds8[l.ring_b + (at & 63u)] = (uint8_t)b; };
    auto event = [&]() {
        const uint32_t sh = 31u - c;
        const uint32_t bit = 0x80000000u >> (c & 31u);
        const uint32_t lv = ~c >> 31;
        uint32_t iB = __builtin_amdgcn_ubfe(e.Im, sh, lv), dx = __builtin_amdgcn_ubfe(DX, sh, lv);
        const uint32_t xB = __builtin_amdgcn_ubfe(e.X, sh, lv);
        const uint32_t t = w.mbase + c;                            // matches pending
        E = bitop3<TT_ANDN>(E, bit, bit);
        const uint32_t nx = ffbh_u32(E);
        const uint32_t step = 0xC0u - 0x80u * xB;                  // 'D' 3 << 6, 'X' 1 << 6
        uint32_t k63 = 0;                                          // bytes 0x3F owed before the edit byte
        if constexpr (LONG) k63 = ((t >= 63u ? 1u : 0u) + (t >= 126u ? 1u : 0u)) * (iB | dx);      // (iB | dx: 0 only for a lane that is done)
        const uint32_t r = (t - 63u * k63) & 63u;
        const bool side = max(ni * iB, 2u * k63) > 3u;             // more than 3 insertions or 125 matches pending
        if (wave_any(side)) {
            if (side) {
                auto emit = [&](uint32_t b) {
                    put(w.pos, b);
                    w.pos++;
                    if (w.pos - w.flushed >= 32u) write_piece<true>(a, l.lds, l.ring_b, w.cigar_off, w.cigar_cap, w.flushed);
                };
                for (uint32_t q = k63; q; q--) emit(0x3Fu);
                if (!LONG || iB) {                                 // (not LONG: a long insertion run is the side path's only cause)
                    emit(0x80u | r);
                    for (uint32_t q = 1; q < ni; q++) emit(0x80u);
                    w.mbase = 0u - c;
                }
                if (dx) {
                    emit(step | ((!LONG || iB) ? 0u : r));
                    w.mbase = ~c;
                }
                iB = dx = k63 = 0;
            }
        }
        // in line: (LONG: one byte 0x3F, 63..125 matches pending,) up to three insertions, the step
        if constexpr (LONG) {
            put(w.pos, 0x3Fu);
            w.pos += k63;
        }
        put(w.pos, 0x80u | r);
        put(w.pos + 1u, 0x80u);
        put(w.pos + 2u, 0x80u);
        w.pos += iB ? ni : 0u;
        put(w.pos, step | (iB ? 0u : r));
        w.pos += dx;
        w.mbase = dx ? ~c : (iB ? 0u - c : w.mbase);
        ni = lds8[l.scr_b + (nx & (uint32_t)(COLS - 1))];
        c = nx;
    };
    uint32_t trips = 0;
    while (wave_any(E != 0u)) {
        event();
        event();
        if (++trips == TRIPS) {
            trips = 0;
            flush();
        }
    }
    flush();
    w.mbase += e.ti;
}

// The window ends (edit_stream.h): the matches since its last edit — each 63 of them a byte 0x3F first: at most one (a
// whole window of W-O = 63 without an edit), LONG: at most two (W-O <= 127) — and the mark.
template <bool LONG> __device__ __forceinline__ void window_end_bytes(const LaneLds& l, LaneWork& w)
{
    uint8_t* const lds8 = l.u8();
    uint32_t k63 = w.mbase >= 63u ? 1u : 0u;
    lds8[l.ring_b + (w.pos & 63u)] = (uint8_t)0x3Fu;
    if constexpr (LONG) {
        k63 += w.mbase >= 126u ? 1u : 0u;
        lds8[l.ring_b + ((w.pos + 1u) & 63u)] = (uint8_t)0x3Fu;
    }
    w.pos += w.has_pair ? k63 : 0u;
    lds8[l.ring_b + (w.pos & 63u)] = (uint8_t)(w.mbase - 63u * k63);
    w.pos += w.has_pair ? 1u : 0u;
    w.mbase = 0;
}

}  // namespace scrg
