// lane_common.h — what the one-pair-per-lane aligner kernels share (genasm_lane_kernel.hip, genasm_lane_wide_kernel.hip,
// genasm_lane_parts_kernel.hip, genasm_lane_mw_kernel.hip): the truth tables and instruction helpers of their tables and
// walks, the wavefront priority rotation, the work-queue claim, the unpacking of a pair descriptor, a pair's edit limit and the
// writer of a lane's output (its CIGAR staging ring -> its slice of a.runs, and the pair's result words).  Each kernel keeps its
// own policy of WHEN to write (flush_pieces and the like): that is where store timing is tuned.  With the output mode LANE_OUT_NONE
// (genasm_kernels.h: distance-only) there is no ring and no slice: a pair leaves through retire_pair_distance.  (Helpers that the GenASM-row
// kernels use as well are in genasm_device.h.)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "genasm_kernels.h"
#include "genasm_device.h"
#include "text_revcomp.h"

namespace scrg {

// truth tables (inputs a, b, c in that order)
// (two-input operations are left to plain and/or/xor: 4-byte encodings, a v_bitop3_b32 takes 8)
constexpr int TT_XH  = bitop3_table([](int sum, int pv, int eq) { return (sum ^ pv) | eq; });
constexpr int TT_PH  = bitop3_table([](int mv, int xh, int pv) { return mv | ~(xh | pv); });
constexpr int TT_PVN = bitop3_table([](int mhs, int xv, int phs) { return mhs | ~(xv | phs); });
constexpr int TT_NOR3 = bitop3_table([](int a, int b, int c) { return ~(a | b | c); });
constexpr int TT_NIV  = bitop3_table([](int nv1, int v0, int stop) { return nv1 | ~v0 | stop; });     // not (insertion), or the stop row
constexpr int TT_ANDN = bitop3_table([](int a, int b, int) { return a & ~b; });
constexpr int TT_BFI = bitop3_table([](int a, int b, int c) { return (a & c) | (b & ~c); });       // bits of a where c is set, else b
constexpr int TT_ANDOR = bitop3_table([](int a, int b, int c) { return (a & b) | c; });
constexpr int TT_V0  = bitop3_table([](int pvn, int ph, int xh) { return pvn | ~(ph | xh); });

// LDS accesses by 32-bit LDS address (no generic-pointer arithmetic in front of the ds instruction)
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x2_t lds_u32x2_t;
__device__ __forceinline__ uint2 lds_read64(uint32_t addr)
{
    const u32x2_t v = *reinterpret_cast<const lds_u32x2_t*>((uintptr_t)addr);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void lds_write64(uint32_t addr, uint2 v)
{
    u32x2_t w;
    w.x = v.x;
    w.y = v.y;
    *reinterpret_cast<lds_u32x2_t*>((uintptr_t)addr) = w;
}
// One byte to LDS AS WRITTEN: one ds_write_b8 whose offset field takes the constant part of the address.  A plain byte store in an
// unrolled loop is merged with its neighbours into dword stores, and the packing is done on the VALU, which the lane kernels are
// bound by — five instructions of the slow class per dword (v_lshlrev_b16, v_bitop3_b16, v_or_b32_sdwa) where the LDS pipe has time.
__device__ __forceinline__ void lds_store_u8(uint32_t addr, uint32_t v)
{
    *reinterpret_cast<volatile __attribute__((address_space(3))) uint8_t*>((uintptr_t)addr) = (uint8_t)v;
}

__device__ __forceinline__ uint32_t ffbh_u32(uint32_t v)      // count leading zeros; 0xffffffff for v == 0
{
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

__device__ __forceinline__ uint32_t ffbl_u32(uint32_t v)      // count trailing zeros; 0xffffffff for v == 0
{
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// q + 2 * bit as ONE instruction, and as written (the optimiser otherwise sums the bits of an iteration first and rebuilds every
// slot offset from the offset at the start of the iteration: one more instruction per slot)
__device__ __forceinline__ uint32_t add_twice(uint32_t q, uint32_t bit)
{
    uint32_t r;
    asm("v_lshl_add_u32 %0, %1, 1, %2" : "=v"(r) : "v"(bit), "v"(q));
    return r;
}

__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c)      // a * b + c for a, b < 2^24, as written (v_mad_u32_u24)
{
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
    return r;
}

__device__ __forceinline__ uint32_t add3(uint32_t a, uint32_t b, uint32_t c)       // a + b + c (c wave-uniform), as written (v_add3_u32)
{
    uint32_t r;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

__device__ __forceinline__ uint64_t shl64(uint64_t v, uint32_t s)      // one v_lshlrev_b64 (count modulo 64)
{
    uint64_t r;
    asm("v_lshlrev_b64 %0, %1, %2" : "=v"(r) : "v"(s), "v"(v));
    return r;
}
__device__ __forceinline__ uint64_t shr64(uint64_t v, uint32_t s)
{
    uint64_t r;
    asm("v_lshrrev_b64 %0, %1, %2" : "=v"(r) : "v"(s), "v"(v));
    return r;
}
__device__ __forceinline__ uint32_t clz64(uint64_t v)                  // 64 for v == 0 (through 0xffffffff + 32 -> min)
{
    return min(ffbh_u32((uint32_t)(v >> 32)), ffbh_u32((uint32_t)v) + 32u);
}

// A wavefront vote that only steers a uniform branch: the lane mask of the compare that made `pred`, tested against zero on the
// scalar unit.  (__any(pred) first makes a 0 / 1 integer of that mask and compares it with zero again — v_cndmask_b32 0, 1 and
// v_cmp_ne_u32 into VCC, both of the slow class — to arrive at the mask it started from.)
__device__ __forceinline__ bool wave_any(bool pred)
{
    return __builtin_amdgcn_ballot_w64(pred) != 0ull;
}

// hardware wave slot on my SIMD (HW_ID bits 3:0)
__device__ __forceinline__ uint32_t hw_wave_slot()
{
    return __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 4);
}

// The SIMD's arbiter issues oldest-wave-first: left alone, the first wavefront on a SIMD runs at the speed of a lone wave and
// the last one finishes 2.7x later, with the SIMD half idle at the end of a launch.  Rotating the priorities (one step per
// round, starting from the wave slot: a different wavefront is on top from round to round) lets the wavefronts of a SIMD
// progress, and finish, together.  (Until round 4 the rotation was keyed on the clock: s_memtime and the wait for it — which
// is a wait for every LDS operation in flight as well — cost a wavefront that has its SIMD to itself ~1 000 cycles per round:
// one launch of 100 k pairs 2.45 -> 2.30 ms without it.)
__device__ __forceinline__ void rotate_priority(uint32_t round)
{
    const uint32_t pr = round & 3u;
    if (pr == 0) __builtin_amdgcn_s_setprio(0);
    else if (pr == 1) __builtin_amdgcn_s_setprio(1);
    else if (pr == 2) __builtin_amdgcn_s_setprio(2);
    else __builtin_amdgcn_s_setprio(3);
}

// The work queue: one atomic per wavefront for all the lanes that want a pair.  Returns my queue index (consecutive over
// the askers; >= a.n_pairs: the queue is empty).
__device__ __forceinline__ uint32_t claim_pairs(const AlignArgs& a, uint32_t lane, bool want)
{
    const uint64_t askers = __ballot(want);
    const int first = __ffsll((unsigned long long)askers) - 1;
    uint32_t base = 0;
    if ((int)lane == first) base = atomicAdd(a.counter, (uint32_t)__popcll(askers));
    base = (uint32_t)__shfl((int)base, first);
    return base + (uint32_t)__popcll(askers & ((1ull << lane) - 1ull));
}

// Texts taken as the reverse complement of their stretch (a.text_rev, bit 63 of text_off; text_revcomp.h): word w (characters
// 64 w .. 64 w + 63, bit k <-> character 64 w + k, as a forward load delivers them) of the window at ref_idx, from the text's one
// packed (forward) copy.  off / text_len: the stretch as text_stretch left it.  A word past the text returns garbage that the
// tables never look at (its columns read "no character matches").
__device__ __forceinline__ Planes text_revcomp_word(const uint64_t* __restrict__ seq, uint64_t off, uint32_t text_len, uint32_t ref_idx,
                                                    uint32_t w, uint32_t stride)
{
    const TextRevAt r = text_rev_at(text_len, ref_idx, w);
    const Planes f = load_window_strided(seq, off, r.at, stride);
    Planes t;
    t.lo = ~brev64(f.lo << r.sh);
    t.hi = ~brev64(f.hi << r.sh);
    return t;
}

// A pair descriptor as the lane kernels use it: lengths and capacity saturated to 32 bits, the strand bit taken out of
// read_off (only when a.stranded: rev = align the read's reverse complement), the text's out of text_off (only when a.text_rev:
// trev = align against the reverse complement of the stretch; text_off / text_len: text_revcomp.h, text_stretch).
struct LanePair {
    uint64_t text_off, read_off, cigar_off;
    uint32_t text_len, read_len, cigar_cap;
    bool rev, trev;
};
__device__ __forceinline__ LanePair unpack_pair(const AlignArgs& a, uint32_t idx)
{
    const scrg_pair_desc pd = a.pairs[idx];
    LanePair p;
    const TextStretch ts = text_stretch(pd.text_off, pd.text_len, a.text_rev != 0u, a.text_stride);
    p.text_off = ts.off;
    p.trev = ts.rev;
    p.read_off = a.stranded ? pd.read_off & ~SCRG_READ_REVCOMP : pd.read_off;
    p.rev = a.stranded && (pd.read_off & SCRG_READ_REVCOMP) != 0;
    p.text_len = ts.len;
    p.read_len = (uint32_t)pd.read_len;
    p.cigar_off = pd.cigar_off;
    p.cigar_cap = pd.cigar_cap > 0xffffffffull ? 0xffffffffu : (uint32_t)pd.cigar_cap;
    return p;
}

// The edit limit of a pair with this read length, once per claim: min(max_edits, floor(per_mille * read_len / 1000)), a part
// that is off (0xffffffff / 0) dropping out; 0xffffffff with both off, which no running sum of edits exceeds.  A pair whose
// running sum exceeds it at the end of a window is retired there with abandon_pair.
__device__ __forceinline__ uint32_t pair_edit_limit(const AlignArgs& a, uint32_t read_len)
{
    const uint32_t by_len = a.per_mille ? (uint32_t)((uint64_t)a.per_mille * read_len / 1000u) : 0xffffffffu;
    return min(a.max_edits, by_len);
}

// One 16-run piece of my ring (ring_b: its LDS byte address, 32 runs) -> my slice (two 16-byte stores); pieces past the
// slice's capacity are dropped.  flushed: runs already written, a multiple of 16.  EDITS: the slice holds bytes — it starts
// at byte 2 * cigar_off and is 2 * cigar_cap bytes long — the ring 64 of them, a piece is 32 bytes of the stream and flushed
// counts bytes.  store = false (ablation builds) drops every piece.
template <bool EDITS>
__device__ __forceinline__ void write_piece(const AlignArgs& a, const uint32_t* lds, uint32_t ring_b, uint64_t cigar_off, uint32_t cigar_cap,
                                            uint32_t& flushed, bool store = true)
{
    const uint32_t rd = EDITS ? (ring_b >> 2) + ((flushed & 32u) >> 2) : (ring_b >> 2) + ((flushed & 16u) >> 1);
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = lds[rd + k];
    const bool room = EDITS ? flushed + 32u <= 2u * (uint64_t)cigar_cap : flushed + 16u <= cigar_cap;
    if (store && room) {
        uint4* const dst = EDITS ? reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(a.runs + cigar_off) + flushed)
                                 : reinterpret_cast<uint4*>(a.runs + cigar_off + flushed);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    flushed += EDITS ? 32u : 16u;
}

// Retire a finished pair: the rest of its output (n runs; EDITS: n bytes, the matches after the last edit being implied by
// the read length) and its result words.  The last, partial piece goes out as whole dwords (EDITS: bytes past the end
// zeroed): cigar_cap is a multiple of 16 runs, so rounding up to a dword stays inside the slice.  nr: EDITS only, the index
// of the last run the same alignment has (a.run_count reports nr + 1).  PIECES = false: the kernel never leaves a whole piece
// behind, and there is no loop for them.
template <bool EDITS, bool PIECES = true>
__device__ __forceinline__ void retire_pair(const AlignArgs& a, const uint32_t* lds, uint32_t ring_b, uint32_t pair, uint64_t cigar_off,
                                            uint32_t cigar_cap, uint32_t& flushed, uint32_t n, int32_t nr, uint32_t edits, bool store = true)
{
    if (EDITS) {
        if (PIECES)
            while (n - flushed >= 32u) write_piece<true>(a, lds, ring_b, cigar_off, cigar_cap, flushed, store);
        const uint32_t rem = n - flushed;                            // < 32
        const uint32_t rd = (ring_b >> 2) + ((flushed & 32u) >> 2);
        uint32_t* const dst = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.runs + cigar_off) + flushed);
        for (uint32_t k = 0; 4u * k < rem; k++) {
            const uint32_t left = rem - 4u * k;
            const uint32_t keep = left >= 4u ? 0xffffffffu : (0xffffffffu >> (32u - 8u * left));
            if (flushed + 4u * k < 2u * (uint64_t)cigar_cap) dst[k] = lds[rd + k] & keep;
        }
        a.ed[pair] = (int64_t)edits;
        a.n_runs[pair] = n;
        a.status[pair] = n > 2u * (uint64_t)cigar_cap ? LANE_STATUS_OVERFLOW : LANE_STATUS_DONE;
        if (a.run_count) a.run_count[pair] = (uint32_t)(nr + 1);
    } else {
        if (PIECES)
            while (n - flushed >= 16u) write_piece<false>(a, lds, ring_b, cigar_off, cigar_cap, flushed, store);
        const uint32_t rem = n - flushed;                            // < 16
        const uint32_t rd = (ring_b >> 2) + ((flushed & 16u) >> 1);
        uint32_t* const dst = reinterpret_cast<uint32_t*>(a.runs + cigar_off + flushed);
        for (uint32_t k = 0; 2u * k < rem; k++)
            if (flushed + 2u * k < cigar_cap) dst[k] = lds[rd + k];
        a.ed[pair] = (int64_t)edits;
        a.n_runs[pair] = n;
        a.status[pair] = n > cigar_cap ? LANE_STATUS_OVERFLOW : LANE_STATUS_DONE;
    }
}

// Retire a pair over its edit limit (pair_edit_limit): the edit distance is the running sum (> the limit, <= the full
// distance), no runs (EDITS: no stream bytes, a.run_count 0), status LANE_STATUS_OVER_EDIT_LIMIT.  What of its output was
// already written stays in its slice, past the length reported.  OUT (LaneOutput) = LANE_OUT_NONE: text_end 0, and a.n_runs
// does not exist.
template <int OUT>
__device__ __forceinline__ void abandon_pair(const AlignArgs& a, uint32_t pair, uint32_t edits)
{
    a.ed[pair] = (int64_t)edits;
    if (OUT != LANE_OUT_NONE) a.n_runs[pair] = 0u;
    a.status[pair] = LANE_STATUS_OVER_EDIT_LIMIT;
    if (OUT == LANE_OUT_EDITS && a.run_count) a.run_count[pair] = 0u;
    if (OUT == LANE_OUT_NONE && a.text_end) a.text_end[pair] = 0u;
}

// LANE_OUT_NONE: retire a finished pair — its edit distance, its status (0: there is no slice to overflow) and the text
// characters its alignment consumed (ref_idx after its last window: the '=', 'X' and 'D' counts of the CIGAR nobody wrote).
__device__ __forceinline__ void retire_pair_distance(const AlignArgs& a, uint32_t pair, uint32_t edits, uint32_t ref_idx)
{
    a.ed[pair] = (int64_t)edits;
    a.status[pair] = 0u;
    if (a.text_end) a.text_end[pair] = ref_idx;
}

}  // namespace scrg
