// diff_kernels.hip — difference strings (SAM's MD:Z: and PAF's short cs:Z:) of every pair, from its runs and the two packed
// sequences: a length pass and a render pass with offsets by prefix sum between them.  Both walk the pairs' runs with run_walk.h
// (which the CIGAR text and the alignment report share).  HBM-bound helpers: a pair's runs are read once per pass and a few
// sequence words per edit besides.
//
// The string of a pair is the concatenation of what its runs emit, in order, then a tail and a NUL:
//   MD  '=' nothing;  'X' per base: the number of '=' bases pending (0 after the first), the TEXT base;  'D' the pending number and
//       '^' unless the run before it was a 'D', then its text bases;  'I' nothing (and the pending count stays);  tail: the number.
//   cs  '=' nothing;  'X' ":n" if n '=' bases are pending, then "*tq" per base;  'I' / 'D' ":n" likewise, '+' / '-' unless the
//       run before it had the same operation, then the read / text bases;  tail: ":n" if n are pending.
// So a run's bytes depend on three things that come from the runs before it: the pending '=' count (a SEGMENTED sum: it starts
// again after every run that emits it — X, D and for cs I), the operation of the run before it, and its text and read positions
// (prefix sums).  One pair per lane walks them serially; one wavefront per pair gets them for 512 runs at a time — the operation and
// the positions from run_walk.h's tile step, the pending count from a segmented scan here — and carries them from tile to tile.
// A pair without runs has "" in both kinds.
#include <hipcub/hipcub.hpp>

#include "genasm_kernels.h"
#include "host_path.h"
#include "run_walk.h"

namespace scrg {

constexpr uint32_t DIFF_TILE_BYTES = 4096;        // LDS staging per wavefront; a tile with more bytes (long X runs) goes straight to memory

// (the text is always forward here: a pair with SCRG_TEXT_REVCOMP is not served, its desc_ok is false and none of its bases is read)
__device__ __forceinline__ uint32_t fwd_text_code(const PairSeq& s, uint64_t t) { return base_code(s.seq, s.text_off, s.text_stride, t); }

__device__ __forceinline__ uint32_t num_digits(uint32_t v)
{
    uint32_t d = 1;
    while (v >= 10u) { v /= 10u; d++; }
    return d;
}
__device__ __forceinline__ uint32_t put_num(uint8_t* o, uint32_t v)
{
    const uint32_t d = num_digits(v);
    for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10u); v /= 10u; }
    return d;
}

struct DiffState : WalkPos {      // what a run needs to know of the runs before it: the positions, the operation of the run before, and
    uint32_t pend;                // the '=' bases since the last run that emitted the count
};

// does the run emit (and so clear) the pending count?
__device__ __forceinline__ bool run_resets(int32_t kind, uint32_t op) { return op == 'X' || op == 'D' || (kind == SCRG_DIFF_CS && op == 'I'); }

// One run: its bytes (written at o if WRITE), the state moved past it.  The run is valid (run_ok).
template <bool WRITE> __device__ __forceinline__ uint32_t emit_run(int32_t kind, uint32_t run, DiffState& st, uint8_t* o, const PairSeq& sq)
{
    const uint32_t c = run & 0xffu, op = run >> 8;
    uint32_t n = 0;
    if (op == '=') {
        st.pend += c;
        st.t += c;
        st.q += c;
    } else if (kind == SCRG_DIFF_MD) {
        if (op == 'X') {
            n = num_digits(st.pend) + 1u + 2u * (c - 1u);
            if (WRITE) {
                uint32_t w = put_num(o, st.pend);
                o[w++] = (uint8_t)"ACGT"[fwd_text_code(sq, st.t)];
                for (uint32_t j = 1; j < c; j++) {
                    o[w++] = (uint8_t)'0';
                    o[w++] = (uint8_t)"ACGT"[fwd_text_code(sq, st.t + j)];
                }
            }
            st.pend = 0;
            st.t += c;
            st.q += c;
        } else if (op == 'D') {
            const bool open = st.prev != 'D';
            n = (open ? num_digits(st.pend) + 1u : 0u) + c;
            if (WRITE) {
                uint32_t w = 0;
                if (open) {
                    w = put_num(o, st.pend);
                    o[w++] = (uint8_t)'^';
                }
                for (uint32_t j = 0; j < c; j++) o[w++] = (uint8_t)"ACGT"[fwd_text_code(sq, st.t + j)];
            }
            st.pend = 0;
            st.t += c;
        } else {
            st.q += c;
        }
    } else {
        const uint32_t lead = st.pend ? 1u + num_digits(st.pend) : 0u;
        uint32_t w = 0;
        if (WRITE && lead) {
            o[w++] = (uint8_t)':';
            w += put_num(o + w, st.pend);
        }
        if (op == 'X') {
            n = lead + 3u * c;
            if (WRITE)
                for (uint32_t j = 0; j < c; j++) {
                    o[w++] = (uint8_t)'*';
                    o[w++] = (uint8_t)"acgt"[fwd_text_code(sq, st.t + j)];
                    o[w++] = (uint8_t)"acgt"[read_code(sq, st.q + j)];
                }
            st.t += c;
            st.q += c;
        } else if (op == 'I') {
            const bool open = st.prev != 'I';
            n = lead + (open ? 1u : 0u) + c;
            if (WRITE) {
                if (open) o[w++] = (uint8_t)'+';
                for (uint32_t j = 0; j < c; j++) o[w++] = (uint8_t)"acgt"[read_code(sq, st.q + j)];
            }
            st.q += c;
        } else {
            const bool open = st.prev != 'D';
            n = lead + (open ? 1u : 0u) + c;
            if (WRITE) {
                if (open) o[w++] = (uint8_t)'-';
                for (uint32_t j = 0; j < c; j++) o[w++] = (uint8_t)"acgt"[fwd_text_code(sq, st.t + j)];
            }
            st.t += c;
        }
        st.pend = 0;
    }
    st.prev = op;
    return n;
}

// what follows the last run (without the NUL)
template <bool WRITE> __device__ __forceinline__ uint32_t emit_tail(int32_t kind, const DiffState& st, uint8_t* o)
{
    if (kind == SCRG_DIFF_MD) return WRITE ? put_num(o, st.pend) : num_digits(st.pend);
    if (!st.pend) return 0u;
    if (WRITE) {
        o[0] = (uint8_t)':';
        put_num(o + 1, st.pend);
    }
    return 1u + num_digits(st.pend);
}

// a pair's runs may consume no more than its sequences hold (and no more than 2^32 - 1 text bases: what an alignment can reach)
__device__ __forceinline__ bool consumed_ok(const DiffState& st, uint64_t text_len, uint64_t read_len)
{
    return st.t <= text_len && st.q <= read_len && st.t <= 0xffffffffull && st.q <= 0xffffffffull;
}

struct DiffArgs {
    PairRuns pr;
    int32_t kind;
    uint64_t* len;                // length pass: out; render pass: in
    const uint64_t* off;          // render pass
    uint8_t* text;
    uint64_t capacity;
    uint32_t* bad;
};

struct DiffPair {                 // a pair as a kernel takes it
    uint64_t cnt, src;            // runs, first run
    bool desc_ok;                 // no strand bit the kernels do not serve
    PairSeq sq;
};

__device__ __forceinline__ void load_pair(DiffPair& d, const PairRuns& a, uint64_t p)
{
    run_slice(a.run_off, a.run_off_stride, a.n_runs, p, d.cnt, d.src);
    d.sq = pair_seq(a, a.pairs[p]);
    d.desc_ok = !d.sq.text_rev && (!d.sq.read_rev || a.stranded);
}

// ---------------------------------------------------------------------------------------------------------------
// one pair per lane: a serial walk.  Returns the length incl. the NUL; *ok: the pair is valid (else the length is 1).
// ---------------------------------------------------------------------------------------------------------------
template <bool WRITE> __device__ __forceinline__ uint64_t walk_lane(int32_t kind, const DiffPair& d, const uint16_t* __restrict__ runs, uint8_t* o, bool* ok)
{
    DiffState st{};
    const uint16_t* const s = runs + d.src;
    uint64_t n = 0;
    bool good = d.desc_ok;
    for (uint64_t k = 0; k < d.cnt; k++) {
        const uint32_t r = s[k];
        if (!run_ok(r)) { good = false; break; }
        if (WRITE) n += emit_run<true>(kind, r, st, o + n, d.sq);
        else n += emit_run<false>(kind, r, st, nullptr, d.sq);
    }
    if (!WRITE) good = good && consumed_ok(st, d.sq.text_len, d.sq.read_len);        // (a render walks a pair only after its measuring walk)
    *ok = good;
    if (!good) return 1;
    if (d.cnt == 0) {                     // a pair without runs: "" in both kinds (no "0")
        if (WRITE) o[0] = 0;
        return 1;
    }
    n += WRITE ? emit_tail<true>(kind, st, o + n) : emit_tail<false>(kind, st, nullptr);
    if (WRITE) o[n] = 0;
    return n + 1;
}

// ---------------------------------------------------------------------------------------------------------------
// one wavefront per pair: tiles of 512 runs, eight per lane.  All 64 lanes call it with the same pair.
//   WRITE = false: the length incl. the NUL and *ok as above (nothing is read but the runs).
//   WRITE = true : the pair is valid; its bytes go to out[0 ..) — a tile's through `tile` (LDS) as contiguous bytes unless it has
//                  more than DIFF_TILE_BYTES (long X / I / D runs), when the lanes store their pieces themselves.
// ---------------------------------------------------------------------------------------------------------------
template <bool WRITE> __device__ __forceinline__ uint64_t walk_wave(int32_t kind, const DiffPair& d, const uint16_t* __restrict__ runs, uint8_t* out,
                                                                    uint8_t* tile, uint32_t lane, bool* ok)
{
    const uint16_t* const s = runs + d.src;
    DiffState carry{};                            // the state after the tiles so far (wavefront-uniform)
    uint64_t total = 0;
    bool bad_run = false;
    for (uint64_t t0 = 0; t0 < d.cnt; t0 += WALK_TILE_RUNS) {
        // my eight runs, the positions in front of them and the operation before them; and what my runs leave pending
        uint32_t tail = 0;
        bool reset = false;
        RunTile x = load_tile(s, d.cnt, t0, lane, carry, [&](uint32_t& run) {
            if (!run_ok(run)) { bad_run = true; run = (uint32_t)'I' << 8; }      // (counted as nothing; the pair is dropped below)
            const uint32_t c = run & 0xffu, op = run >> 8;
            if (run_resets(kind, op)) { reset = true; tail = 0; }
            else if (op == '=') tail += c;
        });
        uint32_t (&r)[WALK_LANE_RUNS] = x.r;
        const uint32_t mine = x.mine;
        // the pending count: a segmented sum over the lanes — a lane with a reset starts it again
        uint32_t seg_v = tail, seg_f = reset ? 1u : 0u;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t vv = (uint32_t)__shfl_up((int)seg_v, dd, 64), vf = (uint32_t)__shfl_up((int)seg_f, dd, 64);
            if (lane >= (uint32_t)dd) {
                if (!seg_f) seg_v += vv;
                seg_f |= vf;
            }
        }
        // exclusive: what the lanes before me leave
        uint32_t ex_v = (uint32_t)__shfl_up((int)seg_v, 1, 64), ex_f = (uint32_t)__shfl_up((int)seg_f, 1, 64);
        if (lane == 0) { ex_v = 0; ex_f = 0; }
        DiffState st;
        static_cast<WalkPos&>(st) = x.at;
        st.pend = ex_f ? ex_v : carry.pend + ex_v;
        // the tile's state after its last lane, for the next tile
        const uint32_t end_v = (uint32_t)__shfl((int)seg_v, 63, 64), end_f = (uint32_t)__shfl((int)seg_f, 63, 64);
        // my bytes, and where they go
        uint32_t bytes = 0;
        {
            DiffState m = st;
#pragma unroll
            for (uint32_t k = 0; k < WALK_LANE_RUNS; k++)
                if (k < mine) bytes += emit_run<false>(kind, r[k], m, nullptr, d.sq);
        }
        const uint32_t incl = wave_scan_incl(bytes, lane);
        const uint32_t tile_bytes = (uint32_t)__shfl((int)incl, 63, 64);
        if (WRITE) {
            const bool staged = tile_bytes <= DIFF_TILE_BYTES;
            if (staged) {                 // (two copies of the loop: one stores to LDS, the other to memory)
                uint8_t* o = tile + (incl - bytes);
#pragma unroll
                for (uint32_t k = 0; k < WALK_LANE_RUNS; k++)
                    if (k < mine) o += emit_run<true>(kind, r[k], st, o, d.sq);
            } else {
                uint8_t* o = out + total + (incl - bytes);
#pragma unroll
                for (uint32_t k = 0; k < WALK_LANE_RUNS; k++)
                    if (k < mine) o += emit_run<true>(kind, r[k], st, o, d.sq);
            }
            if (staged) flush_tile(out + total, tile, tile_bytes, lane);
        }
        total += tile_bytes;
        carry.pend = end_f ? end_v : carry.pend + end_v;
        move_past(carry, x);
    }
    bool good = d.desc_ok;
    if (!WRITE) good = good && __ballot(bad_run) == 0ull && consumed_ok(carry, d.sq.text_len, d.sq.read_len);
    *ok = good;
    if (!good) return 1;
    if (WRITE) {
        if (lane == 0) {
            const uint32_t n = emit_tail<true>(kind, carry, out + total);
            out[total + n] = 0;
        }
    }
    return total + emit_tail<false>(kind, carry, nullptr) + 1u;
}

// ---------------------------------------------------------------------------------------------------------------
// pass 1: every pair's length incl. the NUL (1 for a pair whose runs do not fit its sequences)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diff_len_kernel(DiffArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    for_each_group<DiffPair>(
        a.pr.n, split, [&](DiffPair& me, uint64_t p, uint32_t) { load_pair(me, a.pr, p); },
        [&](const DiffPair& me, uint64_t p) {
            bool ok;
            a.len[p] = walk_lane<false>(a.kind, me, a.pr.runs, nullptr, &ok);
        },
        [&](const DiffPair&, uint64_t g0, uint32_t q, uint32_t lane) {
            DiffPair dq;
            load_pair(dq, a.pr, g0 + q);
            bool ok;
            const uint64_t len = walk_wave<false>(a.kind, dq, a.pr.runs, nullptr, nullptr, lane, &ok);
            if (lane == 0) a.len[g0 + q] = len;
        },
        NothingAfter());
}

// ---------------------------------------------------------------------------------------------------------------
// pass 2: the bytes, NUL-terminated, at off[p].  A pair is measured again first (its runs only): lengths and offsets may come off
// a wire, and nothing is written for a pair whose segment [off, off + len) is not inside [0, capacity) or whose len is not the
// length of its string — both are counted in *bad, as is a pair whose runs do not fit its sequences (its string is "").
// ---------------------------------------------------------------------------------------------------------------
struct DiffRenderPair : DiffPair {
    uint64_t len, off;            // what the caller says of its string
    bool seg_ok;                  // that segment is inside the buffer
    uint32_t bad;                 // the pair is counted in *bad
};

__global__ __launch_bounds__(256) void diff_render_kernel(DiffArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    __shared__ __attribute__((aligned(16))) uint8_t tile_all[4][DIFF_TILE_BYTES];
    uint8_t* const tile = tile_all[threadIdx.x >> 6];
    for_each_group<DiffRenderPair>(
        a.pr.n, split,
        [&](DiffRenderPair& me, uint64_t p, uint32_t) {
            load_pair(me, a.pr, p);
            me.len = a.len[p];
            me.off = a.off[p];
            me.seg_ok = me.len >= 1 && me.off <= a.capacity && me.len <= a.capacity - me.off;
        },
        [&](DiffRenderPair& me, uint64_t) {
            bool ok;
            const uint64_t len = walk_lane<false>(a.kind, me, a.pr.runs, nullptr, &ok);
            if (!ok || !me.seg_ok || len != me.len) me.bad = 1;
            if (me.seg_ok && len == me.len) {
                if (ok) walk_lane<true>(a.kind, me, a.pr.runs, a.text + me.off, &ok);
                else a.text[me.off] = 0;
            }
        },
        [&](DiffRenderPair& me, uint64_t g0, uint32_t q, uint32_t lane) {
            DiffPair dq;
            load_pair(dq, a.pr, g0 + q);
            const uint64_t q_len = __shfl(me.len, (int)q, 64), q_off = __shfl(me.off, (int)q, 64);
            const bool q_seg = __shfl((int)me.seg_ok, (int)q, 64) != 0;
            bool ok;
            const uint64_t len = walk_wave<false>(a.kind, dq, a.pr.runs, nullptr, nullptr, lane, &ok);
            if (lane == q && (!ok || !q_seg || len != q_len)) me.bad = 1;
            if (q_seg && len == q_len) {
                if (ok) walk_wave<true>(a.kind, dq, a.pr.runs, a.text + q_off, tile, lane, &ok);
                else if (lane == 0) a.text[q_off] = 0;
            }
        },
        [&](const DiffRenderPair& me, uint32_t lane) {
            const uint32_t n_bad = (uint32_t)__popcll(__ballot(me.bad != 0));
            if (n_bad && lane == 0) atomicAdd(a.bad, n_bad);
        });
}

// ---------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------
hipError_t launch_diff_lengths(const PairRuns& pr, int32_t kind, uint64_t* len, int n_cus, hipStream_t s)
{
    if (pr.n == 0) return hipSuccess;
    DiffArgs a{};
    a.pr = pr;
    a.kind = kind;
    a.len = len;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(pr.n, n_cus, &split);
    hipLaunchKernelGGL(diff_len_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    return hipGetLastError();
}

hipError_t launch_diff_render(const PairRuns& pr, int32_t kind, const uint64_t* len, const uint64_t* off, uint8_t* text, uint64_t capacity,
                              uint32_t* bad, int n_cus, hipStream_t s)
{
    if (pr.n == 0) return hipSuccess;
    DiffArgs a{};
    a.pr = pr;
    a.kind = kind;
    a.len = const_cast<uint64_t*>(len);
    a.off = off;
    a.text = text;
    a.capacity = capacity;
    a.bad = bad;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(pr.n, n_cus, &split);
    hipLaunchKernelGGL(diff_render_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    return hipGetLastError();
}

// the host path's offsets: off[0 .. n] = exclusive sums of len[0 .. n), the total in off[n] (len has room for the zero at [n])
hipError_t launch_diff_offsets(uint64_t n, uint64_t* len, uint64_t* off, void* temp, size_t temp_bytes, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(len + n, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, len, off, (int)(n + 1), s);
}

}  // namespace scrg
