// diff_kernels.hip — difference strings (SAM's MD:Z: and PAF's short cs:Z:) of every pair, from its runs and the two packed
// sequences: a length pass and a render pass with offsets by prefix sum between them, as text_len_kernel / render_text_kernel
// (host_path_kernels.hip) do it for the CIGAR text.  HBM-bound helpers: a pair's runs are read once per pass and a few
// sequence words per edit besides.
//
// The string of a pair is the concatenation of what its runs emit, in order, then a tail and a NUL:
//   MD  '=' nothing;  'X' per base: the number of '=' bases pending (0 after the first), the TEXT base;  'D' the pending number and
//       '^' unless the run before it was a 'D', then its text bases;  'I' nothing (and the pending count stays);  tail: the number.
//   cs  '=' nothing;  'X' ":n" if n '=' bases are pending, then "*tq" per base;  'I' / 'D' ":n" likewise, '+' / '-' unless the
//       run before it had the same operation, then the read / text bases;  tail: ":n" if n are pending.
// So a run's bytes depend on three things that come from the runs before it: the pending '=' count (a SEGMENTED sum: it starts
// again after every run that emits it — X, D and for cs I), the operation of the run before it, and its text and read positions
// (prefix sums).  One pair per lane walks them serially; one wavefront per pair gets them for 512 runs at a time from wavefront
// scans over the lanes' eight runs each, and carries them from tile to tile.  A pair without runs has "" in both kinds.
#include <hipcub/hipcub.hpp>

#include "genasm_kernels.h"
#include "host_path.h"

namespace scrg {

// the thresholds the tests name (tests/test_diff_strings.py walks both neighbours of each)
constexpr uint32_t DIFF_LANE_MAX_RUNS = 24;       // up to this many runs: one pair per lane; more: one wavefront per pair
constexpr uint32_t DIFF_LANE_RUNS = 8;            // runs per lane and tile
constexpr uint32_t DIFF_TILE_RUNS = 64 * DIFF_LANE_RUNS;       // 512
constexpr uint32_t DIFF_TILE_BYTES = 4096;        // LDS staging per wavefront; a tile with more bytes (long X runs) goes straight to memory

struct DiffSeq {                  // where a pair's bases are (scrg_pair_desc, scrg_params)
    const uint64_t* seq;
    uint64_t text_off, read_off, read_len;
    uint32_t text_stride, read_stride, read_rev;
};

// base k of a sequence with offset `off` and word stride s: word off / 32 + ((off % 32 + k) / 32) * s, bit (off + k) % 32 of each plane
__device__ __forceinline__ uint32_t base_code(const uint64_t* __restrict__ seq, uint64_t off, uint32_t stride, uint64_t k)
{
    const uint64_t pos = (off & 31ull) + k;
    const uint64_t w = seq[(off >> 5) + (pos >> 5) * stride];
    const uint32_t b = (uint32_t)pos & 31u;
    return (uint32_t)((w >> b) & 1ull) | ((uint32_t)((w >> (32u + b)) & 1ull) << 1);
}
__device__ __forceinline__ uint32_t text_code(const DiffSeq& s, uint64_t t) { return base_code(s.seq, s.text_off, s.text_stride, t); }
// (the read as aligned: on the minus strand base q is the complement of packed base read_len - 1 - q)
__device__ __forceinline__ uint32_t read_code(const DiffSeq& s, uint64_t q)
{
    return s.read_rev ? 3u - base_code(s.seq, s.read_off, s.read_stride, s.read_len - 1ull - q) : base_code(s.seq, s.read_off, s.read_stride, q);
}

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

struct DiffState {                // what a run needs to know of the runs before it
    uint32_t pend;                // '=' bases since the last run that emitted the count
    uint32_t prev;                // the operation of the run before (0: none)
    uint64_t t, q;                // text and read positions
};

__device__ __forceinline__ bool run_ok(uint32_t run)
{
    const uint32_t op = run >> 8;
    return (run & 0xffu) != 0u && (op == '=' || op == 'X' || op == 'I' || op == 'D');
}
// does the run emit (and so clear) the pending count?
__device__ __forceinline__ bool run_resets(int32_t kind, uint32_t op) { return op == 'X' || op == 'D' || (kind == SCRG_DIFF_CS && op == 'I'); }

// One run: its bytes (written at o if WRITE), the state moved past it.  The run is valid (run_ok).
template <bool WRITE> __device__ __forceinline__ uint32_t emit_run(int32_t kind, uint32_t run, DiffState& st, uint8_t* o, const DiffSeq& sq)
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
                o[w++] = (uint8_t)"ACGT"[text_code(sq, st.t)];
                for (uint32_t j = 1; j < c; j++) {
                    o[w++] = (uint8_t)'0';
                    o[w++] = (uint8_t)"ACGT"[text_code(sq, st.t + j)];
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
                for (uint32_t j = 0; j < c; j++) o[w++] = (uint8_t)"ACGT"[text_code(sq, st.t + j)];
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
                    o[w++] = (uint8_t)"acgt"[text_code(sq, st.t + j)];
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
                for (uint32_t j = 0; j < c; j++) o[w++] = (uint8_t)"acgt"[text_code(sq, st.t + j)];
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

struct DiffPair {                 // a pair as a kernel takes it
    uint64_t cnt, src;            // runs, first run
    uint64_t text_len;
    bool desc_ok;                 // no strand bit the kernels do not serve
    DiffSeq sq;
};

__device__ __forceinline__ DiffPair load_pair(uint64_t p, const uint64_t* __restrict__ seq, const scrg_pair_desc* __restrict__ pairs,
                                              const uint64_t* __restrict__ run_off, uint64_t run_off_stride, const uint32_t* __restrict__ n_runs,
                                              uint32_t text_stride, uint32_t read_stride, uint32_t stranded)
{
    DiffPair d;
    const scrg_pair_desc pd = pairs[p];
    d.cnt = n_runs[p];
    d.src = run_off[p * run_off_stride];
    // (the slices as scrg_align_device left them: the offsets are the descriptors' cigar_off, the count is capped at cigar_cap)
    if (run_off_stride == 6) d.cnt = d.cnt > run_off[p * 6 + 1] ? run_off[p * 6 + 1] : d.cnt;
    d.text_len = pd.text_len;
    const bool rrev = (pd.read_off & SCRG_READ_REVCOMP) != 0;
    d.desc_ok = !(pd.text_off & SCRG_TEXT_REVCOMP) && (!rrev || stranded);
    d.sq.seq = seq;
    d.sq.text_off = pd.text_off & ~SCRG_TEXT_REVCOMP;
    d.sq.read_off = pd.read_off & ~SCRG_READ_REVCOMP;
    d.sq.read_len = pd.read_len;
    d.sq.text_stride = text_stride;
    d.sq.read_stride = read_stride;
    d.sq.read_rev = rrev ? 1u : 0u;
    return d;
}

// ---------------------------------------------------------------------------------------------------------------
// one pair per lane: a serial walk.  Returns the length incl. the NUL; *ok: the pair is valid (else the length is 1).
// ---------------------------------------------------------------------------------------------------------------
template <bool WRITE> __device__ __forceinline__ uint64_t walk_lane(int32_t kind, const DiffPair& d, const uint16_t* __restrict__ runs, uint8_t* o, bool* ok)
{
    DiffState st{0u, 0u, 0ull, 0ull};
    const uint16_t* const s = runs + d.src;
    uint64_t n = 0;
    bool good = d.desc_ok;
    for (uint64_t k = 0; k < d.cnt; k++) {
        const uint32_t r = s[k];
        if (!run_ok(r)) { good = false; break; }
        if (WRITE) n += emit_run<true>(kind, r, st, o + n, d.sq);
        else n += emit_run<false>(kind, r, st, nullptr, d.sq);
    }
    if (!WRITE) good = good && consumed_ok(st, d.text_len, d.sq.read_len);        // (a render walks a pair only after its measuring walk)
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
    DiffState carry{0u, 0u, 0ull, 0ull};          // the state after the tiles so far (wavefront-uniform)
    uint64_t total = 0;
    bool bad_run = false;
    for (uint64_t t0 = 0; t0 < d.cnt; t0 += DIFF_TILE_RUNS) {
        // my eight runs (the dense array is only 2-byte aligned: plain loads) and what they add up to
        uint32_t r[DIFF_LANE_RUNS], mine = 0;
        uint32_t sum_t = 0, sum_q = 0, tail = 0, last_op = 0;
        bool reset = false;
#pragma unroll
        for (uint32_t k = 0; k < DIFF_LANE_RUNS; k++) {
            const uint64_t idx = t0 + DIFF_LANE_RUNS * lane + k;
            r[k] = idx < d.cnt ? s[idx] : 0u;
            if (idx >= d.cnt) continue;
            mine = k + 1;
            if (!run_ok(r[k])) { bad_run = true; r[k] = (uint32_t)'I' << 8; }      // (counted as nothing; the pair is dropped below)
            const uint32_t c = r[k] & 0xffu, op = r[k] >> 8;
            if (op != 'I') sum_t += c;
            if (op != 'D') sum_q += c;
            if (run_resets(kind, op)) { reset = true; tail = 0; }
            else if (op == '=') tail += c;
            last_op = op;
        }
        // wavefront scans: text and read positions (sums), the pending count (a segmented sum: a lane with a reset starts it again)
        uint32_t in_t = sum_t, in_q = sum_q, seg_v = tail, seg_f = reset ? 1u : 0u;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t vt = (uint32_t)__shfl_up((int)in_t, dd, 64), vq = (uint32_t)__shfl_up((int)in_q, dd, 64);
            const uint32_t vv = (uint32_t)__shfl_up((int)seg_v, dd, 64), vf = (uint32_t)__shfl_up((int)seg_f, dd, 64);
            if (lane >= (uint32_t)dd) {
                in_t += vt;
                in_q += vq;
                if (!seg_f) seg_v += vv;
                seg_f |= vf;
            }
        }
        // exclusive: what the lanes before me leave
        uint32_t ex_v = (uint32_t)__shfl_up((int)seg_v, 1, 64), ex_f = (uint32_t)__shfl_up((int)seg_f, 1, 64);
        uint32_t ex_op = (uint32_t)__shfl_up((int)last_op, 1, 64);
        if (lane == 0) { ex_v = 0; ex_f = 0; ex_op = carry.prev; }
        DiffState st;
        st.pend = ex_f ? ex_v : carry.pend + ex_v;
        st.prev = ex_op;
        st.t = carry.t + (in_t - sum_t);
        st.q = carry.q + (in_q - sum_q);
        // the tile's state after its last lane, for the next tile
        const uint32_t runs_here = (uint32_t)(d.cnt - t0 < DIFF_TILE_RUNS ? d.cnt - t0 : DIFF_TILE_RUNS);
        const uint32_t end_v = (uint32_t)__shfl((int)seg_v, 63, 64), end_f = (uint32_t)__shfl((int)seg_f, 63, 64);
        const uint32_t end_t = (uint32_t)__shfl((int)in_t, 63, 64), end_q = (uint32_t)__shfl((int)in_q, 63, 64);
        const uint32_t end_op = (uint32_t)__shfl((int)last_op, (int)((runs_here - 1u) / DIFF_LANE_RUNS), 64);
        // my bytes, and where they go
        uint32_t bytes = 0;
        {
            DiffState m = st;
#pragma unroll
            for (uint32_t k = 0; k < DIFF_LANE_RUNS; k++)
                if (k < mine) bytes += emit_run<false>(kind, r[k], m, nullptr, d.sq);
        }
        uint32_t incl = bytes;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, dd, 64);
            if (lane >= (uint32_t)dd) incl += v;
        }
        const uint32_t tile_bytes = (uint32_t)__shfl((int)incl, 63, 64);
        if (WRITE) {
            const bool staged = tile_bytes <= DIFF_TILE_BYTES;
            if (staged) {                 // (two copies of the loop: one stores to LDS, the other to memory)
                uint8_t* o = tile + (incl - bytes);
#pragma unroll
                for (uint32_t k = 0; k < DIFF_LANE_RUNS; k++)
                    if (k < mine) o += emit_run<true>(kind, r[k], st, o, d.sq);
            } else {
                uint8_t* o = out + total + (incl - bytes);
#pragma unroll
                for (uint32_t k = 0; k < DIFF_LANE_RUNS; k++)
                    if (k < mine) o += emit_run<true>(kind, r[k], st, o, d.sq);
            }
            if (staged) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                uint8_t* const dst = out + total;
                for (uint32_t b = lane; b < tile_bytes; b += 64) dst[b] = tile[b];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        total += tile_bytes;
        carry.pend = end_f ? end_v : carry.pend + end_v;
        carry.prev = end_op;
        carry.t += end_t;
        carry.q += end_q;
    }
    bool good = d.desc_ok;
    if (!WRITE) good = good && __ballot(bad_run) == 0ull && consumed_ok(carry, d.text_len, d.sq.read_len);
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

struct DiffArgs {
    uint64_t n;
    int32_t kind;
    const uint64_t* seq;
    const scrg_pair_desc* pairs;
    const uint16_t* runs;
    const uint64_t* run_off;
    uint64_t run_off_stride;
    const uint32_t* n_runs;
    uint32_t text_stride, read_stride, stranded;
    uint64_t* len;                // length pass: out; render pass: in
    const uint64_t* off;          // render pass
    uint8_t* text;
    uint64_t capacity;
    uint32_t* bad;
};

// ---------------------------------------------------------------------------------------------------------------
// pass 1: every pair's length incl. the NUL (1 for a pair whose runs do not fit its sequences)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diff_len_kernel(DiffArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    // pairs are taken 64 at a time; `split` wavefronts share a group of 64 (each takes every split-th long pair of it)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave_all = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t wave = wave_all / split, n_waves = (((uint64_t)gridDim.x * blockDim.x) >> 6) / split;
    const uint32_t sub = (uint32_t)(wave_all % split);
    if (wave >= n_waves) return;                       // (the grid is rounded up to whole workgroups)
    for (uint64_t g0 = wave * 64; g0 < a.n; g0 += n_waves * 64) {
        const uint64_t mine = g0 + lane;
        DiffPair d{};
        if (mine < a.n) d = load_pair(mine, a.seq, a.pairs, a.run_off, a.run_off_stride, a.n_runs, a.text_stride, a.read_stride, a.stranded);
        const bool big_me = d.cnt > DIFF_LANE_MAX_RUNS;
        if (mine < a.n && sub == 0 && !big_me) {
            bool ok;
            a.len[mine] = walk_lane<false>(a.kind, d, a.runs, nullptr, &ok);
        }
        uint64_t big = __ballot(big_me);
        for (uint32_t ord = 0; big != 0; ord++) {
            const uint32_t q = (uint32_t)__builtin_ctzll(big);
            big &= big - 1;
            if (ord % split != sub) continue;
            const DiffPair dq = load_pair(g0 + q, a.seq, a.pairs, a.run_off, a.run_off_stride, a.n_runs, a.text_stride, a.read_stride, a.stranded);
            bool ok;
            const uint64_t len = walk_wave<false>(a.kind, dq, a.runs, nullptr, nullptr, lane, &ok);
            if (lane == 0) a.len[g0 + q] = len;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// pass 2: the bytes, NUL-terminated, at off[p].  A pair is measured again first (its runs only): lengths and offsets may come off
// a wire, and nothing is written for a pair whose segment [off, off + len) is not inside [0, capacity) or whose len is not the
// length of its string — both are counted in *bad, as is a pair whose runs do not fit its sequences (its string is "").
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diff_render_kernel(DiffArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    __shared__ __attribute__((aligned(16))) uint8_t tile_all[4][DIFF_TILE_BYTES];
    const uint32_t lane = threadIdx.x & 63u;
    uint8_t* const tile = tile_all[threadIdx.x >> 6];
    const uint64_t wave_all = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t wave = wave_all / split, n_waves = (((uint64_t)gridDim.x * blockDim.x) >> 6) / split;
    const uint32_t sub = (uint32_t)(wave_all % split);
    if (wave >= n_waves) return;                       // (the grid is rounded up to whole workgroups)
    for (uint64_t g0 = wave * 64; g0 < a.n; g0 += n_waves * 64) {
        const uint64_t mine = g0 + lane;
        DiffPair d{};
        uint64_t my_len = 0, my_off = 0;
        bool seg_ok = false;
        if (mine < a.n) {
            d = load_pair(mine, a.seq, a.pairs, a.run_off, a.run_off_stride, a.n_runs, a.text_stride, a.read_stride, a.stranded);
            my_len = a.len[mine];
            my_off = a.off[mine];
            seg_ok = my_len >= 1 && my_off <= a.capacity && my_len <= a.capacity - my_off;
        }
        const bool big_me = d.cnt > DIFF_LANE_MAX_RUNS;
        uint32_t bad = 0;
        if (mine < a.n && sub == 0 && !big_me) {
            bool ok;
            const uint64_t len = walk_lane<false>(a.kind, d, a.runs, nullptr, &ok);
            if (!ok || !seg_ok || len != my_len) bad = 1;
            if (seg_ok && len == my_len) {
                if (ok) walk_lane<true>(a.kind, d, a.runs, a.text + my_off, &ok);
                else a.text[my_off] = 0;
            }
        }
        uint64_t big = __ballot(big_me);
        for (uint32_t ord = 0; big != 0; ord++) {
            const uint32_t q = (uint32_t)__builtin_ctzll(big);
            big &= big - 1;
            if (ord % split != sub) continue;
            const DiffPair dq = load_pair(g0 + q, a.seq, a.pairs, a.run_off, a.run_off_stride, a.n_runs, a.text_stride, a.read_stride, a.stranded);
            const uint64_t q_len = __shfl(my_len, (int)q, 64), q_off = __shfl(my_off, (int)q, 64);
            const bool q_seg = __shfl((int)seg_ok, (int)q, 64) != 0;
            bool ok;
            const uint64_t len = walk_wave<false>(a.kind, dq, a.runs, nullptr, nullptr, lane, &ok);
            if (lane == q && (!ok || !q_seg || len != q_len)) bad = 1;
            if (q_seg && len == q_len) {
                if (ok) walk_wave<true>(a.kind, dq, a.runs, a.text + q_off, tile, lane, &ok);
                else if (lane == 0) a.text[q_off] = 0;
            }
        }
        const uint32_t n_bad = (uint32_t)__popcll(__ballot(bad != 0));
        if (n_bad && lane == 0) atomicAdd(a.bad, n_bad);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------
// (as host_path_kernels.hip: workgroups of four wavefronts, about sixteen wavefronts per CU; a batch with fewer groups of 64 pairs
// than that lets `split` wavefronts share a group)
static uint64_t diff_grid(uint64_t n, int n_cus, uint32_t* split)
{
    const uint64_t groups = (n + 63) / 64, target_waves = (uint64_t)n_cus * 16;
    uint64_t sp = 1;
    while (sp < 64 && groups * sp * 2 <= target_waves) sp *= 2;
    uint64_t waves = groups * sp;
    if (waves > target_waves * 2) waves = target_waves * 2 / sp * sp;       // (whole sets of `split` wavefronts)
    *split = (uint32_t)sp;
    return (waves + 3) / 4;
}

static DiffArgs diff_args(int32_t kind, uint64_t n, const uint64_t* seq, const scrg_pair_desc* pairs, const uint16_t* runs, const uint64_t* run_off,
                          uint64_t run_off_stride, const uint32_t* n_runs, uint32_t text_stride, uint32_t read_stride, uint32_t stranded)
{
    DiffArgs a{};
    a.n = n;
    a.kind = kind;
    a.seq = seq;
    a.pairs = pairs;
    a.runs = runs;
    a.run_off = run_off;
    a.run_off_stride = run_off_stride;
    a.n_runs = n_runs;
    a.text_stride = text_stride;
    a.read_stride = read_stride;
    a.stranded = stranded;
    return a;
}

hipError_t launch_diff_lengths(int32_t kind, uint64_t n, const uint64_t* seq, const scrg_pair_desc* pairs, const uint16_t* runs,
                               const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs, uint32_t text_stride,
                               uint32_t read_stride, uint32_t stranded, uint64_t* len, int n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    DiffArgs a = diff_args(kind, n, seq, pairs, runs, run_off, run_off_stride, n_runs, text_stride, read_stride, stranded);
    a.len = len;
    uint32_t split = 1;
    const uint64_t blocks = diff_grid(n, n_cus, &split);
    hipLaunchKernelGGL(diff_len_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    return hipGetLastError();
}

hipError_t launch_diff_render(int32_t kind, uint64_t n, const uint64_t* seq, const scrg_pair_desc* pairs, const uint16_t* runs,
                              const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs, uint32_t text_stride,
                              uint32_t read_stride, uint32_t stranded, const uint64_t* len, const uint64_t* off, uint8_t* text,
                              uint64_t capacity, uint32_t* bad, int n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    DiffArgs a = diff_args(kind, n, seq, pairs, runs, run_off, run_off_stride, n_runs, text_stride, read_stride, stranded);
    a.len = const_cast<uint64_t*>(len);
    a.off = off;
    a.text = text;
    a.capacity = capacity;
    a.bad = bad;
    uint32_t split = 1;
    const uint64_t blocks = diff_grid(n, n_cus, &split);
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
