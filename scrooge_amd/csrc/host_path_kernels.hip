// host_path_kernels.hip — the small kernels of the pipelined host-pointer path (scrg_host.cpp): problem descriptors
// built on the device from a few bytes per pair, per-pair CIGAR text lengths, offsets by prefix sum (hipCUB), and the
// "%d%c" rendering of the runs (src/genasm_cpu.cpp:387-403 produces that text on the host, one sprintf per run).
// All HBM-bound helpers: the work of the path is genasm_lane_kernel.
#include <hipcub/hipcub.hpp>

#include "genasm_kernels.h"
#include "host_path.h"
#include "run_walk.h"

namespace scrg {

// ---------------------------------------------------------------------------------------------------------------
// descriptors.  Pair i of a chunk (issue order).  Reads live in lane-interleaved groups of 64 rows (stride 64 words):
// row r starts at word read_base + (r / 64) * read_words * 64 + r % 64.
//   pairwise: the text of pair i is row i of a second such region (text_base, text_words);
//   mapping : the text is the packed genome at word 0 of the sequence array, from base start[i] to its end
//             (src/genasm_cpu.cpp:512-514) — a leftward candidate's (ROW_LEFTWARD): the reverse complement of the genome up to start[i]; the read row of pair i is row[i] (candidates of one read share a row).
// Every pair gets a slice of `cap` runs (a multiple of 16) at i * cap.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void build_desc_kernel(HostDescArgs a)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    scrg_pair_desc d;
    const uint32_t row_word = a.row ? a.row[i] : 0u;
    const uint64_t row = a.row ? row_word & ROW_INDEX_MASK : i;
    d.read_off = a.linear ? 32ull * (a.read_base + row * a.read_words) : 32ull * (a.read_base + (row >> 6) * a.read_words * 64ull + (row & 63ull));
    if (row_word & ROW_REVERSE) d.read_off |= SCRG_READ_REVCOMP;
    d.read_len = a.read_len[i];
    if (a.start) {
        const uint64_t st = a.start[i];
        d.text_off = st;
        d.text_len = a.genome_len - st;
        if (row_word & ROW_LEFTWARD) {          // leftward from st: the reverse complement of genome[0, st)
            d.text_off = 0ull | SCRG_TEXT_REVCOMP;
            d.text_len = st;
        }
    } else {
        d.text_off = a.linear ? 32ull * (a.text_base + i * a.text_words) : 32ull * (a.text_base + (i >> 6) * a.text_words * 64ull + (i & 63ull));
        d.text_len = a.text_len[i];
    }
    d.cigar_off = i * a.cap;
    d.cigar_cap = a.cap;
    a.desc[i] = d;
}

// ---------------------------------------------------------------------------------------------------------------
// per pair: run count (capped at the slice) and the length of its CIGAR text incl. the terminating NUL, as uint64 for
// the scans.  Long alignments: one wavefront per pair over the pair's slice; short ones: one pair per lane (run_walk.h:
// for_each_group).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t run_chars(uint32_t run)        // digits of the count + the op character
{
    const uint32_t c = run & 0xffu;
    return 2u + (c >= 10u ? 1u : 0u) + (c >= 100u ? 1u : 0u);
}

struct TextRec {                  // a pair's runs (text_len_kernel: in its slice; render_text_kernel: dense) and where its text goes
    uint64_t cnt, src, dst;
};

// ---------------------------------------------------------------------------------------------------------------
// The forms of the text (scrooge_amd.h, CIGAR FORMS).  A run has a class: its operation, or under SCRG_CIGAR_M 'M' for '=' and
// 'X'.  The text is written per STRETCH — a maximal sequence of directly adjacent runs of one class: the decimal sum of their
// counts (64 bits) and the class letter.  Under SCRG_CIGAR_WINDOWED no two runs share a stretch, which is "%d%c" per run.
// A stretch is never longer than the windowed text of its runs (the digits of a sum are no more than the digits of its terms
// together, and a letter goes for every run joined), so what the pipeline sizes by run counts holds for every form.
// One pair per lane: a serial walk with the open stretch.  One wavefront per pair: per tile of 512 runs a segmented scan over
// the lanes gives the sum of the open stretch in front of each lane; a stretch is written by the lane that sees it close (the
// lane of the first run of another class), the open stretch is carried from tile to tile, and the last one is written after
// the last tile.  The walks print what the runs hold and never stop; *ok says whether every run was one (run_ok).
// ---------------------------------------------------------------------------------------------------------------
template <int FORM> __device__ __forceinline__ uint32_t run_class(uint32_t op)
{
    return (FORM == SCRG_CIGAR_M && (op == '=' || op == 'X')) ? (uint32_t)'M' : op;
}
template <int FORM> __device__ __forceinline__ bool same_stretch(uint32_t cls_a, uint32_t cls_b) { return FORM != SCRG_CIGAR_WINDOWED && cls_a == cls_b; }

// a stretch's bytes: the digits of its sum and its class (written at o if WRITE)
template <bool WRITE> __device__ __forceinline__ uint32_t put_stretch(uint8_t* o, uint64_t sum, uint32_t cls)
{
    uint32_t d = 1;
    if (sum <= 0xffffffffull) {           // (nearly always: 32-bit divisions)
        uint32_t v = (uint32_t)sum;
        for (uint32_t w = v; w >= 10u; w /= 10u) d++;
        if (WRITE)
            for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + v % 10u); v /= 10u; }
    } else {
        for (uint64_t w = sum; w >= 10ull; w /= 10ull) d++;
        if (WRITE)
            for (uint32_t k = d; k-- > 0;) { o[k] = (uint8_t)('0' + (uint32_t)(sum % 10ull)); sum /= 10ull; }
    }
    if (WRITE) o[d] = (uint8_t)cls;
    return d + 1u;
}

struct Stretch {                  // the open stretch: the class and the sum of the runs of it so far
    bool open;
    uint32_t cls;
    uint64_t sum;
};
// one run more: the open stretch closes (its bytes, written at o if WRITE) unless the run joins it
template <int FORM, bool WRITE> __device__ __forceinline__ uint32_t stretch_run(Stretch& st, uint32_t run, uint8_t* o)
{
    const uint32_t cls = run_class<FORM>(run >> 8);
    uint32_t n = 0;
    if (st.open && !same_stretch<FORM>(st.cls, cls)) {
        n = put_stretch<WRITE>(o, st.sum, st.cls);
        st.sum = 0;
    }
    st.open = true;
    st.cls = cls;
    st.sum += run & 0xffu;
    return n;
}

// the length incl. the NUL of the text of runs s[0 .. cnt); WRITE: the text goes to o
template <int FORM, bool WRITE> __device__ __forceinline__ uint64_t form_walk_lane(const uint16_t* __restrict__ s, uint64_t cnt, uint8_t* o, bool* ok)
{
    Stretch st{false, 0u, 0ull};
    uint64_t n = 0;
    bool good = true;
    for (uint64_t k = 0; k < cnt; k++) {
        const uint32_t r = s[k];
        good = good && run_ok(r);
        n += stretch_run<FORM, WRITE>(st, r, o + n);
    }
    if (st.open) n += put_stretch<WRITE>(o + n, st.sum, st.cls);
    if (WRITE) o[n] = 0;
    *ok = good;
    return n + 1;
}

// a tile's bytes: the stretches that close in it — the first may hold a carried sum of twenty digits, every other lies in the tile
constexpr uint32_t FORM_TILE_BYTES = WALK_TILE_RUNS * 4 + 32;

// the same by all 64 lanes (cnt > 0); WRITE: a tile's bytes go through `tile` (LDS, FORM_TILE_BYTES) to out
template <int FORM, bool WRITE> __device__ __forceinline__ uint64_t form_walk_wave(const uint16_t* __restrict__ s, uint64_t cnt, uint8_t* out, uint8_t* tile,
                                                                                   uint32_t lane, bool* ok)
{
    Stretch carry{false, 0u, 0ull};               // the open stretch after the tiles so far (wavefront-uniform)
    uint64_t total = 0;
    bool bad_run = false;
    for (uint64_t t0 = 0; t0 < cnt; t0 += WALK_TILE_RUNS) {
        uint32_t r[WALK_LANE_RUNS];
        const uint32_t mine = load_lane_runs(s, cnt, t0, lane, r);
        // my last stretch: its class, the sum of my runs of it, and whether it begins at one of my runs after the first
        uint32_t tail = 0, first_cls = 0, last_cls = 0;
        bool inner = false;
#pragma unroll
        for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
            if (k >= mine) continue;
            if (!run_ok(r[k])) bad_run = true;
            const uint32_t cls = run_class<FORM>(r[k] >> 8);
            if (k == 0) first_cls = cls;
            else if (!same_stretch<FORM>(last_cls, cls)) { inner = true; tail = 0; }
            tail += r[k] & 0xffu;
            last_cls = cls;
        }
        // the stretch that is open in front of my first run: its class from the lane before (a lane with runs has only lanes with
        // eight runs before it), its sum by a segmented scan — a lane whose last stretch does not reach back past its first run
        // starts the sum again
        Stretch st;
        st.cls = (uint32_t)__shfl_up((int)last_cls, 1, 64);
        st.open = true;
        if (lane == 0) { st.cls = carry.cls; st.open = carry.open; }
        const bool joins = st.open && same_stretch<FORM>(st.cls, first_cls);
        uint32_t seg_v = tail, seg_f = (mine != 0u && (inner || !joins)) ? 1u : 0u;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint32_t vv = (uint32_t)__shfl_up((int)seg_v, dd, 64), vf = (uint32_t)__shfl_up((int)seg_f, dd, 64);
            if (lane >= (uint32_t)dd) {
                if (!seg_f) seg_v += vv;
                seg_f |= vf;
            }
        }
        uint32_t ex_v = (uint32_t)__shfl_up((int)seg_v, 1, 64), ex_f = (uint32_t)__shfl_up((int)seg_f, 1, 64);
        if (lane == 0) { ex_v = 0; ex_f = 0; }
        st.sum = ex_f ? (uint64_t)ex_v : carry.sum + ex_v;
        // the tile's state after its last run, for the next tile
        const uint32_t runs_here = (uint32_t)(cnt - t0 < WALK_TILE_RUNS ? cnt - t0 : WALK_TILE_RUNS);
        const int last_lane = (int)((runs_here - 1u) / WALK_LANE_RUNS);
        const uint32_t end_v = (uint32_t)__shfl((int)seg_v, last_lane, 64), end_f = (uint32_t)__shfl((int)seg_f, last_lane, 64);
        const uint32_t end_cls = (uint32_t)__shfl((int)last_cls, last_lane, 64);
        // the stretches that close at my runs: their bytes, and where they go
        uint32_t bytes = 0;
        {
            Stretch m = st;
#pragma unroll
            for (uint32_t k = 0; k < WALK_LANE_RUNS; k++)
                if (k < mine) bytes += stretch_run<FORM, false>(m, r[k], nullptr);
        }
        const uint32_t incl = wave_scan_incl(bytes, lane);
        const uint32_t tile_bytes = (uint32_t)__shfl((int)incl, 63, 64);
        if (WRITE) {
            uint8_t* o = tile + (incl - bytes);
#pragma unroll
            for (uint32_t k = 0; k < WALK_LANE_RUNS; k++)
                if (k < mine) o += stretch_run<FORM, true>(st, r[k], o);
            flush_tile(out + total, tile, tile_bytes, lane);
        }
        total += tile_bytes;
        carry.sum = end_f ? (uint64_t)end_v : carry.sum + end_v;
        carry.cls = end_cls;
        carry.open = true;
    }
    // the last stretch
    if (carry.open) {
        if (WRITE) {
            if (lane == 0) put_stretch<true>(out + total, carry.sum, carry.cls);
        }
        total += put_stretch<false>(nullptr, carry.sum, carry.cls);
    }
    if (WRITE) {
        if (lane == 0) out[total] = 0;
    }
    *ok = __ballot(bad_run) == 0ull;
    return total + 1;
}

// (FORM: SCRG_CIGAR_WINDOWED is the "%d%c" walk below; the other two forms go through form_walk_lane / form_walk_wave)
template <int FORM>
__global__ __launch_bounds__(256) void text_len_kernel(uint64_t n, const scrg_pair_desc* __restrict__ pairs,
                                                       const uint16_t* __restrict__ runs, const uint32_t* __restrict__ n_runs,
                                                       uint64_t* __restrict__ cnt64, uint64_t* __restrict__ len64, int want_text,
                                                       uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    for_each_group<TextRec>(
        n, split,
        [&](TextRec& me, uint64_t p, uint32_t sub) {
            run_slice(&pairs[0].cigar_off, 6, n_runs, p, me.cnt, me.src);
            if (sub == 0) cnt64[p] = me.cnt;
            if (!want_text) me.cnt = 0;           // (no lengths: nothing of the group is walked)
        },
        [&](const TextRec& me, uint64_t p) {
            if (!want_text) return;
            if constexpr (FORM != SCRG_CIGAR_WINDOWED) {
                bool ok;
                len64[p] = form_walk_lane<FORM, false>(runs + me.src, me.cnt, nullptr, &ok);
                return;
            }
            uint64_t chars = 1;
            const uint16_t* const s = runs + me.src;
            for (uint64_t k = 0; k < me.cnt; k++) chars += run_chars(s[k]);
            len64[p] = chars;
        },
        [&](const TextRec& me, uint64_t g0, uint32_t q, uint32_t lane) {
            const uint64_t cnt = __shfl(me.cnt, (int)q, 64), src = __shfl(me.src, (int)q, 64);
            if constexpr (FORM != SCRG_CIGAR_WINDOWED) {
                bool ok;
                const uint64_t len = form_walk_wave<FORM, false>(runs + src, cnt, nullptr, nullptr, lane, &ok);
                if (lane == 0) len64[g0 + q] = len;
                return;
            }
            const uint32_t* const s32 = reinterpret_cast<const uint32_t*>(runs + src);       // slices are 32-byte aligned: two runs per load
            uint32_t chars = 0;
            for (uint64_t k = lane; 2 * k < cnt; k += 64) {
                const uint32_t w = s32[k];
                chars += run_chars(w & 0xffffu) + (2 * k + 1 < cnt ? run_chars(w >> 16) : 0u);
            }
            chars = wave_sum(chars);
            if (lane == 0) len64[g0 + q] = (uint64_t)chars + 1u;
        },
        NothingAfter());
}

// totals[0] = all runs, totals[1] = all text bytes of the chunk (the offsets are exclusive prefix sums); and what of the
// per-pair results travels to the host: 12 bytes per pair instead of the 28 of the four arrays the caller gets — the edit
// distance as 32 bits, the run count with its flags (host_path.h: wire_count_word), the text length; the host makes the
// offsets from the counts again (scrg_host.cpp, stage 3).  For read mapping that is a tenth of all the bytes that come back.
__global__ __launch_bounds__(256) void wire_totals_kernel(uint64_t n, const int64_t* __restrict__ ed, const uint32_t* __restrict__ status,
                                                          const uint64_t* __restrict__ cnt64, const uint64_t* __restrict__ run_off,
                                                          const uint64_t* __restrict__ len64, const uint64_t* __restrict__ text_off,
                                                          uint64_t* __restrict__ totals, uint32_t* __restrict__ wire, int want_text)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        totals[0] = n ? run_off[n - 1] + cnt64[n - 1] : 0;
        totals[1] = (n && want_text) ? text_off[n - 1] + len64[n - 1] : 0;
    }
    if (i >= n) return;
    wire[i] = (uint32_t)ed[i];
    wire[n + i] = wire_count_word((uint32_t)cnt64[i], status[i]);
    if (want_text) wire[2 * n + i] = (uint32_t)len64[i];
}

// ---------------------------------------------------------------------------------------------------------------
// "%d%c" text of every pair from its DENSE runs (after the compaction), NUL-terminated, at text_off[p].
// One wavefront per pair for long alignments: a tile of 512 runs (8 per lane, one 16-byte load) is rendered into LDS at
// the positions a wavefront scan of the lanes' character counts gives, then leaves as contiguous bytes.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t put_run(uint8_t* o, uint32_t run)
{
    const uint32_t c = run & 0xffu, op = run >> 8;
    uint32_t k = 0;
    if (c >= 100u) o[k++] = (uint8_t)('0' + c / 100u);
    if (c >= 10u) o[k++] = (uint8_t)('0' + (c / 10u) % 10u);
    o[k++] = (uint8_t)('0' + c % 10u);
    o[k++] = (uint8_t)op;
    return k;
}

constexpr uint32_t TEXT_TILE_BYTES = WALK_TILE_RUNS * 4;

// (FORM as for text_len_kernel: the two passes of a chunk take the same one, and so give every pair the same length)
template <int FORM>
__global__ __launch_bounds__(256) void render_text_kernel(uint64_t n, const uint16_t* __restrict__ dense,
                                                          const uint64_t* __restrict__ run_off, const uint64_t* __restrict__ cnt64,
                                                          const uint64_t* __restrict__ text_off, uint8_t* __restrict__ text, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    __shared__ __attribute__((aligned(16))) uint8_t tile_all[4][FORM == SCRG_CIGAR_WINDOWED ? TEXT_TILE_BYTES : FORM_TILE_BYTES];
    uint8_t* const tile = tile_all[threadIdx.x >> 6];
    for_each_group<TextRec>(
        n, split,
        [&](TextRec& me, uint64_t p, uint32_t) {
            me.cnt = cnt64[p];
            me.src = run_off[p];
            me.dst = text_off[p];
        },
        [&](const TextRec& me, uint64_t) {        // straight to memory
            if constexpr (FORM != SCRG_CIGAR_WINDOWED) {
                bool ok;
                form_walk_lane<FORM, true>(dense + me.src, me.cnt, text + me.dst, &ok);
                return;
            }
            uint8_t* o = text + me.dst;
            const uint16_t* const s = dense + me.src;
            for (uint64_t k = 0; k < me.cnt; k++) o += put_run(o, s[k]);
            *o = 0;
        },
        [&](const TextRec& me, uint64_t, uint32_t q, uint32_t lane) {
            const uint64_t cnt = __shfl(me.cnt, (int)q, 64), src = __shfl(me.src, (int)q, 64);
            uint64_t dst = __shfl(me.dst, (int)q, 64);
            if constexpr (FORM != SCRG_CIGAR_WINDOWED) {
                bool ok;
                form_walk_wave<FORM, true>(dense + src, cnt, text + dst, tile, lane, &ok);
                return;
            }
            for (uint64_t t0 = 0; t0 < cnt; t0 += WALK_TILE_RUNS) {
                uint32_t r[WALK_LANE_RUNS], chars = 0;
                const uint32_t mine = load_lane_runs(dense + src, cnt, t0, lane, r);
#pragma unroll
                for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) chars += k < mine ? run_chars(r[k]) : 0u;
                const uint32_t incl = wave_scan_incl(chars, lane);
                const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
                uint8_t* o = tile + (incl - chars);
#pragma unroll
                for (uint32_t k = 0; k < WALK_LANE_RUNS; k++)
                    if (k < mine) o += put_run(o, r[k]);
                flush_tile(text + dst, tile, total, lane);
                dst += total;
            }
            if (lane == 0) text[dst] = 0;
        },
        NothingAfter());
}

// ---------------------------------------------------------------------------------------------------------------
// The same text for callers that run their own pipeline (scrg_cigar_text_lengths / scrg_cigar_text_render): runs by offset and
// stride (run_slice), a length pass, the caller's prefix sum, a render pass that takes nothing on trust.  A pair is measured
// again before it is rendered: nothing is written for a pair whose segment [off, off + len) is not inside [0, capacity) or
// whose len is not the length of its string, and it is counted in *bad.  In the merged forms a pair with a run that is none
// (run_ok) has "" in both passes and is counted; SCRG_CIGAR_WINDOWED prints what the runs hold.
// ---------------------------------------------------------------------------------------------------------------
struct CigarTextArgs {
    uint64_t n;
    const uint16_t* runs;
    const uint64_t* run_off;
    uint64_t run_off_stride;      // 1 or 6
    const uint32_t* n_runs;
    uint64_t* len;                // length pass: out; render pass: in
    const uint64_t* off;          // render pass
    uint8_t* text;
    uint64_t capacity;
    uint32_t* bad;
};
struct CigarTextPair {
    uint64_t cnt, src;
    uint64_t len, off;            // render pass: what the caller says of its string
    bool seg_ok;                  // that segment is inside the buffer
    uint32_t bad;                 // the pair is counted in *bad
};

// a pair's length incl. the NUL; *ok as the form defines it
template <int FORM> __device__ __forceinline__ uint64_t measure_lane(const uint16_t* __restrict__ s, uint64_t cnt, bool* ok)
{
    const uint64_t len = form_walk_lane<FORM, false>(s, cnt, nullptr, ok);
    if (FORM == SCRG_CIGAR_WINDOWED) *ok = true;
    return *ok ? len : 1;
}
template <int FORM> __device__ __forceinline__ uint64_t measure_wave(const uint16_t* __restrict__ s, uint64_t cnt, uint32_t lane, bool* ok)
{
    const uint64_t len = form_walk_wave<FORM, false>(s, cnt, nullptr, nullptr, lane, ok);
    if (FORM == SCRG_CIGAR_WINDOWED) *ok = true;
    return *ok ? len : 1;
}

template <int FORM> __global__ __launch_bounds__(256) void cigar_len_kernel(CigarTextArgs a, uint32_t split)
{
    for_each_group<CigarTextPair>(
        a.n, split, [&](CigarTextPair& me, uint64_t p, uint32_t) { run_slice(a.run_off, a.run_off_stride, a.n_runs, p, me.cnt, me.src); },
        [&](const CigarTextPair& me, uint64_t p) {
            bool ok;
            a.len[p] = measure_lane<FORM>(a.runs + me.src, me.cnt, &ok);
        },
        [&](const CigarTextPair& me, uint64_t g0, uint32_t q, uint32_t lane) {
            const uint64_t cnt = __shfl(me.cnt, (int)q, 64), src = __shfl(me.src, (int)q, 64);
            bool ok;
            const uint64_t len = measure_wave<FORM>(a.runs + src, cnt, lane, &ok);
            if (lane == 0) a.len[g0 + q] = len;
        },
        NothingAfter());
}

template <int FORM> __global__ __launch_bounds__(256) void cigar_render_kernel(CigarTextArgs a, uint32_t split)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile_all[4][FORM_TILE_BYTES];
    uint8_t* const tile = tile_all[threadIdx.x >> 6];
    for_each_group<CigarTextPair>(
        a.n, split,
        [&](CigarTextPair& me, uint64_t p, uint32_t) {
            run_slice(a.run_off, a.run_off_stride, a.n_runs, p, me.cnt, me.src);
            me.len = a.len[p];
            me.off = a.off[p];
            me.seg_ok = me.len >= 1 && me.off <= a.capacity && me.len <= a.capacity - me.off;
        },
        [&](CigarTextPair& me, uint64_t) {
            bool ok;
            const uint64_t len = measure_lane<FORM>(a.runs + me.src, me.cnt, &ok);
            if (!ok || !me.seg_ok || len != me.len) me.bad = 1;
            if (me.seg_ok && len == me.len) {
                if (ok) form_walk_lane<FORM, true>(a.runs + me.src, me.cnt, a.text + me.off, &ok);
                else a.text[me.off] = 0;
            }
        },
        [&](CigarTextPair& me, uint64_t, uint32_t q, uint32_t lane) {
            const uint64_t cnt = __shfl(me.cnt, (int)q, 64), src = __shfl(me.src, (int)q, 64);
            const uint64_t q_len = __shfl(me.len, (int)q, 64), q_off = __shfl(me.off, (int)q, 64);
            const bool q_seg = __shfl((int)me.seg_ok, (int)q, 64) != 0;
            bool ok;
            const uint64_t len = measure_wave<FORM>(a.runs + src, cnt, lane, &ok);
            if (lane == q && (!ok || !q_seg || len != q_len)) me.bad = 1;
            if (q_seg && len == q_len) {
                if (ok) form_walk_wave<FORM, true>(a.runs + src, cnt, a.text + q_off, tile, lane, &ok);
                else if (lane == 0) a.text[q_off] = 0;
            }
        },
        [&](const CigarTextPair& me, uint32_t lane) {
            const uint32_t n_bad = (uint32_t)__popcll(__ballot(me.bad != 0));
            if (n_bad && lane == 0) atomicAdd(a.bad, n_bad);
        });
}

// ---------------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------------
// (form: SCRG_CIGAR_WINDOWED, _MERGED or _M — the entry points let no other through)
#define SCRG_LAUNCH_FORM(kernel, form, blocks, s, ...)                                                                  \
    do {                                                                                                                \
        if ((form) == SCRG_CIGAR_MERGED) hipLaunchKernelGGL(kernel<SCRG_CIGAR_MERGED>, dim3((unsigned)(blocks)), dim3(256), 0, s, __VA_ARGS__);       \
        else if ((form) == SCRG_CIGAR_M) hipLaunchKernelGGL(kernel<SCRG_CIGAR_M>, dim3((unsigned)(blocks)), dim3(256), 0, s, __VA_ARGS__);            \
        else hipLaunchKernelGGL(kernel<SCRG_CIGAR_WINDOWED>, dim3((unsigned)(blocks)), dim3(256), 0, s, __VA_ARGS__);   \
    } while (0)

hipError_t launch_cigar_text_lengths(uint64_t n, const uint16_t* runs, const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs,
                                     int32_t form, uint64_t* len, int n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    CigarTextArgs a{};
    a.n = n;
    a.runs = runs;
    a.run_off = run_off;
    a.run_off_stride = run_off_stride;
    a.n_runs = n_runs;
    a.len = len;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(n, n_cus, &split);
    SCRG_LAUNCH_FORM(cigar_len_kernel, form, blocks, s, a, split);
    return hipGetLastError();
}

hipError_t launch_cigar_text_render(uint64_t n, const uint16_t* runs, const uint64_t* run_off, uint64_t run_off_stride, const uint32_t* n_runs,
                                    int32_t form, const uint64_t* len, const uint64_t* off, uint8_t* text, uint64_t capacity, uint32_t* bad,
                                    int n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    CigarTextArgs a{};
    a.n = n;
    a.runs = runs;
    a.run_off = run_off;
    a.run_off_stride = run_off_stride;
    a.n_runs = n_runs;
    a.len = const_cast<uint64_t*>(len);
    a.off = off;
    a.text = text;
    a.capacity = capacity;
    a.bad = bad;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(n, n_cus, &split);
    SCRG_LAUNCH_FORM(cigar_render_kernel, form, blocks, s, a, split);
    return hipGetLastError();
}

hipError_t launch_build_desc(const HostDescArgs& a, hipStream_t s)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(build_desc_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

size_t host_scan_temp_bytes(uint64_t n)
{
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n, (hipStream_t)0);
    return bytes;
}

// cnt64 / len64 -> run_off / text_off (exclusive sums) and the two totals
hipError_t launch_result_layout(uint64_t n, const scrg_pair_desc* pairs, const uint16_t* runs, const uint32_t* n_runs, const int64_t* ed,
                                const uint32_t* status, uint64_t* cnt64, uint64_t* len64, uint64_t* run_off, uint64_t* text_off,
                                uint64_t* totals, uint32_t* wire, void* temp, size_t temp_bytes, int want_text, int32_t form, int n_cus,
                                hipStream_t s)
{
    if (n == 0) return hipMemsetAsync(totals, 0, 16, s);
    uint32_t split = 1;
    const uint64_t blocks = group_grid(n, n_cus, &split);
    SCRG_LAUNCH_FORM(text_len_kernel, form, blocks, s, n, pairs, runs, n_runs, cnt64, len64, want_text, split);
    size_t tb = temp_bytes;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(temp, tb, cnt64, run_off, (int)n, s);
    if (e != hipSuccess) return e;
    if (want_text) {
        tb = temp_bytes;
        e = hipcub::DeviceScan::ExclusiveSum(temp, tb, len64, text_off, (int)n, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(wire_totals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, ed, status, cnt64, run_off, len64, text_off, totals,
                       wire, want_text);
    return hipGetLastError();
}

hipError_t launch_render_text(uint64_t n, const uint16_t* dense, const uint64_t* run_off, const uint64_t* cnt64, const uint64_t* text_off,
                              uint8_t* text, int32_t form, int n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(n, n_cus, &split);
    SCRG_LAUNCH_FORM(render_text_kernel, form, blocks, s, n, dense, run_off, cnt64, text_off, text, split);
    return hipGetLastError();
}

}  // namespace scrg
