// report_kernels.hip — the alignment report (scrg_pair_report, include/scrooge_amd.h: ALIGNMENT REPORT): per pair the bases under
// each operation, the gap openings and indel stretches, and a verdict — is this list of runs an alignment of these two sequences
// with this edit distance — from the pair's runs, the two packed sequences and the edit distance.  One pass, 32 bytes out per pair,
// over run_walk.h: one pair per lane up to WALK_LANE_MAX_RUNS runs, one wavefront per pair above that in tiles of 512 runs, eight
// per lane, with the text and read positions and the operation of the run before from the shared tile step.
//
// The verdict is scrg_validate_alignment's walk (scrg_io.cpp) on runs and 2-bit codes; the first failure in run order wins.  In
// the wavefront form every lane checks its own eight runs at the positions the scan gives it — positions behind a run that fails
// are of no interest, and lane L holds runs 8 L .. 8 L + 7 of the tile, so the lowest lane that met a failure has the first one.
//
// The base check is word-parallel: 32 bases of text and read per step, each fetched as the one or two words that hold them and
// funnel-shifted to the run's bit offset; (tlo ^ qlo) | (thi ^ qhi) over the run's bases is zero for '=' and all ones for 'X'.
// A reversed sequence (SCRG_READ_REVCOMP, SCRG_TEXT_REVCOMP) gives the forward bases that END where the step starts, bit-reversed
// and inverted in both planes.  Only words that hold a base of the pair's own sequences are read: a step is fetched after its
// run was found to lie inside both sequences.  (PER_BASE: the same walk with one base_code per base and sequence — the build the
// word-parallel form is measured against, tests/tools/bench_report.py.)
#include "genasm_kernels.h"
#include "host_path.h"
#include "run_walk.h"
#include "text_revcomp.h"

namespace scrg {

constexpr uint32_t REPORT_NO_ALIGNMENT = 7;       // SCRG_REPORT_NO_ALIGNMENT

// m (1 .. 32) forward bases from base k of the sequence at `off`: bit j of lo / hi = the low / high code bit of base k + j for
// j < m (the bits above are whatever follows).  The second word is read only if one of the m bases lies in it.
__device__ __forceinline__ void fetch_forward(const uint64_t* __restrict__ seq, uint64_t off, uint32_t stride, uint64_t k, uint32_t m, uint32_t& lo, uint32_t& hi)
{
    const uint64_t pos = (off & 31ull) + k;
    const uint64_t w = (off >> 5) + (pos >> 5) * stride;
    const uint32_t bit = (uint32_t)pos & 31u;
    const uint64_t w0 = seq[w];
    const uint64_t w1 = bit + m > 32u ? seq[w + stride] : 0ull;
    lo = __funnelshift_r((uint32_t)w0, (uint32_t)w1, bit);
    hi = __funnelshift_r((uint32_t)(w0 >> 32), (uint32_t)(w1 >> 32), bit);
}
// the same of the sequence AS ALIGNED: character k of a reversed sequence of `len` bases is the complement of base len - 1 - k, so
// characters k .. k + m - 1 are the forward bases len - k - m .. len - k - 1 backwards, inverted in both planes (A0 C1 G2 T3)
__device__ __forceinline__ void fetch_aligned(const uint64_t* __restrict__ seq, uint64_t off, uint32_t stride, uint64_t len, bool rev, uint64_t k, uint32_t m,
                                              uint32_t& lo, uint32_t& hi)
{
    if (!rev) {
        fetch_forward(seq, off, stride, k, m, lo, hi);
    } else {
        fetch_forward(seq, off, stride, len - k - m, m, lo, hi);
        lo = ~__brev(lo << (32u - m));
        hi = ~__brev(hi << (32u - m));
    }
}
// do the c bases of text from t and of read from q all agree (equal = true) / all differ (false)?  They lie inside both sequences.
template <bool PER_BASE> __device__ __forceinline__ bool bases_agree(const PairSeq& s, uint64_t t, uint64_t q, uint32_t c, bool equal)
{
    if (PER_BASE) {
        for (uint32_t j = 0; j < c; j++) {
            if ((text_code(s, t + j) == read_code(s, q + j)) != equal) return false;
        }
        return true;
    }
    for (uint32_t j = 0; j < c; j += 32u) {
        const uint32_t m = c - j < 32u ? c - j : 32u;
        uint32_t tlo, thi, qlo, qhi;
        fetch_aligned(s.seq, s.text_off, s.text_stride, s.text_len, s.text_rev, t + j, m, tlo, thi);
        fetch_aligned(s.seq, s.read_off, s.read_stride, s.read_len, s.read_rev, q + j, m, qlo, qhi);
        const uint32_t mask = 0xffffffffu >> (32u - m);
        const uint32_t differ = ((tlo ^ qlo) | (thi ^ qhi)) & mask;
        if (differ != (equal ? 0u : mask)) return false;
    }
    return true;
}

// one run at text position t and read position q: 0, or the verdict it ends the walk with (scrg_validate_alignment's order)
template <bool PER_BASE> __device__ __forceinline__ uint32_t check_run(uint32_t run, uint64_t t, uint64_t q, const PairSeq& s)
{
    const uint32_t c = run & 0xffu, op = run >> 8;
    if (c == 0u) return 2u;
    if (op == '=' || op == 'X') {
        if (q + c > s.read_len) return 3u;
        if (t + c > s.text_len) return 4u;
        return bases_agree<PER_BASE>(s, t, q, c, op == '=') ? 0u : 5u;
    }
    if (op == 'I') return q + c > s.read_len ? 3u : 0u;
    if (op == 'D') return t + c > s.text_len ? 4u : 0u;
    return 1u;
}

struct RepCounts {
    uint32_t match, mismatch, ins, del, gap_open, indel;
};
// a valid run, and the operation of the run before it (0: none)
__device__ __forceinline__ void count_run(RepCounts& n, uint32_t run, uint32_t prev)
{
    const uint32_t c = run & 0xffu, op = run >> 8;
    if (op == '=') n.match += c;
    else if (op == 'X') n.mismatch += c;
    else {
        if (op == 'I') n.ins += c;
        else n.del += c;
        if (prev != 'I' && prev != 'D') n.gap_open++;
        if (prev != op) n.indel++;
    }
}

__device__ __forceinline__ scrg_pair_report failed_at(uint32_t verdict, uint32_t run)
{
    scrg_pair_report r{};
    r.verdict = verdict;
    r.bad_run = run;
    return r;
}
// after the last run: the read consumed exactly, the edits the edit distance
__device__ __forceinline__ scrg_pair_report finish(const RepCounts& n, uint64_t q, uint64_t read_len, uint64_t cnt, int64_t ed)
{
    scrg_pair_report r;
    r.n_match = n.match;
    r.n_mismatch = n.mismatch;
    r.n_ins = n.ins;
    r.n_del = n.del;
    r.n_gap_open = n.gap_open;
    r.n_indel = n.indel;
    r.verdict = 0u;
    r.bad_run = 0u;
    if (q != read_len) r.verdict = 3u;
    else if ((int64_t)((uint64_t)n.mismatch + n.ins + n.del) != ed) r.verdict = 6u;
    if (r.verdict) r.bad_run = (uint32_t)cnt;
    return r;
}

struct ReportArgs {
    PairRuns pr;
    const int64_t* ed;
    const uint32_t* status;       // may be null
    uint32_t text_strands;
    scrg_pair_report* report;
    uint32_t* fail;               // may be null
};

struct RepPair {                  // a pair as the kernel takes it
    uint64_t cnt, src;            // runs, first run
    bool desc_ok;                 // no strand bit the call does not honour
    bool aligned;                 // its status says it has an alignment
    int64_t ed;
    PairSeq sq;
    uint32_t bad;                 // (its lane) the pair is counted in *fail
};

__device__ __forceinline__ void load_pair(RepPair& d, const ReportArgs& a, uint64_t p)
{
    const scrg_pair_desc pd = a.pr.pairs[p];
    run_slice(a.pr.run_off, a.pr.run_off_stride, a.pr.n_runs, p, d.cnt, d.src);
    const uint32_t st = a.status ? a.status[p] : (uint32_t)LANE_STATUS_DONE;
    d.aligned = st != LANE_STATUS_OVER_EDIT_LIMIT && st != LANE_STATUS_NOT_BEST;
    d.ed = a.ed[p];
    d.sq = pair_seq(a.pr, pd);
    d.desc_ok = (!d.sq.read_rev || a.pr.stranded) && (!d.sq.text_rev || a.text_strands);
    // (a flagged text as the align kernels take it — of a stretch longer than 2^32 - 1 bases the last ones: text_revcomp.h)
    const TextStretch ts = text_stretch(pd.text_off, pd.text_len, d.sq.text_rev, a.pr.text_stride);
    d.sq.text_off = ts.off;
    if (d.sq.text_rev) d.sq.text_len = ts.len;
    if (!d.aligned || !d.desc_ok) d.cnt = 0;          // (nothing of such a pair is walked)
}

// what a pair that is not walked reports
__device__ __forceinline__ bool unwalked(const RepPair& d, scrg_pair_report* r)
{
    if (!d.aligned) { *r = failed_at(REPORT_NO_ALIGNMENT, 0u); return true; }
    if (!d.desc_ok) { *r = failed_at(1u, 0u); return true; }
    return false;
}

// ---------------------------------------------------------------------------------------------------------------
// one pair per lane: a serial walk
// ---------------------------------------------------------------------------------------------------------------
template <bool PER_BASE> __device__ __forceinline__ scrg_pair_report walk_lane(const RepPair& d, const uint16_t* __restrict__ runs)
{
    scrg_pair_report r;
    if (unwalked(d, &r)) return r;
    const uint16_t* const s = runs + d.src;
    RepCounts n{0u, 0u, 0u, 0u, 0u, 0u};
    uint64_t t = 0, q = 0;
    uint32_t prev = 0;
    for (uint64_t k = 0; k < d.cnt; k++) {
        const uint32_t run = s[k];
        const uint32_t v = check_run<PER_BASE>(run, t, q, d.sq);
        if (v) return failed_at(v, (uint32_t)k);
        count_run(n, run, prev);
        const uint32_t c = run & 0xffu, op = run >> 8;
        if (op != 'I') t += c;
        if (op != 'D') q += c;
        prev = op;
    }
    return finish(n, q, d.sq.read_len, d.cnt, d.ed);
}

// ---------------------------------------------------------------------------------------------------------------
// one wavefront per pair: tiles of 512 runs, eight per lane.  All 64 lanes call it with the same pair (which is walked: aligned,
// desc_ok) and all return its record.
// ---------------------------------------------------------------------------------------------------------------
template <bool PER_BASE> __device__ __forceinline__ scrg_pair_report walk_wave(const RepPair& d, const uint16_t* __restrict__ runs, uint32_t lane)
{
    const uint16_t* const s = runs + d.src;
    RepCounts n{0u, 0u, 0u, 0u, 0u, 0u};          // my runs' share
    WalkPos carry{};                              // the state after the tiles so far (wavefront-uniform)
    for (uint64_t t0 = 0; t0 < d.cnt; t0 += WALK_TILE_RUNS) {
        // my eight runs, the positions in front of them and the operation before them.  (A run that is no run ends the walk.)
        const RunTile x = load_tile(s, d.cnt, t0, lane, carry, [](uint32_t&) {});
        uint64_t t = x.at.t, q = x.at.q;
        uint32_t prev = x.at.prev;
        // my runs: the first that fails, the counts of those before it
        uint32_t fail = 0;                        // (k << 3 | verdict) + 1 of my first failure
#pragma unroll
        for (uint32_t k = 0; k < WALK_LANE_RUNS; k++) {
            if (k >= x.mine || fail) continue;
            const uint32_t v = check_run<PER_BASE>(x.r[k], t, q, d.sq);
            if (v) {
                fail = ((k << 3) | v) + 1u;
                continue;
            }
            count_run(n, x.r[k], prev);
            const uint32_t c = x.r[k] & 0xffu, op = x.r[k] >> 8;
            if (op != 'I') t += c;
            if (op != 'D') q += c;
            prev = op;
        }
        const uint64_t failed = __ballot(fail != 0u);
        if (failed) {                             // lane L holds runs 8 L .. 8 L + 7: the lowest lane has the first failure
            const uint32_t first = (uint32_t)__builtin_ctzll(failed);
            const uint32_t key = (uint32_t)__shfl((int)fail, (int)first, 64) - 1u;
            return failed_at(key & 7u, (uint32_t)(t0 + WALK_LANE_RUNS * first + (key >> 3)));
        }
        move_past(carry, x);
    }
    RepCounts all;
    all.match = wave_sum(n.match);
    all.mismatch = wave_sum(n.mismatch);
    all.ins = wave_sum(n.ins);
    all.del = wave_sum(n.del);
    all.gap_open = wave_sum(n.gap_open);
    all.indel = wave_sum(n.indel);
    return finish(all, carry.q, d.sq.read_len, d.cnt, d.ed);
}

__device__ __forceinline__ void store_report(scrg_pair_report* dst, const scrg_pair_report& r)
{
    // (a record is 32 bytes, the array 4-byte aligned as far as the interface says: eight dword stores)
    uint32_t* const o = reinterpret_cast<uint32_t*>(dst);
    o[0] = r.n_match;
    o[1] = r.n_mismatch;
    o[2] = r.n_ins;
    o[3] = r.n_del;
    o[4] = r.n_gap_open;
    o[5] = r.n_indel;
    o[6] = r.verdict;
    o[7] = r.bad_run;
}

template <bool PER_BASE> __global__ __launch_bounds__(256) void report_kernel(ReportArgs a, uint32_t split)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    for_each_group<RepPair>(
        a.pr.n, split, [&](RepPair& me, uint64_t p, uint32_t) { load_pair(me, a, p); },
        [&](RepPair& me, uint64_t p) {
            const scrg_pair_report r = walk_lane<PER_BASE>(me, a.pr.runs);
            store_report(a.report + p, r);
            me.bad = r.verdict != 0u && r.verdict != REPORT_NO_ALIGNMENT;
        },
        [&](RepPair& me, uint64_t g0, uint32_t q, uint32_t lane) {
            RepPair dq;
            load_pair(dq, a, g0 + q);
            const scrg_pair_report r = walk_wave<PER_BASE>(dq, a.pr.runs, lane);
            if (lane == q) {
                store_report(a.report + g0 + q, r);
                me.bad = r.verdict != 0u;
            }
        },
        [&](const RepPair& me, uint32_t lane) {
            const uint32_t n_bad = (uint32_t)__popcll(__ballot(me.bad != 0u));
            if (a.fail && n_bad && lane == 0) atomicAdd(a.fail, n_bad);
        });
}

hipError_t launch_report(const PairRuns& pr, const int64_t* ed, const uint32_t* status, uint32_t text_strands, scrg_pair_report* report,
                         uint32_t* fail, bool per_base, int n_cus, hipStream_t s)
{
    if (pr.n == 0) return hipSuccess;
    ReportArgs a{};
    a.pr = pr;
    a.ed = ed;
    a.status = status;
    a.text_strands = text_strands;
    a.report = report;
    a.fail = fail;
    uint32_t split = 1;
    const uint64_t blocks = group_grid(pr.n, n_cus, &split);
    if (per_base) hipLaunchKernelGGL(report_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    else hipLaunchKernelGGL(report_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a, split);
    return hipGetLastError();
}

}  // namespace scrg
