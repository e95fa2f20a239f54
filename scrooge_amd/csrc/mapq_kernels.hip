// mapq_kernels.hip — the per-read candidate summary and its mapping quality (scrg_read_summary, the host calls' read summary; the
// rule: mapq_rule.h): for every read the winner by best-candidate mode's rule, its distance, how many eligible candidates share it,
// the next distance above it and the counts, graded into a MAPQ, as one 32-byte record; and, where asked for, a copy of the pairs'
// statuses in which only the winners of confidently placed reads are still "done" — what the pileup is then summed from.
//
// Two forms in one launch, as the run-walk passes have them.  A LANE takes a read of up to 16 candidates and walks them serially
// (the common case: a handful of candidates, 12 bytes read per candidate).  Reads with more are balloted, and the whole WAVEFRONT
// then takes them one after another, 64 candidates per step (four steps' loads in flight), every lane keeping the partial summary of what it saw; a butterfly of
// mapq_merge over the lanes (the merge is associative and commutative) leaves the same summary in all 64, lanes 0 .. 7 store one
// dword of the record each, and a second sweep writes the statuses' copy.  No atomics, no LDS, no scratch to initialise, nothing
// crosses a wavefront, and the result does not depend on which form served a read or on the schedule.
#include <algorithm>

#include "genasm_kernels.h"
#include "host_path.h"
#include "mapq_rule.h"

namespace scrg {

namespace {

struct SummaryArgs {
    MapqRule rule;
    uint64_t n_reads, n_pairs;
    const uint64_t* first;        // [n_reads + 1]
    const uint32_t* read_len;     // per pair
    const int64_t* ed;
    const uint32_t* status;
    uint32_t* out;                // 8 dwords per read
    uint32_t* keep;               // may be null; per pair
};

__device__ __forceinline__ uint64_t mapq_shfl64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ MapqPart mapq_xor(const MapqPart& p, int d)
{
    MapqPart o;
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)p.best, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(p.best >> 32), d, 64);
    o.best = ((uint64_t)hi << 32) | lo;
    o.n_tied = (uint32_t)__shfl_xor((int)p.n_tied, d, 64);
    o.second_ed = (uint32_t)__shfl_xor((int)p.second_ed, d, 64);
    o.n_eligible = (uint32_t)__shfl_xor((int)p.n_eligible, d, 64);
    return o;
}

__device__ __forceinline__ void mapq_see(const SummaryArgs& k, MapqPart& part, uint64_t p)
{
    if (k.status[p] != (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT) part = mapq_merge(part, mapq_part_one(mapq_ed(k.ed[p]), (uint32_t)p));
}

__device__ __forceinline__ void mapq_keep(const SummaryArgs& k, uint64_t p, bool kept, uint32_t winner)
{
    k.keep[p] = mapq_keep_status(k.status[p], kept && (uint32_t)p == winner, (uint32_t)LANE_STATUS_NOT_BEST);
}

}  // namespace

__global__ __launch_bounds__(256) void read_summary_kernel(const SummaryArgs k)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t f0 = 0, n = 0;
    if (r < k.n_reads) {
        f0 = k.first[r];
        const uint64_t f1 = k.first[r + 1];
        if (f0 <= f1 && f1 <= k.n_pairs) n = f1 - f0;              // (offsets that run backwards or past the arrays name no candidates: nothing is read)
    }
    // the lane form
    if (r < k.n_reads && n <= MAPQ_LANE_READ) {
        MapqPart part = mapq_part_none();
        for (uint64_t c = 0; c < n; c++) mapq_see(k, part, f0 + c);
        const MapqWords rec = mapq_record(k.rule, part, n ? k.read_len[f0] : 0u, (uint32_t)n);
        uint32_t* const o = k.out + 8 * r;
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = rec.w[j];
        if (k.keep) {
            const bool kept = mapq_words_kept(rec);
            for (uint64_t c = 0; c < n; c++) mapq_keep(k, f0 + c, kept, rec.w[0]);
        }
    }
    // the wavefront form: the reads the lanes above left, one after another (the ballot is the wavefront's, so the loop is uniform)
    uint64_t big = __ballot(r < k.n_reads && n > MAPQ_LANE_READ);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const uint64_t F0 = mapq_shfl64(f0, src), N = mapq_shfl64(n, src), R = r - lane + (uint32_t)src;
        MapqPart part = mapq_part_none();
        // four steps' loads are issued together (a lane's own steps depend on each other only through the fold): the few wavefronts
        // a batch of long reads occupies wait for memory, not for arithmetic
        for (uint64_t c0 = lane; c0 < N; c0 += 256) {
            uint32_t st[4];
            int64_t e[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t c = c0 + 64u * (uint32_t)u;
                const bool in = c < N;
                st[u] = in ? k.status[F0 + c] : (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT;
                e[u] = in ? k.ed[F0 + c] : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (st[u] != (uint32_t)LANE_STATUS_OVER_EDIT_LIMIT) part = mapq_merge(part, mapq_part_one(mapq_ed(e[u]), (uint32_t)(F0 + c0 + 64u * (uint32_t)u)));
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part = mapq_merge(part, mapq_xor(part, d));
        const MapqWords rec = mapq_record(k.rule, part, k.read_len[F0], (uint32_t)(N < 0xffffffffull ? N : 0xffffffffull));
        if (lane < 8) {
            uint32_t w = rec.w[0];
#pragma unroll
            for (int j = 1; j < 8; j++) w = lane == (uint32_t)j ? rec.w[j] : w;
            k.out[8 * R + lane] = w;
        }
        if (k.keep) {
            const bool kept = mapq_words_kept(rec);
            for (uint64_t c = lane; c < N; c += 64) mapq_keep(k, F0 + c, kept, rec.w[0]);
        }
    }
}

hipError_t launch_read_summary(const scrg_mapq_rule& rule, uint64_t n_reads, uint64_t n_pairs, const uint64_t* first, const uint32_t* read_len,
                               const int64_t* ed, const uint32_t* status, scrg_read_record* out, uint32_t* keep_status, hipStream_t s)
{
    if (n_reads == 0) return hipSuccess;
    SummaryArgs k;
    k.rule = MapqRule{rule.per_edit, rule.max_q, rule.zero_per_mille, rule.min_keep_q};
    k.n_reads = n_reads;
    k.n_pairs = n_pairs;
    k.first = first;
    k.read_len = read_len;
    k.ed = ed;
    k.status = status;
    k.out = reinterpret_cast<uint32_t*>(out);
    k.keep = keep_status;
    hipLaunchKernelGGL(read_summary_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, s, k);
    return hipGetLastError();
}

}  // namespace scrg
