// seed_kernels.hip — seeding on the GPU (include/scrooge_amd.h: SEEDING; the rule: seed_rule.h; the calls: scrg_host.cpp).
//
//   index     seed_index_keys_kernel     one lane per indexed position: (key, p) from the packed genome
//             (with sampling, seed_key_selected, the entries depend on the data: seed_select_count_kernel, one lane per considered
//             position, leaves one count per workgroup — a wavefront ballot and its popcount —, an exclusive sum of those the
//             workgroups' bases, and seed_select_emit_kernel makes the keys again and writes the selected (key, p) compacted, each at
//             its workgroup's base plus the ballot's prefix; no array per considered position exists)
//             hipcub radix sort over the key's 2k bits
//             seed_index_buckets_kernel  a table over the key's top bits: a lookup is one read of two neighbouring table words
//                                        and a search among the bucket's few entries, not a search of the whole index
//   lookup    seed_lookup_kernel         one workgroup per read, its lanes stride over (strand, r): the key straight from the packed
//                                        read — the reverse strand from the same copy — and its entries counted; three forms:
//                                        totals per read (what the host cuts chunks by), counts per lane, and, behind an exclusive
//                                        sum of those, the hits themselves: word (read in chunk, strand, d + 2^32), value r
//             hipcub radix sort of the chunk's hits by their word
//   clusters  seed_heads_kernel          flags the hits that begin a cluster; an inclusive sum numbers the clusters
//             seed_clusters_kernel       a head leaves its position (votes = the distance to the next head), every hit takes part
//                                        in the minimum of (r, d) of its cluster: atomicMin on one word per cluster
//   pick      seed_pick_kernel           one wavefront per read: max_candidates rounds of "the smallest rank above the last one"
//
// Every store is a vector store; nothing here depends on the order in which lanes or atomics arrive.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "host_path.h"
#include "seed_rule.h"

namespace scrg {

namespace {

constexpr int SEED_BLOCK = 256;

__global__ __launch_bounds__(SEED_BLOCK) void seed_index_keys_kernel(const uint64_t* __restrict__ genome, uint64_t n_entries, uint32_t k, uint32_t stride,
                                                                     uint32_t* __restrict__ keys, uint32_t* __restrict__ pos)
{
    const uint64_t e = (uint64_t)blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (e >= n_entries) return;
    const uint64_t p = e * stride;                       // (below 2^32: the genome is)
    const uint64_t w = p >> 5;
    uint32_t lo, hi;
    seed_planes16(genome[w], genome[w + 1], (uint32_t)p & 31u, lo, hi);          // (the word behind the genome's last is padding)
    keys[e] = seed_key_forward(lo, hi, k);
    pos[e] = (uint32_t)p;
}

// Position e of the considered ones (p = e * stride): its key, and whether the index takes it.  One text for the count and the emit.
__device__ inline bool seed_select_lane(const uint64_t* __restrict__ genome, uint64_t e, uint64_t n_positions, uint32_t k, uint32_t stride, uint32_t smer,
                                        uint32_t& key, uint32_t& p32)
{
    key = p32 = 0;
    if (e >= n_positions) return false;
    const uint64_t p = e * stride;
    const uint64_t w = p >> 5;
    uint32_t lo, hi;
    seed_planes16(genome[w], genome[w + 1], (uint32_t)p & 31u, lo, hi);
    key = seed_key_forward(lo, hi, k);
    p32 = (uint32_t)p;
    return seed_key_selected(key, k, smer);
}

// block_cnt[workgroup] = its selected positions
__global__ __launch_bounds__(SEED_BLOCK) void seed_select_count_kernel(const uint64_t* __restrict__ genome, uint64_t n_positions, uint32_t k, uint32_t stride,
                                                                       uint32_t smer, uint32_t* __restrict__ block_cnt)
{
    __shared__ uint32_t wave_cnt[SEED_BLOCK / 64];
    uint32_t key, p;
    const bool sel = seed_select_lane(genome, (uint64_t)blockIdx.x * SEED_BLOCK + threadIdx.x, n_positions, k, stride, smer, key, p);
    const uint64_t ballot = __ballot(sel);
    if ((threadIdx.x & 63u) == 0u) wave_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < SEED_BLOCK / 64; w++) t += wave_cnt[w];
        block_cnt[blockIdx.x] = t;
    }
}

// block_base: the exclusive sum of block_cnt.  A selected position's entry: its workgroup's base, the wavefronts before its own,
// the selected lanes below it in the ballot — positions ascending, so the order is the unsampled build's with the others left out.
__global__ __launch_bounds__(SEED_BLOCK) void seed_select_emit_kernel(const uint64_t* __restrict__ genome, uint64_t n_positions, uint32_t k, uint32_t stride,
                                                                      uint32_t smer, const uint32_t* __restrict__ block_base, uint32_t n_entries,
                                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ pos)
{
    __shared__ uint32_t wave_cnt[SEED_BLOCK / 64];
    uint32_t key, p;
    const bool sel = seed_select_lane(genome, (uint64_t)blockIdx.x * SEED_BLOCK + threadIdx.x, n_positions, k, stride, smer, key, p);
    const uint64_t ballot = __ballot(sel);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) wave_cnt[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (!sel) return;
    uint32_t at = block_base[blockIdx.x] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; w++) at += wave_cnt[w];
    if (at >= n_entries) return;                         // (never, when block_base is the sum of this genome's counts: a guard, not a path)
    keys[at] = key;
    pos[at] = p;
}

// buckets[b] = the first entry whose key >> shift is at least b, b in [0, n_buckets]
__global__ __launch_bounds__(SEED_BLOCK) void seed_index_buckets_kernel(const uint32_t* __restrict__ keys, uint32_t n_entries, uint32_t shift,
                                                                        uint64_t n_buckets, uint32_t* __restrict__ buckets)
{
    const uint64_t b = (uint64_t)blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (b > n_buckets) return;
    uint32_t a = 0, e = n_entries;
    while (a < e) {
        const uint32_t m = a + ((e - a) >> 1);
        if ((uint64_t)(keys[m] >> shift) < b) a = m + 1;
        else e = m;
    }
    buckets[b] = a;
}

// the entries of `key`: their first, and their number as far as it matters (at most max_occ + 1)
__device__ inline uint32_t seed_entries(const SeedIndexView& ix, uint32_t key, uint32_t& first)
{
    const uint32_t b = key >> ix.shift;
    const uint32_t lo = ix.buckets[b], hi = ix.buckets[b + 1];
    if (ix.shift == 0u) {                                // a bucket per key
        first = lo;
        return hi - lo;
    }
    uint32_t a = lo, e = hi;
    while (a < e) {
        const uint32_t m = a + ((e - a) >> 1);
        if (ix.keys[m] < key) a = m + 1;
        else e = m;
    }
    first = a;
    uint32_t u = a;
    e = hi - a > ix.max_occ + 1u ? a + ix.max_occ + 1u : hi;
    while (u < e) {
        const uint32_t m = u + ((e - u) >> 1);
        if (ix.keys[m] <= key) u = m + 1;
        else e = m;
    }
    return u - a;
}

__device__ inline uint64_t seed_block_sum(uint64_t v, uint64_t* lds)
{
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SEED_BLOCK / 64; w++) t += lds[w];
    __syncthreads();
    return t;                                            // (thread 0's is the sum)
}

// MODE 0: read_hits[read], read_over[read], read_lookups[read] (all reads of the launch); 1: cnt[lane] of the chunk; 2: the hits, at
// off[lane].  A lane whose key the sampling leaves out (ix.smer) has no entries and reads nothing of the index.
template <int MODE>
__global__ __launch_bounds__(SEED_BLOCK) void seed_lookup_kernel(SeedIndexView ix, SeedReadsView rd, uint64_t read0, uint64_t lane_base,
                                                                 uint64_t* __restrict__ read_hits, uint32_t* __restrict__ read_over,
                                                                 uint32_t* __restrict__ read_lookups, uint64_t* __restrict__ cnt, const uint64_t* __restrict__ off,
                                                                 uint64_t* __restrict__ hit_word, uint32_t* __restrict__ hit_r)
{
    __shared__ uint64_t lds[3][SEED_BLOCK / 64];
    const uint64_t read = read0 + blockIdx.x;
    const uint32_t L = rd.len[read];
    const uint32_t nr = L >= ix.k ? L - ix.k + 1u : 0u;
    const uint32_t n_lanes = nr * rd.n_strands;
    const uint64_t* const seq = rd.seq + rd.word[read];
    const uint64_t lane0 = rd.lane_off[read] - lane_base;
    uint64_t hits = 0, over = 0, looked = 0;
    for (uint32_t l = threadIdx.x; l < n_lanes; l += SEED_BLOCK) {
        const uint32_t strand = l >= nr ? 1u : 0u, r = strand ? l - nr : l;
        const uint32_t at = seed_window_at(L, ix.k, strand, r);
        uint32_t lo, hi, first = 0, n = 0;
        seed_planes16(seq[at >> 5], seq[(at >> 5) + 1], at & 31u, lo, hi);      // (a read's words end with one of padding)
        const uint32_t key = strand ? seed_key_revcomp(lo, hi, ix.k) : seed_key_forward(lo, hi, ix.k);
        if (seed_key_selected(key, ix.k, ix.smer)) {
            looked++;
            n = seed_entries(ix, key, first);
            if (n > ix.max_occ) {
                n = 0;
                over++;
            }
        }
        if (MODE == 0) hits += n;
        if (MODE == 1) cnt[lane0 + l] = n;
        if (MODE == 2) {
            const uint64_t at_hit = off[lane0 + l];
            for (uint32_t j = 0; j < n; j++) {
                hit_word[at_hit + j] = seed_hit_word((uint64_t)blockIdx.x, strand, ix.pos[first + j], r);
                hit_r[at_hit + j] = r;
            }
        }
    }
    if (MODE == 0) {
        const uint64_t h = seed_block_sum(hits, lds[0]), o = seed_block_sum(over, lds[1]);
        const uint64_t n = ix.smer ? seed_block_sum(looked, lds[2]) : n_lanes;          // (a branch the whole launch takes alike)
        if (threadIdx.x == 0) {
            read_hits[read] = h;
            read_over[read] = (uint32_t)o;
            read_lookups[read] = (uint32_t)n;
        }
    }
}

__global__ __launch_bounds__(SEED_BLOCK) void seed_heads_kernel(const uint64_t* __restrict__ hit_word, uint32_t n_hits, uint32_t band,
                                                                uint32_t* __restrict__ head)
{
    const uint64_t i = (uint64_t)blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (i >= n_hits) return;
    head[i] = i == 0 || seed_is_head(hit_word[i - 1], hit_word[i], band) ? 1u : 0u;
}

// cluster[i]: the inclusive sum of head[]: hit i belongs to cluster cluster[i] - 1.  anchor[]: all ones before the launch.
__global__ __launch_bounds__(SEED_BLOCK) void seed_clusters_kernel(const uint64_t* __restrict__ hit_word, const uint32_t* __restrict__ hit_r,
                                                                   const uint32_t* __restrict__ head, const uint32_t* __restrict__ cluster,
                                                                   uint32_t n_hits, uint32_t* __restrict__ first, unsigned long long* __restrict__ anchor)
{
    const uint64_t i = (uint64_t)blockIdx.x * SEED_BLOCK + threadIdx.x;
    if (i >= n_hits) return;
    const uint32_t c = cluster[i] - 1u;
    if (head[i]) first[c] = (uint32_t)i;
    if (i == n_hits - 1u) first[c + 1u] = n_hits;        // the end of the last cluster
    atomicMin(&anchor[c], (unsigned long long)seed_anchor_word(hit_r[i], seed_hit_dbias(hit_word[i])));
}

// One wavefront per read.  A read's hits are [off[its first lane], off[the next read's first lane]) before AND after the sort (the
// read is the word's top field), and its clusters those of its first and last hit.
__global__ __launch_bounds__(SEED_BLOCK) void seed_pick_kernel(SeedReadsView rd, uint64_t read0, uint64_t n_reads, uint64_t lane_base,
                                                               const uint64_t* __restrict__ off, const uint64_t* __restrict__ hit_word,
                                                               const uint32_t* __restrict__ cluster, const uint32_t* __restrict__ first,
                                                               const unsigned long long* __restrict__ anchor, uint32_t min_hits, uint32_t max_candidates,
                                                               uint32_t* __restrict__ out_n, uint32_t* __restrict__ out_start,
                                                               uint32_t* __restrict__ out_votes, uint8_t* __restrict__ out_strand)
{
    const uint64_t q = (uint64_t)blockIdx.x * (SEED_BLOCK / 64) + (threadIdx.x >> 6);          // read in chunk
    if (q >= n_reads) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t hb = off[rd.lane_off[read0 + q] - lane_base], he = off[rd.lane_off[read0 + q + 1] - lane_base];
    uint32_t c0 = 0, nc = 0;
    if (he > hb) {
        c0 = cluster[hb] - 1u;
        nc = cluster[he - 1] - c0;
    }
    SeedRank last{0, 0};
    bool have_last = false;
    uint32_t n = 0;
    for (; n < max_candidates; n++) {
        SeedRank best{~0ull, ~0ull};
        for (uint32_t c = lane; c < nc; c += 64u) {
            const uint32_t f = first[c0 + c], votes = first[c0 + c + 1u] - f;
            if (votes < min_hits) continue;
            const SeedRank x = seed_rank(votes, seed_anchor_start(anchor[c0 + c]), seed_hit_strand(hit_word[f]), c);
            if ((!have_last || seed_rank_less(last, x)) && seed_rank_less(x, best)) best = x;
        }
        for (int o = 32; o; o >>= 1) {
            const SeedRank y{__shfl_xor(best.hi, o), __shfl_xor(best.lo, o)};
            if (seed_rank_less(y, best)) best = y;
        }
        if (best.hi == ~0ull && best.lo == ~0ull) break;                        // (no rank is all ones: a cluster has at least one vote)
        if (lane == 0) {
            const uint64_t at = q * max_candidates + n;
            out_start[at] = seed_rank_start(best);
            out_votes[at] = seed_rank_votes(best);
            out_strand[at] = (uint8_t)seed_rank_strand(best);
        }
        last = best;
        have_last = true;
    }
    if (lane == 0) out_n[q] = n;
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + SEED_BLOCK - 1) / SEED_BLOCK); }

}  // namespace

uint32_t seed_bucket_bits(uint64_t n_entries, uint32_t k)
{
    uint32_t bits = 8;
    while (bits < 26u && (1ull << bits) < n_entries) bits++;
    return bits < 2u * k ? bits : 2u * k;
}

size_t seed_index_sort_temp_bytes(uint64_t n_entries, uint32_t k)
{
    size_t bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)n_entries, 0, (int)(2u * k), (hipStream_t)0);
    return bytes + 256;
}

uint64_t seed_select_blocks(uint64_t n_positions) { return blocks_for(n_positions); }

size_t seed_select_temp_bytes(uint64_t n_positions)
{
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(seed_select_blocks(n_positions) + 1), (hipStream_t)0);
    return bytes + 256;
}

hipError_t launch_seed_select_count(const uint64_t* genome, uint64_t n_positions, uint32_t k, uint32_t stride, uint32_t smer, uint32_t* block_cnt,
                                    uint32_t* block_base, void* temp, size_t temp_bytes, hipStream_t s)
{
    const uint64_t nb = seed_select_blocks(n_positions);
    hipError_t e;
    // (the word behind the last workgroup's: 0, so that the sum's last word is the total)
    if ((e = hipMemsetAsync(block_cnt + nb, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if (nb) {
        seed_select_count_kernel<<<(unsigned)nb, SEED_BLOCK, 0, s>>>(genome, n_positions, k, stride, smer, block_cnt);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, (const uint32_t*)block_cnt, block_base, (int)(nb + 1), s);
}

hipError_t launch_seed_index(const uint64_t* genome, uint64_t n_entries, uint32_t k, uint32_t stride, uint32_t* keys_tmp, uint32_t* pos_tmp, uint32_t* keys,
                             uint32_t* pos, uint32_t bucket_bits, uint32_t* buckets, void* temp, size_t temp_bytes, hipStream_t s, uint32_t smer,
                             uint64_t n_positions, const uint32_t* block_base)
{
    if (n_entries) {
        if (smer)
            seed_select_emit_kernel<<<blocks_for(n_positions), SEED_BLOCK, 0, s>>>(genome, n_positions, k, stride, smer, block_base, (uint32_t)n_entries, keys_tmp,
                                                                                   pos_tmp);
        else
            seed_index_keys_kernel<<<blocks_for(n_entries), SEED_BLOCK, 0, s>>>(genome, n_entries, k, stride, keys_tmp, pos_tmp);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const uint32_t*)keys_tmp, keys, (const uint32_t*)pos_tmp, pos, (int)n_entries, 0,
                                               (int)(2u * k), s);
        if (e != hipSuccess) return e;
    }
    const uint64_t n_buckets = 1ull << bucket_bits;
    seed_index_buckets_kernel<<<blocks_for(n_buckets + 1), SEED_BLOCK, 0, s>>>(keys, (uint32_t)n_entries, 2u * k - bucket_bits, n_buckets, buckets);
    return hipGetLastError();
}

hipError_t launch_seed_totals(const SeedIndexView& ix, const SeedReadsView& rd, uint64_t read0, uint64_t n_reads, uint64_t* read_hits, uint32_t* read_over,
                              uint32_t* read_lookups, hipStream_t s)
{
    if (!n_reads) return hipSuccess;
    seed_lookup_kernel<0><<<(unsigned)n_reads, SEED_BLOCK, 0, s>>>(ix, rd, read0, 0, read_hits, read_over, read_lookups, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

size_t seed_chunk_temp_bytes(uint64_t n_lanes, uint64_t n_hits, uint64_t n_reads)
{
    size_t a = 0, b = 0, c = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n_lanes + 1), (hipStream_t)0);
    int end_bit = (int)SEED_READ_SHIFT;
    while (end_bit < 64 && (1ull << (end_bit - SEED_READ_SHIFT)) < n_reads) end_bit++;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)n_hits, 0, end_bit, (hipStream_t)0);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, c, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_hits, (hipStream_t)0);
    return std::max(a, std::max(b, c)) + 256;
}

hipError_t launch_seed_chunk(const SeedIndexView& ix, const SeedReadsView& rd, const SeedChunk& ch, hipStream_t s)
{
    hipError_t e;
    // counts per lane (the word behind the last lane: 0, so that the sum's last word is the chunk's total), their exclusive sum
    if ((e = hipMemsetAsync(ch.cnt + ch.n_lanes, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
    seed_lookup_kernel<1><<<(unsigned)ch.n_reads, SEED_BLOCK, 0, s>>>(ix, rd, ch.read0, ch.lane_base, nullptr, nullptr, nullptr, ch.cnt, nullptr, nullptr, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = ch.temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(ch.temp, tb, (const uint64_t*)ch.cnt, ch.off, (int)(ch.n_lanes + 1), s)) != hipSuccess) return e;
    if (ch.n_hits) {
        seed_lookup_kernel<2><<<(unsigned)ch.n_reads, SEED_BLOCK, 0, s>>>(ix, rd, ch.read0, ch.lane_base, nullptr, nullptr, nullptr, nullptr, ch.off, ch.word_tmp, ch.r_tmp);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        int end_bit = (int)SEED_READ_SHIFT;
        while (end_bit < 64 && (1ull << (end_bit - SEED_READ_SHIFT)) < ch.n_reads) end_bit++;
        tb = ch.temp_bytes;
        if ((e = hipcub::DeviceRadixSort::SortPairs(ch.temp, tb, (const uint64_t*)ch.word_tmp, ch.word, (const uint32_t*)ch.r_tmp, ch.r, (int)ch.n_hits, 0,
                                                    end_bit, s)) != hipSuccess)
            return e;
        seed_heads_kernel<<<blocks_for(ch.n_hits), SEED_BLOCK, 0, s>>>(ch.word, (uint32_t)ch.n_hits, ix.band, ch.head);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        tb = ch.temp_bytes;
        if ((e = hipcub::DeviceScan::InclusiveSum(ch.temp, tb, (const uint32_t*)ch.head, ch.cluster, (int)ch.n_hits, s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(ch.anchor, 0xff, ch.n_hits * sizeof(uint64_t), s)) != hipSuccess) return e;
        seed_clusters_kernel<<<blocks_for(ch.n_hits), SEED_BLOCK, 0, s>>>(ch.word, ch.r, ch.head, ch.cluster, (uint32_t)ch.n_hits, ch.first,
                                                                          reinterpret_cast<unsigned long long*>(ch.anchor));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    seed_pick_kernel<<<blocks_for(ch.n_reads * 64), SEED_BLOCK, 0, s>>>(rd, ch.read0, ch.n_reads, ch.lane_base, ch.off, ch.word, ch.cluster, ch.first,
                                                                        reinterpret_cast<const unsigned long long*>(ch.anchor), ix.min_hits, ix.max_candidates,
                                                                        ch.out_n, ch.out_start, ch.out_votes, ch.out_strand);
    return hipGetLastError();
}

}  // namespace scrg
