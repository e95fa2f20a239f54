// site_kernels.hip — the pileup sites (include/scrooge_amd.h: PILEUP SITES): of the finished counts of a pileup, the positions where
// reads disagree with the target or insertions pile up (site_rule.h, shared with the host twin), compacted on the device into
// 40-byte records in position order, so that a consumer brings down the sites and not 28 bytes per base.
//
// Three launches over finished counts, no atomics, the same result in any schedule, no workgroup waits for another:
//   mark   one position per thread and round, SITE_ROUNDS rounds per workgroup: a tile is SITE_TILE = 4096 positions.  A wavefront
//          reads 64 adjacent words of each of the seven planes (256 contiguous bytes per load) and the two or three genome words its
//          positions lie in, evaluates the rule, and its __ballot IS word (position / 64) of the site bitmap; the workgroup's popcount
//          is the tile's count.  This is the one full read of the planes: 28 bytes per position in, 1/8 byte out.
//   scan   ONE workgroup turns the tile counts into what lies in front of every tile (block_scan.h, as the pileup's finish does) and
//          stores the grand total and the rule, which the write pass reads from the scratch.
//   write  every tile reads its 64 bitmap words and its offset, ranks its set bits by popcount prefix, and fetches the seven counts
//          and the reference base for SET positions only; a tile without a site ends after 512 bytes.  Records of rank >= cap are not
//          stored.
// A tile's bitmap words are all written by mark, the ones past the target as 0, so the write pass reads whole tiles.
#include "block_scan.h"
#include "genasm_kernels.h"
#include "host_path.h"
#include "pileup_rule.h"
#include "run_walk.h"
#include "site_rule.h"

namespace scrg {

constexpr uint32_t SITE_THREADS = 256, SITE_WAVES = SITE_THREADS / 64u, SITE_ROUNDS = 16;
constexpr uint32_t SITE_TILE = SITE_THREADS * SITE_ROUNDS, SITE_TILE_WORDS = SITE_TILE / 64u;      // 4096 positions, 64 bitmap words
constexpr uint64_t SITE_HEADER_BYTES = 16;                                                        // the rule, in front of the bitmap
static_assert(SITE_TILE_WORDS == 64u, "the write pass ranks a tile's words with one wavefront scan");
static_assert(sizeof(scrg_site_rule) == SITE_HEADER_BYTES && sizeof(scrg_site) == 40, "the layouts scrooge_amd.h states");

struct SiteArgs {
    const uint32_t* counts;       // [PILE_PLANES][len + 1], counts form
    const uint64_t* seq;          // the target's bases: linear 2-bit packing from base genome_off
    uint64_t genome_off;
    uint64_t len;                 // target_len
};

struct SiteScratch {              // the caller's scratch, cut up
    scrg_site_rule* rule;
    uint64_t* bitmap;             // [n_tiles * SITE_TILE_WORDS]
    uint32_t* tile;               // [n_tiles]: counts after mark, what lies in front of the tile after scan
    uint64_t n_tiles;
};
static uint64_t site_tiles(uint64_t target_len) { return (target_len + SITE_TILE - 1ull) / SITE_TILE; }
static SiteScratch cut_scratch(void* scratch, uint64_t target_len)
{
    SiteScratch s;
    char* const p = static_cast<char*>(scratch);
    s.n_tiles = site_tiles(target_len);
    s.rule = reinterpret_cast<scrg_site_rule*>(p);
    s.bitmap = reinterpret_cast<uint64_t*>(p + SITE_HEADER_BYTES);
    s.tile = reinterpret_cast<uint32_t*>(p + SITE_HEADER_BYTES + s.n_tiles * SITE_TILE_WORDS * sizeof(uint64_t));
    return s;
}

// position g < len: its counts and its reference code
__device__ __forceinline__ uint32_t load_position(const SiteArgs& a, uint64_t g, uint32_t c[PILE_PLANES])
{
    const uint64_t stride = a.len + 1ull;
#pragma unroll
    for (uint32_t pl = 0; pl < PILE_PLANES; pl++) c[pl] = a.counts[pl * stride + g];
    return base_code(a.seq, a.genome_off, 1u, g);
}

// the bitmap word a wavefront has in round k of its tile: the wavefronts of a workgroup take adjacent words
__device__ __forceinline__ uint32_t tile_word(uint32_t k) { return k * SITE_WAVES + (threadIdx.x >> 6); }

__global__ __launch_bounds__(SITE_THREADS) void site_mark_kernel(SiteArgs a, SiteRule rule, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ tile_cnt)
{
    __builtin_amdgcn_s_setprio(3);      // (a helper between align launches: it goes first, see compact_runs_kernel)
    __shared__ uint32_t wave_cnt[SITE_WAVES];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < SITE_ROUNDS; k++) {
        const uint64_t word = (uint64_t)blockIdx.x * SITE_TILE_WORDS + tile_word(k), g = word * 64ull + lane;
        bool site = false;
        if (g < a.len) {
            uint32_t c[PILE_PLANES];
            const uint32_t r = load_position(a, g, c);
            site = site_verdict(rule, c, r).site;
        }
        const uint64_t m = __ballot(site);
        if (lane == 0) bitmap[word] = m;
        mine += (uint32_t)__popcll(m);
    }
    if (lane == 0) wave_cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < SITE_WAVES; w++) all += wave_cnt[w];
        tile_cnt[blockIdx.x] = all;
    }
}

// (a target has fewer than 2^32 - 1 positions: the total fits the 32 bits the scan sums in)
__global__ __launch_bounds__(SCAN_THREADS) void site_scan_kernel(uint32_t* __restrict__ tile, uint64_t n_tiles, scrg_site_rule rule, scrg_site_rule* __restrict__ kept,
                                                                  uint64_t* __restrict__ n_sites)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t wave_tot[SCAN_THREADS / 64u];
    const uint32_t total = block_scan_excl_in_place(tile, n_tiles, wave_tot);
    if (threadIdx.x == 0) {
        *kept = rule;
        *n_sites = total;
    }
}

__global__ __launch_bounds__(SITE_THREADS) void site_write_kernel(SiteArgs a, const scrg_site_rule* __restrict__ kept, const uint64_t* __restrict__ bitmap,
                                                                   const uint32_t* __restrict__ tile_off, uint64_t cap, scrg_site* __restrict__ out)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint64_t words[SITE_TILE_WORDS];
    __shared__ uint32_t before[SITE_TILE_WORDS];      // set bits of the tile in front of each word
    __shared__ uint32_t tile_total;
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < SITE_TILE_WORDS) {
        const uint64_t w = bitmap[(uint64_t)blockIdx.x * SITE_TILE_WORDS + threadIdx.x];
        const uint32_t pc = (uint32_t)__popcll(w), incl = wave_scan_incl(pc, lane);
        words[threadIdx.x] = w;
        before[threadIdx.x] = incl - pc;
        if (threadIdx.x == SITE_TILE_WORDS - 1u) tile_total = incl;
    }
    __syncthreads();
    if (tile_total == 0u) return;
    const SiteRule rule{kept->min_depth, kept->min_alt, kept->min_alt_per_mille};
    const uint64_t first = tile_off[blockIdx.x];
    for (uint32_t k = 0; k < SITE_ROUNDS; k++) {
        const uint32_t wi = tile_word(k);
        const uint64_t w = words[wi];
        if (!((w >> lane) & 1ull)) continue;
        const uint64_t rank = first + before[wi] + (uint32_t)__popcll(w & ((1ull << lane) - 1ull));
        const uint64_t g = ((uint64_t)blockIdx.x * SITE_TILE_WORDS + wi) * 64ull + lane;
        if (rank >= cap || g >= a.len) continue;      // (g: a scratch that mark did not leave must not lead outside the planes)
        uint32_t c[PILE_PLANES];
        const uint32_t r = load_position(a, g, c);
        const SiteVerdict v = site_verdict(rule, c, r);
        scrg_site s;
        s.pos = g;
#pragma unroll
        for (uint32_t pl = 0; pl < PILE_PLANES; pl++) s.counts[pl] = c[pl];
        s.ref = (uint8_t)r;
        s.alt = v.alt;
        s.call = v.call;
        s.flags = v.flags;
        out[rank] = s;
    }
}

size_t site_scratch_bytes(uint64_t target_len)
{
    const uint64_t n_tiles = site_tiles(target_len);
    return (size_t)((SITE_HEADER_BYTES + n_tiles * (SITE_TILE_WORDS * sizeof(uint64_t) + sizeof(uint32_t)) + 7ull) & ~7ull);
}

hipError_t launch_site_mark(uint64_t target_len, const uint32_t* counts, const uint64_t* seq, uint64_t genome_off, const scrg_site_rule& rule, void* scratch,
                            uint64_t* n_sites, hipStream_t s)
{
    const SiteScratch sc = cut_scratch(scratch, target_len);
    if (sc.n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
    const SiteArgs a{counts, seq, genome_off, target_len};
    if (sc.n_tiles)
        hipLaunchKernelGGL(site_mark_kernel, dim3((unsigned)sc.n_tiles), dim3(SITE_THREADS), 0, s, a, SiteRule{rule.min_depth, rule.min_alt, rule.min_alt_per_mille},
                           sc.bitmap, sc.tile);
    hipLaunchKernelGGL(site_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, sc.tile, sc.n_tiles, rule, sc.rule, n_sites);
    return hipGetLastError();
}

hipError_t launch_site_write(uint64_t target_len, const uint32_t* counts, const uint64_t* seq, uint64_t genome_off, void* scratch, uint64_t cap, scrg_site* sites,
                             hipStream_t s)
{
    const SiteScratch sc = cut_scratch(scratch, target_len);
    if (sc.n_tiles > 0x7fffffffull) return hipErrorInvalidValue;
    if (sc.n_tiles == 0 || cap == 0) return hipSuccess;
    const SiteArgs a{counts, seq, genome_off, target_len};
    hipLaunchKernelGGL(site_write_kernel, dim3((unsigned)sc.n_tiles), dim3(SITE_THREADS), 0, s, a, sc.rule, sc.bitmap, sc.tile, cap, sites);
    return hipGetLastError();
}

}  // namespace scrg
