// site_rule.h — the per-position rule of the pileup sites (include/scrooge_amd.h: PILEUP SITES) that the kernels (site_kernels.hip)
// and the host twin (scrg_pileup_sites_from_counts, scrg_io.cpp, which sees nothing of HIP) share: is a position with these seven
// counts and this reference base a site, and what are its alternative allele, its call and its flags.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SCRG_SITE_HD __host__ __device__
#else
#define SCRG_SITE_HD
#endif

namespace scrg {

constexpr uint32_t SITE_DEL = 4, SITE_NONE = 255;                                 // SCRG_SITE_DEL, SCRG_SITE_NONE
constexpr uint32_t SITE_F_NONREF = 1, SITE_F_INS = 2, SITE_F_CALL = 4;            // SCRG_SITE_F_*

struct SiteRule {                 // scrg_site_rule, valid (site_rule_valid)
    uint32_t min_depth, min_alt, per_mille;
};
struct SiteVerdict {
    bool site;
    uint8_t alt, call, flags;
};

SCRG_SITE_HD inline bool site_rule_valid(uint32_t min_depth, uint32_t per_mille, uint32_t reserved)
{
    return min_depth >= 1u && per_mille <= 1000u && reserved == 0u;
}

// x observations of `depth` are enough.  (64 bits: a count is a sum mod 2^32, the depth six of them; x * 1000 stays below 2^45.)
SCRG_SITE_HD inline bool site_passes(const SiteRule& k, uint64_t x, uint64_t depth)
{
    return x >= k.min_alt && x * 1000ull >= (uint64_t)k.per_mille * depth;
}

// c: the position's SCRG_PILE_* counts; r: its reference code, 0..3
SCRG_SITE_HD inline SiteVerdict site_verdict(const SiteRule& k, const uint32_t c[7], uint32_t r)
{
    const uint64_t depth = (uint64_t)c[0] + c[1] + c[2] + c[3] + c[4] + c[5];
    uint64_t n_ref = 0, n_alt = 0;
    uint32_t alt = SITE_NONE;
    for (uint32_t b = 0; b <= SITE_DEL; b++) {
        const uint64_t n = b == SITE_DEL ? (uint64_t)c[5] : (uint64_t)c[1 + b] + (b == r ? (uint64_t)c[0] : 0ull);
        if (b == r) n_ref = n;
        else if (alt == SITE_NONE || n > n_alt) {      // (a tie keeps the smaller code)
            alt = b;
            n_alt = n;
        }
    }
    const uint64_t nonref = depth - n_ref, ins = c[6];
    if (nonref == 0) alt = SITE_NONE;
    const uint32_t call = alt != SITE_NONE && n_alt > n_ref ? alt : r;      // (a tie keeps the reference)
    const bool by_nonref = site_passes(k, nonref, depth), by_ins = site_passes(k, ins, depth);
    SiteVerdict v;
    v.site = depth >= k.min_depth && (by_nonref || by_ins);
    v.alt = (uint8_t)alt;
    v.call = (uint8_t)call;
    v.flags = (uint8_t)((nonref > 0 && by_nonref ? SITE_F_NONREF : 0u) | (ins > 0 && by_ins ? SITE_F_INS : 0u) | (call != r ? SITE_F_CALL : 0u));
    return v;
}

}  // namespace scrg
