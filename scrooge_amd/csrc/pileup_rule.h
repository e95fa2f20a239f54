// pileup_rule.h — the per-run rule of the pileup (include/scrooge_amd.h: PILEUP) that the kernel (pileup_kernels.hip) and the host
// twin (scrg_pileup_from_runs, scrg_io.cpp, which sees nothing of HIP) share: which plane a run counts in, where a stretch of
// '=' or 'D' columns begins and ends, what is one insertion, and what lies outside the target.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SCRG_PILE_HD __host__ __device__
#else
#define SCRG_PILE_HD
#endif

namespace scrg {

constexpr uint32_t PILE_MATCH = 0, PILE_BASE = 1, PILE_DEL = 5, PILE_INS = 6, PILE_PLANES = 7;      // SCRG_PILE_*

// the target position of text column t of a pair that starts at `start` (a start near 2^64 saturates: it lies outside every target)
SCRG_PILE_HD inline uint64_t pile_pos(uint64_t start, uint64_t t)
{
    const uint64_t g = start + t;
    return g < start ? ~0ull : g;
}
// '=' and 'D' columns are counted by stretch: directly adjacent runs of the same operation (what a window seam leaves) are one
SCRG_PILE_HD inline bool pile_stretch_op(uint32_t op) { return op == '=' || op == 'D'; }
SCRG_PILE_HD inline uint32_t pile_stretch_plane(uint32_t op) { return op == '=' ? PILE_MATCH : PILE_DEL; }
// a run of `op` behind a run of `prev` (0: none): does it begin a stretch / does it end the stretch in front of it (op 0: the end
// of the pair) / is it an insertion event (directly adjacent I runs are ONE insertion)
SCRG_PILE_HD inline bool pile_opens(uint32_t op, uint32_t prev) { return pile_stretch_op(op) && prev != op; }
SCRG_PILE_HD inline bool pile_closes(uint32_t op, uint32_t prev) { return pile_stretch_op(prev) && prev != op; }
SCRG_PILE_HD inline bool pile_ins_event(uint32_t op, uint32_t prev) { return op == 'I' && prev != 'I'; }
// c columns from position g: does one of them lie outside a target of `len` positions; an insertion in front of position g
SCRG_PILE_HD inline bool pile_columns_outside(uint64_t g, uint32_t c, uint64_t len) { return c != 0u && (g >= len || len - g < c); }
SCRG_PILE_HD inline bool pile_ins_outside(uint64_t g, uint64_t len) { return g > len; }

}  // namespace scrg
