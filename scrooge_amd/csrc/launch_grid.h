// launch_grid.h — the grid arithmetic of the kernels that take their work in a loop over a capped grid, stated once: how many
// workgroups a launcher starts for n items on a GPU of n_cus compute units, and how many wavefronts share a group of 64 pairs.
// Plain C++ with no HIP include: the launchers call these functions, and tests/proto/launch_grid_host.cpp compiles the same header
// for the host, so that the tests derive their batch sizes — one per `split`, and one past the cap, where the loops take a
// second and a third trip — from the arithmetic the library runs (tests/walk_geometry.py, tests/test_walk_geometry.py).
//
// All kernels here run workgroups of 256 threads: four wavefronts.
#pragma once

#include <stdint.h>

namespace scrg {

// Kernels that take pairs in groups of 64 (run_walk.h: for_each_group): about sixteen wavefronts per CU; a batch with fewer
// groups than that lets `split` (a power of two, up to 64) wavefronts share a group.  (More than twice the target only without
// a split, so the wavefronts are always whole sets of `split`.)  Capped at 2 * 16 * n_cus wavefronts: above
// 64 * 2 * 16 * n_cus pairs a wavefront takes more than one group.
inline uint64_t group_grid(uint64_t n, int n_cus, uint32_t* split)
{
    const uint64_t groups = (n + 63) / 64, target_waves = (uint64_t)n_cus * 16;
    uint64_t sp = 1;
    while (sp < 64 && groups * sp * 2 <= target_waves) sp *= 2;
    uint64_t waves = groups * sp;
    if (waves > target_waves * 2) waves = target_waves * 2;
    *split = (uint32_t)sp;
    return (waves + 3) / 4;
}

// compact_runs_kernel (seq_kernels.hip): groups of 64 pairs; up to 8 wavefronts share a group while there are fewer groups than
// the GPU has room for.  Capped at n_cus * 8 workgroups; n_pairs > 0.
inline uint64_t compact_runs_grid(uint64_t n_pairs, int n_cus, uint32_t* split_out)
{
    const uint64_t groups = (n_pairs + 63) / 64, room = (uint64_t)n_cus * 32;
    uint32_t split = 1;
    while (split < 8 && groups * split * 2 <= room) split *= 2;
    uint64_t blocks = (groups * split + 3) / 4;                  // four wavefronts per workgroup
    const uint64_t cap = (uint64_t)n_cus * 8;
    if (blocks > cap) blocks = cap;
    if (split == 8 && (blocks & 1)) blocks++;                    // (the wavefronts of a launch: a multiple of `split`)
    *split_out = split;
    return blocks;
}

// compact_runs_packed_kernel: one wavefront per pair, capped at n_cus * 8 workgroups; n_pairs > 0
inline uint64_t compact_runs_packed_grid(uint64_t n_pairs, int n_cus)
{
    uint64_t blocks = (n_pairs + 3) / 4;
    const uint64_t cap = (uint64_t)n_cus * 8;
    if (blocks > cap) blocks = cap;
    return blocks;
}

// unpack_runs_kernel: one thread per four runs, at least one workgroup, capped at n_cus * 16; n_runs > 0
inline uint64_t unpack_runs_grid(uint64_t n_runs, int n_cus)
{
    uint64_t blocks = ((n_runs >> 2) + 255) / 256;
    if (blocks < 1) blocks = 1;
    const uint64_t cap = (uint64_t)n_cus * 16;
    if (blocks > cap) blocks = cap;
    return blocks;
}

// pack_planar_kernel: one thread per word of 32 bases, capped at n_cus * 32 workgroups; n_words > 0
inline uint64_t pack_planar_grid(uint64_t n_words, int n_cus)
{
    uint64_t blocks = (n_words + 255) / 256;
    const uint64_t cap = (uint64_t)n_cus * 32;
    if (blocks > cap) blocks = cap;
    return blocks;
}

// pack_planar_groups_kernel: a thread takes two words of a row, rows in whole groups of 64 -> the threads' items (0: no launch)
inline uint64_t pack_planar_groups_items(uint64_t n_rows, uint64_t words_per_row)
{
    return ((n_rows + 63) / 64) * 64 * ((words_per_row + 1) / 2);
}
// ... and its workgroups, capped at n_cus * 32; n_out > 0
inline uint64_t pack_planar_groups_grid(uint64_t n_out, int n_cus)
{
    uint64_t blocks = (n_out + 255) / 256;
    const uint64_t cap = (uint64_t)n_cus * 32;
    if (blocks > cap) blocks = cap;
    return blocks;
}

}  // namespace scrg
