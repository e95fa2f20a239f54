// Host build of scrooge_amd/csrc/launch_grid.h (g++): C entry points for tests/walk_geometry.py, which sizes the batches of
// tests/test_walk_geometry_gpu.py from the arithmetic the launchers run.  Every function returns the workgroups of the launch
// (256 threads: four wavefronts each).
#include <stdint.h>
#include "launch_grid.h"

using namespace scrg;

extern "C" {
uint64_t lg_group_grid(uint64_t n, int n_cus, uint32_t* split) { return group_grid(n, n_cus, split); }
uint64_t lg_compact_runs_grid(uint64_t n, int n_cus, uint32_t* split) { return compact_runs_grid(n, n_cus, split); }
uint64_t lg_compact_runs_packed_grid(uint64_t n, int n_cus) { return compact_runs_packed_grid(n, n_cus); }
uint64_t lg_unpack_runs_grid(uint64_t n_runs, int n_cus) { return unpack_runs_grid(n_runs, n_cus); }
uint64_t lg_pack_planar_grid(uint64_t n_words, int n_cus) { return pack_planar_grid(n_words, n_cus); }
uint64_t lg_pack_planar_groups_items(uint64_t n_rows, uint64_t words_per_row) { return pack_planar_groups_items(n_rows, words_per_row); }
uint64_t lg_pack_planar_groups_grid(uint64_t n_out, int n_cus) { return pack_planar_groups_grid(n_out, n_cus); }
}
