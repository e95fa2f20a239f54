"""(CPU) What tests/test_walk_geometry_gpu.py stands on, so that it cannot pass vacuously: the grid arithmetic of
scrooge_amd/csrc/launch_grid.h (compiled for the host) against a literal restatement; the batch sizes derived from it, which at
256 CUs must reach every `split`, two and three trips of the group loop, long pairs and tile pairs in the later trips, and every
counted sort of pair; and the distinct pairs of tests/walk_geometry.py against their models."""
import numpy as np
import pytest

from tests import walk_geometry as wg

MI355X_CUS = 256


# ---------------------------------------------------------------------------------------------------------------
# the header against a literal restatement
# ---------------------------------------------------------------------------------------------------------------
def lit_group_grid(n, n_cus):
    groups, target = (n + 63) // 64, 16 * n_cus
    split = 1
    while split < 64 and groups * split * 2 <= target:
        split *= 2
    return (min(groups * split, 2 * target) + 3) // 4, split


def lit_compact_runs_grid(n, n_cus):
    groups, room = (n + 63) // 64, 32 * n_cus
    split = 1
    while split < 8 and groups * split * 2 <= room:
        split *= 2
    blocks = min((groups * split + 3) // 4, 8 * n_cus)
    return blocks + (split == 8 and blocks % 2), split


def class_borders(lit, n_cus):
    """The smallest n of every split class, the first n the cap cuts, and the first of a third trip"""
    out = [1]
    for g in range(2, 40 * n_cus + 2):
        if lit(64 * g, n_cus)[1] != lit(64 * (g - 1), n_cus)[1]:
            out.append(64 * (g - 1) + 1)
    cap = lit(1 << 40, n_cus)[0] * 4
    return out + [64 * cap + 1, 64 * 2 * cap + 1]


def sweep(lit, n_cus):
    ns = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1 << 18, (1 << 22) - 1, 1 << 22, 1 << 32, (1 << 40) + 17}
    for b in class_borders(lit, n_cus):
        ns |= {max(b + d, 0) for d in (-65, -64, -2, -1, 0, 1, 63, 64)}
    rng = np.random.Generator(np.random.PCG64(41 + n_cus))
    ns |= {int(x) for x in rng.integers(0, 70 * 64 * n_cus, size=300)}
    return sorted(ns)


@pytest.mark.parametrize("n_cus", wg.CU_COUNTS)
def test_header_is_the_literal_arithmetic(n_cus):
    for n in sweep(lit_group_grid, n_cus):
        assert wg.group_grid(n, n_cus) == lit_group_grid(n, n_cus), n
    for n in sweep(lit_compact_runs_grid, n_cus):
        if n:                                           # (the launchers return before the arithmetic for an empty batch)
            assert wg.compact_runs_grid(n, n_cus) == lit_compact_runs_grid(n, n_cus), n
    for n in sweep(lit_group_grid, n_cus):
        if n == 0:
            continue
        assert wg.compact_runs_packed_grid(n, n_cus) == min((n + 3) // 4, 8 * n_cus), n
        assert wg.unpack_runs_grid(n, n_cus) == min(max(((n >> 2) + 255) // 256, 1), 16 * n_cus), n
        assert wg.pack_planar_grid(n, n_cus) == min((n + 255) // 256, 32 * n_cus), n
        for wpr in (1, 2, 5):
            items = (n + 63) // 64 * 64 * ((wpr + 1) // 2)
            assert wg.pack_planar_groups_grid(n, wpr, n_cus) == (items, min((items + 255) // 256, 32 * n_cus)), (n, wpr)
    assert wg.pack_planar_groups_grid(0, 3, n_cus) == (0, 0) == wg.pack_planar_groups_grid(5, 0, n_cus)


@pytest.mark.parametrize("n_cus", wg.CU_COUNTS)
def test_wavefronts_are_whole_sets_of_split(n_cus):
    """The kernels divide the launch's wavefronts by `split`: none may be left over that would take groups with a partner missing,
    and every group must have its wavefront set."""
    for grid, lit in ((wg.group_grid, lit_group_grid), (wg.compact_runs_grid, lit_compact_runs_grid)):
        for n in sweep(lit, n_cus):
            if n == 0:
                continue
            blocks, split = grid(n, n_cus)
            waves, groups = 4 * blocks, (n + 63) // 64
            taking = waves // split
            assert blocks >= 1 and split in (1, 2, 4, 8, 16, 32, 64) and taking >= 1, n
            # the wavefronts past the last whole set: only those the rounding to a workgroup added, and they must find no group
            assert waves % split == 0 or (waves % split < 4 and taking >= groups), (n, blocks, split)
            assert split == 1 or taking >= groups, n                  # a split launch takes one trip


# ---------------------------------------------------------------------------------------------------------------
# the sizes the GPU tests derive, at the MI355X's CU count
# ---------------------------------------------------------------------------------------------------------------
def test_sizes_reach_every_regime():
    cat = wg.catalog()
    sizes = wg.group_sizes(MI355X_CUS)
    assert set(sizes) == {"split%d" % s for s in (64, 32, 16, 8, 4, 2, 1)} | {"trips"}
    for name, n in sizes.items():
        assert 0 < n <= wg.MAX_PAIRS and n % 64 != 0, name
        _, split = wg.group_grid(n, MI355X_CUS)
        assert split == (1 if name == "trips" else int(name[5:])), name
        idx, shift, cap_out = wg.batch_index(n)
        assert wg.total_runs(idx) <= wg.MAX_RUNS, name
        long = wg.long_per_group(idx)
        assert len(long) == (n + 63) // 64
        if split in (2, 4):
            assert (long[:-1] > split).all(), name                    # more long pairs than wavefronts: some take two
        if split >= 16:
            assert (long < split).all() and long.min() >= 1 and (long[:-1] >= 6).all(), name      # fewer: some wavefronts of a set take none
        assert cap_out.sum() >= 1 and (cat.cnt[idx] == wg.TILE_RUNS + 1).any(), name
        if n > wg.TILE_PERIOD + wg.TILE_AT:
            assert (cat.cnt[idx] == 2 * wg.TILE_RUNS + 1).any(), name
    assert sizes["split64"] < 64 < sizes["split32"]                   # one group that is not full; more than one group
    # the large batch: two whole trips and a part of a third
    n = sizes["trips"]
    t = wg.trips(wg.group_grid, n, MI355X_CUS)
    assert set(t.tolist()) == {2, 3} and 1.04e6 < n < 1.07e6
    n_waves, _ = wg.group_waves(wg.group_grid, n, MI355X_CUS)
    assert n_waves == 2 * 16 * MI355X_CUS
    idx, shift, cap_out = wg.batch_index(n)
    trip_of_pair = (np.arange(n) // 64) // n_waves
    for trip in (1, 2):
        here = idx[trip_of_pair == trip]
        assert (cat.cnt[here] > wg.LANE_MAX_RUNS).sum() > 100 and (wg.long_per_group(here) > 0).all(), trip
        assert {wg.TILE_RUNS + 1, 2 * wg.TILE_RUNS + 1} <= set(cat.cnt[here].tolist()), trip
        assert all(v > 0 for v in cat.multiplicity(here, cap_out[trip_of_pair == trip]).values()), trip
    assert all(v > 0 for v in cat.multiplicity(idx, cap_out).values())
    # every distinct pair meets every lane
    assert len(set(zip((np.arange(n) % 64).tolist(), idx.tolist()))) >= 64 * wg.D


def test_compaction_sizes_reach_every_regime():
    cat = wg.catalog()
    sizes = wg.compact_sizes(MI355X_CUS)
    assert set(sizes) == {"split8", "split4", "split2", "split1", "trips"}
    for name, n in sizes.items():
        assert 0 < n <= wg.MAX_PAIRS and n % 64 != 0, name
        assert wg.compact_runs_grid(n, MI355X_CUS)[1] == (1 if name == "trips" else int(name[5:])), name
        idx, _, _ = wg.batch_index(n)
        long = wg.long_per_group(idx, wg.COMPACT_LANE_MAX_RUNS)
        assert long.min() >= 1 and (name not in ("split2", "split4") or (long[:-1] > int(name[5:])).all()), name
    n = sizes["trips"]
    assert set(wg.trips(wg.compact_runs_grid, n, MI355X_CUS).tolist()) == {2, 3}
    assert {0, 1, 16, 17} <= set(cat.cnt.tolist())                    # both sides of the compaction's own threshold
    # compact_runs_packed: one wavefront per pair, three trips and five pairs
    n = wg.packed_size(MI355X_CUS)
    waves = 4 * wg.compact_runs_packed_grid(n, MI355X_CUS)
    assert n == 3 * waves + 5 and n <= wg.MAX_PAIRS
    # unpack_runs on the large batch's run total: more than one trip of its grid, four runs per thread
    total = wg.total_runs(wg.batch_index(wg.group_sizes(MI355X_CUS)["trips"])[0])
    assert total > 4 * 256 * wg.unpack_runs_grid(total, MI355X_CUS) and total <= wg.MAX_RUNS


@pytest.mark.parametrize("n_cus", wg.CU_COUNTS)
def test_sizes_on_other_devices(n_cus):
    """Whatever the CU count: every size is in range, of the class it is named for, and "trips" takes two and three trips."""
    for sizes, grid in ((wg.group_sizes(n_cus), wg.group_grid), (wg.compact_sizes(n_cus), wg.compact_runs_grid)):
        assert "trips" in sizes and "split1" in sizes
        for name, n in sizes.items():
            assert 0 < n <= wg.MAX_PAIRS and grid(n, n_cus)[1] == (1 if name == "trips" else int(name[5:])), name
        assert set(wg.trips(grid, sizes["trips"], n_cus).tolist()) == {2, 3}
        assert wg.total_runs(wg.batch_index(sizes["trips"])[0]) <= wg.MAX_RUNS


# ---------------------------------------------------------------------------------------------------------------
# the distinct pairs
# ---------------------------------------------------------------------------------------------------------------
def test_distinct_pairs_hold_what_the_batches_need():
    cat = wg.catalog()
    assert cat.n == wg.D + 2 and np.gcd(wg.D, 64) == 1 and np.gcd(wg.STEP, wg.D) == 1
    counts = set(cat.cnt[:wg.D].tolist())
    assert {0, 1, 16, 17, 24, 25, 40, 300} <= counts
    assert (cat.cnt[:wg.D] > wg.LANE_MAX_RUNS).sum() >= 6
    assert cat.cnt[wg.D:].tolist() == [513, 1025]
    assert cat.read_rev.sum() >= 10 and cat.read_rev[wg.D + 1] and not cat.read_rev[wg.D]
    assert (cat.tl >= 0).all() and (cat.rl >= 0).all()
    sort = np.array(cat.sort)
    for s in wg.COUNTED_SORTS[:-1]:                                   # every counted sort on the lane walk and on the wavefront walk
        c = cat.cnt[sort == s]
        assert (c <= wg.LANE_MAX_RUNS).any() and (c > wg.LANE_MAX_RUNS).any(), s


def test_models_accept_the_pairs_and_tell_neighbours_apart():
    from tests import clip_model as clm, diff_model as dm, pileup_model as pm, report_model as rm
    cat = wg.catalog()
    sort = np.array(cat.sort)
    # what each sort is for, by the models
    v = np.array([r["verdict"] for r in cat.report])
    assert (v[sort == "ok"] == 0).all() and (v[sort == "outside"] == 0).all()
    assert sorted(v[sort == "bad_run"].tolist()) == [1, 2] and (v[sort == "over_text"] == 4).all() and (v[sort == "over_read"] == 3).all()
    assert (v[sort == "status"] == rm.NO_ALIGNMENT).all() and cat.report_fail.sum() == 6
    for k in range(cat.n):
        if sort[k] in ("ok", "outside", "status"):
            assert dm.apply_cs(cat.text[k], cat.diff_strings["cs"][k]) == (cat.read[k], dm.consumed(cat.runs[k])[0]), k
            assert not cat.runs[k] or dm.md_text_consumed(cat.diff_strings["md"][k]) == dm.consumed(cat.runs[k])[0], k
            assert clm.model(cat.runs[k]) == clm.brute(cat.runs[k]) or cat.cnt[k] > 400, k
        if cat.pile_counted[k]:
            for s in (0, wg.START_SHIFTS - 1):
                start = int(cat.start[k]) + s * wg.START_SHIFT
                a, out_a = pm.model(cat.runs[k], cat.read[k], start, wg.TARGET_LEN)
                b, out_b = pm.brute(cat.runs[k], cat.read[k], start, wg.TARGET_LEN)
                assert np.array_equal(a, b) and out_a == out_b == bool(cat.pile_outside[k, s]) == (sort[k] == "outside"), k
    assert cat.diff_bad.sum() == 6 and all(b.sum() == (0 if f == "windowed" else 2) for f, b in cat.text_bad.items())
    assert (~cat.clip_touched).sum() == 4 and cat.pile_counted.sum() == cat.n - 7
    # neighbours in the list and in a batch (STEP apart) never share an answer: a pair that was given another's is a mismatch
    for k in range(wg.D):
        for j in ((k + 1) % wg.D, (k + wg.STEP) % wg.D, wg.D, wg.D + 1):
            for form in wg.FORMS:
                assert cat.text_strings[form][k] != cat.text_strings[form][j], (form, k, j)
            for kind in wg.KINDS:
                assert cat.diff_strings[kind][k] != cat.diff_strings[kind][j], (kind, k, j)
            assert cat.report[k] != cat.report[j] and cat.clip[k] != cat.clip[j], (k, j)
            assert cat.start[k] != cat.start[j]


def test_batch_arrays():
    cat = wg.catalog()
    n = 5000
    idx, shift, cap_out = wg.batch_index(n)
    assert idx[:4].tolist() == [0, 7, 14, 21] and idx[wg.TILE_AT] == wg.D and idx[wg.TILE_PERIOD + wg.TILE_AT] == wg.D + 1
    assert cap_out.sum() == 2 and cap_out[wg.CAP_AT] and cap_out[wg.CAP_PERIOD + wg.CAP_AT]
    desc = cat.descriptors(idx)
    assert desc.shape == (n, 6) and desc.dtype == np.uint64
    lens = cat.text_cat["windowed"][0][idx]
    told, off, total = wg.segments(lens, cap_out)
    assert (told[cap_out] > total).all() and np.array_equal(told[~cap_out], off[~cap_out])
    assert off[0] == 2 and (off[1:] >= off[:-1] + lens[:-1]).all() and off[-1] + lens[-1] <= total - 5
    want, outside, counted = cat.pileup_expected(idx, shift)
    assert want.max() < 2 ** 31 and outside > 0 and counted == int(cat.pile_counted[idx].sum())
    runs = np.random.Generator(np.random.PCG64(3)).integers(0, 256, size=1000).astype(np.uint8)
    assert np.array_equal(wg.run_to_byte(wg.byte_to_run(runs)), runs)
    assert wg.byte_to_run([0x45, 0xC3]).tolist() == [(ord("X") << 8) | 5, (ord("D") << 8) | 3]


# ---------------------------------------------------------------------------------------------------------------
# the host calls of the text kernels that have no device entry point
# ---------------------------------------------------------------------------------------------------------------
def test_host_calls_plan_chunks_of_three_split_classes(oracle):
    """scrg_host_plan_mapping (no GPU): the three call sizes' chunks fall into three `split` classes between 32 and 2, in both
    modes; the distinct (read, candidate) pairs hold short and long alignments, winners and losers."""
    hc = wg.host_catalog(oracle)
    assert (hc.cnt <= wg.LANE_MAX_RUNS).sum() >= 40 and (hc.cnt > wg.LANE_MAX_RUNS).sum() >= 12 and hc.cnt.max() < wg.TILE_RUNS
    assert hc.wins.reshape(-1, 2).sum(axis=1).tolist() == [1] * wg.D and hc.wins[1::2].any()
    for mode in ("all", "best"):
        for name, (lens, _, _) in hc.strings[mode].items():
            assert ((lens > 1) == (hc.wins | (mode == "all"))).all(), (mode, name)
    for best in (False, True):
        plan = dict(best=best, sort_by_length=int(best))
        seen = set()
        for split in wg.HOST_SPLITS:
            n_reads = wg.host_call_reads(hc, MI355X_CUS, split, **plan)
            classes = wg.host_chunk_classes(hc, n_reads, MI355X_CUS, **plan)
            assert classes.count(split) >= 2 and 2 * n_reads <= wg.MAX_PAIRS, (best, split)
            seen |= set(classes)
        assert len(seen & {32, 16, 8, 4, 2}) >= 3, best
