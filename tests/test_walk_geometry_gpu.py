"""The per-pair output passes at every launch geometry (scrooge_amd/csrc/run_walk.h: for_each_group on a grid of
launch_grid.h's group_grid; seq_kernels.hip: the run compaction's own copy of the loop): one batch per `split` 64 .. 1, each with a
last group that is not full, and one on which the capped grid takes two whole trips and a part of a third — through the
device-pointer entry points, the only way to more than 2^18 pairs per launch.

The batches, their sizes (from the device's CU count through the host build of launch_grid.h) and the expected outputs are those
of tests/walk_geometry.py: 63 distinct pairs laid out by index, the Python models' answers indexed the same way.  Every pair and
every byte is compared — lengths, rendered bytes with a canary outside every segment, records, rewritten offsets, all planes, and
the exact value of every counter.  Outputs are filled with sentinels before each call: a pair nobody took shows as a sentinel.
The index plumbing of the expectations (gathers by idx, the ragged scatter of the 63 strings) runs in torch on the device; no
kernel of the library has a part in it.  tests/test_walk_geometry.py (CPU) holds what this file relies on.

`counted` of the pileup is not compared here: scrg_pileup_add has no such counter, only the host path's launch does."""
import time

import numpy as np
import pytest

from tests import pileup_model as pm
from tests import walk_geometry as wg
from tests.test_edit_limit import ragged_mismatch

GROUP_SIZES = ["split64", "split32", "split16", "split8", "split4", "split2", "split1", "trips"]
COMPACT_SIZES = ["split8", "split4", "split2", "split1", "trips"]
REC_CANARY = 0x5A5A5A5A
GUARD = 64


# ---------------------------------------------------------------------------------------------------------------
# the device's copy of the catalog, and a batch
# ---------------------------------------------------------------------------------------------------------------
class Device:
    def __init__(self, al):
        import torch
        self.al = al
        self.dev = torch.device("cuda", al.device)
        al.set_stream(0)
        self.n_cus = al.query_launch()["n_cus"]
        self.group_sizes = wg.group_sizes(self.n_cus)
        self.compact_sizes = wg.compact_sizes(self.n_cus)
        cat = self.cat = wg.catalog()
        self.seq = self.to(cat.words.view(np.int64))
        self.dense_tab = self.to(cat.dense_tab)
        # (the compaction's 16-byte loads of an odd destination read one dword past a pair's last run: room behind the last slice)
        self.slice_tab = self.to(np.concatenate([cat.slice_tab, np.zeros((GUARD, 2), np.uint8)]))
        self.batch = None

    def to(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def size(self, table, name):
        if name not in table:
            pytest.skip("a device of %d CUs has no launch of class %s" % (self.n_cus, name))
        return table[name]

    def get_batch(self, n):
        self.al.set_stream(0)
        if self.batch is None or self.batch.n != n:
            self.batch = None
            self.batch = Batch(self, n)
        return self.batch


class Batch:
    """n pairs by index: what every pass takes of them, on the device.  Nothing here is written by a pass: a test that lets one
    write (clip with apply) works on clones."""

    def __init__(self, d, n):
        cat = d.cat
        self.n = n
        self.idx, self.shift, self.cap_out = wg.batch_index(n)
        assert n <= wg.MAX_PAIRS and wg.total_runs(self.idx) <= wg.MAX_RUNS
        self.idx_t = d.to(self.idx)
        self.desc = d.to(cat.descriptors(self.idx).view(np.int64))
        self.cnt = cat.cnt[self.idx]
        self.n_runs = d.to(self.cnt.astype(np.int32))
        self.dense_first = d.to(cat.dense_first[self.idx].astype(np.int64))

    def runs_of(self, d, stride):
        """-> (runs, run_offset, pairs) as the entry points take them: stride 6 the slices behind the descriptors, 1 the dense table"""
        return (d.slice_tab, None, self.desc) if stride == 6 else (d.dense_tab, self.dense_first, self.desc)


@pytest.fixture(scope="module")
def dev(aligner):
    d = Device(aligner)
    yield d
    d.batch = None


@pytest.fixture(autouse=True)
def wall_time_and_peak_memory(request):
    """Prints what DESIGN.md (Launch geometry) quotes: a test's wall time and its peak device memory."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("\n[walk geometry] %s: %.2f s, peak device memory %.0f MiB" % (request.node.name, time.perf_counter() - t0, peak / 2**20))
    assert peak < 4 << 30


def first_row_that_differs(got, want):
    import torch
    rows = torch.nonzero((got != want).reshape(len(got), -1).any(dim=1))
    return int(rows[0]) if len(rows) else None


def same_rows(got, want, b, what):
    """Two device tensors with a row per pair"""
    import torch
    if not torch.equal(got, want):
        p = first_row_that_differs(got, want)
        n_bad = int((got != want).reshape(len(got), -1).any(dim=1).sum())
        raise AssertionError("%s: %d of %d pairs differ, first pair %d (distinct pair %d, %d runs): got %r want %r" % (
            what, n_bad, b.n, p, b.idx[p], b.cnt[p], got[p].cpu().tolist(), want[p].cpu().tolist()))


def ragged_expected(d, total, fill, dtype, lens, off, src, table, chunk=1 << 17):
    """A buffer of `total` elements of `fill` with table[src[p] : src[p] + lens[p]] at off[p] for every pair p (numpy arrays of n;
    table: a device tensor) — on the device, in chunks of pairs, no loop over pairs"""
    import torch
    exp = torch.full((total,), fill, dtype=dtype, device=d.dev)
    for a in range(0, len(lens), chunk):
        ln = d.to(lens[a:a + chunk].astype(np.int64))
        tot = int(ln.sum())
        if tot == 0:
            continue
        within = torch.arange(tot, dtype=torch.int64, device=d.dev) - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln)
        exp[torch.repeat_interleave(d.to(off[a:a + chunk].astype(np.int64)), ln) + within] = \
            table[torch.repeat_interleave(d.to(src[a:a + chunk].astype(np.int64)), ln) + within]
    return exp


def same_buffer(got, exp, b, lens, off, src, table, what):
    """Every element of a rendered buffer; on a difference: which pairs' segments differ (ragged_mismatch), or that the
    difference lies outside every segment"""
    import torch
    if torch.equal(got, exp):
        return
    at = int(torch.nonzero(got != exp)[0])
    pairs = ragged_mismatch(got.cpu().numpy(), off, table.cpu().numpy(), src, lens)
    if len(pairs) == 0:
        raise AssertionError("%s: element %d, outside every pair's segment (or in one that must stay unwritten), was written" % (what, at))
    p = int(pairs[0])
    raise AssertionError("%s: %d of %d pairs differ, first pair %d (distinct pair %d, %d runs) at element %d: got %r want %r" % (
        what, len(pairs), b.n, p, b.idx[p], b.cnt[p], at, got[off[p]:off[p] + min(lens[p], 60)].cpu().tolist(),
        table[src[p]:src[p] + min(lens[p], 60)].cpu().tolist()))


def render_and_check(d, b, strings, bad_d, lengths, render, what):
    """A length pass, the offsets made here, a render pass: the lengths, every byte of the text buffer and the bad count.
    strings: (lengths incl. NUL, bytes, where each begins) of the distinct pairs; lengths(out), render(len, off, buf, bad): the calls."""
    import torch
    lens_d, bytes_d, src_d = strings
    got_len = torch.full((b.n,), -7, dtype=torch.int64, device=d.dev)
    lengths(got_len)
    torch.cuda.synchronize()
    same_rows(got_len, d.to(lens_d)[b.idx_t], b, what + ": lengths")
    lens, src = lens_d[b.idx], src_d[b.idx]
    told, off, total = wg.segments(lens, b.cap_out)
    buf = torch.full((total,), wg.CANARY, dtype=torch.uint8, device=d.dev)
    bad = torch.full((3,), 1000, dtype=torch.int32, device=d.dev)
    render(got_len, d.to(told.astype(np.int64)), buf, bad[1:])
    torch.cuda.synchronize()
    table = d.to(bytes_d)
    written = np.where(b.cap_out, 0, lens)                            # a segment outside the capacity: counted, nothing written
    same_buffer(buf, ragged_expected(d, total, wg.CANARY, torch.uint8, written, off, src, table), b, written, off, src, table, what + ": bytes")
    assert bad.cpu().tolist() == [1000, 1000 + int(bad_d[b.idx].sum()) + int(b.cap_out.sum()), 1000], what + ": bad count"


# ---------------------------------------------------------------------------------------------------------------
# the CIGAR text and the difference strings
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("form", wg.FORMS)
@pytest.mark.parametrize("size", GROUP_SIZES)
def test_cigar_text(dev, size, form, stride):
    b = dev.get_batch(dev.size(dev.group_sizes, size))
    runs, ro, pairs = b.runs_of(dev, stride)
    al = dev.al
    render_and_check(dev, b, dev.cat.text_cat[form], dev.cat.text_bad[form],
                     lambda out: al.cigar_text_lengths(form, b.n, runs, ro, stride, b.n_runs, out, pairs=pairs),
                     lambda ln, off, buf, bad: al.cigar_text_render(form, b.n, runs, ro, stride, b.n_runs, ln, off, buf, bad, pairs=pairs),
                     "cigar text %s stride %d, %s (%d pairs)" % (form, stride, size, b.n))


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("kind", wg.KINDS)
@pytest.mark.parametrize("size", GROUP_SIZES)
def test_diff_strings(dev, size, kind, stride):
    b = dev.get_batch(dev.size(dev.group_sizes, size))
    runs, ro, pairs = b.runs_of(dev, stride)
    al = dev.al
    kw = dict(text_stride_words=1, read_stride_words=1, stranded=1)
    render_and_check(dev, b, dev.cat.diff_cat[kind], dev.cat.diff_bad,
                     lambda out: al.diff_lengths(kind, b.n, dev.seq, pairs, runs, ro, stride, b.n_runs, out, **kw),
                     lambda ln, off, buf, bad: al.diff_render(kind, b.n, dev.seq, pairs, runs, ro, stride, b.n_runs, ln, off, buf, bad, **kw),
                     "diff %s stride %d, %s (%d pairs)" % (kind, stride, size, b.n))


# ---------------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------------
def check_report(d, al, b, stride, what, **kw):
    import torch
    cat = d.cat
    runs, ro, pairs = b.runs_of(d, stride)
    rep = torch.full((b.n + 3, 8), REC_CANARY, dtype=torch.int32, device=d.dev)
    fail = torch.full((3,), 1000, dtype=torch.int32, device=d.dev)
    al.set_stream(0)
    al.report_device(b.n, d.seq, pairs, runs, ro, stride, b.n_runs, d.to(np.array(cat.ed, dtype=np.int64)[b.idx]), d.to(cat.status[b.idx]), rep,
                     fail[1:], text_stride_words=1, read_stride_words=1, stranded=1, **kw)
    torch.cuda.synchronize()
    same_rows(rep[:b.n], d.to(cat.report_rec.astype(np.int32))[b.idx_t], b, what)
    assert bool((rep[b.n:] == REC_CANARY).all()), what + ": a record behind the last pair's was written"
    assert fail.cpu().tolist() == [1000, 1000 + int(cat.report_fail[b.idx].sum()), 1000], what + ": fail count"


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("size", GROUP_SIZES)
def test_report(dev, size, stride):
    b = dev.get_batch(dev.size(dev.group_sizes, size))
    check_report(dev, dev.al, b, stride, "report stride %d, %s (%d pairs)" % (stride, size, b.n))


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["split2", "trips"])
def test_report_per_base_build(dev, aligner_select, size):
    """The test build's one-base-at-a-time form of the same kernel (tests/test_pair_report_gpu.py), where long pairs outnumber the
    wavefronts of a set and on the second and third trip"""
    b = dev.get_batch(dev.size(dev.group_sizes, size))
    check_report(dev, aligner_select, b, 1, "report per base, %s (%d pairs)" % (size, b.n), per_base=True)


# ---------------------------------------------------------------------------------------------------------------
# clipping
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("apply", [False, True])
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("size", GROUP_SIZES)
def test_clip(dev, size, stride, apply):
    import torch
    cat = dev.cat
    b = dev.get_batch(dev.size(dev.group_sizes, size))
    what = "clip stride %d apply %d, %s (%d pairs)" % (stride, apply, size, b.n)
    runs, ro, pairs = b.runs_of(dev, stride)
    pairs, n_runs = pairs.clone(), b.n_runs.clone()                    # apply writes them
    ro = None if ro is None else ro.clone()
    before = pairs.clone()
    rec = torch.full((b.n + 3, 8), REC_CANARY, dtype=torch.int32, device=dev.dev)
    dev.al.clip_device(b.n, runs, ro, stride, n_runs, dev.to(cat.status[b.idx]), rec, apply=apply, pairs=pairs)
    torch.cuda.synchronize()
    want = dev.to(cat.clip_rec.astype(np.int32))[b.idx_t]
    same_rows(rec[:b.n], want, b, what)
    assert bool((rec[b.n:] == REC_CANARY).all()), what + ": a record behind the last pair's was written"
    # what apply rewrites: the count, the first run and (stride 6) the capacity behind it — of the pairs it looked at only
    on = dev.to(cat.clip_touched)[b.idx_t] if apply else torch.zeros(b.n, dtype=torch.bool, device=dev.dev)
    moved = torch.where(on, want[:, 4].to(torch.int64), 0)
    same_rows(n_runs, torch.where(on, want[:, 5], b.n_runs), b, what + ": n_runs")
    if stride == 6:
        after = before.clone()
        after[:, 4] += moved
        after[:, 5] -= moved
        same_rows(pairs, after, b, what + ": descriptors")
    else:
        same_rows(ro, b.dense_first + moved, b, what + ": run offsets")
        assert torch.equal(pairs, before), what


# ---------------------------------------------------------------------------------------------------------------
# the pileup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("size", GROUP_SIZES)
def test_pileup(dev, size, stride):
    """Two adds into one accumulator, then the finish: twice the model's planes and twice its out-of-range count."""
    import torch
    cat = dev.cat
    b = dev.get_batch(dev.size(dev.group_sizes, size))
    what = "pileup stride %d, %s (%d pairs)" % (stride, size, b.n)
    runs, ro, pairs = b.runs_of(dev, stride)
    L = wg.TARGET_LEN
    words = pm.PLANES * (L + 1)
    acc_all = torch.full((words + 2 * GUARD,), REC_CANARY, dtype=torch.int32, device=dev.dev)
    acc = acc_all[GUARD:GUARD + words]
    acc.zero_()
    oor = torch.full((3,), 1000, dtype=torch.int32, device=dev.dev)
    status = dev.to(cat.status_pile[b.idx])
    start = dev.to(cat.start[b.idx] + wg.START_SHIFT * b.shift)
    for _ in range(2):
        dev.al.pileup_add(b.n, dev.seq, pairs, runs, ro, stride, b.n_runs, status, start, L, acc, oor[1:], text_stride_words=1,
                          read_stride_words=1, stranded=1)
    dev.al.pileup_finish(L, acc)
    torch.cuda.synchronize()
    want, outside, counted = cat.pileup_expected(b.idx, b.shift)
    assert counted > 0 and 2 * want.max() < 2 ** 31
    got = acc.cpu().numpy().astype(np.int64).reshape(pm.PLANES, L + 1)
    differ = np.argwhere(got != 2 * want)
    assert len(differ) == 0, "%s: %d words differ, first at plane %d position %d: got %d want %d" % (
        what, len(differ), differ[0][0], differ[0][1], got[tuple(differ[0])], 2 * want[tuple(differ[0])])
    assert bool((acc_all[:GUARD] == REC_CANARY).all()) and bool((acc_all[GUARD + words:] == REC_CANARY).all()), what
    assert oor.cpu().tolist() == [1000, 1000 + 2 * outside, 1000], what + ": out of range"


# ---------------------------------------------------------------------------------------------------------------
# run compaction
# ---------------------------------------------------------------------------------------------------------------
SENTINEL_RUN = 0x7777


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("size", COMPACT_SIZES)
def test_compact_runs(dev, size, lead):
    """Slices -> dense: every run of every pair, at even and odd destinations (lead: where the first pair's runs go), sentinels in
    front of the first and behind the last."""
    import torch
    cat = dev.cat
    b = dev.get_batch(dev.size(dev.compact_sizes, size))
    what = "compact_runs lead %d, %s (%d pairs)" % (lead, size, b.n)
    off = lead + np.cumsum(b.cnt) - b.cnt
    total = lead + int(b.cnt.sum()) + GUARD
    assert ((off[b.cnt > wg.COMPACT_LANE_MAX_RUNS] & 1) == 0).any() and ((off[b.cnt > wg.COMPACT_LANE_MAX_RUNS] & 1) == 1).any()
    dense = torch.full((total,), SENTINEL_RUN, dtype=torch.int16, device=dev.dev)
    dev.al.compact_runs(b.n, b.desc, dev.slice_tab, b.n_runs, dev.to(off.astype(np.int64)), dense)
    torch.cuda.synchronize()
    table = dev.slice_tab.view(torch.int16).reshape(-1)
    src = cat.slice_first[b.idx]
    same_buffer(dense, ragged_expected(dev, total, SENTINEL_RUN, torch.int16, b.cnt, off, src, table), b, b.cnt, off, src, table, what)


@pytest.mark.gpu
def test_compact_runs_packed_and_unpack(dev):
    """One wavefront per pair, three trips of the capped grid and five pairs: a byte per run at every byte alignment, and back."""
    import torch
    cat = dev.cat
    n = wg.packed_size(dev.n_cus)
    b = dev.get_batch(n)
    cnt = np.where(np.array(cat.sort)[b.idx] == "bad_run", 0, b.cnt)     # (a run that is none has no packed form; and pairs without runs)
    off = 3 + np.cumsum(cnt) - cnt
    total = 3 + int(cnt.sum())
    room = (total + GUARD + 7) // 8 * 8
    packed = torch.full((room,), wg.CANARY, dtype=torch.uint8, device=dev.dev)
    dev.al.compact_runs_packed(n, b.desc, dev.slice_tab, dev.to(cnt.astype(np.int32)), dev.to(off.astype(np.int64)), packed)
    torch.cuda.synchronize()
    tab16 = np.concatenate([cat.slice_tab, np.zeros((GUARD, 2), np.uint8)]).view(np.uint16).reshape(-1)
    table = dev.to(wg.run_to_byte(tab16))
    src = cat.slice_first[b.idx]
    exp = ragged_expected(dev, room, wg.CANARY, torch.uint8, cnt, off, src, table)
    same_buffer(packed, exp, b, cnt, off, src, table, "compact_runs_packed (%d pairs)" % n)
    # back: the packed bytes (canaries and all: any byte has a run) -> runs, a sentinel behind them
    runs = torch.full((room + 8,), SENTINEL_RUN, dtype=torch.int16, device=dev.dev)
    dev.al.unpack_runs(room - 3, packed, runs)
    torch.cuda.synchronize()
    want = np.concatenate([wg.byte_to_run(exp.cpu().numpy()[:room - 3]), np.full(11, SENTINEL_RUN, np.uint16)]).view(np.int16)
    assert torch.equal(runs, dev.to(want)), "unpack_runs of %d runs" % (room - 3)
    got16 = runs.cpu().numpy().view(np.uint16)
    p = int(np.flatnonzero(cnt > 40)[0])
    assert np.array_equal(got16[off[p]:off[p] + cnt[p]], tab16[src[p]:src[p] + cnt[p]])      # (a pair's runs are what they were)


@pytest.mark.gpu
def test_unpack_runs_takes_more_than_one_trip(dev):
    """As many runs as the large batch has — more than the capped grid restores in one trip, and 1, 2 or 3 runs behind the last
    four: every byte value, a sentinel behind the last run."""
    import torch
    total = wg.total_runs(wg.batch_index(dev.group_sizes["trips"])[0])
    total += (3 - total) % 4                                          # three runs behind the last quad
    assert total % 4 == 3 and total > 4 * 256 * wg.unpack_runs_grid(total, dev.n_cus) and total <= wg.MAX_RUNS
    rng = np.random.Generator(np.random.PCG64(99))
    packed = dev.to(rng.integers(0, 256, size=total + 1, dtype=np.uint8))
    runs = torch.full((total + 9,), SENTINEL_RUN, dtype=torch.int16, device=dev.dev)
    dev.al.unpack_runs(total, packed, runs)
    torch.cuda.synchronize()
    table = dev.to(wg.byte_to_run(np.arange(256)).view(np.int16))
    assert torch.equal(runs[:total], table[packed[:total].to(torch.int64)]), "unpack_runs of %d runs" % total
    assert bool((runs[total:] == SENTINEL_RUN).all())


# ---------------------------------------------------------------------------------------------------------------
# the host path's own text kernels (text_len_kernel, render_text_kernel), which have no device entry point: mapping calls on a
# resident genome whose planned chunks are of three `split` classes, every output against the models by index
# ---------------------------------------------------------------------------------------------------------------
def same_strings(text, offsets, strings, ids, what):
    """A call's strings (bytes and n + 1 offsets) against the distinct pairs' by index: every offset, every byte"""
    lens_d, bytes_d, src_d = strings
    lens = lens_d[ids]
    off = np.asarray(offsets).astype(np.int64)
    want_off = np.concatenate([[0], np.cumsum(lens)])
    assert len(off) == len(want_off) and off[-1] == len(text), what
    if not np.array_equal(off, want_off):
        p = int(np.flatnonzero(off != want_off)[0]) - 1
        raise AssertionError("%s: pair %d (distinct pair %d) has %d bytes, not %d" % (what, p, ids[p], off[p + 1] - off[p], lens[p]))
    differ = ragged_mismatch(np.frombuffer(text, dtype=np.uint8), off[:-1], bytes_d, src_d[ids], lens)
    assert len(differ) == 0, "%s: %d pairs differ, first pair %d (distinct pair %d): got %r" % (
        what, len(differ), differ[0], ids[differ[0]], text[off[differ[0]]:off[differ[0] + 1]][:80])


@pytest.mark.gpu
@pytest.mark.parametrize("best", [False, True])
@pytest.mark.parametrize("split", wg.HOST_SPLITS + ["windowed"])
def test_host_text_kernels(aligner, oracle, split, best):
    """Best-candidate mode off (caller order: every group mixes short and long pairs) and on (longest first, the losers without
    text); the report, cs and the merged form on.  "windowed": the smallest call once more in the default form."""
    from scrooge_amd import api
    form, split = ("windowed", wg.HOST_SPLITS[0]) if split == "windowed" else ("merged", split)
    hc = wg.host_catalog(oracle)
    n_cus = aligner.query_launch()["n_cus"]
    if "split%d" % split not in wg.group_sizes(n_cus):
        pytest.skip("a device of %d CUs has no launch of class split%d" % (n_cus, split))
    plan = dict(best=best, sort_by_length=int(best))
    n_reads = wg.host_call_reads(hc, n_cus, split, **plan)
    assert split in wg.host_chunk_classes(hc, n_reads, n_cus, **plan)
    reads, cands, ids = hc.call(n_reads)
    what = "host call of %d pairs, chunks of split %d, best %d, %s" % (2 * n_reads, split, best, form)
    aligner.set_genome(hc.genome)
    arr = aligner.align_mapping(None, reads, cands, arrays=True, report=True, diff="cs", cigar_form=form, **plan)
    mode = "best" if best else "all"
    assert np.array_equal(arr["edit_distance"], hc.ed[ids]), what
    assert np.array_equal(arr["status"], np.where(hc.wins[ids] | (not best), api.SCRG_OK, api.SCRG_PAIR_NOT_BEST)), what
    same_strings(arr["cigar_text"], arr["cigar_offset"], hc.strings[mode][form], ids, what + ": CIGAR text")
    same_strings(arr["diff_text"], arr["diff_offset"], hc.strings[mode]["cs"], ids, what + ": cs")
    rep = np.ascontiguousarray(arr["report"]).view(np.uint32).reshape(-1, 8)
    want = hc.report_rec[mode][ids]
    assert rep.shape == want.shape, what
    differ = np.flatnonzero((rep != want).any(axis=1))
    assert len(differ) == 0, "%s: %d records differ, first pair %d (distinct pair %d): got %r want %r" % (
        what, len(differ), differ[0], ids[differ[0]], rep[differ[0]].tolist(), want[differ[0]].tolist())
    has = hc.wins[ids] | (not best)
    assert np.array_equal(np.diff(arr["run_offset"].astype(np.int64)), np.where(has, hc.cnt[ids], 0)), what
