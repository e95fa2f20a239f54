"""The default kernel's band round after its votes and its diagonal count were trimmed (genasm_lane_kernel.hip: wave_any and the
values a lane without a pair votes with, add_masked2): none of it may show in a result.

One batch of 256 pairs (four wavefronts) at W = 64 / O = 33, reads of 400 and 437 bases in turn, so that the lanes of a wavefront
retire at different rounds (a launch of 256 pairs refills no lane: tests/test_queue_refill.py).  Of every eight pairs six carry
ONT-profile errors, one is clean but for ONE block — an insertion of 20..22 bases or a deletion of 9..11, in a full window: the
banded distance exceeds the threshold and the wavefront redoes the round on the full table — and one is clean with a text that ends
10..40 bases early: its last rounds are short-text rounds.  What the batch makes the kernel do is replayed on the CPU from the
band's restatement in C and asserted (test_the_oracle_takes_every_pair), with the oracle's verdict on every pair.

Compared with oracle.pyoracle: edit distance, run count and every run (runs), every stream byte and the CIGAR the stream decodes
to (edit streams), edit distance and text end (distance only), in both sequence layouts; the split kernel (64 pairs per launch)
against the plain one; the test build without the band and with the band in every eligible round."""
import functools

import numpy as np
import pytest

from scrooge_amd import api, synth
from tests.test_gpu_band_table import BAND_ALWAYS, NO_BAND, SAFE, W, O, _block, _ont, compare, expected, launch, replay, tally, window_trace

SPLIT, NO_SPLIT = 512, 1024                # scrg_params.reserved[0] of the test build (genasm_kernels.h)
N = 256
LAYOUTS = ["contiguous", "groups"]
MODES = ("runs", "edits", "distance")


def _kind(k):
    """Pair k: 0..5 ONT errors, 6 one block, 7 an early text end; the sorts move through the lanes from group to group, so that
    each comes with both read lengths."""
    return (k + k // 8) % 8


@functools.lru_cache(maxsize=None)
def batch():
    rng = np.random.Generator(np.random.PCG64(2009))
    texts, reads = [], []
    for k in range(N):
        L = 400 if k % 2 == 0 else 437
        kind = _kind(k)
        if kind < 6:
            t, q = _ont(L, rng)
        elif kind == 6:
            first = 3 + (k // 8) % 4            # the block's window: rounds 3..8 of the pair, the first three stay clean
            if (k // 16) % 2 == 0:
                t, q = _block(L, rng, False, (20, 22), (0, 0), first)
            else:
                t, q = _block(L, rng, False, (0, 0), (9, 11), first)
        else:
            q = synth.random_seq(L, rng)
            t = q[:L - int(rng.integers(10, 41))]
        texts.append(t), reads.append(q)
    none = np.zeros(N, dtype=bool)
    return dict(texts=texts, reads=reads, rflag=none, tflag=none)


def part(b, lo, hi):
    return {k: v[lo:hi] for k, v in b.items()}


def want(oracle):
    b = batch()
    return expected(oracle, ("lane_diet2", N, 2009), b["texts"], b["reads"])


def same(x, y, mode, what):
    """Two launches' results, field by field: every pair's distance, status and count, and its output up to that count."""
    for f in ("ed", "status", "count") + (("run_count",) if mode == "edits" else ()):
        assert np.array_equal(x[f], y[f]), (what, f, np.flatnonzero(x[f] != y[f])[:8])
    if mode == "distance":
        return
    unit = 1 if mode == "edits" else 2
    for k in range(len(x["ed"])):
        lo, n = 2 * x["cap"] * k, unit * int(x["count"][k])
        assert np.array_equal(x["buf"][lo:lo + n], y["buf"][lo:lo + n]), (what, "pair", k)


def joined(parts):
    out = dict(cap=parts[0]["cap"])
    for f in parts[0]:
        if f != "cap":
            out[f] = np.concatenate([p[f] for p in parts])
    return out


def test_the_oracle_takes_every_pair(oracle):
    """(CPU.)  The oracle aligns all 256 pairs — none is left out of the GPU tests below — and the batch holds what it says: the
    sorts in their shares, block pairs whose banded distance exceeds the threshold in a full window, texts that end inside a
    window; replayed per wavefront: rounds committed on the band, rounds redone, short-text rounds, lanes retiring out of step."""
    b = batch()
    exp = want(oracle)                      # (Oracle.align raises if the oracle turns a batch down)
    assert len(exp["ed"]) == N == len(exp["cigars"])
    for q, cg in zip(b["reads"], exp["cigars"]):
        assert sum(c for c, op in api._parse_cigar(cg) if op in "=XI") == len(q)          # the whole read, every pair
    kinds = np.array([_kind(k) for k in range(N)])
    lens = np.array([len(q) for q in b["reads"]])
    assert (kinds < 6).sum() == 3 * N // 4 and (kinds == 6).sum() == N // 8 and (kinds == 7).sum() == N // 8
    assert set(lens) == {400, 437} and all(set(lens[kinds == s]) == {400, 437} for s in (0, 6, 7))
    assert (exp["ed"][kinds < 6] > 20).all()                                                   # ~10 % errors
    early = np.array([len(q) - len(t) for t, q in zip(b["texts"], b["reads"])])[kinds == 7]
    assert early.min() >= 10 and early.max() <= 40 and (exp["ed"][kinds == 7] == early).all()
    over = [int((window_trace(b["texts"][k], b["reads"][k]) > SAFE).sum()) for k in np.flatnonzero(kinds == 6)]
    print("block pairs with a full window over the threshold: %d of %d" % (sum(x > 0 for x in over), len(over)))
    assert sum(x > 0 for x in over) >= 3 * len(over) // 4           # (9 deletions alone cost 18: under it)
    for always in (False, True):
        for w, rounds in enumerate(replay(b, always)):
            print("8192" if always else "shipped", "wavefront", w, " ".join("%s%d" % (x[0], n) for x, n in rounds))
            assert tally(rounds, "committed", 64) >= 2 and tally(rounds, "redone", 64) >= 3 and tally(rounds, "short") >= 3
            assert len({n for x, n in rounds}) >= 3               # the wavefront shrinks in steps
    assert any(tally(r, "backed off") for r in replay(b)) or all(tally(r, "redone") <= 6 for r in replay(b))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_runs_streams_and_distances(aligner, oracle, layout):
    """The shipped build, the plain kernel: runs, edit streams (the bytes, and what they decode to) and distance-only."""
    b, exp = batch(), want(oracle)
    for mode in MODES:
        res = launch(aligner, b, layout, mode)
        compare(res, exp, mode, "shipped, %s, %s" % (mode, layout))
        if mode == "edits":
            for k in range(N):
                lo = 2 * res["cap"] * k
                stream = res["buf"][lo:lo + int(res["count"][k])].tobytes()
                assert api.edit_stream_to_cigar(stream, len(b["reads"][k]), W, O) == exp["cigars"][k], ("decoded", layout, k)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_split_and_plain_kernels_agree(aligner, aligner_select, oracle, layout):
    """The split kernel's producer shares the table with the plain kernel: the batch in four launches of 64 pairs through
    genasm_lane_split_kernel (reserved[0] = 512), whole through genasm_lane_kernel (1024, and the shipped build)."""
    b, exp = batch(), want(oracle)
    split = joined([launch(aligner_select, part(b, lo, lo + 64), layout, "runs", SPLIT) for lo in range(0, N, 64)])
    compare(split, exp, "runs", "split, %s" % layout)
    for al, select in ((aligner_select, NO_SPLIT), (aligner, 0)):
        plain = launch(al, b, layout, "runs", select)
        compare(plain, exp, "runs", "plain (reserved[0] = %d), %s" % (select, layout))
        same(split, plain, "runs", "split against plain (reserved[0] = %d), %s" % (select, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_with_and_without_the_band(aligner_select, oracle, layout):
    """The test build with every round on the full table (reserved[0] = 4096) and with the band in every eligible round, no
    back-off (8192): the same results, and the oracle's."""
    b, exp = batch(), want(oracle)
    for mode in MODES:
        full = launch(aligner_select, b, layout, mode, NO_BAND)
        band = launch(aligner_select, b, layout, mode, BAND_ALWAYS)
        compare(full, exp, mode, "reserved[0] = 4096, %s, %s" % (mode, layout))
        compare(band, exp, mode, "reserved[0] = 8192, %s, %s" % (mode, layout))
        same(full, band, mode, "4096 against 8192, %s, %s" % (mode, layout))
