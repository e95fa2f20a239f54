"""The CIGAR text kernels of the host path (text_len_kernel, render_text_kernel) at the thresholds of run_walk.h.

Up to 24 runs a pair is measured and rendered by one lane, from 25 by a whole wavefront in tiles of 512 runs, eight per lane; a
batch of few pairs lets several wavefronts share a group of 64 pairs.  At W = 64, O = 33 a read that equals its text and is
31 k bases long has exactly k runs "31=", so the run counts can be set: 1, 24 | 25, 26 (both sides of the lane limit), 511,
512 | 513 (both sides of a tile) and 1025 (a third tile with one run), with an empty read (no runs, "") among them.  Reads with
substitutions mix one-digit counts ("9=", "1X") with the two-digit ones, and two pairs at W = 256, O = 129 have "127=" runs:
the three-digit branch of run_chars / put_run, by a lane and by a wavefront.  Batches: the 1025-run pair alone (64 wavefronts share
its group), 65 pairs (a second group of one) and 200.  Expected values come from the CPU oracle."""
import os
import re

import numpy as np
import pytest

from scrooge_amd import api, synth

STEP = 31                   # W - O: the bases a window commits
COUNTS = [1, 24, 25, 26, 511, 512, 513, 1025]
THREADS = min(16, os.cpu_count() or 1)
_cache = {}


def _pair(seq, k):
    return seq[:STEP * k + 64], seq[:STEP * k]


def _with_substitutions(read, every, at):
    """base `at` of every `every`-th stretch of 31 bases replaced by another one"""
    q = bytearray(read)
    for s in range(0, len(q) - STEP + 1, STEP * every):
        q[s + at] = ord("ACGT"[("ACGT".index(chr(q[s + at])) + 1) % 4])
    return bytes(q)


def cases(oracle):
    """the distinct pairs (texts, reads) with the oracle's (edit distances, CIGARs), and the same for the W = 256 pairs"""
    if not _cache:
        rng = np.random.Generator(np.random.PCG64(4711))
        seq = synth.BASES[rng.integers(0, 4, STEP * max(COUNTS) + 64)].tobytes()
        pairs = [_pair(seq, k) for k in [0] + COUNTS]
        for k, every, at in ((2, 1, 9), (25, 3, 9), (26, 1, 0), (513, 2, 30)):
            t, q = _pair(seq, k)
            pairs.append((t, _with_substitutions(q, every, at)))
        texts, reads = [t for t, _ in pairs], [q for _, q in pairs]
        eds, cigars, _, _ = oracle.align(texts, reads, threads=THREADS)
        _cache["w64"] = (texts, reads, list(eds), list(cigars))
        wide = [(seq[:127 * k + 256], seq[:127 * k]) for k in (3, 30)]
        texts, reads = [t for t, _ in wide], [q for _, q in wide]
        eds, cigars, _, _ = oracle.align(texts, reads, W=256, O=129, threads=2)
        _cache["w256"] = (texts, reads, list(eds), list(cigars))
    return _cache["w64"], _cache["w256"]


def n_runs(cigar):
    return len(re.findall(r"\d+[=XID]", cigar))


def check(aligner, texts, reads, eds, cigars, what, **kw):
    arr = aligner.align_pairs(texts, reads, arrays=True, **kw)
    n = len(texts)
    to = arr["cigar_offset"].astype(np.int64)
    assert arr["status"].tolist() == [api.SCRG_OK] * n, what
    assert arr["edit_distance"].tolist() == [int(e) for e in eds], what
    for p in range(n):
        assert arr["cigar_text"][to[p]:to[p + 1]] == cigars[p].encode() + b"\0", (what, p, n_runs(cigars[p]))


def test_the_inputs_have_the_run_counts_they_are_built_for(oracle):
    (_, _, eds, cigars), (_, _, _, wide) = cases(oracle)
    assert [n_runs(c) for c in cigars[:1 + len(COUNTS)]] == [0] + COUNTS
    assert cigars[0] == "" and cigars[1] == "31=" and all(e == 0 for e in eds[:1 + len(COUNTS)])
    assert all(e > 0 and "1X" in c for e, c in zip(eds[1 + len(COUNTS):], cigars[1 + len(COUNTS):]))
    assert any(re.search(r"(^|\D)\d=", c) for c in cigars[1 + len(COUNTS):])         # a one-digit '=' run
    assert wide[0] == "127=" * 3 and wide[1] == "127=" * 30


@pytest.mark.gpu
def test_cigar_text_at_the_lane_and_tile_thresholds(aligner, oracle):
    (texts, reads, eds, cigars), wide = cases(oracle)
    m = len(texts)
    counts_200 = {n_runs(cigars[p % m]) for p in range(200)}
    assert counts_200 >= {1, 24, 25, 511, 512, 513, 1025}
    big = 1 + COUNTS.index(1025)
    check(aligner, [texts[big]], [reads[big]], [eds[big]], [cigars[big]], "n=1")
    for n in (65, 200):
        idx = [p % m for p in range(n)]
        check(aligner, [texts[i] for i in idx], [reads[i] for i in idx], [eds[i] for i in idx], [cigars[i] for i in idx], "n=%d" % n)
    check(aligner, *wide, "W=256", W=256, O=129)
