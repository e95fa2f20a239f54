"""The host entry points at the chunk sizes where the per-pair layouts' padding and the partial last group change.

Per chunk of n pairs the host path uploads [read_len 4n | text_len or row 4n | pad to 16 | start 8n | key 4n], keeps
[ed 8n | status 4n | pad to 16 | run_off 8n | text_off 8n | pad to 256 | wire 12n] on the device (distance-only mode:
[ed 8n | status 4n | text_end 4n]) and reads the wire back: odd n moves the padded offsets, n = 63 | 65 the groups of 64, and
2 * 512 + 37 pairs are three chunks, the last with a partial group.  Every output mode of align_pairs and align_mapping runs at every
size; expected values come from the CPU oracle (edit distances, CIGARs; text_end = the text a CIGAR consumes) and from
api.best_per_read (the winners)."""
import numpy as np
import pytest

from scrooge_amd import api, synth
from tests.test_best_candidate import COMP, offsets_of, oracle_mapping
from tests.test_distance_only import text_end_of

OK, NOT_BEST = api.SCRG_OK, api.SCRG_PAIR_NOT_BEST
ALL, TEXT, RUNS, BEST, DIST = api.SCRG_OUT_ALL, api.SCRG_OUT_TEXT, api.SCRG_OUT_RUNS, api.SCRG_OUT_BEST, api.SCRG_OUT_DISTANCE
SIZES = [1, 2, 3, 15, 17, 63, 65, 2 * 512 + 37]
_cache = {}


def batch(oracle, n):
    """n pairs (reads of 20..200 bases, texts 0..15 % longer) and the mapping call made of them: the genome is the concatenated
    texts, read r = the read of pair 2r with two candidates — its text's start and that start + 7, so every read has a loser —
    (n odd: the last read has one); a third of the reads are stored reverse-complemented for the stranded calls."""
    if n in _cache:
        return _cache[n]
    rng = np.random.Generator(np.random.PCG64(9000 + n))
    texts, reads = [], []
    for _ in range(n):
        t, q = synth.make_pair(int(rng.integers(20, 201)), 0.08, (1, 1, 1), rng, slack=float(rng.uniform(0.0, 0.15)))
        texts.append(synth.BASES[t].tobytes())
        reads.append(synth.BASES[q].tobytes())
    b = {"texts": texts, "reads": reads}
    b["eds"], b["cigars"], _, _ = oracle.align(texts, reads, threads=16)
    starts = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    b["genome"] = b"".join(texts)
    b["m_reads"] = [reads[2 * r] for r in range((n + 1) // 2)]
    b["cands"] = [[int(starts[2 * r]), int(starts[2 * r]) + 7][:n - 2 * r] for r in range((n + 1) // 2)]
    assert sum(len(c) for c in b["cands"]) == n
    b["m_eds"], b["m_cigars"] = oracle_mapping(oracle, b["genome"], b["m_reads"], b["cands"])
    b["reverse"] = [[int(rng.random() < 0.4) for _ in c] for c in b["cands"]]
    b["s_reads"] = list(b["m_reads"])
    for r in range(0, len(b["s_reads"]), 3):
        b["s_reads"][r] = b["s_reads"][r].translate(COMP)[::-1]
        b["reverse"][r] = [1 - x for x in b["reverse"][r]]
    b["s_eds"], b["s_cigars"] = oracle_mapping(oracle, b["genome"], b["s_reads"], b["cands"], reverse=b["reverse"])
    _cache[n] = b
    return b


def check(arr, outputs, eds, cigars, cand_offsets=None, what="", ed_only=None):
    """Every array of a result.  outputs: the mode's flags; cand_offsets: the reads' candidates (SCRG_OUT_BEST); ed_only[p]: compare
    the pair's status and edit distance only."""
    n = len(eds)
    eds = np.asarray(eds, dtype=np.int64)
    want_st = np.zeros(n, dtype=np.int64)
    if outputs & BEST:
        best = api.best_per_read(eds, want_st, cand_offsets)["best_pair"]
        want_st[:] = NOT_BEST
        want_st[best[best >= 0]] = OK
        assert (want_st == NOT_BEST).sum() == n // 2, what       # every read with two candidates has a loser
    want = [c if s == OK else "" for c, s in zip(cigars, want_st)]
    distance = bool(outputs & DIST)
    want_runs, want_text = not distance and (outputs & 3) != TEXT, not distance and (outputs & 3) != RUNS
    ed, st, ro, to = arr["edit_distance"], arr["status"], arr["run_offset"].astype(np.int64), arr["cigar_offset"].astype(np.int64)
    runs, text = arr["runs"], arr["cigar_text"]
    assert len(ed) == len(st) == n and len(ro) == len(to) == n + 1, what
    assert ed.tolist() == eds.tolist() and st.tolist() == want_st.tolist(), what
    assert ro[0] == 0 and np.all(np.diff(ro) >= 0) and ro[n] == len(runs) and (want_runs or ro[n] == 0), what
    assert to[0] == 0 and np.all(np.diff(to) >= 0) and to[n] == len(text) and (want_text or to[n] == 0), what
    assert ("text_end" in arr) == distance, what
    if distance:
        want_te = [text_end_of(c) if s == OK else 0 for c, s in zip(cigars, want_st)]
        assert arr["text_end"].tolist() == want_te, what
    for p in range(n):
        if ed_only is not None and ed_only[p]:
            continue
        if want_runs:
            assert "".join("%d%s" % (c, chr(o)) for c, o in runs[ro[p]:ro[p + 1]]) == want[p], (what, p)
        if want_text:
            assert text[to[p]:to[p + 1]] == want[p].encode() + b"\0", (what, p)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_pairs(aligner, oracle, n):
    b = batch(oracle, n)
    for outputs in (ALL, TEXT, RUNS, DIST):
        arr = aligner.align_pairs(b["texts"], b["reads"], arrays=True, outputs=outputs)
        check(arr, outputs, b["eds"], b["cigars"], what="pairs n=%d outputs=%d" % (n, outputs))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_mapping(aligner, oracle, n):
    b = batch(oracle, n)
    co = offsets_of(b["cands"])
    for outputs in (ALL, BEST, BEST | TEXT, BEST | DIST):
        arr = aligner.align_mapping(b["genome"], b["m_reads"], b["cands"], arrays=True, outputs=outputs)
        check(arr, outputs, b["m_eds"], b["m_cigars"], co, what="mapping n=%d outputs=%d" % (n, outputs))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 8])
@pytest.mark.parametrize("n", SIZES)
def test_mapping_reverse(aligner, oracle, n, lanes):
    """cand_reverse: at one pair per lane the strand is bit 31 of the row word; the GenASM-row mappings get rows split by strand, and
    best-candidate mode then uploads the read index as the key of its own."""
    b = batch(oracle, n)
    try:
        arr = aligner.align_mapping_multi([0], b["genome"], b["s_reads"], b["cands"], reverse=b["reverse"], arrays=True, best=True,
                                          lanes_per_pair=lanes)
    finally:
        api.load_library().scrg_multi_release()
    ed_only = [bool(x) for r in b["reverse"] for x in r] if lanes == 8 else None
    check(arr, BEST, b["s_eds"], b["s_cigars"], offsets_of(b["cands"]), what="stranded n=%d lanes=%d" % (n, lanes), ed_only=ed_only)
