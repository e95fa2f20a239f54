"""The alignment report on the GPU (scrooge_amd/csrc/report_kernels.hip; scrg_report_device, scrg_ctx_set_report /
scrg_ctx_take_report): the device layer on synthetic runs against the host mirror scrg_report_from_runs (which
tests/test_pair_report.py holds to the Python model), then the host calls against the mirror of the runs the same call returned."""
import subprocess

import numpy as np
import pytest

from scrooge_amd import api
from scrooge_amd import io as sio
from tests import diff_model as dm
from tests import report_model as rm
from tests.test_best_candidate import offsets_of

OK, OVER, NOT_BEST = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST
FIELDS = list(rm.FIELDS)
CANARY = 0x5A5A5A5A
SHIFTS = [0, 1, 31, 13, 0, 17, 31, 1, 30, 2]          # text_off % 32 of the contiguous layout's texts


def mirror(text, read, runs, ed):
    return api.report_from_runs(text, read, runs, ed)


def device_report(al, cases, layout, source, read_rev=None, text_rev=None, stranded=1, text_strands=True, status=None, shifts=None,
                  cap=None, n_runs=None, with_fail=True, per_base=False):
    """scrg_report_device on cases = [(text, read, runs, ed)], the sequences AS ALIGNED -> (records: a structured array of len(cases),
    the fail count, the canary rows behind the records).  read_rev / text_rev (per pair): the sequence is stored as its reverse
    complement and its offset flagged; source "slices": the runs lie in slices (stride 6 on the descriptors), "dense": back to back."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    n = len(cases)
    read_rev = np.zeros(n, bool) if read_rev is None else np.asarray(read_rev, bool)
    text_rev = np.zeros(n, bool) if text_rev is None else np.asarray(text_rev, bool)
    texts = [dm.revcomp(c[0]) if tv else c[0] for c, tv in zip(cases, text_rev)]
    reads = [dm.revcomp(c[1]) if rv else c[1] for c, rv in zip(cases, read_rev)]
    if layout == "contiguous":
        sh = shifts if shifts is not None else [SHIFTS[k % len(SHIFTS)] for k in range(n)] + [0] * n
        words, offs = dm.pack_contiguous(texts + reads, sh)
        stride = 1
    else:
        words, offs = dm.pack_groups(texts + reads)
        stride = 64
    t_off = offs[:n] | np.where(text_rev, np.uint64(api.TEXT_REVCOMP), np.uint64(0))
    r_off = offs[n:] | np.where(read_rev, np.uint64(api.READ_REVCOMP), np.uint64(0))
    tl = np.array([len(t) for t in texts], dtype=np.uint64)
    rl = np.array([len(r) for r in reads], dtype=np.uint64)
    cnt = np.array([len(c[2]) for c in cases], dtype=np.int64)
    caps = np.maximum(16, (cnt + 15) // 16 * 16) if cap is None else np.asarray(cap, dtype=np.int64)
    cig_off = np.concatenate([[0], np.cumsum(np.maximum(caps, (cnt + 15) // 16 * 16))])
    if source == "slices":
        runs = np.zeros((int(cig_off[n]), 2), dtype=np.uint8)
        first = cig_off[:n]
    else:
        runs = np.zeros((int(cnt.sum()) + 1, 2), dtype=np.uint8)
        first = np.concatenate([[0], np.cumsum(cnt)])[:n]
    for k, c in enumerate(cases):
        if c[2]:
            runs[first[k]:first[k] + len(c[2])] = [(x, ord(o)) for x, o in c[2]]
    desc = np.stack([t_off, tl, r_off, rl, cig_off[:n].astype(np.uint64), caps.astype(np.uint64)], axis=1)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    seq_t, desc_t, runs_t = to(words.view(np.int64)), to(desc.view(np.int64)), to(runs)
    nruns_t = to((cnt if n_runs is None else np.asarray(n_runs)).astype(np.int32))
    ed_t = to(np.array([c[3] for c in cases], dtype=np.int64))
    st_t = None if status is None else to(np.asarray(status, dtype=np.int32))
    ro_t = None if source == "slices" else to(first.astype(np.int64))
    rep = torch.full((n + 3, 8), CANARY, dtype=torch.int32, device=dev)
    fail = torch.full((1,), 1000, dtype=torch.int32, device=dev) if with_fail else None
    al.set_text_strands(text_strands)
    try:
        al.report_device(n, seq_t, desc_t, runs_t, ro_t, 6 if source == "slices" else 1, nruns_t, ed_t, st_t, rep, fail,
                         text_stride_words=stride, read_stride_words=stride, stranded=stranded, per_base=per_base)
        torch.cuda.synchronize()
    finally:
        al.set_text_strands(False)
    raw = rep.cpu().numpy().view(np.uint32)
    return raw[:n].copy().view(api.report_dtype()).reshape(n), (int(fail.cpu()[0]) - 1000 if with_fail else None), raw[n:]


def check_records(got, want, what):
    for p, w in enumerate(want):
        g = {f: int(got[p][f]) for f in FIELDS}
        assert g == w, "%s: pair %d: got %r want %r" % (what, p, g, w)


_cases = {}


def cases_of(n):
    """n pairs whose run counts walk dm.RUN_COUNTS (n = 200) — alignments, and every corruption of rm.CORRUPTIONS applied to a copy."""
    if n in _cases:
        return _cases[n]
    rng = np.random.Generator(np.random.PCG64(500 + n))
    # (run count, corruption): every count as an alignment, every corruption on both paths and in a second tile, then small ones
    plan = [(1025, None)] if n == 1 else [(c, None) for c in dm.RUN_COUNTS] + [(c, kind) for c in (5, 24, 25, 300, 513) for kind in rm.CORRUPTIONS] + \
        [(int(x), ([None] + rm.CORRUPTIONS)[j % 8]) for j, x in enumerate(rng.integers(0, 40, size=n))]
    out = [(t, r, dm.parse(c) if isinstance(c, str) else c, e) for t, r, c, e, _ in rm.TABLE] if n >= 64 else []
    for c, kind in plan[:n - len(out)]:
        case = rm.valid_case(rng, c, max_count=255 if c <= 26 or c == 255 else 12, slack=0 if kind == "extra_D" else None)   # (no text left: 4, not 6)
        bad = rm.corrupt(kind, *case, rng) if kind else None
        out.append(bad if bad is not None else case)
    _cases[n] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["slices", "dense"])
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_device_layer(aligner, n, layout, source):
    cases = cases_of(n)
    want = [mirror(*c) for c in cases]
    if n == 200:
        assert {len(c[2]) for c in cases} >= {0, 1, 24, 25, 511, 512, 513, 1025}
        assert {w["verdict"] for w in want} == {0, 1, 2, 3, 4, 5, 6}
        long = [w["verdict"] for c, w in zip(cases, want) if len(c[2]) > 24]
        assert set(long) == {0, 1, 2, 3, 4, 5, 6}                                   # the wavefront path meets the failures, too
    if n >= 64:
        assert want[:len(rm.TABLE)] == [row[4] for row in rm.TABLE]
    rev = np.arange(n) % 2 == 1                                       # every second read stored reverse-complemented
    got, fail, behind = device_report(aligner, cases, layout, source, read_rev=rev)
    check_records(got, want, "n=%d %s %s" % (n, layout, source))
    assert fail == sum(w["verdict"] != 0 for w in want)
    assert (behind == CANARY).all()                                  # exactly n records were written
    # without a fail counter
    got2, _, _ = device_report(aligner, cases, layout, source, read_rev=rev, with_fail=False)
    assert got2.tobytes() == got.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
def test_per_base_build_gives_the_same_records(aligner, aligner_select, layout):
    """The test build's one-base-at-a-time form of the kernel (what the word-parallel form is measured against): identical records.
    The shipped library has no such switch."""
    cases = cases_of(200)
    want = [mirror(*c) for c in cases]
    rev = np.arange(200) % 2 == 1
    trev = np.arange(200) % 3 == 1
    got, fail, _ = device_report(aligner_select, cases, layout, "dense", read_rev=rev, text_rev=trev, per_base=True)
    check_records(got, want, "per base " + layout)
    word, fail_w, _ = device_report(aligner_select, cases, layout, "dense", read_rev=rev, text_rev=trev)
    assert word.tobytes() == got.tobytes() and fail == fail_w
    with pytest.raises(api.ScroogeError) as e:
        device_report(aligner, cases[:3], layout, "dense", per_base=True)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG


EDGE_OFFSETS = [(0, 0), (0, 1), (31, 0), (5, 27), (31, 31)]
EDGE_POSITIONS = [None, 0, 1, 30, 31, 32, 33, 63, 64, 254]
FILLER = 40


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["=", "X"])
def test_word_edges(aligner, op):
    """One 255-base run per pair at every word offset of text and read, forward and reversed, one base spoilt at the positions either
    side of the word edges: verdict 5 at that run, 0 without.  On the lane path, and behind 40 filler runs on the wavefront path."""
    rng = np.random.Generator(np.random.PCG64(61 if op == "=" else 62))
    cases, shifts_t, shifts_r, rrev, trev, want_v = [], [], [], [], [], []
    for filler in (0, FILLER):
        for to, qo in EDGE_OFFSETS:
            for mode in range(4):
                for pos in EDGE_POSITIONS:
                    runs = [(1, "=")] * filler + [(255, op)]
                    text, read = rm.sequences_for(runs, rng)
                    text += dm.random_seq(rng, int(rng.integers(0, 3)))
                    if pos is not None:
                        read = list(read)
                        read[filler + pos] = rm.flip(text[filler + pos]) if op == "=" else text[filler + pos]
                        read = "".join(read)
                    cases.append((text, read, runs, 255 if op == "X" else 0))
                    shifts_t.append(to)
                    shifts_r.append(qo)
                    rrev.append(mode & 1)
                    trev.append(mode >> 1)
                    want_v.append((5, filler) if pos is not None else (0, 0))
    want = [mirror(*c) for c in cases]
    assert [(w["verdict"], w["bad_run"]) for w in want] == want_v
    got, fail, behind = device_report(aligner, cases, "contiguous", "dense", read_rev=rrev, text_rev=trev, shifts=shifts_t + shifts_r)
    check_records(got, want, "word edges " + op)
    assert fail == sum(v != 0 for v, _ in want_v) and (behind == CANARY).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
def test_reversed_texts_and_reads(aligner, layout):
    """Random alignments and spoilt ones with every combination of the two strand bits, both layouts, both paths."""
    rng = np.random.Generator(np.random.PCG64(63))
    cases = []
    for k in range(96):
        case = rm.valid_case(rng, [3, 20, 30, 600][k % 4], max_count=[255, 40, 12, 9][k % 4])
        bad = rm.corrupt(["flip_in_eq", "equal_in_X"][k % 2], *case, rng) if k % 3 == 0 else None
        cases.append(bad or case)
    want = [mirror(*c) for c in cases]
    assert {w["verdict"] for w in want} == {0, 5}
    got, fail, _ = device_report(aligner, cases, layout, "slices", read_rev=np.arange(96) // 4 % 2, text_rev=np.arange(96) // 8 % 2)
    check_records(got, want, "strands " + layout)
    assert fail == sum(w["verdict"] != 0 for w in want)


@pytest.mark.gpu
def test_stretches_across_boundaries(aligner):
    """...I|I..., ...I|D... and ...D|=|D... with the | at the boundaries of a lane's eight runs and of a tile's 512."""
    rng = np.random.Generator(np.random.PCG64(64))
    cases, want_counts = [], []
    for b in (8, 16, 504, 512, 1024):
        for pattern, gap_open, indel in (("II", 1, 1), ("ID", 1, 2), ("DI", 1, 2), ("DD", 1, 1), ("D=D", 2, 2), ("I=I", 2, 2), ("I=D", 2, 2)):
            for at in (b - 1, b - len(pattern) + 1):                 # the | before the pattern's last run, and behind its first
                runs = [(2, "=")] * (b + 8)
                runs[at:at + len(pattern)] = [(3, o) for o in pattern]
                text, read = rm.sequences_for(runs, rng)
                cases.append((text, read, runs, rm.edits(runs)))
                want_counts.append((gap_open, indel))
    want = [mirror(*c) for c in cases]
    assert [(w["n_gap_open"], w["n_indel"]) for w in want] == want_counts and all(w["verdict"] == 0 for w in want)
    for source in ("slices", "dense"):
        got, fail, _ = device_report(aligner, cases, "contiguous", source)
        check_records(got, want, "stretches " + source)
        assert fail == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs", [5, 300])
def test_strand_bits_not_honoured(aligner, n_runs):
    """SCRG_READ_REVCOMP without params.stranded, SCRG_TEXT_REVCOMP without text strands on the handle: verdict 1 at run 0, the
    neighbours intact."""
    rng = np.random.Generator(np.random.PCG64(65 + n_runs))
    cases = [rm.valid_case(rng, n_runs, max_count=9) for _ in range(6)]
    want = [mirror(*c) for c in cases]
    flagged = [k in (1, 4) for k in range(6)]
    refused = [rm.record(verdict=1) if f else w for w, f in zip(want, flagged)]
    got, fail, _ = device_report(aligner, cases, "contiguous", "slices", read_rev=flagged, stranded=0)
    check_records(got, refused, "read strand %d" % n_runs)
    assert fail == 2
    got, fail, _ = device_report(aligner, cases, "groups", "dense", text_rev=flagged, text_strands=False)
    check_records(got, refused, "text strand %d" % n_runs)
    assert fail == 2
    got, fail, _ = device_report(aligner, cases, "groups", "dense", text_rev=flagged, read_rev=flagged)       # both honoured
    check_records(got, want, "both honoured %d" % n_runs)
    assert fail == 0


@pytest.mark.gpu
def test_slices_cap_the_run_count(aligner):
    """Stride 6: d_n_runs is capped at cigar_cap — an overflowed pair reports 3 at bad_run = cigar_cap with the counts of its first
    cigar_cap runs."""
    rng = np.random.Generator(np.random.PCG64(66))
    cases = [rm.valid_case(rng, 40, max_count=9), rm.valid_case(rng, 20, max_count=9), rm.valid_case(rng, 100, max_count=9)]
    caps = [16, 32, 32]
    got, fail, _ = device_report(aligner, cases, "contiguous", "slices", cap=caps, n_runs=[40, 20, 100])
    want = [mirror(t, r, runs[:c], ed) for (t, r, runs, ed), c in zip(cases, caps)]
    assert [(w["verdict"], w["bad_run"]) for w in want] == [(3, 16), (0, 0), (3, 32)] and want[0]["n_match"] > 0
    check_records(got, want, "cap")
    assert fail == 2


@pytest.mark.gpu
def test_pair_status(aligner):
    """Status 2 (over the edit limit) and 3 (not best): verdict 7 and zeros, not counted as failures; NULL: all walked."""
    rng = np.random.Generator(np.random.PCG64(67))
    cases = [rm.valid_case(rng, c, max_count=9) for c in (5, 5, 300, 300, 5, 300, 0)]
    status = [0, 2, 3, 0, 3, 1, 2]
    want = [mirror(*c) for c in cases]
    none = rm.record(verdict=7)
    got, fail, _ = device_report(aligner, cases, "contiguous", "dense", status=status)
    check_records(got, [none if s in (2, 3) else w for w, s in zip(want, status)], "status")
    assert fail == 0
    got, fail, _ = device_report(aligner, cases, "contiguous", "dense", status=None)
    check_records(got, want, "no status")


# ---------------------------------------------------------------------------------------------------------------
# the host calls
# ---------------------------------------------------------------------------------------------------------------
def runs_of(arr, p):
    ro = arr["run_offset"]
    return [(int(c), chr(o)) for c, o in arr["runs"][int(ro[p]):int(ro[p + 1])]]


def cigars_of(arr):
    off, text = arr["cigar_offset"].astype(np.int64), arr["cigar_text"]
    return [text[int(off[k]):int(off[k + 1]) - 1].decode() for k in range(len(off) - 1)]


def check_against_runs(arr, texts, reads, what):
    """Every record is the mirror's for the runs the SAME result holds and the as-aligned sequences; every verdict is 0 or 7; the
    score is scrg_affine_score of the returned CIGAR text."""
    rep = arr["report"]
    assert rep.dtype == api.report_dtype() and len(rep) == len(texts), what
    cigars = cigars_of(arr)
    scored = 0
    for p in range(len(texts)):
        got = {f: int(rep[p][f]) for f in FIELDS}
        if arr["status"][p] in (OVER, NOT_BEST):
            assert got == rm.record(verdict=7), (what, p)
            continue
        assert got == mirror(texts[p], reads[p], runs_of(arr, p), int(arr["edit_distance"][p])), (what, p)
        assert got["verdict"] == 0, (what, p)
        assert api.report_score(got) == sio.affine_score(cigars[p]), (what, p)
        scored += 1
    ok = ~np.isin(arr["status"], (OVER, NOT_BEST))
    assert api.report_score(rep[ok]).tolist() == [sio.affine_score(c) for c, k in zip(cigars, ok) if k], what
    return scored


def records(arr):
    return arr["report"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2 * 512 + 37])
def test_host_pairs(aligner, oracle, n):
    """The pairs call under both issue orders (2 * 512 + 37 pairs: three chunks), and the rows call."""
    from tests.test_host_layouts import batch
    b = batch(oracle, n)
    texts, reads = b["texts"], b["reads"]
    a0 = aligner.align_pairs(texts, reads, arrays=True, report=True, sort_by_length=0)
    assert not aligner.report()                                      # the per-call keyword restores the handle's setting
    assert check_against_runs(a0, texts, reads, "pairs n=%d" % n) == n
    assert cigars_of(a0) == b["cigars"]
    a1 = aligner.align_pairs(texts, reads, arrays=True, report=True, sort_by_length=1)
    assert records(a1) == records(a0)
    rows = np.zeros((n, 512), dtype=np.uint8)
    for k, (t, r) in enumerate(zip(texts, reads)):
        rows[k, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        rows[k, 256:256 + len(r)] = np.frombuffer(r, dtype=np.uint8)
    a2 = aligner.align_pairs_rows(rows, 0, [len(t) for t in texts], 256, [len(r) for r in reads], report=True)
    assert records(a2) == records(a0)
    aligner.align_pairs(texts[:20], reads[:20], report=True)         # the list form leaves the records in last_report
    assert aligner.last_report.tobytes() == a0["report"][:20].tobytes() and aligner.last_report_failed == 0


_ont = {}


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (64, 0), (128, 65), (256, 129)])
def test_host_pairs_window_settings(aligner, W, O):
    if not _ont:
        from scrooge_amd import synth
        rng = np.random.Generator(np.random.PCG64(301))
        err, ratio = synth.PROFILES["ont"]
        texts, reads = [], []
        for _ in range(120):
            t, q = synth.make_pair(int(rng.integers(200, 3001)), err, ratio, rng, slack=0.1)
            texts.append(synth.BASES[t].tobytes())
            reads.append(synth.BASES[q].tobytes())
        texts[7], reads[7] = b"ACGTACGT", b""                       # an empty read: no runs, verdict 0
        _ont["texts"], _ont["reads"] = texts, reads
    texts, reads = _ont["texts"], _ont["reads"]
    arr = aligner.align_pairs(texts, reads, arrays=True, report=True, W=W, O=O)
    assert check_against_runs(arr, texts, reads, "W=%d O=%d" % (W, O)) == len(texts)
    assert {f: int(arr["report"][7][f]) for f in FIELDS} == rm.record()
    assert (arr["report"]["n_match"] > 100).sum() > 100


def mapping_texts(b, reads, reverse=None, leftward=None):
    """Per pair of a tests/test_host_layouts.py batch: the text and the read AS ALIGNED — for a leftward candidate the reverse
    complements of the genome before it and of the read as the candidate names it."""
    texts, qs = [], []
    for r, cs in enumerate(b["cands"]):
        for k, c in enumerate(cs):
            q = reads[r]
            if reverse is not None and reverse[r][k]:
                q = q.translate(dm.COMP)[::-1]
            if leftward is not None and leftward[r][k]:
                texts.append(b["genome"][max(0, c - 2 * len(q) - 256):c].translate(dm.COMP)[::-1])
                qs.append(q.translate(dm.COMP)[::-1])
            else:
                texts.append(b["genome"][c:c + 2 * len(q) + 256])
                qs.append(q)
    return texts, qs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2 * 512 + 37])
def test_host_mapping(aligner, oracle, n):
    """The plain, the resident and the stranded call, all three outputs, best-candidate mode (losers 7), an edit limit (over it: 7)
    and directed candidates, leftward ones among them."""
    from tests.test_host_layouts import batch
    b = batch(oracle, n)
    co = offsets_of(b["cands"])
    texts, qs = mapping_texts(b, b["m_reads"])
    what = "mapping n=%d" % n
    plain = aligner.align_mapping(b["genome"], b["m_reads"], b["cands"], arrays=True, report=True)
    assert check_against_runs(plain, texts, qs, what) == n
    for kw in ({"sort_by_length": 0}, {"sort_by_length": 1}, {"outputs": api.SCRG_OUT_TEXT}, {"outputs": api.SCRG_OUT_RUNS}):
        arr = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, report=True, **kw)
        assert records(arr) == records(plain), (what, kw)
        for k in ("edit_distance", "status"):
            assert np.array_equal(arr[k], plain[k])
    arr = aligner.align_mapping_rows(None, np.array([np.frombuffer(r.ljust(256, b"A"), dtype=np.uint8) for r in b["m_reads"]]),
                                     [len(r) for r in b["m_reads"]], co, [c for cs in b["cands"] for c in cs], report=True)
    assert records(arr) == records(plain), what
    # best-candidate mode: the losers have no alignment; with text only, the same records
    best = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, report=True, best=True)
    assert check_against_runs(best, texts, qs, what + " best") == n - n // 2
    lost = best["status"] == NOT_BEST
    assert lost.sum() == n // 2 and (best["report"]["verdict"][lost] == 7).all()
    assert best["report"][~lost].tobytes() == plain["report"][~lost].tobytes()
    best_text = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, report=True, outputs=api.SCRG_OUT_TEXT | api.SCRG_OUT_BEST)
    assert records(best_text) == records(best)
    # an edit limit: pairs over it have no alignment
    lim = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, report=True, max_edits=12)
    over = lim["status"] == OVER
    assert 0 < over.sum() < n and check_against_runs(lim, texts, qs, what + " limit") == n - over.sum()
    assert lim["report"][~over].tobytes() == plain["report"][~over].tobytes()
    # both strands; then every second candidate leftward
    s_texts, s_qs = mapping_texts(b, b["s_reads"], b["reverse"])
    arr = aligner.align_mapping_directed(b["s_reads"], b["cands"], reverse=b["reverse"], arrays=True, report=True)
    assert check_against_runs(arr, s_texts, s_qs, what + " stranded") == n and any(x for r in b["reverse"] for x in r)
    left = [[(r + k) % 2 for k in range(len(c))] for r, c in enumerate(b["cands"])]
    l_texts, l_qs = mapping_texts(b, b["s_reads"], b["reverse"], left)
    for kw in ({}, {"sort_by_length": 0}):
        arr = aligner.align_mapping_directed(b["s_reads"], b["cands"], reverse=b["reverse"], leftward=left, arrays=True, report=True, **kw)
        assert check_against_runs(arr, l_texts, l_qs, what + " leftward") == n
    assert sum(x for r in left for x in r) > n // 3


@pytest.mark.gpu
def test_with_a_diff_kind(aligner, oracle):
    """Set together with a difference-string kind: both arrive; diff's refusal of leftward candidates still holds."""
    from tests.test_host_layouts import batch
    b = batch(oracle, 65)
    arr = aligner.align_pairs(b["texts"], b["reads"], arrays=True, report=True, diff="cs")
    assert check_against_runs(arr, b["texts"], b["reads"], "with cs") == 65
    off = arr["diff_offset"].astype(np.int64)
    for p in range(65):
        assert arr["diff_text"][off[p]:off[p + 1] - 1].decode() == dm.model("cs", b["texts"][p], b["reads"][p], runs_of(arr, p))
    aligner.set_genome(b["genome"])
    aligner.set_diff("md")
    try:
        with pytest.raises(api.ScroogeError) as e:
            aligner.align_mapping_directed(b["m_reads"], b["cands"], leftward=[[1] * len(c) for c in b["cands"]], report=True)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    finally:
        aligner.set_diff(None)


@pytest.mark.gpu
def test_refusals_and_take_once(aligner, oracle):
    from tests.test_host_layouts import batch
    b = batch(oracle, 65)
    aligner.set_genome(b["genome"])
    assert not aligner.report()
    aligner.set_report(True)
    try:
        assert aligner.report()
        for call in (lambda: aligner.align_pairs(b["texts"], b["reads"], lanes_per_pair=8),
                     lambda: aligner.align_mapping(None, b["m_reads"], b["cands"], lanes_per_pair=64),
                     lambda: aligner.align_pairs(b["texts"], b["reads"], distance_only=True),
                     lambda: aligner.align_mapping(None, b["m_reads"], b["cands"], distance_only=True),
                     lambda: aligner.align_anchored(b["m_reads"], [[(c, 0) for c in cs] for cs in b["cands"]])):
            with pytest.raises(api.ScroogeError) as e:
                call()
            assert e.value.status == api.SCRG_ERR_INVALID_ARG
            with pytest.raises(api.ScroogeError):                     # a failed call leaves nothing to take
                aligner.take_report()
        aligner.align_mapping(None, b["m_reads"], b["cands"])
        first = aligner.take_report()
        assert len(first) == 65 and (first["verdict"] == 0).all() and aligner.last_report_failed == 0
        with pytest.raises(api.ScroogeError) as e:                    # handed over once
            aligner.take_report()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
        aligner.align_pairs(b["texts"][:3], b["reads"][:3])          # a report nobody took is discarded by the next call
        aligner.align_pairs(b["texts"][:2], b["reads"][:2])
        assert len(aligner.take_report()) == 2
        aligner.align_pairs([], [])
        assert len(aligner.take_report()) == 0
    finally:
        aligner.set_report(False)
    aligner.align_pairs(b["texts"][:2], b["reads"][:2])
    with pytest.raises(api.ScroogeError):                             # off: a call makes none
        aligner.take_report()


@pytest.mark.gpu
def test_off_path_is_what_it_was(aligner, oracle):
    from tests.test_host_layouts import batch
    b = batch(oracle, 65)
    before = aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    with_report = aligner.align_pairs(b["texts"], b["reads"], arrays=True, report=True)
    after = aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    assert sorted(before) == sorted(after) and "report" not in after and sorted(with_report) == sorted(list(before) + ["report"])
    for k in before:
        for other in (after, with_report):                           # what `outputs` returns is unchanged with the setting on, too
            assert np.array_equal(np.asarray(before[k]), np.asarray(other[k])) if not isinstance(before[k], bytes) else before[k] == other[k], k
    assert cigars_of(before) == b["cigars"]


@pytest.mark.gpu
def test_shim_runs(tmp_path):
    from tests.test_pair_report import build_shim
    p = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines == ["verdict 0 matches 6 score 8", "pair: verdict 0 matches 15", "pair: verdict 0 matches 7", "failed 0", "nothing to take"]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["paf", "sam"])
def test_cli_end_to_end(tmp_path, capsys, fmt):
    """--report --verify on the small job tests/test_io.py uses: every record's tags are the model's for the record's own CIGAR."""
    from scrooge_amd import cli
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=120, seed=33)
    out = str(tmp_path / ("o." + fmt))
    costs = (1, 3, 5, 1) if fmt == "sam" else rm.COSTS
    args = ["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--out=" + out, "--report", "--verify", "--format=" + fmt, "--reverse_strand",
            "--dataset_inflation=2"]
    assert cli.main(args + (["--score=%d,%d,%d,%d" % costs] if fmt == "sam" else [])) == 0
    printed = capsys.readouterr().out
    assert "verified 240 alignments, 0 failed" in printed.splitlines()
    job = sio.Job(fa, fq, seeds, reverse_strand=1, inflation=2)
    genome, reads, cands, names = job.views()
    pairs = [(genome[start:start + 2 * len(r) + 256], r.translate(dm.COMP)[::-1] if rv else r) for r, cs in zip(reads, cands) for start, rv in cs]
    lines = [x.split("\t") for x in open(out).read().splitlines() if not x.startswith("@")]
    assert len(lines) == job.n_pairs == len(pairs) == 240
    edits = 0
    for (text, q), f in zip(pairs, lines):
        cigar = f[5] if fmt == "sam" else [x for x in f if x.startswith("cg:Z:")][0][5:]
        nm = int([x for x in f if x.startswith("NM:i:")][0][5:])
        rec = rm.model(text, q, dm.parse(cigar), nm)
        assert rec["verdict"] == 0 and f[-2:] == ["AS:i:%d" % rm.score(rec, costs), "de:f:%.4f" % rm.divergence(rec)], f[0]
        if fmt == "paf":
            assert int(f[9]) == rec["n_match"] and int(f[10]) == sum(rec[k] for k in FIELDS[:4])
        edits += nm
    assert edits > 0
    # --verify alone adds no tags
    out2 = str(tmp_path / ("plain." + fmt))
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--out=" + out2, "--verify", "--format=" + fmt, "--reverse_strand",
                     "--dataset_inflation=2"]) == 0
    capsys.readouterr()
    assert [x.split("\t")[:-2] for x in open(out).read().splitlines() if not x.startswith("@")] == \
        [x.split("\t") for x in open(out2).read().splitlines() if not x.startswith("@")]
