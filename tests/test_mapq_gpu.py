"""The read summary and MAPQ on the GPU: scrg_read_summary against the host twin on synthetic distances (both forms of the kernel,
every batch edge, before and after the selection), the host path's records across many chunks against the plain Python model, the
pileup filter against the model's KEPT winners, and the refusals."""
import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from tests import mapq_model as mq

LANE_OVER, LANE_NOT_BEST = 2, 3
PUBLIC = np.array([api.SCRG_OK, api.SCRG_ERR_CIGAR_OVERFLOW, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST], dtype=np.uint32)    # lane status -> a result's
COUNTS = [0, 1, 2, 16, 17, 63, 64, 65, 128, 129, 5000]


def synthetic_batch(seed):
    """Reads with every candidate count of COUNTS in shuffled order among many short ones (several wavefronts and blocks), a read
    of each form whose candidates are all over the limit, and ties at the first and at the last candidate of wavefront-form reads."""
    rng = np.random.Generator(np.random.PCG64(seed))
    counts = COUNTS + [17, 65, 129, 40, 16, 3] + [int(x) for x in rng.integers(0, 9, 600)]
    counts = [counts[i] for i in rng.permutation(len(counts))]
    if seed % 2:                       # the first and the last read of the batch: once a wavefront-form read, once a lane-form one
        counts = [5000] + [c for c in counts if c != 5000] + [129]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(first[-1])
    ed = rng.integers(0, 30, n).astype(np.int64)
    status = rng.choice(np.array([0, 0, 0, 0, 1, LANE_OVER], dtype=np.int32), n)
    read_len = np.zeros(n, dtype=np.int32)
    special = {"all_over": 0, "tie_first": 0, "tie_last": 0, "tie_ends": 0}
    n_wave = seed
    for r, c in enumerate(counts):
        a = int(first[r])
        read_len[a:a + c] = int(rng.choice([0, 36, 150, 1000])) if c < 100 else 150
        if c in (3, 40) and not special["all_over"] & (1 if c == 3 else 2):
            status[a:a + c] = LANE_OVER
            special["all_over"] |= 1 if c == 3 else 2
        elif c > 16 and c != 5000:
            kind = ("tie_first", "tie_last", "tie_ends", None)[n_wave % 4]
            n_wave += 1
            if kind:
                ed[a:a + c] = rng.integers(5, 30, c)
                status[a:a + c] = 0
                where = {"tie_first": (0, 1), "tie_last": (c - 2, c - 1), "tie_ends": (0, c - 1)}[kind]
                ed[a + where[0]] = ed[a + where[1]] = 2
                special[kind] += 1
    assert special["all_over"] == 3 and min(special["tie_first"], special["tie_last"], special["tie_ends"]) >= 1, special
    # a distance near 2^32 - 2 is counted in 32 bits
    ed[int(first[counts.index(5000)]) + 7] = 2 ** 32 - 2
    return counts, first, read_len, ed, status


def device_summary(aligner, first, read_len, ed, status, rule, keep):
    import torch
    dev = torch.device("cuda", aligner.device)
    nr, n = len(first) - 1, len(ed)
    pad = lambda a, dtype: torch.from_numpy(np.concatenate([np.asarray(a, dtype=dtype), np.zeros(1, dtype=dtype)])).to(dev)
    t_first, t_len, t_ed, t_status = torch.from_numpy(np.asarray(first, dtype=np.int64)).to(dev), pad(read_len, np.int32), pad(ed, np.int64), pad(status, np.int32)
    out = torch.full((32 * (nr + 1),), 0xEE, dtype=torch.uint8, device=dev)
    t_keep = torch.full((n + 1,), 77, dtype=torch.int32, device=dev) if keep else None
    aligner.read_summary(nr, n, t_first, t_len, t_ed, t_status, out, t_keep, rule=None if rule is None else api.MapqRule(*rule))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert set(got[32 * nr:].tolist()) == {0xEE}                                  # nothing past the end is written
    assert t_status.cpu().numpy()[:n].tolist() == list(status) and t_ed.cpu().numpy()[:n].tolist() == list(ed)      # the inputs are only read
    k = None
    if keep:
        k = t_keep.cpu().numpy()
        assert int(k[n]) == 77
        k = k[:n]
    return got[:32 * nr].view(api.read_summary_dtype()), k


def check_against_twin(got, keep, first, read_len, ed, status, rule, what):
    want, want_keep = api.read_summary_from_distances(None if rule is None else api.MapqRule(*rule), first, read_len, ed, PUBLIC[status], keep=True)
    bad = [r for r in range(len(want)) if got[r].tobytes() != want[r].tobytes()]
    assert not bad, "%s: %d records differ, first read %d (%d candidates): %r != %r" % (what, len(bad), bad[0], first[bad[0] + 1] - first[bad[0]], got[bad[0]], want[bad[0]])
    if keep is not None:
        assert np.array_equal(PUBLIC[keep], want_keep), what
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("seed,rule", [(0, None), (1, (10, 60, 250, 21)), (2, (3, 254, 1000, 1))])
def test_device_entry_against_the_host_twin(aligner, seed, rule):
    import torch
    counts, first, read_len, ed, status = synthetic_batch(seed)
    assert set(COUNTS) <= set(counts)
    # the twin itself is the model's (tests/test_mapq_rule.py holds it to the model on drawn inputs; here on this batch)
    k = mq.DEFAULT_RULE if rule is None else rule
    model = mq.summarise_all(k, first.tolist(), read_len.tolist(), [int(x) for x in ed], [s != LANE_OVER for s in status])
    for with_keep in (False, True):
        got, keep = device_summary(aligner, first, read_len, ed, status, rule, with_keep)
        want = check_against_twin(got, keep, first, read_len, ed, status, rule, "before the selection, keep %r" % with_keep)
        assert [mq.as_tuple(w) for w in want] == [mq.as_tuple(m) for m in model]
        if with_keep:
            assert keep.tolist() == mq.keep_status(model, first.tolist(), status.tolist(), 0, LANE_NOT_BEST)
    before = got
    # both forms served reads, and they agree with the twin on ties at a wavefront-form read's first and last candidate
    wave = np.array(counts) > 16
    assert (before["flags"][wave] & mq.TIED).any() and (before["flags"][~wave] & mq.TIED).any() and (before["n_eligible"][np.array(counts) == 5000] > 3000).all()
    # after scrg_select_best the records are the same (a loser's status 3 is as eligible as the 0 it was), and the copy follows the new statuses
    dev = torch.device("cuda", aligner.device)
    n = len(ed)
    key = torch.from_numpy(np.repeat(np.arange(len(counts), dtype=np.int32), counts)).to(dev)
    t_ed, t_status = torch.from_numpy(ed).to(dev), torch.from_numpy(status.astype(np.int32)).to(dev)
    t_runs = torch.ones(n, dtype=torch.int32, device=dev)
    aligner.select_best(n, key, t_ed, t_status, t_runs)
    torch.cuda.synchronize()
    selected = t_status.cpu().numpy()
    assert (selected == LANE_NOT_BEST).any() and np.array_equal(selected == LANE_OVER, status == LANE_OVER)
    got, keep = device_summary(aligner, first, read_len, ed, selected, rule, True)
    assert got.tobytes() == before.tobytes()
    check_against_twin(got, keep, first, read_len, ed, selected, rule, "after the selection")
    winners = {int(w) for w in got["winner"] if int(w) != mq.NONE}
    assert {int(p) for p in np.nonzero((selected == 0) | (selected == 1))[0]} == winners      # the summary's winners are the selection's


@pytest.mark.gpu
def test_device_entry_edges(aligner):
    import torch
    dev = torch.device("cuda", aligner.device)
    # no reads: SCRG_OK, nothing launched, nothing looked at
    aligner.read_summary(0, 0, None, None, None, None, None)
    # one read without candidates; offsets that run backwards or past n_pairs name no candidates
    first = torch.tensor([0, 0, 3, 2, 9], dtype=torch.int64, device=dev)
    ed, st, ln = torch.tensor([5, 4, 6, 0], dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev), torch.full((4,), 100, dtype=torch.int32, device=dev)
    out = torch.zeros(32 * 4, dtype=torch.uint8, device=dev)
    aligner.read_summary(4, 3, first, ln, ed, st, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(api.read_summary_dtype())
    assert [mq.as_tuple(g) for g in got] == [(mq.NONE, mq.NO_ED, mq.NO_ED, 0, 0, 0, 0, 0), (1, 4, 5, 1, 3, 3, 10, mq.HAS_WINNER | mq.HAS_SECOND | mq.KEPT),
                                             (mq.NONE, mq.NO_ED, mq.NO_ED, 0, 0, 0, 0, 0), (mq.NONE, mq.NO_ED, mq.NO_ED, 0, 0, 0, 0, 0)]
    for bad in ((256, 60, 250, 0), (10, 255, 250, 0), (10, 60, 0, 0), (10, 60, 1001, 0), (10, 60, 250, 255), (10, 60, 250, 0, 1)):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            aligner.read_summary(4, 3, first, ln, ed, st, out, rule=bad)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG and "mapq rule" in aligner.lib.scrg_last_error(aligner.h).decode()
    for args in ((None, ln, ed, st, out), (first, None, ed, st, out), (first, ln, None, st, out), (first, ln, ed, None, out), (first, ln, ed, st, None)):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            aligner.read_summary(4, 3, *args)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(scrooge_amd.ScroogeError):                                  # the copy cannot be the statuses themselves
        aligner.read_summary(4, 3, first, ln, ed, st, out, st)


# ---------------------------------------------------------------------------------------------------------------
# the host path
# ---------------------------------------------------------------------------------------------------------------
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def mutate(rng, seq, n):
    s = bytearray(seq)
    for p in rng.choice(len(s), n, replace=False):
        s[p] = b"ACGT"[(b"ACGT".index(bytes([s[p]])) + int(rng.integers(1, 4))) % 4]
    return bytes(s)


@pytest.fixture(scope="module")
def chunked_batch():
    """24 reads of 50 bp with up to 3000 candidates each — the true place first, last or in the middle, for every fourth read twice
    (a tie) — and, in between, a few reads with 0 to 3 candidates; a third of the candidates on the reverse strand."""
    from scrooge_amd import synth
    rng = np.random.Generator(np.random.PCG64(19))
    G, K = 30000, 3000
    genome = synth.random_seq(G + 1024, rng)
    reads, cands, rev = [], [], []
    for m in range(24):
        s = int(rng.integers(0, G - 600))
        k = K - int(rng.integers(0, 40)) if m % 5 else K
        read = mutate(rng, genome[s:s + 50], m % 3)
        on_reverse = m % 3 == 1
        reads.append(read.translate(COMP)[::-1] if on_reverse else read)
        cs = [int(x) for x in rng.integers(0, G, k)]
        rv = [int(x) for x in rng.integers(0, 3, k) == 0]
        at = (0, k - 1, int(rng.integers(1, k - 1)))[m % 3]
        cs[at], rv[at] = s, int(on_reverse)
        if m % 4 == 0:
            other = (at + 1711) % k
            cs[other], rv[other] = s, int(on_reverse)
        cands.append(cs), rev.append(rv)
        if m % 4 == 1:
            n_small = (m // 4) % 4
            t = int(rng.integers(0, G - 600))
            reads.append(mutate(rng, genome[t:t + 50], 3))
            cands.append([t, int(rng.integers(0, G)), t + 1][:n_small]), rev.append([0, 1, 0][:n_small])
    co = np.concatenate([[0], np.cumsum([len(c) for c in cands])])
    return {"genome": genome, "reads": reads, "cands": cands, "rev": rev, "co": co}


def model_of_plain(b, plain, rule):
    over = plain["status"] == api.SCRG_PAIR_OVER_EDIT_LIMIT
    read_len = np.repeat([len(r) for r in b["reads"]], np.diff(b["co"]))
    return mq.summarise_all(rule, b["co"].tolist(), read_len.tolist(), [int(x) & 0xffffffff for x in plain["edit_distance"]], (~over).tolist())


def same_result(a, b):
    keys = [k for k in ("edit_distance", "status", "run_offset", "cigar_offset", "runs", "text_end") if k in a or k in b]
    return all(np.array_equal(a[k], b[k]) for k in keys) and a.get("cigar_text") == b.get("cigar_text")


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"distance_only": True}, {"max_edits": 21}, {"sort_by_length": 0, "outputs": api.SCRG_OUT_RUNS}],
                         ids=["runs_text", "distance", "edit_limit", "unsorted_runs"])
def test_host_path_across_chunks(aligner, chunked_batch, kw):
    b = chunked_batch
    order, first = api.host_plan_mapping([len(r) for r in b["reads"]], b["co"], best=True)
    assert len(first) - 1 > 3, "the batch should be cut into more than three chunks"
    aligner.set_genome(b["genome"])
    call = lambda **more: aligner.align_mapping_directed(b["reads"], b["cands"], reverse=b["rev"], arrays=True, **kw, **more)
    plain = call()
    off = call(best=True)
    assert "read_summary" not in off
    rule = (10, 60, 250, 0)
    on = call(best=True, mapq=True)
    assert same_result(on, off) and not aligner.mapq()[0]                      # byte-identical with the setting off; the keyword is this call's
    got = on["read_summary"]
    want = model_of_plain(b, plain, rule)
    assert len(got) == len(b["reads"]) and [mq.as_tuple(g) for g in got] == [mq.as_tuple(w) for w in want]
    assert not got["reserved"].any()
    flags = got["flags"]
    assert (flags & mq.TIED).sum() >= 6 and (got["n_candidates"] == 0).any() and (got["n_candidates"] == 3000).any() and len(set(got["mapq"].tolist())) >= 2
    # the winners are the result's: caller pair indices
    winners = {int(w) for w in got["winner"] if int(w) != mq.NONE}
    assert winners == {int(p) for p in np.nonzero((on["status"] != api.SCRG_PAIR_NOT_BEST) & (on["status"] != api.SCRG_PAIR_OVER_EDIT_LIMIT))[0]}
    if "max_edits" in kw:
        assert (got["n_eligible"] < got["n_candidates"]).any()
    # another rule, set on the handle: the records follow it, the result does not change
    other = (1, 30, 100, 0)
    aligner.set_mapq(api.MapqRule(*other))
    try:
        assert aligner.mapq() == (True, api.MapqRule(*other))
        again = call(best=True)
        rec = aligner.take_read_summary()
        assert same_result(again, off) and [mq.as_tuple(g) for g in rec] == [mq.as_tuple(w) for w in model_of_plain(b, plain, other)]
        with pytest.raises(scrooge_amd.ScroogeError):                          # handed over once
            aligner.take_read_summary()
    finally:
        aligner.set_mapq(None, False)


@pytest.mark.gpu
def test_setting_off(aligner, chunked_batch):
    b = chunked_batch
    aligner.set_genome(b["genome"])
    reads, cands = b["reads"][:3], [c[:50] for c in b["cands"][:3]]
    assert aligner.mapq() == (False, api.MapqRule())
    one = aligner.align_mapping(None, reads, cands, arrays=True, best=True)
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        aligner.take_read_summary()
    assert e.value.status == api.SCRG_ERR_INVALID_ARG and "no read summary" in aligner.lib.scrg_last_error(aligner.h).decode()
    two = aligner.align_mapping(None, reads, cands, arrays=True, best=True, mapq=False)
    assert same_result(one, two) and "read_summary" not in two
    three = aligner.align_mapping(None, reads, cands, arrays=True, best=True, mapq=True)
    assert same_result(one, three) and len(three["read_summary"]) == 3
    # reads without candidates at all: records, no chunk
    four = aligner.align_mapping(None, [b"ACGT", b""], [[], []], arrays=True, best=True, mapq=True)
    assert [mq.as_tuple(g) for g in four["read_summary"]] == [(mq.NONE, mq.NO_ED, mq.NO_ED, 0, 0, 0, 0, 0)] * 2


# ---------------------------------------------------------------------------------------------------------------
# the pileup filter
# ---------------------------------------------------------------------------------------------------------------
def repeat_batch():
    """A genome with one 600-base stretch present twice, exactly.  Reads from inside the stretch carry both placements and tie; reads
    that leave the stretch by a few bases carry both and separate by the edits of those bases; the others are placed uniquely."""
    from scrooge_amd import synth
    rng = np.random.Generator(np.random.PCG64(23))
    G, A, B, S, L = 20000, 2000, 9000, 600, 100
    g = bytearray(synth.random_seq(G + 1024, rng))
    g[B:B + S] = g[A:A + S]
    for d in range(1, 4):                                   # the bases behind the two copies differ, so that leaving a copy costs edits
        g[B + S - 1 + d] = b"ACGT"[(b"ACGT".index(bytes([g[A + S - 1 + d]])) + 1) % 4]
    genome = bytes(g)
    reads, cands, kinds = [], [], []
    for k in range(90):
        kind = ("inside", "edge", "unique")[k % 3]
        if kind == "inside":
            o = int(rng.integers(0, S - L - 40))
            s, c = A + o, [A + o, B + o]
        elif kind == "edge":
            past = 1 + (k // 3) % 3                         # 1, 2 or 3 bases behind the stretch
            s, c = A + S - L + past, [A + S - L + past, B + S - L + past]
        else:
            s = int(rng.integers(10000, G - 300)) if k % 2 else int(rng.integers(3000, 8000))
            c = [s]
        # (an edge read's mutations stay in front of the bases that tell the placements apart)
        reads.append(mutate(rng, genome[s:s + 80], int(rng.integers(0, 3))) + genome[s + 80:s + L])
        cands.append(c if k % 2 else c[::-1])
        kinds.append(kind)
    return {"genome": genome, "reads": reads, "cands": cands, "kinds": kinds, "co": np.concatenate([[0], np.cumsum([len(c) for c in cands])])}


@pytest.mark.gpu
def test_only_confidently_placed_reads_pile_up(aligner):
    b = repeat_batch()
    L = len(b["genome"])
    aligner.set_genome(b["genome"])
    plain = aligner.align_mapping(None, b["reads"], b["cands"], arrays=True)
    best = aligner.align_mapping(None, b["reads"], b["cands"], arrays=True, best=True)
    assert (plain["status"] == api.SCRG_OK).all()
    pair_read = np.repeat(np.arange(len(b["reads"])), np.diff(b["co"]))
    taken = {}
    aligner.set_pileup()
    try:
        for q in (0, 1, 21):
            rule = (10, 60, 250, q)
            got = aligner.align_mapping(None, b["reads"], b["cands"], arrays=True, best=True, mapq=api.MapqRule(*rule))
            assert same_result(got, best)                                      # everything but the pileup goes on seeing every winner
            want = model_of_plain(b, plain, rule)
            assert [mq.as_tuple(g) for g in got["read_summary"]] == [mq.as_tuple(w) for w in want]
            kept = [w["winner"] for w in want if w["flags"] & mq.KEPT]
            counts = np.zeros((api.SCRG_PILE_PLANES, L + 1), dtype=np.uint32)
            for p in kept:
                runs = [(int(c), chr(o)) for c, o in plain["runs"][int(plain["run_offset"][p]):int(plain["run_offset"][p + 1])]]
                _, outside = api.pileup_from_runs(runs, b["reads"][pair_read[p]], int(np.concatenate(b["cands"])[p]), L, counts)
                assert not outside
            pile = aligner.take_pileup()
            assert pile["n_alignments"] == len(kept) and pile["n_out_of_range"] == 0
            assert np.array_equal(pile["counts"], counts), q
            taken[q] = (len(kept), pile["counts"])
            mapqs = {kind: {int(g["mapq"]) for g, k in zip(got["read_summary"], b["kinds"]) if k == kind} for kind in ("inside", "edge", "unique")}
            assert mapqs["inside"] == {0} and mapqs["edge"] <= set(range(1, 31)) and min(mapqs["unique"]) > 30
    finally:
        aligner.set_pileup(False)
    # the filter acts: ties leave at 1, reads with a placement in the repeat one or two edits behind leave at 21, the unique ones stay
    assert taken[0][0] == 90 and taken[1][0] == 60 and 30 <= taken[21][0] < 60
    assert not np.array_equal(taken[0][1], taken[1][1]) and not np.array_equal(taken[1][1], taken[21][1])


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(aligner):
    aligner.set_genome(b"ACGTTGCA" * 100)
    reads, cands = [b"ACGTTGCAAC", b"TTGCAACGTT"], [[0, 8], [3]]
    refused = [
        (lambda: aligner.align_mapping(None, reads, cands, mapq=True), ("SCRG_OUT_BEST",)),
        (lambda: aligner.align_mapping(None, reads, cands, distance_only=True, mapq=True), ("SCRG_OUT_BEST",)),
        (lambda: (aligner.set_mapq(), aligner.align_pairs([b"ACGTACGT"], [b"ACGTACGT"])), ("mapping call",)),
        (lambda: (aligner.set_mapq(), aligner.align_mapping_paired(reads, cands)), ("paired", "mate")),
        (lambda: (aligner.set_mapq(), aligner.align_anchored(reads, [[(0, 0), (8, 0)], [(3, 0)]])), ("anchored",)),
        (lambda: aligner.align_mapping(None, reads, cands, best=True, mapq=api.MapqRule(min_keep_q=5)), ("min_keep_q", "pileup")),
    ]
    try:
        for k, (call, words) in enumerate(refused):
            ok = aligner.align_mapping(None, reads, cands, arrays=True, best=True, mapq=True)      # a call that leaves something ...
            assert len(ok["read_summary"]) == 2
            aligner.set_mapq()
            aligner.align_mapping(None, reads, cands, best=True)                                    # ... on the handle
            aligner.set_mapq(None, False)
            with pytest.raises(scrooge_amd.ScroogeError) as e:
                call()
            aligner.set_mapq(None, False)
            assert e.value.status == api.SCRG_ERR_INVALID_ARG, k
            msg = aligner.lib.scrg_last_error(aligner.h).decode()
            assert "scrg_ctx_set_read_summary" in msg and all(w in msg for w in words), (k, msg)
            with pytest.raises(scrooge_amd.ScroogeError):                                           # ... and a refused call leaves nothing to take
                aligner.take_read_summary()
        # an invalid rule never reaches the handle
        with pytest.raises(scrooge_amd.ScroogeError):
            aligner.set_mapq(api.MapqRule(max_q=255))
        assert aligner.mapq() == (False, api.MapqRule())
        # min_keep_q > 0 with the pileup on is served
        aligner.set_pileup()
        got = aligner.align_mapping(None, reads, cands, arrays=True, best=True, mapq=api.MapqRule(min_keep_q=5))
        assert aligner.take_pileup()["n_alignments"] == int(((got["read_summary"]["flags"] & mq.KEPT) != 0).sum())
    finally:
        aligner.set_mapq(None, False)
        aligner.set_pileup(False)


# ---------------------------------------------------------------------------------------------------------------
# loader and command line
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_job_and_cli_write_graded_mapqs(aligner, tmp_path, capsys):
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=60, seed=34)
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    out = str(tmp_path / "a.sam")
    job.align(aligner, out_path=out, fmt="sam", best=True, mapq=True)
    rec = aligner.last_read_summary
    assert len(rec) == job.n_reads and not aligner.mapq()[0]
    lines = [x.split("\t") for x in open(out).read().splitlines() if not x.startswith("@")]
    assert len(lines) == job.n_reads
    # one record per read, in the reads' order: column 5 is the read's MAPQ, 0 on an unmapped record
    assert [int(x[4]) for x in lines] == [int(r["mapq"]) if r["flags"] & mq.HAS_WINNER else 0 for r in rec]
    assert all(0 <= int(x[4]) <= 60 for x in lines) and len({int(x[4]) for x in lines}) > 1
    sam2, sites = str(tmp_path / "b.sam"), str(tmp_path / "s.tsv")
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--reverse_strand", "--out=" + sam2, "--format=sam", "--mapq",
                     "--sites=" + sites, "--pileup_min_mapq=20"]) == 0
    err = capsys.readouterr().err
    n_kept = int(((rec["flags"] & mq.HAS_WINNER) != 0).sum() - ((rec["mapq"] < 20) & ((rec["flags"] & mq.HAS_WINNER) != 0)).sum())
    assert "%d of %d reads placed with MAPQ >= 20" % (n_kept, job.n_reads) in err and "piled up %d alignments" % n_kept in err
    assert open(sam2).read() == open(out).read()
    for bad in (["--mapq", "--paired"], ["--mapq", "--clip"], ["--mapq", "--distance_only"], ["--mapq", "--format=tsv"], ["--pileup_min_mapq=3"],
                ["--mapq", "--pileup_min_mapq=3"], ["--mapq_rule=1,2,3"], ["--mapq", "--mapq_rule=1,255,3"]):
        with pytest.raises(SystemExit):
            cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds] + bad)
    capsys.readouterr()
