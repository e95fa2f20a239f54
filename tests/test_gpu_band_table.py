"""The default kernel's 32-row band table (genasm_lane_kernel.hip: lane_window_table_band) on the GPU.

A round of a wavefront sweeps the band when every lane that holds a pair has a full window, walks it when every lane's banded
distance proves its window safe, and redoes the round on the full table otherwise; a back-off stops the attempts where too many
rounds are redone.  None of that may show in a result: every byte of the runs / edit streams, the run counts, lengths, edit
distances, text ends and statuses are compared with the oracle — for the shipped build, and for the test build with the band
switched off (reserved[0] = 4096) and attempted in every eligible round (8192).

The mixed batches put, in the SAME wavefront: clean 10 %-error pairs, low-complexity "AC" pairs and unrelated random pairs
(windows far above the threshold), and pairs with one block insertion of 18..22 bases and one block deletion of 8..11 bases (both
sides of the threshold: tests/test_band_proto.py).  Reads of 150..700 bases: every pair has full windows and a short last one,
lanes retire at different rounds.  Next to a hopeless lane no round commits, so the band batches hold wavefronts of clean pairs and
block pairs only, with read lengths such that a dozen rounds are eligible with 48 lanes live: there band rounds commit, single ones
are redone in between, and the back-off engages.  What each batch makes the kernel do is replayed on the CPU from the band's
restatement in C and asserted (test_the_batches_hold_what_they_say).  (The refill path: tests/test_queue_refill.py.)"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from scrooge_amd import api, synth
from tests.test_edit_limit import pack_sequences, ragged_mismatch, revcomp
from tests.test_lane_proto import CODE

NO_BAND, BAND_ALWAYS = 4096, 8192          # scrg_params.reserved[0] of the test build (genasm_kernels.h)
W, O = 64, 33


def _ac(n, rng):
    return bytes(rng.choice(np.frombuffer(b"AC", np.uint8), n))


def _ont(L, rng):
    t, q = synth.make_pair(L, *synth.PROFILES["ont"], rng)
    return synth.BASES[t].tobytes(), synth.BASES[q].tobytes()


def _block(L, rng, low, ins, dele, first):
    """One block insertion and one block deletion, each within the first 31 columns of some window, otherwise clean; the
    insertion in window `first` or the next one, the deletion two or three windows on."""
    t = _ac(L + 60, rng) if low else synth.random_seq(L + 60, rng)
    p1 = 31 * (first + int(rng.integers(0, 2))) + int(rng.integers(1, 31))
    p2 = p1 + 31 * int(rng.integers(2, 4))
    ins, dele = int(rng.integers(ins[0], ins[1] + 1)), int(rng.integers(dele[0], dele[1] + 1))
    extra = _ac(ins, rng) if low else synth.random_seq(ins, rng)
    return t, (t[:p1] + extra + t[p1:p2] + t[p2 + dele:])[:L]


MIXED = ("ont", "ac", "unrelated", "block", "ont", "block", "ont", "ac")


def _plan(kind, k, rng):
    """-> (what, read length) of pair k; pairs 64 w .. 64 w + 63 are wavefront w's first claims, and its only ones: no launch
    here has more pairs than the grid has lanes.
    mixed      the four sorts side by side in every group of 8 lanes, reads of 150..700 bases: some lane is in its short last
               windows in nearly every round, and nearly every eligible round is redone;
    unrelated  nothing else; the first wavefront's reads have 600..700 bases, so that it is still whole when the back-off engages;
    band       wavefronts in which band rounds COMMIT with many live lanes: a quarter of the lanes hold short reads and retire
               early, at different rounds, the others reads of 620..700 bases whose full windows overlap for a dozen rounds.
               Wavefront 0: clean ONT pairs and block pairs below the threshold ("sub").  Wavefront 1: two lanes with blocks above
               it ("over") as well — committed and redone rounds in one wavefront, too few redone for the back-off.  Wavefront 2:
               twelve such lanes, blocks at staggered rounds — the shipped build backs off with the wavefront nearly whole.  Any
               further pairs: mixed."""
    if kind == "unrelated":
        return "unrelated", int(rng.integers(600, 701)) if k < 64 else int(rng.integers(150, 701))
    if kind == "band" and k < 192:
        w, lane = divmod(k, 64)
        if lane % 4 == 0:
            return ("ont", "sub")[(lane // 4) % 2], int(rng.integers(150, 231))
        L = int(rng.integers(620, 701))
        if (w == 1 and lane in (21, 42)) or (w == 2 and lane % 5 == 1):
            return "over", L
        return ("ont", "sub", "ont")[lane % 3], L
    return MIXED[k % 8], int(rng.integers(150, 701))


@functools.lru_cache(maxsize=None)
def batch(kind, n, seed):
    """-> dict: texts, reads, read / text flags (which pairs a stranded / reversed-text launch stores as reverse complements)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    texts, reads = [], []
    for k in range(n):
        what, L = _plan(kind, k, rng)
        low = k % 16 >= 8
        if what == "ont":
            t, q = _ont(L, rng)
        elif what == "ac":
            t, q = _ac(L + 40, rng), _ac(L, rng)
        elif what == "unrelated":
            t, q = synth.random_seq(L + 40, rng), synth.random_seq(L, rng)
        elif what == "block":       # both sides of the threshold
            t, q = _block(L, rng, low, (18, 22), (8, 11), 0)
        elif what == "sub":         # 18 insertions cost 18, 8 or 9 deletions twice that (the window owes them back): <= BAND_SAFE, and
            # -9 <= delta <= 18 stays inside the band.  (Random surroundings only: in low-complexity ones the window walk can lose
            # the diagonal after a block, and the rest of the pair is above the threshold.)
            t, q = _block(L, rng, False, (18, 18), (8, 9), int(rng.integers(0, 12)) if L > 400 else 0)
        else:                       # "over": 21 or 22 insertions cost more than BAND_SAFE, 11 deletions leave the band
            # (where: wavefront 1 in two places well apart, wavefront 2 staggered over the rounds in which it is eligible)
            first = (9 if k % 64 == 21 else 14) if k < 128 else 7 + (k % 64 // 5) % 10
            t, q = _block(L, rng, low, (21, 22), (11, 11), first)
        texts.append(t), reads.append(q)
    return dict(texts=texts, reads=reads, rflag=rng.random(n) < 0.5, tflag=rng.random(n) < 0.5)


# ---- the rounds of a wavefront, replayed on the CPU from tests/proto/lane_band_proto.c (the band's table, restated) ----
UP, DOWN, SAFE = 10, 21, 19                 # genasm_lane_kernel.hip: BAND_UP, BAND_DOWN, BAND_SAFE
STRETCH, REDO_MAX = 32, 6                   # ... BAND_STRETCH, BAND_REDO_MAX
MANY = 40                                   # "many live lanes"


@functools.lru_cache(maxsize=None)
def _proto():
    here = os.path.dirname(os.path.abspath(__file__))
    so = os.path.join(here, "proto", "liblane_band_trace.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fopenmp", "-fPIC", "-shared", "-w", "-o", so, os.path.join(here, "proto", "lane_band_proto.c")])
    return C.CDLL(so)


def window_trace(t, q):
    """-> per window of the pair: its banded distance if the window is full (m = n = 64), -1 if not."""
    tc, qc = CODE[np.frombuffer(t, np.uint8)], CODE[np.frombuffer(q, np.uint8)]
    out = np.full(len(q) + 2, -2, dtype=np.int32)
    k = _proto().lane_band_window_trace(tc.ctypes.data_as(C.c_void_p), C.c_size_t(len(tc)), qc.ctypes.data_as(C.c_void_p), C.c_size_t(len(qc)),
                                        C.c_int(W), C.c_int(O), C.c_int(UP), C.c_int(DOWN), out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out)))
    assert 0 < k <= len(out)
    return out[:k]


def replay(b, always=False):
    """The kernel's rounds, wavefront by wavefront (pairs 64 w .. 64 w + 63): a round is eligible when every live lane's window
    is full; the back-off then leaves it to the full table, or the band is swept and the round committed if every live lane's
    banded distance is <= SAFE, redone if not.  -> per wavefront a list of (what, live lanes) per round, what in
    "short" / "committed" / "redone" / "backed off".  (The back-off as in the kernel: as soon as more than REDO_MAX rounds of a
    stretch of STRETCH band rounds were redone, the next 32 eligible rounds — doubled per stretch given up in a row, up to
    2 048 — are not attempted; always: reserved[0] = 8192.)"""
    traces = [window_trace(t, q) for t, q in zip(b["texts"], b["reads"])]
    waves = []
    for w0 in range(0, len(traces), 64):
        lanes = traces[w0:w0 + 64]
        rounds, in_stretch, redone, fails, pause = [], 0, 0, 0, 0
        for r in range(max(len(x) for x in lanes)):
            d = np.array([x[r] for x in lanes if r < len(x)])
            if (d < 0).any():
                rounds.append(("short", len(d)))
            elif pause:
                pause -= 1
                rounds.append(("backed off", len(d)))
            else:
                ok = bool((d <= SAFE).all())
                rounds.append(("committed" if ok else "redone", len(d)))
                in_stretch, redone = in_stretch + 1, redone + (not ok)
                if redone > REDO_MAX and not always:
                    pause, fails, in_stretch, redone = 32 << fails, min(fails + 1, 6), 0, 0
                elif in_stretch == STRETCH:
                    in_stretch = redone = fails = 0
        waves.append(rounds)
    return waves


def tally(rounds, what, live=1):
    return sum(1 for x, n in rounds if x == what and n >= live)


_expected = {}


def expected(oracle, key, texts, reads):
    """The oracle's answers in the units the kernels deliver, once per batch: ed, cigars, run bytes, stream bytes, text ends."""
    if key not in _expected:
        eds, cigars, _, _ = oracle.align(texts, reads, W=W, O=O)
        runs = [np.array([x for c, op in api._parse_cigar(cg) for x in (c, ord(op))], dtype=np.uint8) for cg in cigars]
        streams = [np.frombuffer(api.cigar_to_edit_stream(cg, W, O), dtype=np.uint8) for cg in cigars]
        text_end = np.array([sum(c for c, op in api._parse_cigar(cg) if op in "=XD") for cg in cigars], dtype=np.int64)
        _expected[key] = dict(ed=np.array(eds, dtype=np.int64), cigars=cigars, runs=runs, streams=streams, text_end=text_end)
    return _expected[key]


def launch(al, b, layout, mode, select=0, stranded=False, text_rev=False):
    """One scrg_align_device / _edits / _distance launch on the batch -> host arrays."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    stored_t = [revcomp(t) if (text_rev and f) else t for t, f in zip(b["texts"], b["tflag"])]
    stored_q = [revcomp(q) if (stranded and f) else q for q, f in zip(b["reads"], b["rflag"])]
    seq, t_off, r_off, stride = pack_sequences(al, stored_t, stored_q, layout)
    n = len(stored_t)
    tl = np.array([len(x) for x in stored_t], dtype=np.uint64)
    ql = np.array([len(x) for x in stored_q], dtype=np.uint64)
    t_off, r_off = t_off.astype(np.uint64), r_off.astype(np.uint64)
    if text_rev:
        t_off = t_off | np.where(b["tflag"], np.uint64(api.TEXT_REVCOMP), np.uint64(0)).astype(np.uint64)
    if stranded:
        r_off = r_off | np.where(b["rflag"], np.uint64(api.READ_REVCOMP), np.uint64(0)).astype(np.uint64)
    cap = (2 * 704 + 16 + 15) // 16 * 16
    cig_off = np.arange(n, dtype=np.uint64) * np.uint64(cap)
    desc = np.stack([t_off, tl, r_off, ql, cig_off, np.full(n, cap, dtype=np.uint64)], axis=1)
    desc_t = torch.from_numpy(desc.view(np.int64)).to(dev)
    ed = torch.full((n,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    # (waves_per_cu set by the caller — to its default — keeps small runs launches on genasm_lane_kernel: left alone, the library gives a
    # launch of at most one wavefront per SIMD to the split form, which has no band)
    p = al._params(dict(W=W, O=O, text_stride_words=stride, read_stride_words=stride, stranded=int(stranded), waves_per_cu=16))
    p.reserved[0] = select
    out = dict(cap=cap)
    if mode == "distance":
        al._check(al.lib.scrg_align_device_distance(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, ed, cnt, st)]))
    else:
        buf = torch.zeros(n * cap * 2, dtype=torch.uint8, device=dev)
        if mode == "edits":
            rc = torch.full((n,), -7, dtype=torch.int32, device=dev)
            al._check(al.lib.scrg_align_device_edits(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, buf, ed, cnt, st, rc)]))
        else:
            al._check(al.lib.scrg_align_device(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, buf, ed, cnt, st)]))
    torch.cuda.synchronize()
    if mode != "distance":
        out["buf"] = buf.cpu().numpy()
    if mode == "edits":
        out["run_count"] = rc.cpu().numpy().astype(np.int64)
    out.update(ed=ed.cpu().numpy(), status=st.cpu().numpy(), count=cnt.cpu().numpy().astype(np.int64))
    return out


def compare(res, exp, mode, what):
    n = len(res["ed"])
    assert (res["status"] == 0).all(), (what, np.flatnonzero(res["status"] != 0)[:8])
    bad = np.flatnonzero(res["ed"] != exp["ed"])
    assert len(bad) == 0, "%s: %d of %d edit distances differ, first pair %d: %d, want %d" % (what, len(bad), n, bad[0], res["ed"][bad[0]], exp["ed"][bad[0]])
    if mode == "distance":
        assert (res["count"] == exp["text_end"]).all(), (what, np.flatnonzero(res["count"] != exp["text_end"])[:8])
        return
    want = exp["streams"] if mode == "edits" else exp["runs"]
    unit = 1 if mode == "edits" else 2
    lens = np.array([len(x) // unit for x in want], dtype=np.int64)
    assert (res["count"] == lens).all(), (what, np.flatnonzero(res["count"] != lens)[:8])
    if mode == "edits":
        n_runs = np.array([len(x) // 2 for x in exp["runs"]], dtype=np.int64)
        assert (res["run_count"] == n_runs).all(), (what, np.flatnonzero(res["run_count"] != n_runs)[:8])
    flat = np.concatenate(want) if n else np.zeros(0, np.uint8)
    w_off = np.concatenate([[0], np.cumsum(unit * lens)])[:-1]
    diff = ragged_mismatch(res["buf"], 2 * res["cap"] * np.arange(n, dtype=np.int64), flat, w_off, unit * lens)
    assert len(diff) == 0, "%s: the output of %d of %d pairs differs, first pair %d (want %s)" % (what, len(diff), n, diff[0], exp["cigars"][diff[0]][:80])


def test_the_batches_hold_what_they_say(oracle):
    """(CPU.)  So that the GPU tests below cannot pass vacuously: what the batches hold by the oracle's edit distances, and — from
    the CPU restatement of the band's table, replayed round by round per wavefront — how many rounds the band form of pass 1
    commits, how many are redone on the full table and how many the back-off leaves out, with how many live lanes."""
    b = batch("mixed", 200, 1)
    exp = expected(oracle, ("mixed", 200, 1, "plain"), b["texts"], b["reads"])
    rate = exp["ed"] / np.array([len(q) for q in b["reads"]])
    assert (rate < 0.2).sum() >= 60 and (rate > 0.45).sum() >= 20          # clean and block pairs; unrelated pairs
    u = batch("unrelated", 200, 2)
    eu = expected(oracle, ("unrelated", 200, 2, "plain"), u["texts"], u["reads"])
    assert (eu["ed"] / np.array([len(q) for q in u["reads"]]) > 0.4).all()
    for key in GPU_BATCHES:
        bb = batch(*key)
        assert min(len(q) for q in bb["reads"]) >= 150 and max(len(q) for q in bb["reads"]) <= 700
        for always in (False, True):
            for w, rounds in enumerate(replay(bb, always)):
                print(key, "8192" if always else "shipped", "wavefront", w, " ".join("%s%d" % (x[0], n) for x, n in rounds))

    # the mixed batches: every whole wavefront has eligible rounds, all of them redone — next to a hopeless lane nothing commits
    for n in (64, 65, 200):
        for rounds in replay(batch("mixed", n, n))[:n // 64]:
            assert tally(rounds, "redone", 64) >= 3 and tally(rounds, "committed") == 0 and tally(rounds, "short") >= 3

    # the unrelated batch: no round ever commits; the first wavefront is whole when the back-off engages (after REDO_MAX + 1 redone
    # rounds) and stays out for the rest of its eligible rounds; reserved[0] = 8192 goes on redoing
    waves = replay(u)
    assert all(tally(r, "committed") == 0 for r in waves)
    assert tally(waves[0], "redone", 64) == REDO_MAX + 1 and tally(waves[0], "backed off", MANY) >= 8
    assert tally(replay(u, True)[0], "redone", MANY) >= REDO_MAX + 1 + 8

    # the band batches (seed 5: plain launches; seed 4: stranded reads and reversed texts), shipped and 8192 alike unless said
    for seed in (5, 4):
        bb = batch("band", 200, seed)
        shipped, always = replay(bb), replay(bb, True)
        # wavefront 0: a dozen rounds committed by 48 and more live lanes, lanes retiring in between
        assert shipped[0] == always[0] and tally(shipped[0], "committed", MANY) >= 12 and tally(shipped[0], "redone") <= 1
        assert len({n for x, n in shipped[0] if x == "short"}) >= 4
        # wavefront 1: committed and redone rounds of the nearly whole wavefront next to each other, no back-off
        r1 = shipped[1]
        assert r1 == always[1] and tally(r1, "committed", MANY) >= 8 and 2 <= tally(r1, "redone", MANY) <= REDO_MAX
        order = "".join(x[0] for x, n in r1 if x != "short")
        assert "cr" in order and "rc" in order
        # wavefront 2: the shipped build backs off with 48 lanes live, 8192 redoes and commits on
        assert tally(shipped[2], "committed", MANY) >= 3 and tally(shipped[2], "redone", MANY) == REDO_MAX + 1
        assert tally(shipped[2], "backed off", MANY) >= 3
        assert tally(always[2], "redone", MANY) > REDO_MAX + 1 and tally(always[2], "backed off") == 0


GPU_BATCHES = (("mixed", 64, 64), ("mixed", 65, 65), ("mixed", 200, 200), ("unrelated", 200, 2), ("band", 200, 5), ("band", 200, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
@pytest.mark.parametrize("n", [64, 65, 200])
def test_mixed_wavefronts(aligner, aligner_select, oracle, n, layout):
    """One wavefront exactly, one pair more, and four wavefronts with a partly filled last one; runs, edit streams and distances
    from the shipped build, and from the test build without the band and with the band in every eligible round.  (Clean, block,
    "AC" and unrelated pairs side by side: the band is swept and the round redone — see test_the_batches_hold_what_they_say.)"""
    b = batch("mixed", n, n)
    exp = expected(oracle, ("mixed", n, n, "plain"), b["texts"], b["reads"])
    for mode in ("runs", "edits", "distance"):
        compare(launch(aligner, b, layout, mode), exp, mode, "shipped, %s, %d pairs, %s" % (mode, n, layout))
        for select in (NO_BAND, BAND_ALWAYS):
            compare(launch(aligner_select, b, layout, mode, select), exp, mode, "reserved[0] = %d, %s, %d pairs, %s" % (select, mode, n, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
def test_band_rounds_commit(aligner, aligner_select, oracle, layout):
    """Wavefronts whose band rounds COMMIT with 48 and more live lanes: the band form of pass 1, its stop marks and the way back to
    the full form's row and masks make the output.  One wavefront commits throughout, one redoes single rounds in between, one
    backs off (shipped) or goes on (8192); the last, partly filled one is mixed."""
    b = batch("band", 200, 5)
    exp = expected(oracle, ("band", 200, 5, "plain"), b["texts"], b["reads"])
    for mode in ("runs", "edits", "distance"):
        compare(launch(aligner, b, layout, mode), exp, mode, "shipped, %s, %s" % (mode, layout))
        for select in (NO_BAND, BAND_ALWAYS):
            compare(launch(aligner_select, b, layout, mode, select), exp, mode, "reserved[0] = %d, %s, %s" % (select, mode, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
def test_unrelated_pairs_only(aligner, aligner_select, oracle, layout):
    """Every eligible round is redone.  The first wavefront (reads of 600..700 bases) has a dozen and a half of them: the shipped
    build backs off after seven, the test build (8192) never does.  The other wavefronts' reads retire at all rounds: three or four
    eligible rounds each, redone."""
    b = batch("unrelated", 200, 2)
    exp = expected(oracle, ("unrelated", 200, 2, "plain"), b["texts"], b["reads"])
    for mode in ("runs", "edits", "distance"):
        compare(launch(aligner, b, layout, mode), exp, mode, "shipped, %s, %s" % (mode, layout))
        compare(launch(aligner_select, b, layout, mode, BAND_ALWAYS), exp, mode, "reserved[0] = 8192, %s, %s" % (mode, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
def test_stranded_reads_and_reversed_texts(aligner, aligner_select, oracle, layout):
    """What the table is fed changes: a read stored as its reverse complement (the pattern's planes come from the other end,
    inverted) and a text taken as the reverse complement of its stretch, half of the pairs each, in wavefronts that commit band
    rounds, redo some and back off (the band batch), with a mixed last one."""
    b = batch("band", 200, 4)
    exp = expected(oracle, ("band", 200, 4, "plain"), b["texts"], b["reads"])
    for al, select in ((aligner, 0), (aligner_select, BAND_ALWAYS), (aligner_select, NO_BAND)):
        for mode in ("runs", "edits", "distance"):
            compare(launch(al, b, layout, mode, select, stranded=True), exp, mode, "stranded, reserved[0] = %d, %s, %s" % (select, mode, layout))
        al.set_text_strands(True)
        try:
            for mode in ("runs", "edits", "distance"):
                compare(launch(al, b, layout, mode, select, text_rev=True), exp, mode, "reversed texts, reserved[0] = %d, %s, %s" % (select, mode, layout))
            compare(launch(al, b, layout, "runs", select, stranded=True, text_rev=True), exp, "runs", "both, reserved[0] = %d, %s" % (select, layout))
        finally:
            al.set_text_strands(False)
