"""Soft clipping on the GPU (scrooge_amd/csrc/clip_kernels.hip; scrg_clip_device, scrg_ctx_set_clip / scrg_ctx_take_clip): the
device layer on synthetic run lists against the Python model (tests/clip_model.py, which tests/test_clip.py holds to its brute
force and the host function to it), then the host calls with clipping on against the model applied to the runs the same call
returns with clipping off."""
import numpy as np
import pytest

from scrooge_amd import api, synth
from tests import clip_model as cm
from tests.test_best_candidate import COMP

OK, OVER, NOT_BEST, OVERFLOW = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST, api.SCRG_ERR_CIGAR_OVERFLOW
FIELDS = list(cm.FIELDS)
CANARY = 0x5A5A5A5A
RUN_COUNTS = [0, 1, 24, 25, 511, 512, 513, 1024, 1025]      # the lane / wavefront switch, the tile seams (run_walk.h)


def device_clip(al, lists, stride, status=None, costs=None, apply=False, caps=None, n_runs=None):
    """scrg_clip_device on run lists -> (records: a structured array, the canary rows behind them, n_runs, first-run offsets and
    capacities afterwards, and what they were before).  stride 6: the runs lie in slices behind descriptors; 1: back to back."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    n = len(lists)
    cnt = np.array([len(x) for x in lists], dtype=np.int64)
    if stride == 6:
        caps = np.maximum(16, (cnt + 15) // 16 * 16) if caps is None else np.asarray(caps, dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(np.maximum(caps, (cnt + 15) // 16 * 16))])
    else:
        caps = np.zeros(n, dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(cnt)])
    runs = np.zeros((int(first[n]) + 1, 2), dtype=np.uint8)
    for k, x in enumerate(lists):
        if x:
            runs[first[k]:first[k] + len(x)] = [(c, ord(o)) for c, o in x]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc = np.zeros((n, 6), dtype=np.uint64)
    desc[:, 4], desc[:, 5] = first[:n], caps
    desc_t = to(desc.view(np.int64))
    off_t = to(first[:n].astype(np.int64))
    nruns_t = to((cnt if n_runs is None else np.asarray(n_runs)).astype(np.int32))
    st_t = None if status is None else to(np.asarray(status, dtype=np.int32))
    rec = torch.full((n + 3, 8), CANARY, dtype=torch.int32, device=dev)
    runs_t = to(runs)
    al.clip_device(n, runs_t, None if stride == 6 else off_t, stride, nruns_t, st_t, rec, costs=costs, apply=apply, pairs=desc_t)
    torch.cuda.synchronize()
    assert np.array_equal(runs_t.cpu().numpy(), runs)                 # the runs themselves are never written
    raw = rec.cpu().numpy().view(np.uint32)
    after = desc_t.cpu().numpy().view(np.uint64)
    return {"rec": raw[:n].copy().view(api.clip_dtype()).reshape(n), "behind": raw[n:], "n_runs": nruns_t.cpu().numpy().astype(np.int64),
            "first": (after[:, 4] if stride == 6 else off_t.cpu().numpy()).astype(np.int64), "cap": after[:, 5].astype(np.int64),
            "first0": first[:n].astype(np.int64), "cap0": caps, "n_runs0": cnt if n_runs is None else np.asarray(n_runs, dtype=np.int64)}


def check(got, want, what, stride, apply, touched=None):
    """Records against the model's; after apply the counts, offsets and capacities of the pairs that were looked at (`touched`,
    default: all), and those of the others unchanged; without it everything unchanged."""
    n = len(want)
    for p, w in enumerate(want):
        g = {f: int(got["rec"][p][f]) for f in FIELDS}
        assert g == w, "%s: pair %d: got %r want %r" % (what, p, g, w)
    assert (got["behind"] == CANARY).all(), what                      # exactly n records were written
    touched = np.ones(n, bool) if touched is None else np.asarray(touched, bool)
    nr = np.array([w["n_runs"] for w in want])
    fr = np.array([w["first_run"] for w in want])
    on = touched & apply
    assert np.array_equal(got["n_runs"], np.where(on, nr, got["n_runs0"])), what
    assert np.array_equal(got["first"], got["first0"] + np.where(on, fr, 0)), what
    if stride == 6:
        assert np.array_equal(got["cap"], got["cap0"] - np.where(on, fr, 0)), what


def seam_lists():
    """Engineered lists: gap stretches laid across a lane seam (runs 7|8) and a tile seam (511|512), the best start in an earlier
    tile than the best end, and the two ties of tests/test_clip.py laid across a tile seam."""
    out = []
    for b in (8, 512):
        for pattern in ("ID", "DI", "II", "DD", "I=D", "=I", "D="):
            for at in (b - 1, b - len(pattern) + 1):
                runs = [(5, "=")] * (b + 20)
                runs[at:at + len(pattern)] = [(2, o) for o in pattern]
                out.append(runs)
    # a poor stretch early on: the kept stretch starts behind it, in tile 0 (and in tile 1), and ends in tile 2
    for bad_at, width in ((100, 1), (520, 6)):
        runs = [(3, "=")] * 1100
        runs[bad_at:bad_at + width] = [(255, "X")] * width
        runs[-1] = (9, "I")
        out.append(runs)
    for lead in ([], [(1, "X")]):
        pad = lead + [(1, "="), (3, "X")] * 255                       # 510 / 511 runs in front: P falls, no stretch from there pays
        out.append(pad + [(5, "="), (3, "X"), (5, "=")])              # two stretches of 10 either side of the seam: the later one
        out.append(pad + [(4, "="), (2, "X"), (4, "=")])              # two starts of equal P either side of it: the earlier one
    return out


def test_seam_lists_are_what_they_say():
    """(CPU) the engineered lists do what their comments claim, by the model."""
    lists = seam_lists()
    recs = [cm.model(x) for x in lists]
    assert (recs[-4]["first_run"], recs[-4]["n_runs"], recs[-4]["score"]) == (512, 1, 10)
    assert (recs[-3]["first_run"], recs[-3]["n_runs"], recs[-3]["score"]) == (510, 3, 8)
    assert (recs[-2]["first_run"], recs[-2]["n_runs"], recs[-2]["score"]) == (513, 1, 10)
    assert (recs[-1]["first_run"], recs[-1]["n_runs"], recs[-1]["score"]) == (511, 3, 8)
    assert (recs[-6]["first_run"], recs[-6]["n_runs"]) == (101, 998) and (recs[-5]["first_run"], recs[-5]["n_runs"]) == (526, 573)
    # the lists with I next to D score one opening: charging two would differ
    assert recs[0]["score"] == 2 * 5 * 26 - (4 + 2 * 4) and recs[0]["n_runs"] == 28


_lists = {}


def count_lists():
    """Random lists at every run count of RUN_COUNTS under three cost sets, then the engineered ones."""
    if not _lists:
        rng = np.random.Generator(np.random.PCG64(710))
        lists = [cm.random_runs(rng, c, max_count=[3, 12, 255][k % 3], p_match=[0.45, 0.6, 0.8][(k // 3) % 3]) for c in RUN_COUNTS for k in range(6)]
        lists += [[(3, "I")] * 5, [(3, "X"), (2, "D")] * 20, [(7, "=")], [(7, "=")] * 40]      # only gaps (both forms), a single '='
        _lists["all"] = lists + seam_lists()
    return _lists["all"]


@pytest.mark.gpu
@pytest.mark.parametrize("apply", [False, True])
@pytest.mark.parametrize("stride", [1, 6])
@pytest.mark.parametrize("costs", [None, (1, 0, 0, 0), (3, 1, 7, 1)])
def test_device_layer(aligner, stride, apply, costs):
    lists = count_lists()
    assert {len(x) for x in lists} >= set(RUN_COUNTS)
    want = [cm.model(x, costs or cm.COSTS) for x in lists]
    if costs is None:
        assert sum(0 < w["n_runs"] < len(x) for w, x in zip(want, lists)) > 30 and sum(w["first_run"] >= 512 for w in want) > 5
    got = device_clip(aligner, lists, stride, costs=costs, apply=apply)
    check(got, want, "stride %d apply %d costs %r" % (stride, apply, costs), stride, apply)


@pytest.mark.gpu
@pytest.mark.parametrize("apply", [False, True])
def test_three_pairs_share_a_group(aligner, apply):
    """A batch of 3 pairs: `split` wavefronts share the one group — each long pair is walked by one of them, once."""
    rng = np.random.Generator(np.random.PCG64(711))
    lists = [[(9, "X"), (2, "=")] * 3 + cm.random_runs(rng, c, max_count=9, p_match=0.8) for c in (700, 30, 1300)]
    want = [cm.model(x) for x in lists]
    assert all(len(x) > 24 and 0 < w["first_run"] and w["n_runs"] > 0 for x, w in zip(lists, want))
    for stride in (1, 6):
        check(device_clip(aligner, lists, stride, apply=apply), want, "three pairs", stride, apply)


@pytest.mark.gpu
def test_grid_stride_loop_wraps(aligner):
    """More groups of 64 short pairs than the grid has wavefronts (twice sixteen per CU, by the device's CU count): `split` is 1 and
    every wavefront takes a second group.  The lists come from a pool of 512, tiled."""
    import torch
    n_cus = aligner.query_launch()["n_cus"]
    n = 2 * 16 * n_cus * 64 + 64
    assert n >= 2 * 16 * n_cus * 64 // 2 + 64
    rng = np.random.Generator(np.random.PCG64(712))
    pool = [cm.random_runs(rng, int(c), max_count=40, p_match=0.5) for c in rng.integers(0, 7, size=512)]
    pool[5] = [(3, "="), (0, "X"), (2, "=")]                          # a run that is no run: not looked at
    want_pool = np.zeros(512, dtype=api.clip_dtype())
    for k, x in enumerate(pool):
        w = cm.model(x)
        for f in FIELDS:
            want_pool[k][f] = w[f]
    L = 6
    pool_runs = np.zeros((512, L, 2), dtype=np.uint8)
    for k, x in enumerate(pool):
        if x:
            pool_runs[k, :len(x)] = [(c, ord(o)) for c, o in x]
    which = (np.arange(n) * 7 + np.arange(n) // 512) % 512
    dev = torch.device("cuda", aligner.device)
    aligner.set_stream(0)
    runs_t = torch.from_numpy(pool_runs[which].reshape(n * L, 2)).to(dev)
    off0 = np.arange(n, dtype=np.int64) * L
    cnt0 = np.array([len(x) for x in pool], dtype=np.int32)[which]
    off_t, cnt_t = torch.from_numpy(off0.copy()).to(dev), torch.from_numpy(cnt0.copy()).to(dev)
    rec = torch.full((n + 3, 8), CANARY, dtype=torch.int32, device=dev)
    aligner.clip_device(n, runs_t, off_t, 1, cnt_t, None, rec, apply=True)
    torch.cuda.synchronize()
    raw = rec.cpu().numpy().view(np.uint32)
    assert (raw[n:] == CANARY).all()
    got = raw[:n].copy().view(api.clip_dtype()).reshape(n)
    want = want_pool[which]
    assert got.tobytes() == want.tobytes()
    touched = which != 5
    assert np.array_equal(cnt_t.cpu().numpy(), np.where(touched, want["n_runs"].astype(np.int32), cnt0))
    assert np.array_equal(off_t.cpu().numpy(), off0 + want["first_run"])


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
def test_pair_status_and_bad_runs(aligner, stride):
    """Pairs over the limit (2), not best (3) and overflowed (1) mixed in, and lists with a run that is no run, on both forms: an
    all-zero record, and apply leaves them as they are.  A pair with status OK and no '=' run gets n_runs = 0."""
    rng = np.random.Generator(np.random.PCG64(713))
    lists = [cm.random_runs(rng, c, max_count=9, p_match=0.6) for c in (5, 5, 300, 300, 5, 300, 0, 20, 600, 600, 12, 40)]
    status = [0, 2, 3, 0, 3, 1, 2, 1, 0, 2, 0, 0]
    lists[10] = [(3, "I"), (2, "X")] * 6                              # OK, no '=' run
    lists[11] = [(3, "D"), (2, "X")] * 20
    bad = [list(x) for x in (lists[0], lists[3], lists[8], lists[8])]
    bad[0][2] = (0, "=")
    bad[1][299] = (4, "M")
    bad[2][0] = (0, "I")
    bad[3][520] = (1, "N")
    lists += bad
    status += [0, 0, 0, 0]
    want = [cm.model(x) if s == 0 else cm.record() for x, s in zip(lists, status)]
    assert all(w == cm.record() for w in want[12:]) and want[10] == cm.record() == want[11]
    touched = [s == 0 for s in status[:12]] + [False] * 4
    for apply in (False, True):
        got = device_clip(aligner, lists, stride, status=status, apply=apply)
        check(got, want, "status", stride, apply, touched)
        if apply:
            assert got["n_runs"][10] == 0 == got["n_runs"][11] and got["n_runs"][12] == len(lists[12])
    # no status array: every pair is OK
    got = device_clip(aligner, lists[:12], stride, status=None)
    check(got, [cm.model(x) for x in lists[:12]], "no status", stride, False)


@pytest.mark.gpu
def test_slices_cap_the_run_count(aligner):
    """Stride 6: d_n_runs is capped at cigar_cap, as for every pass over slices."""
    rng = np.random.Generator(np.random.PCG64(714))
    lists = [cm.random_runs(rng, c, max_count=9, p_match=0.7) for c in (40, 20, 100)]
    caps = [16, 32, 32]
    got = device_clip(aligner, lists, 6, caps=caps, n_runs=[40, 20, 100], apply=True)
    want = [cm.model(x[:c]) for x, c in zip(lists, caps)]
    check(got, want, "cap", 6, True)


@pytest.mark.gpu
def test_device_arguments(aligner):
    import torch
    dev = torch.device("cuda", aligner.device)
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    for kw in ({"stride": 2}, {"costs": (0, 1, 1, 1)}, {"costs": (1, 1, 1, 256)}):
        with pytest.raises(api.ScroogeError) as e:
            aligner.clip_device(1, z, z, kw.get("stride", 1), z, None, z, costs=kw.get("costs"))
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    aligner.clip_device(0, None, None, 1, None, None, None)           # no pairs: nothing to do


# ---------------------------------------------------------------------------------------------------------------
# the host calls
# ---------------------------------------------------------------------------------------------------------------
_data = {}


def noisy_batch():
    """300 reads of 300 bases (ONT errors) with 0..40 random bases spliced on at either end.  600 pairs: every read against its
    text and against its text from 5 bases further on.  The mapping call: the genome is the concatenated texts, read r has a
    rightward candidate at its text's start and a leftward one where its text ends; a third of the reads are stored
    reverse-complemented (and flagged so)."""
    if _data:
        return _data
    rng = np.random.Generator(np.random.PCG64(720))
    err, ratio = synth.PROFILES["ont"]
    texts, reads, cores = [], [], []
    for _ in range(300):
        t, q = synth.make_pair(300, err, ratio, rng, slack=0.02)
        core = synth.BASES[q].tobytes()
        cores.append(len(core))
        reads.append(synth.random_seq(int(rng.integers(0, 41)), rng) + core + synth.random_seq(int(rng.integers(0, 41)), rng))
        texts.append(synth.BASES[t].tobytes())
    starts = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    _data["texts"] = texts + [t[5:] for t in texts]
    _data["reads"] = reads + reads
    _data["genome"] = b"".join(texts)
    _data["cands"] = [[int(starts[r]), int(starts[r + 1])] for r in range(300)]
    _data["leftward"] = [[0, 1] for _ in range(300)]
    _data["reverse"] = [[int(r % 3 == 1)] * 2 for r in range(300)]
    _data["m_reads"] = [q.translate(COMP)[::-1] if r % 3 == 1 else q for r, q in enumerate(reads)]
    return _data


def runs_of(arr, p):
    ro = arr["run_offset"]
    return [(int(c), chr(o)) for c, o in arr["runs"][int(ro[p]):int(ro[p + 1])]]


def cigars_of(arr):
    off, text = arr["cigar_offset"].astype(np.int64), arr["cigar_text"]
    return [text[int(off[k]):int(off[k + 1]) - 1].decode() for k in range(len(off) - 1)]


def check_clipped(on, off, what, costs=cm.COSTS, form="windowed"):
    """`on`: a call with clipping; `off`: the same call without.  Every record is the model's for the pair's runs in `off`; the runs,
    offsets and text of `on` are those of the kept stretch (the text by scrg_cigar_from_runs in the call's form); edit distances and
    statuses are unchanged.  -> the pairs that lost runs."""
    n = len(off["status"])
    rec = on["clip"]
    assert rec.dtype == api.clip_dtype() and len(rec) == n, what
    assert np.array_equal(on["edit_distance"], off["edit_distance"]) and np.array_equal(on["status"], off["status"]), what
    ro = on["run_offset"].astype(np.int64)
    assert ro[0] == 0 and ro[n] == len(on["runs"]) and np.all(np.diff(ro) >= 0), what
    cigars = cigars_of(on)
    clipped = 0
    for p in range(n):
        full = runs_of(off, p)
        want = cm.model(full, costs) if off["status"][p] == OK else cm.record()
        assert {f: int(rec[p][f]) for f in FIELDS} == want, (what, p)
        kept = cm.kept(full, want) if off["status"][p] == OK else full
        assert runs_of(on, p) == kept, (what, p)
        assert cigars[p] == api.cigar_from_runs(form, kept), (what, p)
        clipped += len(kept) < len(full)
    return clipped


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (256, 129)])
def test_host_pairs(aligner, W, O):
    b = noisy_batch()
    texts, reads = b["texts"], b["reads"]
    off = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O)
    plain = off["runs"].tobytes(), off["cigar_text"]
    # 600 pairs are two chunks; both issue orders
    for kw, form in (({"sort_by_length": 0}, "windowed"), ({"sort_by_length": 1}, "merged"), ({}, "m")):
        ref = off if form == "windowed" else aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, cigar_form=form)
        on = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, clip=True, cigar_form=form, **kw)
        assert check_clipped(on, ref, "pairs %r %s" % (kw, form), form=form) > 300
        assert not aligner.clip()[0]                                  # the per-call keyword restores the handle's setting
    # an edit limit: the pairs over it are not looked at
    lim_off = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, max_edits=70)
    lim_on = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, max_edits=70, clip=True)
    over = lim_off["status"] == OVER
    assert 5 < over.sum() < 595 and check_clipped(lim_on, lim_off, "pairs limit") > 0
    assert (lim_on["clip"]["n_runs"][over] == 0).all()
    # other costs; the list form leaves the records in last_clip
    on = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, clip=(1, 3, 5, 1))
    check_clipped(on, off, "pairs costs", costs=(1, 3, 5, 1))
    aligner.align_pairs(texts[:20], reads[:20], W=W, O=O, clip=(1, 3, 5, 1))
    assert aligner.last_clip.tobytes() == on["clip"][:20].tobytes()
    # clipping off after clipping on: the bytes it always gave
    again = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O)
    assert (again["runs"].tobytes(), again["cigar_text"]) == plain and "clip" not in again
    for k in ("edit_distance", "status", "run_offset", "cigar_offset"):
        assert np.array_equal(again[k], off[k])


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (256, 129)])
def test_host_mapping_directed(aligner, W, O):
    """Stranded and leftward candidates; two chunks, both issue orders, best-candidate mode, an edit limit."""
    b = noisy_batch()
    aligner.set_genome(b["genome"])
    call = lambda **kw: aligner.align_mapping_directed(b["m_reads"], b["cands"], reverse=b["reverse"], leftward=b["leftward"], arrays=True, W=W, O=O, **kw)
    off = call()
    assert len(off["status"]) == 600
    for kw, form in (({"sort_by_length": 0}, "windowed"), ({"sort_by_length": 1}, "m"), ({}, "merged")):
        ref = off if form == "windowed" else call(cigar_form=form)
        assert check_clipped(call(clip=True, cigar_form=form, **kw), ref, "directed %r %s" % (kw, form), form=form) > 300
    best_off, best_on = call(best=True), call(best=True, clip=True)
    lost = best_off["status"] == NOT_BEST
    assert lost.sum() == 300 and check_clipped(best_on, best_off, "directed best") > 150
    assert (best_on["clip"]["n_runs"][lost] == 0).all() and (best_on["clip"]["n_runs"][~lost] > 0).all()
    text_only = call(best=True, clip=True, outputs=api.SCRG_OUT_TEXT | api.SCRG_OUT_BEST)
    assert text_only["clip"].tobytes() == best_on["clip"].tobytes() and text_only["cigar_text"] == best_on["cigar_text"]
    lim_off, lim_on = call(max_edits=70), call(max_edits=70, clip=True)
    over = lim_off["status"] == OVER
    assert 5 < over.sum() < 595 and check_clipped(lim_on, lim_off, "directed limit") > 0
    # the plain mapping call (forward candidates only) takes the setting, too
    fw = [[c[0]] for c in b["cands"]]
    m_off = aligner.align_mapping(None, _data["reads"][:300], fw, arrays=True, W=W, O=O)
    m_on = aligner.align_mapping(None, _data["reads"][:300], fw, arrays=True, W=W, O=O, clip=True)
    assert check_clipped(m_on, m_off, "mapping") > 150


@pytest.mark.gpu
def test_refusals_and_take_once(aligner):
    b = noisy_batch()
    texts, reads = b["texts"][:65], b["reads"][:65]
    aligner.set_genome(b["genome"])
    m_reads, cands = b["reads"][:30], [[c[0]] for c in b["cands"][:30]]
    assert aligner.clip() == (False, cm.COSTS)
    with pytest.raises(api.ScroogeError) as e:
        aligner.set_clip((0, 1, 1, 1))
    assert e.value.status == api.SCRG_ERR_INVALID_ARG and aligner.clip() == (False, cm.COSTS)
    aligner.set_clip((3, 4, 5, 6))
    try:
        assert aligner.clip() == (True, (3, 4, 5, 6))
        for call in (lambda: aligner.align_pairs(texts, reads, lanes_per_pair=8),
                     lambda: aligner.align_mapping(None, m_reads, cands, lanes_per_pair=64),
                     lambda: aligner.align_pairs(texts, reads, distance_only=True),
                     lambda: aligner.align_mapping(None, m_reads, cands, distance_only=True),
                     lambda: aligner.align_anchored(m_reads, [[(c, 0) for c in cs] for cs in cands]),
                     lambda: aligner.align_pairs(texts, reads, diff="md"),
                     lambda: aligner.align_pairs(texts, reads, diff="cs"),
                     lambda: aligner.align_mapping(None, m_reads, cands, report=True)):
            with pytest.raises(api.ScroogeError) as e:
                call()
            assert e.value.status == api.SCRG_ERR_INVALID_ARG
            assert "clip" in aligner.lib.scrg_last_error(aligner.h).decode()          # the message says what refused it
            with pytest.raises(api.ScroogeError):                     # a failed call leaves nothing to take
                aligner.take_clip()
        aligner.align_mapping(None, m_reads, cands)
        first = aligner.take_clip()
        assert len(first) == 30 and (first["n_runs"] > 0).all()
        with pytest.raises(api.ScroogeError) as e:                    # handed over once
            aligner.take_clip()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
        aligner.align_pairs(texts[:3], reads[:3])                     # records nobody took are discarded by the next call
        aligner.align_pairs(texts[:2], reads[:2])
        assert len(aligner.take_clip()) == 2
        aligner.align_pairs([], [])
        assert len(aligner.take_clip()) == 0
        # scores are summed in 32 bits: a call whose longest read and text could overflow them is refused before anything runs
        aligner.set_clip((255, 255, 255, 255))
        big = b"A" * 2200000
        with pytest.raises(api.ScroogeError) as e:
            aligner.align_pairs([big, b"ACGT"], [big, b"ACGT"])
        assert e.value.status == api.SCRG_ERR_INVALID_ARG and "2^31" in aligner.lib.scrg_last_error(aligner.h).decode()
    finally:
        aligner.set_clip(None, False)
    aligner.align_pairs(texts[:2], reads[:2])
    with pytest.raises(api.ScroogeError):                             # off: a call makes none
        aligner.take_clip()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["paf", "sam"])
def test_cli_end_to_end(tmp_path, capsys, fmt):
    """--clip on the small job tests/test_io.py uses: every record is what the model keeps of the same job's unclipped CIGAR."""
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=60, seed=34)
    common = ["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--format=" + fmt, "--reverse_strand"]
    plain, out = str(tmp_path / ("plain." + fmt)), str(tmp_path / ("clip." + fmt))
    assert cli.main(common + ["--out=" + plain]) == 0
    assert cli.main(common + ["--out=" + out, "--clip", "--clip_costs=1,3,5,1"]) == 0
    capsys.readouterr()
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    rows = lambda path: [x.split("\t") for x in open(path).read().splitlines() if not x.startswith("@")]
    a, c = rows(plain), rows(out)
    assert len(a) == len(c) == job.n_pairs
    moved = 0
    for k, (fa_, fc) in enumerate(zip(a, c)):
        cigar = fa_[5] if fmt == "sam" else [x for x in fa_ if x.startswith("cg:Z:")][0][5:]
        full = [(int(n), o) for n, o in __import__("re").findall(r"(\d+)([=XID])", cigar)]
        rec = cm.model(full, (1, 3, 5, 1))
        kept = "".join("%d%s" % r for r in cm.kept(full, rec))
        read_len = sum(n for n, o in full if o != "D")
        assert rec["n_runs"] > 0 and fc[-1] == "AS:i:%d" % rec["score"] and "NM:i:%d" % rec["n_edits"] in fc, k
        if fmt == "sam":
            head, tail = rec["read_start"], read_len - rec["read_end"]
            assert fc[5] == ("%dS" % head if head else "") + kept + ("%dS" % tail if tail else "") and fc[9] == fa_[9], k
            assert int(fc[3]) == int(fa_[3]) + rec["text_start"], k
        else:
            rev = fc[4] == "-"
            assert (int(fc[2]), int(fc[3])) == ((read_len - rec["read_end"], read_len - rec["read_start"]) if rev else (rec["read_start"], rec["read_end"])), k
            assert (int(fc[7]), int(fc[8])) == (int(fa_[7]) + rec["text_start"], int(fa_[7]) + rec["text_end"]) and "cg:Z:" + kept in fc, k
        moved += rec["n_runs"] < len(full)
    assert moved > 0
