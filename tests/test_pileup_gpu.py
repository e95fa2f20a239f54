"""The pileup on the GPU (scrooge_amd/csrc/pileup_kernels.hip; scrg_pileup_add / scrg_pileup_finish, scrg_ctx_set_pileup /
scrg_ctx_take_pileup): the device layer on synthetic run lists against the Python model (tests/pileup_model.py, which
tests/test_pileup.py holds to its brute force and the host function to it) — reads packed by the library's packer, the accumulator
between canary words — then the host calls with the setting on against the model summed over the runs the same call returns."""
import numpy as np
import pytest

from scrooge_amd import api
from tests import pileup_model as pm

OK, OVER, NOT_BEST = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST
CANARY = 0x5A5A5A5A
GUARD = 64                        # canary words in front of and behind every buffer


def revcomp(b):
    return bytes(b).translate(pm.COMP)[::-1]


class Buf:
    """7 * (target_len + 1) words of 32 bits between canary words."""

    def __init__(self, dev, target_len, fill=0):
        import torch
        self.words = pm.PLANES * (target_len + 1)
        self.all = torch.full((self.words + 2 * GUARD,), CANARY, dtype=torch.int32, device=dev)
        self.t = self.all[GUARD:GUARD + self.words]
        self.t.fill_(fill)
        self.target_len = target_len

    def planes(self):
        return self.t.cpu().numpy().view(np.uint32).reshape(pm.PLANES, self.target_len + 1).copy()

    def intact(self):
        return bool((self.all[:GUARD] == CANARY).all()) and bool((self.all[GUARD + self.words:] == CANARY).all())


def pack_reads(al, reads, dev):
    """Reads back to back, a few random bases between them (so that offsets take every value mod 32), through scrg_pack_planar
    -> (the planar words on the device, every read's offset in bases)."""
    import torch
    rng = np.random.Generator(np.random.PCG64(77))
    parts, offs, pos = [], [], 0
    for k, r in enumerate(reads):
        gap = [0, 1, 31, 13, 17, 5][k % 6]
        parts.append(np.frombuffer(pm.random_read(rng, gap), dtype=np.uint8))
        pos += gap
        offs.append(pos)
        parts.append(np.frombuffer(bytes(r), dtype=np.uint8))
        pos += len(r)
    parts.append(np.frombuffer(pm.random_read(rng, (-pos) % 32 + 32 * (api.SEQ_PAD_WORDS + 1)), dtype=np.uint8))
    flat = np.concatenate(parts)
    seq = torch.zeros(len(flat) // 32 + api.SEQ_PAD_WORDS, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    al.pack_planar(torch.from_numpy(flat.copy()).to(dev), seq, bad)
    assert int(bad) == 0
    return seq, np.array(offs, dtype=np.uint64)


def device_pileup(al, reads, which_read, read_rev, run_table, first, cnt, starts, target_len, stride=1, caps=None, status=None, stranded=1,
                  n_runs=None, finish=("in", "out")):
    """scrg_pileup_add on prepared arrays, then scrg_pileup_finish in place and out of place -> (counts, out-of-range count).
    reads: the distinct reads AS STORED; pair p has reads[which_read[p]], flagged SCRG_READ_REVCOMP where read_rev[p]; its runs are
    run_table[first[p] : first[p] + cnt[p]] (stride 6: first and caps travel in the descriptors)."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    n = len(cnt)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    seq_t, r_offs = pack_reads(al, reads, dev)
    which_read = np.asarray(which_read, dtype=np.int64)
    desc = np.zeros((n, 6), dtype=np.uint64)
    if n:
        desc[:, 2] = r_offs[which_read] | np.where(np.asarray(read_rev, bool), np.uint64(api.READ_REVCOMP), np.uint64(0))
        desc[:, 3] = np.array([len(r) for r in reads], dtype=np.uint64)[which_read]
        desc[:, 4] = first
        desc[:, 5] = cnt if caps is None else caps
    desc_t = to(desc.view(np.int64))
    runs_t = to(np.concatenate([run_table, np.zeros((1, 2), dtype=np.uint8)]))
    ro_t = None if stride == 6 else to(np.asarray(first, dtype=np.int64))
    nruns_t = to(np.asarray(cnt if n_runs is None else n_runs).astype(np.int32))
    st_t = None if status is None else to(np.asarray(status, dtype=np.int32))
    start_t = to(np.asarray(starts, dtype=np.uint64).view(np.int64))
    acc = Buf(dev, target_len)
    oor = torch.full((3,), CANARY, dtype=torch.int32, device=dev)
    oor[1] = 1000
    al.pileup_add(n, seq_t, desc_t, runs_t, ro_t, stride, nruns_t, st_t, start_t, target_len, acc.t, oor[1:], stranded=stranded)
    torch.cuda.synchronize()
    assert acc.intact()
    assert int(oor[0]) == CANARY == int(oor[2])
    edges = acc.planes()
    results = []
    if "out" in finish:
        out = Buf(dev, target_len, fill=-1)
        al.pileup_finish(target_len, acc.t, out.t)
        torch.cuda.synchronize()
        assert out.intact() and acc.intact() and np.array_equal(acc.planes(), edges)      # the accumulator still takes adds
        results.append(out.planes())
    if "in" in finish:
        al.pileup_finish(target_len, acc.t)
        torch.cuda.synchronize()
        assert acc.intact()
        results.append(acc.planes())
    for r in results:
        assert r.tobytes() == results[0].tobytes()
        assert r.tobytes() == pm.edges_to_counts(edges).tobytes()
    return results[0], int(oor[1]) - 1000


def run_items(al, items, target_len, stride=1, status=None, **kw):
    """items: [(runs, read AS ALIGNED, start, reverse)] -> device_pileup's result.  A reverse item's read is stored as its reverse
    complement and flagged."""
    reads = [revcomp(r) if rev else bytes(r) for _, r, _, rev in items] or [b"ACGT"]
    cnt = np.array([len(x[0]) for x in items], dtype=np.int64)
    if stride == 6:
        caps = np.maximum(16, (cnt + 15) // 16 * 16)
        first = np.concatenate([[0], np.cumsum(caps)])
    else:
        caps = None
        first = np.concatenate([[0], np.cumsum(cnt)])
    table = np.zeros((int(first[-1]), 2), dtype=np.uint8)
    for k, x in enumerate(items):
        if x[0]:
            table[first[k]:first[k] + len(x[0])] = [(c, ord(o)) for c, o in x[0]]
    return device_pileup(al, reads, np.arange(len(items)), [x[3] for x in items], table, first[:len(items)], cnt, [x[2] for x in items],
                         target_len, stride=stride, caps=caps, status=status, **kw)


def model_sum(items, target_len, status=None):
    want = pm.empty(target_len)
    outside = 0
    for k, (runs, read, start, _) in enumerate(items):
        if status is not None and status[k] != 0:
            continue
        outside += pm.model(runs, read, start, target_len, counts=want)[1]
    return want, outside


def check(got, want, what):
    counts, outside = got
    assert outside == want[1], what
    bad = np.argwhere(counts != want[0])
    assert len(bad) == 0, "%s: %d words differ, first at plane %d position %d: got %d want %d" % (
        what, len(bad), bad[0][0], bad[0][1], counts[tuple(bad[0])], want[0][tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------------
# the device layer
# ---------------------------------------------------------------------------------------------------------------
def hand_items():
    return [([(3, "="), (1, "X"), (2, "=")], b"ACGTAC", 4, False),
            ([(2, "I"), (2, "I"), (3, "=")], b"ACGTACG", 5, False),          # ONE insertion
            ([(4, "="), (3, "D")], b"ACGT", 23, False),                       # the D run ends exactly at target_len
            ([(3, "="), (2, "X"), (2, "=")], b"ACGGTCG", 10, True),           # stored reverse-complemented: G and T under X
            ([], b"ACGT", 7, False),                                          # no runs: nothing
            ([(2, "="), (3, "I")], b"ACGTA", 28, False)]                      # the insertion lands in slot target_len


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
def test_hand_cases(aligner, stride):
    items = hand_items()
    L = 30
    want = model_sum(items, L)
    assert want[1] == 0 and want[0][pm.INS, 5] == 1 and want[0][pm.INS, 30] == 1 and want[0][pm.DEL, 27:30].tolist() == [1, 1, 1]
    assert want[0][pm.G, 13] == 1 and want[0][pm.T, 14] == 1 and want[0][pm.A:pm.DEL].sum() == 3
    check(run_items(aligner, items, L, stride), want, "hand cases")
    for k, item in enumerate(items):                                          # and each alone
        check(run_items(aligner, [item], L, stride, finish=("in",)), model_sum([item], L), "hand case %d" % k)
    # no pairs: nothing is launched, nothing is written
    counts, outside = run_items(aligner, [], L, stride)
    assert not counts.any() and outside == 0


def seam_items(rng):
    """Engineered lists: an I stretch split across a lane seam (runs 7|8) and a tile seam (511|512), '=' runs adjacent across both (the
    filler), D stretches likewise, and X runs straddling both behind an insertion, so that a wrong read position shows."""
    out = []
    for b in (8, 512):
        for pattern in ("II", "III", "DD", "XX", "XXX", "ID", "DI", "IXI", "=="):
            for at in (b - 1, b - len(pattern) + 1):
                runs = [(5, "=")] * (b + 20)
                runs[2] = (3, "I")                                            # from here on q runs ahead of t
                runs[at:at + len(pattern)] = [(2 + k, o) for k, o in enumerate(pattern)]
                out.append(runs)
    items = []
    for k, runs in enumerate(out):
        items.append((runs, pm.random_read(rng, pm.consumed(runs)[1]), 11 * k, k % 4 == 3))
    return items


_cases = {}


def count_items():
    if not _cases:
        rng = np.random.Generator(np.random.PCG64(810))
        items = []
        for c in (24, 25, 511, 512, 513, 1025):                               # the lane / wavefront switch, the tile seams (run_walk.h)
            for k in range(4):
                runs, read = pm.random_alignment(rng, c, max_count=[3, 6, 9, 3][k], p_match=[0.45, 0.6, 0.8, 0.3][k])
                items.append((runs, read, int(rng.integers(0, 3000)), k == 1))
        _cases["items"] = items + seam_items(rng)
        _cases["L"] = 4800                                                    # two of the long pairs run over the end
        _cases["want"] = model_sum(_cases["items"], _cases["L"])
    return _cases


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
def test_forms_and_seams(aligner, stride):
    c = count_items()
    assert c["want"][1] > 0 and (c["want"][0][:, :4000].sum(axis=1) > 0).all()       # every plane is exercised; some pairs run over the end
    check(run_items(aligner, c["items"], c["L"], stride), c["want"], "forms and seams, stride %d" % stride)


@pytest.mark.gpu
def test_seam_items_alone(aligner):
    """Every engineered list as its own batch of one: what goes wrong at a seam cannot cancel against another pair."""
    rng = np.random.Generator(np.random.PCG64(811))
    for k, item in enumerate(seam_items(rng)):
        L = pm.consumed(item[0])[0] + item[2] + 3
        check(run_items(aligner, [item], L, 1, finish=("in",)), model_sum([item], L), "seam item %d" % k)


@pytest.mark.gpu
def test_three_pairs_share_a_group(aligner):
    """A batch of 3 pairs: `split` wavefronts share the one group — each long pair is walked by one of them, once."""
    rng = np.random.Generator(np.random.PCG64(812))
    items = []
    for c in (700, 30, 1300):
        runs, read = pm.random_alignment(rng, c, max_count=9, p_match=0.7)
        items.append((runs, read, int(rng.integers(0, 50)), c == 30))
    L = 9000
    for stride in (1, 6):
        check(run_items(aligner, items, L, stride), model_sum(items, L), "three pairs")


def pool_arrays(rng, n_pool, target_len):
    """A pool of alignments of 0..6 runs with their reads, starts (a few over the end) and models."""
    pool = []
    for k in range(n_pool):
        runs, read = pm.random_alignment(rng, int(rng.integers(0, 7)), max_count=40, p_match=0.5)
        start = int(rng.integers(target_len - 100, target_len + 20)) if k % 16 == 0 else int(rng.integers(0, target_len - 300))
        pool.append((runs, read, start, k % 5 == 0))
    return pool


@pytest.mark.gpu
def test_grid_stride_loop_wraps(aligner):
    """More groups of 64 short pairs than the grid has wavefronts (twice sixteen per CU, by the device's CU count): `split` is 1 and
    every wavefront takes a second group.  The pairs come from a pool of 512, tiled; the planes are the sum of the pool's models."""
    n_cus = aligner.query_launch()["n_cus"]
    n = 2 * 16 * n_cus * 64 + 64
    rng = np.random.Generator(np.random.PCG64(813))
    L = 3000
    pool = pool_arrays(rng, 512, L)
    which = (np.arange(n) * 7 + np.arange(n) // 512) % 512
    mult = np.bincount(which, minlength=512)
    want = np.zeros((pm.PLANES, L + 1), dtype=np.int64)
    outside = 0
    for k, (runs, read, start, _) in enumerate(pool):
        one, out = pm.model(runs, read, start, L)
        want += one.astype(np.int64) * int(mult[k])
        outside += int(out) * int(mult[k])
    assert outside > 0 and want.max() < 2**32
    W = 6
    table = np.zeros((512, W, 2), dtype=np.uint8)
    for k, x in enumerate(pool):
        if x[0]:
            table[k, :len(x[0])] = [(c, ord(o)) for c, o in x[0]]
    reads = [revcomp(r) if rev else r for _, r, _, rev in pool]
    cnt = np.array([len(x[0]) for x in pool], dtype=np.int64)[which]
    got = device_pileup(aligner, reads, which, np.array([x[3] for x in pool])[which], table.reshape(512 * W, 2), which * W, cnt,
                        np.array([x[2] for x in pool], dtype=np.uint64)[which], L)
    check(got, (want.astype(np.uint32), outside), "grid-stride wrap")


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 6])
def test_pair_status_and_bad_runs(aligner, stride):
    """Statuses 1, 2, 3 mixed in are not counted; no status array counts every pair.  A pair with a run that is no run lies on a stretch
    of the target no other pair touches: outside [start, start + 255 * n_runs) everything is exact."""
    rng = np.random.Generator(np.random.PCG64(814))
    items = []
    for c in (5, 5, 300, 300, 5, 300, 0, 20, 600, 600, 12, 40):
        runs, read = pm.random_alignment(rng, c, max_count=9, p_match=0.6)
        items.append((runs, read, int(rng.integers(0, 4000)), c == 20))
    status = [0, 2, 3, 0, 3, 1, 2, 1, 0, 2, 0, 0]
    L = 100000
    check(run_items(aligner, items, L, stride, status=status), model_sum(items, L, status), "statuses")
    check(run_items(aligner, items, L, stride, status=None, finish=("in",)), model_sum(items, L), "no status array")
    # runs that are no runs, in the lane form (10 runs) and in the wavefront form (300 runs: one at a lane seam, one further on), each
    # pair on its own stretch
    bad_lane, read_lane = pm.random_alignment(rng, 10, max_count=9, p_match=0.6)
    bad_lane[4] = (0, "=")
    bad_wave, read_wave = pm.random_alignment(rng, 300, max_count=9, p_match=0.6)
    bad_wave[8] = (4, "M")
    bad_wave[200] = (0, "I")
    spans = [(12000, 12000 + 255 * 10), (20000, 20000 + 255 * 300)]
    assert spans[1][1] < L
    more = items + [(bad_lane, read_lane + b"ACGT" * 8, spans[0][0], False), (bad_wave, read_wave + b"ACGT" * 8, spans[1][0], False)]
    counts, outside = run_items(aligner, more, L, stride, status=status + [0, 0], finish=("in",))
    want, want_out = model_sum(items, L, status)
    keep = np.ones(L + 1, bool)
    for a, e in spans:
        keep[a:e] = False
        assert not want[:, a:e].any()
    assert np.array_equal(counts[:, keep], want[:, keep]) and outside == want_out


@pytest.mark.gpu
def test_out_of_range(aligner):
    """Pairs that start inside the target and run over it, pairs that start at or beyond target_len: the clamped planes are exact and
    the counter is the number of such pairs.  Nothing is written outside the buffer (the canaries, device_pileup)."""
    rng = np.random.Generator(np.random.PCG64(815))
    L = 700
    items = []
    for k in range(40):
        runs, read = pm.random_alignment(rng, [6, 20, 30, 200][k % 4], max_count=9, p_match=0.6)
        span = pm.consumed(runs)[0]
        start = [L - span // 2, L, L + 1 + int(rng.integers(0, 50)), L - span, int(rng.integers(0, L // 2)), L - 1, 2**64 - 5, 2**63][k % 8]
        items.append((runs, read, max(start, 0), k % 3 == 0))
    items.append(([(3, "="), (2, "I")], b"ACGTA", L - 3, False))              # an insertion in slot target_len: inside
    items.append(([(3, "="), (1, "D"), (2, "I")], b"ACGTA", L - 3, False))    # one further: outside
    items.append(([(2, "I"), (3, "=")], b"ACGTA", L, False))                  # the insertion inside, the columns outside
    want = model_sum(items, L)
    assert 20 < want[1] < len(items) and want[0][pm.INS, L] >= 2
    for stride in (1, 6):
        check(run_items(aligner, items, L, stride), want, "out of range")
    # a target of no positions: one slot per plane
    check(run_items(aligner, items[:8], 0, 1), model_sum(items[:8], 0), "empty target")


@pytest.mark.gpu
def test_contention(aligner):
    """4096 copies of one 40-run pair at one start and 4096 staggered by one base: exact counts."""
    rng = np.random.Generator(np.random.PCG64(816))
    runs, read = pm.random_alignment(rng, 40, max_count=9, p_match=0.55)
    span = pm.consumed(runs)[0]
    L = 4096 + span + 10
    one = pm.model(runs, read, 0, span)[0].astype(np.int64)                   # (7, span + 1)
    want = np.zeros((pm.PLANES, L + 1), dtype=np.int64)
    want[:, 100:100 + span + 1] += 4096 * one
    for i in range(4096):
        want[:, i:i + span + 1] += one
    table = np.array([(c, ord(o)) for c, o in runs], dtype=np.uint8)
    n = 8192
    starts = np.concatenate([np.full(4096, 100), np.arange(4096)]).astype(np.uint64)
    got = device_pileup(aligner, [read], np.zeros(n, dtype=np.int64), np.zeros(n, bool), table, np.zeros(n, dtype=np.int64),
                        np.full(n, 40, dtype=np.int64), starts, L)
    check(got, (want.astype(np.uint32), 0), "contention")


@pytest.mark.gpu
def test_slices_cap_the_run_count(aligner):
    """Stride 6: d_n_runs is capped at cigar_cap, as for every pass over slices."""
    rng = np.random.Generator(np.random.PCG64(817))
    items = []
    for c in (40, 20, 100):
        runs, read = pm.random_alignment(rng, c, max_count=9, p_match=0.7)
        items.append((runs, read, 5 * c, False))
    caps = [16, 32, 32]
    reads = [x[1] for x in items]
    first = np.array([0, 48, 80], dtype=np.int64)
    table = np.zeros((200, 2), dtype=np.uint8)
    for k, x in enumerate(items):
        table[first[k]:first[k] + len(x[0])] = [(c, ord(o)) for c, o in x[0]]
    got = device_pileup(aligner, reads, np.arange(3), [False] * 3, table, first, np.array(caps), [x[2] for x in items], 2000, stride=6,
                        caps=np.array(caps), n_runs=[40, 20, 100])
    check(got, model_sum([(x[0][:c], x[1], x[2], False) for x, c in zip(items, caps)], 2000), "cap")


@pytest.mark.gpu
def test_device_arguments(aligner):
    import torch
    dev = torch.device("cuda", aligner.device)
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    with pytest.raises(api.ScroogeError) as e:
        aligner.pileup_add(1, z, z, z, z, 2, z, None, z, 4, z)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(api.ScroogeError) as e:
        aligner.pileup_add(1, z, z, z, z, 1, z, None, z, 4, None)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    aligner.set_text_strands(True)                                            # texts are forward only
    try:
        with pytest.raises(api.ScroogeError) as e:
            aligner.pileup_add(0, z, z, z, z, 1, z, None, z, 4, z)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    finally:
        aligner.set_text_strands(False)
    # a flagged read in a call that is not stranded is not counted
    item = hand_items()[3]
    counts, outside = run_items(aligner, [item], 30, 1, stranded=0, finish=("in",))
    assert not counts.any() and outside == 0


SCAN_SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 2**20 + 1, 2**24 + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_finish_alone(aligner, n):
    """Edges written by the test, random int32 (so sums wrap), target_len + 1 = n — one tile, tile seams, and 2^24 + 5, where the
    single workgroup that scans the tile sums loops more than once.  Against torch.cumsum in int64 mod 2^32; planes 1-4 and 6 are
    copied (out of place) or left (in place)."""
    import torch
    dev = torch.device("cuda", aligner.device)
    aligner.set_stream(0)
    L = n - 1
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    acc = Buf(dev, L)
    acc.t.copy_(torch.randint(-2**31, 2**31, (acc.words,), dtype=torch.int64, device=dev, generator=g).to(torch.int32))
    before = acc.t.clone()
    want = before.clone().view(pm.PLANES, n)
    for plane in (pm.MATCH, pm.DEL):
        s = torch.cumsum(want[plane].to(torch.int64), 0) & 0xFFFFFFFF
        want[plane] = torch.where(s >= 2**31, s - 2**32, s).to(torch.int32)
    out = Buf(dev, L, fill=7)
    aligner.pileup_finish(L, acc.t, out.t)
    torch.cuda.synchronize()
    assert acc.intact() and out.intact() and torch.equal(acc.t, before)
    assert torch.equal(out.t.view(pm.PLANES, n), want)
    aligner.pileup_finish(L, acc.t)
    torch.cuda.synchronize()
    assert acc.intact() and torch.equal(acc.t.view(pm.PLANES, n), want)


# ---------------------------------------------------------------------------------------------------------------
# the host calls
# ---------------------------------------------------------------------------------------------------------------
def host_batch():
    """The 300 noisy reads of tests/test_clip_gpu.py on their genome, two forward-text candidates each — at the text's start and 5
    bases further on — a third of the reads stored reverse-complemented (and flagged so): 600 pairs, two chunks."""
    from tests.test_clip_gpu import noisy_batch
    b = noisy_batch()
    cands = [[c[0], c[0] + 5] for c in b["cands"]]
    return {"genome": b["genome"], "reads": b["m_reads"], "aligned": b["reads"][:300], "cands": cands, "reverse": b["reverse"]}


def runs_of(arr, p):
    ro = arr["run_offset"]
    return [(int(c), chr(o)) for c, o in arr["runs"][int(ro[p]):int(ro[p + 1])]]


def model_of_result(b, arr):
    """The model summed over the call's own returned runs, starts and reads -> (counts, pairs out of range, pairs counted)."""
    L = len(b["genome"])
    want = pm.empty(L)
    outside = counted = p = 0
    for r, cs in enumerate(b["cands"]):
        for start in cs:
            runs = runs_of(arr, p)
            if arr["status"][p] == OK and runs:
                outside += pm.model(runs, b["aligned"][r], start, L, counts=want)[1]
                counted += 1
            p += 1
    return want, outside, counted


def check_take(al, want, what):
    got = al.take_pileup()
    assert got["target_len"] == want[0].shape[1] - 1 and got["counts"].shape == want[0].shape and got["counts"].dtype == np.uint32, what
    assert (got["n_out_of_range"], got["n_alignments"]) == (want[1], want[2]), what
    bad = np.argwhere(got["counts"] != want[0])
    assert len(bad) == 0, "%s: %d words differ, first at %r" % (what, len(bad), bad[0])
    with pytest.raises(api.ScroogeError) as e:                                # a take empties: handed over once
        al.take_pileup()
    assert e.value.status == api.SCRG_ERR_INVALID_ARG


def same_result(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("edit_distance", "status", "run_offset", "cigar_offset", "runs")) and a["cigar_text"] == b["cigar_text"]


@pytest.mark.gpu
def test_host_mapping(aligner):
    b = host_batch()
    aligner.set_genome(b["genome"])
    call = lambda **kw: aligner.align_mapping_directed(b["reads"], b["cands"], reverse=b["reverse"], arrays=True, **kw)
    off = call()
    assert len(off["status"]) == 600 and not aligner.pileup()
    aligner.set_pileup()
    try:
        assert aligner.pileup()
        for kw in ({"sort_by_length": 0}, {"sort_by_length": 1}):
            on = call(**kw)
            assert same_result(on, off), kw                                   # the call's own result is what it is with the setting off
            want = model_of_result(b, on)
            assert want[2] == 600 and want[0][pm.A:pm.DEL].sum() > 1000 and want[0][pm.INS].sum() > 1000
            check_take(aligner, want, "mapping %r" % kw)
        # two calls sum
        one = model_of_result(b, off)
        call()
        call(outputs=api.SCRG_OUT_TEXT)
        check_take(aligner, (2 * one[0], 2 * one[1], 2 * one[2]), "two calls")
        # best-candidate mode: the winners only
        best = call(best=True)
        assert (best["status"] == NOT_BEST).sum() == 300
        want = model_of_result(b, best)
        assert want[2] == 300
        check_take(aligner, want, "best")
        # an edit limit: the pairs over it are left out
        lim = call(max_edits=70)
        over = (lim["status"] == OVER).sum()
        want = model_of_result(b, lim)
        assert 5 < over < 595 and want[2] == 600 - over
        check_take(aligner, want, "edit limit")
        # with difference strings, the report and another CIGAR form; the staged-genome call and the plain forward call
        fw = [[c[0]] for c in b["cands"]]
        plain = aligner.align_mapping(b["genome"], b["aligned"], fw, arrays=True, diff="cs", report=True, cigar_form="merged")
        hb = dict(b, cands=fw)
        check_take(aligner, model_of_result(hb, plain), "staged genome, diff, report, merged")
    finally:
        aligner.set_pileup(False)
    again = call()
    assert same_result(again, off)
    with pytest.raises(api.ScroogeError):                                     # off: a call piles nothing up
        aligner.take_pileup()


@pytest.mark.gpu
def test_refusals(aligner):
    from tests.test_clip_gpu import noisy_batch
    b = host_batch()
    nb = noisy_batch()
    texts, reads = nb["texts"][:65], nb["reads"][:65]
    aligner.set_genome(b["genome"])
    m_reads, cands = b["aligned"][:30], [[c[0]] for c in b["cands"][:30]]
    aligner.set_pileup()
    try:
        refused = [lambda: aligner.align_pairs(texts, reads),
                   lambda: aligner.align_mapping(None, m_reads, cands, distance_only=True),
                   lambda: aligner.align_mapping(None, m_reads, cands, lanes_per_pair=64),
                   lambda: aligner.align_mapping_directed(m_reads, cands, leftward=[[1]] + [[0]] * 29),
                   lambda: aligner.align_anchored(m_reads, [[(c, 0) for c in cs] for cs in cands]),
                   lambda: aligner.align_mapping(None, m_reads, cands, clip=True),
                   lambda: aligner.align_mapping(b["genome"][:-7], m_reads, cands)]
        for k, call in enumerate(refused):
            aligner.set_genome(b["genome"])
            aligner.align_mapping(None, m_reads, cands)                       # something is accumulated ...
            with pytest.raises(api.ScroogeError) as e:
                call()
            assert e.value.status == api.SCRG_ERR_INVALID_ARG, k
            msg = aligner.lib.scrg_last_error(aligner.h).decode()
            assert "scrg_ctx_set_pileup" in msg, (k, msg)                     # the message says what refused it
            if k == len(refused) - 1:
                assert "take the pileup first" in msg
            with pytest.raises(api.ScroogeError):                             # ... and a failed call leaves nothing to take
                aligner.take_pileup()
        # a directed call without a leftward candidate is served
        aligner.set_genome(b["genome"])
        res = aligner.align_mapping_directed(m_reads, cands, leftward=[[0]] * 30, arrays=True)
        assert aligner.take_pileup()["n_alignments"] == 30 and (res["status"] == OK).all()
    finally:
        aligner.set_pileup(False)
    aligner.set_genome(b["genome"])


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path, capsys):
    """--pileup on the small job tests/test_io.py uses: the file's rows are the model's for the CIGARs the same run writes."""
    import re
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=60, seed=34)
    out, pile = str(tmp_path / "a.paf"), str(tmp_path / "p.tsv")
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--reverse_strand", "--out=" + out, "--pileup=" + pile,
                     "--pileup_min_depth=2"]) == 0
    capsys.readouterr()
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    genome, reads, cands, _ = job.views()
    lines = [x.split("\t") for x in open(out).read().splitlines()]
    assert len(lines) == job.n_pairs
    want = pm.empty(job.genome_len)
    k = 0
    for r, cs in zip(reads, cands):
        for start, rev in cs:
            cigar = [x for x in lines[k] if x.startswith("cg:Z:")][0][5:]
            runs = [(int(c), o) for c, o in re.findall(r"(\d+)([=XID])", cigar)]
            pm.model(runs, revcomp(r) if rev else r, start, job.genome_len, counts=want)
            k += 1
    ref = str(tmp_path / "want.tsv")
    job.write_pileup({"counts": want, "target_len": job.genome_len}, ref, 2)
    got = open(pile).read()
    assert got == open(ref).read()
    rows = got.splitlines()[1:]
    depth = want[:pm.INS, :job.genome_len].sum(axis=0)
    assert len(rows) == int((depth >= 2).sum()) > 100
    assert {x.split("\t")[0] for x in rows} == {"chr1", "chr2"}
