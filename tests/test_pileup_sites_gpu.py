"""The pileup sites on the GPU (scrooge_amd/csrc/site_kernels.hip; scrg_pileup_sites_mark / scrg_pileup_sites_write,
scrg_ctx_take_pileup_sites): the device passes alone on counts the test writes — counts, scratch, site count and records all
between canary words, the genome packed by the library's packer at base offsets 0, 1 and 31 — against the numpy model
(tests/site_model.py, which tests/test_pileup_sites.py holds to its plain-integer statement and the host twin to it), record for
record and byte for byte; then the handle's take against the model applied to a full take of the same calls, and the CLI."""
import numpy as np
import pytest

from scrooge_amd import api
from tests import site_model as sm
from tests.test_pileup_gpu import GUARD, Buf, host_batch, same_result

# the kernels' geometry (site_kernels.hip: SITE_TILE; block_scan.h: SCAN_THREADS), which scrg_pileup_sites_scratch_bytes shows
TILE, SCAN_THREADS = 4096, 1024
CANARY64 = 0x5A5A5A5A5A5A5A5A
# target_len + 1: one wavefront, one tile and their seams, many tiles, and more tiles than the single workgroup that scans the tile
# counts takes in one round
SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 65537, 2**20 + 1, SCAN_THREADS * TILE + TILE + 2]
OFFSETS = [0, 1, 31]


@pytest.mark.gpu
def test_sizes_name_the_kernels_geometry(aligner):
    """(no GPU work: the scratch size is the geometry) 16 bytes, and a 64-word bitmap and a count per tile of 4096 positions"""
    for L in (0, 1, TILE, TILE + 1, 10 * TILE - 1, SIZES[-1] - 1):
        assert aligner.pileup_sites_scratch_bytes(L) == (16 + (L + TILE - 1) // TILE * (TILE // 64 * 8 + 4) + 7) // 8 * 8
    assert (SIZES[-1] - 1 + TILE - 1) // TILE > SCAN_THREADS          # the scan of the tile counts loops more than once
    assert aligner.pileup_sites_scratch_bytes(2**32 - 1) == 0


class Guarded:
    """n 64-bit words between canary words, filled with a pattern (a buffer that need not be initialised is not)."""

    def __init__(self, dev, n, fill=0x7777777777777777):
        import torch
        self.n = n
        self.all = torch.full((n + 2 * GUARD,), CANARY64, dtype=torch.int64, device=dev)
        self.t = self.all[GUARD:GUARD + n]
        self.t.fill_(fill)

    def intact(self):
        return bool((self.all[:GUARD] == CANARY64).all()) and bool((self.all[GUARD + self.n:] == CANARY64).all())


def pack_genome(al, genome, off, dev):
    """`off` random bases, the genome, random bases up to whole words and the pad, through scrg_pack_planar: base 0 of the genome is
    base `off` of the words."""
    import torch
    rng = np.random.Generator(np.random.PCG64(off + 5))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    tail = (-(off + len(genome))) % 32 + 32 * (api.SEQ_PAD_WORDS + 1)
    flat = np.concatenate([letters[rng.integers(0, 4, off)], np.frombuffer(genome, dtype=np.uint8), letters[rng.integers(0, 4, tail)]])
    seq = torch.zeros(len(flat) // 32 + api.SEQ_PAD_WORDS, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    al.pack_planar(torch.from_numpy(flat.copy()).to(dev), seq, bad)
    assert int(bad) == 0
    return seq


def forced_positions(L):
    """the last position of a wavefront, of a tile and of the target, and the first of the next (or of the target)"""
    want = {0, 63, 64, 127, 128, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, L - 1, L - 2, L - 64, L - 65, (L - 1) // 64 * 64, (L - 1) // 64 * 64 - 1,
            (L - 1) // TILE * TILE, (L - 1) // TILE * TILE - 1, SCAN_THREADS * TILE - 1, SCAN_THREADS * TILE}
    return np.array(sorted(p for p in want if 0 <= p < L), dtype=np.int64)


def make_counts(rng, L, ref, density):
    """-> (counts (7, L + 1), rule).  Slot L holds insertions (and must never be a site)."""
    counts = np.zeros((7, L + 1), dtype=np.uint32)
    pos = np.arange(L)
    if density == "none":                       # every read agrees, nothing is inserted; some positions uncovered
        counts[0, :L] = rng.integers(0, 5, L)
        rule = (1, 1, 0)
    elif density == "all":                      # every position covered and a site of (1, 0, 0): all alleles, calls and flags occur
        counts[:, :L] = rng.integers(0, 4, (7, L))
        counts[0, :L] += 1
        rule = (1, 0, 0)
    else:                                       # sparse: agreeing background, sites at the seams and a few elsewhere
        counts[0, :L] = rng.integers(3, 7, L)
        at = forced_positions(L)
        if L > 300:
            at = np.union1d(at, rng.choice(L, max(3, L // 3000), replace=False))
        kind = rng.integers(0, 3, len(at))
        other = (ref[at].astype(np.int64) + rng.integers(1, 4, len(at))) % 4
        counts[1 + other[kind == 0], at[kind == 0]] = rng.integers(2, 4, int((kind == 0).sum()))
        counts[5, at[kind == 1]] = rng.integers(2, 9, int((kind == 1).sum()))      # deletions, sometimes the majority
        counts[6, at[kind == 2]] = rng.integers(2, 4, int((kind == 2).sum()))      # insertions alone
        counts[6, pos[::97]] += 1                                                   # single insertions: below min_alt
        rule = (3, 2, 200)
    counts[6, L] = 7
    return counts, rule


def run_device(al, dev, counts, seq, off, rule, want, what):
    """mark, write with cap = n_sites, write with cap = n_sites - 1: everything the issue asserts for one packing of the genome"""
    import torch
    L = counts.shape[1] - 1
    acc = Buf(dev, L)
    acc.t.copy_(torch.from_numpy(counts.view(np.int32).reshape(-1)).to(dev))
    before = acc.t.clone()
    sbytes = al.pileup_sites_scratch_bytes(L)
    assert sbytes % 8 == 0 and sbytes >= 16
    scratch = Guarded(dev, sbytes // 8)
    n_dev = Guarded(dev, 1)
    al.pileup_sites_mark(L, acc.t, seq, off, rule, scratch.t, n_dev.t)
    torch.cuda.synchronize()
    n = int(n_dev.t[0])
    assert n == len(want), "%s: %d sites, the model has %d" % (what, n, len(want))
    assert acc.intact() and scratch.intact() and n_dev.intact() and torch.equal(acc.t, before), what
    for cap in sorted({n, max(n - 1, 0)}, reverse=True):
        out = Guarded(dev, 5 * max(n, 1), fill=CANARY64)
        n_dev.t.fill_(-1)
        if cap == n:
            al.pileup_sites_write(L, acc.t, seq, off, scratch.t, cap, out.t)
        else:       # (a second mark first: the write reads what THIS mark left, and *d_n_sites is the full count whatever the cap)
            al.pileup_sites_mark(L, acc.t, seq, off, rule, scratch.t, n_dev.t)
            al.pileup_sites_write(L, acc.t, seq, off, scratch.t, cap, out.t)
        torch.cuda.synchronize()
        assert acc.intact() and scratch.intact() and n_dev.intact() and out.intact() and torch.equal(acc.t, before), (what, cap)
        if cap != n:
            assert int(n_dev.t[0]) == n, (what, cap)
        raw = out.t.cpu().numpy()
        got = raw[:5 * cap].view(np.uint8).view(sm.DTYPE)
        if got.tobytes() != want[:cap].tobytes():
            bad = [k for k in range(cap) if got[k].tobytes() != want[k].tobytes()]
            raise AssertionError("%s, cap %d: %d records differ, first %d: %r, the model has %r" % (what, cap, len(bad), bad[0], got[bad[0]], want[bad[0]]))
        assert (raw[5 * cap:].view(np.uint64) == CANARY64).all(), "%s: written beyond cap %d" % (what, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_device_passes(aligner, n):
    """target_len + 1 = n, three densities; the model is made once per density and held against the passes on all three packings."""
    import torch
    dev = torch.device("cuda", aligner.device)
    aligner.set_stream(0)
    L = n - 1
    rng = np.random.Generator(np.random.PCG64(n))
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].tobytes()
    ref = sm.ref_codes(genome)
    seqs = [(off, pack_genome(aligner, genome, off, dev)) for off in OFFSETS]
    for density in ("none", "all", "sparse"):
        counts, rule = make_counts(rng, L, ref, density)
        want = sm.sites(counts, ref, rule)
        if density == "none":
            assert len(want) == 0
        elif density == "all":
            assert len(want) == L
            if L > 4000:
                assert set(np.unique(want["alt"])) == {0, 1, 2, 3, 4, 255} and set(np.unique(want["flags"])) == {0, 1, 2, 3, 5, 7}
        elif L:
            at = forced_positions(L)
            assert 0 < len(want) < max(L, 2) and np.isin(at, want["pos"].astype(np.int64)).all()
            if L > 60000:
                assert len(want) < L // 50 and (want["flags"] & 2).any() and (want["alt"] == 4).any() and (want["flags"] & 4).any()
        for off, seq in seqs:
            run_device(aligner, dev, counts, seq, off, rule, want, "n %d, %s, offset %d" % (n, density, off))


@pytest.mark.gpu
def test_device_refusals(aligner):
    import torch
    dev = torch.device("cuda", aligner.device)
    aligner.set_stream(0)
    L = 100
    z = torch.zeros(7 * (L + 1) + 64, dtype=torch.int64, device=dev)
    scratch = torch.zeros(aligner.pileup_sites_scratch_bytes(L) // 8, dtype=torch.int64, device=dev)
    mark = lambda **kw: aligner.pileup_sites_mark(**dict(dict(target_len=L, counts_u32=z, seq=z, genome_off=0, rule=(1, 1, 0), scratch_u8=scratch, n_sites_i64=z), **kw))
    write = lambda **kw: aligner.pileup_sites_write(**dict(dict(target_len=L, counts_u32=z, seq=z, genome_off=0, scratch_u8=scratch, cap=4, sites_u8=z), **kw))
    mark()
    write()
    refused = [lambda: mark(rule=(0, 1, 0)), lambda: mark(rule=(1, 1, 1001)), lambda: mark(rule=(1, 1, 0, 1)),
               lambda: mark(counts_u32=None), lambda: mark(seq=None), lambda: mark(scratch_u8=None), lambda: mark(n_sites_i64=None),
               lambda: mark(target_len=2**32 - 1), lambda: mark(target_len=2**40), lambda: mark(scratch_u8=scratch.view(torch.int32)[1:]),
               lambda: write(counts_u32=None), lambda: write(seq=None), lambda: write(scratch_u8=None), lambda: write(sites_u8=None),
               lambda: write(target_len=2**32 - 1), lambda: write(scratch_u8=scratch.view(torch.int32)[1:])]
    for k, call in enumerate(refused):
        with pytest.raises(api.ScroogeError) as e:
            call()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG, k
    write(cap=0, sites_u8=None)                                               # nothing to store: no array needed
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# the handle's take
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_host_take(aligner):
    b = host_batch()
    L = len(b["genome"])
    ref = sm.ref_codes(b["genome"])
    aligner.set_genome(b["genome"])
    call = lambda **kw: aligner.align_mapping_directed(b["reads"], b["cands"], reverse=b["reverse"], arrays=True, **kw)
    off = call()
    with pytest.raises(api.ScroogeError):                                     # the setting is off: nothing can be taken
        aligner.take_pileup_sites()
    aligner.set_pileup()
    try:
        with pytest.raises(api.ScroogeError) as e:                            # on, and nothing accumulated yet
            aligner.take_pileup_sites()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
        on = call()
        full = aligner.take_pileup()
        depth = full["counts"][:6, :L].astype(np.int64).sum(axis=0)
        for rule in ((1, 1, 0), (3, 2, 200), (1, 0, 0)):
            assert same_result(call(), off), rule
            got = aligner.take_pileup_sites(*rule)
            want = sm.sites(full["counts"], ref, rule)
            assert got["sites"].dtype == sm.DTYPE and got["n_sites"] == len(got["sites"]) == len(want), rule
            assert got["sites"].tobytes() == want.tobytes(), rule
            assert (got["target_len"], got["n_alignments"], got["n_out_of_range"]) == (L, full["n_alignments"], full["n_out_of_range"]), rule
            assert got["n_alignments"] == 600
            if rule == (1, 0, 0):
                assert np.array_equal(got["sites"]["pos"].astype(np.int64), np.nonzero(depth >= 1)[0])
            else:
                assert 0 < got["n_sites"] < L, rule
            for take in (aligner.take_pileup_sites, aligner.take_pileup):     # a take empties: handed over once
                with pytest.raises(api.ScroogeError) as e:
                    take()
                assert e.value.status == api.SCRG_ERR_INVALID_ARG
        assert same_result(on, off)
        # a refused rule keeps the accumulator
        call()
        for rule in ((0, 1, 0), (1, 1, 1001)):
            with pytest.raises(api.ScroogeError) as e:
                aligner.take_pileup_sites(*rule)
            assert e.value.status == api.SCRG_ERR_INVALID_ARG
        assert aligner.take_pileup_sites(3, 2, 200)["sites"].tobytes() == sm.sites(full["counts"], ref, (3, 2, 200)).tobytes()
        # another genome, of another length, or none: refused, and the accumulator is kept for the full take
        call()
        aligner.set_genome(b["genome"][:-7])
        with pytest.raises(api.ScroogeError) as e:
            aligner.take_pileup_sites()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG and "scrg_ctx_take_pileup" in aligner.lib.scrg_last_error(aligner.h).decode()
        aligner.clear_genome()
        with pytest.raises(api.ScroogeError) as e:
            aligner.take_pileup_sites()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
        again = aligner.take_pileup()
        assert again["counts"].tobytes() == full["counts"].tobytes() and again["n_alignments"] == 600
    finally:
        aligner.set_pileup(False)
        aligner.set_genome(b["genome"])
    assert same_result(call(), off)
    with pytest.raises(api.ScroogeError):                                     # off again: a call piles nothing up
        aligner.take_pileup_sites()


# ---------------------------------------------------------------------------------------------------------------
# the CLI
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_end_to_end(tmp_path, capsys):
    """--sites alone (the device path) and --pileup with --sites (one full take, the host twin) on the small job tests/test_io.py
    uses: both site files are write_sites of the host twin on the pileup file read back, and the model's records."""
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    from tests.test_io import make_dataset
    fa, fq, seeds, _, _ = make_dataset(str(tmp_path), n_reads=60, seed=34)
    base = ["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--reverse_strand"]
    alone, both, pile = str(tmp_path / "s1.tsv"), str(tmp_path / "s2.tsv"), str(tmp_path / "p.tsv")
    for rule in ((1, 1, 0), (2, 1, 400)):
        arg = [] if rule == (1, 1, 0) else ["--sites_rule=%d,%d,%d" % rule]
        assert cli.main(base + ["--sites=" + alone] + arg) == 0
        assert cli.main(base + ["--pileup=" + pile, "--sites=" + both] + arg) == 0
        capsys.readouterr()
        job = sio.Job(fa, fq, seeds, reverse_strand=1)
        genome = job.genome()
        L = job.genome_len
        # the pileup file read back: a position without a row is uncovered (its insertions are lost, and never make a site)
        first = {"chr1": 0, "chr2": 6000}
        counts = np.zeros((7, L + 1), dtype=np.uint32)
        for row in open(pile).read().splitlines()[1:]:
            x = row.split("\t")
            counts[:, first[x[0]] + int(x[1]) - 1] = [int(v) for v in x[4:11]]
        found = api.pileup_sites_from_counts(counts, genome, *rule)
        model = sm.sites(counts, sm.ref_codes(genome), rule)
        assert found.tobytes() == model.tobytes() and len(found) > 20
        want = str(tmp_path / "want.tsv")
        job.write_sites({"sites": found, "target_len": L}, want)
        assert open(both).read() == open(want).read() == open(alone).read(), rule
        rows = open(alone).read().splitlines()[1:]
        assert len(rows) == len(found) and {x.split("\t")[0] for x in rows} == {"chr1", "chr2"}
