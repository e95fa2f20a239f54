"""The pileup on the CPU (include/scrooge_amd.h: PILEUP): the rule's two Python statements against each other
(tests/pileup_model.py), the host function scrg_pileup_from_runs against them — on random lists and on alignments the oracle makes
— the interface, the writer scrg_job_write_pileup on a hand-made pileup and the CLI's argument refusals.  The kernels are held to
the same model in tests/test_pileup_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from scrooge_amd import io as sio
from tests import pileup_model as pm
from tests.test_best_candidate import write_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["scrg_ctx_set_pileup", "scrg_ctx_get_pileup", "scrg_ctx_take_pileup", "scrg_pileup_free", "scrg_pileup_add", "scrg_pileup_finish"]
NEW_IO = ["scrg_pileup_from_runs", "scrg_job_write_pileup"]


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


def test_interface(lib):
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    for name in NEW_IO:
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS, name
    assert "PILEUP:" in hdr
    names = ["MATCH", "A", "C", "G", "T", "DEL", "INS", "PLANES"]
    for value, name in enumerate(names):
        assert re.search(r"#define\s+SCRG_PILE_%s\s+%d\b" % (name, value), hdr), name
        assert getattr(api, "SCRG_PILE_" + name) == value
    assert [pm.MATCH, pm.A, pm.C, pm.G, pm.T, pm.DEL, pm.INS, pm.PLANES] == list(range(8))
    m = re.search(r"typedef struct scrg_pileup \{(.*?)\} scrg_pileup;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [f for f, _ in api.Pileup._fields_]
    # new entry points only: no struct of the interface moved
    assert lib.scrg_abi_version() == 8 == api.SCRG_ABI_VERSION
    for name in ("set_pileup", "pileup", "take_pileup", "pileup_add", "pileup_finish"):
        assert hasattr(api.Aligner, name)
    assert hasattr(sio.Job, "write_pileup")
    assert "pileup_kernels.hip" in open(os.path.join(ROOT, "scrooge_amd", "csrc", "Makefile")).read()


def random_case(rng, k):
    """Random runs with their read, a target and a start: mostly inside, often over the end, sometimes at or beyond it."""
    runs, read = pm.random_alignment(rng, int(rng.integers(0, 30)), max_count=[3, 12, 255][k % 3], p_match=[0.5, 0.3, 0.7][k % 3])
    span = pm.consumed(runs)[0]
    target_len = int(rng.integers(0, 2 * span + 8))
    where = k % 5
    if where == 0:
        start = target_len + int(rng.integers(0, 4))                  # at or beyond the end
    elif where == 1:
        start = max(0, target_len - int(rng.integers(0, span + 2)))   # runs over the end, or ends exactly at it
    else:
        start = int(rng.integers(0, target_len + 1))
    return runs, read, start, target_len


def test_the_two_statements_of_the_rule_agree():
    rng = np.random.Generator(np.random.PCG64(800))
    outside = seams = 0
    for k in range(3000):
        runs, read, start, target_len = random_case(rng, k)
        got, out = pm.model(runs, read, start, target_len)
        want, want_out = pm.brute(runs, read, start, target_len)
        assert np.array_equal(got, want) and out == want_out, (runs, read, start, target_len)
        assert (got[:pm.INS, target_len] == 0).all()                  # slot target_len: insertions only
        outside += out
        seams += any(a[1] == b[1] == "I" for a, b in zip(runs, runs[1:]))
    assert outside > 500 and seams > 300


def test_host_function_against_the_model():
    rng = np.random.Generator(np.random.PCG64(801))
    outside = 0
    for k in range(3000):
        runs, read, start, target_len = random_case(rng, k)
        want, want_out = pm.model(runs, read, start, target_len)
        got, out = api.pileup_from_runs(runs, read if k % 2 else read.lower(), start, target_len)
        assert np.array_equal(got, want) and out == want_out, (runs, read, start, target_len)
        outside += out
    assert outside > 500
    # it ADDS: two alignments into one array, and the read may be longer than the runs consume
    a, ra = pm.random_alignment(rng, 12, max_count=9)
    b, rb = pm.random_alignment(rng, 12, max_count=9)
    acc, _ = api.pileup_from_runs(a, ra, 3, 200)
    acc2, _ = api.pileup_from_runs(b, rb + b"ACGT", 10, 200, counts=acc)
    assert acc2 is acc and np.array_equal(acc, pm.model(a, ra, 3, 200)[0] + pm.model(b, rb, 10, 200)[0])
    # a start near 2^64 lies outside every target
    got, out = api.pileup_from_runs("3=", b"ACG", 2**64 - 2, 50)
    assert out and not got.any()


def test_oracle_alignments():
    """Alignments the oracle makes for seeded random pairs at W/O 64/33: the twin is the model on real window seams."""
    from oracle.pyoracle import Oracle
    texts, reads = synth.make_pairs(40, 600, "ont", seed=802)
    _, cigars, _, _ = Oracle().align(texts, reads, W=64, O=33)
    target_len = 700
    acc = pm.empty(target_len)
    want = pm.empty(target_len)
    seams = 0
    for k, (cigar, read) in enumerate(zip(cigars, reads)):
        runs = api._parse_cigar(cigar)
        seams += any(a[1] == b[1] for a, b in zip(runs, runs[1:]))
        start = 3 * k
        _, out = api.pileup_from_runs(cigar, read, start, target_len, counts=acc)
        _, want_out = pm.model(runs, read, start, target_len, counts=want)
        assert out == want_out == (start + pm.consumed(runs)[0] > target_len)
    assert seams > 30 and np.array_equal(acc, want)
    assert np.array_equal(want, sum(pm.brute(api._parse_cigar(c), r, 3 * k, target_len)[0] for k, (c, r) in enumerate(zip(cigars, reads))))
    # where all 40 start within 120 bases, far from the end, the depth is 40
    depth = want[:pm.INS].sum(axis=0)
    assert (depth[150:500] == 40).all()


def test_hand_cases():
    got, out = api.pileup_from_runs("2I2I3=", b"ACGTACG", 5, 20)
    want = pm.empty(20)
    want[pm.INS, 5] = 1                                               # the 2I2I a window seam leaves is ONE insertion
    want[pm.MATCH, 5:8] = 1
    assert np.array_equal(got, want) and not out
    # an insertion behind the last target base lands in slot target_len; one position further it is out of range
    got, out = api.pileup_from_runs("3=2I", b"ACGTA", 17, 20)
    assert got[pm.INS, 20] == 1 and got[pm.MATCH, 17:20].tolist() == [1, 1, 1] and got.sum() == 4 and not out
    got, out = api.pileup_from_runs("3=1D2I", b"ACGTA", 17, 20)
    assert got[pm.INS].sum() == 0 and got[pm.DEL].sum() == 0 and out
    # X counts the read's base as aligned; D ending exactly at target_len is inside
    got, out = api.pileup_from_runs("3=1X2=2D", b"ACGTAC", 12, 20)
    assert got[pm.T, 15] == 1 and got[pm.A:pm.DEL].sum() == 1 and got[pm.DEL, 18:20].tolist() == [1, 1] and not out
    assert np.array_equal(got, pm.brute(api._parse_cigar("3=1X2=2D"), b"ACGTAC", 12, 20)[0])
    # I D I: two insertions
    got, _ = api.pileup_from_runs("1=1I1D1I1=", b"ACGT", 0, 9)
    assert got[pm.INS, :4].tolist() == [0, 1, 1, 0]
    # no runs: nothing
    got, out = api.pileup_from_runs([], b"", 0, 9)
    assert not got.any() and not out


def test_refusals_leave_the_array_untouched():
    base, _ = api.pileup_from_runs("5=1X5=", b"ACGTACGTACG", 2, 40)
    before = base.copy()
    bad = [([(5, "="), (0, "X"), (5, "=")], b"ACGTACGTACG"),          # a zero count
           ([(5, "="), (2, "M")], b"ACGTACG"),                        # another operation
           ([(5, "="), (2, "S")], b"ACGTACG"),
           ([(5, "="), (3, "X")], b"ACGTACG"),                        # the read is shorter than the runs consume
           ([(5, "="), (3, "I")], b"ACGTACG"),
           ([(8, "=")], b"ACGTACG"),
           ([(3, "="), (2, "X"), (2, "=")], b"ACGNACG"),              # a base under X that is no base
           ([(3, "="), (2, "X"), (2, "=")], b"ACGA-CG")]
    for runs, read in bad:
        with pytest.raises(api.ScroogeError) as e:
            api.pileup_from_runs(runs, read, 1, 40, counts=base)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG, (runs, read)
        assert np.array_equal(base, before), (runs, read)
    # a base that is no base under '=' or 'I' is not looked at
    api.pileup_from_runs([(3, "="), (2, "I"), (2, "=")], b"ACNNNCG", 1, 40, counts=base)
    assert base.sum() == before.sum() + 6
    with pytest.raises(api.ScroogeError):
        api.pileup_from_runs("3=", b"ACG", 0, 40, counts=np.zeros((7, 40), dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------
def test_job_write_pileup(tmp_path):
    """A hand-made pileup on the 2 kb chromosome of tests/test_best_candidate.py's job."""
    job, chrom, reads, cands, names = write_job(tmp_path)
    L = job.genome_len
    assert L == 2000
    counts = pm.empty(L)
    counts[pm.MATCH, 100:140] = 3
    counts[pm.MATCH, 120] = 1
    counts[pm.G, 120] = 2
    counts[pm.DEL, 139] = 1
    counts[pm.INS, 130] = 2
    counts[pm.INS, 500] = 5                                           # an insertion where nothing else is: depth 0, no row
    counts[pm.A, 1999] = 1                                            # the last base
    counts[pm.INS, 2000] = 1                                          # behind the last base: no position, no row
    pile = {"counts": counts, "target_len": L, "n_alignments": 3, "n_out_of_range": 0}

    def rows(min_depth):
        path = str(tmp_path / ("p%d.tsv" % min_depth))
        job.write_pileup(pile, path, min_depth)
        lines = open(path).read().splitlines()
        assert lines[0].split("\t") == ["chrom", "pos", "ref", "depth", "match", "A", "C", "G", "T", "del", "ins"]
        return [x.split("\t") for x in lines[1:]]

    def want_row(i):
        n = counts[:, i]
        return ["chrT", str(i + 1), chr(chrom[i]).upper(), str(int(n[:pm.INS].sum()))] + [str(int(x)) for x in n]

    covered = list(range(100, 140)) + [1999]
    assert rows(1) == [want_row(i) for i in covered] == rows(0)
    assert rows(4) == [want_row(139)] and rows(3) == [want_row(i) for i in range(100, 140)] and rows(5) == []
    assert want_row(120)[3:] == ["3", "1", "0", "0", "2", "0", "0", "0"] and want_row(130)[-1] == "2"
    # a pileup of another genome's length
    short = {"counts": pm.empty(L - 1), "target_len": L - 1}
    with pytest.raises(api.ScroogeError) as e:
        job.write_pileup(short, str(tmp_path / "bad.tsv"))
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    rec = api.Pileup(L, 0, 0, None)
    assert job.lib.scrg_job_write_pileup(job.h, C.byref(rec), str(tmp_path / "null.tsv").encode(), 1) == api.SCRG_ERR_INVALID_ARG


def test_cli_arguments():
    from scrooge_amd import cli
    base = ["--reference=g.fa", "--reads=r.fq", "--seeds=s.paf"]
    for extra in (["--pileup=p.tsv", "--distance_only"], ["--pileup=p.tsv", "--clip"], ["--pileup_min_depth=3"],
                  ["--pileup=p.tsv", "--pileup_min_depth=x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2, extra
