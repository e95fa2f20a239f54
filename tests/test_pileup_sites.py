"""The pileup sites on the CPU (include/scrooge_amd.h: PILEUP SITES): the numpy model (tests/site_model.py, written from the rule's
text) against its own plain-integer statement, the host twin scrg_pileup_sites_from_counts against the model — record for record,
byte for byte — on hand-written counts and on random ones, the interface, the writer scrg_job_write_sites on a two-chromosome job
and the CLI's argument refusals.  The kernels are held to the same model in tests/test_pileup_sites_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from scrooge_amd import io as sio
from tests import site_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["scrg_ctx_take_pileup_sites", "scrg_pileup_sites_free", "scrg_pileup_sites_scratch_bytes", "scrg_pileup_sites_mark", "scrg_pileup_sites_write"]
NEW_IO = ["scrg_pileup_sites_from_counts", "scrg_job_write_sites"]
M32 = 2**32 - 1
A, Cc, G, T = 0, 1, 2, 3


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
    assert "PILEUP SITES:" in hdr
    for name, value in (("SCRG_SITE_DEL", 4), ("SCRG_SITE_NONE", 255), ("SCRG_SITE_F_NONREF", 1), ("SCRG_SITE_F_INS", 2), ("SCRG_SITE_F_CALL", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
        assert getattr(api, name) == value
    assert (sm.DEL, sm.NONE, sm.F_NONREF, sm.F_INS, sm.F_CALL) == (4, 255, 1, 2, 4)

    def fields(struct):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S)
        return re.findall(r"\b(\w+)\s*(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))

    assert fields("scrg_site_rule") == [f for f, _ in api.SiteRule._fields_]
    assert fields("scrg_site") == list(api.site_dtype().names) == list(sm.DTYPE.names)
    assert fields("scrg_pileup_sites") == [f for f, _ in api.PileupSites._fields_]
    assert api.site_dtype().itemsize == 40 == sm.DTYPE.itemsize and api.site_dtype() == sm.DTYPE
    assert C.sizeof(api.SiteRule) == 16 and C.sizeof(api.PileupSites) == 56
    # new entry points only: no struct of the interface moved
    assert lib.scrg_abi_version() == 8 == api.SCRG_ABI_VERSION
    for name in ("take_pileup_sites", "pileup_sites_mark", "pileup_sites_write", "pileup_sites_scratch_bytes"):
        assert hasattr(api.Aligner, name)
    assert hasattr(sio.Job, "write_sites") and hasattr(api, "pileup_sites_from_counts")
    mk = open(os.path.join(ROOT, "scrooge_amd", "csrc", "Makefile")).read()
    assert "site_kernels.hip" in mk and "site_rule.h" in mk
    # the kernel and the host twin compile one text
    for src in ("site_kernels.hip", "scrg_io.cpp"):
        assert '#include "site_rule.h"' in open(os.path.join(ROOT, "scrooge_amd", "csrc", src)).read()


def counts_of(cols):
    """[(c0 .. c6)] per position -> (7, len + 1) counts with an empty slot target_len"""
    out = np.zeros((7, len(cols) + 1), dtype=np.uint32)
    for g, c in enumerate(cols):
        out[:, g] = c
    return out


def twin(counts, genome, rule, **kw):
    return api.pileup_sites_from_counts(counts, genome, *rule, **kw)


def count_only(counts, genome, rule, reserved=0):
    """the C call with out = NULL -> (status, *n_sites)"""
    genome = genome.encode("latin-1") if isinstance(genome, str) else bytes(genome)
    n = C.c_uint64(0)
    st = api._lazy(api.load_library(), "scrg_pileup_sites_from_counts")(C.c_void_p(counts.ctypes.data), len(genome), genome,
                                                                        C.byref(api.SiteRule(*rule, reserved)), None, 0, C.byref(n))
    return st, n.value


def same(got, want):
    return got.dtype == want.dtype and len(got) == len(want) and got.tobytes() == want.tobytes()


def check(cols, genome, rule):
    counts = counts_of(cols)
    want = sm.sites(counts, sm.ref_codes(genome), rule)
    # the model's vectorised statement against its plain-integer one
    by_one = [(g,) + sm.one(c, int(sm.ref_codes(genome)[g]), rule)[1:] for g, c in enumerate(cols) if sm.one(c, int(sm.ref_codes(genome)[g]), rule)[0]]
    assert [(int(s["pos"]), int(s["alt"]), int(s["call"]), int(s["flags"])) for s in want] == by_one
    got = twin(counts, genome, rule)
    assert same(got, want), (rule, got, want)
    assert count_only(counts, genome, rule) == (api.SCRG_OK, len(want))
    return want


def test_tie_rules():
    # alt: C and T tie at 3 -> the smaller code; G and deleted tie -> G; reference A
    w = check([(4, 0, 3, 0, 3, 0, 0), (4, 0, 0, 2, 0, 2, 0), (0, 0, 0, 0, 5, 5, 0)], "AAA", (1, 1, 0))
    assert [int(x) for x in w["alt"]] == [Cc, G, T] and [int(x) for x in w["call"]] == [A, A, T]
    # call: a tie between alt and the reference keeps the reference; one more observation moves it
    w = check([(3, 0, 0, 3, 0, 0, 0), (3, 0, 0, 4, 0, 0, 0), (1, 2, 0, 3, 0, 0, 0)], "AAA", (1, 1, 0))
    assert [int(x) for x in w["call"]] == [A, G, A] and [int(x) for x in w["flags"]] == [1, 1 | 4, 1]
    # the same with every reference base: the alleles rotate
    for r, ch in enumerate("ACGT"):
        cols = [tuple([5] + [2 if b != r else 0 for b in range(4)] + [2, 0])]
        w = check(cols, ch, (1, 1, 0))
        assert int(w["alt"][0]) == (1 if r == 0 else 0) and int(w["call"][0]) == r


def test_threshold_at_equality_and_one_below():
    # depth 10, 2 nonref: 2 * 1000 == 200 * 10 passes, 201 does not; depth 7, 1 nonref: 1000 >= 142 * 7 = 994, not 143 * 7 = 1001
    cols = [(8, 0, 2, 0, 0, 0, 0), (6, 0, 0, 0, 1, 0, 0)]
    assert [int(p) for p in check(cols, "AA", (1, 1, 200))["pos"]] == [0]
    assert [int(p) for p in check(cols, "AA", (1, 1, 201))["pos"]] == []
    assert [int(p) for p in check(cols, "AA", (1, 1, 142))["pos"]] == [0, 1]
    assert [int(p) for p in check(cols, "AA", (1, 1, 143))["pos"]] == [0]
    # min_alt at equality and one above; min_depth at equality and one above
    assert len(check(cols, "AA", (1, 2, 0))) == 1 and len(check(cols, "AA", (1, 3, 0))) == 0
    assert len(check(cols, "AA", (7, 1, 0))) == 2 and len(check(cols, "AA", (8, 1, 0))) == 1 and len(check(cols, "AA", (11, 1, 0))) == 0
    # per mille 1000: every observation disagrees
    assert [int(p) for p in check([(0, 0, 4, 0, 0, 0, 0), (1, 0, 4, 0, 0, 0, 0)], "AA", (1, 1, 1000))["pos"]] == [0]


def test_min_alt_zero_is_coverage():
    cols = [(0, 0, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 4), (2, 0, 0, 1, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0)]
    w = check(cols, "ACGTA", (1, 0, 0))
    assert [int(p) for p in w["pos"]] == [1, 3, 4]                      # exactly the positions of depth >= 1
    assert [int(x) for x in w["alt"]] == [sm.NONE, G, sm.NONE] and [int(x) for x in w["flags"]] == [0, 1, 0]
    assert [int(p) for p in check(cols, "ACGTA", (2, 0, 0))["pos"]] == [1, 3]
    # min_alt 0 with a share: agreeing positions pass only with share 0
    assert [int(p) for p in check(cols, "ACGTA", (1, 0, 1))["pos"]] == [3]


def test_insertion_only_deletion_majority_and_own_x_plane():
    cols = [(6, 0, 0, 0, 0, 0, 3),        # every read agrees, three insertions in front
            (0, 0, 0, 0, 0, 0, 9),        # insertions where nothing else is: depth 0, never a site
            (2, 0, 0, 0, 0, 5, 0),        # a deletion majority
            (2, 0, 3, 0, 0, 0, 0),        # reference C with a count in its OWN X plane (a device caller can make it): 5 agree
            (2, 0, 3, 0, 4, 0, 1)]        # ... and T below them: alt T, call stays C
    w = check(cols, "GACCC", (1, 1, 0))
    assert [int(p) for p in w["pos"]] == [0, 2, 4]
    assert (int(w["alt"][0]), int(w["call"][0]), int(w["flags"][0])) == (sm.NONE, G, sm.F_INS)
    assert (int(w["alt"][1]), int(w["call"][1]), int(w["flags"][1])) == (sm.DEL, sm.DEL, sm.F_NONREF | sm.F_CALL)
    assert (int(w["alt"][2]), int(w["call"][2]), int(w["flags"][2])) == (T, Cc, sm.F_NONREF | sm.F_INS)
    assert len(check(cols, "GACCC", (1, 4, 0))) == 2                    # the insertions alone no longer carry position 0


def test_counts_near_two_to_the_32():
    cols = [(M32, M32, M32, 0, 0, M32, 0),            # depth 4 * (2^32 - 1) > 2^32
            (M32, 0, 0, 0, 0, 0, M32),
            (M32, M32, M32, M32, M32, M32, M32),
            (1, 0, M32, 0, 0, 0, 0)]
    for rule in ((1, 1, 0), (M32, M32, 1000), (M32, M32, 500), (1, 0, 250), (M32, 1, 999)):
        check(cols, "ACGT", rule)
    w = check(cols, "ACGT", (1, 1, 0))
    assert len(w) == 4 and int(w["counts"][2].astype(np.uint64).sum()) == 7 * M32


def test_slot_target_len_is_never_a_site():
    counts = counts_of([(2, 0, 1, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0, 0)])
    counts[6, 2] = 50                                                   # insertions behind the last base
    counts[0, 2] = 50                                                   # (a device caller's garbage in the slot is not looked at either)
    for rule in ((1, 1, 0), (1, 0, 0)):
        want = sm.sites(counts, sm.ref_codes("AC"), rule)
        assert same(twin(counts, "AC", rule), want) and int(want["pos"].max()) < 2
    # an empty target
    assert len(twin(np.zeros((7, 1), dtype=np.uint32), b"", (1, 0, 0))) == 0


def test_refusals_lower_case_and_modes():
    cols = [(2, 0, 1, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 1, 0, 0, 0)]
    counts = counts_of(cols)
    want = sm.sites(counts, sm.ref_codes("ACGT"), (1, 1, 0))
    assert len(want) == 3
    assert same(twin(counts, "acgt", (1, 1, 0)), want) and same(twin(counts, b"aCgT", (1, 1, 0)), want)
    for rule in ((0, 1, 0), (1, 1, 1001)):
        with pytest.raises(api.ScroogeError) as e:
            twin(counts, "ACGT", rule)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG, rule
    assert count_only(counts, "ACGT", (1, 1, 0), reserved=1)[0] == api.SCRG_ERR_INVALID_ARG
    for genome in ("ACNT", "AC-T", "ACG\0"):
        with pytest.raises(api.ScroogeError) as e:
            twin(counts, genome, (1, 1, 0))
        assert e.value.status == api.SCRG_ERR_BAD_BASE, genome
    # count only / enough room / one record too few: nothing is written
    assert count_only(counts, "ACGT", (1, 1, 0)) == (api.SCRG_OK, 3)
    assert same(twin(counts, "ACGT", (1, 1, 0), cap=3), want) and same(twin(counts, "ACGT", (1, 1, 0), cap=10), want)
    fn = api._lazy(api.load_library(), "scrg_pileup_sites_from_counts")
    rule = api.SiteRule(1, 1, 0, 0)
    for cap in (2, 0):
        out = np.frombuffer(bytearray(b"\x77" * 160), dtype=sm.DTYPE)
        before = out.tobytes()
        n = C.c_uint64(99)
        st = fn(C.c_void_p(counts.ctypes.data), 4, b"ACGT", C.byref(rule), C.c_void_p(out.ctypes.data), cap, C.byref(n))
        assert st == api.SCRG_ERR_CIGAR_OVERFLOW and n.value == 3 and out.tobytes() == before
    n = C.c_uint64(99)
    assert fn(C.c_void_p(counts.ctypes.data), 4, b"ACGT", C.byref(rule), None, 0, None) == api.SCRG_OK       # n_sites may be NULL
    assert fn(None, 4, b"ACGT", C.byref(rule), None, 0, C.byref(n)) == api.SCRG_ERR_INVALID_ARG
    assert fn(C.c_void_p(counts.ctypes.data), 4, None, C.byref(rule), None, 0, C.byref(n)) == api.SCRG_ERR_INVALID_ARG
    assert fn(C.c_void_p(counts.ctypes.data), 4, b"ACGT", None, None, 0, C.byref(n)) == api.SCRG_ERR_INVALID_ARG
    assert fn(C.c_void_p(counts.ctypes.data), 2**32 - 1, b"ACGT", C.byref(rule), None, 0, C.byref(n)) == api.SCRG_ERR_INVALID_ARG


def random_counts(rng, L):
    counts = rng.integers(0, 4, (7, L + 1)).astype(np.uint32)
    counts[:, rng.random(L + 1) < 0.3] = 0                              # uncovered stretches
    agree = rng.random(L + 1) < 0.4                                     # positions where every read agrees
    counts[1:6, agree] = 0
    return counts


def test_random_positions():
    rng = np.random.Generator(np.random.PCG64(2024))
    L = 2000
    genome = bytes(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), L))
    counts = random_counts(rng, L)
    ref = sm.ref_codes(genome)
    sizes = []
    for rule in ((1, 1, 0), (3, 2, 200), (1, 0, 0), (2, 1, 334), (5, 3, 500), (1, 2, 1000)):
        want = sm.sites(counts, ref, rule)
        for s in want[::37]:                                            # the model against its plain-integer statement
            assert sm.one(counts[:, int(s["pos"])], int(s["ref"]), rule) == (True, int(s["alt"]), int(s["call"]), int(s["flags"]))
        assert same(twin(counts, genome, rule), want), rule
        sizes.append(len(want))
    assert 0 < sizes[1] < sizes[0] < sizes[2] < L and (np.diff(sm.sites(counts, ref, (1, 0, 0))["pos"].astype(np.int64)) > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------
def test_job_write_sites(tmp_path):
    """Hand-made counts on the two chromosomes (6000 and 4000 bases, the first hundred of each lower case) of tests/test_io.py's job."""
    from tests.test_io import make_dataset
    fa, fq, seeds, _, _ = make_dataset(str(tmp_path), n_reads=5, seed=34)
    job = sio.Job(fa, fq, seeds)
    L = job.genome_len
    genome = job.genome()
    assert L == 10000 == len(genome) and job.n_chromosomes == 2
    ref = sm.ref_codes(genome)
    counts = np.zeros((7, L + 1), dtype=np.uint32)

    def put(g, match, other, n_other, dele=0, ins=0):
        counts[0, g] = match
        counts[1 + (int(ref[g]) + other) % 4, g] = n_other
        counts[5, g] = dele
        counts[6, g] = ins

    put(5, 4, 1, 2)                      # lower-case reference, a minority base
    put(5999, 1, 2, 3)                   # the last base of chr1: the call moves
    put(6000, 2, 0, 0, dele=5)           # the first of chr2: a deletion majority
    put(7000, 6, 0, 0, ins=2)            # insertions only
    put(9999, 3, 3, 1)                   # the last base of the genome
    counts[6, L] = 4
    found = api.pileup_sites_from_counts(counts, genome, 1, 1, 0)
    assert [int(p) for p in found["pos"]] == [5, 5999, 6000, 7000, 9999]
    path = str(tmp_path / "s.tsv")
    job.write_sites({"sites": found, "target_len": L}, path)
    lines = [x.split("\t") for x in open(path).read().splitlines()]
    assert lines[0] == ["chrom", "pos", "ref", "depth", "match", "A", "C", "G", "T", "del", "ins", "alt", "call", "flags"]
    # the first eleven columns are write_pileup's rows of the same positions
    pile = str(tmp_path / "p.tsv")
    job.write_pileup({"counts": counts, "target_len": L}, pile, 1)
    assert [x[:11] for x in lines] == [x.split("\t") for x in open(pile).read().splitlines()]
    letter = lambda a: "ACGT"[a] if a < 4 else "*" if a == 4 else "."
    up = lambda g: chr(genome[g]).upper()
    assert [x[0] for x in lines[1:]] == ["chr1", "chr1", "chr2", "chr2", "chr2"] and [x[1] for x in lines[1:]] == ["6", "6000", "1", "1001", "4000"]
    assert [x[2] for x in lines[1:]] == [up(g) for g in (5, 5999, 6000, 7000, 9999)]
    assert [x[11:] for x in lines[1:]] == [[letter(int(s["alt"])), letter(int(s["call"])), str(int(s["flags"]))] for s in found]
    assert lines[1][11:] == [letter((int(ref[5]) + 1) % 4), up(5), "1"] and lines[2][11:] == [letter((int(ref[5999]) + 2) % 4)] * 2 + ["5"]
    assert lines[3][11:] == ["*", "*", "5"] and lines[4][11:] == [".", up(7000), "2"]
    # no site: a header alone
    job.write_sites({"sites": found[:0], "target_len": L}, path)
    assert open(path).read().count("\n") == 1
    # sites of another genome's length, a position outside it, a NULL array
    for bad in ({"sites": found, "target_len": L - 1}, {"sites": np.array([(L, (0,) * 7, 0, 0, 0, 0)], dtype=sm.DTYPE), "target_len": L}):
        with pytest.raises(api.ScroogeError) as e:
            job.write_sites(bad, str(tmp_path / "bad.tsv"))
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    rec = api.PileupSites(L, 0, 0, 2, api.SiteRule(1, 1, 0, 0), None)
    assert job.lib.scrg_job_write_sites(job.h, C.byref(rec), str(tmp_path / "null.tsv").encode()) == api.SCRG_ERR_INVALID_ARG


def test_cli_arguments(capsys):
    """Every refusal with its own message: an option the parser does not know would end with the same exit code."""
    from scrooge_amd import cli
    base = ["--reference=g.fa", "--reads=r.fq", "--seeds=s.paf"]
    rule_of, three, whole = "--sites_rule sets the rule of --sites", "--sites_rule takes three integers", "do not go with --distance_only or --clip"
    for extra, why in ((["--sites_rule=1,1,0"], rule_of), (["--pileup=p.tsv", "--sites_rule=1,1,0"], rule_of),
                       (["--sites=s.tsv", "--distance_only"], whole), (["--sites=s.tsv", "--clip"], whole),
                       (["--sites=s.tsv", "--sites_rule=1,1"], three), (["--sites=s.tsv", "--sites_rule=0,1,0"], three),
                       (["--sites=s.tsv", "--sites_rule=1,1,1001"], three), (["--sites=s.tsv", "--sites_rule=1,x,0"], three),
                       (["--sites=s.tsv", "--sites_rule=1,-1,0"], three), (["--sites=s.tsv", "--sites_rule=%d,1,0" % 2**32], three),
                       (["--sites=s.tsv", "--sites_rule=1,%d,0" % 2**32], three)):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and why in err and "unrecognized" not in err, (extra, err)
    # a rule at the limits passes the argument checks: the run then ends at the files, which are not there
    with pytest.raises(api.ScroogeError):
        cli.main(base + ["--sites=s.tsv", "--sites_rule=%d,%d,1000" % (2**32 - 1, 2**32 - 1)])
    assert "usage:" not in capsys.readouterr().err
