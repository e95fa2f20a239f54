"""Seeding on the host (CPU): scrg_seed_rule_check at every range edge, the host twin (scrg_candidates_from_genome) against the plain
Python model on the shapes the GPU tests use, and the model's recall on the two synthetic batches."""
import os
import re

import pytest

import scrooge_amd
from scrooge_amd import api
from scrooge_amd import io as sio
from tests import seed_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


def test_entry_points_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    for name in ("scrg_seed_rule_default", "scrg_seed_rule_check", "scrg_genome_index", "scrg_genome_index_clear", "scrg_genome_index_info",
                 "scrg_find_candidates", "scrg_candidates_free"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    for name in ("scrg_candidates_from_genome", "scrg_job_load_unseeded", "scrg_job_seed"):
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS, name
    assert "#define SCRG_ABI_VERSION 8" in hdr          # new entry points only


def test_defaults(lib):
    import ctypes as C
    k = api._SeedRuleC()
    assert C.sizeof(k) == 32
    api._lazy(lib, "scrg_seed_rule_default")(C.byref(k))
    assert tuple(getattr(k, f) for f, _ in api._SeedRuleC._fields_) == (13, 4, 64, 32, 2, 4, 3, 0)
    assert api.SeedRule() == api.SeedRule(13, 4, 64, 32, 2, 4, 3, 0)
    assert api.seed_rule_check(None, 0) == api.SCRG_ERR_INVALID_ARG          # (the check wants a rule)
    assert api.seed_rule_check(api.SeedRule(), 0) == api.SCRG_OK


def test_rule_check_at_every_range_edge(lib):
    base = dict(k=13, stride=4, max_occ=64, band=32, min_hits=2, max_candidates=4, strands=3, hit_budget_mb=0)
    edges = {"k": ((8, 16), (7, 17, 0)), "stride": ((1, 64), (0, 65)), "max_occ": ((1, 65535), (0, 65536)), "band": ((0, 65535), (65536,)),
             "min_hits": ((1, 2**32 - 1), (0,)), "max_candidates": ((1, 64), (0, 65)), "strands": ((1, 3), (0, 2, 4)),
             "hit_budget_mb": ((0, 1, 2**32 - 1), ())}
    for field, (good, bad) in edges.items():
        for v in good:
            assert api.seed_rule_check(api.SeedRule(**dict(base, **{field: v})), 1000) == api.SCRG_OK, (field, v)
        for v in bad:
            assert api.seed_rule_check(api.SeedRule(**dict(base, **{field: v})), 1000) == api.SCRG_ERR_INVALID_ARG, (field, v)
    assert api.seed_rule_check(api.SeedRule(), 2**32 - 1) == api.SCRG_OK
    assert api.seed_rule_check(api.SeedRule(), 2**32) == api.SCRG_ERR_INVALID_ARG
    # at most 2^31 - 1 index entries, (genome_len - k) / stride + 1: at stride 1 the genome's limit is 2^31 + k - 2 bases
    for k in (8, 13, 16):
        assert api.seed_rule_check(api.SeedRule(k=k, stride=1), 2**31 + k - 2) == api.SCRG_OK
        assert api.seed_rule_check(api.SeedRule(k=k, stride=1), 2**31 + k - 1) == api.SCRG_ERR_INVALID_ARG
        assert api.seed_rule_check(api.SeedRule(k=k, stride=2), 2**32 - 1) == api.SCRG_OK          # the longest genome: below 2^31 entries at stride 2
    with pytest.raises(api.ScroogeError) as e:
        api.candidates_from_genome(api.SeedRule(k=7), b"ACGT" * 10, [b"ACGTACGTACGT"])
    assert e.value.status == api.SCRG_ERR_INVALID_ARG


def test_twin_refuses_bad_bases_and_takes_nothing(lib):
    for genome, reads in ((b"ACGTNACGTACGTACGT", [b"ACGTACGTACGTAC"]), (b"ACGTACGTACGTACGT", [b"ACGTACGTACGTAC", b"ACGTACGTNCGTAC"])):
        with pytest.raises(api.ScroogeError) as e:
            api.candidates_from_genome(None, genome, reads)
        assert e.value.status == api.SCRG_ERR_BAD_BASE
    c, r, v, info = api.candidates_from_genome(None, b"ACGTTGCATGCATGCAAGCT", [], info=True)
    assert (c, r, v) == ([], [], []) and info["n_hits"] == 0 and info["rule"] == api.SeedRule(hit_budget_mb=256)
    assert api.candidates_from_genome(None, b"", [b"ACGTACGTACGTACGT"]) == ([[]], [[]], [[]])
    lower = api.candidates_from_genome((13, 1, 64, 32, 2, 4, 3), b"acgttgcatgcatgcaagct", [b"CGTTGCATGCATGCA", b"tgcatgcatgcaacg"])
    assert lower == ([[1], [1]], [[0], [1]], [[3], [3]])


def _check_case(case):
    name, rule, genome, reads = case
    want = sm.candidates(rule, genome, reads)
    got = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True)
    assert got[0] == want[0], name
    assert got[1] == want[1], name
    assert got[2] == want[2], name
    assert {k: got[3][k] for k in want[3]} == want[3], name


@pytest.mark.parametrize("group", ["genome_length_cases", "read_length_cases", "occupancy_cases", "cluster_cases", "big_read_cases"])
def test_twin_is_the_model_on_the_gpu_shapes(lib, group):
    cases = getattr(sm, group)()
    assert len(cases) >= 3
    for case in cases:
        _check_case(case)


def test_twin_is_the_model_on_the_chunk_batch(lib):
    _check_case(sm.chunk_case())


def test_the_shapes_are_what_they_claim():
    """The cases hold what their names say: the occupancy case's two keys, the band case's gaps, the heavy read's hits."""
    by_name = {c[0]: c for c in sm.all_shape_cases()}
    _, rule, genome, reads = by_name["occ_exact"]
    c, r, v, info = sm.candidates(rule, genome, reads[:2])
    assert len(c[0]) == 3 and c[1] == [] and info["n_keys_over_max_occ"] == 1         # m1: max_occ entries; m2: one more
    _, rule, genome, reads = by_name["band"]
    c, r, v, info = sm.candidates(rule, genome, reads[:3])
    # (28 k-mers either side of the deleted bases; a k-mer across the deletion hits too where the base behind it repeats the one deleted)
    assert len(c[0]) == 1 and 56 <= v[0][0] <= 58 and len(c[1]) == 2 and all(28 <= x <= 29 for x in v[1]) and v[2] == [68]
    c0, _, v0, _ = sm.candidates(by_name["band0"][1], genome, reads[:3])
    assert len(c0[0]) == 2 and len(c0[1]) == 2 and v0[2] == [68]
    _, rule, genome, reads = by_name["ties"]
    c, r, v, info = sm.candidates(rule, genome, reads[:1])
    assert v[0] == [48] * 4 and c[0] == sorted(c[0]) and info["n_clusters"] == 6
    assert sm.candidates(by_name["ties_none"][1], genome, reads[:1])[0] == [[]]
    assert len(sm.candidates(by_name["ties_all"][1], genome, reads[:1])[0][0]) == 6
    _, rule, genome, reads = by_name["heavy_read"]
    assert sm.candidates(rule, genome, reads[1:2])[3]["n_hits"] * 48 > 2 * 2**20
    _, rule, genome, reads = by_name["bucket_per_key"]
    assert (len(genome) - rule[0]) // rule[1] + 1 > 2 ** 15 and 2 * rule[0] == 16          # 16 bucket bits = the whole key
    c, r, v, _ = sm.candidates(rule, genome, reads)
    assert all(c[:6]) and [x[0] for x in r[:6]] == [0, 0, 0, 1, 1, 1]
    _, rule, genome, reads = by_name["reads_s1"]
    own = reads[18]
    assert own == sm.revcomp(own)
    c, r, v, _ = sm.candidates(rule, genome, [own] + reads[19:23])
    assert r[0][:2] == [0, 1] and c[0][0] == c[0][1] and v[0][0] == v[0][1]            # the same cluster on both strands: the order falls to strand
    assert c[1][0] == 0 and c[2][0] == 0                                                # overhanging the start: negative diagonals, start clamps to 0


@pytest.mark.parametrize("kind", ["illumina", "ont"])
def test_recall_of_the_model_and_the_twin(lib, kind):
    """The true start is among a read's candidates, on the true strand, within 4 bases (150 bp reads) or 40 (2 kb reads) for at least
    95 % of the reads.  Measured: 200 / 200 (worst error 1) and 100 / 100 (worst error 6): random genomes and i.i.d. errors, which
    says nothing about a real sample."""
    rule, genome, reads, truth = sm.recall_batch(kind)
    cands, rev, votes, info = sm.candidates(rule, genome, reads)
    found, worst = sm.recall(cands, rev, truth)
    print("recall %s: %d of %d, worst start error %d, %d hits, %d clusters" % (kind, found, len(reads), worst, info["n_hits"], info["n_clusters"]))
    assert found * 100 >= 95 * len(reads)
    got = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True)
    assert got[:3] == (cands, rev, votes) and {k: got[3][k] for k in info} == info
