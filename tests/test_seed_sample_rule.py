"""Seed sampling on the host (CPU): the closed-syncmer predicate (scrg_seed_key_selected) and the sampled twin
(scrg_candidates_from_genome_sampled) against the plain Python statement of the rule (tests/seed_sample_model.py), the two facts
that follow from the definition, and the recall batches at stride 1."""
import os
import re

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from scrooge_amd import io as sio
from tests import seed_model as sm
from tests import seed_sample_model as ssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


@pytest.fixture(scope="module")
def stretch():
    """20 000 random bases, with a run of A and a run of T planted"""
    s = bytearray(synth.random_seq(20000, np.random.Generator(np.random.PCG64(31))))
    s[5000:5040] = b"A" * 40
    s[9000:9040] = b"T" * 40
    return bytes(s)


def test_entry_points_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    for name in ("scrg_ctx_set_seed_sampling", "scrg_seed_sampling_info", "scrg_seed_key_selected"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    name = "scrg_candidates_from_genome_sampled"
    assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS
    assert "#define SCRG_ABI_VERSION 8" in hdr          # new entry points only
    import ctypes as C
    assert C.sizeof(api._SeedRuleC) == 32


@pytest.mark.parametrize("k", [8, 13, 16])
def test_predicate_is_the_model(lib, stretch, k):
    keys = ssm.keys_of(stretch, k)
    top = 4 ** k - 1
    keys += [0, top, top - 1, top ^ 0x5, 1 << (2 * k - 1), 3 << (2 * k - 2), (3 << (2 * k - 2)) | 1]          # all A, all T, the top bits set
    assert any(key >> (2 * k - 2) == 3 for key in keys[:-7])
    for s in (3, k - 4, k - 1):
        want = [ssm.selected(key, k, s) for key in keys]
        got = [api.seed_key_selected(key, k, s) for key in keys]
        assert got == want, (k, s)
        assert want[len(keys) - 7] and want[len(keys) - 6]                       # all A and all T: every s-mer ties
        if s < k - 1:
            assert 0 < sum(want) < len(want)
    assert all(api.seed_key_selected(key, k, 0) for key in keys[:100])
    for bad in (1, 2, k, 16):
        assert not api.seed_key_selected(0, k, bad)
    assert not api.seed_key_selected(0, 7, 3) and not api.seed_key_selected(0, 17, 3)


def test_what_follows_from_the_definition(lib, stretch):
    """s = k - 1 selects every key; at stride 1 the longest unselected run is at most k - s - 1; the density on random sequence is
    2 / (k - s + 1) within 5 %."""
    k = 13
    keys = ssm.keys_of(stretch, k)
    sel = {s: [api.seed_key_selected(key, k, s) for key in keys] for s in (12, 11, 9, 7, 5)}
    assert all(sel[12])
    for s in (11, 9, 7, 5):
        run = worst = 0
        for x in sel[s]:
            run = 0 if x else run + 1
            worst = max(worst, run)
        assert worst <= k - s - 1 and worst == ssm.longest_unselected_run(keys, k, s), s
    for s in (9, 7, 5):
        density, expect = sum(sel[s]) / len(keys), 2 / (k - s + 1)
        print("density k 13 s %d: %.4f, expected %.4f" % (s, density, expect))
        assert abs(density - expect) <= 0.05 * expect, s


def _check_case(case, s):
    name, rule, genome, reads = case
    want = ssm.candidates(rule, s, genome, reads)
    got = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=s)
    for what, g, w in zip(("starts", "strands", "votes"), got, want):
        assert g == w, (name, s, what)
    assert {k: got[3][k] for k in want[3]} == want[3], (name, s)
    return got


@pytest.mark.parametrize("group", ["genome_length_cases", "read_length_cases", "occupancy_cases", "cluster_cases", "big_read_cases", "chunk_case"])
def test_sampled_twin_is_the_model(lib, group):
    cases = getattr(sm, group)()
    cases = [cases] if group == "chunk_case" else cases
    some = 0
    for case in cases:
        some += sum(len(c) for c in _check_case(case, case[1][0] - 4)[0])
    assert some > 0


def test_smer_k_minus_1_and_0_are_the_unsampled_twin(lib):
    for case in sm.read_length_cases() + sm.occupancy_cases() + sm.genome_length_cases()[::7]:
        name, rule, genome, reads = case
        plain = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True)
        k, stride = rule[0], rule[1]
        n_positions = 0 if len(genome) < k else (len(genome) - k) // stride + 1
        n_lanes = (2 if rule[6] == 3 else 1) * sum(max(0, len(r) - k + 1) for r in reads)
        assert plain[3]["n_entries"] == n_positions and plain[3]["n_lookups"] == n_lanes, name
        assert plain[:3] == sm.candidates(rule, genome, reads)[:3], name
        assert api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=0) == plain, name
        assert api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=k - 1) == plain, name


# (entries, lookups, hits) of the plain Python model, on the rule of the batch with stride 1
RECALL_COUNTS = {("illumina", 7): (17126, 15903, 6890), ("illumina", 5): (13522, 12326, 5406),
                 ("ont", 7): (17099, 113834, 15874), ("ont", 5): (13442, 89247, 12548)}


@pytest.mark.parametrize("kind", ["illumina", "ont"])
@pytest.mark.parametrize("s", [7, 5])
def test_recall_at_stride_1(lib, kind, s):
    """Every read of the two synthetic batches keeps a candidate at its true start (what the default rule reaches on them) with an
    index no larger than the default rule's at s = 5 and a quarter of its lookups: random genomes and i.i.d. errors, which says
    nothing about a real sample."""
    rule, genome, reads, truth = sm.recall_batch(kind)
    rule = (rule[0], 1) + rule[2:]
    cands, rev, votes, info = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=s)
    found, worst = sm.recall(cands, rev, truth)
    print("recall %s s %d: %d of %d, worst start error %d, %d entries, %d lookups, %d hits"
          % (kind, s, found, len(reads), worst, info["n_entries"], info["n_lookups"], info["n_hits"]))
    assert found == len(reads)
    assert (info["n_entries"], info["n_lookups"], info["n_hits"]) == RECALL_COUNTS[kind, s]
    want = ssm.candidates(rule, s, genome, reads)
    assert (cands, rev, votes) == want[:3] and {k: info[k] for k in want[3]} == want[3]


def test_refusals(lib):
    genome, reads = b"ACGTTGCATGCATGCAAGCTTTGACCA", [b"CGTTGCATGCATGCAAG"]
    for k in (8, 13, 16):
        for bad in (1, 2, k, 16, 2**32 - 1):
            with pytest.raises(api.ScroogeError) as e:
                api.candidates_from_genome(api.SeedRule(k=k, stride=1), genome, reads, smer=bad)
            assert e.value.status == api.SCRG_ERR_INVALID_ARG, (k, bad)
        api.candidates_from_genome(api.SeedRule(k=k, stride=1), genome, reads, smer=k - 1)
    for g, r in ((b"ACGTNACGTACGTACGT", [b"ACGTACGTACGTAC"]), (b"ACGTACGTACGTACGT", [b"ACGTACGTACGTAC", b"ACGTACGTNCGTAC"])):
        with pytest.raises(api.ScroogeError) as e:
            api.candidates_from_genome(None, g, r, smer=5)
        assert e.value.status == api.SCRG_ERR_BAD_BASE


def test_the_unselected_inputs_are_what_they_claim():
    for k, s in ((13, 9), (13, 5), (8, 4), (16, 12)):
        kmer = ssm.unselected_kmer(k, s)
        assert len(kmer) == k and not ssm.selected(sm.key_of(kmer), k, s)
        genome = ssm.unselected_genome(k, s, 64, 5)
        assert len(genome) == 4 * 64 + k and ssm.build_index(genome, k, 64, s) == ({}, 5)
        assert ssm.build_index(genome, k, 1, s)[0]                                   # (at stride 1 it has entries)
