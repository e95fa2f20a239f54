"""Seeding on the GPU: scrg_genome_index + scrg_find_candidates against the host twin, array for array — offsets, starts, strands,
votes and the three counters — on the smallest shapes at which the index, the lookup, the clusters or the pick can go wrong
(tests/seed_model.py), at a hit budget of 1 MB and at the default; the two recall batches end to end through best-candidate mode;
the index's lifetime; and the command line without --seeds."""
import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, cli
from scrooge_amd import io as sio
from tests import seed_model as sm

pytestmark = pytest.mark.gpu


def device_candidates(aligner, rule, genome, reads, budget_mb):
    aligner.set_genome(genome)
    info = aligner.index_genome(api.SeedRule(*rule, budget_mb))
    assert info["rule"] == api.SeedRule(*rule, budget_mb or 256)
    k, stride = rule[0], rule[1]
    assert info["n_entries"] == (0 if len(genome) < k else (len(genome) - k) // stride + 1) and info["device_bytes"] > 0
    return aligner.find_candidates(reads, info=True)


def check_case(aligner, case, budgets=(1, 0)):
    name, rule, genome, reads = case
    want = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True)
    for mb in budgets:
        got = device_candidates(aligner, rule, genome, reads, mb)
        for what, g, w in zip(("starts", "strands", "votes"), got, want):
            assert g == w, (name, mb, what)
        for counter in ("n_hits", "n_clusters", "n_keys_over_max_occ"):
            assert got[3][counter] == want[3][counter], (name, mb, counter)
    return want


@pytest.mark.parametrize("k", [8, 13, 16])
def test_genome_lengths_and_strides(aligner, k):
    """Genomes of k - 1 (an empty index), k, k + 1 and the word seams of the planar packing plus k; strides 1, 3, 4 and 64; k = 16
    fills the 32-bit key (runs of T); each at a hit budget of 1 MB and at the default."""
    cases = [c for c in sm.genome_length_cases() if c[1][0] == k]
    assert len(cases) == 48
    some = 0
    for case in cases:
        some += sum(len(c) for c in check_case(aligner, case)[0])
    assert some > 100


@pytest.mark.parametrize("group", ["read_length_cases", "occupancy_cases", "cluster_cases", "big_read_cases"])
def test_shapes_at_both_budgets(aligner, group):
    """Read lengths 0 .. 2000, a read that is its own reverse complement, reads overhanging either end of the genome; keys with
    max_occ and max_occ + 1 entries, an all-A genome; gaps of band and band + 1, band 0, ties in votes, min_hits one above a
    cluster's votes; reads whose hits fill several workgroups and exceed the budget alone; a batch in which most reads hit nothing;
    an index with a bucket per key (the lookup then reads no key at all)."""
    for case in getattr(sm, group)():
        check_case(aligner, case)


def test_chunks_do_not_show(aligner):
    """A batch of several chunks at 1 MB, the heavy read in a chunk of its own: the same arrays at 1 MB, 2 MB and the default."""
    want = check_case(aligner, sm.chunk_case(), budgets=(1, 2, 0))
    assert want[3]["n_hits"] * 48 > 4 * 2**20


def test_empty_batch_bad_base_and_a_refused_rule(aligner):
    genome, rule = b"ACGTTGCATGCATGCAAGCTTTGACCA", (13, 1, 64, 32, 1, 4, 3)
    aligner.set_genome(genome)
    aligner.index_genome(rule)
    c, r, v, info = aligner.find_candidates([], info=True)
    assert (c, r, v) == ([], [], []) and info["n_hits"] == 0 and info["n_clusters"] == 0
    with pytest.raises(api.ScroogeError) as e:
        aligner.find_candidates([b"ACGTTGCATGCATGCA", b"ACGTTGCATGNATGCA"])
    assert e.value.status == api.SCRG_ERR_BAD_BASE
    lower = aligner.find_candidates([b"cgttgcatgcatgcaag"])
    assert lower == api.candidates_from_genome(rule, genome, [b"CGTTGCATGCATGCAAG"]) and lower[0][0][0] == 1 and lower[2][0][0] == 5
    with pytest.raises(api.ScroogeError) as e:
        aligner.index_genome(api.SeedRule(k=17))
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(api.ScroogeError):          # (a refused rule leaves no index behind)
        aligner.index_info()


def test_index_lifetime(aligner):
    """find_candidates before any index, after clear_genome, after set_genome with another genome and after clear_index is
    SCRG_ERR_INVALID_ARG; a pairwise call in between (which may move the genome) leaves the index good."""
    rng = np.random.Generator(np.random.PCG64(5))
    genome, other = scrooge_amd.synth.random_seq(3000, rng), scrooge_amd.synth.random_seq(2000, rng)
    reads = [genome[100:250], sm.revcomp(genome[900:1100])]

    def refused():
        with pytest.raises(api.ScroogeError) as e:
            aligner.find_candidates(reads)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG and "index" in str(e.value)

    aligner.clear_genome()
    with pytest.raises(api.ScroogeError) as e:
        aligner.index_genome()
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    refused()
    aligner.set_genome(genome)
    refused()                                      # a genome, no index yet
    aligner.index_genome()
    want = api.candidates_from_genome(None, genome, reads)
    assert aligner.find_candidates(reads) == want and want[0][0][0] == 100 and want[1][1][0] == 1
    texts, queries = scrooge_amd.synth.make_pairs(300, 3000, "ont", seed=9)          # grows the sequence array: the genome moves
    aligner.align_pairs(texts, queries)
    assert aligner.find_candidates(reads) == want
    aligner.set_genome(other)
    refused()
    aligner.set_genome(genome)
    aligner.index_genome()
    aligner.clear_genome()
    refused()
    aligner.set_genome(genome)
    aligner.index_genome()
    aligner.clear_index()
    refused()
    aligner.index_genome()
    aligner.align_mapping(other, [other[10:100]], [[10]])          # a mapping call that stages a genome of its own
    refused()


@pytest.mark.parametrize("kind", ["illumina", "ont"])
def test_end_to_end_through_best_candidate_mode(aligner, kind):
    """index_genome, find_candidates, then the resident mapping call with best=True.  What this test holds is that the candidates are
    the twin's; the mapping call is then run on both (equal) sets, which shows that the arrays go into it as they are and that it
    answers the same twice, nothing more."""
    rule, genome, reads, truth = sm.recall_batch(kind)
    want = api.candidates_from_genome(api.SeedRule(*rule), genome, reads)
    aligner.set_genome(genome)
    aligner.index_genome(api.SeedRule(*rule))
    got = aligner.find_candidates(reads)
    assert got == want
    res = aligner.align_mapping_directed(reads, got[0], reverse=got[1], arrays=True, best=True)
    ref = aligner.align_mapping_directed(reads, want[0], reverse=want[1], arrays=True, best=True)
    assert np.array_equal(res["edit_distance"], ref["edit_distance"]) and np.array_equal(res["status"], ref["status"])
    assert len(res["edit_distance"]) == sum(len(c) for c in got[0]) >= len(reads)


def test_cli_without_seeds(aligner, tmp_path):
    """A FASTA and a FASTQ, no --seeds, --best --format=sam: record for record what find_candidates + the mapping call give."""
    rule, genome, reads, truth = sm.recall_batch("illumina")
    reads = reads[:60] + [scrooge_amd.synth.random_seq(150, np.random.Generator(np.random.PCG64(1)))]          # one read that maps nowhere
    fa, fq, out = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "o.sam")
    with open(fa, "w") as f:
        f.write(">chr1\n" + "\n".join(genome[i:i + 80].decode() for i in range(0, len(genome), 80)) + "\n")
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--best", "--format=sam", "--out=" + out, "--seed_rule=13,4,64,8,2,4"]) == 0
    aligner.set_genome(genome)
    aligner.index_genome(api.SeedRule(*rule))
    cands, rev, votes = aligner.find_candidates(reads)
    assert cands[-1] == [] and all(cands[:60])
    res = aligner.align_mapping_directed(reads, cands, reverse=rev, best=True)
    status = aligner.last_status
    want, p = {}, 0
    for i, c in enumerate(cands):
        if c:                  # (a read without a candidate has no pair, and the writers write pairs: no record, as with a seeds file)
            want["r%d" % i] = None
        for j in range(len(c)):
            if status[p] == api.SCRG_OK:
                want["r%d" % i] = (16 if rev[i][j] else 0, c[j] + 1, res[p].cigar, res[p].edit_distance)
            p += 1
    got = {}
    for line in open(out):
        if line.startswith("@"):
            continue
        f = line.rstrip("\n").split("\t")
        got[f[0]] = None if int(f[1]) & 4 else (int(f[1]) & 16, int(f[3]), f[5], int([t for t in f[11:] if t.startswith("NM:i:")][0][5:]))
    assert got == want and len(want) == 60 and "r60" not in got
    # the loader's own way: a job with no pairs, seeded on the GPU, holds those candidates in its (longest first) read order
    job = sio.Job(fa, fq)
    assert job.seed(aligner, api.SeedRule(*rule)) == sum(len(c) for c in cands)
    _, job_reads, job_cands, names = job.views()
    for name, r, c in zip(names, job_reads, job_cands):
        i = int(name[1:])
        assert r == reads[i] and c == [(s, bool(x)) for s, x in zip(cands[i], rev[i])]
        assert all(job.pair_chromosome(k)[0] == "chr1" for k in range(job.n_pairs))
