"""Seed sampling on the GPU: scrg_ctx_set_seed_sampling + scrg_genome_index + scrg_find_candidates against the sampled host twin,
array for array — offsets, starts, strands, votes, n_hits, n_clusters, n_keys_over_max_occ, n_lookups and n_entries — on the shapes
of tests/seed_model.py, at the sizes where the index's compaction can go wrong, on an index of zero entries over a non-empty genome,
through the setting's lifetime and through the command line.

The tests use an Aligner of their own: the shared one is session-scoped, and a sampling setting left on it would change what other
tests index."""
import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, cli, synth
from tests import seed_model as sm
from tests import seed_sample_model as ssm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sampler():
    scrooge_amd.build_library()
    a = scrooge_amd.Aligner(0)
    yield a
    a.close()


def n_positions_of(rule, genome):
    k, stride = rule[0], rule[1]
    return 0 if len(genome) < k else (len(genome) - k) // stride + 1


def device_candidates(a, rule, s, genome, reads, budget_mb=0):
    a.set_genome(genome)
    a.set_seed_sampling(s)
    info = a.index_genome(api.SeedRule(*rule, budget_mb))
    assert info["rule"] == api.SeedRule(*rule, budget_mb or 256) and info["smer"] == s and info["n_positions"] == n_positions_of(rule, genome)
    assert info["n_entries"] <= info["n_positions"] and info["device_bytes"] > 0
    assert a.seed_sampling_info()["n_lookups"] == 0          # (of this index: no call yet)
    got = a.find_candidates(reads, info=True)
    got[3]["n_entries"] = info["n_entries"]
    assert a.seed_sampling_info() == {"smer": s, "n_positions": info["n_positions"], "n_lookups": got[3]["n_lookups"]}
    return got


COUNTERS = ("n_hits", "n_clusters", "n_keys_over_max_occ", "n_lookups", "n_entries")


def check_case(a, case, s, budgets=(0,)):
    name, rule, genome, reads = case
    want = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=s)
    for mb in budgets:
        got = device_candidates(a, rule, s, genome, reads, mb)
        for what, g, w in zip(("starts", "strands", "votes"), got, want):
            assert g == w, (name, s, mb, what)
        for counter in COUNTERS:
            assert got[3][counter] == want[3][counter], (name, s, mb, counter)
    return want


@pytest.mark.parametrize("k", [8, 13, 16])
def test_genome_lengths_and_strides(sampler, k):
    """Genomes of k - 1, k, k + 1 and the word seams of the packing plus k, strides 1, 3, 4 and 64, reads equal to the genome on both
    strands: s = k - 4 at 1 MB and at the default budget, s = 3 and s = k - 1 at the default; s = k - 1 is also the unsampled
    device result."""
    cases = [c for c in sm.genome_length_cases() if c[1][0] == k]
    assert len(cases) == 48
    some = left_out = 0
    for case in cases:
        want = check_case(sampler, case, k - 4, budgets=(1, 0))
        some += sum(len(c) for c in want[0])
        left_out += n_positions_of(case[1], case[2]) - want[3]["n_entries"]
        check_case(sampler, case, 3)
        all_keys = check_case(sampler, case, k - 1)
        plain = device_candidates(sampler, case[1], 0, case[2], case[3])
        assert plain == all_keys, case[0]
    assert some > 100 and left_out > 100


@pytest.mark.parametrize("group", ["read_length_cases", "occupancy_cases", "cluster_cases", "big_read_cases"])
def test_shapes(sampler, group):
    """The read-length, occupancy (the all-A genome: every k-mer ties and is selected), cluster and big-read groups at s = k - 4."""
    for case in getattr(sm, group)():
        want = check_case(sampler, case, case[1][0] - 4)
        if case[0].startswith("all_a"):
            assert want[3]["n_entries"] == n_positions_of(case[1], case[2])


def test_chunks_do_not_show(sampler):
    """The chunk batch at s = 9, more hits than 1 MB holds (48 bytes a hit): the same arrays at 1 MB, 2 MB and the default."""
    want = check_case(sampler, sm.chunk_case(), 9, budgets=(1, 2, 0))
    assert want[3]["n_hits"] * 48 > 2**20


def test_compaction_edges(sampler):
    """Considered positions of 63, 64, 65 (a wavefront), 255, 256, 257 (a workgroup), 513 and the 60 kb recall genome (several
    hundred workgroups), stride 1.  Each genome is read by itself and by its reverse complement: the diagonal-0 cluster's votes
    count every entry of the index."""
    rng = np.random.Generator(np.random.PCG64(41))
    k = 13
    genomes = [synth.random_seq(n + k - 1, rng) for n in (63, 64, 65, 255, 256, 257, 513)] + [sm.recall_batch("illumina")[1]]
    for genome in genomes:
        for s in (9, 5):
            rule = (k, 1, 64, 0, 1, 4, 3)
            want = check_case(sampler, ("edge%d" % len(genome), rule, genome, [genome, sm.revcomp(genome)]), s)
            n = want[3]["n_entries"]
            assert 0 < n < len(genome) - k + 1
            if len(genome) < 1000:          # (no repeated k-mer: every entry is one hit on diagonal 0)
                assert want[0][0][0] == 0 and want[1][0][0] == 0 and want[2][0][0] == n, (len(genome), s)
                assert want[0][1][0] == 0 and want[1][1][0] == 1 and want[2][1][0] == n, (len(genome), s)


def test_an_index_of_no_entries(sampler):
    """A genome of one unselected k-mer, and a longer one whose positions at stride 64 all hold unselected k-mers: no entries, no
    candidates, and the next index on the handle is good."""
    k, s = 13, 9
    one = ssm.unselected_kmer(k, s)
    strided = ssm.unselected_genome(k, s, 64, 5)
    case = sm.read_length_cases()[0]
    for rule, genome in (((k, 1, 64, 32, 1, 4, 3), one), ((k, 64, 64, 32, 1, 4, 3), strided)):
        reads = [genome, sm.revcomp(genome), genome[:k], b"", synth.random_seq(150, np.random.Generator(np.random.PCG64(2)))]
        got = device_candidates(sampler, rule, s, genome, reads)
        assert got[3]["n_entries"] == 0 and n_positions_of(rule, genome) in (1, 5)
        assert got[0] == [[]] * len(reads) and got[3]["n_hits"] == 0 and got[3]["n_clusters"] == 0 and got[3]["n_keys_over_max_occ"] == 0
        want = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=s)
        assert got[:3] == want[:3] and all(got[3][c] == want[3][c] for c in COUNTERS)
        check_case(sampler, case, s)


def test_the_settings_lifetime(sampler):
    rule, genome, reads, truth = sm.recall_batch("illumina")
    reads = reads[:40]
    sampler.clear_genome()
    with pytest.raises(api.ScroogeError) as e:
        sampler.seed_sampling_info()
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    for bad in (1, 2, 16, 17, 2**32 - 1):
        with pytest.raises(api.ScroogeError) as e:
            sampler.set_seed_sampling(bad)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    sampled = device_candidates(sampler, rule, 7, genome, reads)
    assert sampled == api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=7)
    # set after the build: the index and the results stay
    sampler.set_seed_sampling(0)
    assert sampler.index_info()["smer"] == 7 and sampler.index_info()["n_entries"] == sampled[3]["n_entries"]
    again = sampler.find_candidates(reads, info=True)
    assert again[:3] == sampled[:3] and again[3]["n_lookups"] == sampled[3]["n_lookups"]
    # smer >= k refuses and leaves no index
    sampler.set_seed_sampling(13)
    with pytest.raises(api.ScroogeError) as e:
        sampler.index_genome(api.SeedRule(*rule))
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(api.ScroogeError):
        sampler.index_info()
    with pytest.raises(api.ScroogeError) as e:
        sampler.seed_sampling_info()
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    sampler.index_genome(api.SeedRule(k=14, stride=1))          # (13 is good below k = 14)
    assert sampler.index_info()["smer"] == 13
    # back at 0: today's results
    sampler.set_seed_sampling(0)
    info = sampler.index_genome(api.SeedRule(*rule))
    assert info["smer"] == 0 and info["n_entries"] == info["n_positions"] == n_positions_of(rule, genome)
    plain = sampler.find_candidates(reads, info=True)
    want = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True)
    assert plain[:3] == want[:3] and all(plain[3][c] == want[3][c] for c in COUNTERS[:4])
    assert plain[3]["n_lookups"] == 2 * sum(len(r) - 13 + 1 for r in reads)


def test_cli_with_seed_sample(sampler, tmp_path):
    """A FASTA and a FASTQ through the command line without --seeds, at stride 1 and --seed_sample=5: the PAF is the one the twin's
    candidates give through the same mapping call."""
    rule, genome, reads, truth = sm.recall_batch("illumina")
    rule = (13, 1, 64, 8, 2, 4, 3)
    fa, fq, out = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "o.paf")
    with open(fa, "w") as f:
        f.write(">chr1\n" + "\n".join(genome[i:i + 80].decode() for i in range(0, len(genome), 80)) + "\n")
    with open(fq, "w") as f:
        for i, r in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
    with pytest.raises(SystemExit):
        cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + fa + ".paf", "--seed_sample=5"])
    with pytest.raises(SystemExit):
        cli.main(["--reference=" + fa, "--reads=" + fq, "--seed_rule=13,1,64,8,2,4", "--seed_sample=13"])
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--out=" + out, "--seed_rule=13,1,64,8,2,4", "--seed_sample=5"]) == 0
    cands, rev, votes, info = api.candidates_from_genome(api.SeedRule(*rule), genome, reads, info=True, smer=5)
    assert all(cands) and (info["n_entries"], info["n_lookups"], info["n_hits"]) == (13522, 12326, 5406)
    sampler.set_genome(genome)
    res = sampler.align_mapping_directed(reads, cands, reverse=rev)
    assert all(st == api.SCRG_OK for st in sampler.last_status)
    want, p = [], 0
    for i, c in enumerate(cands):
        for j in range(len(c)):
            want.append(("r%d" % i, "-" if rev[i][j] else "+", c[j], res[p].edit_distance, res[p].cigar))
            p += 1
    got = []
    for line in open(out):
        f = line.rstrip("\n").split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        got.append((f[0], f[4], int(f[7]), int(tags["NM:i:"]), tags["cg:Z:"]))
    assert sorted(got) == sorted(want) and len(want) >= len(reads)
