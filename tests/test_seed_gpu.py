"""Seeding on the GPU: scrg_genome_index + scrg_find_candidates against the host twin, array for array — offsets, starts, strands,
votes and the three counters — on the smallest shapes at which the index, the lookup, the clusters or the pick can go wrong
(tests/seed_model.py), at a hit budget of 1 MB and at the default; the two recall batches end to end through best-candidate mode;
the index's lifetime; the command line without --seeds; and one call of more reads than a chunk holds (2^22 + 5), against the plain
Python model indexed by the batch's period."""
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


CHUNK_READS = 1 << 22                                # the most reads of one chunk (Chunks)
HIT_BYTES = 48                                       # what the budget counts per hit (include/scrooge_amd.h, scrg_find_candidates)


def chunk_limit_case():
    """-> (rule, genome, 61 distinct short reads): a 4 kb random genome at (16, 1, 64, 32, 1, 4, 3); 16-mers of it, forward (20) and
    reverse (15: one hit each), stretches of 17 and of 20 bases on both strands (6 each), a read of 15 bases (no lanes), an empty
    one, 10 random 16-mers (no hit), and one 16-mer planted three times, forward and reverse."""
    rng = np.random.Generator(np.random.PCG64(17))
    synth = scrooge_amd.synth
    planted = synth.random_seq(16, rng)
    genome = bytearray(synth.random_seq(4000, rng))
    for at in (301, 1777, 3984):                     # (the last one ends with the genome)
        genome[at:at + 16] = planted
    genome = bytes(genome)
    at = [int(x) for x in rng.choice(np.arange(400, 1700), 47, replace=False)]
    cut = lambda i, n: genome[at[i]:at[i] + n]
    distinct = [cut(i, 16) for i in range(20)] + [sm.revcomp(cut(i, 16)) for i in range(20, 35)]
    distinct += [cut(i, 17) if i % 2 else sm.revcomp(cut(i, 17)) for i in range(35, 41)]
    distinct += [cut(i, 20) if i % 2 else sm.revcomp(cut(i, 20)) for i in range(41, 47)]
    distinct += [genome[2000:2015], b""] + [synth.random_seq(16, rng) for _ in range(10)] + [planted, sm.revcomp(planted)]
    assert len(distinct) == 61 == len(set(distinct))
    return (16, 1, 64, 32, 1, 4, 3), genome, distinct


def simulated_chunks(hits, lanes, budget_mb):
    """The chunks find_candidates cuts, by the arithmetic its header documents: whole reads, at most 2^22, whose hits fit the budget
    at 48 bytes a hit and whose lanes fit four times as many; a read over either alone is a chunk.  -> the first read of each."""
    budget_hits = max(1, (budget_mb << 20) // HIT_BYTES)
    H, L = np.concatenate([[0], np.cumsum(hits)]), np.concatenate([[0], np.cumsum(lanes)])
    n, r0, first = len(hits), 0, []
    while r0 < n:
        first.append(r0)
        r1 = min(n, r0 + CHUNK_READS, int(np.searchsorted(H, H[r0] + budget_hits, "right")) - 1, int(np.searchsorted(L, L[r0] + 4 * budget_hits, "right")) - 1)
        r0 = max(r1, r0 + 1)
    return first


def find_flat(aligner, buffers, lengths, idx):
    """scrg_find_candidates on the reads buffers[idx[i]], the pointer and length arrays made with numpy -> (cand_offsets,
    cand_start, cand_reverse, cand_votes as numpy arrays, the counters)."""
    import ctypes as C
    addr = np.array([C.addressof(b) for b in buffers], dtype=np.uint64)
    ptrs, lens = np.ascontiguousarray(addr[idx]), np.ascontiguousarray(np.asarray(lengths, dtype=np.uint64)[idx])
    cp = C.POINTER(api.Candidates)()
    aligner._check(api._lazy(aligner.lib, "scrg_find_candidates")(aligner.h, len(idx), ptrs.ctypes.data, lens.ctypes.data, C.byref(cp)))
    try:
        c = cp.contents
        assert int(c.n_reads) == len(idx)
        offs = np.ctypeslib.as_array(c.cand_offsets, shape=(len(idx) + 1,)).copy()
        n = int(offs[-1])
        starts, rev, votes = (np.ctypeslib.as_array(a, shape=(max(n, 1),))[:n].copy() for a in (c.cand_start, c.cand_reverse, c.cand_votes))
        info = {"n_hits": int(c.n_hits), "n_clusters": int(c.n_clusters), "n_keys_over_max_occ": int(c.n_keys_over_max_occ)}
    finally:
        api._lazy(aligner.lib, "scrg_candidates_free")(cp)
    info["n_lookups"] = aligner.seed_sampling_info()["n_lookups"]
    return offs, starts, rev, votes, info


def test_more_reads_than_one_chunk_holds(aligner):
    """2^22 + 5 reads in one call, at a budget under which neither the hits nor the lanes of the first 2^22 reads cut a chunk
    (asserted from the model's counts): the read count does, which no smaller batch can reach.  Read i is one of 61 distinct
    short reads, distinct[7 i mod 61], so the expected arrays are the model's 61 answers indexed, the counters sums by
    multiplicity, and reads 2^22 - 1, 2^22 and 2^22 + 1 — the last of the first chunk, the first two of the second — are three
    different reads with three different answers.  Then the first 2^20 + 1 reads at 1 MB, where the hits cut dozens of chunks,
    and the same reads up to the first of a chunk, so that the last chunk holds one read.

    What it would catch.  A cut at `>` instead of `>=` 2^22 reads, or a chunk's read0 not added in seed_lookup_kernel / seed_pick_kernel
    (read = read0 + blockIdx.x): the reads from 2^22 on get the answers of reads 0, 1, ... — other reads, as 7 * 2^22 mod 61 = 35
    is not 0 — or none.  The totals pass launches in slices of 2^22 reads: a second slice that wrote read_hits[blockIdx.x]
    instead of [read0 + blockIdx.x] leaves the last five reads' counts unset, and n_hits and the chunk sizes differ.  The hit
    sort's end_bit is 34 + 22 = 56 here and nowhere else in the suite: a sort that stopped at fewer bits than the read field holds
    leaves hits of different reads interleaved, and the clusters, votes and n_clusters differ for most reads.  lane_off - lane_base
    and cand_offsets past the first chunk: offsets that restarted at 0 would break the flat arrays' comparison at 2^22."""
    import ctypes as C
    import time
    t0 = time.perf_counter()
    rule, genome, distinct = chunk_limit_case()
    index = sm.build_index(genome, rule[0], rule[1])
    model = [sm.read_candidates(rule, index, r) for r in distinct]
    d_n = np.array([len(m[0]) for m in model])
    d_hits, d_clusters, d_over = (np.array([m[j] for m in model], dtype=np.int64) for j in (1, 2, 3))
    d_lanes = np.array([2 * max(0, len(r) - rule[0] + 1) for r in distinct], dtype=np.int64)
    assert d_hits[:35].tolist() == [1] * 35 and d_hits[-2:].tolist() == [3, 3] and d_n[-2:].tolist() == [3, 3] and not d_hits[47:59].any()
    assert d_lanes[47] == 0 and d_lanes[48] == 0 and d_over.sum() == 0
    n = CHUNK_READS + 5
    idx = (7 * np.arange(n, dtype=np.int64)) % 61
    # the three reads around the cut: three different reads, three different answers
    around = [model[int(idx[i])][0] for i in (CHUNK_READS - 1, CHUNK_READS, CHUNK_READS + 1)]
    assert idx[CHUNK_READS - 1: CHUNK_READS + 2].tolist() == [28, 35, 42] and all(around) and len({tuple(a) for a in around}) == 3
    # the expected flat arrays
    counts = d_n[idx]
    want_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    want = [np.zeros(int(want_offs[-1]), dtype=t) for t in (np.uint64, np.uint8, np.uint32)]
    for j in range(int(d_n.max())):
        has = counts > j
        for col, w in enumerate(want):
            w[want_offs[:-1][has].astype(np.int64) + j] = np.array([m[0][j][col] if len(m[0]) > j else 0 for m in model], dtype=np.int64)[idx[has]]
    hits, lanes = d_hits[idx], d_lanes[idx]
    # a condition, not a measurement: at this budget it is the read count that cuts the first chunk
    mb = 1024
    budget_hits = (mb << 20) // HIT_BYTES
    assert hits[:CHUNK_READS].sum() + hits[CHUNK_READS] <= budget_hits and lanes[:CHUNK_READS + 1].sum() <= 4 * budget_hits
    assert simulated_chunks(hits, lanes, mb) == [0, CHUNK_READS]
    assert hits[:CHUNK_READS].sum() > ((256 << 20) // HIT_BYTES)          # (the default budget would cut by the hits first)
    buffers = [C.create_string_buffer(r, len(r) + 1) for r in distinct]
    lengths = [len(r) for r in distinct]
    aligner.set_genome(genome)
    calls = [(mb, n), (1, (1 << 20) + 1)]
    first = simulated_chunks(hits[:calls[1][1]], lanes[:calls[1][1]], 1)
    if first[-1] != 1 << 20:                         # the same reads up to the first of that call's last chunk: a last chunk of one read
        calls.append((1, first[-1] + 1))
    try:
        for budget, n_reads in calls:
            first = simulated_chunks(hits[:n_reads], lanes[:n_reads], budget)
            aligner.index_genome(api.SeedRule(*rule, budget))
            t1 = time.perf_counter()
            offs, starts, rev, votes, info = find_flat(aligner, buffers, lengths, idx[:n_reads])
            t2 = time.perf_counter()
            print("test_more_reads_than_one_chunk_holds: %d reads at %d MB, %d chunks, the last of %d reads: %.2f s in scrg_find_candidates"
                  % (n_reads, budget, len(first), n_reads - first[-1], t2 - t1))
            tag = (budget, n_reads)
            if budget == 1:
                assert len(first) >= 60, tag         # 1.36 hits a read, 2^20 reads, 21 845 hits a chunk: 65 chunks
            m = int(want_offs[n_reads])
            assert np.array_equal(offs, want_offs[:n_reads + 1]), (tag, "offsets", int(np.argmax(offs != want_offs[:n_reads + 1])))
            for what, g, w in zip(("starts", "strands", "votes"), (starts, rev, votes), want):
                assert g.dtype == w.dtype and np.array_equal(g, w[:m]), (tag, what, int(np.argmax(g != w[:m])))
            assert info == {"n_hits": int(hits[:n_reads].sum()), "n_clusters": int(d_clusters[idx[:n_reads]].sum()), "n_keys_over_max_occ": 0,
                            "n_lookups": int(lanes[:n_reads].sum())}, tag
        assert n_reads - first[-1] == 1
    finally:
        aligner.clear_index()                        # (the chunk's buffers go with it)
        aligner.clear_genome()
    print("test_more_reads_than_one_chunk_holds: %.2f s" % (time.perf_counter() - t0))


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
