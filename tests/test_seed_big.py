"""Seeding past 2^31, the part that needs no GPU (tests/seed_big.py; the GPU part: test_seeding_past_2_31 of
tests/test_big_offsets_gpu.py).

1. The sparse index gives what the dense one gives — sm.candidates, ssm.candidates and the host twin on the whole genome — on a
   150 kb genome of the big genome's structure, at every rule and sampling the GPU test uses.
2. The big inputs, built from the loci alone: every fixture read's best candidate is its true locus (so the GPU test's expected
   values are real loci, not empty lists), the filler reads meet keys over max_occ, and an index whose positions lost bit 31, or
   whose keys past 2^31 were read 2^31 bases too low, answers differently for every read past 2^31: a truncated address is a
   mismatch, not luck ("Offsets past 2^31 and 2^32").
3. The words of seed_rule.h — hit, anchor, rank — at the ends of their ranges against Python integers (the header compiled for
   the host with g++: tests/proto/seed_words_host.cpp).  The kernels and the host twin compile the same header, so a wrong field
   width there is wrong on both alike, and a genome of 2^32 - 1 bases cannot be staged on every run: this is how the top of the
   range is covered."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

import scrooge_amd
from scrooge_amd import api
from tests import seed_big as sb
from tests import seed_model as sm
from tests import seed_sample_model as ssm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
T31 = sb.T31
COUNTERS = ("n_hits", "n_clusters", "n_keys_over_max_occ")


# ------------------------------------------------------------------------------------------------ 1. sparse = dense
@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


@pytest.mark.parametrize("rule,s", sb.SETUPS, ids=["k%d_s%d" % (r[0], s) for r, s in sb.SETUPS])
def test_sparse_index_equals_dense(lib, rule, s):
    """Candidates, strands, votes, the three counters, the entries and the lookups: the sparse index against the two models and
    the twin on the dense genome.  The reads: from every locus on both strands (one ends with the genome), from filler into a
    locus and its reverse complement, all T, one overhanging the last base, one that maps nowhere."""
    S = sb.small_inputs()
    genome, reads = S["genome"], S["stored"]
    dense = genome.slice(0, len(genome))
    assert len(dense) == len(genome) and dense.count(b"A") > len(dense) - 3 * 2000 and dense[-2000:] == genome.loci[-1][1]
    index, n_entries, considered = sb.sparse_index(genome, rule[0], rule[1], s)
    got = sb.model_candidates(rule, s, index, reads)
    # the filler's key really is over max_occ and really is counted, not listed
    filler = index[0]
    assert isinstance(filler, sb.Filler) and len(filler) > 1000 > rule[2]
    want_s = ssm.candidates(rule, s, dense, reads)
    assert got[:3] == want_s[:3]
    for c in COUNTERS + ("n_lookups",):
        assert got[3][c] == want_s[3][c], c
    assert n_entries == want_s[3]["n_entries"] and considered == ssm.build_index(dense, rule[0], rule[1], s)[1]
    if s == 0:
        want = sm.candidates(rule, dense, reads)
        assert got[:3] == want[:3] and all(got[3][c] == want[3][c] for c in COUNTERS)
        assert n_entries == considered == (len(dense) - rule[0]) // rule[1] + 1
    twin = api.candidates_from_genome(api.SeedRule(*rule), dense, reads, info=True, smer=s)
    assert got[:3] == twin[:3]
    for c in COUNTERS + ("n_lookups",):
        assert got[3][c] == twin[3][c], c
    assert n_entries == twin[3]["n_entries"]
    # and it says something: the locus reads are found where they were drawn, the filler reads meet the filler's key
    # (unsampled; with sampling on top of a stride a short noisy read may keep no hit, so there only most of them)
    at_locus = [i for i, p in enumerate(S["where"]) if got[0][i] and abs(got[0][i][0] - p) <= sb.RECALL_TOLERANCE and got[1][i][0] == i % 2]
    assert len(at_locus) >= (len(S["where"]) if s == 0 else 3), at_locus
    assert got[3]["n_keys_over_max_occ"] > 0 and got[0][len(S["where"]) + S["names"].index("nowhere")] == []


# ------------------------------------------------------------------------------------------------ 2. the big inputs
@pytest.fixture(scope="module")
def big():
    B = sb.big_inputs()
    out = dict(B)
    for rule, s in sb.SETUPS:
        out[(rule, s)] = sb.sparse_index(B["genome"], rule[0], rule[1], s)
    return out


def test_big_inputs_are_the_fixtures(big):
    """The loci where the GPU module has them, the reads below, across and past 2^31 and at the genome's last base."""
    g, where, reads = big["genome"], big["where"], big["reads"]
    assert len(g) == T31 + (1 << 22) and [len(s) for _, s in g.loci] == [sb.LOCUS] * 4
    assert g.slice(4_990, 5_000) == b"A" * 10 and g.slice(len(g) - 10, len(g) + 5) == g.loci[-1][1][-10:]
    assert len(reads) == 9 and sum(p > T31 for p in where) >= 4 and any(p < T31 < p + len(r) for p, r in zip(where, reads))
    assert any(p + len(r) > len(g) for p, r in zip(where, reads))
    for rule, s in sb.SETUPS:
        index, n_entries, considered = big[(rule, s)]
        assert considered == (len(g) - rule[0]) // rule[1] + 1 and len(index[0]) > considered - 4 * (sb.LOCUS + 16)
        assert (n_entries == considered) if s == 0 else (considered - 4 * (sb.LOCUS + 16) < n_entries < considered)
    assert big[(sb.K13, 0)][1] == (1 << 29) + (1 << 20) - 3


@pytest.mark.parametrize("rule,s", sb.SETUPS[:2], ids=["k13", "k16"])
def test_big_reads_are_found_at_their_loci(big, rule, s):
    """All nine fixture reads have their best candidate within 8 bases of where they were drawn, on the right strand (measured:
    errors -1, 0, 1, 2, 5, 0, 6, 0, 3; 16 to 217 hits at k = 13 and 7 to 83 at k = 16), and none meets a key over max_occ; the
    read from filler into a locus and the all-T read do."""
    index = big[(rule, s)][0]
    stored, where = big["stored"], big["where"]
    lo, hi = {13: (16, 217), 16: (7, 83)}[rule[0]]
    for i, p in enumerate(where):
        found, n_hits, _, n_over = sm.read_candidates(rule, index, stored[i])
        print("k = %d, read %d: best candidate %+d from its locus, %d hits" % (rule[0], i, found[0][0] - p if found else 0, n_hits))
        assert found and abs(found[0][0] - p) <= sb.RECALL_TOLERANCE and found[0][1] == i % 2, (i, found, p)
        assert lo <= n_hits <= hi and n_over == 0, (i, n_hits, n_over)
    for name in ("filler_to_locus", "filler_to_locus_rc", "poly_t"):
        read = stored[len(where) + big["names"].index(name)]
        assert sm.read_candidates(rule, index, read)[3] > 0, name
    into = sm.read_candidates(rule, index, stored[len(where)])[0]
    assert into and abs(into[0][0] - (big["loci"]["high"] - 30)) <= rule[0] + rule[1]          # (its first indexed window lies in the locus)
    assert sm.read_candidates(rule, index, stored[-1])[0] == []                                # the read that maps nowhere


@pytest.mark.parametrize("rule,s", sb.SETUPS, ids=["k%d_s%d" % (r[0], s) for r, s in sb.SETUPS])
def test_a_lost_bit_31_changes_the_answer(big, rule, s):
    """For every read that reaches past 2^31: the model answers differently on an index whose positions are taken & (2^31 - 1),
    and on the index of the genome whose bases past 2^31 are read 2^31 too low — which is filler wherever these reads lie, so a
    read wholly past 2^31 has no candidate left at its locus."""
    g, stored, where = big["genome"], big["stored"], big["where"]
    index = big[(rule, s)][0]
    low_pos = sb.wrapped(index, 31)
    low_keys = sb.sparse_index(g.aliased(31), rule[0], rule[1], s)[0]
    past = [i for i, p in enumerate(where) if p + len(stored[i]) > T31]
    assert len(past) >= 7
    reads = [stored[i] for i in past] + stored[len(where): len(where) + 2]          # and the two that run from filler into "high"
    true = sb.model_candidates(rule, s, index, reads)
    a = sb.model_candidates(rule, s, low_pos, reads)
    b = sb.model_candidates(rule, s, low_keys, reads)
    # (sampling on top of the stride leaves one short read without a hit: there is nothing to lose for it)
    found = [j for j in range(len(reads)) if true[0][j]]
    assert len(found) >= (len(reads) if s == 0 else len(reads) - 1)
    for j in found:
        assert max(true[0][j]) > T31 - 1000
        assert (a[0][j], a[2][j]) != (true[0][j], true[2][j]), ("positions", j)
        assert all(x < T31 for x in a[0][j])
        assert (b[0][j], b[2][j]) != (true[0][j], true[2][j]), ("keys", j)
        if j >= len(past) or where[past[j]] >= T31:
            assert not any(abs(x - true[0][j][0]) < 4000 for x in b[0][j]), ("keys", j, b[0][j])


# ------------------------------------------------------------------------------------------------ 3. the words of seed_rule.h
@pytest.fixture(scope="module")
def words():
    so = os.path.join(HERE, "proto", "libseed_words_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "scrooge_amd", "csrc"), "-o", so, os.path.join(HERE, "proto", "seed_words_host.cpp")])
    lib = C.CDLL(so)
    u32, u64, p64 = C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)
    for name, res, args in (("sw_hit_word", u64, [u64, u32, u32, u32]), ("sw_hit_group", u64, [u64]), ("sw_hit_read", u64, [u64]),
                            ("sw_hit_strand", u32, [u64]), ("sw_hit_dbias", u64, [u64]), ("sw_is_head", C.c_int, [u64, u64, u32]),
                            ("sw_anchor_word", u64, [u32, u64]), ("sw_anchor_start", u32, [u64]), ("sw_rank", None, [u32, u32, u32, u32, p64]),
                            ("sw_rank_less", C.c_int, [p64, p64]), ("sw_rank_votes", u32, [p64]), ("sw_rank_start", u32, [p64]),
                            ("sw_rank_strand", u32, [p64]), ("sw_index_entries", u64, [u64, u32, u32])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


P = [0, 1, 2**31 - 1, 2**31, 2**32 - 2]
R = [0, 1, 2**30 - 1]
READ = [0, 2**22 - 1, 2**30 - 1]
BIAS = 1 << 32


def test_hit_words_at_the_ends_of_their_ranges(words):
    """Every field reads back what was put in; the integer order of the words is the order of (read, strand, p - r); a head is
    another (read, strand) or a diagonal more than `band` further, at bands 0 and 65535 on either side of 2^31."""
    made = {}
    for q, strand, p, r in itertools.product(READ, (0, 1), P, R):
        w = words.sw_hit_word(q, strand, p, r)
        assert w == (q << 34) | (strand << 33) | (p - r + BIAS) and w < 1 << 64
        assert (words.sw_hit_read(w), words.sw_hit_strand(w), words.sw_hit_dbias(w) - BIAS) == (q, strand, p - r), (q, strand, p, r)
        assert words.sw_hit_group(w) == 2 * q + strand
        made[w] = (q, strand, p - r)
    assert sorted(made) == sorted(made, key=lambda w: made[w]) and len(set(made.values())) == len(made)
    assert min(d for _, _, d in made.values()) == -(2**30 - 1) and max(d for _, _, d in made.values()) == 2**32 - 2
    order = sorted(made)
    for band in (0, 65535):
        for prev, w in zip(order, order[1:]):
            (q0, s0, d0), (q1, s1, d1) = made[prev], made[w]
            assert words.sw_is_head(prev, w, band) == int((q0, s0) != (q1, s1) or d1 - d0 > band), (made[prev], made[w], band)
        for q, strand, p in itertools.product(READ, (0, 1), (2**31 - 1 - band, 2**31 - band, 2**31, 2**32 - 2 - band - 1)):
            prev = words.sw_hit_word(q, strand, p, 1)
            assert words.sw_is_head(prev, words.sw_hit_word(q, strand, p + band, 1), band) == 0
            assert words.sw_is_head(prev, words.sw_hit_word(q, strand, p + band + 1, 1), band) == 1
            assert words.sw_is_head(prev, words.sw_hit_word(q, strand, p + band + 1, 0), band) == 1          # (r is no part of it: d is)
            assert words.sw_is_head(prev, words.sw_hit_word(q, strand ^ 1, p, 1), band) == 1
            assert words.sw_is_head(prev, words.sw_hit_word((q + 1) % 2**30, strand, p, 1), band) == 1


def test_anchor_words_and_the_start_clamp(words):
    """The order of anchor words is (r, d); the start is max(0, d), also for d = -(2^30 - 1) and d = 2^32 - 2."""
    ds = sorted({p - r for p in P for r in R})
    assert ds[0] == -(2**30 - 1) and ds[-1] == 2**32 - 2
    made = {}
    for r, d in itertools.product(R, ds):
        a = words.sw_anchor_word(r, d + BIAS)
        assert a == (r << 33) | (d + BIAS) and a < 2**64 - 1          # (below the all-ones word the minimum starts from)
        assert words.sw_anchor_start(a) == max(0, d), (r, d)
        made[a] = (r, d)
    assert sorted(made) == sorted(made, key=lambda a: made[a]) and len(made) == len(R) * len(ds)
    # through the hit word, as the kernels take it: the diagonal of (p, r)
    for p, r in itertools.product(P, R):
        a = words.sw_anchor_word(r, words.sw_hit_dbias(words.sw_hit_word(READ[-1], 1, p, r)))
        assert words.sw_anchor_start(a) == max(0, p - r)


def test_rank_words(words):
    """votes, start and strand read back; seed_rank_less is the order of (-votes, start, strand, nth)."""
    made = []
    for votes, start, strand, nth in itertools.product((1, 2, 2**32 - 2), P, (0, 1), (0, 1, 2**32 - 1)):
        x = (C.c_uint64 * 2)()
        words.sw_rank(votes, start, strand, nth, x)
        assert (words.sw_rank_votes(x), words.sw_rank_start(x), words.sw_rank_strand(x)) == (votes, start, strand)
        assert (x[0], x[1]) != (2**64 - 1, 2**64 - 1)                  # (what seed_pick_kernel takes for "none left")
        made.append(((-votes, start, strand, nth), x))
    for (ka, a), (kb, b) in itertools.product(made, made):
        assert words.sw_rank_less(a, b) == int(ka < kb), (ka, kb)


def test_entries_of_the_set_ups(words, lib):
    """seed_index_entries of the GPU test's genome: 2^29 + 2^20 - 3 at the defaults, the sparse index's arithmetic at every set-up,
    and at stride 1 more than the 2^31 - 1 the rule check allows."""
    n = sb.GENOME_LEN
    assert words.sw_index_entries(n, 13, 4) == 2**29 + 2**20 - 3
    for (rule, s) in sb.SETUPS:
        assert words.sw_index_entries(n, rule[0], rule[1]) == sb.n_positions(n, rule[0], rule[1])
        assert api.seed_rule_check(api.SeedRule(*rule), n) == api.SCRG_OK
    assert words.sw_index_entries(n, 13, 1) == 2**31 + 2**22 - 12 > 2**31 - 1
    assert api.seed_rule_check(api.SeedRule(stride=1), n) == api.SCRG_ERR_INVALID_ARG
    for length, k, stride in ((0, 13, 4), (12, 13, 4), (13, 13, 4), (2**32 - 1, 16, 64), (2**32 - 1, 8, 2)):
        assert words.sw_index_entries(length, k, stride) == sb.n_positions(length, k, stride)
