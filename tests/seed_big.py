"""Seeding on a genome too long for the Python model to walk: a sparse form of the model's index, and the inputs of the tests that
use it (tests/test_seed_big.py on the CPU, test_seeding_past_2_31 of tests/test_big_offsets_gpu.py on the GPU).  Helpers and inputs
only, no library code.

The genome is one letter (the filler, A) with a few random stretches (loci) planted.  Every window that lies wholly in filler has
the filler's key, so the model's index (tests/seed_model.py: key -> positions) is built from the windows that touch a locus alone,
each with its real position; the filler's key holds an object whose len() is the true number of its entries — all entries, minus
the windows visited, plus the visited windows whose key is the filler's anyway.  The model only asks len(entries) > max_occ before
it iterates, so sm.read_candidates and ssm.read_candidates run on this index unchanged.  tests/test_seed_big.py proves on a genome
of 150 kb that it gives what the dense index gives.

The big inputs are those of the `big_genome` fixture of tests/test_big_offsets_gpu.py, which takes them from here: 2^31 + 2^22
bases, four loci of 20 kb (near the start, across 2^31, past it, up to the last base), nine reads drawn from them with ONT-profile
edits, and the reads that fixture does not have (extra_reads)."""
import numpy as np

from scrooge_amd import synth
from tests import anchored_inputs as ai
from tests import seed_model as sm
from tests import seed_sample_model as ssm

T31 = 1 << 31
GENOME_LEN = T31 + (1 << 22)
LOCUS = 20_000
K13, K16 = (13, 4, 64, 32, 2, 4, 3), (16, 8, 64, 32, 1, 4, 3)
# (rule, smer): what the GPU test runs and the CPU test proves the sparse index on
SETUPS = [(K13, 0), (K16, 0), (K13, 5), (K16, 7)]
RECALL_TOLERANCE = 8


class SparseGenome:
    """`length` bases of `fill` with the loci [(position, bases)] planted; nothing of that size is allocated unless asked for."""

    def __init__(self, length, loci, fill=b"A"):
        self.length, self.fill = int(length), fill
        self.loci = sorted((int(at), bytes(s)) for at, s in loci)
        ends = [0] + [at + len(s) for at, s in self.loci]
        assert all(at >= e for (at, _), e in zip(self.loci, ends)) and ends[-1] <= self.length          # apart, and inside

    def __len__(self):
        return self.length

    def slice(self, a, b):
        """genome[a:b]"""
        a, b = max(0, int(a)), min(int(b), self.length)
        if b <= a:
            return b""
        out = bytearray(self.fill * (b - a))
        for at, s in self.loci:
            lo, hi = max(a, at), min(b, at + len(s))
            if lo < hi:
                out[lo - a: hi - a] = s[lo - at: hi - at]
        return bytes(out)

    def array(self):
        """The whole genome as a uint8 array."""
        g = np.full(self.length, self.fill[0], dtype=np.uint8)
        for at, s in self.loci:
            g[at: at + len(s)] = np.frombuffer(s, dtype=np.uint8)
        return g

    def aliased(self, bit):
        """The genome a reader that lost `bit` of its base address would see: base p is base p - 2^bit wherever p >= 2^bit."""
        T = 1 << bit
        low = [(at, s[:T - at]) for at, s in self.loci if at < T]
        high = [(at + T, s[:self.length - T - at]) for at, s in low if at + T < self.length]
        return SparseGenome(self.length, low + high, self.fill)


class Filler:
    """The entries of the filler's key: counted, and listed only where every one of them was visited."""

    def __init__(self, n, listed):
        self.n, self.listed = int(n), listed

    def __len__(self):
        return self.n

    def __iter__(self):
        assert self.n == len(self.listed), "the filler's %d entries are counted, not listed: max_occ must lie below them" % self.n
        return iter(self.listed)


def n_positions(genome_len, k, stride):
    """The positions an index considers: the p with p % stride == 0 and p + k <= genome_len."""
    return (genome_len - k) // stride + 1 if genome_len >= k else 0


def sparse_index(genome, k, stride, s=0):
    """-> (index: key -> positions as the models take it, its entries, the positions considered) of a SparseGenome, sampled by s
    (0: every key).  Visited: every p with p % stride == 0, p + k <= len(genome) and p + k > a locus's start, up to that locus's
    end; every other window is filler."""
    fill_key = sm.key_of(genome.fill * k)
    assert ssm.selected(fill_key, k, s)                  # (all its s-mers tie: selected at every s)
    considered = n_positions(len(genome), k, stride)
    index, visited = {}, set()
    for at, seq in genome.loci:
        first = max(0, at - k + 1)
        first += (-first) % stride
        last = min(at + len(seq) - 1, len(genome) - k)
        if last < first:
            continue
        keys = ssm.keys_of(genome.slice(first, last + k), k)
        for p in range(first, last + 1, stride):
            if p not in visited:
                visited.add(p)
                if ssm.selected(keys[p - first], k, s):
                    index.setdefault(keys[p - first], []).append(p)
    listed = index.pop(fill_key, [])
    index[fill_key] = Filler(considered - len(visited) + len(listed), listed)
    return index, sum(len(v) for v in index.values()), considered


def wrapped(index, bit):
    """The index with bit `bit` and above of every listed position lost."""
    mask = (1 << bit) - 1
    return {key: v if isinstance(v, Filler) else sorted(p & mask for p in v) for key, v in index.items()}


def model_candidates(rule, s, index, reads):
    """The model on an index already built -> (candidates, reverse, votes, counters) as Aligner.find_candidates(reads, info=True)
    returns them: n_hits, n_clusters, n_keys_over_max_occ, n_lookups."""
    cands, rev, votes = [], [], []
    info = {"n_hits": 0, "n_clusters": 0, "n_keys_over_max_occ": 0, "n_lookups": 0}
    for read in reads:
        if s:
            found, h, c, o, n = ssm.read_candidates(rule, s, index, read)
        else:
            found, h, c, o = sm.read_candidates(rule, index, read)
            n = (2 if rule[6] == 3 else 1) * max(0, len(read) - rule[0] + 1)
        cands.append([f[0] for f in found])
        rev.append([f[1] for f in found])
        votes.append([f[2] for f in found])
        info["n_hits"] += h
        info["n_clusters"] += c
        info["n_keys_over_max_occ"] += o
        info["n_lookups"] += n
    return cands, rev, votes, info


def extra_reads(genome, locus_at, rng):
    """Reads the fixture's nine do not cover, as stored -> (reads, names): one that begins 30 bases inside the filler and runs 200
    bases into the locus at `locus_at` (boundary windows, and all-filler keys over max_occ), its reverse complement, 40 T (every
    reverse-strand key is the filler's), one that overhangs the genome's last base by 30 random bases, and 40 random bases that map
    nowhere."""
    into = genome.slice(locus_at - 30, locus_at + 200)
    over = genome.slice(len(genome) - 100, len(genome)) + synth.random_seq(30, rng)
    return ([into, sm.revcomp(into), b"T" * 40, over, synth.random_seq(40, rng)],
            ["filler_to_locus", "filler_to_locus_rc", "poly_t", "overhang", "nowhere"])


_big = []


def big_inputs():
    """The inputs of the `big_genome` fixture, drawn as it always drew them -> dict: genome (a SparseGenome), loci (name ->
    position), reads and where (the nine reads as drawn, forward, and the position each was drawn from), stored (what a seeding
    call is given: the nine with the odd ones reverse-complemented, then extra_reads), names of the extra ones."""
    if _big:
        return _big[0]
    rng = np.random.Generator(np.random.PCG64(7031))
    loci = {"low": 5_000, "across": T31 - LOCUS // 2, "high": T31 + (1 << 21) + 13, "end": GENOME_LEN - LOCUS}
    genome = SparseGenome(GENOME_LEN, [(at, synth.random_seq(LOCUS, rng)) for at in loci.values()])
    reads, where = [], []
    for name, L, back in (("low", 700, 9000), ("across", 900, 300), ("across", 1500, 2500), ("across", 400, -50), ("high", 3000, 5000),
                          ("high", 250, 100), ("end", 600, -580 + LOCUS), ("end", 2000, 15000), ("end", 300, -299 + LOCUS)):
        p = min(loci[name] + (LOCUS // 2 - back if name == "across" else back), GENOME_LEN - 1)
        reads.append(ai.mutated(genome.slice(p, p + int(1.1 * L) + 50), rng)[:L])
        where.append(p)
    extra, names = extra_reads(genome, loci["high"], np.random.Generator(np.random.PCG64(7032)))
    stored = [sm.revcomp(r) if i % 2 else r for i, r in enumerate(reads)] + extra
    _big.append(dict(genome=genome, loci=loci, reads=reads, where=where, stored=stored, names=names))
    return _big[0]


_small = []


def small_inputs():
    """A genome of the same structure small enough to index densely: 150 013 bases of filler, three loci of 2 000 bases (one at
    the last base), reads of the same kinds -> dict: genome, stored, where (of the reads drawn from loci, strand i % 2)."""
    if _small:
        return _small[0]
    rng = np.random.Generator(np.random.PCG64(7033))
    n, L = 150_013, 2_000
    at = [3_001, 74_990, n - L]
    genome = SparseGenome(n, [(a, synth.random_seq(L, rng)) for a in at])
    reads, where = [], []
    for a, length, back in ((at[0], 300, 200), (at[0], 700, 1250), (at[1], 250, 0), (at[1], 1200, 700), (at[2], 400, 1000), (at[2], 300, L - 299)):
        p = a + back
        reads.append(ai.mutated(genome.slice(p, p + int(1.1 * length) + 50), rng)[:length])
        where.append(p)
    extra, names = extra_reads(genome, at[1], rng)
    stored = [sm.revcomp(r) if i % 2 else r for i, r in enumerate(reads)] + extra
    _small.append(dict(genome=genome, stored=stored, where=where, names=names))
    return _small[0]
