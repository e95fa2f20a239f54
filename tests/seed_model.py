"""The seeding rule (include/scrooge_amd.h, SEEDING) in plain Python — lists, dicts and sorted(), no code shared with the library —
and the inputs the seeding tests share: the small shapes at which an index, a lookup, a cluster or a pick can go wrong, and the two
recall batches.

A rule is a tuple (k, stride, max_occ, band, min_hits, max_candidates, strands)."""
import numpy as np

from scrooge_amd import synth

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
DEFAULT = (13, 4, 64, 32, 2, 4, 3)


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def key_of(s):
    v = 0
    for ch in s.decode().upper():
        v = v * 4 + CODE[ch]
    return v


def build_index(genome, k, stride):
    index = {}
    for p in range(0, len(genome) - k + 1, stride):
        index.setdefault(key_of(genome[p:p + k]), []).append(p)
    return index


def read_candidates(rule, index, read):
    """-> ([(start, strand, votes)] in the rule's order, n_hits, n_clusters, n_over) of one read"""
    k, stride, max_occ, band, min_hits, max_candidates, strands = rule
    found, n_hits, n_clusters, n_over = [], 0, 0, 0
    for strand in ((0, 1) if strands == 3 else (0,)):
        r_ = revcomp(read) if strand else bytes(read)
        hits = []
        for r in range(0, len(r_) - k + 1):
            entries = index.get(key_of(r_[r:r + k]), [])
            if len(entries) > max_occ:
                n_over += 1
                continue
            hits += [(p - r, r) for p in entries]
        hits = sorted(hits)
        n_hits += len(hits)
        clusters = []
        for i, h in enumerate(hits):
            if i == 0 or h[0] - hits[i - 1][0] > band:
                clusters.append([])
            clusters[-1].append(h)
        n_clusters += len(clusters)
        for c in clusters:
            r_star, d_star = min((r, d) for d, r in c)
            if len(c) >= min_hits:
                found.append((max(0, d_star), strand, len(c)))
    found = sorted(found, key=lambda c: (-c[2], c[0], c[1]))[:max_candidates]
    return found, n_hits, n_clusters, n_over


def candidates(rule, genome, reads):
    """-> (candidates, reverse, votes, counters): per-read lists, as api.candidates_from_genome(..., info=True) returns them"""
    index = build_index(bytes(genome), rule[0], rule[1])
    cands, rev, votes, info = [], [], [], {"n_hits": 0, "n_clusters": 0, "n_keys_over_max_occ": 0}
    for read in reads:
        found, h, c, o = read_candidates(rule, index, read)
        cands.append([f[0] for f in found])
        rev.append([f[1] for f in found])
        votes.append([f[2] for f in found])
        info["n_hits"] += h
        info["n_clusters"] += c
        info["n_keys_over_max_occ"] += o
    return cands, rev, votes, info


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _codes(seq):
    lut = np.zeros(256, dtype=np.uint8)
    for ch, v in CODE.items():
        lut[ord(ch)] = v
    return lut[np.frombuffer(bytes(seq), dtype=np.uint8)]


def _stretch(genome, at, n):
    return bytes(genome[at:at + n])


def genome_length_cases():
    """Every k with genomes of k - 1 (an empty index), k, k + 1 and the word seams of the planar packing plus k, strides that do and
    do not divide the length; k = 16 on a genome with runs of T (the key's top bits set).  Reads: stretches of the genome of the
    lengths at which a read's own packing has a seam, either strand, and one that is not of the genome."""
    rng = _rng(11)
    out = []
    for k in (8, 13, 16):
        for n in [k - 1, k, k + 1] + [w + k for w in (31, 32, 33, 63, 64, 65, 127, 128, 129)]:
            genome = bytearray(synth.random_seq(n, rng))
            if k == 16:
                for at in range(0, n, 37):
                    genome[at:at + 19] = b"T" * len(genome[at:at + 19])
            genome = bytes(genome)
            reads = [b"", genome, revcomp(genome), synth.random_seq(40, rng)]
            for L in (k - 1, k, k + 1, 63, 64, 65):
                if L <= n:
                    at = int(rng.integers(0, n - L + 1))
                    reads += [_stretch(genome, at, L), revcomp(_stretch(genome, n - L, L))]
            for stride in (1, 3, 4, 64):
                out.append(("len%d_k%d_s%d" % (n, k, stride), (k, stride, 64, 32, 1, 4, 3), genome, reads))
    return out


def read_length_cases():
    """Reads of 0, k - 1, k, k + 1, 63, 64, 65, 150 and 2000 bases, exact and with errors, alternating strands; a read that is its own
    reverse complement; reads that overhang the genome's start and its end; forward only."""
    rng = _rng(12)
    genome = synth.random_seq(5000, rng)
    k = 13
    reads = []
    for i, L in enumerate((0, k - 1, k, k + 1, 63, 64, 65, 150, 2000)):
        at = int(rng.integers(0, len(genome) - L + 1))
        exact = _stretch(genome, at, L)
        noisy = synth.BASES[synth.mutate(_codes(exact), 0.05, (1, 1, 1), rng)].tobytes() if L else b""
        reads += [exact if i % 2 else revcomp(exact), revcomp(noisy) if i % 2 else noisy]
    half = _stretch(genome, 1234, 40)
    own = half + revcomp(half)                       # its own reverse complement: both strands give the same cluster
    genome_p = genome[:3000] + own + genome[3000:]
    over_start = synth.random_seq(30, rng) + genome_p[:100]
    over_end = genome_p[-100:] + synth.random_seq(30, rng)
    reads += [own, over_start, revcomp(over_start), over_end, revcomp(over_end)]
    return [("reads_s1", (k, 1, 64, 32, 2, 4, 3), genome_p, reads), ("reads_s4", (k, 4, 64, 32, 2, 4, 3), genome_p, reads),
            ("reads_fwd", (k, 1, 64, 32, 2, 4, 1), genome_p, reads), ("reads_k8", (8, 1, 64, 8, 3, 8, 3), genome_p, reads),
            ("reads_k16", (16, 3, 64, 32, 1, 4, 3), genome_p, reads)]


def occupancy_cases():
    """A key with exactly max_occ entries and one with max_occ + 1; an all-A genome: one bucket holds the whole index."""
    rng = _rng(13)
    k, occ = 13, 3
    m1, m2 = b"ACGTTGCAAGCTA", b"GGATCCTTAGACC"
    parts = []
    for i in range(occ + 1):
        parts += [synth.random_seq(90, rng), m1 if i < occ else b"", synth.random_seq(57, rng), m2]
    genome = b"".join(parts) + synth.random_seq(50, rng)
    assert genome.count(m1) == occ and genome.count(m2) == occ + 1
    reads = [m1, m2, revcomp(m1), revcomp(m2), m1 + m2, genome[60:200], revcomp(genome[300:420])]
    all_a = b"A" * 500
    return [("occ_exact", (k, 1, occ, 32, 1, 8, 3), genome, reads), ("occ_more", (k, 1, occ + 1, 32, 1, 8, 3), genome, reads),
            ("all_a_counted", (k, 1, 65535, 32, 1, 4, 3), all_a, [b"A" * 20, b"T" * 20, b"A" * 13, b"AAAAAAAAAAAAC"]),
            ("all_a_over", (k, 1, 64, 32, 1, 4, 3), all_a, [b"A" * 20, b"T" * 20]),
            ("all_a_k8_s3", (8, 3, 200, 0, 1, 64, 3), all_a, [b"A" * 30, b"T" * 9])]


def cluster_cases():
    """Gaps of exactly band and band + 1 between neighbouring diagonals; band 0; more clusters than max_candidates with ties in votes
    (the order falls to start); min_hits one above a cluster's votes."""
    rng = _rng(14)
    k, band = 13, 8
    genome = synth.random_seq(4000, rng)
    a = 700
    gap_band = genome[a:a + 40] + genome[a + 40 + band:a + 80 + band]               # a deletion of `band` bases: diagonals d and d + band
    gap_more = genome[a + 1000:a + 1040] + genome[a + 1040 + band + 1:a + 1080 + band + 1]
    exact = genome[2500:2580]
    reads = [gap_band, gap_more, exact, revcomp(gap_band), revcomp(gap_more)]
    out = [("band", (k, 1, 64, band, 2, 4, 3), genome, reads), ("band0", (k, 1, 64, 0, 2, 4, 3), genome, reads),
           ("band_s4", (k, 4, 64, band, 1, 4, 3), genome, reads)]
    unit = synth.random_seq(60, rng)
    rep = b"".join(synth.random_seq(int(n), rng) + unit for n in rng.integers(50, 90, 6)) + synth.random_seq(70, rng)
    votes = 60 - k + 1
    for name, min_hits, max_cand in (("ties", 2, 4), ("ties_all", votes, 64), ("ties_none", votes + 1, 4), ("ties_one", 1, 1)):
        out.append((name, (k, 1, 64, band, min_hits, max_cand, 3), rep, [unit, revcomp(unit), unit[:30], unit + unit]))
    return out


def big_read_cases():
    """A read whose hits fill more than one wavefront and more than one workgroup, in one cluster and in many (a tandem repeat: its
    clusters cross both seams); its hits alone are more than 1 MB holds (48 bytes a hit).  A batch in which most reads hit nothing.
    An index with one bucket per key."""
    rng = _rng(15)
    k = 13
    genome = synth.random_seq(6000, rng)
    long_read = genome[1000:3000]
    unit = synth.random_seq(100, rng)
    tandem = synth.random_seq(300, rng) + unit * 60 + synth.random_seq(300, rng)
    heavy = unit * 10                                # ~990 positions x 51 .. 60 entries each: over 50,000 hits
    noise = [synth.random_seq(150, rng) for _ in range(300)]
    some = [genome[int(s):int(s) + 150] for s in rng.integers(0, 5800, 10)]
    mixed = noise[:150] + some[:5] + [long_read] + noise[150:] + some[5:] + [revcomp(long_read)]
    # k = 8 and more than 2^15 entries: the bucket table has one bucket per key, and a lookup is the two table words alone
    wide = synth.random_seq(70000, rng)
    per_key = [wide[int(s):int(s) + 150] for s in rng.integers(0, 69000, 6)]
    per_key = per_key[:3] + [revcomp(r) for r in per_key[3:]] + [synth.random_seq(150, rng), wide[:8], wide[-9:]]
    return [("bucket_per_key", (8, 1, 64, 4, 6, 4, 3), wide, per_key),
            ("long_read", (k, 1, 64, 32, 2, 4, 3), genome, [long_read, revcomp(long_read), long_read[:300]]),
            ("heavy_read", (k, 1, 64, 32, 2, 8, 3), tandem, [unit, heavy, revcomp(heavy), unit[:50]]),
            ("mostly_nothing", (k, 1, 64, 32, 2, 4, 3), genome, mixed)]


def chunk_case():
    """A batch of more than 1 MB of hits in reads of every size, the heavy read (a chunk of its own) in its middle."""
    rng = _rng(16)
    k = 13
    unit = synth.random_seq(100, rng)
    genome = synth.random_seq(20000, rng) + unit * 60 + synth.random_seq(500, rng)
    reads = []
    for i in range(260):
        L = int(rng.choice([0, 12, 40, 150, 150, 150, 400]))
        s = int(rng.integers(0, 19000))
        r = genome[s:s + L]
        reads.append(revcomp(r) if i % 2 else r)
    reads.insert(130, unit * 10)
    reads.insert(200, genome[3000:5000])
    return ("chunks", (k, 1, 64, 32, 2, 4, 3), genome, reads)


def all_shape_cases():
    return genome_length_cases() + read_length_cases() + occupancy_cases() + cluster_cases() + big_read_cases() + [chunk_case()]


def recall_batch(kind):
    """-> (rule, genome, reads, truth): a random genome of 60 kb with no planted repeat; reads made with synth.mutate from stretches
    of it, alternating strands; truth[i] = (start of the stretch, strand, tolerance in bases).  "illumina": 200 x 150 bp at
    (k 13, stride 4, band 8, min_hits 2); "ont": 100 x 2 kb at (13, 4, 32, 4)."""
    n, L, profile, rule, tol, seed = {"illumina": (200, 150, "illumina", (13, 4, 64, 8, 2, 4, 3), 4, 21),
                                      "ont": (100, 2000, "ont", (13, 4, 64, 32, 4, 4, 3), 40, 22)}[kind]
    rng = _rng(seed)
    err, ratio = synth.PROFILES[profile]
    codes = rng.integers(0, 4, 60000, dtype=np.uint8)
    genome = synth.BASES[codes].tobytes()
    reads, truth = [], []
    for i in range(n):
        need = int(L * 1.25) + 64
        s = int(rng.integers(0, len(genome) - need))
        read = synth.mutate(codes[s:s + need], err, ratio, rng)[:L]
        assert len(read) == L
        read = synth.BASES[read].tobytes()
        reads.append(revcomp(read) if i % 2 else read)
        truth.append((s, i % 2, tol))
    return rule, genome, reads, truth


def recall(cands, rev, truth):
    """-> (reads whose true start is among their candidates on the true strand, within the tolerance; the worst error among them)"""
    found, worst = 0, 0
    for c, r, (s, strand, tol) in zip(cands, rev, truth):
        errs = [abs(int(x) - s) for x, y in zip(c, r) if int(y) == strand and abs(int(x) - s) <= tol]
        if errs:
            found += 1
            worst = max(worst, min(errs))
    return found, worst
