"""Closed-syncmer sampling of the seeding rule (include/scrooge_amd.h, SEEDING) in plain Python, on top of tests/seed_model.py: the
key, the reverse complement and the inputs are that module's, and no code is shared with the library.

A rule is seed_model's tuple (k, stride, max_occ, band, min_hits, max_candidates, strands); the sampling parameter s (`smer`) is
given beside it.  s = 0: no sampling, which is seed_model.candidates itself."""
import numpy as np

from tests import seed_model as sm


def order_word(v):
    m = (v * 0x9E3779B1) % (1 << 32)
    return m ^ (m >> 15)


def selected(key, k, s):
    """Is the key of k bases (base 0 at the top) a closed syncmer of s-mers?  s = 0: every key is."""
    if s == 0:
        return True
    words = [order_word((key >> (2 * (k - s - j))) % (4 ** s)) for j in range(k - s + 1)]
    least = min(words)
    return words[0] == least or words[-1] == least


def keys_of(seq, k):
    """The key of every window of k bases, by the base: [key_of(seq[p:p + k]) for p in ...], made in one pass."""
    out, v = [], 0
    for i, ch in enumerate(bytes(seq).decode().upper()):
        v = (v * 4 + sm.CODE[ch]) % (4 ** k)
        if i + 1 >= k:
            out.append(v)
    return out


def build_index(genome, k, stride, s):
    """-> (index: key -> positions, the positions considered)"""
    keys = keys_of(genome, k)
    index, considered = {}, 0
    for p in range(0, len(genome) - k + 1, stride):
        considered += 1
        if selected(keys[p], k, s):
            index.setdefault(keys[p], []).append(p)
    return index, considered


def read_candidates(rule, s, index, read):
    """seed_model.read_candidates with the predicate in front of the lookup -> (found, n_hits, n_clusters, n_over, n_lookups)"""
    k, stride, max_occ, band, min_hits, max_candidates, strands = rule
    found, n_hits, n_clusters, n_over, n_lookups = [], 0, 0, 0, 0
    for strand in ((0, 1) if strands == 3 else (0,)):
        r_ = sm.revcomp(read) if strand else bytes(read)
        hits = []
        for r, key in enumerate(keys_of(r_, k)):
            if not selected(key, k, s):
                continue
            n_lookups += 1
            entries = index.get(key, [])
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
    return found, n_hits, n_clusters, n_over, n_lookups


def candidates(rule, s, genome, reads):
    """-> (candidates, reverse, votes, counters) as api.candidates_from_genome(..., smer=s, info=True) returns them: the three
    counters of seed_model.candidates, n_entries and n_lookups"""
    index, _ = build_index(bytes(genome), rule[0], rule[1], s)
    cands, rev, votes = [], [], []
    info = {"n_hits": 0, "n_clusters": 0, "n_keys_over_max_occ": 0, "n_entries": sum(len(v) for v in index.values()), "n_lookups": 0}
    for read in reads:
        found, h, c, o, n = read_candidates(rule, s, index, read)
        cands.append([f[0] for f in found])
        rev.append([f[1] for f in found])
        votes.append([f[2] for f in found])
        info["n_hits"] += h
        info["n_clusters"] += c
        info["n_keys_over_max_occ"] += o
        info["n_lookups"] += n
    return cands, rev, votes, info


def longest_unselected_run(keys, k, s):
    run = worst = 0
    for key in keys:
        run = 0 if selected(key, k, s) else run + 1
        worst = max(worst, run)
    return worst


def unselected_kmer(k, s, avoid=()):
    """A k-mer (bytes) that is not selected at (k, s), found by search from a fixed seed; `avoid`: k-mers not to return."""
    rng = np.random.Generator(np.random.PCG64(1000 * k + s))
    for _ in range(100000):
        kmer = bytes(b"ACGT"[int(c)] for c in rng.integers(0, 4, k))
        if kmer not in avoid and not selected(sm.key_of(kmer), k, s):
            return kmer
    raise AssertionError("no unselected k-mer at k = %d, s = %d" % (k, s))


def unselected_genome(k, s, stride, n_positions):
    """A genome whose positions p % stride == 0 all hold unselected k-mers (stride >= k: the k-mers do not overlap), n_positions of
    them; the bases between them are A."""
    assert stride >= k
    out, seen = b"", []
    for _ in range(n_positions - 1):
        kmer = unselected_kmer(k, s, avoid=seen)
        seen.append(kmer)
        out += kmer + b"A" * (stride - k)
    return out + unselected_kmer(k, s, avoid=seen)
