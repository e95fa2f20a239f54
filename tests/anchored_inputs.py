"""Inputs for the host-layer tests of directed and anchored alignment (tests/test_anchored_host_gpu.py, the anchored shim test of
tests/test_cpp_shim.py): one genome, a directed set and an anchored set that are large and uneven enough for a call to be cut
into several chunks, and the oracle's answer for every location.

A plain module like tests/plane_inputs.py and tests/refill_inputs.py: no fixtures, no pytest settings, everything a function of
a seed.  What is drawn (genome, reads, lengths, positions, strands, directions) is the same for every window setting; what
depends on W and O is computed, never drawn: the positions W - 1, W, W + 1 among the special ones, the position of a true
leftward candidate (where its read's rightward alignment ends) and the expected results.  So how a call is cut does not depend
on the window setting.

Expected values are the oracle's on explicitly reverse-complemented Python strings, composed as tests/test_anchored_gpu.py
(host_inputs, anchored_inputs) composes them:

    a candidate (pos, reverse, leftward) of a stored read:  R' = revcomp(stored) if reverse else stored
        rightward:  oracle(genome[pos:], R')
        leftward:   oracle(revcomp(genome[:pos]), revcomp(R'))
    an anchor (ga, ra, reverse):  the leftward candidate at ga of R'[:ra] and the rightward one of R'[ra:], joined: the left
        half's runs in reversed order, then the right half's; text_start = ga - text consumed by the left half.

The conditions that tests/test_anchored_inputs.py asserts about these inputs are constants here."""
import re

import numpy as np

from scrooge_amd import synth

GENOME_LEN = 70_001                 # 17 mod 32; positions above 65 535 occur
SEED = 20_001
DIRECTED_READS, DIRECTED_LONG = 1_000, 24
ANCHORED_READS, ANCHORED_LONG = 700, 16
SEED_BASES = 12                     # bases copied exactly at an anchor
# what the sets must hold (the CPU test asserts them)
MIN_DIRECTED_CANDIDATES, MIN_ANCHORS = 2_300, 1_300
MIN_CHUNKS = 4
MIN_SHARE = 0.2                     # of the candidates, in each of the four (reverse, leftward) combinations
MIN_SPLIT_ANCHORS = MIN_UNSPLIT_ANCHORS = 100

_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(b):
    return b.translate(_RC)[::-1]


def runs_of(cigar):
    return [(int(c), o) for c, o in re.findall(r"(\d+)([=XID])", cigar)]


def text_used(cigar):
    return sum(c for c, o in runs_of(cigar) if o != "I")


def read_used(cigar):
    return sum(c for c, o in runs_of(cigar) if o != "D")


def mutated(seq, rng, err=0.10):
    """seq with ONT-profile edits (synth.mutate)."""
    if not seq:
        return b""
    codes = np.searchsorted(synth.BASES, np.frombuffer(seq, dtype=np.uint8)).astype(np.uint8)
    return synth.BASES[synth.mutate(codes, err, synth.PROFILES["ont"][1], rng)].tobytes()


def special_positions(W):
    """The positions every directed set holds in both directions (duplicates kept: W = 64 names 63, 64, 65 twice)."""
    return [0, 1, 31, 32, 33, 63, 64, 65, W - 1, W, W + 1, GENOME_LEN - 1, GENOME_LEN]


_genome = []


def genome():
    if not _genome:
        _genome.append(synth.random_seq(GENOME_LEN, np.random.Generator(np.random.PCG64(SEED))))
    return _genome[0]


# ================================================================================================ directed candidates
_directed = {}


def directed_inputs(oracle, W=64, O=33, threads=8):
    """-> dict: genome, reads (as stored), cands / rev / left (one list per read), offs (candidate offsets, n_reads + 1), and per
    candidate in nested order: eds, cigars, text_end, read_len.

    Reads 0 .. 999 have 0 to 500 bases — read 0 none, read 1 one, every tenth fewer than 16, which is shorter than any window
    used — and 1 to 4 candidates; reads 1000 .. 1023 have 3 000 to 8 000 bases and 1 or 2 candidates.  A read's first candidate
    is its true location (the read is a genome stretch with ONT-profile edits), leftward or rightward and on either strand as
    drawn; a true leftward candidate sits where the oracle's rightward alignment of the read ends.  The other candidates are
    random positions in [0, G] with strand and direction drawn independently, except that every seventh of them takes the next
    of the special positions x both directions (each combination twice), and that reads 5 and 6 hold a leftward candidate
    nearer to the genome's beginning than the read is long, and a rightward one nearer to its end."""
    key = (int(W), int(O))
    if key in _directed:
        return _directed[key]
    G, gen = GENOME_LEN, genome()
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    combos = [(p, lw) for lw in (0, 1) for p in special_positions(W)]
    aligned, g0s, cands, rev, left = [], [], [], [], []
    n_other = 0
    for r in range(DIRECTED_READS + DIRECTED_LONG):
        long_read = r >= DIRECTED_READS
        if long_read:
            L = int(rng.integers(3_000, 8_001))
        elif r < 2:
            L = r
        elif r in (5, 6):
            L = 300
        else:
            L = int(rng.integers(2, 16)) if r % 10 == 2 else int(rng.integers(1, 501))
        g0 = int(rng.integers(0, G - int(1.1 * L) - 60))
        a = mutated(gen[g0: g0 + int(1.1 * L) + 50], rng)[:L]            # the read as its TRUE candidate aligns it, left to right on the genome
        assert len(a) == L
        n_c = 1 + r % 2 if long_read else 1 + r % 4
        c_pos, c_rev, c_left = [], [], []
        for c in range(n_c):
            rv = int(rng.integers(0, 2))
            if c == 0:
                pos, lw = g0, int(rng.integers(0, 2))                  # (a leftward one is moved to where the alignment ends, below)
            elif c == 1 and r in (5, 6):
                pos, lw = (100, 1) if r == 5 else (G - 50, 0)          # the text (100 / 50 bases) is shorter than the read (300)
            elif not long_read and n_other % 7 == 0 and n_other // 7 < 2 * len(combos):
                pos, lw = combos[(n_other // 7) % len(combos)]
            else:
                pos, lw = int(rng.integers(0, G + 1)), int(rng.integers(0, 2))
            if c and not long_read and r not in (5, 6):
                n_other += 1
            c_pos.append(pos), c_rev.append(rv), c_left.append(lw)
        aligned.append(a), g0s.append(g0), cands.append(c_pos), rev.append(c_rev), left.append(c_left)
    # a true leftward candidate ends where the rightward alignment from g0 does
    lw_reads = [r for r in range(len(aligned)) if left[r][0]]
    _, cg, _, _ = oracle.align([gen[g0s[r]:] for r in lw_reads], [aligned[r] for r in lw_reads], W=W, O=O, threads=threads)
    for r, c in zip(lw_reads, cg):
        cands[r][0] = g0s[r] + text_used(c)
    # the read as stored: such that its FIRST candidate, with its strand flag, names `aligned`
    reads = [revcomp(a) if rv[0] else a for a, rv in zip(aligned, rev)]
    inp = dict(genome=gen, reads=reads, cands=cands, rev=rev, left=left, offs=np.cumsum([0] + [len(c) for c in cands]), W=int(W), O=int(O))
    inp.update(directed_expectation(oracle, gen, reads, cands, rev, left, W, O, threads))
    _directed[key] = inp
    return inp


def directed_expectation(oracle, gen, reads, cands, rev, left, W=64, O=33, threads=8):
    """The oracle's alignment of every candidate on explicit strings -> dict of lists in nested order: eds, cigars, text_end,
    read_len."""
    o_text, o_read = [], []
    for stored, c_pos, c_rev, c_left in zip(reads, cands, rev, left):
        for pos, rv, lw in zip(c_pos, c_rev, c_left):
            named = revcomp(stored) if rv else stored                  # R'
            o_text.append(revcomp(gen[:pos]) if lw else gen[pos:])
            o_read.append(revcomp(named) if lw else named)
    eds, cigars, _, _ = oracle.align(o_text, o_read, W=W, O=O, threads=threads)
    return dict(eds=eds, cigars=cigars, text_end=[text_used(c) for c in cigars], read_len=[len(x) for x in o_read])


# ================================================================================================ anchors
_anchored = {}


def anchored_inputs(oracle, W=64, O=33, threads=8):
    """-> dict: genome, reads (as stored), anchors (per read a list of (genome position, read position)), rev (per read a list),
    offs, and per anchor in nested order: named (R'), ed, cigars (joined), text_start, text_used, half_len ((ra, L - ra)).

    Reads 0 .. 699 have 1 to 3 anchors and are a genome stretch with ONT-profile edits around 12 bases copied exactly — the
    first anchor —; every third read is stored as its reverse complement.  r % 7 = 1: the anchor at the read's first position
    (ra = 0); 2: behind its last (ra = L); 3: at the genome's first position (ga = 0: what lies left of it in the read is
    inserted); 4: behind the genome's last (ga = G: what lies right of it is inserted).  An extra anchor is either a second
    true seed — every second read with extra anchors and none of these edge cases copies 12 more bases exactly further right
    and names that copy as its second anchor — or a wrong location: any genome position, any read position, either strand.
    Reads 700 .. 715 have 4 000 to 9 000 bases and one anchor in their middle third."""
    key = (int(W), int(O))
    if key in _anchored:
        return _anchored[key]
    G, gen = GENOME_LEN, genome()
    rng = np.random.Generator(np.random.PCG64(SEED + 2))
    reads, anchors, rev, kinds = [], [], [], []
    for r in range(ANCHORED_READS + ANCHORED_LONG):
        long_read = r >= ANCHORED_READS
        n_a = 1 if long_read else 1 + r % 3
        edge = 0 if long_read else r % 7
        second = n_a > 1 and edge not in (1, 2, 3, 4) and r % 2 == 0     # a second true seed, named as the read's second anchor
        if long_read:
            L = int(rng.integers(4_000, 9_001))
            la = int(L * (1 + rng.random()) / 3)
            lb = L - la - SEED_BASES
            ga = int(rng.integers(int(1.1 * la) + 100, G - int(1.1 * lb) - 200))
            left_part = mutated(gen[ga - int(1.1 * la) - 50: ga], rng)[-la:]
            right_part = gen[ga: ga + SEED_BASES] + mutated(gen[ga + SEED_BASES: ga + SEED_BASES + int(1.1 * lb) + 50], rng)[:lb]
            assert len(left_part) == la and len(left_part) + len(right_part) == L and L // 3 <= la <= 2 * L // 3 + 1
        else:
            ga = int(rng.integers(300, G - 1_000))
            la, lb, lm = int(rng.integers(0, 280)), int(rng.integers(0, 300)), int(rng.integers(0, 200))
            left_part = mutated(gen[ga - la: ga], rng)
            right_part = gen[ga: ga + SEED_BASES]
            ga2 = ga + SEED_BASES
            if second:
                right_part += mutated(gen[ga2: ga2 + lm], rng)
                ga2 += lm
                ra2 = len(left_part) + len(right_part)
                right_part += gen[ga2: ga2 + SEED_BASES]
                ga2 += SEED_BASES
            right_part += mutated(gen[ga2: ga2 + lb], rng)
            if edge == 1:
                left_part = b""                                # ra = 0
            if edge == 2:
                right_part = b""                               # ra = L
            if edge == 3:
                ga, left_part = 0, left_part[:9]               # ga = 0: whatever lies left of the anchor is inserted
                right_part = gen[:SEED_BASES] + mutated(gen[SEED_BASES: SEED_BASES + lb], rng)
            if edge == 4:
                ga, left_part = G, mutated(gen[G - la:], rng)  # ga = G: whatever lies right of the anchor is inserted
                right_part = right_part[:9]
        named = left_part + right_part                         # R' of the first anchor
        rv = 1 if r % 3 == 0 else 0
        stored = revcomp(named) if rv else named
        a, v, k = [(ga, len(left_part))], [rv], ["seed"]
        for c in range(1, n_a):
            w_ga, w_ra, w_rv = int(rng.integers(0, G + 1)), int(rng.integers(0, len(named) + 1)), int(rng.integers(0, 2))
            if second and c == 1:
                a.append((ga2 - SEED_BASES, ra2)), v.append(rv), k.append("second seed")
            else:
                a.append((w_ga, w_ra)), v.append(w_rv), k.append("wrong")
        reads.append(stored), anchors.append(a), rev.append(v), kinds.extend(k)
    inp = dict(genome=gen, reads=reads, anchors=anchors, rev=rev, kinds=kinds, offs=np.cumsum([0] + [len(a) for a in anchors]), W=int(W), O=int(O))
    inp.update(anchored_expectation(oracle, gen, reads, anchors, rev, W, O, threads))
    _anchored[key] = inp
    return inp


def anchored_expectation(oracle, gen, reads, anchors, rev, W=64, O=33, threads=8):
    """Two oracle calls per anchor on explicit strings, composed -> dict of lists in nested order: named (R'), ed, cigars (the
    left half's runs reversed, then the right half's), text_start, text_used, half_len ((ra, L - ra)); half_eds / half_cigars:
    the n left halves, then the n right halves."""
    flat = [(ga, ra, revcomp(stored) if rv else stored) for stored, a, v in zip(reads, anchors, rev) for (ga, ra), rv in zip(a, v)]
    n = len(flat)
    o_text = [revcomp(gen[:ga]) for ga, _, _ in flat] + [gen[ga:] for ga, _, _ in flat]
    o_read = [revcomp(nm[:ra]) for _, ra, nm in flat] + [nm[ra:] for _, ra, nm in flat]
    eds, cigars, _, _ = oracle.align(o_text, o_read, W=W, O=O, threads=threads)
    joined, start, used = [], [], []
    for q in range(n):
        lr, rr = runs_of(cigars[q]), runs_of(cigars[n + q])
        joined.append("".join("%d%s" % x for x in lr[::-1] + rr))
        start.append(flat[q][0] - text_used(cigars[q]))
        used.append(text_used(cigars[q]) + text_used(cigars[n + q]))
    return dict(named=[nm for _, _, nm in flat], ed=[eds[q] + eds[n + q] for q in range(n)], cigars=joined, text_start=start, text_used=used,
                half_len=[(ra, len(nm) - ra) for _, ra, nm in flat], half_eds=eds, half_cigars=cigars)


def cigars_from_arrays(out, outputs):
    """The CIGARs of an arrays=True result as strings: from the runs (outputs 2) or from the text."""
    n = len(out["edit_distance"])
    if outputs == 2:
        ro, runs = out["run_offset"], out["runs"]
        return ["".join("%d%s" % (c, chr(o)) for c, o in runs[int(ro[k]): int(ro[k + 1])]) for k in range(n)]
    co, text = out["cigar_offset"], out["cigar_text"]
    return [text[int(co[k]): int(co[k + 1]) - 1].decode() for k in range(n)]
