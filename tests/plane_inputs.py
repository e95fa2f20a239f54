"""One adversarial input set for every window setting (W, O) of the plane tests (tests/test_plane.py, tests/golden/make_golden_plane.py).

A plain module: no fixtures, no pytest settings.  Everything is a function of (W, O): numpy PCG64 streams seeded from them, so the
fixtures under tests/golden/plane_w*_o*.json store RESULTS only (the reference's edit distances and CIGARs) and a digest of the
inputs; a test recomputes the digest before it compares any answer.

Also here: the list of settings (= the reference builds of oracle/Makefile) and a test-side statement of which kernel serves a
setting at one pair per lane, with the borders between them."""
import hashlib
import re

import numpy as np

from scrooge_amd import synth

# The reference builds of oracle/Makefile (VARIANTS, in its order) and the default build 64/33.  (256, 0) is built only to
# document why it is refused (W-O <= 255: a run count is one byte); it has no fixture.
REFUSED = (256, 0)
_VARIANTS = """32_17 64_2 48_24 64_40 128_65 96_49 100_40 256_129 192_97 128_20 200_50 16_0 24_0 40_0 64_0 128_0
  2_1 3_2 17_16 33_2 63_32 64_31 64_32 64_63 64_1 65_1 65_33 65_34 95_32 100_99 127_63 128_64 128_97 128_1
  129_1 129_2 129_65 129_66 129_98 130_2 191_64 193_97 255_127 255_128 256_1 256_127 256_128 256_255
  2_0 3_0 31_0 32_0 33_0 63_0 65_0 129_0 255_0 256_0"""
VARIANTS = [tuple(int(x) for x in v.split("_")) for v in _VARIANTS.split()]
SETTINGS = [(64, 33)] + [s for s in VARIANTS if s != REFUSED]

GROUPS = ("related", "unrelated", "low_complexity", "long_gap", "degenerate", "lattice", "short_text")
FULL_TEXT_GROUPS = ("lattice", "degenerate")      # their CIGARs are stored in full whatever their length
CIGAR_TEXT_LIMIT = 16                             # other groups: a longer CIGAR is stored as "#" + 16 hex digits of its sha256


# ------------------------------------------------------------------------------------------------ which kernel serves (W, O)
def kernel_class(W, O):
    """One pair per lane (README; genasm_kernels.h: lane_wide_serves, lane_parts_serves; scrg_api.cpp: the dispatch):
    'default' W <= 64, T <= 31 (table in 62 registers) | 'halves' W <= 128, 32 <= T <= 63 | 'parts' 64 < W <= 256 with
    64 <= T <= 127, or W > 128 with T <= 63 | 'hbm' the rest (multi-word rows in HBM), T = W - O."""
    T = W - O
    assert 2 <= W <= 256 and 1 <= T <= 255 and O >= 0, (W, O)
    if W <= 64 and T <= 31:
        return "default"
    if W <= 128 and 32 <= T <= 63:
        return "halves"
    if W > 64 and (64 <= T <= 127 or (W > 128 and T <= 63)):
        return "parts"
    return "hbm"


CLASSES = ("default", "halves", "parts", "hbm")

# every border between two kernels, or between two builds of one (vectors of one and of two words): name -> (one side, the other
# side) as predicates of (W, T, O), and the classes that serve the two sides
BORDERS = {
    "T 31|32 at W <= 64": (lambda W, T, O: W <= 64 and T == 31, lambda W, T, O: W <= 64 and T == 32, "default", "halves"),
    "T 63|64 at W = 64": (lambda W, T, O: W == 64 and T == 63, lambda W, T, O: W == 64 and T == 64, "halves", "hbm"),       # (64/0)
    "T 63|64 at 64 < W <= 128": (lambda W, T, O: 64 < W <= 128 and T == 63, lambda W, T, O: 64 < W <= 128 and T == 64, "halves", "parts"),
    "T 127|128": (lambda W, T, O: T == 127, lambda W, T, O: T == 128, "parts", "hbm"),
    "W 64|65 at T <= 31": (lambda W, T, O: W == 64 and T <= 31, lambda W, T, O: W == 65 and T <= 31, "default", "hbm"),
    "W 64|65 at 32 <= T <= 63": (lambda W, T, O: W == 64 and 32 <= T <= 63, lambda W, T, O: W == 65 and 32 <= T <= 63, "halves", "halves"),
    "W 128|129 at T <= 31": (lambda W, T, O: W == 128 and T <= 31, lambda W, T, O: W == 129 and T <= 31, "hbm", "parts"),
    "W 128|129 at 32 <= T <= 63": (lambda W, T, O: W == 128 and 32 <= T <= 63, lambda W, T, O: W == 129 and 32 <= T <= 63, "halves", "parts"),
}
for _c in CLASSES:                                 # every class accepts O = 0 somewhere: 16/0, 40/0, 65/0, 64/0
    BORDERS["O 0|1 in %s" % _c] = (lambda W, T, O, c=_c: O == 0 and kernel_class(W, O) == c,
                                   lambda W, T, O, c=_c: O == 1 and kernel_class(W, O) == c, _c, _c)


def border_cover(settings):
    """name -> (settings on one side, settings on the other) for every border."""
    return {name: tuple([(W, O) for W, O in settings if side(W, W - O, O)] for side in b[:2]) for name, b in BORDERS.items()}


# ------------------------------------------------------------------------------------------------ the inputs
def plane_inputs(W, O):
    """-> (texts, reads, groups): 90 to 200 pairs of at most ~1 kb, groups[k] names the group of pair k."""
    T = W - O
    seed = 7 * W + O
    rng = np.random.Generator(np.random.PCG64(seed))
    t, q, g = [], [], []

    def add(group, texts, reads):
        assert len(texts) == len(reads)
        t.extend(texts), q.extend(reads), g.extend([group] * len(texts))

    # related: the three error profiles; illumina long enough for several windows at this W (long match runs that cross
    # windows, halves and parts)
    add("related", *synth.make_pairs(4, 700, "ont", seed=seed))
    add("related", *synth.make_pairs(2, 900, "pacbio15", seed=seed + 1))
    add("related", *synth.make_pairs(6, min(1000, max(300, 3 * W + 40)), "illumina", seed=seed + 2))
    # unrelated: random against random, ragged and empty
    for _ in range(16):
        add("unrelated", [synth.random_seq(int(rng.integers(0, 600)), rng)], [synth.random_seq(int(rng.integers(0, 600)), rng)])
    # low complexity: a two-letter alphabet (ties), homopolymers against each other and against another letter
    for _ in range(8):
        add("low_complexity", [bytes(rng.choice(np.frombuffer(b"AC", np.uint8), int(rng.integers(1, 500))))],
            [bytes(rng.choice(np.frombuffer(b"AC", np.uint8), int(rng.integers(1, 500))))])
    add("low_complexity", [b"A" * 600, b"A" * 10, b"ACGT" * 150, b"T" * 400, b"G" * 300], [b"A" * 10, b"A" * 600, b"TGCA" * 150, b"A" * 400, b"G" * 300])
    # one long gap, in both directions
    for _ in range(6):
        s = synth.random_seq(int(rng.integers(300, 900)), rng)
        cut, gap = int(rng.integers(10, 250)), int(rng.integers(10, 140))
        add("long_gap", [s, s[:cut] + s[cut + gap:]], [s[:cut] + s[cut + gap:], s])
    add("degenerate", [b"", b"ACGT", b"", b"ACGT", b"ACGT", b"ACGT", b"AAAA"], [b"ACGT", b"", b"", b"ACGT", b"ACGA", b"TGCA", b"CCCC"])
    # the length lattice: identical and one-edit pairs whose read ends exactly on, one before and one after every window
    # boundary, with the text ending before, with and after the read
    base = synth.random_seq(4 * W + 3 * T + 8, rng)
    for L in sorted({1, 2, T - 1, T, T + 1, W - 1, W, W + 1, 2 * T, W + T - 1, W + T, W + T + 1, 2 * W, 3 * T + 1}):
        if L <= 0:
            continue
        r = bytearray(base[:L])
        r[-1] = ord("A") if r[-1] != ord("A") else ord("C")
        for read in (base[:L], bytes(r)):
            for d in (-1, 0, 1, T):
                add("lattice", [base[:max(0, L + d)]], [read])
    # reads that outlast their texts: whole windows of insertions (last, so that in the mapping-shaped call these are the
    # texts that reach the genome's end)
    for _ in range(4):
        add("short_text", [synth.random_seq(int(rng.integers(0, 60)), rng)], [synth.random_seq(int(rng.integers(300, 800)), rng)])
    return t, q, g


def inputs_digest(texts, reads, groups):
    h = hashlib.sha256()
    for a, b, c in zip(texts, reads, groups):
        h.update(b"%d,%d,%s:" % (len(a), len(b), c.encode()))
        h.update(a)
        h.update(b)
    return h.hexdigest()


def mapping_inputs(W, O):
    """The mapping-shaped call of a setting: every read against one genome made of the concatenated texts, its candidate the
    start of its own text — so a pair's text is the genome's SUFFIX from there (the reference's semantics), and the last
    texts reach the genome's end.  -> (genome, reads, candidates)"""
    t, q, _ = plane_inputs(W, O)
    starts, pos = [], 0
    for x in t:
        starts.append([pos])
        pos += len(x)
    return b"".join(t), q, starts


# settings whose fixture carries the mapping-shaped call: one per kernel class
MAPPING_SETTINGS = [(64, 33), (64, 2), (129, 65), (64, 0)]


# ------------------------------------------------------------------------------------------------ fixture helpers
SAME = "^"        # in a fixture's CIGAR list: the CIGAR of the entry before (the lattice repeats itself: one read, four texts)


def stored_cigar(cigar, group):
    """What a fixture holds for a CIGAR: its text, or '#' + the first 16 hex digits of its sha256."""
    if group in FULL_TEXT_GROUPS or len(cigar) <= CIGAR_TEXT_LIMIT:
        return cigar
    return "#" + hashlib.sha256(cigar.encode()).hexdigest()[:16]


def pack_cigars(cigars, groups):
    """The CIGAR list of a fixture: stored_cigar of every pair, SAME where it repeats the entry before."""
    full = [stored_cigar(c, g) for c, g in zip(cigars, groups)]
    return [SAME if k and c == full[k - 1] and len(c) > len(SAME) else c for k, c in enumerate(full)]


def unpack_cigars(stored):
    out = []
    for c in stored:
        out.append(out[-1] if c == SAME else c)
    return out


def same_cigar(got, stored):
    return ("#" + hashlib.sha256(got.encode()).hexdigest()[:16]) == stored if stored.startswith("#") else got == stored


def cigar_runs(cigar):
    return [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]


def fixture_name(W, O):
    return "plane_w%d_o%d.json" % (W, O)
