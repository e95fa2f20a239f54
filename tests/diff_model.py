"""The difference strings (MD and short cs) as a Python model written from the rules of include/scrooge_amd.h (DIFFERENCE STRINGS),
and the inputs of tests/test_diff_strings.py.  Nothing here calls the library.

A pair's alignment is its runs in order, never merged across windows.  t and q are the positions in the text and in the read as
aligned (a minus-strand pair's read is its reverse complement; text bases are the forward text's).
  MD: a number, then an item and a number per mismatched base ('X': the text base) and per maximal stretch of directly adjacent
      'D' runs ('^' and its text bases); a number is the count of '=' bases since the previous item; insertions are not written and
      neither add to a number nor reset it.
  cs: ":n" per maximal stretch of '=' bases (no ":0"), "*tq" per 'X' base, "+bases" / "-bases" per maximal stretch of adjacent
      'I' / 'D' runs (read / text bases), lower case.
  A pair without runs has "" in both kinds."""
import re

import numpy as np

BASES = b"ACGT"
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")

# text, read, runs, MD, cs: the worked cases of the interface's description
TABLE = [
    ("ACGTACGTAC", "ACGTTCGAC", "4=1X2=1D2=", "4A2^T2", ":4*at:2-t:2"),
    ("ACGTAC", "ACGGGTAC", "3=2I3=", "6", ":3+gg:3"),
    ("ACGTACGTTA", "ACGTGTA", "2=2=1X1X1D2D1=", "4A0C0^GTT1", ":4*ag*ct-gtt:1"),
    ("ACGT", "TCGT", "1X3=", "0A3", "*at:3"),
    ("ACGT", "ACGA", "3=1X", "3T0", ":3*ta"),
    ("ACACTG", "ACGG", "2=2D1X1=", "2^AC0T1", ":2-ac*tg:1"),
    ("ACTCGA", "ACGA", "2=1X2D1=", "2T0^CG1", ":2*tg-cg:1"),
    ("AC", "GTG", "1D1I1D2I", "0^A0^C0", "-a+g-c+tg"),
    ("AC", "GAT", "1X1I1X", "0A0C0", "*ag+a*ct"),
    ("", "ACGT", "4I", "0", "+acgt"),
    ("ACGTTTT", "ACGT", "2=2=", "4", ":4"),
]


def parse(cigar):
    """"4=1X" -> [(4, "="), (1, "X")]"""
    return [(int(n), o) for n, o in re.findall(r"(\d+)([=XID])", cigar)]


def consumed(runs):
    """-> (text bases, read bases) the runs consume"""
    return sum(n for n, o in runs if o != "I"), sum(n for n, o in runs if o != "D")


def model(kind, text, read, runs):
    """The string of one pair; text / read: str or bytes, the read as aligned; runs: [(count, op)]; kind "md" or "cs"."""
    text = text.decode() if isinstance(text, (bytes, bytearray)) else text
    read = read.decode() if isinstance(read, (bytes, bytearray)) else read
    if not runs:
        return ""
    t = q = pend = 0
    out, prev = [], None
    for n, o in runs:
        if o == "=":
            pend += n
            t += n
            q += n
        elif o == "X":
            # per base: MD the pending number (0 after the first base) and the text base; cs "*tq", after ":n" if n are pending
            if kind == "md":
                out.append(str(pend) + "0".join(text[t:t + n].upper()))
            else:
                if pend:
                    out.append(":%d" % pend)
                out.append("".join("*" + a + b for a, b in zip(text[t:t + n].lower(), read[q:q + n].lower())))
            pend = 0
            t += n
            q += n
        elif o == "D":
            if kind == "md":
                out.append(("" if prev == "D" else str(pend) + "^") + text[t:t + n].upper())
            else:
                if pend:
                    out.append(":%d" % pend)
                out.append(("" if prev == "D" else "-") + text[t:t + n].lower())
            pend = 0
            t += n
        else:
            assert o == "I"
            if kind == "cs":
                if pend:
                    out.append(":%d" % pend)
                    pend = 0
                out.append(("" if prev == "I" else "+") + read[q:q + n].lower())
            q += n
        prev = o
    if kind == "md":
        out.append(str(pend))
    elif pend:
        out.append(":%d" % pend)
    assert t <= len(text) and q <= len(read)
    return "".join(out)


def apply_cs(text, cs):
    """The read a short cs string makes of a text, and the text bases it consumes: a check that needs no model."""
    text = text.decode() if isinstance(text, (bytes, bytearray)) else text
    t, out = 0, []
    for m in re.finditer(r":(\d+)|\*([acgt])([acgt])|\+([acgt]+)|-([acgt]+)", cs):
        if m.group(1) is not None:
            n = int(m.group(1))
            out.append(text[t:t + n].upper())
            t += n
        elif m.group(2) is not None:
            assert text[t].lower() == m.group(2), "cs names a text base the text does not have"
            out.append(m.group(3).upper())
            t += 1
        elif m.group(4) is not None:
            out.append(m.group(4).upper())
        else:
            assert text[t:t + len(m.group(5))].lower() == m.group(5), "cs names deleted bases the text does not have"
            t += len(m.group(5))
    assert "".join(m.group(0) for m in re.finditer(r":\d+|\*[acgt]{2}|\+[acgt]+|-[acgt]+", cs)) == cs, "malformed cs"
    return "".join(out), t


def md_text_consumed(md):
    """The text bases an MD string accounts for: its numbers, its mismatched bases and its deleted bases."""
    assert re.fullmatch(r"\d+(?:(?:[ACGT]|\^[ACGT]+)\d+)*", md), "malformed MD"
    return sum(int(x) for x in re.findall(r"\d+", md)) + len(re.findall(r"[ACGT]", md))


def random_runs(rng, n_runs, max_count=255):
    """A valid run list of n_runs runs: all four operations, counts 1..max_count (a quarter of them the extremes 1 and
    max_count), neighbours free to repeat an operation (adjacent D D / I I / = = runs are what window ends leave)."""
    ops = rng.choice(4, size=n_runs, p=[0.55, 0.15, 0.15, 0.15])
    cnt = rng.integers(1, max_count + 1, size=n_runs)
    ext = rng.random(n_runs)
    cnt = np.where(ext < 0.125, 1, np.where(ext > 0.875, max_count, cnt))
    return [(int(c), "=XID"[o]) for c, o in zip(cnt, ops)]


def random_seq(rng, n):
    return np.frombuffer(BASES, dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes().decode()


def random_case(rng, n_runs, max_count=255, slack=None):
    """-> (text, read, runs): random bases, the read exactly as long as the runs consume, the text up to `slack` bases longer."""
    runs = random_runs(rng, n_runs, max_count)
    tl, ql = consumed(runs)
    slack = int(rng.integers(0, 40)) if slack is None else slack
    return random_seq(rng, tl + slack), random_seq(rng, ql), runs


# Run counts per pair for the device tests.  The kernels' constants (scrooge_amd/csrc/run_walk.h, diff_kernels.hip):
#   WALK_LANE_MAX_RUNS = 24   up to 24 runs one pair per lane, from 25 one wavefront per pair
#   WALK_LANE_RUNS     = 8    runs per lane and tile of the wavefront path
#   WALK_TILE_RUNS     = 512  runs per tile: 513 is a second tile with one run, 1 025 a third
#   DIFF_TILE_BYTES    = 4096 a tile with more bytes than that is stored without staging (long X runs at 3 bytes per base)
# and both neighbours of each: 0, 1, 2 and 255 besides.
RUN_COUNTS = [0, 1, 2, 7, 8, 9, 23, 24, 25, 26, 255, 511, 512, 513, 1023, 1024, 1025]


def revcomp(s):
    s = s.encode() if isinstance(s, str) else bytes(s)
    return s.translate(COMP)[::-1].decode()


def codes_of(seq):
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    return np.searchsorted(np.frombuffer(BASES, dtype=np.uint8), np.frombuffer(seq.upper(), dtype=np.uint8)).astype(np.uint64)


def planar_words(codes):
    """Base codes (a multiple of 32 of them) -> planar 2-bit words: bit k of the low dword = bit 0 of base k's code, bit k of
    the high dword = bit 1 (include/scrooge_amd.h)."""
    c = np.asarray(codes, dtype=np.uint64).reshape(-1, 32)
    k = np.arange(32, dtype=np.uint64)
    return (((c & np.uint64(1)) << k).sum(axis=1) | (((c >> np.uint64(1)) & np.uint64(1)) << (k + np.uint64(32))).sum(axis=1)).astype(np.uint64)


def pack_contiguous(seqs, shifts):
    """Sequences one after the other in one planar array (word stride 1), sequence k starting `shifts[k]` bases past a word
    boundary; the gaps hold random bases (a kernel that reads a neighbour's base gets a wrong one, not a zero).
    -> (words incl. 4 words of padding, offsets in bases)"""
    rng = np.random.Generator(np.random.PCG64(77))
    parts, offs, pos = [], [], 0
    for s, sh in zip(seqs, shifts):
        pad = (sh - pos) % 32
        parts.append(rng.integers(0, 4, size=pad).astype(np.uint64))
        pos += pad
        offs.append(pos)
        parts.append(codes_of(s))
        pos += len(s)
    parts.append(rng.integers(0, 4, size=(-pos) % 32).astype(np.uint64))
    codes = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    words = np.concatenate([planar_words(codes), np.zeros(4, np.uint64)])
    return words, np.array(offs, dtype=np.uint64)


def pack_groups(seqs):
    """Sequences as rows of the lane-interleaved layout (word stride 64): word w of row r at ((r // 64) * words_per_row + w) * 64
    + r % 64.  -> (words incl. 2 * 64 + 2 words of padding, offsets in bases)"""
    n = len(seqs)
    wpr = max(1, max((len(s) + 31) // 32 for s in seqs)) if n else 1
    groups = (n + 63) // 64
    words = np.zeros(groups * 64 * wpr + 2 * 64 + 2, dtype=np.uint64)
    offs = np.zeros(n, dtype=np.uint64)
    for r, s in enumerate(seqs):
        c = codes_of(s)
        c = np.concatenate([c, np.zeros((-len(c)) % 32, np.uint64)])
        w = planar_words(c) if len(c) else np.zeros(0, np.uint64)
        base = (r // 64) * wpr * 64 + r % 64
        words[base + 64 * np.arange(len(w))] = w
        offs[r] = 32 * base
    return words, offs
