"""One batch and its PLACEMENTS for the tests that move the buffers past 2^31 and 2^32 (tests/test_big_offsets.py on the CPU,
tests/test_big_offsets_gpu.py on the GPU).

A plain module: no fixtures, no pytest settings.  Everything is a function of numpy PCG64 seeds.

The batch (`batch()`): about 100 pairs — groups of plane_inputs.plane_inputs(64, 33), short related pairs whose run counts lie
on both sides of 16 (the compaction's threshold) and 24 (WALK_LANE_MAX_RUNS), and 3-6 kb noisy pairs of more than 512 runs
(WALK_TILE_RUNS).  A third of the reads are flagged SCRG_READ_REVCOMP, a third of the texts SCRG_TEXT_REVCOMP.  Every text has
a TAIL of random bases behind it, so that the same pair can be declared as mapping declares it — a forward text is the suffix
up to the buffer's end, a reversed one the whole prefix — with an answer that does not depend on where the pair lies:
the oracle gets the first K = 4 read_len + 4 W characters of text + tail (`cut`).

A placement says where every pair's text and read lie in ONE sequence buffer of TOP = 2^32 + 2^28 bases
(`place_sequences`) and where its run slice lies in an arena of runs (`place_slices`).  For each threshold T in 2^31, 2^32 and
for the swept quantity, pairs lie wholly below T, one straddles it (with T in the middle of the bases an alignment really
uses) and the rest lie above; the other quantity lies above 2^32.  At each object's offset - 2^31 and - 2^32 lies a DECOY —
other bases, or a sentinel in an output buffer — so that a truncated or wrapped address lands inside the allocation and shows
as a mismatch."""
import numpy as np

from scrooge_amd import synth
from tests import plane_inputs as pi

T31, T32 = 1 << 31, 1 << 32
THRESHOLDS = (T31, T32)
TOP = T32 + (1 << 28)                      # bases in the sequence buffer: the highest offset is just below it
FLAG = 1 << 63                             # SCRG_READ_REVCOMP / SCRG_TEXT_REVCOMP
W_MAX = 130                                # the largest window the align tests use (129/65): tails are cut for it
PAGE = 1 << 20                             # bases per page of the sparse image; a multiple of 32
RESIDUES = (0, 31, 1, 17, 5, 30, 16, 8, 13, 26)      # offsets modulo 32, in the order they are handed out
MEMORY_CAP = 20 << 30                      # peak device memory of one test

_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return bytes(b).translate(_RC)[::-1]


# ------------------------------------------------------------------------------------------------ the batch
class Batch:
    """texts / reads: as ALIGNED; tails[k]: random bases behind text k (a multiple of 32, >= 2 K at W_MAX); read_rc / text_rc:
    the pair's flags; groups[k]: where the pair comes from."""

    def __init__(self, texts, reads, tails, groups):
        self.texts, self.reads, self.tails, self.groups = texts, reads, tails, groups
        self.n = len(texts)
        self.read_rc = [k % 3 == 1 for k in range(self.n)]
        self.text_rc = [(k // 3) % 3 == 1 for k in range(self.n)]

    def ext(self, k):
        return self.texts[k] + self.tails[k]

    def stored_text(self, k):
        """What the buffer holds for text k, tail included: forward, or the reverse complement of text + tail."""
        return revcomp(self.ext(k)) if self.text_rc[k] else self.ext(k)

    def stored_read(self, k):
        return revcomp(self.reads[k]) if self.read_rc[k] else self.reads[k]

    def cut(self, k, W, times=1):
        """The text of pair k declared as mapping declares it, as the oracle gets it: K = 4 read_len + 4 W characters."""
        return self.ext(k)[: times * (4 * len(self.reads[k]) + 4 * W)]

    def cap(self, k):
        """The pair's slice in runs: the reference's 2 x read length (and room for a text-only pair), a multiple of 16."""
        return (2 * len(self.reads[k]) + 24 + 15) // 16 * 16


_BATCH = []


def batch():
    if _BATCH:
        return _BATCH[0]
    t, q, g = pi.plane_inputs(64, 33)
    keep = {"related": 12, "unrelated": 16, "low_complexity": 13, "long_gap": 6, "degenerate": 7, "lattice": 24, "short_text": 4}
    texts, reads, groups, seen = [], [], [], {}
    for a, b, c in zip(t, q, g):
        seen[c] = seen.get(c, 0) + 1
        step = 4 if c == "lattice" else 1                      # the lattice: every fourth pair
        if (seen[c] - 1) % step == 0 and (seen[c] - 1) // step < keep[c]:
            texts.append(a), reads.append(b), groups.append(c)
    for j, L in enumerate((40, 70, 100, 130, 160, 200, 240, 280, 330, 400, 470, 520)):      # run counts around 16 and 24
        a, b = synth.make_pairs(1, L, ("illumina", "pacbio", "ont")[j % 3], seed=9100 + j)
        texts += a; reads += b; groups.append("short_related")
    for j, (L, prof) in enumerate(((3000, "ont"), (3700, "pacbio15"), (4400, "ont"), (5100, "pacbio15"), (6000, "ont"), (3300, "uniform"))):
        a, b = synth.make_pairs(1, L, prof, seed=9200 + j)     # more than 512 runs
        texts += a; reads += b; groups.append("long_noisy")
    rng = np.random.Generator(np.random.PCG64(20311))
    tails = []
    for a, b in zip(texts, reads):
        need = 2 * (4 * len(b) + 4 * W_MAX) + 64
        tails.append(synth.random_seq((max(need - len(a), 64) + 31) // 32 * 32, rng))
    _BATCH.append(Batch(texts, reads, tails, groups))
    return _BATCH[0]


def run_bands(n_runs):
    """How many pairs have run counts in 1..16, 17..24, 25..512 and above 512."""
    a = np.asarray(n_runs)
    return [int(((a >= lo) & (a <= hi)).sum()) for lo, hi in ((1, 16), (17, 24), (25, 512), (513, 1 << 30))]


# ------------------------------------------------------------------------------------------------ the sparse image of a buffer
class Image:
    """The bases of a buffer of `size` bytes, held page by page: ASCII, 0 where nothing was written (packs as A)."""

    def __init__(self, size=TOP):
        self.size, self.pages = size, {}

    def _page(self, p):
        if p not in self.pages:
            self.pages[p] = np.zeros(PAGE, dtype=np.uint8)
        return self.pages[p]

    def _spans(self, off, n):
        assert 0 <= off and off + n <= self.size, (off, n)
        done = 0
        while done < n:
            p, at = divmod(off + done, PAGE)
            m = min(n - done, PAGE - at)
            yield p, at, done, m
            done += m

    def write(self, off, data):
        """Only onto bases nobody wrote."""
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        for p, at, done, m in self._spans(off, len(data)):
            page = self._page(p)
            assert not page[at: at + m].any(), "two objects overlap at base %d" % (off + done)
            page[at: at + m] = data[done: done + m]

    def fill_unwritten(self, off, n, rng):
        for p, at, done, m in self._spans(off, n):
            page = self._page(p)
            hole = page[at: at + m] == 0
            page[at: at + m][hole] = synth.BASES[rng.integers(0, 4, int(hole.sum()))]

    def read(self, off, n):
        out = np.zeros(n, dtype=np.uint8)
        for p, at, done, m in self._spans(off, n):
            if p in self.pages:
                out[done: done + m] = self.pages[p][at: at + m]
        out[out == 0] = ord("A")
        return out.tobytes()


# ------------------------------------------------------------------------------------------------ sequences
class SeqPlacement:
    """swept: "text" or "read".  text_at[k] / read_at[k]: the first base of the stored object (text: tail included);
    image: the buffer's bases, decoys included."""

    def __init__(self, b, swept):
        self.b, self.swept, self.image = b, swept, Image()
        self.text_at, self.read_at = [0] * b.n, [0] * b.n

    # where the bases an alignment really uses lie inside the stored object
    def used(self, kind, k):
        b = self.b
        if kind == "read":
            return 0, len(b.reads[k])
        n, L = len(b.texts[k]), len(b.ext(k))
        return (L - n, L) if b.text_rc[k] else (0, n)

    def extent(self, kind, k):
        at = (self.text_at if kind == "text" else self.read_at)[k]
        return at, at + len(self.b.stored_text(k) if kind == "text" else self.b.stored_read(k))

    def used_extent(self, kind, k):
        at = self.extent(kind, k)[0]
        lo, hi = self.used(kind, k)
        return at + lo, at + hi

    def desc(self, declare):
        """-> (text_off, text_len, read_off, read_len) as Python ints per pair, flags in.  declare "exact": the text is text k
        and ends where it ends; "mapping": a forward text is the suffix up to the buffer's end, a reversed one the prefix from
        base 0 (text + tail are its first characters)."""
        b, out = self.b, []
        for k in range(b.n):
            lo, hi = self.used_extent("text", k)
            s, e = self.extent("text", k)
            if declare == "exact":
                to, tl = lo, hi - lo
            elif b.text_rc[k]:
                to, tl = 0, e
            else:
                to, tl = s, TOP - s
            out.append((to | (FLAG if b.text_rc[k] else 0), tl, self.read_at[k] | (FLAG if b.read_rc[k] else 0), len(b.reads[k])))
        return out

    def category(self, kind, k, T):
        """-1 wholly below T, 0 straddling (of the bases an alignment uses), 1 above."""
        lo, hi = self.used_extent(kind, k)
        return -1 if hi <= T else (1 if lo >= T else 0)


def _straddlers(b, kind):
    """Two long related pairs, one of each strand, whose `kind` straddles 2^31 and 2^32."""
    rc = b.text_rc if kind == "text" else b.read_rc
    long_ = [k for k in range(b.n) if b.groups[k] == "long_noisy"]
    fwd = [k for k in long_ if not rc[k]][0]
    rev = [k for k in long_ if rc[k]][0]
    return (fwd, rev) if kind == "text" else (rev, fwd)


def place_sequences(swept, b=None):
    b = b or batch()
    P = SeqPlacement(b, swept)
    other = "read" if swept == "text" else "text"
    stored = {"text": b.stored_text, "read": b.stored_read}
    at = {"text": P.text_at, "read": P.read_at}
    res = [0]

    def put(kind, k, start):
        at[kind][k] = start
        if len(stored[kind](k)):
            P.image.write(start, stored[kind](k))

    def pack(kind, ks, cursor):
        for k in ks:
            r = RESIDUES[res[0] % len(RESIDUES)]
            res[0] += 1
            cursor = (cursor + 31) // 32 * 32 + r
            put(kind, k, cursor)
            cursor += len(stored[kind](k)) + 7
        return cursor

    s31, s32 = _straddlers(b, swept)
    for k, T in ((s31, T31), (s32, T32)):
        lo, hi = P.used(swept, k)
        put(swept, k, T - (lo + hi) // 2 - (3 if T == T31 else 0))      # T in the middle of the used bases; residues differ
    rest = [k for k in range(b.n) if k not in (s31, s32)]
    below, between, above = rest[0::7], rest[1::7], [k for j, k in enumerate(rest) if j % 7 > 1]      # (7: every strand pattern in each)
    pack(swept, below, 1 << 16)
    pack(swept, between, T31 + (1 << 27))
    end = pack(swept, above, T32 + (1 << 26))
    assert end < T32 + (1 << 27)
    # the other quantity: all above 2^32, the last object ending with the buffer
    ks = list(range(b.n))
    tail_k = ks[-1]
    end = pack(other, ks[:-1], T32 + (1 << 27) + (1 << 26))
    put(other, tail_k, TOP - len(stored[other](tail_k)))
    assert end <= at[other][tail_k]
    # decoys: other bases wherever an address that lost 2^31 or 2^32 would land
    rng = np.random.Generator(np.random.PCG64(31 if swept == "text" else 32))
    for kind in ("text", "read"):
        for k in range(b.n):
            s, e = P.extent(kind, k)
            for T in THRESHOLDS:
                if e - T > 0:
                    P.image.fill_unwritten(max(0, s - T), e - T - max(0, s - T), rng)
    return P


def decoy_pair(P, k, kind, T, W):
    """(text, read) as aligned that a kernel would see if pair k's `kind` address lost T (None: the address would be negative),
    the text cut as the oracle's."""
    b = P.b
    s, e = P.extent(kind, k)
    if s - T < 0:
        return None
    got = P.image.read(s - T, e - s)
    if kind == "read":
        return b.cut(k, W), (revcomp(got) if b.read_rc[k] else got)
    ext = revcomp(got) if b.text_rc[k] else got
    return ext[: 4 * len(b.reads[k]) + 4 * W], b.reads[k]


def decoy_pair_groups(P, k, kind, T, W):
    """decoy_pair for a GroupPlacement: the object's first word moved down by T / 32 (None: that would be negative)."""
    b = P.b
    at = (P.text_at if kind == "text" else P.read_at)[k]
    n = len(P.stored(kind, k))
    if at - T < 0:
        return None
    got = P.read_words((at - T) // 32, (n + 31) // 32)[:n]
    if kind == "read":
        return b.ext(k)[: 4 * len(b.reads[k]) + 4 * W], (revcomp(got) if b.read_rc[k] else got)
    ext = revcomp(got) if b.text_rc[k] else got
    return ext[: 4 * len(b.reads[k]) + 4 * W], b.reads[k]


def seq_words(stride=1):
    """Words of the sequence buffer: TOP bases and the pad the header asks for."""
    return TOP // 32 + (4 if stride == 1 else 2 * stride + 2)


# ------------------------------------------------------------------------------------------------ sequences, grouped layout
GROUP = 64


class GroupPlacement:
    """The same sweep in the lane-interleaved layout (scrg_pack_planar_groups, word stride 64): objects are rows of BLOCKS of up
    to 64 rows, word w of row r of a block at word `base` + 64 w + r, so every object starts at a multiple of 32 bases.
    blocks: (base word, words per row, [(kind, k)] rows); decoys: (base word, words per row, rows) of random bases at a true
    block's base - 2^31 / 32 and - 2^32 / 32 where that is not negative, written BEFORE the true blocks (`uploads`).  A text cannot be longer than its row here (2^32 bases at
    stride 64 would take 64 GiB): "mapping" declares text + tail."""

    def __init__(self, b, swept):
        self.b, self.swept, self.blocks, self.decoys = b, swept, [], []
        self.text_at, self.read_at = [0] * b.n, [0] * b.n

    def stored(self, kind, k):
        return self.b.stored_text(k) if kind == "text" else self.b.stored_read(k)

    def used(self, kind, k):
        return SeqPlacement.used(self, kind, k)

    def used_extent(self, kind, k):
        """First base of the first and one past the last base of the last WORD the used bases lie in."""
        at = (self.text_at if kind == "text" else self.read_at)[k]
        lo, hi = self.used(kind, k)
        if hi == lo:
            return at, at
        return at + 32 * GROUP * (lo // 32), at + 32 * GROUP * ((hi - 1) // 32) + 32

    def category(self, kind, k, T):
        lo, hi = self.used_extent(kind, k)
        return -1 if hi <= T else (1 if lo >= T else 0)

    def desc(self, declare):
        b, out = self.b, []
        for k in range(b.n):
            to, tl = self.text_at[k], len(b.ext(k))
            if declare == "exact":
                tl = len(b.texts[k])
                if b.text_rc[k]:
                    to += 32 * GROUP * (len(b.tails[k]) // 32)       # (tails are multiples of 32: the stretch starts a word)
            out.append((to | (FLAG if b.text_rc[k] else 0), tl, self.read_at[k] | (FLAG if b.read_rc[k] else 0), len(b.reads[k])))
        return out

    def rows_of(self, block):
        base, wpr, rows = block
        a = np.zeros((len(rows), wpr * 32), dtype=np.uint8)
        for r, (kind, k) in enumerate(rows):
            s = self.stored(kind, k)
            a[r, : len(s)] = np.frombuffer(s, dtype=np.uint8)
        return a

    def words(self, block):
        base, wpr, rows = block
        return base, base + (len(rows) + GROUP - 1) // GROUP * GROUP * wpr

    def uploads(self):
        """(base word, words per row, ASCII rows) in the order they are packed into the buffer: the decoys, then the true blocks
        (a block packs all 64 rows of its range, the rows it does not have as zeros)."""
        return list(self.decoys) + [(blk[0], blk[1], self.rows_of(blk)) for blk in self.blocks]

    def read_words(self, first_word, n_words):
        """The bases of n_words words from first_word on at word stride 64, as the buffer holds them after `uploads`: ASCII, A
        where nothing (or a zero) was written."""
        out = np.zeros((n_words, 32), dtype=np.uint8)
        w = first_word + GROUP * np.arange(n_words)
        for base, wpr, rows in self.uploads():
            inside = (w >= base) & (w < base + GROUP * wpr)
            if inside.any():
                r, c = (w[inside] - base) % GROUP, (w[inside] - base) // GROUP
                got = np.zeros((int(inside.sum()), 32), dtype=np.uint8)
                have = r < rows.shape[0]
                view = rows.reshape(rows.shape[0], wpr, 32)
                got[have] = view[r[have], c[have]]
                out[inside] = got
        out[out == 0] = ord("A")
        return out.reshape(-1).tobytes()


def place_groups(swept, b=None):
    b = b or batch()
    P = GroupPlacement(b, swept)
    other = "read" if swept == "text" else "text"
    at = {"text": P.text_at, "read": P.read_at}

    def block(kind, ks, base):
        wpr = max(1, max((len(P.stored(kind, k)) + 31) // 32 for k in ks))
        P.blocks.append((base, wpr, [(kind, k) for k in ks]))
        for r, k in enumerate(ks):
            at[kind][k] = 32 * (base + r)
        return P.words(P.blocks[-1])[1]

    s31, s32 = _straddlers(b, swept)
    rest = [k for k in range(b.n) if k not in (s31, s32)]
    below, between, above = rest[0::7], rest[1::7], [k for j, k in enumerate(rest) if j % 7 > 1]
    for k, T, mates in ((s31, T31, above[:5]), (s32, T32, above[5:10])):
        lo, hi = P.used(swept, k)
        block(swept, [k] + mates, T // 32 - GROUP * (((lo + hi) // 2) // 32))
    above = above[10:]
    block(swept, below, 1 << 12)
    block(swept, between, (T31 + (1 << 27)) // 32 + 1)
    end = block(swept, above[:GROUP], (T32 + (1 << 26)) // 32)
    if above[GROUP:]:
        end = block(swept, above[GROUP:], end + 3)
    assert end < (T32 + (1 << 27)) // 32
    ks = list(range(b.n))
    end = block(other, ks[:GROUP], (T32 + (1 << 27) + (1 << 26)) // 32)
    end = block(other, ks[GROUP:], end + 5)
    assert end + 2 * GROUP + 2 <= seq_words(GROUP)
    rng = np.random.Generator(np.random.PCG64(64))
    for blk in P.blocks:                             # (a decoy may lie across a true block: it is written first, the true one over it)
        lo, hi = P.words(blk)
        for T in THRESHOLDS:
            if lo - T // 32 >= 0:
                P.decoys.append((lo - T // 32, blk[1], synth.BASES[rng.integers(0, 4, (len(blk[2]), blk[1] * 32), dtype=np.uint8)]))
    return P


# ------------------------------------------------------------------------------------------------ run slices and other outputs
class SlicePlacement:
    """off[k], cap[k]: pair k's slice in units (runs, or bytes for a byte buffer); size: units the buffer needs; sentinels: the
    (first, count) stretches where an offset that lost 2^31 or 2^32 would write, clear of every slice."""

    def __init__(self, off, cap, size, level):
        self.off, self.cap, self.size, self.level = off, cap, size, level
        taken = sorted(zip(off, cap))
        self.sentinels = []
        for o, c in zip(off, cap):
            for T in THRESHOLDS:
                lo, hi = max(0, o - T), o + c - T
                if hi <= lo:
                    continue
                for s, n in taken:                                  # cut out what a true slice covers
                    if s < hi and s + n > lo:
                        if s > lo:
                            self.sentinels.append((lo, s - lo))
                        lo = max(lo, s + n)
                if hi > lo:
                    self.sentinels.append((lo, hi - lo))

    def category(self, k, T, used):
        """As SeqPlacement.category, for the first `used` units of the slice (what a call really writes)."""
        lo, hi = self.off[k], self.off[k] + used
        return -1 if hi <= T else (1 if lo >= T else 0)


def place_slices(caps, used, level, align=16, straddle_at=None):
    """caps[k]: units pair k needs (multiples of `align`); used[k]: units a call writes (so that a straddling slice is written
    on both sides of T).  level 31: everything up to 2^31 + 2^27, the straddler at 2^31; level 32: up to 2^32 + 2^27, with a
    straddler at each threshold.  The straddlers are the pairs that write most."""
    n = len(caps)
    order = sorted(range(n), key=lambda k: -used[k])
    ts = (T31,) if level == 31 else (T31, T32)
    off = [None] * n
    for k, T in zip(order, ts):
        assert used[k] >= 2 * align
        off[k] = T - (used[k] // 2) // align * align
    rest = [k for k in range(n) if off[k] is None]

    def pack(ks, cursor):
        for j, k in enumerate(ks):
            off[k] = cursor
            cursor += caps[k] + (align if j % 2 else 0)             # odd and even multiples of the alignment
        return cursor

    top = ts[-1]
    if level == 31:
        below, above = rest[0::4], [k for j, k in enumerate(rest) if j % 4]
        pack(below, 1 << 12)
        end = pack(above, T31 + (1 << 26))
    else:
        below, between, above = rest[0::9], rest[1::9], [k for j, k in enumerate(rest) if j % 9 > 1]
        pack(below, 1 << 12)
        pack(between, T31 + (1 << 29))
        end = pack(above, T32 + (1 << 26))
    assert end <= top + (1 << 27)
    return SlicePlacement(off, list(caps), top + (1 << 27), level)


def plan_bytes(*sizes):
    """Device bytes of the buffers a test holds at once; asserts the cap."""
    total = int(sum(sizes))
    assert total <= MEMORY_CAP, total
    return total
