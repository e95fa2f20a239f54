"""Texts taken as the reverse complement of their stretch (SCRG_TEXT_REVCOMP), the parts that need no GPU: the kernels' window
load compiled for the host (scrg_text_window_planes) against a plain statement of the semantics and its bounds, the join of an
anchored pair's halves (scrg_join_anchored_runs), and the argument checks of the bindings."""
import ctypes as C

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api

COMP = bytes.maketrans(b"ACGT", b"TGCA")
CODE = {65: 0, 67: 1, 71: 2, 84: 3}
LANE = 5                      # the strided sequence is row 5 of its group of 64
SEQ_BASES = 95 + 2 * 256 + 5  # the longest stretch of the grid at the largest offset


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return api.load_library()


@pytest.fixture(scope="module")
def packed(lib):
    """One random sequence, packed once per layout by the library's host packer: stride -> (planar array, its bases)."""
    rng = np.random.Generator(np.random.PCG64(63))
    seq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), SEQ_BASES))
    words = (SEQ_BASES + 31) // 32
    out = {}
    for stride, pad in ((1, api.SEQ_PAD_WORDS), (64, api.SEQ_PAD_WORDS_GROUPS)):
        first = 0 if stride == 1 else LANE
        planar = np.full(first + (words - 1) * stride + 1 + pad, 0x5555AAAA3333CCCC, dtype=np.uint64)     # (not zeros: a word read by mistake shows)
        st = lib.scrg_pack_planar_host(seq, len(seq), planar[first:].ctypes.data, stride, words)
        assert st == 0
        out[stride] = (planar, seq, first)
    return out


def _offset(stride, first, s):
    """text_off of the stretch that starts at base s of the packed sequence (scrooge_amd.h: scrg_pair_desc)."""
    return 32 * (first + (s // 32) * stride) + s % 32


def _ref_idx_grid(text_len):
    g = {0, text_len} | {text_len - d for d in (1, 31, 32, 33, 64, 65) if text_len >= d} | set(range(0, text_len, 37))
    return sorted(g)


@pytest.mark.parametrize("W", [16, 64, 128, 256])
@pytest.mark.parametrize("stride", [1, 64])
def test_window_load_matches_the_semantics_and_stays_in_bounds(packed, stride, W):
    """Character k of a flagged text is the complement of base text_off + text_len - 1 - k: every window of the grid, flagged and
    forward, has the planes of exactly those characters on its valid bits; a flagged window reads no word below the first word of
    its stretch, and none past the padding a forward pair may read (SCRG_SEQ_PAD_WORDS, _STRIDED)."""
    planar, seq, first = packed[stride]
    pad = api.SEQ_PAD_WORDS if stride == 1 else api.SEQ_PAD_WORDS_GROUPS
    checked = 0
    for s in (0, 1, 31, 32, 33, 95):
        for text_len in (0, 1, 31, 32, 33, 63, 64, 65, W - 1, W, W + 1, 2 * W + 5):
            stretch = seq[s:s + text_len]
            assert len(stretch) == text_len
            word_lo = first + (s // 32) * stride
            word_hi = first + ((s + max(text_len, 1) - 1) // 32) * stride
            for flagged in (False, True):
                text = stretch.translate(COMP)[::-1] if flagged else stretch
                off = _offset(stride, first, s) | (api.TEXT_REVCOMP if flagged else 0)
                for ref_idx in _ref_idx_grid(text_len):
                    lo, hi, w_first, w_last = api.text_window_planes(planar, off, text_len, ref_idx, W=W, stride=stride)
                    n = min(W, text_len - ref_idx)
                    for k in range(n):
                        c = CODE[text[ref_idx + k]]
                        got = ((lo[k // 64] >> (k % 64)) & 1) | (((hi[k // 64] >> (k % 64)) & 1) << 1)
                        assert got == c, (s, text_len, flagged, ref_idx, k)
                    if n == 0:
                        assert w_first is None and w_last is None
                        continue
                    assert w_first >= word_lo, (s, text_len, flagged, ref_idx, w_first, word_lo)
                    assert w_last <= word_hi + pad, (s, text_len, flagged, ref_idx, w_last, word_hi)
                    assert (w_first - first) % stride == 0 and (w_last - first) % stride == 0       # (only words of this sequence)
                    checked += 1
    assert checked > 400                # (the grid was walked)


def test_window_load_refuses_what_it_cannot_read(packed):
    planar, seq, first = packed[1]
    with pytest.raises(scrooge_amd.ScroogeError):
        api.text_window_planes(planar, 0, 64, 65, W=64)                  # ref_idx past the text
    with pytest.raises(scrooge_amd.ScroogeError):
        api.text_window_planes(planar, 0, 64, 0, W=257)
    with pytest.raises(scrooge_amd.ScroogeError):
        api.text_window_planes(planar[:2], 0, 64, 0, W=64)               # the load's third word is not there: nothing is read
    with pytest.raises(scrooge_amd.ScroogeError):
        api.text_window_planes(planar[:2], api.TEXT_REVCOMP, 64, 0, W=64)


def test_long_stretch_keeps_its_last_bases(lib):
    """The 32-bit clamp of text_len comes after the end of the stretch is formed in 64 bits: of a stretch of 2^32 + 40 bases
    the LAST 2^32 - 1 are the text.  Its first window holds the complements of the stretch's last bases, its last character is
    the complement of base text_off + 41, and no word below that base's is read.  (The array is 1 GiB of untouched zero pages
    with a few packed words at either end.)"""
    off, text_len, reach = 7, 2 ** 32 + 40, 2 ** 32 - 1
    end = off + text_len
    planar = np.zeros((end + 31) // 32 + api.SEQ_PAD_WORDS, dtype=np.uint64)
    rng = np.random.Generator(np.random.PCG64(64))
    head = bytes(rng.choice(np.frombuffer(b"CGT", np.uint8), 128))
    tail = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 160))
    tail_at = (end - 130) // 32 * 32                               # the tail's first base, at a word boundary
    assert lib.scrg_pack_planar_host(head, len(head), planar.ctypes.data, 1, 4) == 0
    assert lib.scrg_pack_planar_host(tail, len(tail), planar[tail_at // 32:].ctypes.data, 1, 5) == 0

    def codes(lo, hi, n):
        return [((lo[k // 64] >> (k % 64)) & 1) | (((hi[k // 64] >> (k % 64)) & 1) << 1) for k in range(n)]

    lo, hi, w_first, w_last = api.text_window_planes(planar, off | api.TEXT_REVCOMP, text_len, 0, W=128)
    want = tail[end - 128 - tail_at:end - tail_at].translate(COMP)[::-1]
    assert codes(lo, hi, 128) == [CODE[c] for c in want]
    assert w_last <= (end - 1) // 32 + api.SEQ_PAD_WORDS
    # the last reachable characters: the bases from text_off + 41 on, none before
    first_base = end - reach
    assert first_base == off + 41
    lo, hi, w_first, w_last = api.text_window_planes(planar, off | api.TEXT_REVCOMP, text_len, reach - 20, W=64)
    want = head[first_base:first_base + 20].translate(COMP)[::-1]
    assert codes(lo, hi, 20) == [CODE[c] for c in want]
    assert w_first >= first_base // 32
    with pytest.raises(scrooge_amd.ScroogeError):
        api.text_window_planes(planar, off | api.TEXT_REVCOMP, text_len, reach + 1, W=64)      # past the reachable text
    # a forward text of that length keeps its FIRST 2^32 - 1 bases, as ever
    lo, hi, w_first, w_last = api.text_window_planes(planar, off, text_len, 0, W=64)
    assert codes(lo, hi, 64) == [CODE[c] for c in head[off:off + 64]]


# ------------------------------------------------------------------------------------------------ the join
def test_join_reverses_the_left_half_and_merges_nothing():
    cigar, runs, left_text = api.join_anchored("3=1X2I4=", "5=1D2=")
    assert cigar == "4=2I1X3=5=1D2="
    assert runs[0] == (4, "=") and runs[-1] == (2, "=")
    assert left_text == 3 + 1 + 4
    # the left half's last run (as produced: its first) and the right half's first have the same operation: two runs still
    cigar, runs, left_text = api.join_anchored("7=1X", "7=2I")
    assert cigar == "1X7=7=2I" and len(runs) == 4 and left_text == 8


@pytest.mark.parametrize("left,right,want,consumed", [("", "3=1I", "3=1I", 0), ("2D3=", "", "3=2D", 5), ("", "", "", 0), ("4I", "1=", "4I1=", 0)])
def test_join_empty_halves(left, right, want, consumed):
    cigar, runs, left_text = api.join_anchored(left, right)
    assert (cigar, left_text, len(runs)) == (want, consumed, len(api._parse_cigar(want)))


def test_join_text_start_arithmetic():
    """text_start = anchor - the text characters of the left half: '=', 'X' and 'D' count, 'I' does not."""
    for left, consumed in (("10=", 10), ("10I", 0), ("3=2D1X4I", 6), ("255=255D", 510)):
        assert api.join_anchored(left, "1=")[2] == consumed
        assert 1000 - api.join_anchored(left, "")[2] == 1000 - consumed


def test_join_reports_overflow_like_the_decoder(lib):
    """Too small an output array: SCRG_ERR_CIGAR_OVERFLOW with the number of runs needed, as scrg_edit_stream_to_runs; asking
    with no array at all works the same way."""
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        api.join_anchored("3=1X", "2=1I1=", capacity=4)
    assert e.value.status == api.SCRG_ERR_CIGAR_OVERFLOW and e.value.needed == 5
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        api.join_anchored("3=1X", "2=1I1=", capacity=0)
    assert e.value.status == api.SCRG_ERR_CIGAR_OVERFLOW and e.value.needed == 5
    assert api.join_anchored("3=1X", "2=1I1=", capacity=5)[0] == "1X3=2=1I1="
    # an operation that is none of = X I D
    bad = (api.Run * 1)()
    bad[0].count, bad[0].op = 3, b"M"
    n = C.c_uint64(0)
    fn = api._lazy(lib, "scrg_join_anchored_runs")
    assert fn(C.cast(bad, C.c_void_p), 1, None, 0, None, 0, C.byref(n), None) == api.SCRG_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ bindings, no device
def _no_handle():
    """An Aligner without a handle: the checks below fail before anything reaches the library."""
    return object.__new__(api.Aligner)


def test_anchors_out_of_range_are_refused_by_the_binding():
    a = _no_handle()
    with pytest.raises(ValueError):
        a.align_anchored([b"ACGTACGT"], [[(10, 9)]])               # read position past the read
    with pytest.raises(ValueError):
        a.align_anchored([b"ACGTACGT"], [[(-1, 3)]])
    with pytest.raises(ValueError):
        a.align_anchored([b"ACGTACGT"], [[(10, 3)], [(4, 1)]])     # more anchor lists than reads
    with pytest.raises(ValueError):
        a.align_anchored([b"ACGTACGT"], [[(10, 3)]], reverse=[[0, 1]])


def test_leftward_of_another_shape_is_refused_by_the_binding():
    a = _no_handle()
    with pytest.raises(ValueError):
        a.align_mapping_directed([b"ACGT", b"GGCC"], [[5], [7, 9]], leftward=[[1], [0]])
    with pytest.raises(ValueError):
        a.align_mapping_directed([b"ACGT", b"GGCC"], [[5], [7, 9]], leftward=[[1]])
    with pytest.raises(ValueError):
        a.align_mapping_directed([b"ACGT", b"GGCC"], [[5], [7, 9]], reverse=[[1], [0, 0, 1]], leftward=[[1], [0, 1]])


def test_the_new_entry_points_are_exported(lib):
    for name in ("scrg_ctx_set_text_strands", "scrg_ctx_get_text_strands", "scrg_text_window_planes", "scrg_align_mapping_directed",
                 "scrg_align_mapping_anchored", "scrg_join_anchored_runs"):
        assert name in api.EXPORTED_SYMBOLS and getattr(lib, name)
    assert api.TEXT_REVCOMP == 1 << 63
