"""The off-centre 32-row band of the lane kernel's eligible rounds (genasm_lane_kernel.hip: lane_window_table_band and the band
form of traceback pass 1), restated in C (tests/proto/lane_band_proto.c) and checked on the CPU, run for run, against the
oracle's window loop (go_align_codes).  The band keeps rows i - 10 .. i + 21 of column i; its own D[0][0] <= 19 proves a window
safe (the proof: lane_band_proto.c), any other window is redone on the full table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from scrooge_amd import synth
from tests.conftest import load_golden
from tests.test_lane_proto import _cases, _run

HERE = os.path.dirname(os.path.abspath(__file__))
UP, DOWN, SAFE = 10, 21, 19          # the kernel's constants (genasm_lane_kernel.hip: BAND_UP, BAND_DOWN, BAND_SAFE)


@pytest.fixture(scope="module")
def proto():
    so = os.path.join(HERE, "proto", "liblane_band_proto.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fopenmp", "-fPIC", "-shared", "-w", "-o", so,
                           os.path.join(HERE, "proto", "lane_band_proto.c")])
    return C.CDLL(so)


class LSB32(C.Structure):
    _fields_ = [("windows", C.c_uint64), ("banded", C.c_uint64), ("escapes", C.c_uint64), ("mismatching_safe_windows", C.c_uint64),
                ("hist", C.c_uint64 * 66)]


def _band(proto, t, q, O, ls, band=(UP, DOWN, SAFE)):
    return _run(proto.lane_align_codes_band32, t, q, (C.c_int(64), C.c_int(O), *(C.c_int(x) for x in band)), (C.byref(ls),))


def _full(proto, t, q, O):
    return _run(proto.go_align_codes, t, q, (C.c_int(64), C.c_int(O)), (None,))


def _cigar(runs):
    return "".join("%d%s" % (runs[k], chr(runs[k + 1])) for k in range(0, len(runs), 2))


def _check(proto, T, Q, O, band=(UP, DOWN, SAFE)):
    ls = LSB32()
    for k, (t, q) in enumerate(zip(T, Q)):
        assert _band(proto, t, q, O, ls, band) == _full(proto, t, q, O), k
    assert ls.mismatching_safe_windows == 0
    return ls


@pytest.mark.parametrize("name", ["pairs_w64_o33.json", "pairs_w64_o40.json"])
def test_golden_pairs(proto, name):
    """The pair goldens at W = 64 with W-O <= 31: the reference's own edit distances and CIGARs.  (With test_golden_mapping and
    test_golden_plane: every committed golden at these settings.)"""
    g = load_golden(name)
    ls = LSB32()
    for k, c in enumerate(g["cases"]):
        ed, runs = _band(proto, c["text"].upper().encode(), c["read"].upper().encode(), g["O"], ls)      # (codes: case is the host layer's business)
        assert (ed, _cigar(runs)) == (c["ed"], c["cigar"]), k
    assert ls.mismatching_safe_windows == 0 and ls.banded > 100


def test_golden_mapping(proto, golden_mapping):
    g = golden_mapping
    T, Q = [], []
    for read, cands in zip(g["reads"], g["candidates"]):
        for c in cands:
            T.append(g["genome"][c:].encode())
            Q.append(read.encode())
    ls = LSB32()
    for k, (t, q) in enumerate(zip(T, Q)):
        ed, runs = _band(proto, t, q, g["O"], ls)
        assert (ed, _cigar(runs)) == (g["ed"][k], g["cigar"][k]), k
    assert ls.mismatching_safe_windows == 0 and ls.banded > 50


@pytest.mark.parametrize("O", [33, 40, 63])
def test_golden_plane(proto, O):
    """The plane goldens at W = 64 with W-O <= 31 (tests/golden/plane_w64_o*.json: the reference's answers on the length lattice,
    long gaps, short texts; O = 63 is the only golden at W-O = 1): every pair's edit distance and CIGAR."""
    from tests import plane_inputs as pi
    from tests.test_plane import load
    T, Q, groups, fx = load(64, O)
    ls = LSB32()
    bad = []
    for k, (t, q) in enumerate(zip(T, Q)):
        ed, runs = _band(proto, t.upper().encode() if isinstance(t, str) else t, q.upper().encode() if isinstance(q, str) else q, O, ls)
        if ed != fx["ed"][k] or not pi.same_cigar(_cigar(runs), fx["cigar"][k]):
            bad.append((k, groups[k]))
    assert not bad, bad[:8]
    assert ls.mismatching_safe_windows == 0 and ls.banded > 300          # (the band does decide hundreds of these windows)


@pytest.mark.parametrize("O", [33, 40, 50, 63])
def test_cases_of_the_lane_proto(proto, O):
    T, Q = _cases(6400 + O)
    ls = _check(proto, T, Q, O)
    assert ls.banded > 500 and ls.escapes > 0


def _adversarial(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    T, Q = [], []
    for k in range(n):
        L = int(rng.integers(200, 600))
        if k % 2:
            T.append(synth.random_seq(L, rng)), Q.append(synth.random_seq(L, rng))
        else:
            T.append(bytes(rng.choice(np.frombuffer(b"AC", np.uint8), L))), Q.append(bytes(rng.choice(np.frombuffer(b"AC", np.uint8), L)))
    return T, Q


def test_data_sets_of_the_design_table(proto):
    """ONT 10 % and PacBio 15 % reads of 10 kb, and 600 adversarial pairs (low-complexity "AC" and unrelated random ones)."""
    T, Q = synth.make_pairs(60, 10000, "ont", seed=5)
    ont = _check(proto, T, Q, 33)
    T, Q = synth.make_pairs(60, 10000, "pacbio15", seed=6)
    pb = _check(proto, T, Q, 33)
    adv = _check(proto, *_adversarial(600, 7), 33)
    assert ont.banded > 15000 and pb.banded > 15000 and adv.banded > 500 and adv.escapes > 2000
    assert pb.escapes > ont.escapes


def test_escape_rate_on_ont_reads(proto):
    """Per window below 0.2 % — four times what was measured — so that fewer than 12 % of a wavefront's rounds are redone."""
    T, Q = synth.make_pairs(100, 4000, "ont", seed=77)
    ls = _check(proto, T, Q, 33)
    assert ls.windows > 12000
    p = ls.escapes / ls.windows
    print("escape rate per window: %.5f (%d of %d)" % (p, ls.escapes, ls.windows))
    assert p < 0.002
    assert 1 - (1 - p) ** 64 < 0.12


def _block_pairs(seed):
    """One block insertion of 18..22 bases and one block deletion of 8..11 bases, each within the first 31 columns of a window
    (the pair's first window, and later ones by way of a clean prefix of k * 31 bases), in random and in low-complexity
    surroundings: the latter put ties between I, D and X on the path."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T, Q, kinds = [], [], []
    for low in (False, True):
        for prefix in (0, 31, 62):
            for ins in range(18, 23):
                for dele in range(8, 12):
                    for at in (1, 9, 17, 25, 30):
                        L = prefix + 400
                        a = bytes(rng.choice(np.frombuffer(b"AC", np.uint8), L)) if low else synth.random_seq(L, rng)
                        p = prefix + at
                        extra = bytes(rng.choice(np.frombuffer(b"AC", np.uint8), ins)) if low else synth.random_seq(ins, rng)
                        T.append(a), Q.append(a[:p] + extra + a[p:]), kinds.append(("I", ins))
                        T.append(a), Q.append(a[:p] + a[p + dele:]), kinds.append(("D", dele))
                        # both in one read, three windows apart
                        p2 = p + 93
                        T.append(a), Q.append(a[:p] + extra + a[p:p2] + a[p2 + dele:]), kinds.append(("ID", ins))
    return T, Q, kinds


def test_ties_on_the_edge_rows(proto):
    """Block insertions of 18..22 bases reach delta = +18..+22 (the band ends at +21, a safe window at +19), block deletions of
    8..11 bases delta = -8..-11 (the band ends at -10, a safe window at -9): both sides of the threshold, with and without ties."""
    T, Q, kinds = _block_pairs(11)
    by_kind = {}
    for t, q, kd in zip(T, Q, kinds):
        ls = LSB32()
        assert _band(proto, t, q, 33, ls) == _full(proto, t, q, 33), kd
        assert ls.mismatching_safe_windows == 0
        s = by_kind.setdefault(kd, [0, 0])
        s[0] += ls.escapes
        s[1] += 1
    # both sides of the threshold occur: the longer the block, the more of its windows are redone, and neither end is all or none
    # (in low-complexity surroundings a block is often cheaper to align than its length)
    assert 0 < by_kind[("I", 18)][0] < by_kind[("I", 22)][0]
    assert 0 < by_kind[("D", 8)][0] < by_kind[("D", 11)][0]
    assert by_kind[("I", 18)][0] < by_kind[("I", 18)][1] and by_kind[("D", 8)][0] < by_kind[("D", 8)][1]       # (pairs with no escape at all)
    # the centred band of the earlier prototype is exact on its own claim as well ...
    _check(proto, T[::7], Q[::7], 33, (15, 16, 14))
    # ... and the threshold is tight: one more edit claimed safe, or one row less above the diagonal, and a visited cell's
    # deletion neighbour lies outside the band, where these windows are decided wrongly.  (The test has teeth.)
    for band in ((10, 21, 20), (9, 22, 19)):
        wrong = 0
        for t, q in zip(T, Q):
            ls = LSB32()
            _band(proto, t, q, 33, ls, band)
            wrong += ls.mismatching_safe_windows
        assert wrong > 0, band
