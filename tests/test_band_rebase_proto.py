"""The band table's kept columns in the coordinates of the column to their right (tests/proto/lane_band_rebase_proto.c: one
addition per kept column instead of two shifts; the words lose the band's top row, delta = -10, and gain a bit without meaning at
delta = +22).  The data sets and edge-row cases of tests/test_band_proto.py are replayed through it: every pair's edit distance and
runs equal the full rows' (go_align_codes), no safe window is walked differently on the two tables, and nothing changes when the
meaningless bit is forced to any of its four values in the two words."""
import ctypes as C
import os
import subprocess

import pytest

from scrooge_amd import synth
from tests.conftest import load_golden
from tests.test_band_proto import DOWN, LSB32, SAFE, UP, _adversarial, _block_pairs, _cigar, _full
from tests.test_lane_proto import _cases, _run

HERE = os.path.dirname(os.path.abspath(__file__))
LOWS = (0, 1, 2, 3, 4)          # bit 0 of (V1, V0): as computed, then forced to 00, 01, 10, 11


@pytest.fixture(scope="module")
def proto():
    so = os.path.join(HERE, "proto", "liblane_band_rebase_proto.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-fopenmp", "-fPIC", "-shared", "-w", "-o", so,
                           os.path.join(HERE, "proto", "lane_band_rebase_proto.c")])
    return C.CDLL(so)


def _rebased(proto, t, q, O, ls, low=0, band=(UP, DOWN, SAFE)):
    return _run(proto.lane_align_codes_band32_rebased, t, q, (C.c_int(64), C.c_int(O), *(C.c_int(x) for x in band), C.c_int(low)), (C.byref(ls),))


def _check(proto, T, Q, O, lows=LOWS):
    """Zero differences to full rows, for every setting of the meaningless bit -> the stats of the as-computed pass."""
    first = None
    for low in lows:
        ls = LSB32()
        for k, (t, q) in enumerate(zip(T, Q)):
            assert _rebased(proto, t, q, O, ls, low) == _full(proto, t, q, O), (k, low)
        assert ls.mismatching_safe_windows == 0, low
        first = first or ls
    return first


@pytest.mark.parametrize("name", ["pairs_w64_o33.json", "pairs_w64_o40.json"])
def test_golden_pairs(proto, name):
    g = load_golden(name)
    for low in LOWS:
        ls = LSB32()
        for k, c in enumerate(g["cases"]):
            ed, runs = _rebased(proto, c["text"].upper().encode(), c["read"].upper().encode(), g["O"], ls, low)
            assert (ed, _cigar(runs)) == (c["ed"], c["cigar"]), (k, low)
        assert ls.mismatching_safe_windows == 0 and ls.banded > 100


def test_golden_mapping(proto, golden_mapping):
    g = golden_mapping
    T, Q = [], []
    for read, cands in zip(g["reads"], g["candidates"]):
        for c in cands:
            T.append(g["genome"][c:].encode())
            Q.append(read.encode())
    for low in LOWS:
        ls = LSB32()
        for k, (t, q) in enumerate(zip(T, Q)):
            ed, runs = _rebased(proto, t, q, g["O"], ls, low)
            assert (ed, _cigar(runs)) == (g["ed"][k], g["cigar"][k]), (k, low)
        assert ls.mismatching_safe_windows == 0 and ls.banded > 50


@pytest.mark.parametrize("O", [33, 40, 63])
def test_golden_plane(proto, O):
    from tests import plane_inputs as pi
    from tests.test_plane import load
    T, Q, groups, fx = load(64, O)
    for low in LOWS:
        ls = LSB32()
        bad = []
        for k, (t, q) in enumerate(zip(T, Q)):
            ed, runs = _rebased(proto, t.upper().encode() if isinstance(t, str) else t, q.upper().encode() if isinstance(q, str) else q, O, ls, low)
            if ed != fx["ed"][k] or not pi.same_cigar(_cigar(runs), fx["cigar"][k]):
                bad.append((k, groups[k]))
        assert not bad, (low, bad[:8])
        assert ls.mismatching_safe_windows == 0 and ls.banded > 300


@pytest.mark.parametrize("O", [33, 40, 50, 63])
def test_cases_of_the_lane_proto(proto, O):
    T, Q = _cases(6400 + O)
    ls = _check(proto, T, Q, O)
    assert ls.banded > 500 and ls.escapes > 0


def test_data_sets_of_the_design_table(proto):
    """ONT 10 % and PacBio 15 % reads of 10 kb and the 600 adversarial pairs: the windows the band decides are the same ones (the
    sweep is untouched), and each is walked as on full rows."""
    T, Q = synth.make_pairs(60, 10000, "ont", seed=5)
    ont = _check(proto, T, Q, 33, (0, 4))
    T, Q = synth.make_pairs(60, 10000, "pacbio15", seed=6)
    pb = _check(proto, T, Q, 33, (0, 1))
    adv = _check(proto, *_adversarial(600, 7), 33)
    assert ont.banded > 15000 and pb.banded > 15000 and adv.banded > 500 and adv.escapes > 2000


def test_ties_on_the_edge_rows(proto):
    """Block insertions of 18..22 bases and block deletions of 8..11: walks that touch delta = -9 — whose deletion neighbour is the
    row the kept words no longer have — and delta = +19, on both sides of the threshold, with and without ties."""
    T, Q, kinds = _block_pairs(11)
    escapes = {}
    for low in LOWS:
        for t, q, kd in zip(T, Q, kinds):
            ls = LSB32()
            assert _rebased(proto, t, q, 33, ls, low) == _full(proto, t, q, 33), (kd, low)
            assert ls.mismatching_safe_windows == 0
            if low == 0:
                s = escapes.setdefault(kd, [0, 0])
                s[0] += ls.escapes
                s[1] += 1
    assert 0 < escapes[("I", 18)][0] < escapes[("I", 22)][0] and 0 < escapes[("D", 8)][0] < escapes[("D", 11)][0]
    assert escapes[("D", 8)][0] < escapes[("D", 8)][1]              # (deletion blocks that a safe window walks through)
    # the test has teeth: a threshold one too high lets walks reach delta = -10, the row that is gone, and they come out wrong
    wrong = 0
    for t, q in zip(T, Q):
        ls = LSB32()
        _rebased(proto, t, q, 33, ls, 0, (UP, DOWN, SAFE + 2))
        wrong += ls.mismatching_safe_windows
    assert wrong > 0
