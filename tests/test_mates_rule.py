"""The paired-end rule without a GPU: the host twin scrg_mates_from_distances (which compiles mate_rule.h, the text the kernel
compiles) against tests/mate_model.py, the rule written out in plain Python — record for record and mark for mark on drawn mate
pairs; the rule's reduction to best-candidate mode; a hand-made case in which the two modes disagree; the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from scrooge_amd import io as sio
from tests import mate_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENTATIONS = (mm.FR, mm.RF, mm.FF, mm.ANY)


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


def draw_side(rng, n, read_len, base=0, width=2000, ed_hi=4, p_over=0.15):
    """n candidates: starts in [base, base + width), strands, distances from a range small enough to tie, some over the limit"""
    return ([int(x) for x in base + rng.integers(0, width, n)], [int(x) for x in rng.integers(0, 2, n)], [int(x) for x in rng.integers(0, ed_hi, n)],
            [bool(x) for x in rng.random(n) >= p_over], read_len)


def draw_rule(rng, side_a, side_b):
    """bounds that sit exactly on a span that occurs (where one does), on both sides of others; every orientation and penalty"""
    spans = sorted({mm.span_of(s, side_a[4], t, side_b[4]) for s in side_a[0] for t in side_b[0]}) or [500]
    lo, hi = sorted(int(spans[int(k)]) for k in rng.integers(0, len(spans), 2))
    if rng.random() < 0.2:
        lo, hi = 0, 2 ** 64 - 1
    return (lo, hi, ORIENTATIONS[int(rng.integers(0, 4))], (0, 1, 1000)[int(rng.integers(0, 3))])


def twin(rule, side_a, side_b):
    """scrg_mates_from_distances through the binding -> the model's dict"""
    def arg(side):
        status = [api.SCRG_OK if ok else api.SCRG_PAIR_OVER_EDIT_LIMIT for ok in side[3]]
        return (side[0], side[1], side[2], status, side[4])
    rec, best_a, best_b = api.mates_from_distances(api.MateRule(*rule), arg(side_a), arg(side_b))
    assert int(rec["reserved"]) == 0
    w = [None if int(x) == api.MATES_NONE else int(x) for x in rec["winner"]]
    return {"winner": (w[0], w[1]), "cost": int(rec["cost"]), "second_cost": int(rec["second_cost"]), "span": int(rec["span"]),
            "n_proper": int(rec["n_proper"]), "flags": int(rec["flags"]), "is_best_a": best_a.tolist(), "is_best_b": best_b.tolist()}


def test_symbols_and_layouts(lib):
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    for name, value in (("SCRG_MATES_FR", 0), ("SCRG_MATES_RF", 1), ("SCRG_MATES_FF", 2), ("SCRG_MATES_ANY", 3), ("SCRG_MATES_PROPER", 1),
                        ("SCRG_MATES_HAS_A", 2), ("SCRG_MATES_HAS_B", 4), ("SCRG_MATES_TIED", 8)):
        assert int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1)) == value == getattr(api, name)
    assert hasattr(lib, "scrg_select_mates") and hasattr(lib, "scrg_mates_from_distances")
    assert "scrg_select_mates" in api.EXPORTED_SYMBOLS and "scrg_mates_from_distances" in sio.IO_SYMBOLS
    assert api.mate_dtype().itemsize == 32 and C.sizeof(api._MateRuleC) == 32
    assert [api.mate_dtype().fields[f][1] for f in ("winner", "cost", "second_cost", "span", "n_proper", "flags", "reserved")] == [0, 16, 20, 24, 28, 30, 31]
    assert hasattr(api.Aligner, "select_mates") and sio.mates_from_distances is api.mates_from_distances


def test_host_twin_equals_the_model(lib):
    rng = np.random.Generator(np.random.PCG64(2024))
    seen = {"proper": 0, "unpaired": 0, "tied_proper": 0, "tied_unpaired": 0, "no_a": 0, "none": 0, "on_bound": 0, "same_start": 0, "second": 0}
    for trial in range(3000):
        n_a, n_b = (int(x) for x in rng.integers(0, 10, 2))
        width = 2000 if trial % 7 else 3          # (a width of 3: equal starts on opposite strands, the FR / RF degenerate case)
        side_a = draw_side(rng, n_a, int(rng.integers(30, 250)), width=width)
        side_b = draw_side(rng, n_b, int(rng.integers(30, 250)), width=width)
        rule = draw_rule(rng, side_a, side_b)
        want, got = mm.choose(rule, side_a, side_b), twin(rule, side_a, side_b)
        assert got == want, (trial, rule, side_a, side_b)
        proper, tied = bool(want["flags"] & mm.PROPER), bool(want["flags"] & mm.TIED)
        seen["proper" if proper else "unpaired"] += 1
        seen["tied_proper"] += proper and tied
        seen["tied_unpaired"] += tied and not proper
        seen["no_a"] += not want["flags"] & mm.HAS_A
        seen["none"] += not want["flags"] & (mm.HAS_A | mm.HAS_B)
        seen["second"] += want["second_cost"] != mm.NONE32
        seen["on_bound"] += proper and want["span"] in rule[:2]
        seen["same_start"] += any(s == t and r != q for s, r in zip(side_a[0], side_a[1]) for t, q in zip(side_b[0], side_b[1]))
    assert all(v > 10 for v in seen.values()), seen


def test_ties_go_to_the_lowest_i_then_the_lowest_j(lib):
    rule = (0, 10 ** 6, mm.ANY, 0)
    a = ([100, 200, 300], [0, 0, 0], [2, 1, 1], [True] * 3, 100)
    b = ([400, 500, 600], [1, 1, 1], [3, 2, 2], [True] * 3, 100)
    got = twin(rule, a, b)
    assert got == mm.choose(rule, a, b) and got["winner"] == (1, 1) and got["cost"] == 3 and got["second_cost"] == 3
    assert got["flags"] == mm.PROPER | mm.HAS_A | mm.HAS_B | mm.TIED and got["n_proper"] == 9


def test_any_orientation_and_any_span_is_best_candidate_mode(lib):
    rng = np.random.Generator(np.random.PCG64(7))
    rule = (0, 2 ** 64 - 1, mm.ANY, 0)
    for trial in range(1500):
        side_a = draw_side(rng, int(rng.integers(0, 10)), 150)
        side_b = draw_side(rng, int(rng.integers(0, 10)), 100)
        got = twin(rule, side_a, side_b)
        for side, w in ((side_a, got["winner"][0]), (side_b, got["winner"][1])):
            status = np.array([api.SCRG_OK if ok else api.SCRG_PAIR_OVER_EDIT_LIMIT for ok in side[3]], dtype=np.uint32)
            best = api.best_per_read(np.array(side[2], dtype=np.int64), status, [0, len(side[2])])
            assert (w if w is not None else -1) == int(best["best_pair"][0]), (trial, side)


def disagreement_case():
    """Side A's lowest-distance candidate (a repeat copy, 1 edit) lies 40 kb from every B candidate; its second lowest (the true
    locus) 300 bp from B's best, forward against B's reverse."""
    side_a = ([60000, 20000, 90000], [0, 0, 1], [1, 3, 9], [True] * 3, 150)
    side_b = ([20150, 130000], [1, 1], [0, 6], [True] * 2, 150)
    return side_a, side_b


def test_best_mode_and_the_paired_rule_disagree(lib):
    side_a, side_b = disagreement_case()
    assert mm.best_of(side_a[2], side_a[3])[0] == 0 and mm.span_of(20000, 150, 20150, 150) == 300
    for penalty, winners, flags in ((2, (1, 0), mm.PROPER | mm.HAS_A | mm.HAS_B), (0, (0, 0), mm.HAS_A | mm.HAS_B)):
        rule = (0, 1000, mm.FR, penalty)
        got = twin(rule, side_a, side_b)
        assert got == mm.choose(rule, side_a, side_b)
        assert got["winner"] == winners and got["flags"] == flags and got["n_proper"] == 1, penalty
    # a three-edit gap between the proper combination and the single bests: penalty 2 is not enough either
    side_a[2][1] = 4
    got = twin((0, 1000, mm.FR, 2), side_a, side_b)
    assert got["winner"] == (0, 0) and not got["flags"] & mm.PROPER and got["cost"] == 1 and got["span"] == 60150 - 20150


@pytest.mark.parametrize("bad", [dict(min_span=2, max_span=1), dict(orientation=4), dict(reserved=(1, 0)), dict(reserved=(0, 7))])
def test_invalid_rules_are_refused_and_nothing_is_written(lib, bad):
    fn = api._lazy(lib, "scrg_mates_from_distances")
    rule = api.MateRule(**bad).as_c()
    start, ed = np.array([5], dtype=np.uint64), np.array([1], dtype=np.int64)
    rec, marks = np.full(32, 0xAB, dtype=np.uint8), np.full(2, 0xCD, dtype=np.uint8)
    st = fn(C.byref(rule), 1, start.ctypes.data, None, ed.ctypes.data, None, 50, 1, start.ctypes.data, None, ed.ctypes.data, None, 50, rec.ctypes.data,
            marks.ctypes.data, marks.ctypes.data + 1)
    assert st == api.SCRG_ERR_INVALID_ARG and set(rec.tolist()) == {0xAB} and set(marks.tolist()) == {0xCD}
    with pytest.raises(scrooge_amd.ScroogeError):
        api.mates_from_distances(api.MateRule(**bad), ([5], None, [1], None, 50), ([5], None, [1], None, 50))


def test_the_default_rule_and_optional_arrays(lib):
    """rule = None is FR with any span and penalty 0; reverse = None is all forward (no FR combination then), status = None all eligible"""
    a, b = ([10, 700], None, [3, 0], None, 100), ([400], None, [2], None, 100)
    rec, best_a, best_b = api.mates_from_distances(None, a, b)
    assert rec["winner"].tolist() == [1, 0] and int(rec["flags"]) == mm.HAS_A | mm.HAS_B and int(rec["n_proper"]) == 0 and int(rec["span"]) == 400
    assert best_a.tolist() == [0, 1] and best_b.tolist() == [1]
    rec, _, _ = api.mates_from_distances(api.MateRule(orientation="ff"), a, b)
    assert rec["winner"].tolist() == [1, 0] and int(rec["flags"]) == mm.PROPER | mm.HAS_A | mm.HAS_B and int(rec["n_proper"]) == 2
    assert int(rec["second_cost"]) == 5 and int(rec["cost"]) == 2


def test_the_twin_refuses_two_to_the_32_combinations(lib):
    n = 1 << 16
    start, ed = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        api.mates_from_distances(None, (start, None, ed, None, 50), (start, None, ed, None, 50))
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    rec, _, _ = api.mates_from_distances(api.MateRule(orientation="any"), (start, None, ed, None, 50), (start[:3], None, ed[:3], None, 50))
    assert int(rec["n_proper"]) == 65535 and rec["winner"].tolist() == [0, 0]


def mates_of(order, cand_offsets):
    read = np.repeat(np.arange(len(cand_offsets) - 1), np.diff(np.asarray(cand_offsets, dtype=np.int64)))
    return read[order] // 2


@pytest.mark.parametrize("sort_by_length", [0, 1])
def test_plan_mates_keeps_mate_pairs_whole(lib, sort_by_length):
    """scrg_host_plan_mates: chunks cover the batch once, no cut falls inside a mate pair, and mates of mixed lengths stay adjacent
    and in the caller's order when the issue order is sorted — by the longer mate's length, stably."""
    rng = np.random.Generator(np.random.PCG64(11))
    nr = 4000
    read_lens = rng.choice([50, 100, 150, 250, 2000], nr)
    counts = rng.integers(0, 40, nr)
    counts[rng.integers(0, nr, 200)] = 0
    counts[100:104] = 3000                                  # mate pairs larger than what a cut would leave whole by chance
    co = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(co[-1])
    order, first = api.host_plan_mates(read_lens, co, sort_by_length=sort_by_length)
    assert sorted(order.tolist()) == list(range(n))
    assert first[0] == 0 and first[-1] == n and np.all(np.diff(first.astype(np.int64)) > 0) and len(first) > 4
    mate = mates_of(order, co)
    for cut in first[1:-1]:
        assert mate[int(cut) - 1] != mate[int(cut)], cut
    # every mate pair is one run of the issue order, in the caller's order
    change = np.flatnonzero(np.diff(mate)) + 1
    runs = np.split(order.astype(np.int64), change)
    assert len({int(mate[int(c)]) for c in np.concatenate([[0], change])}) == len(runs)
    assert all(np.all(np.diff(r) == 1) for r in runs)
    key = np.maximum(read_lens[0::2], read_lens[1::2])
    issued = [int(mate[int(c)]) for c in np.concatenate([[0], change])]
    if sort_by_length:
        assert issued == sorted(issued, key=lambda m: -int(key[m]))            # (sorted() is stable: equal keys keep the caller's order)
        assert len(set(read_lens[0::2] != read_lens[1::2])) == 2
    else:
        assert issued == sorted(issued)
    # the plan of the call without mates cuts differently somewhere: the cuts above are the paired call's own
    plain_order, _ = api.host_plan_mapping(read_lens, co, sort_by_length=sort_by_length, best=True)
    assert sort_by_length == 0 or not np.array_equal(plain_order, order)


def test_plan_mates_refuses_an_odd_number_of_reads(lib):
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        api.host_plan_mates([100, 100, 100], [0, 1, 2, 3])
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    order, first = api.host_plan_mates([], [0])
    assert len(order) == 0 and first.tolist() == [0]
