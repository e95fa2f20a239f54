"""The read summary and MAPQ rule without a GPU: the header's worked values, scrg_read_summary_from_distances against the plain
Python model (tests/mapq_model.py) and against api.best_per_read on drawn inputs of every class, the statuses' copy, the refusal of
every invalid rule field, and the merge of partial summaries held associative and commutative."""
import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from tests import mapq_model as mq

OVER = api.SCRG_PAIR_OVER_EDIT_LIMIT
NOT_BEST = api.SCRG_PAIR_NOT_BEST


def test_constants_and_layout():
    assert api.read_summary_dtype().itemsize == 32
    assert (api.SCRG_MAPQ_HAS_WINNER, api.SCRG_MAPQ_TIED, api.SCRG_MAPQ_HAS_SECOND, api.SCRG_MAPQ_KEPT) == (mq.HAS_WINNER, mq.TIED, mq.HAS_SECOND, mq.KEPT)
    assert api.MAPQ_NONE == mq.NONE and api.MAPQ_NO_ED == mq.NO_ED
    r = api.MapqRule()
    assert (r.per_edit, r.max_q, r.zero_per_mille, r.min_keep_q, r.reserved) == mq.DEFAULT_RULE + (0,)
    import ctypes as C
    assert C.sizeof(api._MapqRuleC) == 16 and scrooge_amd.MapqRule is api.MapqRule


# L, best_ed, second_ed (None: no second), q — the header's table, at the defaults
WORKED = [(150, 0, None, 60), (150, 0, 1, 10), (150, 3, 5, 20), (150, 38, None, 0), (150, 38, 39, 0), (150, 38, 4000, 0), (10000, 1000, None, 36)]


@pytest.mark.parametrize("L,best,second,q", WORKED)
def test_worked_values(L, best, second, q):
    assert mq.mapq(mq.DEFAULT_RULE, L, True, 1, best, second) == q
    eds = [best] if second is None else [second, best]
    got = api.read_summary_from_distances(None, [0, len(eds)], [L] * len(eds), eds)[0]
    assert int(got["mapq"]) == q and int(got["best_ed"]) == best and int(got["winner"]) == len(eds) - 1
    assert int(got["second_ed"]) == (mq.NO_ED if second is None else second)
    if (L, best, second) == (150, 3, 5):
        assert mq.mapq(mq.DEFAULT_RULE, L, True, 1, best, None) == 56          # its cap


def test_a_tie_and_no_winner_are_zero():
    got = api.read_summary_from_distances(None, [0, 2, 2, 3], [150] * 3, [4, 4, 0], [0, 0, OVER])
    assert [mq.as_tuple(g) for g in got] == [(0, 4, mq.NO_ED, 2, 2, 2, 0, mq.HAS_WINNER | mq.TIED | mq.KEPT),
                                             (mq.NONE, mq.NO_ED, mq.NO_ED, 0, 0, 0, 0, 0), (mq.NONE, mq.NO_ED, mq.NO_ED, 0, 0, 1, 0, 0)]
    assert [int(g["reserved"]) for g in got] == [0, 0, 0]


RULES = [mq.DEFAULT_RULE, (0, 60, 250, 1), (10, 0, 250, 0), (255, 254, 1000, 254), (3, 40, 1, 7), (10, 60, 250, 60), (1, 254, 37, 100)]


def draw_batch(rng, n_reads=400):
    """Reads of every class; -> first, read_len, ed, status (a result's codes), classes seen."""
    first, read_len, ed, status, seen = [0], [], [], [], set()
    for r in range(n_reads):
        kind = ("none", "all_over", "unique", "unique_second", "tie", "tie_second", "huge", "len0", "mixed")[r % 9 if r < 18 else int(rng.integers(0, 9))]
        L = 0 if kind == "len0" else int(rng.choice([1, 36, 150, 151, 10000, 2 ** 31 - 1]))
        if kind == "none":
            eds, sts = [], []
        elif kind == "all_over":
            n = int(rng.integers(1, 5))
            eds, sts = [int(x) for x in rng.integers(0, 50, n)], [OVER] * n
        elif kind == "unique":
            eds, sts = [int(rng.integers(0, 60))], [0]
            if rng.integers(0, 2):                       # a better candidate that is over the limit does not count
                eds, sts = [0] + eds, [OVER, 0]
        elif kind == "unique_second":
            b = int(rng.integers(0, 40))
            eds = [b + int(x) for x in rng.integers(1, 9, int(rng.integers(1, 6)))] + [b]
            eds = [eds[i] for i in rng.permutation(len(eds))]
            sts = [int(rng.choice([0, NOT_BEST, api.SCRG_ERR_CIGAR_OVERFLOW])) for _ in eds]
        elif kind in ("tie", "tie_second"):
            b = int(rng.integers(0, 40))
            eds = [b] * int(rng.integers(2, 5)) + ([b + int(rng.integers(1, 4))] if kind == "tie_second" else [])
            eds = [eds[i] for i in rng.permutation(len(eds))]
            sts = [0] * len(eds)
        elif kind == "huge":                              # distances near 2^32 - 2: counted in 32 bits, no overflow in the MAPQ
            eds = [2 ** 32 - 2 - int(x) for x in rng.integers(0, 3, int(rng.integers(1, 4)))]
            sts = [0] * len(eds)
        elif kind == "len0":
            eds = [int(x) for x in rng.integers(0, 3, int(rng.integers(1, 4)))]
            sts = [0] * len(eds)
        else:
            n = int(rng.integers(1, 40))
            eds = [int(x) for x in rng.integers(0, 12, n)]
            sts = [int(rng.choice([0, 0, 0, OVER, NOT_BEST])) for _ in eds]
        seen.add(kind)
        ed += eds
        status += sts
        read_len += [L] * len(eds)
        first.append(len(ed))
    return first, read_len, ed, status, seen


@pytest.mark.parametrize("rule", RULES)
def test_host_twin_against_the_model(rule):
    rng = np.random.Generator(np.random.PCG64(sum(rule)))
    first, read_len, ed, status, seen = draw_batch(rng)
    assert seen == {"none", "all_over", "unique", "unique_second", "tie", "tie_second", "huge", "len0", "mixed"}
    want = mq.summarise_all(rule, first, read_len, ed, [s != OVER for s in status])
    got, keep = api.read_summary_from_distances(api.MapqRule(*rule), first, read_len, ed, status, keep=True)
    assert [mq.as_tuple(g) for g in got] == [mq.as_tuple(w) for w in want]
    assert not got["reserved"].any()
    # every class did occur in what was drawn
    flags = got["flags"]
    assert ((got["n_candidates"] == 0).any() and ((got["n_candidates"] > 0) & (got["n_eligible"] == 0)).any() and (flags & mq.TIED).any()
            and ((flags & (mq.HAS_WINNER | mq.HAS_SECOND | mq.TIED)) == mq.HAS_WINNER).any()
            and ((flags & (mq.HAS_SECOND | mq.TIED)) == mq.HAS_SECOND).any() and (got["best_ed"][(flags & 1) == 1] >= 2 ** 32 - 4).any())
    # winner, best_ed, n_tied and second_ed are api.best_per_read's on the same arrays
    per = api.best_per_read(ed, status, first)
    assert np.array_equal(per["best_pair"], np.where(got["winner"] == mq.NONE, -1, got["winner"].astype(np.int64)))
    assert np.array_equal(per["best_ed"], np.where(flags & 1, got["best_ed"].astype(np.int64), -1))
    assert np.array_equal(per["n_tied"], got["n_tied"].astype(np.int64))
    assert np.array_equal(per["second_ed"], np.where(flags & mq.HAS_SECOND, got["second_ed"].astype(np.int64), -1))
    # the statuses' copy
    assert keep.tolist() == mq.keep_status(want, first, status, 0, NOT_BEST)
    # without statuses everything is eligible
    bare = api.read_summary_from_distances(api.MapqRule(*rule), first, read_len, ed)
    assert [mq.as_tuple(g) for g in bare] == [mq.as_tuple(w) for w in mq.summarise_all(rule, first, read_len, ed, [True] * len(ed))]


@pytest.mark.parametrize("min_keep_q", [0, 1, 60])
def test_keep_status_at_the_thresholds(min_keep_q):
    rule = (10, 60, 250, min_keep_q)
    rng = np.random.Generator(np.random.PCG64(77))
    first, read_len, ed, status, _ = draw_batch(rng, 200)
    want = mq.summarise_all(rule, first, read_len, ed, [s != OVER for s in status])
    got, keep = api.read_summary_from_distances(api.MapqRule(*rule), first, read_len, ed, status, keep=True)
    assert keep.tolist() == mq.keep_status(want, first, status, 0, NOT_BEST)
    kept = [bool(w["flags"] & mq.KEPT) for w in want]
    assert [bool(f & mq.KEPT) for f in got["flags"]] == kept
    n_done_kept = sum(1 for w in want if w["flags"] & mq.KEPT and status[w["winner"]] == 0)
    assert int((keep == 0).sum()) == n_done_kept
    if min_keep_q == 0:
        assert all(k == bool(w["flags"] & mq.HAS_WINNER) for k, w in zip(kept, want))
    else:
        assert any(kept) and not all(k for k, w in zip(kept, want) if w["flags"] & mq.HAS_WINNER)


@pytest.mark.parametrize("rule", [(256, 60, 250, 0, 0), (10, 255, 250, 0, 0), (10, 60, 0, 0, 0), (10, 60, 1001, 0, 0), (10, 60, 250, 255, 0), (10, 60, 250, 0, 1),
                                  (2 ** 32 - 1, 60, 250, 0, 0), (10, 2 ** 32 - 1, 250, 0, 0), (10, 60, 65535, 0, 0), (10, 60, 250, 65535, 0)])
def test_every_invalid_rule_field_is_refused(rule):
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        api.read_summary_from_distances(api.MapqRule(*rule), [0, 1], [100], [0])
    assert e.value.status == api.SCRG_ERR_INVALID_ARG


def test_the_edges_of_the_valid_ranges_pass():
    for rule in ((0, 0, 1, 0, 0), (255, 254, 1000, 254, 0)):
        api.read_summary_from_distances(api.MapqRule(*rule), [0, 1], [100], [0])
    with pytest.raises(scrooge_amd.ScroogeError):
        api.read_summary_from_distances(None, [0, 2, 1], [100, 100], [0, 0])            # offsets that run backwards


def part_of(eds, first=0):
    """The partial summary of eligible candidates `eds` at pair indices first ..: a left fold of single-candidate parts."""
    part = (mq.NONE, 0, mq.NO_ED, 0)
    for c, e in enumerate(eds):
        part = api.read_summary_merge(part, ((e << 32) | (first + c), 1, mq.NO_ED, 1))
    return part


def test_the_merge_is_associative_and_commutative():
    rng = np.random.Generator(np.random.PCG64(5))
    for trial in range(80):
        n = int(rng.integers(0, 10))
        hi = int(rng.choice([2, 4, 50]))
        eds = [int(x) for x in rng.integers(0, hi, n)] if trial % 7 else [2 ** 32 - 2 - int(x) for x in rng.integers(0, 2, n)]
        whole = part_of(eds)
        s = mq.summarise(mq.DEFAULT_RULE, 100, eds, [True] * n)
        want = (mq.NONE, 0, mq.NO_ED, 0) if not n else ((s["best_ed"] << 32) | s["winner"], s["n_tied"], s["second_ed"], n)
        assert whole == want, eds
        # split at every point, and at every pair of points: the parts merge to the whole in any order and any grouping
        for i in range(n + 1):
            a, b = part_of(eds[:i]), part_of(eds[i:], i)
            assert api.read_summary_merge(a, b) == whole == api.read_summary_merge(b, a), (eds, i)
            for j in range(i, n + 1):
                x, y, z = part_of(eds[:i]), part_of(eds[i:j], i), part_of(eds[j:], j)
                m = api.read_summary_merge
                assert m(m(x, y), z) == m(x, m(y, z)) == m(m(z, x), y) == whole, (eds, i, j)
