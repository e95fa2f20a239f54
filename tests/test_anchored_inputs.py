"""The inputs of the host-layer tests of directed and anchored alignment (tests/anchored_inputs.py) meet the conditions that keep
those tests from passing for the wrong reason — no GPU involved: how a call with these lengths is cut (scrg_host_plan_mapping),
which halves of an anchor land in which chunk, the shares of strands and directions, the special positions, and that the
oracle aligned every pair."""
import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from tests import anchored_inputs as ai

# every window setting the GPU tests use (tests/test_anchored_host_gpu.py)
DIRECTED_SETTINGS = [(64, 33), (16, 0), (64, 2), (128, 65), (64, 0), (192, 97), (256, 129), (256, 1)]
ANCHORED_SETTINGS = [(64, 33), (128, 65), (192, 97), (256, 1)]


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return api.load_library()


def chunk_of(n, order, first):
    """-> int64 [n]: the chunk each pair of the call lands in."""
    at = np.empty(n, dtype=np.int64)
    at[order] = np.arange(n)
    return np.searchsorted(first, at, side="right") - 1


@pytest.mark.parametrize("W,O", DIRECTED_SETTINGS)
def test_directed_set_meets_its_conditions(lib, oracle, W, O):
    d = ai.directed_inputs(oracle, W, O)
    G, offs = ai.GENOME_LEN, d["offs"]
    n, nr = int(offs[-1]), len(d["reads"])
    assert len(d["genome"]) == G == 70_001 and G % 32 == 17
    assert nr == ai.DIRECTED_READS + ai.DIRECTED_LONG and n >= ai.MIN_DIRECTED_CANDIDATES
    lens = [len(x) for x in d["reads"]]
    assert set(len(c) for c in d["cands"][:ai.DIRECTED_READS]) == {1, 2, 3, 4}
    assert lens[0] == 0 and lens[1] == 1 and max(lens[:ai.DIRECTED_READS]) <= 500
    assert sum(1 < x < 16 for x in lens) >= 50                                    # shorter than any window used
    assert all(3_000 <= x <= 8_000 for x in lens[ai.DIRECTED_READS:]) and nr - ai.DIRECTED_READS == 24
    pos = np.array([p for c in d["cands"] for p in c])
    rev = np.array([x for c in d["rev"] for x in c])
    left = np.array([x for c in d["left"] for x in c])
    rlen = np.repeat(lens, np.diff(offs))
    assert pos.min() == 0 and pos.max() == G and (pos > 65_535).sum() >= 50
    # the shares of the four (reverse, leftward) combinations, and the special positions in both directions
    for rv in (0, 1):
        for lw in (0, 1):
            assert ((rev == rv) & (left == lw)).sum() >= ai.MIN_SHARE * n, (rv, lw)
    for p in ai.special_positions(W):
        for lw in (0, 1):
            assert ((pos == p) & (left == lw)).any(), (p, lw)
    assert ((left == 1) & (pos < rlen)).any()                                     # a leftward text shorter than its read
    assert ((left == 0) & (pos < G) & (G - pos < rlen)).any()                     # a rightward one: the genome ends first
    # a read's first candidate is its true location: few edits, where a random location has about half the read's length (asked
    # where windows overlap by half: with less overlap no later window corrects a window's choice, and on reads with ten per
    # cent of edits even a true location's distance is large)
    first = offs[:-1]
    eds = np.array(d["eds"])
    big = np.array(lens) >= 100
    if 2 * O >= W:
        assert (eds[first][big] < 0.25 * np.array(lens)[big]).all()
    assert left[first].sum() >= 0.4 * nr and (1 - left[first]).sum() >= 0.4 * nr
    # the oracle aligned every pair: a distance, and a CIGAR that spends the whole read
    assert len(d["eds"]) == len(d["cigars"]) == n and (eds >= 0).all()
    assert [ai.read_used(c) for c in d["cigars"]] == d["read_len"] == rlen.tolist()
    # the call is cut into several chunks, not in the caller's order, and a read's candidates lie on both sides of a cut
    order, chunk_first = api.host_plan_mapping(lens, offs)
    assert len(chunk_first) - 1 >= ai.MIN_CHUNKS
    assert sorted(order.tolist()) == list(range(n)) and order.tolist() != list(range(n))
    chunk = chunk_of(n, order, chunk_first)
    assert any(len(set(chunk[int(a): int(b)])) > 1 for a, b in zip(offs, offs[1:]))
    # best-candidate mode keeps a read's candidates together, and still cuts the call
    best_order, best_first = api.host_plan_mapping(lens, offs, best=True)
    assert len(best_first) - 1 >= ai.MIN_CHUNKS
    best_chunk = chunk_of(n, best_order, best_first)
    assert all(len(set(best_chunk[int(a): int(b)])) <= 1 for a, b in zip(offs, offs[1:]))
    cut = sum(len(set(chunk[int(a): int(b)])) > 1 for a, b in zip(offs, offs[1:]))
    print("W=%d O=%d: %d candidates in %d chunks (%d in best-candidate mode), reads cut in two: %d" % (W, O, n, len(chunk_first) - 1, len(best_first) - 1, cut))


@pytest.mark.parametrize("W,O", ANCHORED_SETTINGS)
def test_anchored_set_meets_its_conditions(lib, oracle, W, O):
    a = ai.anchored_inputs(oracle, W, O)
    G, offs = ai.GENOME_LEN, a["offs"]
    n, nr = int(offs[-1]), len(a["reads"])
    assert nr == ai.ANCHORED_READS + ai.ANCHORED_LONG and n >= ai.MIN_ANCHORS
    assert set(len(x) for x in a["anchors"][:ai.ANCHORED_READS]) == {1, 2, 3}
    lens = [len(x) for x in a["reads"]]
    for r in range(ai.ANCHORED_READS, nr):
        (ga, ra), = a["anchors"][r]
        assert 4_000 <= lens[r] <= 9_000 and lens[r] // 3 <= ra <= 2 * lens[r] // 3 + 1
    assert all(a["rev"][r][0] == (r % 3 == 0) for r in range(nr))
    flat = [x for y in a["anchors"] for x in y]
    L = np.repeat(lens, np.diff(offs))
    ga, ra = np.array([x[0] for x in flat]), np.array([x[1] for x in flat])
    seed = np.array([k == "seed" for k in a["kinds"]])
    for what in ((ra == 0), (ra == L) & (L > 0), (ga == 0), (ga == G)):           # the edge cases, among the true seeds
        assert (what & seed).sum() >= 20
    assert a["kinds"].count("second seed") >= 50 and a["kinds"].count("wrong") >= 300
    assert all(k == "seed" for k in np.array(a["kinds"])[offs[:-1]])
    # a seed's 12 bases are the genome's: the joined alignment of a true anchor has few edits, a wrong one has many
    ed = np.array(a["ed"])
    true = np.array([k != "wrong" for k in a["kinds"]]) & (L >= 100)
    if 2 * O >= W:                                            # (with less overlap even a true location's distance is large)
        assert (ed[true] < 0.25 * L[true]).all() and (ed[~true & (L >= 100)] > 0.25 * L[~true & (L >= 100)]).mean() > 0.9
    for q in np.flatnonzero(np.array([k == "second seed" for k in a["kinds"]]) | (seed & (ga < G) & (ra < L))):
        nm, g, x = a["named"][q], int(ga[q]), int(ra[q])
        assert nm[x: x + ai.SEED_BASES] == a["genome"][g: g + ai.SEED_BASES], q
    # the oracle aligned every half
    assert len(a["half_eds"]) == 2 * n and min(a["half_eds"]) >= 0
    assert [ai.read_used(c) for c in a["half_cigars"]] == [h[0] for h in a["half_len"]] + [h[1] for h in a["half_len"]]
    assert [ai.read_used(c) for c in a["cigars"]] == L.tolist()
    assert all(0 <= s and s + u <= G for s, u in zip(a["text_start"], a["text_used"]))
    # the call as the library sees it: 2 n one-candidate reads, the halves of anchor q being reads 2 q and 2 q + 1
    half = np.array(a["half_len"]).reshape(-1)
    order, chunk_first = api.host_plan_mapping(half, np.arange(2 * n + 1))
    assert len(chunk_first) - 1 >= ai.MIN_CHUNKS
    assert sorted(order.tolist()) == list(range(2 * n)) and order.tolist() != list(range(2 * n))
    chunk = chunk_of(2 * n, order, chunk_first)
    split = int((chunk[0::2] != chunk[1::2]).sum())
    assert split >= ai.MIN_SPLIT_ANCHORS and n - split >= ai.MIN_UNSPLIT_ANCHORS, (split, n - split)
    print("W=%d O=%d: %d anchors in %d chunks, halves in different chunks: %d, in the same: %d" % (W, O, n, len(chunk_first) - 1, split, n - split))
