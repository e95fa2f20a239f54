"""The batch and the placements of tests/big_offsets.py, checked on the CPU: what tests/test_big_offsets_gpu.py relies on when it
says that a truncated or wrapped address cannot pass by luck."""
import numpy as np
import pytest

from tests import big_offsets as bo
from tests import plane_inputs as pi

SETTINGS = pi.MAPPING_SETTINGS + [(128, 65)]
T31, T32 = bo.T31, bo.T32


@pytest.fixture(scope="module")
def answers(oracle):
    """(W, O) -> (edit distances, CIGARs) of the batch, exact texts."""
    b = bo.batch()
    return {s: oracle.align(b.texts, b.reads, W=s[0], O=s[1], threads=8)[:2] for s in SETTINGS}


def test_batch_shape(answers):
    b = bo.batch()
    assert 90 <= b.n <= 120
    for g in ("related", "unrelated", "low_complexity", "long_gap", "degenerate", "lattice", "short_text", "short_related", "long_noisy"):
        assert g in b.groups
    assert b.n // 3 - 1 <= sum(b.read_rc) <= b.n // 3 + 1 and b.n // 3 - 2 <= sum(b.text_rc) <= b.n // 3 + 2
    assert any(r and t for r, t in zip(b.read_rc, b.text_rc)) and any(r and not t for r, t in zip(b.read_rc, b.text_rc))
    assert any(not b.texts[k] for k in range(b.n)) and any(not b.reads[k] for k in range(b.n))
    assert any(len(b.reads[k]) > len(b.texts[k]) + 200 for k in range(b.n))            # a read that outlasts its text
    n_runs = [len(pi.cigar_runs(c)) for c in answers[(64, 33)][1]]
    bands = bo.run_bands(n_runs)
    assert min(bands) >= 3, bands              # on both sides of 16 and of 24, and beyond one tile of 512
    assert 16 in n_runs or (max(x for x in n_runs if x <= 16) >= 10 and min(x for x in n_runs if x > 16) <= 24)
    for k in range(b.n):
        assert len(b.tails[k]) % 32 == 0 and len(b.ext(k)) >= 2 * (4 * len(b.reads[k]) + 4 * bo.W_MAX)
        assert b.cap(k) % 16 == 0 and b.cap(k) >= 2 * len(b.reads[k]) + 16


@pytest.mark.parametrize("W,O", SETTINGS)
def test_the_oracle_cut_is_long_enough(oracle, answers, W, O):
    """The text declared as mapping declares it is endless; the oracle gets K = 4 read_len + 4 W characters.  K and 2 K give
    the same answer, and the alignment ends W characters before the cut."""
    b = bo.batch()
    e1, c1 = oracle.align([b.cut(k, W) for k in range(b.n)], b.reads, W=W, O=O, threads=8)[:2]
    e2, c2 = oracle.align([b.cut(k, W, 2) for k in range(b.n)], b.reads, W=W, O=O, threads=8)[:2]
    assert (e1, c1) == (e2, c2)
    for k in range(b.n):
        text_end = sum(n for n, op in pi.cigar_runs(c1[k]) if op in "=XD")
        assert text_end + W <= 4 * len(b.reads[k]) + 4 * W, k
    # (and the tail changes the answer of the pairs whose text ends early: the two declarations are two cases)
    assert sum(1 for k in range(b.n) if c1[k] != answers[(W, O)][1][k]) >= 5


@pytest.mark.parametrize("swept", ["text", "read"])
def test_sequence_placement(swept):
    b = bo.batch()
    P = bo.place_sequences(swept)                # (Image.write asserts that no two objects overlap)
    other = "read" if swept == "text" else "text"
    for T in bo.THRESHOLDS:
        cats = [P.category(swept, k, T) for k in range(b.n)]
        assert cats.count(-1) >= 1 and cats.count(0) == 1 and cats.count(1) >= b.n // 2, (T, cats)
        k = cats.index(0)
        lo, hi = P.used_extent(swept, k)
        assert lo + 1000 < T < hi - 1000         # really on both sides
        assert all(P.category(other, k, T) == 1 for k in range(b.n))
    assert sum(1 for k in range(b.n) if P.category(swept, k, T31) == 1 and P.category(swept, k, T32) == -1) >= 2
    rc = b.text_rc if swept == "text" else b.read_rc
    strands = {rc[[P.category(swept, k, T) for k in range(b.n)].index(0)] for T in bo.THRESHOLDS}
    assert strands == {False, True}              # one straddler of each strand
    for kind in ("text", "read"):
        res = {P.extent(kind, k)[0] % 32 for k in range(b.n)}
        assert len(res) >= 8 and {0, 31} <= res, res
        assert max(P.extent(kind, k)[1] for k in range(b.n)) <= bo.TOP
    assert max(P.extent(other, k)[1] for k in range(b.n)) == bo.TOP          # the highest object ends with the buffer
    assert max(P.extent(other, k)[0] for k in range(b.n)) > T32 + (1 << 28) - (1 << 17)
    for declare in ("exact", "mapping"):
        d = P.desc(declare)
        for k, (to, tl, ro, rl) in enumerate(d):
            assert (to >> 63) == b.text_rc[k] and (ro >> 63) == b.read_rc[k] and rl == len(b.reads[k])
            to &= bo.FLAG - 1
            assert to + tl <= bo.TOP
            m = min(tl, 1 << 16)
            got = P.image.read(to, m) if not b.text_rc[k] else bo.revcomp(P.image.read(to + tl - m, m))
            want = b.texts[k] if declare == "exact" else b.ext(k)
            assert got[: len(want)] == want[: 1 << 16] and (declare == "mapping" or tl == len(want)), (declare, k)
            stored = P.image.read(ro & (bo.FLAG - 1), rl)
            assert (bo.revcomp(stored) if b.read_rc[k] else stored) == b.reads[k]
    lens = [tl for _, tl, _, _ in P.desc("mapping")]
    fwd = [tl for k, tl in enumerate(lens) if not b.text_rc[k]]
    rev = [tl for k, tl in enumerate(lens) if b.text_rc[k]]
    if swept == "text":                          # lengths past 2^31 and past 2^32 - 1 on both strands, and below them
        for ls in (fwd, rev):
            assert any(x > T32 - 1 for x in ls) and any(T31 < x <= T32 - 1 for x in ls)
        assert any(x < T31 for x in fwd) and any(x < T31 for x in rev)
    assert len(P.image.pages) * bo.PAGE <= 64 << 20
    assert bo.plan_bytes(bo.seq_words() * 8) < 2 << 30


@pytest.mark.parametrize("swept", ["text", "read"])
def test_grouped_placement(swept):
    b = bo.batch()
    P = bo.place_groups(swept)
    other = "read" if swept == "text" else "text"
    spans = sorted(P.words(x) for x in P.blocks)
    assert all(e <= a for (_, e), (a, _) in zip(spans, spans[1:])) and spans[-1][1] + 2 * 64 + 2 <= bo.seq_words(64)
    assert all(len(rows) <= 64 for _, _, rows in P.blocks) and {base % 64 for base, _, _ in P.blocks} != {0}
    for T in bo.THRESHOLDS:
        cats = [P.category(swept, k, T) for k in range(b.n)]
        assert cats.count(-1) >= 1 and cats.count(0) >= 1 and cats.count(1) >= b.n // 2, (T, cats)
        assert any(c == 0 and lo + 32000 < T < hi - 32000 for c, (lo, hi) in zip(cats, (P.used_extent(swept, k) for k in range(b.n))))
        assert all(P.category(other, k, T) == 1 for k in range(b.n))
    # a decoy block wherever a block's base less 2^31 / 32 or 2^32 / 32 is not negative, the straddlers' included
    assert len(P.decoys) == sum(1 for blk in P.blocks for T in bo.THRESHOLDS if blk[0] >= T // 32) >= len(P.blocks)
    assert all(base >= 0 for base, _, _ in P.decoys)
    # read_words gives back what the blocks hold (the true blocks are written last)
    for kind, k in (("text", 0), ("read", b.n - 1), (swept, bo._straddlers(b, swept)[1])):
        at = (P.text_at if kind == "text" else P.read_at)[k]
        s_ = P.stored(kind, k)
        assert P.read_words(at // 32, (len(s_) + 31) // 32)[: len(s_)] == s_
    # what the descriptors name is what the rows hold: word w of an object at word (off / 32) + 64 w
    where = {}
    for blk in P.blocks:
        a = P.rows_of(blk)
        for r, (kind, k) in enumerate(blk[2]):
            where[(kind, k)] = (blk[0] + r, a[r])
    for declare in ("exact", "mapping"):
        for k, (to, tl, ro, rl) in enumerate(P.desc(declare)):
            assert (to >> 63) == b.text_rc[k] and (ro >> 63) == b.read_rc[k]
            to, ro = to & (bo.FLAG - 1), ro & (bo.FLAG - 1)
            assert to % 32 == 0 and ro % 32 == 0
            first, row = where[("text", k)]
            w0 = (to // 32 - first) // 64
            assert (to // 32 - first) % 64 == 0 and w0 >= 0
            got = row[32 * w0: 32 * w0 + tl].tobytes()
            want = b.texts[k] if declare == "exact" else b.ext(k)
            assert (bo.revcomp(got) if b.text_rc[k] else got) == want, (declare, k)
            first, row = where[("read", k)]
            assert ro // 32 == first and rl == len(b.reads[k])
            got = row[:rl].tobytes()
            assert (bo.revcomp(got) if b.read_rc[k] else got) == b.reads[k]
    assert sum(a.size for a in map(P.rows_of, P.blocks)) + sum(d[2].size for d in P.decoys) <= 256 << 20


@pytest.mark.parametrize("W,O", [(64, 33), (129, 65)])
@pytest.mark.parametrize("swept", ["text", "read"])
@pytest.mark.parametrize("layout", ["linear", "groups"])
def test_decoys_give_other_answers(oracle, layout, swept, W, O):
    """Where an address that lost 2^31 or 2^32 would land lie other bases, and the oracle's answer on them is another one:
    for every pair with something to align, each quantity and each threshold, in both layouts."""
    b = bo.batch()
    P = bo.place_sequences(swept) if layout == "linear" else bo.place_groups(swept)
    decoy_pair = bo.decoy_pair if layout == "linear" else bo.decoy_pair_groups
    e0, c0 = oracle.align([b.cut(k, W) for k in range(b.n)], b.reads, W=W, O=O, threads=8)[:2]
    checked = 0
    for kind in ("text", "read"):
        for T in bo.THRESHOLDS:
            ks, tx, rd = [], [], []
            for k in range(b.n):
                d = decoy_pair(P, k, kind, T, W)
                if d is not None and len(b.reads[k]) >= 8:
                    ks.append(k), tx.append(d[0]), rd.append(d[1])
            e, c = oracle.align(tx, rd, W=W, O=O, threads=8)[:2]
            same = [k for j, k in enumerate(ks) if (e[j], c[j]) == (e0[k], c0[k])]
            assert not same, (kind, T, same)
            checked += len(ks)
            assert len(ks) >= (b.n // 2 if T == T32 or kind != swept else b.n * 2 // 3), (kind, T, len(ks))
    assert checked >= (3 * b.n if layout == "linear" else 5 * b.n // 2)      # (groups: a straddler's block mates have no place below 0 either)


@pytest.mark.parametrize("level", [31, 32])
def test_slice_placement(level, answers):
    b = bo.batch()
    caps = [b.cap(k) for k in range(b.n)]
    n_runs = [len(pi.cigar_runs(c)) for c in answers[(64, 33)][1]]
    S = bo.place_slices(caps, n_runs, level)
    assert all(o % 16 == 0 and c % 16 == 0 for o, c in zip(S.off, S.cap))
    assert {(o // 16) % 2 for o in S.off} == {0, 1}
    spans = sorted(zip(S.off, S.cap))
    assert all(a + c <= nxt for (a, c), (nxt, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= S.size
    for T in bo.THRESHOLDS[: level - 30]:
        cats = [S.category(k, T, n_runs[k]) for k in range(b.n)]
        assert cats.count(-1) >= 1 and cats.count(0) == 1 and cats.count(1) >= b.n // 2
        k = cats.index(0)
        assert S.off[k] + 200 < T < S.off[k] + n_runs[k] - 200 and n_runs[k] > 512
    # sentinels: inside the buffer, clear of every slice, and covering every wrapped slice outside the true ones
    for lo, n in S.sentinels:
        assert 0 <= lo and lo + n <= S.size and n > 0
        assert all(lo + n <= a or a + c <= lo for a, c in spans)
    covered = sum(n for _, n in S.sentinels)
    assert covered >= sum(c for o, c in zip(S.off, S.cap) if o >= T31) // 2
    assert bo.plan_bytes(2 * S.size, 2 * S.size, bo.seq_words() * 8) <= bo.MEMORY_CAP      # arena, dense runs, sequences


# ------------------------------------------------------------------------------------------------ the models and their host twins
def test_models_and_host_twins_on_the_batch(answers):
    """The models the GPU tests hold the side passes to, on this batch's runs, against the library's host functions called on
    the same runs: difference strings, report, clip record and the three CIGAR forms of every pair."""
    from scrooge_amd import api
    from tests import cigar_form_model as fm, clip_model as cm, diff_model as dm, report_model as rm
    b = bo.batch()
    eds, cigars = answers[(64, 33)]
    verdicts = set()
    for k in range(b.n):
        runs = pi.cigar_runs(cigars[k])
        for kind in ("md", "cs"):
            assert api.diff_from_runs(kind, b.texts[k], b.reads[k], runs) == dm.model(kind, b.texts[k], b.reads[k], runs), (kind, k)
        rep = rm.model(b.texts[k], b.reads[k], runs, eds[k])
        assert api.report_from_runs(b.texts[k], b.reads[k], runs, eds[k]) == rep, k
        verdicts.add(rep["verdict"])
        assert api.clip_from_runs(runs) == cm.model(runs), k
        for form in ("windowed", "merged", "m"):
            assert api.cigar_from_runs(form, runs) == fm.model(form, runs), (form, k)
        # the forward view the diff kernels get of a reversed text: the stored stretch
        if b.text_rc[k] and runs:
            assert api.diff_from_runs("cs", bo.revcomp(b.texts[k]), b.reads[k], runs) == dm.model("cs", bo.revcomp(b.texts[k]), b.reads[k], runs)
    assert verdicts == {0}


def test_pileup_twin_with_starts_past_the_thresholds(answers):
    """scrg_pileup_from_runs against pileup_model with target_start inside the target and moved up by 2^31, 2^32 and both:
    nothing lands, every alignment with runs is out of range."""
    from scrooge_amd import api
    from tests import pileup_model as pm
    b = bo.batch()
    L = 4096
    cigars = answers[(64, 33)][1]
    for shift in (0, T31, T32, T32 + T31, (1 << 63) - 5000):
        got, want, n_out, m_out = pm.empty(L), pm.empty(L), 0, 0
        for k in range(b.n):
            runs = pi.cigar_runs(cigars[k])
            if not runs:
                continue
            start = (131 * k) % 3900 + shift
            n_out += api.pileup_from_runs(runs, b.reads[k], start, L, counts=got)[1]
            m_out += pm.model(runs, b.reads[k], start, L, counts=want)[1]
        assert got.tobytes() == want.tobytes() and n_out == m_out, shift
        assert (want.any() and 0 < m_out < b.n) if shift == 0 else (not want.any() and m_out == sum(1 for c in cigars if c)), shift


def test_mates_twin_with_starts_past_the_thresholds():
    """scrg_mates_from_distances against mate_model with every start raised past 2^31 and 2^32, with mates on either side of a
    threshold, and with spans that exceed 32 bits: the record saturates the span, the rule compares it in 64 bits."""
    from scrooge_amd import api
    from tests import mate_model as mm
    from tests.test_mates_gpu import draw_mate
    rng = np.random.Generator(np.random.PCG64(6464))
    mates = [draw_mate(rng, int(a), int(c), 0) for a, c in rng.integers(0, 6, (60, 2))]
    rules = [(200, 900, mm.FR, 1), (0, 2 ** 64 - 1, mm.ANY, 0), (T31, T32 + (1 << 20), mm.ANY, 0)]

    def both(sides, rule):
        model = mm.choose(rule, *[(s["start"], s["rev"], s["ed"], [x != 2 for x in s["status"]], s["len"]) for s in sides])
        rec, best_a, best_b = api.mates_from_distances(api.MateRule(*rule), *[(s["start"], s["rev"], s["ed"], [7 if x == 2 else 0 for x in s["status"]],
                                                                             s["len"]) for s in sides])
        win = tuple(api.MATES_NONE if w is None else w for w in model["winner"])
        assert (tuple(int(x) for x in rec["winner"]), int(rec["cost"]), int(rec["second_cost"]), int(rec["span"]), int(rec["n_proper"]), int(rec["flags"])) == \
            (win, model["cost"], model["second_cost"], model["span"], model["n_proper"], model["flags"]), (rule, sides)
        assert best_a.tolist() == model["is_best_a"] and best_b.tolist() == model["is_best_b"]
        return model

    for rule in rules:
        base = [both(m, rule) for m in mates]
        for shift in (T31 + 12345, T32 + 12345, T31 - 1000, T32 - 1000):
            moved = [[dict(s, start=[x + shift for x in s["start"]]) for s in m] for m in mates]
            assert [both(m, rule) for m in moved] == base, (rule, shift)
    far = [[dict(m[0]), dict(m[1], start=[x + T32 + 12345 for x in m[1]["start"]])] for m in mates]
    assert any(both(m, rules[1])["span"] == mm.NONE32 for m in far)
    assert sum(1 for m in far if both(m, rules[2])["flags"] & mm.PROPER) > 5 and not any(both(m, rules[0])["flags"] & mm.PROPER for m in far)
