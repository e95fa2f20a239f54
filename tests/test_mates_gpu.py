"""scrg_select_mates on the GPU against tests/mate_model.py: device tensors in, no alignment involved — distances, statuses, starts
and strands are drawn.  Every team size a launch can resolve to (4, 8, 16, 32, 64 lanes per mate pair), batch sizes around a
wavefront's worth of teams so that idle teams and idle lanes carry the butterflies, mate pairs whose combinations are no multiple
of the team, one that a team loops over many times, empty sides and sides with nothing eligible."""
import numpy as np
import pytest

from scrooge_amd import api
from tests import mate_model as mm

# (n_a, n_b) a batch may hold so that its largest min(n_a x n_b, 64) resolves to the team size; the first one alone does already
SHAPES = {
    4: [(2, 2), (1, 1), (0, 0), (0, 3), (2, 0), (1, 4), (4, 1), (1, 2), (3, 1)],
    8: [(1, 5), (2, 4), (8, 1), (0, 0), (1, 1), (7, 1), (0, 9), (2, 3), (6, 0)],
    16: [(4, 4), (3, 3), (1, 9), (0, 0), (2, 8), (16, 1), (1, 1), (0, 4), (5, 3)],
    32: [(1, 17), (4, 8), (5, 6), (0, 0), (4, 4), (32, 1), (3, 7), (40, 0), (1, 1)],
    64: [(5, 13), (8, 8), (9, 9), (33, 1), (0, 0), (4, 4), (1, 64), (0, 70), (7, 9)],
}
RULES = [(0, 2 ** 64 - 1, mm.ANY, 0), (200, 900, mm.FR, 1), (150, 1500, mm.RF, 1000), (0, 700, mm.FF, 0), (300, 300, mm.ANY, 1)]
LANE_OVER_LIMIT, LANE_NOT_BEST = 2, 3


def draw_mate(rng, n_a, n_b, kind):
    """kind 0: drawn; 1: every candidate over the limit; 2: side B over the limit"""
    sides = []
    for which, n in enumerate((n_a, n_b)):
        status = [int(x) for x in rng.choice([0, 0, 0, 0, 1, 2], n)]
        if kind == 1 or (kind == 2 and which == 1):
            status = [LANE_OVER_LIMIT] * n
        sides.append({"start": [int(x) for x in rng.integers(0, 2000, n)], "rev": [int(x) for x in rng.integers(0, 2, n)],
                      "ed": [int(x) for x in rng.integers(0, 5, n)], "status": status, "len": int(rng.integers(30, 250)),
                      "n_runs": [int(x) for x in rng.integers(1, 40, n)]})
    return sides


def run_and_check(aligner, mates, rule, with_reverse=True, team=None):
    import torch
    dev = torch.device("cuda", aligner.device)
    first, flat = [0], {k: [] for k in ("start", "rev", "ed", "status", "n_runs", "len")}
    for sides in mates:
        for s in sides:
            for k in ("start", "rev", "ed", "status", "n_runs"):
                flat[k] += s[k]
            flat["len"] += [s["len"]] * len(s["start"])
            first.append(len(flat["start"]))
    n, nm = first[-1], len(mates)
    if not with_reverse:
        flat["rev"] = [0] * n

    def tensor(values, dtype, room=1):
        return torch.from_numpy(np.asarray(list(values) + [0] * room, dtype=dtype)).to(dev)
    t_first, t_start, t_len = tensor(first, np.int64, 0), tensor(flat["start"], np.int64), tensor(flat["len"], np.int32)
    t_rev, t_ed = tensor(flat["rev"], np.uint8), tensor(flat["ed"], np.int64)
    t_status, t_runs = tensor(flat["status"], np.int32), tensor(flat["n_runs"], np.int32)
    is_best = torch.full((n + 1,), 9, dtype=torch.uint8, device=dev)
    records = torch.full((32 * (nm + 1),), 0xEE, dtype=torch.uint8, device=dev)
    aligner.select_mates(nm, t_first, t_start, t_len, t_rev if with_reverse else None, t_ed, t_status, t_runs, is_best, records, rule=api.MateRule(*rule),
                         team=team)
    torch.cuda.synchronize()
    got = records.cpu().numpy()
    assert set(got[32 * nm:].tolist()) == {0xEE} and int(is_best[n]) == 9        # nothing past the end is written
    got = got[:32 * nm].view(api.mate_dtype())
    best, status, runs = is_best.cpu().numpy()[:n], t_status.cpu().numpy()[:n], t_runs.cpu().numpy()[:n]
    assert t_ed.cpu().numpy()[:n].tolist() == flat["ed"]
    wants = []
    for m, sides in enumerate(mates):
        a, b = sides
        want = mm.choose(rule, *[(s["start"], s["rev"] if with_reverse else [0] * len(s["start"]), s["ed"], [x != LANE_OVER_LIMIT for x in s["status"]], s["len"])
                                 for s in (a, b)])
        wants.append(want)
        fa, fb = first[2 * m], first[2 * m + 1]
        winner = tuple(api.MATES_NONE if w is None else f + w for w, f in zip(want["winner"], (fa, fb)))
        r = got[m]
        assert (tuple(int(x) for x in r["winner"]), int(r["cost"]), int(r["second_cost"]), int(r["span"]), int(r["n_proper"]), int(r["flags"]), int(r["reserved"])) == \
            (winner, want["cost"], want["second_cost"], want["span"], want["n_proper"], want["flags"], 0), (m, rule, sides)
        marks = want["is_best_a"] + want["is_best_b"]
        assert best[fa:first[2 * m + 2]].tolist() == marks, (m, rule, sides)
        for k, p in enumerate(range(fa, first[2 * m + 2])):
            before = (flat["status"][p], flat["n_runs"][p])
            after = before if marks[k] or before[0] == LANE_OVER_LIMIT else (LANE_NOT_BEST, 0)
            assert (int(status[p]), int(runs[p])) == after, (m, p, rule, sides)
    return wants


@pytest.mark.gpu
@pytest.mark.parametrize("team", [4, 8, 16, 32, 64])
def test_select_mates_every_team_size_and_batch_edge(aligner, team):
    rng = np.random.Generator(np.random.PCG64(100 + team))
    shapes, per_wave = SHAPES[team], 64 // team
    assert all(min(a * b, 64) <= team for a, b in shapes) and team // 2 < min(shapes[0][0] * shapes[0][1], 64) <= team
    kinds = {"proper": 0, "unpaired": 0, "tied": 0, "none": 0}
    for nm in sorted({1, per_wave - 1, per_wave, per_wave + 1, 2500} - {0}):
        picks = [shapes[0]] + [shapes[int(k)] for k in rng.integers(0, len(shapes), nm - 1)]
        mates = [draw_mate(rng, a, b, (0, 0, 0, 0, 0, 1, 2)[int(rng.integers(0, 7))] if m else 0) for m, (a, b) in enumerate(picks)]
        rule = RULES[int(rng.integers(0, len(RULES)))]
        # the team size given (one launch, exact grid), a smaller one (its lanes loop longer: still correct), then found on the device
        run_and_check(aligner, mates, rule, team=team)
        run_and_check(aligner, mates, rule, team=max(4, team // 4))
        for want in run_and_check(aligner, mates, rule):
            kinds["proper" if want["flags"] & mm.PROPER else "unpaired"] += 1
            kinds["tied"] += bool(want["flags"] & mm.TIED)
            kinds["none"] += not want["flags"] & (mm.HAS_A | mm.HAS_B)
    assert all(v > 0 for v in kinds.values()), kinds


@pytest.mark.gpu
def test_select_mates_a_team_loops_many_times(aligner):
    """300 x 300 candidates, every combination proper: n_proper saturates, the winner is the lowest (i, j) of the least cost and
    second_cost ties with it; next to it a 300 x 300 pair under a real rule, and small neighbours on both sides."""
    rng = np.random.Generator(np.random.PCG64(300))
    mates = [draw_mate(rng, 3, 2, 0), draw_mate(rng, 300, 300, 0), draw_mate(rng, 0, 0, 0), draw_mate(rng, 300, 300, 0), draw_mate(rng, 2, 2, 0)]
    for s in mates[1]:
        s["status"] = [0] * 300
    wants = run_and_check(aligner, mates, (0, 2 ** 64 - 1, mm.ANY, 0))
    assert wants[1]["n_proper"] == 65535 and wants[1]["flags"] & mm.TIED and wants[1]["second_cost"] == wants[1]["cost"]
    wants = run_and_check(aligner, mates, (100, 400, mm.FR, 2))
    assert 0 < wants[3]["n_proper"] < 65535


@pytest.mark.gpu
def test_select_mates_without_strands_and_with_the_default_rule(aligner):
    """d_reverse = NULL is all forward: FF sees every combination, FR and RF none; rule = NULL is FR with any span."""
    import torch
    rng = np.random.Generator(np.random.PCG64(5))
    mates = [draw_mate(rng, int(a), int(b), 0) for a, b in rng.integers(0, 7, (200, 2))]
    wants = run_and_check(aligner, mates, (0, 1200, mm.FF, 1), with_reverse=False)
    assert any(w["flags"] & mm.PROPER for w in wants)
    wants = run_and_check(aligner, mates, (0, 2 ** 64 - 1, mm.FR, 0), with_reverse=False)
    assert not any(w["n_proper"] for w in wants)
    # the default rule through the binding (rule=None), with strands
    dev = torch.device("cuda", aligner.device)
    a = ([10, 700], [0, 0], [3, 0])
    t = [torch.tensor(x, device=dev, dtype=d) for x, d in (([0, 2, 3], torch.int64), (a[0] + [750], torch.int64), ([100] * 3, torch.int32),
                                                            (a[1] + [1], torch.uint8), (a[2] + [2], torch.int64), ([0] * 3, torch.int32), ([5] * 3, torch.int32))]
    records = torch.zeros(32, dtype=torch.uint8, device=dev)
    aligner.select_mates(1, *t, None, records)
    torch.cuda.synchronize()
    r = records.cpu().numpy().view(api.mate_dtype())[0]
    # FR: (0, 0) costs 5 and (1, 0) costs 2, both proper; the single bests cost 2 as well
    assert r["winner"].tolist() == [1, 2] and int(r["flags"]) == mm.PROPER | mm.HAS_A | mm.HAS_B and int(r["n_proper"]) == 2 and int(r["second_cost"]) == 5
    assert t[5].cpu().tolist() == [3, 0, 0] and t[6].cpu().tolist() == [0, 5, 5]


@pytest.mark.gpu
def test_select_mates_refuses_an_invalid_rule(aligner):
    import torch
    import scrooge_amd
    dev = torch.device("cuda", aligner.device)
    z64, z32 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    records = torch.full((32,), 0xEE, dtype=torch.uint8, device=dev)
    for bad in (dict(min_span=2, max_span=1), dict(orientation=4), dict(reserved=(0, 1))):
        with pytest.raises(scrooge_amd.ScroogeError):
            aligner.select_mates(1, z64, z64, z32, None, z64, z32, z32, None, records, rule=api.MateRule(**bad))
    torch.cuda.synchronize()
    assert set(records.cpu().tolist()) == {0xEE}


# ---------------------------------------------------------------------------------------------------------------
# the host call
# ---------------------------------------------------------------------------------------------------------------
def revcomp(b):
    return bytes(b)[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def mutate(rng, seq, n):
    q = bytearray(seq)
    for pos in rng.choice(len(q), n, replace=False):
        q[pos] = ord("ACGT"[("ACGT".index(chr(q[pos])) + 1 + int(rng.integers(0, 3))) % 4])
    return bytes(q)


def paired_batch():
    """300 mate pairs of 150 bp from a 200 kb genome with a mutated repeat (genome[100 k .. 120 k) is a 1 % mutated copy of
    [20 k .. 40 k)): per read 1 to 5 candidates — the true location, the other copy, wrong-strand and random decoys."""
    from scrooge_amd import synth
    rng = np.random.Generator(np.random.PCG64(8))
    genome = bytearray(synth.random_seq(200000, rng))
    genome[100000:120000] = mutate(rng, genome[20000:40000], 200)
    genome = bytes(genome)
    reads, cands, rev = [], [], []
    for m in range(300):
        s_a = int(rng.integers(20000, 39000)) if m % 3 else int(rng.integers(130000, 190000))
        s_b = s_a + int(rng.integers(100, 500))
        flip = m % 2                                              # the pair lies the other way round: A reverse, B forward
        for which, s in enumerate((s_b, s_a) if flip else (s_a, s_b)):
            is_rev = int(which != flip)
            frag = mutate(rng, genome[s:s + 150], int(rng.integers(0, 6)))
            reads.append(revcomp(frag) if is_rev else frag)
            # (every tenth mate pair: side B's true location is not among its candidates, so nothing is proper)
            cs, rs = [s if which == 0 or m % 10 != 9 else (s + 90000) % 199000], [is_rev]
            if s < 40000:
                cs.append(s + 80000), rs.append(is_rev)         # the repeat's other copy
            for _ in range(int(rng.integers(0, 4))):
                kind = int(rng.integers(0, 3))
                cs.append(s if kind == 0 else int(rng.integers(0, 199000))), rs.append(1 - is_rev if kind == 0 else int(rng.integers(0, 2)))
            keep = rng.permutation(len(cs))
            cands.append([cs[int(k)] for k in keep]), rev.append([rs[int(k)] for k in keep])
    return genome, reads, cands, rev


def model_records(plain, reads, cands, rev, rule):
    """the model fed with a plain call's distances and statuses -> per mate pair the dict of mate_model.choose, winners as pair indices"""
    co = np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)
    out = []
    for m in range(len(reads) // 2):
        sides = []
        for r in (2 * m, 2 * m + 1):
            sl = slice(int(co[r]), int(co[r + 1]))
            sides.append((cands[r], rev[r] if rev is not None else [0] * len(cands[r]), [int(x) for x in plain["edit_distance"][sl]],
                          [int(x) != api.SCRG_PAIR_OVER_EDIT_LIMIT for x in plain["status"][sl]], len(reads[r])))
        want = mm.choose(rule, *sides)
        want["winner"] = tuple(api.MATES_NONE if w is None else int(co[2 * m + k]) + w for k, w in enumerate(want["winner"]))
        out.append(want)
    return out, co


def check_paired(got, mates, plain, wants, distance=False, runs=True, text=True):
    n = len(plain["status"])
    winners = set()
    for m, want in enumerate(wants):
        r = mates[m]
        assert (tuple(int(x) for x in r["winner"]), int(r["cost"]), int(r["second_cost"]), int(r["span"]), int(r["n_proper"]), int(r["flags"]), int(r["reserved"])) == \
            (want["winner"], want["cost"], want["second_cost"], want["span"], want["n_proper"], want["flags"], 0), m
        winners |= {w for w in want["winner"] if w != api.MATES_NONE}
    assert np.array_equal(got["edit_distance"], plain["edit_distance"])
    for p in range(n):
        if p in winners or int(plain["status"][p]) == api.SCRG_PAIR_OVER_EDIT_LIMIT:
            assert int(got["status"][p]) == int(plain["status"][p]), p
            if distance:
                assert int(got["text_end"][p]) == int(plain["text_end"][p]), p
            if runs and not distance:
                a, b = (slice(int(x["run_offset"][p]), int(x["run_offset"][p + 1])) for x in (got, plain))
                assert np.array_equal(got["runs"][a], plain["runs"][b]) and (p not in winners or a.stop > a.start), p
            if text and not distance:
                ta, tb = (x["cigar_text"][int(x["cigar_offset"][p]):int(x["cigar_offset"][p + 1])] for x in (got, plain))
                assert ta == tb and (p not in winners or len(ta) > 1), p
        else:
            assert int(got["status"][p]) == api.SCRG_PAIR_NOT_BEST, p
            assert got["run_offset"][p] == got["run_offset"][p + 1] and (not text or distance or got["cigar_offset"][p + 1] - got["cigar_offset"][p] == 1), p


@pytest.mark.gpu
def test_align_mapping_paired_end_to_end(aligner):
    genome, reads, cands, rev = paired_batch()
    aligner.set_genome(genome)
    rule = (150, 800, mm.FR, 2)
    seen = None
    for kw, distance in (({}, False), ({"max_edits": 12}, False), ({"outputs": api.SCRG_OUT_DISTANCE}, True), ({"outputs": api.SCRG_OUT_TEXT | api.SCRG_OUT_BEST}, False)):
        plain_kw = dict(kw)
        if plain_kw.get("outputs") == api.SCRG_OUT_TEXT | api.SCRG_OUT_BEST:
            plain_kw["outputs"] = api.SCRG_OUT_ALL
        plain = aligner.align_mapping_directed(reads, cands, reverse=rev, arrays=True, **plain_kw)
        wants, co = model_records(plain, reads, cands, rev, rule)
        per_sort = []
        for sort in (0, 1):
            got, mates = aligner.align_mapping_paired(reads, cands, reverse=rev, rule=api.MateRule(*rule), arrays=True, sort_by_length=sort, **kw)
            text_only = kw.get("outputs") == api.SCRG_OUT_TEXT | api.SCRG_OUT_BEST
            assert not text_only or got["run_offset"][-1] == 0
            check_paired(got, mates, plain, wants, distance, runs=not text_only)
            per_sort.append(mates)
        assert per_sort[0].tobytes() == per_sort[1].tobytes()
        if not kw:
            seen = wants
        elif "max_edits" in kw:
            assert (plain["status"] == api.SCRG_PAIR_OVER_EDIT_LIMIT).sum() > 20
    flags = [w["flags"] for w in seen]
    assert sum(bool(f & mm.PROPER) for f in flags) > 200 and any(not f & mm.PROPER for f in flags)
    # the winners differ from best-candidate mode's somewhere: the repeat's other copy has fewer edits for some mate
    best = aligner.align_mapping_directed(reads, cands, reverse=rev, arrays=True, best=True)
    got, _ = aligner.align_mapping_paired(reads, cands, reverse=rev, rule=api.MateRule(*rule), arrays=True)
    assert not np.array_equal(best["status"], got["status"])


@pytest.mark.gpu
def test_the_paired_call_and_best_mode_disagree(aligner):
    """tests/test_mates_rule.py's hand-made case through the GPU: read A has one edit against a repeat copy 40 kb away and three
    against its true locus 300 bp from its mate; best-candidate mode takes the copy, the paired call with penalty 2 the locus, with
    penalty 0 the copy again."""
    from scrooge_amd import synth
    rng = np.random.Generator(np.random.PCG64(3))
    genome = bytearray(synth.random_seq(140000, rng))
    base = bytearray(genome[60000:60150])
    locus = bytearray(base)
    for pos in (20, 90):
        locus[pos] = ord("A") if locus[pos] != ord("A") else ord("C")
    genome[20000:20150] = locus
    read_a = bytearray(base)
    read_a[55] = ord("G") if read_a[55] != ord("G") else ord("T")
    genome = bytes(genome)
    read_b = revcomp(genome[20150:20300])
    reads, cands, rev = [bytes(read_a), read_b], [[60000, 20000], [20150]], [[0, 0], [1]]
    aligner.set_genome(genome)
    plain = aligner.align_mapping_directed(reads, cands, reverse=rev, arrays=True)
    assert plain["edit_distance"].tolist() == [1, 3, 0]
    best = aligner.align_mapping_directed(reads, cands, reverse=rev, arrays=True, best=True)
    assert best["status"].tolist() == [api.SCRG_OK, api.SCRG_PAIR_NOT_BEST, api.SCRG_OK]
    got, mates = aligner.align_mapping_paired(reads, cands, reverse=rev, rule=api.MateRule(0, 1000, "fr", 2), arrays=True)
    assert got["status"].tolist() == [api.SCRG_PAIR_NOT_BEST, api.SCRG_OK, api.SCRG_OK]
    assert mates["winner"].tolist() == [[1, 2]] and int(mates["flags"][0]) == mm.PROPER | mm.HAS_A | mm.HAS_B and int(mates["span"][0]) == 300
    assert (int(mates["cost"][0]), int(mates["n_proper"][0])) == (3, 1)
    got, mates = aligner.align_mapping_paired(reads, cands, reverse=rev, rule=api.MateRule(0, 1000, "fr", 0), arrays=True)
    assert got["status"].tolist() == best["status"].tolist() and mates["winner"].tolist() == [[0, 2]] and int(mates["flags"][0]) == mm.HAS_A | mm.HAS_B


@pytest.mark.gpu
def test_mate_pairs_larger_than_a_chunk(aligner):
    """Mates of unequal length with thousands of candidates of the 50 bp one: the plan cuts the batch into several chunks, none
    inside a mate pair; records and results are the model's."""
    from scrooge_amd import synth
    rng = np.random.Generator(np.random.PCG64(9))
    G, K = 30000, 3000
    genome = synth.random_seq(G + 1024, rng)
    reads, cands, rev = [], [], []
    for m in range(24):
        s = int(rng.integers(0, G - 600))
        reads.append(mutate(rng, genome[s:s + 50], 1))
        cs = [int(x) for x in rng.integers(0, G, K)]
        cs[(0, K - 1, int(rng.integers(1, K - 1)))[m % 3]] = s
        cands.append(cs), rev.append([0] * K)
        t = s + int(rng.integers(100, 400))
        reads.append(revcomp(mutate(rng, genome[t:t + 80], 2)))
        n_b = int(rng.integers(0, 4))
        cands.append([t, int(rng.integers(0, G)), t][:n_b]), rev.append([1, 0, 1][:n_b])
    co = np.concatenate([[0], np.cumsum([len(c) for c in cands])])
    order, first = api.host_plan_mates([len(r) for r in reads], co)
    assert len(first) > 3, "the batch should be cut into at least three chunks"
    read = np.repeat(np.arange(len(reads)), np.diff(co))
    assert all(read[order[int(c) - 1]] // 2 != read[order[int(c)]] // 2 for c in first[1:-1])
    aligner.set_genome(genome)
    rule = (100, 600, mm.FR, 3)
    plain = aligner.align_mapping_directed(reads, cands, reverse=rev, arrays=True, outputs=api.SCRG_OUT_RUNS)
    wants, _ = model_records(plain, reads, cands, rev, rule)
    got, mates = aligner.align_mapping_paired(reads, cands, reverse=rev, rule=api.MateRule(*rule), arrays=True, outputs=api.SCRG_OUT_RUNS)
    check_paired(got, mates, plain, wants, text=False)
    assert any(w["flags"] & mm.PROPER for w in wants) and any(not w["flags"] & mm.HAS_B for w in wants)


@pytest.mark.gpu
def test_only_the_winners_pile_up(aligner):
    from tests.test_pileup_gpu import check_take, host_batch, model_of_result
    b = host_batch()
    aligner.set_genome(b["genome"])
    rule = api.MateRule(0, 5000, "any", 0)
    plain = aligner.align_mapping_directed(b["reads"], b["cands"], reverse=b["reverse"], arrays=True)
    aligner.set_pileup()
    try:
        got, mates = aligner.align_mapping_paired(b["reads"], b["cands"], reverse=b["reverse"], rule=rule, arrays=True)
        winners = {int(w) for w in mates["winner"].ravel() if int(w) != api.MATES_NONE}
        assert len(mates) == 150 and 0 < len(winners) <= 300
        dropped = dict(plain, status=np.array([s if p in winners else api.SCRG_PAIR_NOT_BEST for p, s in enumerate(plain["status"])], dtype=np.uint32))
        want = model_of_result(b, dropped)
        assert want[2] == len(winners)
        check_take(aligner, want, "paired")
        assert np.array_equal(got["status"], dropped["status"])
    finally:
        aligner.set_pileup(False)


@pytest.mark.gpu
def test_the_paired_call_refuses(aligner):
    import scrooge_amd
    aligner.set_genome(b"ACGT" * 100)
    for reads, cands, kw in (([b"ACGTACGT"] * 3, [[0], [4], [8]], {}), ([b"ACGTACGT"] * 2, [[0], [4]], {"rule": api.MateRule(5, 4)}),
                             ([b"ACGTACGT"] * 2, [[0], [4]], {"rule": api.MateRule(orientation=4)}),
                             ([b"ACGTACGT"] * 2, [[0], [4]], {"rule": api.MateRule(reserved=(0, 1))})):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            aligner.align_mapping_paired(reads, cands, **kw)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    # ... and leaves nothing to take: both out pointers are NULL after a refused call, whatever they held
    import ctypes as C
    reads = (C.c_char_p * 3)(b"ACGTACGT", b"ACGTACGT", b"ACGTACGT")
    lens, offs, starts = (C.c_uint64 * 3)(8, 8, 8), (C.c_uint64 * 4)(0, 1, 2, 3), (C.c_uint64 * 3)(0, 4, 8)
    for n_reads, rule in ((3, None), (2, api.MateRule(5, 4).as_c())):
        res, mt = C.POINTER(api.Result)(), C.c_void_p(12345)
        res.contents = api.Result()
        st = api._lazy(aligner.lib, "scrg_align_mapping_paired")(aligner.h, C.byref(aligner._params({})), n_reads, C.cast(reads, C.c_void_p), C.cast(lens, C.c_void_p),
                                                                 C.cast(offs, C.c_void_p), C.cast(starts, C.c_void_p), None,
                                                                 C.byref(rule) if rule is not None else None, C.byref(mt), C.byref(res))
        assert st == api.SCRG_ERR_INVALID_ARG and not res and mt.value is None
    got, mates = aligner.align_mapping_paired([b"ACGTACGT", b"ACGTACGT", b"", b"ACGT"], [[0], [4, 8], [], []], arrays=True)
    assert len(mates) == 2 and mates["winner"][1].tolist() == [api.MATES_NONE] * 2 and int(mates["flags"][1]) == 0 and int(mates["second_cost"][1]) == 0xffffffff
    assert got["status"].tolist().count(api.SCRG_OK) == 2


def paired_dataset(tmp_path):
    """60 mate pairs from two chromosomes as an interleaved FASTQ with PAF seeds: the true location of each mate (A forward, B
    reverse 150 .. 400 further on) and, for every other read, a decoy far away on the other chromosome."""
    from scrooge_amd import synth
    rng = np.random.Generator(np.random.PCG64(61))
    chroms = {"chr1": synth.random_seq(6000, rng), "chr2": synth.random_seq(5000, rng)}
    fa, fq, seeds = (str(tmp_path / x) for x in ("g.fa", "r.fq", "s.paf"))
    with open(fa, "w") as f:
        for name, seq in chroms.items():
            f.write(">%s\n%s\n" % (name, seq.decode()))
    with open(fq, "w") as f, open(seeds, "w") as s:
        for m in range(60):
            name = "chr1" if m % 2 else "chr2"
            other = "chr2" if m % 2 else "chr1"
            a = int(rng.integers(0, len(chroms[name]) - 700))
            b = a + int(rng.integers(150, 400))
            for side, (start, strand) in enumerate(((a, "+"), (b, "-"))):
                frag = mutate(rng, chroms[name][start:start + 100], int(rng.integers(0, 4)))
                seq = revcomp(frag) if strand == "-" else frag
                f.write("@m%d/%d\n%s\n+\n%s\n" % (m, side + 1, seq.decode(), "I" * 100))
                s.write("m%d/%d\t100\t0\t100\t%s\t%s\t%d\t%d\t%d\t100\t100\t60\n" % (m, side + 1, strand, name, len(chroms[name]), start, start + 100))
                if (m + side) % 2:
                    d = int(rng.integers(0, 4000))
                    s.write("m%d/%d\t100\t0\t100\t%s\t%s\t%d\t%d\t%d\t100\t100\t60\n" % (m, side + 1, "+-"[m % 2], other, len(chroms[other]), d, d + 100))
    return fa, fq, seeds


@pytest.mark.gpu
def test_job_and_cli_paired_end_to_end(aligner, tmp_path, capsys):
    """Job.align_paired and `--paired --mate_rule=`: every mate pair is proper, the SAM has one record per read with the pair's
    columns consistent between the two mates, and the CLI writes the file the loader's call writes."""
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    fa, fq, seeds = paired_dataset(tmp_path)
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    assert job.n_reads == 120 and job.n_pairs == 180
    out = str(tmp_path / "job.sam")
    alns, mates = job.align_paired(aligner, out_path=out, fmt="sam", rule=api.MateRule(100, 700, "fr", 3))
    assert len(alns) == 180 and len(mates) == 60 and int((mates["flags"] & mm.PROPER).sum()) == 60
    assert aligner.last_status.count(api.SCRG_PAIR_NOT_BEST) == 60 and aligner.last_status.count(api.SCRG_OK) == 120
    sam = [x.split("\t") for x in open(out).read().splitlines() if not x.startswith("@")]
    assert [x[0] for x in sam] == ["m%d/%d" % (m, k) for m in range(60) for k in (1, 2)]
    for m in range(60):
        a, b = sam[2 * m], sam[2 * m + 1]
        assert (int(a[1]), int(b[1])) == (0x1 | 0x40 | 0x2 | 0x20, 0x1 | 0x80 | 0x2 | 0x10), m
        assert a[2] == b[2] == ("chr1" if m % 2 else "chr2") and a[6] == b[6] == "=" and (a[7], b[7]) == (b[3], a[3]), m
        assert int(a[8]) == -int(b[8]) and 250 <= int(a[8]) <= 510 and a[5] != "*" and b[5] != "*", m
    paf = str(tmp_path / "job.paf")
    job.align_paired(aligner, out_path=paf, fmt="paf", rule=api.MateRule(100, 700, "fr", 3))
    assert len(open(paf).read().splitlines()) == 120
    cli_out = str(tmp_path / "cli.sam")
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--reverse_strand", "--paired", "--mate_rule=100,700,FR,3",
                     "--format=sam", "--out=" + cli_out]) == 0
    assert "60 of 60 mate pairs proper" in capsys.readouterr().err
    assert open(cli_out).read() == open(out).read()
    for bad in (["--mate_rule=100,700,FR,3"], ["--paired", "--mate_rule=700,100,FR,3"], ["--paired", "--mate_rule=1,2,XX,0"], ["--paired", "--format=tsv"],
                ["--paired", "--distance_only"]):
        with pytest.raises(SystemExit):
            cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds] + bad)
    capsys.readouterr()
