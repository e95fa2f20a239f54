"""Soft clipping on the CPU (include/scrooge_amd.h: SOFT CLIPPING): the rule's two Python statements against each other
(tests/clip_model.py), the host function scrg_clip_from_runs against them, the interface, and the writer scrg_job_write_clipped on
hand-made records.  The kernel is held to the same model in tests/test_clip_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from scrooge_amd import io as sio
from tests import clip_model as cm
from tests.test_best_candidate import COMP, hand_result, write_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVER = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT
NEW = ["scrg_ctx_set_clip", "scrg_ctx_get_clip", "scrg_ctx_take_clip", "scrg_clip_free", "scrg_clip_device"]
NEW_IO = ["scrg_job_write_clipped", "scrg_clip_from_runs"]


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


def test_interface(lib):
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scrooge_amd.hpp")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    for name in NEW_IO:
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS, name
    m = re.search(r"typedef struct scrg_pair_clip \{(.*?)\} scrg_pair_clip;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == list(api.CLIP_FIELDS) == list(cm.FIELDS)
    assert C.sizeof(api.PairClip) == 32 == api.clip_dtype().itemsize
    # new entry points only: no struct of the interface moved
    assert lib.scrg_abi_version() == 8 == api.SCRG_ABI_VERSION
    assert re.search(r"void\s+set_clip\s*\(", hpp) and re.search(r"take_clip\s*\(", hpp)
    for name in ("set_clip", "clip", "take_clip", "clip_device"):
        assert hasattr(api.Aligner, name)
    assert "clip_kernels.hip" in open(os.path.join(ROOT, "scrooge_amd", "csrc", "Makefile")).read()


def test_the_two_statements_of_the_rule_agree():
    rng = np.random.Generator(np.random.PCG64(700))
    seen_ties = 0
    for k in range(3000):
        n = int(rng.integers(0, 40))
        runs = cm.random_runs(rng, n, max_count=[3, 12, 255][k % 3], p_match=[0.5, 0.3, 0.7][k % 3])
        costs = cm.random_costs(rng)
        b = cm.brute(runs, costs)
        assert cm.model(runs, costs) == b, (runs, costs)
        if b["n_runs"]:
            kept = cm.kept(runs, b)
            assert kept[0][1] == "=" and kept[-1][1] == "="
            cigar = "".join("%d%s" % r for r in kept)
            assert b["score"] == sio.affine_score(cigar, *costs) > 0          # the stretch's score is the affine score of its CIGAR
            assert b["n_edits"] == sum(c for c, o in kept if o != "=")
            assert b["read_end"] - b["read_start"] == sum(c for c, o in kept if o != "D")
            assert b["text_end"] - b["text_start"] == sum(c for c, o in kept if o != "I")
            seen_ties += b["first_run"] > 0
        else:
            assert b == cm.record() and not any(o == "=" for _, o in runs)
    assert seen_ties > 500


def test_host_function_against_the_model():
    rng = np.random.Generator(np.random.PCG64(701))
    lengths = list(rng.integers(0, 60, size=2600)) + list(rng.integers(60, 1101, size=400)) + [0, 1, 24, 25, 511, 512, 513, 1024, 1025, 1100]
    clipped = 0
    for k, n in enumerate(lengths):
        runs = cm.random_runs(rng, int(n), max_count=[3, 12, 255][k % 3], p_match=[0.5, 0.3, 0.7, 0.9][k % 4])
        costs = cm.random_costs(rng)
        want = cm.model(runs, costs)
        assert api.clip_from_runs(runs, costs) == want, (k, runs, costs)
        clipped += want["n_runs"] not in (0, len(runs))
    assert clipped > 2000
    runs = cm.random_runs(rng, 300)
    assert api.clip_from_runs(runs) == cm.model(runs, cm.COSTS) == api.clip_from_runs(runs, cm.COSTS)      # NULL costs: 2, 4, 4, 2
    assert api.clip_from_runs("4=1X2=1D2=") == cm.model(cm_parse("4=1X2=1D2="))


def cm_parse(cigar):
    return [(int(c), o) for c, o in re.findall(r"(\d+)(.)", cigar)]


@pytest.mark.parametrize("place", [0, 3])
def test_ties(place):
    """Two stretches of equal score: the later j wins.  Two starts of equal P_i: the earlier i wins."""
    pad = [(1, "="), (3, "X")] * place                   # something in front: = 2, X 12 — P falls, and no stretch from there pays
    # 5= (10) | 3X (-12) | 5= (10): the stretches [0], [2] score 10, [0..2] scores 8 — the later one wins
    runs = pad + [(5, "="), (3, "X"), (5, "=")]
    got = api.clip_from_runs(runs)
    assert got == cm.model(runs) == cm.brute(runs)
    assert (got["first_run"], got["n_runs"], got["score"]) == (2 * place + 2, 1, 10)
    # 4= (8) | 2X (-8) | 4= (8): P is 0 in front of run 0 and of run 2 — for j = 2 both starts score 8; the earlier i wins
    runs = [(4, "="), (2, "X"), (4, "=")]
    got = api.clip_from_runs(runs)
    assert got == cm.model(runs) == cm.brute(runs)
    assert (got["first_run"], got["n_runs"], got["score"], got["n_edits"]) == (0, 3, 8, 2)
    # zero costs: every start scores the same, every later '=' raises the score
    runs = [(1, "X"), (2, "="), (3, "I"), (1, "D"), (2, "="), (1, "X")]
    got = api.clip_from_runs(runs, (1, 0, 0, 0))
    assert got == cm.brute(runs, (1, 0, 0, 0))
    assert (got["first_run"], got["n_runs"], got["score"], got["n_edits"]) == (1, 4, 4, 4)
    assert (got["read_start"], got["read_end"], got["text_start"], got["text_end"]) == (1, 8, 1, 6)


def test_insertion_then_deletion_is_one_gap():
    # 10= 2I 3D 10=: one opening -> 20 - (4 + 2*5) + 20 = 26; charged twice it would be 22.  Either way the whole list is kept.
    runs = [(10, "="), (2, "I"), (3, "D"), (10, "=")]
    got = api.clip_from_runs(runs)
    assert got == cm.model(runs) and got["score"] == 26 == sio.affine_score("10=2I3D10=")
    # where the second opening decides: 4= 1I 1D 5= is kept whole only when I and D share the opening
    runs = [(4, "="), (1, "I"), (1, "D"), (5, "=")]
    got = api.clip_from_runs(runs, (2, 4, 5, 1))           # gap: -(5 + 2) = -7 shared, -12 twice; 8 - 7 + 10 = 11 > 10
    assert (got["first_run"], got["n_runs"], got["score"]) == (0, 4, 11)
    # the run before the stretch does not open its gap: X I = behind an '=' — the I opens
    runs = [(9, "="), (1, "X"), (1, "I"), (9, "=")]
    assert api.clip_from_runs(runs)["score"] == 18 - 4 - 6 + 18 == cm.brute(runs)["score"]


def test_edge_lists():
    zero = cm.record()
    assert api.clip_from_runs([]) == zero
    assert api.clip_from_runs([(3, "I"), (2, "D"), (7, "I")]) == zero == cm.model([(3, "I"), (2, "D"), (7, "I")])
    assert api.clip_from_runs([(5, "X")]) == zero
    one = api.clip_from_runs([(7, "=")])
    assert one == cm.record(read_end=7, text_end=7, n_runs=1, score=14)
    got = api.clip_from_runs([(2, "D"), (7, "="), (1, "I")])
    assert got == cm.record(read_start=0, read_end=7, text_start=2, text_end=9, first_run=1, n_runs=1, score=14)
    # a run that is no run: the list is not looked at
    good = [(5, "="), (1, "X"), (5, "=")]
    for bad in ((0, "="), (3, "M"), (3, "S"), (0, "I"), (1, "\0")):
        for at in (0, 1, 3):
            runs = good[:at] + [bad] + good[at:]
            assert api.clip_from_runs(runs) == zero == cm.model(runs), (bad, at)


def test_cost_ranges_and_the_32_bit_refusal():
    runs = [(5, "="), (1, "X"), (5, "=")]
    for costs in ((0, 4, 4, 2), (256, 4, 4, 2), (2, -1, 4, 2), (2, 4, 256, 2), (2, 4, 4, 256), (-1, 0, 0, 0)):
        with pytest.raises(api.ScroogeError) as e:
            api.clip_from_runs(runs, costs)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    assert api.clip_from_runs(runs, (255, 255, 255, 255)) == cm.brute(runs, (255, 255, 255, 255)) and cm.brute(runs, (255, 255, 255, 255))["score"] == 9 * 255
    assert api.clip_from_runs(runs, (1, 0, 0, 0))["n_runs"] == 3
    # (read + text) * max(match, mismatch, gap_open + gap_extend) >= 2^31 is refused: a run of 255 '=' is 510 bases of read and text
    worst = 255 + 255
    n_ok = ((1 << 31) - 1) // worst // 510                 # the most runs of 255 '=' that stay below
    big = [(255, "=")] * (n_ok + 1)
    assert (n_ok + 1) * 510 * worst >= 1 << 31 > n_ok * 510 * worst
    with pytest.raises(api.ScroogeError) as e:
        api.clip_from_runs(big, (1, 1, 255, 255))
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    got = api.clip_from_runs(big[:n_ok], (1, 1, 255, 255))
    assert got["n_runs"] == n_ok and got["score"] == 255 * n_ok
    assert api.clip_from_runs(big)["score"] == 2 * 255 * (n_ok + 1)       # the default costs leave room


# ---------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------
def hand_clip(records):
    n = len(records)
    arr = (api.PairClip * max(n, 1))(*[api.PairClip(*[r[f] for f in cm.FIELDS]) for r in records])
    c = api.Clip()
    c.n_pairs = n
    c.pairs = C.cast(arr, C.POINTER(api.PairClip))
    return c, arr


def write_clipped(job, res, clip, path, fmt):
    sio._lib()
    st = job.lib.scrg_job_write_clipped(job.h, C.byref(res), C.byref(clip) if clip is not None else None, path.encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
    return st, ([x for x in open(path).read().splitlines() if not x.startswith("@")] if st == 0 else None)


def test_job_write_clipped(tmp_path):
    """Hand-made records on the twelve pairs of tests/test_best_candidate.py's job (reads of 40 bases, both strands): SAM S items,
    POS, NM and AS; PAF intervals on the read's forward strand; nothing kept: unmapped / left out."""
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    assert n == 12
    full = [(40, "=")]
    # per pair: the full alignment's runs -> the record of the model, the result holds the KEPT runs
    alignments = [
        [(3, "X"), (30, "="), (2, "I"), (5, "X")],                    # clipped at both ends: 3S 30= 7S
        full,                                                         # nothing clipped
        [(2, "D"), (38, "="), (2, "X")],                              # a deletion in front: the text starts 2 later, no S in front
        [(4, "I"), (20, "="), (1, "X"), (15, "=")],                   # 4S 20=1X15=
        [(40, "X")],                                                  # nothing kept
        [(20, "="), (1, "D"), (20, "=")],
        [(1, "="), (6, "X"), (33, "=")],                              # 7S 33=
        [(33, "="), (6, "I"), (1, "=")],                              # 33= 7S
        full, full, full,
        [(5, "I"), (35, "=")],
    ]
    st = [OK] * n
    st[9] = OVER
    recs = [cm.record() if st[k] == OVER else cm.model(a) for k, a in enumerate(alignments)]
    kept = [cm.kept(a, r) for a, r in zip(alignments, recs)]
    cigars = ["".join("%d%s" % x for x in k) for k in kept]
    ed = [sum(c for c, o in a if o != "=") for a in alignments]
    res, keep = hand_result(ed, st, cigars)
    clip, keep_clip = hand_clip(recs)
    assert [r["n_runs"] for r in recs] == [1, 1, 1, 3, 0, 3, 1, 1, 1, 0, 1, 1]
    flat = [(r, rev) for r, cs in enumerate(cands) for _, rev in cs]
    assert {rev for _, rev in flat} == {False, True}
    s, sam = write_clipped(job, res, clip, str(tmp_path / "c.sam"), "sam")
    assert s == 0 and len(sam) == n
    s, paf = write_clipped(job, res, clip, str(tmp_path / "c.paf"), "paf")
    assert s == 0 and len(paf) == n - 2                               # pairs 4 (nothing kept) and 9 (over the limit) are left out
    paf_of = dict(zip([k for k in range(n) if recs[k]["n_runs"]], paf))
    for k, (r, rev) in enumerate(flat):
        rec = recs[k]
        chrom_name, ts, clen = job.pair_chromosome(k)
        seq = (reads[r].translate(COMP)[::-1] if rev else reads[r]).decode()
        f = sam[k].split("\t")
        if rec["n_runs"] == 0:
            assert f == [names[r], str(20 if rev else 4), chrom_name.split()[0], str(ts + 1), "0", "*", "*", "0", "0", seq, "*"], k
            assert k not in paf_of
            continue
        head, tail = rec["read_start"], 40 - rec["read_end"]
        want_cigar = ("%dS" % head if head else "") + cigars[k] + ("%dS" % tail if tail else "")
        assert f == [names[r], str(16 if rev else 0), chrom_name.split()[0], str(ts + rec["text_start"] + 1), "255", want_cigar, "*", "0", "0", seq, "*",
                     "NM:i:%d" % rec["n_edits"], "AS:i:%d" % rec["score"]], k
        qs, qe = (40 - rec["read_end"], 40 - rec["read_start"]) if rev else (rec["read_start"], rec["read_end"])
        matches = sum(c for c, o in kept[k] if o == "=")
        cols = sum(c for c, _ in kept[k])
        assert paf_of[k].split("\t") == [names[r], "40", str(qs), str(qe), "-" if rev else "+", chrom_name.split()[0], str(clen), str(ts + rec["text_start"]),
                                         str(ts + rec["text_end"]), str(matches), str(cols), "255", "NM:i:%d" % rec["n_edits"], "cg:Z:" + cigars[k],
                                         "AS:i:%d" % rec["score"]], k
    assert sam[0].split("\t")[5] == "3S30=7S" and sam[2].split("\t")[5] == "38=2S" and sam[3].split("\t")[5] == "4S20=1X15="
    # clip == NULL: scrg_job_write exactly
    for fmt in ("paf", "sam", "tsv"):
        path = str(tmp_path / ("plain." + fmt))
        assert job.lib.scrg_job_write(job.h, C.byref(res), path.encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt]) == 0
        s, same = write_clipped(job, res, None, str(tmp_path / ("null." + fmt)), fmt)
        assert s == 0 and open(path).read() == open(str(tmp_path / ("null." + fmt))).read()
    # TSV with a clip, a clip of another pair count
    assert write_clipped(job, res, clip, str(tmp_path / "c.tsv"), "tsv")[0] == api.SCRG_ERR_INVALID_ARG
    short, keep_short = hand_clip(recs[:-1])
    assert write_clipped(job, res, short, str(tmp_path / "d.sam"), "sam")[0] == api.SCRG_ERR_INVALID_ARG


def test_cli_arguments():
    from scrooge_amd import cli
    base = ["--reference=g.fa", "--reads=r.fq", "--seeds=s.paf"]
    for extra in (["--clip_costs=2,4,4,2"], ["--clip", "--clip_costs=2,4,4"], ["--clip", "--clip_costs=a,b,c,d"], ["--clip", "--md"],
                  ["--clip", "--report"], ["--clip", "--verify"], ["--clip", "--distance_only"], ["--clip", "--format=tsv"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2, extra
