"""The alignment report on the host (no GPU): the Python model of tests/report_model.py held to a hand-written table,
scrg_report_from_runs held to the model and to the two existing checkers, scrg_report_score held to the reference's recorded
affine scores, the writer's tags, and the interface (include/scrooge_amd.h: ALIGNMENT REPORT)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from scrooge_amd import io as sio
from tests import cigar_check
from tests import diff_model as dm
from tests import report_model as rm
from tests.conftest import load_golden
from tests.test_best_candidate import hand_result, write_job
from tests.test_io import random_affine_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVER = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT
NEW_API = ["scrg_ctx_set_report", "scrg_ctx_get_report", "scrg_ctx_take_report", "scrg_report_free", "scrg_report_device"]
NEW_IO = ["scrg_job_write_report", "scrg_report_from_runs", "scrg_report_score"]


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


def runs_of(r):
    return dm.parse(r) if isinstance(r, str) else list(r)


def host_report(lib, text, read, runs, ed):
    """scrg_report_from_runs -> dict; runs: [(count, op)] or an (n, 2) uint8 array (count, op byte)"""
    text = text.encode() if isinstance(text, str) else bytes(text)
    read = read.encode() if isinstance(read, str) else bytes(read)
    arr = np.ascontiguousarray(runs if isinstance(runs, np.ndarray) else np.array([(c, ord(o)) for c, o in runs], dtype=np.uint8).reshape(-1, 2))
    out = api.PairReport(*([0xEEEEEEEE] * 8))
    st = api._lazy(lib, "scrg_report_from_runs")(text, len(text), read, len(read), C.c_void_p(arr.ctypes.data) if len(arr) else None, len(arr),
                                                 int(ed), C.byref(out))
    assert st == 0
    return rm.as_dict(out)


def test_model_reproduces_the_table():
    verdicts = set()
    for text, read, runs, ed, want in rm.TABLE:
        assert rm.model(text, read, runs_of(runs), ed) == want, (text, read, runs)
        verdicts.add((want["verdict"], want["verdict"] == 3 and want["bad_run"] == len(runs_of(runs))))
    assert {v for v, _ in verdicts} == {0, 1, 2, 3, 4, 5, 6} and (3, True) in verdicts and (3, False) in verdicts
    assert len(rm.TABLE) >= 12


def test_report_from_runs_table(lib):
    for text, read, runs, ed, want in rm.TABLE:
        assert host_report(lib, text, read, runs_of(runs), ed) == want, (text, read, runs)
        assert api.report_from_runs(text, read, runs, ed) == want
    assert sio.report_from_runs is api.report_from_runs


def rendered(runs):
    return "".join("%d%s" % r for r in runs)


def check_case(lib, text, read, runs, ed, what):
    """The mirror against the model; the verdict against both existing checkers (every op here is printable)."""
    want = rm.model(text, read, runs, ed)
    assert host_report(lib, text, read, runs, ed) == want, what
    cigar = rendered(runs)
    assert sio.validate_alignment(text, read, cigar, ed) == want["verdict"], what
    assert (cigar_check.validate(text, read, cigar, ed) is None) == (want["verdict"] == 0), what
    return want


@pytest.mark.parametrize("n_runs", dm.RUN_COUNTS)
def test_report_from_runs_random(lib, n_runs):
    rng = np.random.Generator(np.random.PCG64(300 + n_runs))
    max_count = 255 if n_runs <= 26 else 40
    # random bases under random runs: almost always verdict 5 at the first '=' or 'X' run
    text, read, runs = dm.random_case(rng, n_runs, max_count=max_count)
    check_case(lib, text, read, runs, rm.edits(runs), "random %d" % n_runs)
    # an alignment, and the seven ways of spoiling it
    case = rm.valid_case(rng, n_runs, max_count=max_count)
    assert check_case(lib, *case, "valid %d" % n_runs)["verdict"] == 0
    seen = set()
    for kind in rm.CORRUPTIONS:
        bad = rm.corrupt(kind, *case, rng)
        if bad is None:
            continue
        got = check_case(lib, *bad, "%s %d" % (kind, n_runs))
        assert got["verdict"] != 0, (kind, n_runs)
        seen.add(kind)
    if n_runs >= 23:
        assert seen == set(rm.CORRUPTIONS)


def test_corruptions_reach_every_verdict(lib):
    rng = np.random.Generator(np.random.PCG64(41))
    case = rm.valid_case(rng, 40, max_count=30, slack=0)
    got = {kind: rm.model(*rm.corrupt(kind, *case, rng))["verdict"] for kind in rm.CORRUPTIONS}
    assert got == {"zero_count": 2, "op_M": 1, "extra_I": 3, "extra_D": 4, "flip_in_eq": 5, "equal_in_X": 5, "ed_off": 6}


def score_of(lib, rep, costs):
    r = api.PairReport(*[rep[f] for f in rm.FIELDS])
    out = C.c_int64(-12345)
    st = api._lazy(lib, "scrg_report_score")(C.byref(r), *[int(c) for c in costs], C.byref(out))
    return st, int(out.value)


def np_runs(cigar):
    """cigar -> (n, 2) uint8 runs with counts split at 255, made with numpy (the random vectors have counts up to 3 000)"""
    tok = re.findall(r"(\d+)([=XID])", cigar)
    cnt = np.array([int(n) for n, _ in tok], dtype=np.int64)
    op = np.array([ord(o) for _, o in tok], dtype=np.uint8)
    pieces = (cnt + 254) // 255
    last = cnt - (pieces - 1) * 255
    out_op = np.repeat(op, pieces)
    out_cnt = np.full(int(pieces.sum()), 255, dtype=np.int64)
    if len(cnt):
        out_cnt[np.cumsum(pieces) - 1] = last
    return np.stack([out_cnt.astype(np.uint8), out_op], axis=1) if len(cnt) else np.zeros((0, 2), np.uint8)


def np_sequences(runs, rng):
    """A text and a read (bytes) that the (n, 2) uint8 runs are an alignment of."""
    cnt, op = runs[:, 0].astype(np.int64), runs[:, 1]
    in_t, in_q = op != ord("I"), op != ord("D")
    t_ops, q_ops = np.repeat(op[in_t], cnt[in_t]), np.repeat(op[in_q], cnt[in_q])
    text = rng.integers(0, 4, size=len(t_ops))
    read = rng.integers(0, 4, size=len(q_ops))
    t_al, q_al = np.flatnonzero(t_ops != ord("D")), np.flatnonzero(q_ops != ord("I"))
    read[q_al] = np.where(q_ops[q_al] == ord("="), text[t_al], (text[t_al] + 1) % 4)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    return bases[text].tobytes(), bases[read].tobytes()


def test_score_against_reference_vectors(lib):
    """tests/golden/affine_scores.json: the scores the reference's get_alignment_score returned.  The CIGAR as runs (counts above 255
    split), sequences synthesised to fit, the report's score with the vector's costs."""
    cases = load_golden("affine_scores.json")["cases"]
    assert len(cases) == 1178
    rng = np.random.Generator(np.random.PCG64(17))
    for c in cases:
        runs = rm.cigar_runs(c["cigar"])
        text, read = rm.sequences_for(runs, rng)
        rep = host_report(lib, text, read, runs, rm.edits(runs))
        assert rep == rm.model(text, read, runs, rm.edits(runs)) and rep["verdict"] == 0, c
        assert score_of(lib, rep, c["costs"]) == (0, c["score"]), c
        assert api.report_score(rep, c["costs"]) == c["score"] == rm.score(rep, c["costs"])


def test_score_against_affine_score_random(lib):
    want = load_golden("affine_random_scores.json")["scores"]
    cases = list(random_affine_cases())
    assert len(cases) == len(want) == 2000
    rng = np.random.Generator(np.random.PCG64(18))
    recs = np.zeros(len(cases), dtype=api.report_dtype())
    for k, ((cigar, costs), score) in enumerate(zip(cases, want)):
        runs = np_runs(cigar)
        text, read = np_sequences(runs, rng)
        ed = int(runs[runs[:, 1] != ord("="), 0].astype(np.int64).sum())
        rep = host_report(lib, text, read, runs, ed)
        assert rep["verdict"] == 0, cigar
        assert score_of(lib, rep, costs)[1] == sio.affine_score(cigar, *costs) == score, (cigar, costs)
        recs[k] = tuple(rep[f] for f in rm.FIELDS)
    # the vectorised form, one set of costs for all
    assert api.report_score(recs, (2, 4, 4, 2)).tolist() == [sio.affine_score(c, 2, 4, 4, 2) for c, _ in cases]


def test_score_refuses_records_without_counts(lib):
    ok = rm.record(n_match=5, n_ins=2, n_gap_open=1, n_indel=1)
    assert score_of(lib, ok, rm.COSTS) == (0, 10 - 4 - 4)
    for verdict, bad_run, want in ((6, 2, 0), (3, 2, 0), (3, 0, 0)):
        assert score_of(lib, dict(ok, verdict=verdict, bad_run=bad_run), rm.COSTS)[0] == want
    for verdict in (1, 2, 4, 5, 7):
        assert score_of(lib, rm.record(verdict=verdict, bad_run=1), rm.COSTS)[0] == api.SCRG_ERR_INVALID_ARG
        with pytest.raises(api.ScroogeError):
            api.report_score(rm.record(verdict=verdict, bad_run=1))
    assert score_of(lib, rm.record(verdict=3, bad_run=4), rm.COSTS)[0] == api.SCRG_ERR_INVALID_ARG      # a 3 met AT run 4: no counts
    recs = np.zeros(2, dtype=api.report_dtype())
    recs["verdict"] = [0, 5]
    with pytest.raises(api.ScroogeError):
        api.report_score(recs)
    assert api._lazy(lib, "scrg_report_score")(None, 1, 1, 1, 1, C.byref(C.c_int64())) == api.SCRG_ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------
def hand_report(records):
    n = len(records)
    keep = (api.PairReport * max(1, n))(*[api.PairReport(*[r[f] for f in rm.FIELDS]) for r in records])
    rep = api.Report()
    rep.n_pairs = n
    rep.pairs = C.cast(keep, C.POINTER(api.PairReport))
    rep.n_failed = sum(r["verdict"] not in (0, 7) for r in records)
    return rep, keep


def write_with(job, res, diff, report, costs, tmp_path, fmt, name):
    path = str(tmp_path / (name + "." + fmt))
    if os.path.exists(path):
        os.remove(path)
    sio._lib()
    cost_arr = (C.c_int64 * 4)(*costs) if costs is not None else None
    st = job.lib.scrg_job_write_report(job.h, C.byref(res), C.byref(diff) if diff is not None else None,
                                       C.byref(report) if report is not None else None, cost_arr, path.encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
    return st, (open(path, "rb").read() if os.path.exists(path) else None)


@pytest.mark.parametrize("costs", [None, (1, 3, 5, 1)])
def test_job_write_report(tmp_path, costs):
    """A hand-built result and report: every line is scrg_job_write_diff's line — columns 10 and 11 and every other byte — plus the
    model's tags; an unmapped SAM record and a record whose counts do not cover its runs have none."""
    from tests.test_diff_strings import hand_diff
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    st = [OK] * n
    st[4] = OVER
    cigars = ["" if st[k] == OVER else "%d=%dX1D%d=2I%dD" % (20 - k, 1 + k % 3, 16 - k % 3, 1 + k % 2) for k in range(n)]
    ed = [rm.edits(dm.parse(c)) for c in cigars]
    res, keep = hand_result(ed, st, cigars)
    rng = np.random.Generator(np.random.PCG64(3))
    records = []
    for k, c in enumerate(cigars):
        runs = dm.parse(c)
        text, read = rm.sequences_for(runs, rng)
        records.append(rm.record(verdict=7) if st[k] == OVER else rm.model(text, read, runs, ed[k]))
    assert all(r["verdict"] in (0, 7) for r in records)
    records[2] = rm.record(verdict=5, bad_run=1)               # a pair that failed its check: no counts, so no tags
    records[3] = dict(records[3], verdict=6, bad_run=6)        # counts that cover the runs: tags
    report, keep_r = hand_report(records)
    strings = ["" if st[k] == OVER else "cs-string-%d" % k for k in range(n)]
    diff, keep_d = hand_diff("cs", strings)
    use = rm.COSTS if costs is None else costs
    for fmt in ("paf", "sam"):
        for with_diff in (None, diff):
            path = str(tmp_path / ("plain." + fmt))
            assert job.lib.scrg_job_write_diff(job.h, C.byref(res), C.byref(with_diff) if with_diff is not None else None, path.encode(),
                                               1 if fmt == "sam" else 0) == 0
            plain = open(path, "rb").read()
            s, same = write_with(job, res, with_diff, None, costs, tmp_path, fmt, "null")
            assert s == 0 and same == plain                                    # report == NULL: scrg_job_write_diff exactly
            s, got = write_with(job, res, with_diff, report, costs, tmp_path, fmt, "report")
            assert s == 0
            want, k = [], 0
            kept = [p for p in range(n) if fmt == "sam" or st[p] != OVER]
            for line in plain.decode().splitlines():
                if line.startswith("@"):
                    want.append(line)
                    continue
                p = kept[k]
                k += 1
                rec = records[p]
                tagged = rec["verdict"] in (0, 6)
                assert (st[p] == OVER) == (rec["verdict"] == 7)
                if fmt == "paf" and tagged:                                    # the columns the old walk writes are the report's
                    cols = line.split("\t")
                    assert int(cols[9]) == rec["n_match"] and int(cols[10]) == sum(rec[f] for f in rm.FIELDS[:4])
                want.append(line + ("\tAS:i:%d\tde:f:%.4f" % (rm.score(rec, use), rm.divergence(rec)) if tagged else ""))
            assert k == len(kept) and got.decode().splitlines() == want
    assert write_with(job, res, None, report, costs, tmp_path, "tsv", "report") == (api.SCRG_ERR_INVALID_ARG, None)      # TSV has no tags
    s, got = write_with(job, res, None, None, costs, tmp_path, "tsv", "null")
    assert s == 0 and got
    short, keep_s = hand_report(records[:-1])                                  # a report of another call
    assert write_with(job, res, None, short, costs, tmp_path, "paf", "short")[0] == api.SCRG_ERR_INVALID_ARG


def test_divergence_is_gap_compressed():
    rec = rm.model("ACGTACGTAC", "ACGTTCGAC", dm.parse("4=1X2=1D2="), 2)
    assert rm.divergence(rec) == 2 / 10 and rm.divergence(rm.record()) == 0.0
    assert rm.divergence(rm.record(n_match=90, n_del=30, n_indel=1, n_gap_open=1)) == 1 / 91


# ---------------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------------
def test_header_library_and_bindings_have_the_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    for name in NEW_API:
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    for name in NEW_IO:
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS, name
    assert re.search(r"enum\s*\{\s*SCRG_REPORT_NO_ALIGNMENT\s*=\s*7\s*\}", hdr) and api.REPORT_NO_ALIGNMENT == 7
    m = re.search(r"typedef struct scrg_pair_report \{(.*?)\} scrg_pair_report;", hdr, re.S)
    assert m and re.findall(r"\b(n_\w+|verdict|bad_run)\b\s*[,;]", m.group(1)) == list(api.REPORT_FIELDS) == list(rm.FIELDS)
    # new entry points only: no struct of the interface moved
    assert lib.scrg_abi_version() == 8 == api.SCRG_ABI_VERSION
    assert api.Result._fields_[-1][0] == "text_end" and C.sizeof(api.Params) == 48
    assert C.sizeof(api.PairReport) == 32 == api.report_dtype().itemsize and C.sizeof(api.Report) == 24
    for name in ("set_report", "take_report", "report_device"):
        assert callable(getattr(api.Aligner, name))
    hpp = open(os.path.join(ROOT, "include", "scrooge_amd.hpp")).read()
    assert "set_report" in hpp and "take_report" in hpp


SHIM_SRC = r"""
#include <cstdio>
#include "scrooge_amd.hpp"
#include "scrooge_amd_io.h"
static_assert(sizeof(scrg_pair_report) == 32, "scrg_pair_report is 32 bytes");
int main()
{
    // the host mirror needs no device
    const scrg_run runs[3] = {{4, '='}, {1, 'X'}, {2, '='}};
    scrg_pair_report rep;
    if (scrg_report_from_runs("ACGTACG", 7, "ACGTTCG", 7, runs, 3, 1, &rep) != SCRG_OK) return 1;
    int64_t score = 0;
    if (scrg_report_score(&rep, 2, 4, 4, 2, &score) != SCRG_OK) return 1;
    std::printf("verdict %u matches %u score %lld\n", rep.verdict, rep.n_match, (long long)score);
    if (scrg_device_count() == 0) { std::fprintf(stderr, "no usable HIP device\n"); return 2; }
    scrooge_amd::Handle h(0);
    std::vector<std::string> t = {"ACGTACGTACGTACGTAAAA", "ACGTACGT"}, q = {"ACGTACGTTCGTACGT", "ACGTACG"};
    h.set_report(true);
    h.align_all(t, q);
    uint64_t failed = 99;
    for (const scrg_pair_report& r : h.take_report(&failed)) std::printf("pair: verdict %u matches %u\n", r.verdict, r.n_match);
    std::printf("failed %llu\n", (unsigned long long)failed);
    h.set_report(false);
    h.align_all(t, q);
    try { h.take_report(); } catch (const std::exception&) { std::printf("nothing to take\n"); }
    return 0;
}
"""


def build_shim(tmp_path):
    scrooge_amd.build_library()
    src, exe = str(tmp_path / "report.cpp"), str(tmp_path / "report")
    open(src, "w").write(SHIM_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lscrooge_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_shim_compiles_and_links(tmp_path):
    assert os.path.exists(build_shim(tmp_path))


def test_cli_has_the_flags():
    run = lambda *a: subprocess.run([sys.executable, "-m", "scrooge_amd.cli"] + list(a), capture_output=True, text=True, cwd=ROOT)
    p = run("--help")
    assert p.returncode == 0 and all(f in p.stdout for f in ("--report", "--score", "--verify", "--validate"))
    files = ["--reference=none.fa", "--reads=none.fq", "--seeds=none.paf"]
    for bad in (["--report", "--distance_only"], ["--verify", "--distance_only"], ["--report", "--format=tsv"], ["--report", "--score=1,2,3"],
                ["--report", "--score=a,b,c,d"], ["--score=2,4,4,2"]):
        p = run(*bad, *files)
        assert p.returncode == 2 and ("--report" in p.stderr or "--score" in p.stderr), bad       # an argument error, before anything is loaded
