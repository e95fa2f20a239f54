"""scrg_job_write_mapq without a GPU: a hand-built result of best-candidate mode and hand-built read summaries on a tiny job give a
SAM whose column 5 and a PAF whose column 12 equal a table written out here — a unique winner, a tied one (0), a read without a
winner (unmapped, 0), one capped by its own edit rate; without summaries the file is scrg_job_write_report's byte for byte; a
wrong number of reads, a winner that is not the result's, a result that is not best-candidate mode's and TSV are refused."""
import ctypes as C

import numpy as np

from scrooge_amd import api
from scrooge_amd import io as sio
from tests import mapq_model as mq
from tests.test_best_candidate import hand_result, write_job

NB, OVER = api.SCRG_PAIR_NOT_BEST, api.SCRG_PAIR_OVER_EDIT_LIMIT
#           r0: 3 candidates         r1    r3: tie       r4: all over      r5: 4 candidates, the winner capped by its own edits
CIGARS = ["", "40=", "",             "40=", "39=1X", "", "", "",           "", "", "30=6X4=", ""]
ED = [4, 0, 2,                       0,     1, 1,        9, 9,             9, 30, 6, 7]
ST = [NB, 0, NB,                     0,     0, NB,       OVER, OVER,       NB, NB, 0, NB]
FIRST = [0, 3, 4, 4, 6, 8, 12]
L = 40


def hand_summaries(rule=mq.DEFAULT_RULE, n_reads=None, patch=None):
    recs = mq.summarise_all(rule, FIRST, [L] * len(ED), ED, [s != OVER for s in ST])
    arr = np.zeros(len(recs) if n_reads is None else n_reads, dtype=api.read_summary_dtype())
    for r, w in enumerate(recs[:len(arr)]):
        arr[r] = mq.as_tuple(w) + (0,)
    for r, field, value in patch or ():
        arr[field][r] = value
    sm = api.ReadSummaries(len(arr), arr.ctypes.data, api.MapqRule(*rule).as_c())
    return sm, arr


def write(job, res, sm, path, fmt):
    sio._lib()
    st = job.lib.scrg_job_write_mapq(job.h, C.byref(res), None, None, None, C.byref(sm) if sm is not None else None, path.encode(), fmt)
    return st, ([x.split("\t") for x in open(path).read().splitlines() if not x.startswith("@")] if st == 0 else None)


def test_the_table_is_the_rule(tmp_path):
    _, arr = hand_summaries()
    # read: mapq — r0: best 0, second 2: min(60, 20); r1: alone: 60; r2: nothing; r3: tied; r4: none eligible;
    # r5: best 6 of 40 bases: cap = 60 - 60 * 1000 * 6 / (250 * 40) = 24, second 7: min(24, 10)
    assert arr["mapq"].tolist() == [20, 60, 0, 0, 0, 10]
    assert mq.mapq(mq.DEFAULT_RULE, L, True, 1, 6, None) == 24


def test_sam_column_5_and_paf_column_12(tmp_path):
    job, chrom, reads, cands, names = write_job(tmp_path)
    res, keep = hand_result(ED, ST, CIGARS)
    sm, arr = hand_summaries()
    st, sam = write(job, res, sm, str(tmp_path / "m.sam"), 1)
    assert st == 0
    # name, FLAG & 4, MAPQ, CIGAR
    table = [("r0", 0, 20, "40="), ("r1", 0, 60, "40="), ("r2", 4, 0, "*"), ("r3", 0, 0, "39=1X"), ("r4", 4, 0, "*"), ("r5", 0, 10, "30=6X4=")]
    assert [(x[0], int(x[1]) & 4, int(x[4]), x[5]) for x in sam] == table
    st, paf = write(job, res, sm, str(tmp_path / "m.paf"), 0)
    assert st == 0 and [(x[0], int(x[11])) for x in paf] == [("r0", 20), ("r1", 60), ("r3", 0), ("r5", 10)]
    assert all(x[-1] == "tp:A:P" for x in paf)
    # a capped one: with a rule that lets the second placement say nothing, the winner's own edit rate is what is left
    capped, arr = hand_summaries((255, 60, 250, 0))
    st, sam = write(job, res, capped, str(tmp_path / "c.sam"), 1)
    assert st == 0 and [int(x[4]) for x in sam] == [60, 60, 0, 0, 0, 24]
    # the other columns and tags are scrg_job_write's
    plain = str(tmp_path / "plain.sam")
    assert job.lib.scrg_job_write(job.h, C.byref(res), plain.encode(), 1) == 0
    old = [x.split("\t") for x in open(plain).read().splitlines() if not x.startswith("@")]
    assert [x[:4] + x[5:] for x in old] == [x[:4] + x[5:] for x in sam] and [int(x[4]) for x in old] == [255, 255, 0, 0, 0, 255]


def test_without_summaries_it_is_the_report_writer_byte_for_byte(tmp_path):
    job, chrom, reads, cands, names = write_job(tmp_path)
    res, keep = hand_result(ED, ST, CIGARS)
    for fmt in (0, 1, 2):
        a, b = str(tmp_path / ("a%d" % fmt)), str(tmp_path / ("b%d" % fmt))
        assert write(job, res, None, a, fmt)[0] == 0
        assert job.lib.scrg_job_write_report(job.h, C.byref(res), None, None, None, b.encode(), fmt) == 0
        assert open(a, "rb").read() == open(b, "rb").read() and len(open(a, "rb").read()) > 0


def test_the_mapq_writer_refuses(tmp_path):
    job, chrom, reads, cands, names = write_job(tmp_path)
    res, keep = hand_result(ED, ST, CIGARS)
    sm, arr = hand_summaries()
    path = str(tmp_path / "x.out")
    assert write(job, res, sm, path, 2)[0] == api.SCRG_ERR_INVALID_ARG                                  # TSV has no such column
    short, keep_short = hand_summaries(n_reads=5)
    assert write(job, res, short, path, 1)[0] == api.SCRG_ERR_INVALID_ARG                               # summaries of another job
    wrong, keep_wrong = hand_summaries(patch=[(0, "winner", 2)])
    assert write(job, res, wrong, path, 1)[0] == api.SCRG_ERR_INVALID_ARG                               # not this result's winner
    none, keep_none = hand_summaries(patch=[(2, "winner", 3)])
    assert write(job, res, none, path, 1)[0] == api.SCRG_ERR_INVALID_ARG
    plain_st = [0 if s == NB else s for s in ST]                                                       # every candidate of a read kept: no best-mode result
    res2, keep2 = hand_result(ED, plain_st, ["40="] * len(ED))
    assert write(job, res2, sm, path, 1)[0] == api.SCRG_ERR_INVALID_ARG
    assert write(job, res, sm, path, 1)[0] == 0
