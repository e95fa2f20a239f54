"""scrg_job_write_paired without a GPU: a hand-built result and hand-built mate records on a two-chromosome job give a SAM whose
FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT and TLEN columns equal a table written out here — a plain proper pair, an absent mate, a
"proper" pair whose mates lie on different chromosomes, and equal starts — and a PAF of the winners; the loader's refusal of an
odd number of reads."""
import ctypes as C

import numpy as np
import pytest

from scrooge_amd import api, synth
from scrooge_amd import io as sio
from tests import mate_model as mm
from tests.test_best_candidate import COMP, hand_result

L = 40
NONE = api.MATES_NONE
# per read: its candidates as (strand, chromosome, start in the chromosome)
READS = [
    [("+", "chrA", 100)], [("-", "chrA", 300), ("+", "chrA", 500)],          # mate pair 0: proper, FR; read 1's second candidate loses
    [("+", "chrA", 600)], [],                                                # mate pair 1: read 3 has no candidate
    [("+", "chrA", 900)], [("-", "chrB", 50)],                               # mate pair 2: 190 apart in the concatenated coordinate
    [("-", "chrB", 400)], [("+", "chrB", 400)],                              # mate pair 3: equal starts, tied
]


def write_job(tmp_path, reads=READS):
    rng = np.random.Generator(np.random.PCG64(21))
    chroms = {"chrA": synth.random_seq(1000, rng), "chrB": synth.random_seq(1000, rng)}
    fa, fq, seeds = (str(tmp_path / x) for x in ("g.fa", "r.fq", "s.paf"))
    with open(fa, "w") as f:
        for name, seq in chroms.items():
            f.write(">%s some words\n%s\n" % (name, seq.decode()))
    seqs = []
    with open(fq, "w") as f, open(seeds, "w") as s:
        for r, cs in enumerate(reads):
            seqs.append(synth.random_seq(L, rng))
            f.write("@r%d\n%s\n+\n%s\n" % (r, seqs[-1].decode(), "I" * L))
            for strand, chrom, start in cs:
                s.write("r%d\t%d\t0\t%d\t%s\t%s\t1000\t%d\t%d\t%d\t%d\t60\n" % (r, L, L, strand, chrom, start, start + L, L, L))
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    assert job.n_reads == len(reads) and job.n_pairs == sum(len(c) for c in reads) and job.n_chromosomes == 2
    return job, seqs


def hand_mates(records):
    arr = np.zeros(len(records), dtype=api.mate_dtype())
    for m, (winner, cost, second, span, n_proper, flags) in enumerate(records):
        arr[m] = (winner, cost, second, span, n_proper, flags, 0)
    return api.Mates(len(arr), arr.ctypes.data), arr


def write_paired(job, res, mates, path, fmt):
    sio._lib()
    st = job.lib.scrg_job_write_paired(job.h, C.byref(res), C.byref(mates), path.encode(), fmt)
    return st, ([x.split("\t") for x in open(path).read().splitlines() if not x.startswith("@")] if st == 0 else None)


def hand_case():
    #          k0     k1          k2   k3       k4     k5     k6     k7
    cigars = ["40=", "20=2D20=", "", "39=1X", "40=", "40=", "40=", "40="]
    ed = [0, 2, 5, 1, 0, 0, 0, 0]
    st = [0, 0, api.SCRG_PAIR_NOT_BEST, 0, 0, 0, 0, 0]
    both = mm.HAS_A | mm.HAS_B
    records = [((0, 1), 2, 0xffffffff, 242, 1, mm.PROPER | both), ((3, NONE), 1, 0xffffffff, 0, 0, mm.HAS_A),
               ((4, 5), 0, 0xffffffff, 190, 1, mm.PROPER | both), ((6, 7), 0, 0, 40, 2, mm.PROPER | both | mm.TIED)]
    return cigars, ed, st, records


def test_the_sam_columns_of_a_paired_result(tmp_path):
    job, seqs = write_job(tmp_path)
    cigars, ed, st, records = hand_case()
    res, keep = hand_result(ed, st, cigars)
    mates, keep_mates = hand_mates(records)
    s, sam = write_paired(job, res, mates, str(tmp_path / "p.sam"), 1)
    assert s == 0 and len(sam) == 8
    # name, FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN
    table = [
        ("r0", 0x1 | 0x40 | 0x2 | 0x20, "chrA", 101, 255, "40=", "=", 301, 242),             # leftmost: + (100 .. 300 + 42)
        ("r1", 0x1 | 0x80 | 0x2 | 0x10, "chrA", 301, 255, "20=2D20=", "=", 101, -242),
        ("r2", 0x1 | 0x40 | 0x8, "chrA", 601, 255, "39=1X", "*", 0, 0),                      # its mate has no winner
        ("r3", 0x1 | 0x80 | 0x4, "*", 0, 0, "*", "chrA", 601, 0),                            # no winner: unmapped, the mate named
        ("r4", 0x1 | 0x40 | 0x20, "chrA", 901, 255, "40=", "chrB", 51, 0),                   # PROPER in the record, another chromosome: no 0x2, no TLEN
        ("r5", 0x1 | 0x80 | 0x10, "chrB", 51, 255, "40=", "chrA", 901, 0),
        ("r6", 0x1 | 0x40 | 0x2 | 0x10, "chrB", 401, 0, "40=", "=", 401, 40),                # equal starts: the sign goes to mate 1; TIED: MAPQ 0
        ("r7", 0x1 | 0x80 | 0x2 | 0x20, "chrB", 401, 0, "40=", "=", 401, -40),
    ]
    assert [tuple(x[:9]) for x in sam] == [tuple(str(v) for v in row) for row in table]
    # the sequence is the read as aligned; NM is the winner's distance; an unmapped record has no tag
    assert sam[1][9] == seqs[1].translate(COMP)[::-1].decode() and sam[0][9] == seqs[0].decode() and sam[3][9] == seqs[3].decode()
    assert [x[11:] for x in sam] == [["NM:i:0"], ["NM:i:2"], ["NM:i:1"], [], ["NM:i:0"], ["NM:i:0"], ["NM:i:0"], ["NM:i:0"]]
    header = [x for x in open(str(tmp_path / "p.sam")).read().splitlines() if x.startswith("@SQ")]
    assert header == ["@SQ\tSN:chrA\tLN:1000", "@SQ\tSN:chrB\tLN:1000"]


def test_the_paf_of_a_paired_result_holds_the_winners(tmp_path):
    job, _ = write_job(tmp_path)
    cigars, ed, st, records = hand_case()
    res, keep = hand_result(ed, st, cigars)
    mates, keep_mates = hand_mates(records)
    s, paf = write_paired(job, res, mates, str(tmp_path / "p.paf"), 0)
    assert s == 0 and [x[0] for x in paf] == ["r0", "r1", "r2", "r4", "r5", "r6", "r7"]
    assert paf[1][:12] == ["r1", "40", "0", "40", "-", "chrA", "1000", "300", "342", "40", "42", "255"]
    assert paf[1][12:] == ["NM:i:2", "cg:Z:20=2D20=", "tp:A:P"] and all(x[-1] == "tp:A:P" for x in paf)


def test_the_paired_writer_refuses(tmp_path):
    job, _ = write_job(tmp_path)
    cigars, ed, st, records = hand_case()
    res, keep = hand_result(ed, st, cigars)
    mates, keep_mates = hand_mates(records)
    path = str(tmp_path / "x.out")
    assert write_paired(job, res, mates, path, 2)[0] == api.SCRG_ERR_INVALID_ARG                       # no TSV of a paired result
    short, keep_short = hand_mates(records[:3])
    assert write_paired(job, res, short, path, 1)[0] == api.SCRG_ERR_INVALID_ARG                       # records of another job
    wrong, keep_wrong = hand_mates([((2, 1), 2, 0xffffffff, 242, 1, mm.PROPER)] + records[1:])         # pair 2 is read 1's, not read 0's
    assert write_paired(job, res, wrong, path, 1)[0] == api.SCRG_ERR_INVALID_ARG
    past, keep_past = hand_mates([((0, 99), 2, 0xffffffff, 242, 1, mm.PROPER)] + records[1:])
    assert write_paired(job, res, past, path, 1)[0] == api.SCRG_ERR_INVALID_ARG
    tend = (C.c_uint64 * 9)()
    res.text_end = C.cast(tend, C.POINTER(C.c_uint64))                                                # a distance-only result has no CIGARs
    assert write_paired(job, res, mates, path, 1)[0] == api.SCRG_ERR_INVALID_ARG


def test_an_odd_number_of_reads_is_a_format_error(tmp_path):
    """scrg_job_align_paired: reads 2m and 2m+1 are mates, so three reads are no interleaved FASTQ — refused before anything runs
    (no handle is needed to find out), and nothing is left to take."""
    job, _ = write_job(tmp_path, READS[:3])
    sio._lib()
    res, mt = C.POINTER(api.Result)(), C.POINTER(api.Mates)()
    # (the out pointers start as garbage that must not survive)
    junk = api.Mates(1, 0)
    mt.contents = junk
    p = api.Params()
    job.lib.scrg_params_default(C.byref(p))
    st = job.lib.scrg_job_align_paired(None, C.byref(p), job.h, None, C.byref(mt), C.byref(res))
    assert st == sio.SCRG_ERR_FORMAT and not mt and not res
    assert hasattr(sio.Job, "align_paired")
