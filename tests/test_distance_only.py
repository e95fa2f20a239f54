"""Distance-only mode (SCRG_OUT_DISTANCE, include/scrooge_amd.h): edit distance, status and text end of every pair, no CIGARs.

Expected values come from the reference, never from the library's own runs mode: the edit distance is the reference's `ed`
and text_end is the sum of the '=', 'X' and 'D' counts of the reference's CIGAR — from the committed goldens (which the
reference wrote) or from oracle.pyoracle.Oracle (pinned to the reference by tests/test_oracle.py and tests/test_plane.py).  The
one exception is the running sum an over-limit pair reports: the reference has no limit, so there the library's runs mode and
the window-end model of tests/test_edit_limit.py are the comparison.  Every pair is compared, none is left out."""
import ctypes as C
import functools
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from tests import plane_inputs as pi
from tests import refill_inputs as ri
from tests.conftest import GOLDEN
from tests.test_best_candidate import (hand_result, host_plan, make_mapping, offsets_of, oracle_mapping, todays_lines, write_job)
from tests.test_edit_limit import pack_sequences, revcomp, window_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVER, NOT_BEST = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST
DIST = 16


def text_end_of(cigar):
    """The text characters a CIGAR consumes: its '=', 'X' and 'D' counts."""
    return sum(int(c) for c, o in re.findall(r"(\d+)([=XID])", cigar) if o != "I")


# ================================================================================================================ CPU
def test_text_end_of():
    assert text_end_of("") == 0 and text_end_of("31I13I16=2I2I") == 16 and text_end_of("4=1I11=1D11=1X2=") == 30


@pytest.mark.parametrize("outputs,ok", [(16, True), (20, True), (17, False), (18, False), (19, False), (21, False), (22, False), (23, False),
                                        (24, False), (28, False), (32, False), (48, False)])
def test_params_resolve_accepts_16_and_20(outputs, ok):
    lib = api.load_library()
    p, r = api.Params(), api.Params()
    lib.scrg_params_default(C.byref(p))
    p.outputs = outputs
    st = lib.scrg_params_resolve(C.byref(p), C.byref(r))
    if ok:
        assert st == api.SCRG_OK and r.outputs == outputs
    else:
        assert st == api.SCRG_ERR_INVALID_ARG


def test_header_library_and_binding_have_the_entry_point():
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    assert re.search(r"scrg_status\s+scrg_align_device_distance\s*\(", hdr)
    assert re.search(r"\bSCRG_OUT_DISTANCE\s*=\s*16\b", hdr) and api.SCRG_OUT_DISTANCE == DIST
    assert re.search(r"uint64_t\s*\*\s*text_end;", hdr)
    assert "scrg_align_device_distance" in api.EXPORTED_SYMBOLS and hasattr(lib, "scrg_align_device_distance")
    assert api.Result._fields_[-1][0] == "text_end"               # the struct grew at its end
    assert hasattr(api.Aligner, "align_device_distance")


@pytest.mark.parametrize("n_devices", [1, 2])
@pytest.mark.parametrize("sort", [0, 1])
def test_host_plans_do_not_move_with_the_flag(n_devices, sort):
    rng = np.random.Generator(np.random.PCG64(5 + n_devices))
    rl = rng.integers(30, 12000, 5000).astype(np.uint64)
    st0, order0, first0 = host_plan(rl, n_devices, sort_by_length=sort)
    st1, order1, first1 = host_plan(rl, n_devices, sort_by_length=sort, outputs=DIST)
    assert st0 == st1 == api.SCRG_OK and len(first0) > 2
    assert order0.tolist() == order1.tolist() and first0.tolist() == first1.tolist()
    assert host_plan(rl, n_devices, outputs=DIST | api.SCRG_OUT_BEST)[0] == api.SCRG_ERR_INVALID_ARG      # (pairs have no groups: as without the flag)
    counts = rng.integers(0, 9, 1500)
    rl = rng.integers(30, 400, len(counts)).astype(np.uint64)
    co = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    for best in (False, True):
        o0, f0 = api.host_plan_mapping(rl, co, n_devices, sort_by_length=sort, best=best)
        o1, f1 = api.host_plan_mapping(rl, co, n_devices, sort_by_length=sort, best=best, distance_only=True)
        assert o0.tolist() == o1.tolist() and f0.tolist() == f1.tolist() and len(f0) > 2


def write(job, res, tmp_path, fmt):
    """-> (status, the file's bytes or None)."""
    path = str(tmp_path / ("w." + fmt))
    if os.path.exists(path):
        os.remove(path)
    st = job.lib.scrg_job_write(job.h, C.byref(res), path.encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
    return st, (open(path, "rb").read() if os.path.exists(path) else None)


# the job of tests/test_best_candidate.py: six reads of 40 bp with 3, 1, 0, 2, 2, 4 candidates on chrT, candidate k of read r at
# 100 + 200 r + 7 k, strand "+-"[(r + k) % 2] — spelled out here so that the expected lines are hand-made
JOB_PAIRS = [(r, 100 + 200 * r + 7 * k, "+-"[(r + k) % 2]) for r, cnt in enumerate([3, 1, 0, 2, 2, 4]) for k in range(cnt)]


def tsv_lines(keep, ed, span):
    return "".join("r%d\t40\t%s\tchrT\t%d\t%d\t%d\n" % (JOB_PAIRS[k][0], JOB_PAIRS[k][2], JOB_PAIRS[k][1], JOB_PAIRS[k][1] + span[k], ed[k])
                   for k in keep).encode()


def test_job_write_tsv_from_runs(tmp_path):
    """A result with runs and no text_end: target end = start + the text the runs consume (hand-computed spans)."""
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    assert n == len(JOB_PAIRS) == 12
    cigars = ["40=", "10=2D30=", "5=3I32=", "40I", "1X39=", "20=1D1X1I18=", "", "38=2I", "2D40=", "17=6D23=", "39=1X", "1D1I39="]
    span = [40, 42, 37, 0, 40, 40, 0, 38, 42, 46, 40, 40]                       # by hand: '=' + 'X' + 'D'
    ed = [0, 2, 3, 40, 1, 3, 9, 2, 2, 6, 1, 2]
    st = [OK] * n
    st[6] = OVER
    res, keep = hand_result(ed, st, cigars)
    assert not res.text_end
    s, got = write(job, res, tmp_path, "tsv")
    assert s == 0 and got == tsv_lines([k for k in range(n) if k != 6], ed, span)
    # best mode: the winners only, as PAF
    st = [NOT_BEST, OK, NOT_BEST, OK, OVER, OVER, OK, NOT_BEST, NOT_BEST, OVER, NOT_BEST, OK]
    cig2 = [c if s == OK else "" for c, s in zip(cigars, st)]
    cig2[6] = "40="
    res, keep = hand_result(ed, st, cig2)
    s, got = write(job, res, tmp_path, "tsv")
    span2 = list(span)
    span2[6] = 40
    assert s == 0 and got == tsv_lines([1, 3, 6, 11], ed, span2)


def distance_result(ed, st, tend):
    n = len(ed)
    res, keep = hand_result(ed, st, [""] * n)
    keep["roff"] = (C.c_uint64 * (n + 1))()
    keep["toff"] = (C.c_uint64 * (n + 1))()
    keep["tend"] = (C.c_uint64 * n)(*tend)
    res.run_offset = C.cast(keep["roff"], C.POINTER(C.c_uint64))
    res.cigar_offset = C.cast(keep["toff"], C.POINTER(C.c_uint64))
    res.text_end = C.cast(keep["tend"], C.POINTER(C.c_uint64))
    return res, keep


def test_job_write_tsv_of_a_distance_result_and_nothing_else(tmp_path):
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    ed = [0, 2, 3, 40, 1, 3, 9, 2, 2, 6, 1, 2]
    tend = [40, 42, 37, 0, 40, 40, 0, 38, 42, 46, 40, 40]
    st = [OK] * n
    st[6] = OVER
    res, keep = distance_result(ed, st, tend)
    s, got = write(job, res, tmp_path, "tsv")
    assert s == 0 and got == tsv_lines([k for k in range(n) if k != 6], ed, tend)
    for fmt in ("paf", "sam"):                                  # PAF columns 10 and 11 and a SAM CIGAR cannot be made from a distance
        s, got = write(job, res, tmp_path, fmt)
        assert s == api.SCRG_ERR_INVALID_ARG and got is None
    # mode 20: winners only; a loser's and an over-limit pair's text_end (0) is never printed
    st = [NOT_BEST, OK, NOT_BEST, OK, OVER, OVER, OK, NOT_BEST, NOT_BEST, OVER, NOT_BEST, OK]
    tend = [t if s == OK else 0 for t, s in zip([40, 42, 37, 1, 40, 40, 41, 38, 42, 46, 40, 40], st)]
    res, keep = distance_result(ed, st, tend)
    s, got = write(job, res, tmp_path, "tsv")
    assert s == 0 and got == tsv_lines([1, 3, 6, 11], ed, tend)


def test_job_write_paf_and_sam_of_a_result_without_text_end_are_what_they_were(tmp_path):
    """Byte for byte: the writer's rules spelled out (tests/test_best_candidate.py: todays_lines) + the SAM header."""
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    ed = [k % 4 for k in range(n)]
    st = [OK] * n
    st[4] = OVER
    cigars = ["" if st[k] == OVER else "%d=%dX1D%d=2I" % (20 - k, 1 + k % 3, 16 - k % 3) for k in range(n)]
    res, keep = hand_result(ed, st, cigars)
    assert not res.text_end
    s, paf = write(job, res, tmp_path, "paf")
    assert s == 0 and paf == "".join(x + "\n" for x in todays_lines(job, reads, cands, names, ed, st, cigars, "paf")).encode()
    s, sam = write(job, res, tmp_path, "sam")
    head = "@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chrT\tLN:2000\n@PG\tID:scrooge_amd\tPN:scrooge_amd\n"
    assert s == 0 and sam == (head + "".join(x + "\n" for x in todays_lines(job, reads, cands, names, ed, st, cigars, "sam"))).encode()


def test_cli_has_the_flag():
    run = lambda *a: subprocess.run([sys.executable, "-m", "scrooge_amd.cli"] + list(a), capture_output=True, text=True, cwd=ROOT)
    p = run("--help")
    assert p.returncode == 0 and "--distance_only" in p.stdout and "tsv" in p.stdout
    files = ["--reference=none.fa", "--reads=none.fq", "--seeds=none.paf"]
    p = run("--distance_only", "--validate", *files)
    assert p.returncode == 2 and "--validate" in p.stderr            # an argument error, before anything is loaded
    p = run("--distance_only", "--format=sam", *files)
    assert p.returncode == 2 and "tsv" in p.stderr


SHIM_SRC = r"""
#include <cstdio>
#include "scrooge_amd.hpp"
int main()
{
    if (scrg_device_count() == 0) { std::fprintf(stderr, "no usable HIP device\n"); return 2; }
    scrooge_amd::Handle h(0);
    std::vector<std::string> t = {"AAAACCCCGGGGTTTT", "ACGTACGT"}, q = {std::string(44, 'T') + "AAAACCCCGGGGTTTTAAAA", "ACGTACG"};
    for (const auto& d : h.align_distances(t, q))
        std::printf("pair edit_distance=%d text_end=%d over=%d\n", (int)d.edit_distance, (int)d.text_end, (int)d.over_edit_limit);
    h.set_edit_limit(30);
    for (const auto& d : h.align_distances(t, q))
        std::printf("limit30 edit_distance=%d text_end=%d over=%d\n", (int)d.edit_distance, (int)d.text_end, (int)d.over_edit_limit);
    h.set_edit_limit();
    Genome_t g;
    g.content = "TTTTTTTTAAAACCCCGGGGTTTTACGTACGT" + std::string(96, 'A');
    std::vector<Read_t> reads(2);
    reads[0].content = "AAAACCCCGGGGTTTT";
    for (long long s : {7LL, 8LL}) { CandidateLocation_t c; c.start_in_reference = s; reads[0].locations.push_back(c); }
    reads[1].content = "ACGTACGT";
    for (long long s : {24LL}) { CandidateLocation_t c; c.start_in_reference = s; reads[1].locations.push_back(c); }
    for (const auto& d : h.align_distances(g, reads))
        std::printf("mapping edit_distance=%d text_end=%d over=%d\n", (int)d.edit_distance, (int)d.text_end, (int)d.over_edit_limit);
    return 0;
}
"""


def build_shim(tmp_path):
    scrooge_amd.build_library()
    src, exe = str(tmp_path / "dist.cpp"), str(tmp_path / "dist")
    open(src, "w").write(SHIM_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lscrooge_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_shim_align_distances_compiles_and_links(tmp_path):
    assert os.path.exists(build_shim(tmp_path))


# ================================================================================================================ GPU
def check_arrays(arr, want_ed, want_te, what, want_st=None):
    """A flagged host call's arrays: every pair's distance, status and text end; no runs, no text, all-zero offsets."""
    n = len(want_ed)
    assert len(arr["edit_distance"]) == len(arr["status"]) == len(arr["text_end"]) == n, what
    assert arr["run_offset"].shape == (n + 1,) and not arr["run_offset"].any() and arr["runs"].shape == (0, 2), what
    assert arr["cigar_offset"].shape == (n + 1,) and not arr["cigar_offset"].any() and arr["cigar_text"] == b"", what
    want_st = np.zeros(n, dtype=np.int64) if want_st is None else np.asarray(want_st)
    bad = np.flatnonzero((arr["edit_distance"] != np.asarray(want_ed)) | (arr["text_end"].astype(np.int64) != np.asarray(want_te)) |
                         (arr["status"] != want_st))
    assert len(bad) == 0, "%s: %d of %d pairs differ; first: pair %d got (ed %d, status %d, text_end %d) want (%d, %d, %d)" % (
        what, len(bad), n, bad[0], arr["edit_distance"][bad[0]], arr["status"][bad[0]], arr["text_end"][bad[0]], want_ed[bad[0]],
        want_st[bad[0]], want_te[bad[0]])


PAIR_GOLDENS = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "pairs_w*_o*.json")))


def test_every_golden_is_listed():
    assert len(PAIR_GOLDENS) == 16 and len(pi.SETTINGS) == 58
    classes = {pi.kernel_class(*(int(x) for x in re.match(r"pairs_w(\d+)_o(\d+)", f).groups())) for f in PAIR_GOLDENS}
    assert classes == set(pi.CLASSES), "the pair goldens reach all four kernels"


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAIR_GOLDENS)
def test_golden_pairs(aligner, name):
    with open(os.path.join(GOLDEN, name)) as f:
        g = json.load(f)
    cases = g["cases"]
    arr = aligner.align_pairs([c["text"] for c in cases], [c["read"] for c in cases], arrays=True, W=g["W"], O=g["O"], distance_only=True)
    check_arrays(arr, [c["ed"] for c in cases], [text_end_of(c["cigar"]) for c in cases], name)
    # the list form: CIGAR "", and the text ends beside it
    alns = aligner.align_pairs([c["text"] for c in cases[:5]], [c["read"] for c in cases[:5]], W=g["W"], O=g["O"], distance_only=True)
    assert [(a.cigar, a.edit_distance) for a in alns] == [("", c["ed"]) for c in cases[:5]]
    assert aligner.last_text_end == [text_end_of(c["cigar"]) for c in cases[:5]]


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", pi.SETTINGS, ids=["%d-%d" % s for s in pi.SETTINGS])
def test_golden_plane(aligner, oracle, W, O):
    """The fixture stores a long CIGAR as its hash: the oracle's CIGAR is taken where it IS the reference's (same_cigar holds it
    to the stored text or hash), and the edit distance is the fixture's own."""
    from tests.test_plane import load
    t, q, groups, fx = load(W, O)
    eds, cigars, _, _ = oracle.align(t, q, W=W, O=O, threads=8)
    assert all(pi.same_cigar(c, s) for c, s in zip(cigars, fx["cigar"])) and list(eds) == list(fx["ed"])
    arr = aligner.align_pairs(t, q, arrays=True, W=W, O=O, distance_only=True)
    check_arrays(arr, fx["ed"], [text_end_of(c) for c in cigars], "plane %d/%d (%s)" % (W, O, pi.kernel_class(W, O)))


@pytest.mark.gpu
def test_golden_mapping(aligner, golden_mapping):
    g = golden_mapping
    arr = aligner.align_mapping(g["genome"], g["reads"], g["candidates"], arrays=True, W=g["W"], O=g["O"], distance_only=True)
    check_arrays(arr, g["ed"], [text_end_of(c) for c in g["cigar"]], "mapping golden")
    aligner.set_genome(g["genome"])
    try:
        arr = aligner.align_mapping(None, g["reads"], g["candidates"], arrays=True, W=g["W"], O=g["O"], distance_only=True)
    finally:
        aligner.clear_genome()
    check_arrays(arr, g["ed"], [text_end_of(c) for c in g["cigar"]], "mapping golden, resident genome")


# ---- seeded random batches against the oracle
SETTINGS = [(64, 33), (64, 2), (24, 0), (128, 65), (128, 20), (256, 129), (256, 1)]


@functools.lru_cache(maxsize=1)
def seeded_batch():
    """ONT and PacBio profiles, 150 bp to 10 kb in mixed order, an empty read, an empty text, texts that end inside a window
    (the read outlasts them) -> texts, reads, rev (which pairs the stranded launches take as reverse complements)."""
    rng = np.random.Generator(np.random.PCG64(2024))
    texts, reads = [], []
    lengths = [150, 151, 333, 1000, 2500, 10_000, 640, 64, 63, 65, 4097]
    for k in range(230):
        err, ratio = synth.PROFILES["ont" if k % 2 else "pacbio"]
        t, q = synth.make_pair(lengths[k % len(lengths)] if k != 7 else 10_000, err, ratio, rng)
        texts.append(synth.BASES[t].tobytes()), reads.append(synth.BASES[q].tobytes())
    for cut in (1, 17, 40, 100, 129, 300):                       # the text ends inside a window, the read goes on
        t, q = synth.make_pair(400 + cut, *synth.PROFILES["ont"], rng)
        texts.append(synth.BASES[t].tobytes()[:200 + cut]), reads.append(synth.BASES[q].tobytes())
    texts += [b"ACGTACGTAC", b"", b"", b"T" * 300]
    reads += [b"", b"ACGTTGCA", b"", b"T" * 300]
    rev = rng.random(len(texts)) < 0.4
    return texts, reads, rev


_oracle_cache = {}


def oracle_for(oracle, W, O, stranded=False):
    """(ed, text_end, cigars) of the seeded batch at W/O, once per setting."""
    key = (W, O, stranded)
    if key not in _oracle_cache:
        texts, reads, rev = seeded_batch()
        if stranded:
            reads = [revcomp(r) if v else r for r, v in zip(reads, rev)]
        eds, cigars, _, _ = oracle.align(texts, reads, W=W, O=O, threads=16)
        _oracle_cache[key] = (np.array(eds, dtype=np.int64), np.array([text_end_of(c) for c in cigars], dtype=np.int64), cigars)
    return _oracle_cache[key]


def test_seeded_batch_holds_what_it_says():
    texts, reads, rev = seeded_batch()
    rl, tl = np.array([len(x) for x in reads]), np.array([len(x) for x in texts])
    assert rl.min() == 0 and tl.min() == 0 and rl.max() >= 10_000 and ((rl >= 150) & (rl <= 10_000)).sum() > 150
    assert ((tl > 0) & (rl > tl + 64)).sum() >= 6 and 0.2 < rev.mean() < 0.6 and len(texts) > 192       # more than one block of four wavefronts


def device_distance(al, texts, reads, W, O, layout, rev=None, max_edits=None, perm=None, packed=None, select=0, waves_per_cu=0,
                    with_text_end=True, **params):
    """One scrg_align_device_distance launch -> (ed, status, text_end) as numpy arrays, per descriptor.  The descriptors carry
    cigar_off = cigar_cap = 0 (they are not looked at); the status and text-end arrays are pre-filled with a pattern."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    seq, t_off, r_off, stride = packed if packed is not None else pack_sequences(al, texts, reads, layout)
    read_len = np.array([len(x) for x in reads], dtype=np.uint64)
    text_len = np.array([len(x) for x in texts], dtype=np.uint64)
    perm = np.arange(len(texts), dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)
    n = len(perm)
    r_off = r_off.astype(np.uint64)
    if rev is not None:
        r_off = r_off | np.where(np.asarray(rev), np.uint64(api.READ_REVCOMP), np.uint64(0)).astype(np.uint64)
    zero = np.zeros(n, dtype=np.uint64)
    desc = np.stack([t_off.astype(np.uint64)[perm], text_len[perm], r_off[perm], read_len[perm], zero, zero], axis=1)
    desc_t = torch.from_numpy(desc.view(np.int64)).to(dev)
    ed = torch.full((n,), -7, dtype=torch.int64, device=dev)
    te = torch.full((n,), -7, dtype=torch.int32, device=dev) if with_text_end else None
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    kw = dict(W=W, O=O, text_stride_words=stride, read_stride_words=stride, stranded=int(rev is not None), **params)
    if waves_per_cu:
        kw["waves_per_cu"] = waves_per_cu
    p = al._params(kw)
    p.reserved[0] = select
    with al._call_limit(max_edits, None):
        al._check(api._lazy(al.lib, "scrg_align_device_distance")(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, ed, te, st)]))
        torch.cuda.synchronize()
    return ed.cpu().numpy(), st.cpu().numpy(), (te.cpu().numpy().astype(np.int64) if te is not None else None)


def compare_device(got, want_ed, want_te, what, want_st=None):
    ed, st, te = got
    want_st = np.zeros(len(ed), dtype=np.int64) if want_st is None else want_st
    bad = np.flatnonzero((ed != want_ed) | (st != want_st) | ((te != want_te) if te is not None else False))
    assert len(bad) == 0, "%s: %d of %d descriptors differ; first: %d got (ed %d, status %d, text_end %s) want (%d, %d, %d)" % (
        what, len(bad), len(ed), bad[0], ed[bad[0]], st[bad[0]], te[bad[0]] if te is not None else "-", want_ed[bad[0]], want_st[bad[0]],
        want_te[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
@pytest.mark.parametrize("W,O", SETTINGS)
def test_seeded_batches_device(aligner, oracle, W, O, layout):
    texts, reads, rev = seeded_batch()
    ed, te, _ = oracle_for(oracle, W, O)
    packed = pack_sequences(aligner, texts, reads, layout)
    compare_device(device_distance(aligner, texts, reads, W, O, layout, packed=packed), ed, te, "%d/%d %s" % (W, O, layout))
    # d_text_end may be NULL; waves_per_cu as in the other modes (one wavefront per CU: the 240 pairs share four wavefronts)
    got = device_distance(aligner, texts, reads, W, O, layout, packed=packed, with_text_end=False, waves_per_cu=1)
    compare_device(got, ed, te, "%d/%d %s, no text_end, waves_per_cu = 1" % (W, O, layout))
    assert aligner.last_kernel_ms() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", SETTINGS)
def test_seeded_batches_host(aligner, oracle, W, O):
    texts, reads, rev = seeded_batch()
    ed, te, _ = oracle_for(oracle, W, O)
    check_arrays(aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, distance_only=True), ed, te, "host %d/%d" % (W, O))
    check_arrays(aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, distance_only=True, sort_by_length=0), ed, te,
                 "host %d/%d, caller order" % (W, O))


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (64, 2), (128, 65), (256, 129), (256, 1)])
def test_reverse_strand(aligner, oracle, W, O):
    """Minus-strand pairs from the one packed copy of the read, against the oracle on the reverse-complemented string."""
    texts, reads, rev = seeded_batch()
    ed, te, _ = oracle_for(oracle, W, O, stranded=True)
    for layout in ("contiguous", "groups"):
        compare_device(device_distance(aligner, texts, reads, W, O, layout, rev=rev), ed, te, "stranded %d/%d %s" % (W, O, layout))


@pytest.fixture(scope="module")
def mapping_batch(oracle):
    """Reads with 0..8 candidates (true locus, shifted, random, duplicates: ties), both strands."""
    genome, reads, cands = make_mapping(700, [150, 400], seed=303, profile=(0.04, (1, 1, 1)))
    rng = np.random.Generator(np.random.PCG64(8))
    reverse = [[int(rng.random() < 0.3) for _ in c] for c in cands]
    eds, cigars = oracle_mapping(oracle, genome, reads, cands, reverse=reverse)
    f_eds, f_cigars = oracle_mapping(oracle, genome, reads, cands)
    return genome, reads, cands, reverse, np.array(eds, dtype=np.int64), cigars, np.array(f_eds, dtype=np.int64), f_cigars


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_multi(aligner, oracle, mapping_batch, devices):
    texts, reads, rev = seeded_batch()
    ed, te, _ = oracle_for(oracle, 64, 33)
    check_arrays(aligner.align_pairs_multi(devices, texts, reads, arrays=True, distance_only=True), ed, te, "pairs_multi %r" % devices)
    genome, mreads, cands, reverse, eds, cigars, _, _ = mapping_batch
    arr = aligner.align_mapping_multi(devices, genome, mreads, cands, reverse=reverse, arrays=True, distance_only=True)
    check_arrays(arr, eds, [text_end_of(c) for c in cigars], "mapping_multi %r, stranded" % devices)


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (64, 2), (256, 129), (256, 1)])
def test_edit_limit(aligner, oracle, W, O):
    """Over-limit pairs: status 7, text_end 0 and the running sum that runs mode reports (the reference has no limit: the one
    place where the library's runs mode is the comparison — and the window-end model of the reference's CIGAR agrees); pairs
    within the limit are as without a limit."""
    texts, reads, rev = seeded_batch()
    ed, te, cigars = oracle_for(oracle, W, O)
    lim = int(np.median(ed))
    runs = aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, max_edits=lim, outputs=api.SCRG_OUT_RUNS)
    over = runs["status"] == OVER
    assert 0.2 * len(ed) < over.sum() < 0.8 * len(ed) and (over == (ed > lim)).all()
    model = np.array([window_model(c, lim, W, O)[1] for c in cigars], dtype=np.int64)
    assert (runs["edit_distance"] == model).all()
    want_ed, want_te, want_st = np.where(over, runs["edit_distance"], ed), np.where(over, 0, te), np.where(over, OVER, OK)
    check_arrays(aligner.align_pairs(texts, reads, arrays=True, W=W, O=O, max_edits=lim, distance_only=True), want_ed, want_te,
                 "limit %d at %d/%d" % (lim, W, O), want_st)
    got = device_distance(aligner, texts, reads, W, O, "groups", max_edits=lim)
    compare_device(got, want_ed, want_te, "device, limit %d at %d/%d" % (lim, W, O), np.where(over, api.DEVICE_STATUS_OVER_EDIT_LIMIT, 0))
    assert aligner.edit_limit() == (None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("limit", [None, 12])
def test_mode_20_against_best_per_read(aligner, mapping_batch, limit):
    """SCRG_OUT_DISTANCE | SCRG_OUT_BEST: api.best_per_read applied to the oracle's distances names the winners."""
    genome, reads, cands, _, _, _, eds, cigars = mapping_batch          # (scrg_align_mapping: forward candidates)
    co = offsets_of(cands)
    n = len(eds)
    over = (eds > limit) if limit is not None else np.zeros(n, dtype=bool)
    over_ed = np.array([window_model(c, limit)[1] for c in cigars], dtype=np.int64)
    want = api.best_per_read(eds, np.where(over, OVER, OK), co)
    winners = want["best_pair"][want["best_pair"] >= 0]
    assert (want["n_tied"] > 1).any(), "the batch holds no tie"
    if limit is not None:
        all_over = [r for r in range(len(cands)) if len(cands[r]) > 0 and over[co[r]:co[r + 1]].all()]
        assert all_over and (want["best_pair"][all_over] == -1).all(), "no read with every candidate over the limit"
    want_st = np.full(n, NOT_BEST, dtype=np.int64)
    want_st[over] = OVER
    want_st[winners] = OK
    want_te = np.zeros(n, dtype=np.int64)
    want_te[winners] = [text_end_of(cigars[k]) for k in winners]
    want_ed = np.where(over, over_ed, eds)
    arr = aligner.align_mapping(genome, reads, cands, arrays=True, best=True, distance_only=True, max_edits=limit)
    check_arrays(arr, want_ed, want_te, "mode 20, limit %r" % limit, want_st)
    # the flag is rejected on pairwise calls only in combination with BEST, as today
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        aligner.align_pairs([b"ACGT"], [b"ACGT"], outputs=DIST | api.SCRG_OUT_BEST)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 64])
def test_genasm_row_mappings_refuse_the_mode(aligner, lanes):
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        aligner.align_pairs([b"ACGTACGTAA"], [b"ACGTACGT"], lanes_per_pair=lanes, distance_only=True)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        device_distance(aligner, [b"ACGTACGTAA"], [b"ACGTACGT"], 64, 33, "contiguous", lanes_per_pair=lanes)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    assert [a.edit_distance for a in aligner.align_pairs([b"ACGTACGTAA"], [b"ACGTACGT"], lanes_per_pair=lanes)] == [0]


@pytest.mark.gpu
def test_query_launch_reports_the_modes_geometry(aligner):
    """LDS per wavefront shrinks to what the table needs: Eq region and "no match" words (and, parts kernel, the text)."""
    want = {(64, 33): (64 * 144, 64 * 40), (64, 2): (64 * 144, 64 * 40), (128, 65): (64 * 184, 64 * 80),
            (256, 129): (64 * (88 + 160 + 64), 64 * (160 + 64)), (256, 1): (64 * (68 + 260), 0)}
    for (W, O), (runs_lds, dist_lds) in want.items():
        assert aligner.query_launch(W=W, O=O)["lds_bytes"] == runs_lds, (W, O)
        q = aligner.query_launch(W=W, O=O, distance_only=True)
        assert q["lds_bytes"] == dist_lds and q["pairs_per_wave"] == 64 and q["n_waves"] > 0, (W, O)


# ---- the work queue's refill path (tests/test_queue_refill.py, tests/refill_inputs.py) in distance mode, on each kernel form
REFILL_CASES = [("default", 64, 33, "groups", ""), ("default", 64, 33, "contiguous", "stranded"), ("default", 64, 33, "contiguous", "limit"),
                ("halves", 64, 2, "contiguous", ""), ("halves", 128, 65, "groups", ""), ("parts", 256, 129, "groups", ""),
                ("hbm", 256, 1, "contiguous", "")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", REFILL_CASES, ids=lambda c: "-".join(str(x) for x in c if x != ""))
def test_lanes_refill_from_the_queue(aligner, oracle, case):
    from tests.test_queue_refill import launch_slots, over_limit, packed_base
    kernel, W, O, layout, mode = case
    assert pi.kernel_class(W, O) == kernel
    base = ri.base_set()
    stranded = mode == "stranded"
    stride = 64 if layout == "groups" else 1
    slots = launch_slots(aligner, 0, W=W, O=O, waves_per_cu=1, text_stride_words=stride, read_stride_words=stride, distance_only=True)
    n = 3 * slots + 37
    assert slots >= ri.SLOTS_MIN and n % 64 != 0
    perm = ri.build_batch(base, n, seed=500 + REFILL_CASES.index(case), slots=slots)
    facts = ri.batch_facts(base, perm)
    assert facts["first_round"] >= 1 and facts["tail"] >= 1, facts
    exp = ri.expected(oracle, base, W, O, stranded)
    if "text_end" not in exp:
        r = exp["runs"].reshape(-1, 2)
        per_run = np.where(r[:, 1] != ord("I"), r[:, 0], 0).astype(np.int64)
        exp["text_end"] = np.concatenate([[0], np.cumsum(per_run)])[exp["run_off"][1:]] - np.concatenate([[0], np.cumsum(per_run)])[exp["run_off"][:-1]]
        k = int(np.argmax(base["read_len"]))
        assert exp["text_end"][k] == text_end_of(exp["cigars"][k]) and exp["text_end"][3] == text_end_of(exp["cigars"][3])
    want_ed, want_te, want_st, max_edits = exp["ed"][perm], exp["text_end"][perm], np.zeros(n, dtype=np.int64), None
    if mode == "limit":
        max_edits = int(np.median(exp["ed"]))
        over, over_ed = over_limit(exp, max_edits)
        want_ed, want_te = np.where(over[perm], over_ed[perm], want_ed), np.where(over[perm], 0, want_te)
        want_st = np.where(over[perm], api.DEVICE_STATUS_OVER_EDIT_LIMIT, 0)
        assert 0.1 * n < over[perm].sum() < 0.9 * n
    got = device_distance(aligner, base["texts"], base["reads"], W, O, layout, rev=base["rev"] if stranded else None, max_edits=max_edits,
                          perm=perm, packed=packed_base(aligner, base, layout), waves_per_cu=1)
    print("%d descriptors on %d slots, kernel %.1f ms" % (n, slots, aligner.last_kernel_ms()))
    compare_device(got, want_ed, want_te, "refill %r" % (case,), want_st)


@pytest.mark.gpu
def test_shim_align_distances_runs(tmp_path, oracle):
    p = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    # the pairs: the golden pair of tests/test_edit_limit.py (31I13I16=2I2I, 48 edits; 31 at the first window end over a limit of 30)
    genome = b"TTTTTTTTAAAACCCCGGGGTTTTACGTACGT" + b"A" * 96
    eds, cigars, _, _ = oracle.align([genome[7:], genome[8:], genome[24:]], [b"AAAACCCCGGGGTTTT", b"AAAACCCCGGGGTTTT", b"ACGTACGT"])
    assert p.stdout.strip().splitlines() == [
        "pair edit_distance=48 text_end=16 over=0", "pair edit_distance=0 text_end=7 over=0",
        "limit30 edit_distance=31 text_end=0 over=1", "limit30 edit_distance=0 text_end=7 over=0"] + [
        "mapping edit_distance=%d text_end=%d over=0" % (e, text_end_of(c)) for e, c in zip(eds, cigars)]


@pytest.mark.gpu
def test_cli_distance_only(tmp_path, capsys, oracle):
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=12, seed=9)
    out = str(tmp_path / "o.tsv")
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--out=" + out, "--distance_only", "--reverse_strand"]) == 0
    capsys.readouterr()
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    genome, reads, cands, names = job.views()
    texts, qs = [], []
    for r, cs in zip(reads, cands):
        for start, rv in cs:
            q = r.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1] if rv else r
            texts.append(genome[start:start + 2 * len(q) + 128]), qs.append(q)
    eds, cigars, _, _ = oracle.align(texts, qs)
    lines = [x.split("\t") for x in open(out).read().splitlines()]
    assert len(lines) == job.n_pairs == len(eds)
    for k, f in enumerate(lines):
        assert len(f) == 7 and int(f[6]) == eds[k] and int(f[5]) - int(f[4]) == text_end_of(cigars[k]), (k, f)
