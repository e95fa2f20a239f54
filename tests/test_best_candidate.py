"""Best-candidate mode (SCRG_OUT_BEST): of every read's candidates only the one with the fewest edits keeps its runs and text,
chosen on the GPU before anything is compacted or transferred (select_kernels.hip, scrg_host.cpp stage 1).

Expected values never come from the code under test: edit distances and CIGARs are the oracle's (or the golden file's), the
expected winner is computed from those by `model_best` below — a plain loop, not api.best_per_read, which is itself tested
against it."""
import ctypes as C
import os

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from scrooge_amd import io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVERFLOW, OVER, NOT_BEST = 0, 6, 7, 8


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_best(ed, over, cand_offsets):
    """-> per read (best pair or -1, best ed or -1, pairs tied at it, second-best ed or -1): eligible = not over the limit,
    the smallest edit distance wins, ties to the lowest index."""
    out = []
    for r in range(len(cand_offsets) - 1):
        el = [(int(ed[p]), p) for p in range(int(cand_offsets[r]), int(cand_offsets[r + 1])) if not over[p]]
        if not el:
            out.append((-1, -1, 0, -1))
            continue
        b, p = min(el)
        above = [e for e, _ in el if e > b]
        out.append((p, b, sum(1 for e, _ in el if e == b), min(above) if above else -1))
    return out


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def header_constant(name):
    import re
    src = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
    assert m, name
    return int(m.group(1))


def test_constants_and_exports():
    lib = api.load_library()
    assert api.SCRG_PAIR_NOT_BEST == header_constant("SCRG_PAIR_NOT_BEST") == 8
    assert api.SCRG_OUT_BEST == header_constant("SCRG_OUT_BEST") == 4
    assert (api.SCRG_OUT_ALL, api.SCRG_OUT_TEXT, api.SCRG_OUT_RUNS) == tuple(header_constant("SCRG_OUT_" + k) for k in ("ALL", "TEXT", "RUNS"))
    for name in ("scrg_select_best", "scrg_host_plan_mapping"):
        assert name in api.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.scrg_status_string(8).decode() not in ("", "unknown status")


@pytest.mark.parametrize("outputs,ok", [(0, True), (1, True), (2, True), (3, False), (4, True), (5, True), (6, True), (7, False), (8, False),
                                        (12, False), (-1, False)])
def test_params_resolve_outputs(outputs, ok):
    lib = api.load_library()
    p, r = api.Params(), api.Params()
    lib.scrg_params_default(C.byref(p))
    p.outputs = outputs
    st = lib.scrg_params_resolve(C.byref(p), C.byref(r))
    assert (st == api.SCRG_OK) == ok
    if ok:
        assert r.outputs == outputs
    else:
        assert st == api.SCRG_ERR_INVALID_ARG


def random_table(rng, sizes, ed_hi, p_over):
    co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(co[-1])
    ed = rng.integers(0, ed_hi, n).astype(np.int64)
    st = np.where(rng.random(n) < p_over, OVER, np.where(rng.random(n) < 0.1, OVERFLOW, OK)).astype(np.uint32)
    return ed, st, co


@pytest.mark.parametrize("seed", range(6))
def test_best_per_read_against_model(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sizes = [0, 1, 2, 64, 65, 5000, 0, 0, 3, 1] + [int(x) for x in rng.integers(0, 9, 200)]
    rng.shuffle(sizes)
    # few distinct distances: ties everywhere; seed 0: no pair over the limit, seed 1: most of them
    ed, st, co = random_table(rng, sizes, ed_hi=(3, 4, 50, 1000, 5, 2)[seed], p_over=(0.0, 0.8, 0.2, 0.2, 0.5, 0.3)[seed])
    # some groups entirely over the limit, and one with every pair at one distance
    for r in (3, 17, 40):
        st[co[r]:co[r + 1]] = OVER
    ed[co[5]:co[6]] = 7
    want = model_best(ed, st == OVER, co)
    assert any(w[0] < 0 for w in want) and any(w[2] > 1 for w in want) and any(w[3] >= 0 for w in want)
    got = api.best_per_read(ed, st, co)
    assert got["best_pair"].tolist() == [w[0] for w in want]
    assert got["best_ed"].tolist() == [w[1] for w in want]
    assert got["n_tied"].tolist() == [w[2] for w in want]
    assert got["second_ed"].tolist() == [w[3] for w in want]
    # a result of the mode itself (losers marked NOT_BEST) gives the same summary
    st2 = st.copy()
    winners = {w[0] for w in want}
    for p in range(len(ed)):
        if st2[p] != OVER and p not in winners:
            st2[p] = NOT_BEST
    again = api.best_per_read(ed, st2, co)
    assert all(again[k].tolist() == got[k].tolist() for k in got)


def test_best_per_read_empty():
    got = api.best_per_read([], [], [0])
    assert all(len(v) == 0 for v in got.values())
    got = api.best_per_read([], [], [0, 0, 0])
    assert got["best_pair"].tolist() == [-1, -1] and got["n_tied"].tolist() == [0, 0]


def host_plan(read_lens, n_devices, **params):
    lib = api.load_library()
    p = api.Params()
    lib.scrg_params_default(C.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    rl = np.ascontiguousarray(read_lens, dtype=np.uint64)
    n = len(rl)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    first = np.zeros(n // 64 + 1024, dtype=np.uint64)
    nc = C.c_uint64(0)
    st = lib.scrg_host_plan(C.byref(p), n_devices, n, None, rl.ctypes.data, order.ctypes.data, first.ctypes.data, len(first), C.byref(nc))
    return st, order[:n], first[:nc.value + 1]


PLAN_COUNTS = [0, 1, 3, 4, 63, 64, 65, 3000]


@pytest.mark.parametrize("n_devices", [1, 2])
@pytest.mark.parametrize("lengths", ["equal", "mixed"])
@pytest.mark.parametrize("sort", [0, 1])
def test_host_plan_mapping(n_devices, lengths, sort):
    rng = np.random.Generator(np.random.PCG64(11 + n_devices))
    counts = PLAN_COUNTS * 12 + [3000] * 20
    rng.shuffle(counts)
    nr = len(counts)
    rl = np.full(nr, 150, dtype=np.uint64) if lengths == "equal" else rng.integers(30, 400, nr).astype(np.uint64)
    co = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(co[-1])
    read_of = np.repeat(np.arange(nr), counts)
    # flag clear: scrg_host_plan's answer for the per-pair read lengths
    order0, first0 = api.host_plan_mapping(rl, co, n_devices, sort_by_length=sort)
    st, order_p, first_p = host_plan(rl[read_of], n_devices, sort_by_length=sort)
    assert st == api.SCRG_OK
    assert order0.tolist() == order_p.tolist() and first0.tolist() == first_p.tolist()
    # flag set
    order, first = api.host_plan_mapping(rl, co, n_devices, sort_by_length=sort, best=True)
    assert order.tolist() == order0.tolist()                         # the issue order is the same: only the cuts move
    assert sorted(order.tolist()) == list(range(n))
    assert first[0] == 0 and first[-1] == n and np.all(np.diff(first.astype(np.int64)) > 0)       # the chunks cover the batch once
    ro = read_of[order]
    for cut in first[1:-1]:
        assert ro[int(cut)] != ro[int(cut) - 1], "a chunk boundary inside a read's candidates"
    # a read's candidates are adjacent, and in caller order
    change = np.flatnonzero(np.diff(ro) != 0) + 1
    assert len(change) + 1 == int(np.sum(np.asarray(counts) > 0)), "a read's candidates are split"
    same = np.diff(ro) == 0
    assert np.all(np.diff(order.astype(np.int64))[same] == 1)
    assert len(first) > 2
    # the first cut is the plain plan's, moved forward to the next read boundary (the later ones start from the moved ones)
    c = int(first0[1])
    while c < n and ro[c] == ro[c - 1]:
        c += 1
    assert int(first[1]) == c
    assert any(int(c) % 64 for c in first[1:-1]), "this batch should need a cut that is no multiple of 64"
    if sort:
        assert np.all(np.diff(rl[ro].astype(np.int64)) <= 0)


def test_host_plan_rejects_the_flag_for_pairs():
    st, _, _ = host_plan([100] * 200, 1, outputs=api.SCRG_OUT_BEST)
    assert st == api.SCRG_ERR_INVALID_ARG
    st, _, _ = host_plan([100] * 200, 1, outputs=api.SCRG_OUT_TEXT | api.SCRG_OUT_BEST)
    assert st == api.SCRG_ERR_INVALID_ARG
    st, _, _ = host_plan([100] * 200, 1, outputs=api.SCRG_OUT_TEXT)
    assert st == api.SCRG_OK


def hand_result(ed, st, cigars):
    """A hand-filled scrg_result: pair p has CIGAR cigars[p] ('' = no runs)."""
    import re
    n = len(ed)
    runs, roff, text, toff = [], [0], b"", [0]
    for c in cigars:
        for cnt, op in re.findall(r"(\d+)([=XID])", c):
            runs.append((int(cnt), op.encode()))
        text += c.encode() + b"\0"
        roff.append(len(runs))
        toff.append(len(text))
    keep = {
        "ed": (C.c_int64 * n)(*ed), "st": (C.c_uint32 * n)(*st), "roff": (C.c_uint64 * (n + 1))(*roff),
        "runs": (api.Run * max(1, len(runs)))(*[api.Run(c, o) for c, o in runs]),
        "toff": (C.c_uint64 * (n + 1))(*toff), "text": C.create_string_buffer(text, len(text) + 1)}
    r = api.Result()
    r.n_pairs = n
    r.edit_distance = C.cast(keep["ed"], C.POINTER(C.c_int64))
    r.pair_status = C.cast(keep["st"], C.POINTER(C.c_uint32))
    r.run_offset = C.cast(keep["roff"], C.POINTER(C.c_uint64))
    r.runs = C.cast(keep["runs"], C.POINTER(api.Run))
    r.cigar_offset = C.cast(keep["toff"], C.POINTER(C.c_uint64))
    r.cigar_text = C.cast(keep["text"], C.POINTER(C.c_char))
    return r, keep


def write_job(tmp_path):
    """Six reads on one 2 kb chromosome with 3, 1, 0, 2, 2, 4 candidates (PAF seeds, both strands)."""
    rng = np.random.Generator(np.random.PCG64(9))
    chrom = synth.random_seq(2000, rng)
    fa, fq, seeds = (str(tmp_path / x) for x in ("g.fa", "r.fq", "s.paf"))
    with open(fa, "w") as f:
        f.write(">chrT test\n%s\n" % chrom.decode())
    counts = [3, 1, 0, 2, 2, 4]
    L = 40
    with open(fq, "w") as f, open(seeds, "w") as s:
        for r, cnt in enumerate(counts):
            start = 100 + 200 * r
            f.write("@r%d\n%s\n+\n%s\n" % (r, chrom[start:start + L].decode(), "I" * L))
            for k in range(cnt):
                s.write("r%d\t%d\t0\t%d\t%s\tchrT\t2000\t%d\t%d\t%d\t%d\t60\n" % (r, L, L, "+-"[(r + k) % 2], start + 7 * k, start + 7 * k + L, L, L))
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    _, reads, cands, names = job.views()
    assert [len(c) for c in cands] == counts and names == ["r%d" % r for r in range(6)]
    return job, chrom, reads, cands, names


COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def todays_lines(job, reads, cands, names, ed, st, cigars, fmt):
    """The writer's rules as they stand without the mode, spelled out: one record per pair; a pair over the edit limit is left
    out of PAF and is an unmapped record (FLAG 4, MAPQ 0, CIGAR *) at its candidate in SAM."""
    import re
    out, k = [], 0
    for r, cs in enumerate(cands):
        for _, rev in cs:
            chrom, ts, clen = job.pair_chromosome(k)
            chrom = chrom.split()[0]              # (the writers name a chromosome by the first word of its FASTA header)
            ops = [(int(c), o) for c, o in re.findall(r"(\d+)([=XID])", cigars[k])]
            tcons = sum(c for c, o in ops if o != "I")
            matches = sum(c for c, o in ops if o == "=")
            cols = sum(c for c, _ in ops)
            seq = reads[r].translate(COMP)[::-1] if rev else reads[r]
            if fmt == "sam":
                if st[k] == OVER:
                    out.append("%s\t%d\t%s\t%d\t0\t*\t*\t0\t0\t%s\t*" % (names[r], 20 if rev else 4, chrom, ts + 1, seq.decode()))
                else:
                    out.append("%s\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t*\tNM:i:%d" % (names[r], 16 if rev else 0, chrom, ts + 1, cigars[k] or "*",
                                                                                 seq.decode(), ed[k]))
            elif st[k] != OVER:
                out.append("%s\t%d\t0\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tNM:i:%d\tcg:Z:%s" % (
                    names[r], len(reads[r]), len(reads[r]), "-" if rev else "+", chrom, clen, ts, ts + tcons, matches, cols, ed[k], cigars[k]))
            k += 1
    return out


def written(job, res, tmp_path, fmt):
    path = str(tmp_path / ("out." + fmt))
    assert job.lib.scrg_job_write(job.h, C.byref(res), path.encode(), 1 if fmt == "sam" else 0) == 0
    return [x for x in open(path).read().splitlines() if not x.startswith("@")]


def test_job_write_without_the_mode_is_unchanged(tmp_path):
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    ed = [k % 4 for k in range(n)]
    st = [OK] * n
    st[4] = OVER
    cigars = ["" if st[k] == OVER else "%d=%dX%d=" % (20 - k, 1 + k % 3, 19 - k % 3) for k in range(n)]
    res, keep = hand_result(ed, st, cigars)
    for fmt in ("paf", "sam"):
        assert written(job, res, tmp_path, fmt) == todays_lines(job, reads, cands, names, ed, st, cigars, fmt)


def test_job_write_best_mode(tmp_path):
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    assert n == 12
    # reads:   r0 (3 cands: winner in the middle, a loser ties it)  r1 (1)   r2 (0)   r3 (2: both over the limit)
    #          r4 (2: winner first, loser worse)   r5 (4: one over the limit, winner last, no tie)
    ed = [2, 2, 5,        0,        9, 9,     1, 3,     4, 30, 4 + 1, 3]
    st = [NOT_BEST, OK, NOT_BEST,   OK,   OVER, OVER,   OK, NOT_BEST,   NOT_BEST, OVER, NOT_BEST, OK]
    # (r0: the tie's winner is written here as pair 1 to show the writer goes by the statuses, not by its own selection)
    cigars = ["40=" if s == OK else "" for s in st]
    res, keep = hand_result(ed, st, cigars)
    winners = [1, 3, 6, 11]
    paf = written(job, res, tmp_path, "paf")
    assert len(paf) == len(winners)
    full = todays_lines(job, reads, cands, names, ed, [OK] * n, ["40="] * n, "paf")
    assert paf == [full[k] + "\ttp:A:P" for k in winners]
    sam = [x.split("\t") for x in written(job, res, tmp_path, "sam")]
    assert [f[0] for f in sam] == names, "one record per read, in read order"
    full_sam = [x.split("\t") for x in todays_lines(job, reads, cands, names, ed, [OK] * n, ["40="] * n, "sam")]
    by_read = {0: (1, 0), 1: (3, 255), 4: (6, 255), 5: (11, 255)}           # read -> (winner, MAPQ): r0's winner is tied
    for r, f in enumerate(sam):
        if r in by_read:
            k, mapq = by_read[r]
            assert f[:4] == full_sam[k][:4] and int(f[4]) == mapq and f[5:] == full_sam[k][5:]
        else:
            assert f == [names[r], "4", "*", "0", "0", "*", "*", "0", "0", reads[r].decode(), "*"]


def test_cli_has_the_flag():
    import subprocess
    import sys
    p = subprocess.run([sys.executable, "-m", "scrooge_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and "--best" in p.stdout


SHIM_SRC = r"""
#include <cstdio>
#include "scrooge_amd.hpp"
int main()
{
    if (scrg_device_count() == 0) { std::fprintf(stderr, "no usable HIP device\n"); return 2; }
    scrooge_amd::Handle h(0);
    Genome_t g;
    g.content = "TTTTTTTTAAAACCCCGGGGTTTTACGTACGTAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA";
    std::vector<Read_t> reads(3);
    reads[0].content = "AAAACCCCGGGGTTTT";
    for (long long s : {7LL, 8LL, 9LL, 8LL}) { CandidateLocation_t c; c.start_in_reference = s; reads[0].locations.push_back(c); }
    reads[1].content = "ACGTACGT";
    reads[2].content = "ACGTACGT";
    for (long long s : {24LL}) { CandidateLocation_t c; c.start_in_reference = s; reads[2].locations.push_back(c); }
    for (const auto& b : h.align_best(g, reads))
        std::printf("best read=%d location=%d cigar=%s edit_distance=%d\n", (int)b.read, (int)b.location, b.alignment.cigar.c_str(),
                    (int)b.alignment.edit_distance);
    return 0;
}
"""


def build_shim(tmp_path):
    import subprocess
    scrooge_amd.build_library()
    src, exe = str(tmp_path / "best.cpp"), str(tmp_path / "best")
    open(src, "w").write(SHIM_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lscrooge_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_shim_align_best_compiles_and_links(tmp_path):
    assert os.path.exists(build_shim(tmp_path))


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def make_mapping(n_reads, lengths, seed, profile, max_cands=8):
    """A genome and reads with 0..max_cands candidates each in SHUFFLED order: the true locus, the true locus shifted by
    +-1..3, random loci, and a duplicate of the true locus (a guaranteed tie).  -> genome, reads, candidates (lists of starts)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    Lmax = max(lengths)
    G = max(20000, 40 * Lmax)
    genome = synth.random_seq(G + 2 * Lmax + 1024, rng)            # (no candidate's text runs into the end of the genome)
    err, ratio = synth.PROFILES[profile] if isinstance(profile, str) else profile
    codes = np.searchsorted(synth.BASES, np.frombuffer(genome, dtype=np.uint8)).astype(np.uint8)
    reads, cands = [], []
    for r in range(n_reads):
        L = int(lengths[r % len(lengths)])
        s = int(rng.integers(8, G - L))
        q = synth.mutate(codes[s:s + 2 * L + 64], err, ratio, rng)[:L]
        assert len(q) == L
        reads.append(synth.BASES[q].tobytes())
        pool = [s, s - int(rng.integers(1, 4)), s + int(rng.integers(1, 4)), int(rng.integers(0, G)), s, s + int(rng.integers(1, 4)),
                int(rng.integers(0, G)), s - int(rng.integers(1, 4))]
        k = 0 if r % 23 == 5 else 1 if r % 23 == 11 else int(rng.integers(1, max_cands + 1))
        pick = [pool[i] for i in rng.permutation(len(pool))[:k]] if k <= len(pool) else pool
        cands.append([int(x) for x in pick])
    return genome, reads, cands


def oracle_mapping(oracle, genome, reads, cands, W=64, O=33, reverse=None):
    texts, qs = [], []
    for r, cs in enumerate(cands):
        for k, c in enumerate(cs):
            q = reads[r]
            if reverse is not None and reverse[r][k]:
                q = q.translate(COMP)[::-1]
            texts.append(genome[c:c + 2 * len(q) + W + 64])
            qs.append(q)
    eds, cigars, _, _ = oracle.align(texts, qs, W=W, O=O, threads=16)
    return eds, cigars


def offsets_of(cands):
    return np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)


def check_best(arr, eds, cigars, co, outputs=0, over=None, over_ed=None, need_ties=True, what=""):
    """Every pair of a best-mode result against the oracle's numbers and the model's winners."""
    n = len(eds)
    over = [False] * n if over is None else over
    want = model_best(eds, over, co)
    winners = {w[0] for w in want if w[0] >= 0}
    if need_ties:
        # the batch holds both kinds before anything is checked
        assert any(w[2] == 1 and w[3] >= 0 for w in want), "no read with a unique winner among several candidates"
        assert any(w[2] > 1 for w in want), "no read with a tie"
    want_runs, want_text = (outputs & 3) != api.SCRG_OUT_TEXT, (outputs & 3) != api.SCRG_OUT_RUNS
    ed, st, ro, to = arr["edit_distance"], arr["status"], arr["run_offset"].astype(np.int64), arr["cigar_offset"].astype(np.int64)
    runs, text = arr["runs"], arr["cigar_text"]
    assert len(ed) == n and len(ro) == n + 1 and len(to) == n + 1
    assert ro[0] == 0 and np.all(np.diff(ro) >= 0) and ro[n] == (len(runs) if want_runs else 0)
    assert to[0] == 0 and np.all(np.diff(to) >= 0) and to[n] == (len(text) if want_text else 0)
    if not want_runs:
        assert not ro.any() and len(runs) == 0
    if not want_text:
        assert not to.any()
    with_runs = 0
    for p in range(n):
        tag = (what, p)
        r_text = "".join("%d%s" % (c, chr(o)) for c, o in runs[ro[p]:ro[p + 1]]) if want_runs else None
        t_text = text[to[p]:to[p + 1] - 1].decode() if want_text else None
        if want_text:
            assert text[to[p + 1] - 1] == 0, tag
        with_runs += 1 if (ro[p + 1] > ro[p] if want_runs else to[p + 1] - to[p] > 1) else 0
        if over[p]:
            assert st[p] == OVER and ed[p] == over_ed[p], tag
            assert r_text in (None, "") and t_text in (None, ""), tag
        elif p in winners:
            assert st[p] == OK and ed[p] == eds[p], tag
            assert r_text in (None, cigars[p]) and t_text in (None, cigars[p]), tag
        else:
            assert st[p] == NOT_BEST and ed[p] == eds[p], tag
            assert r_text in (None, "") and t_text in (None, ""), tag
    assert with_runs == sum(1 for p in winners if cigars[p]), what
    return want


@pytest.fixture(scope="module")
def short_batch(oracle):
    genome, reads, cands = make_mapping(2500, [150], seed=101, profile=(0.03, (1, 0, 0)))
    eds, cigars = oracle_mapping(oracle, genome, reads, cands)
    return genome, reads, cands, eds, cigars


@pytest.fixture(scope="module")
def long_batch(oracle):
    rng = np.random.Generator(np.random.PCG64(7))
    lengths = [int(x) for x in rng.integers(2000, 10001, 60)]            # random length order
    genome, reads, cands = make_mapping(180, lengths, seed=202, profile="ont")
    eds, cigars = oracle_mapping(oracle, genome, reads, cands)
    return genome, reads, cands, eds, cigars


@pytest.mark.gpu
@pytest.mark.parametrize("outputs", [4, 5, 6])
@pytest.mark.parametrize("batch", ["short", "long"])
def test_mapping_vs_oracle(aligner, short_batch, long_batch, outputs, batch):
    genome, reads, cands, eds, cigars = short_batch if batch == "short" else long_batch
    assert any(len(c) == 0 for c in cands) and any(len(c) == 1 for c in cands)
    arr = aligner.align_mapping(genome, reads, cands, arrays=True, outputs=outputs)
    check_best(arr, eds, cigars, offsets_of(cands), outputs, what="%s outputs=%d" % (batch, outputs))
    # the keyword says the same
    arr2 = aligner.align_mapping(genome, reads, cands, arrays=True, outputs=outputs & 3, best=True)
    for k in arr:
        assert np.array_equal(np.asarray(arr[k]), np.asarray(arr2[k])) if k != "cigar_text" else arr[k] == arr2[k]


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [0, 1])
def test_resident_rows_and_sort_order(aligner, long_batch, short_batch, sort):
    for genome, reads, cands, eds, cigars in (long_batch, short_batch):
        co = offsets_of(cands)
        aligner.set_genome(genome)
        try:
            arr = aligner.align_mapping(None, reads, cands, arrays=True, best=True, sort_by_length=sort)
            check_best(arr, eds, cigars, co, what="resident sort=%d" % sort)
            L = max(map(len, reads))
            rows = np.zeros((len(reads), L), dtype=np.uint8)
            for r, q in enumerate(reads):
                rows[r, :len(q)] = np.frombuffer(q, dtype=np.uint8)
            arr = aligner.align_mapping_rows(None, rows, [len(q) for q in reads], co, [c for cs in cands for c in cs], best=True,
                                             sort_by_length=sort)
            check_best(arr, eds, cigars, co, what="resident rows sort=%d" % sort)
        finally:
            aligner.clear_genome()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0], [0, 0]])
@pytest.mark.parametrize("lanes", [1, 64])
def test_stranded_multi(aligner, oracle, devices, lanes):
    genome, reads, cands = make_mapping(1200 if lanes == 1 else 300, [150, 90, 333], seed=303, profile=(0.03, (1, 0, 0)))
    rng = np.random.Generator(np.random.PCG64(4))
    reverse = [[int(rng.random() < 0.4) for _ in cs] for cs in cands]
    # a read stored as its reverse complement: its minus-strand candidates are the true ones
    for r in range(0, len(reads), 3):
        reads[r] = reads[r].translate(COMP)[::-1]
        reverse[r] = [1 - x for x in reverse[r]]
    eds, cigars = oracle_mapping(oracle, genome, reads, cands, reverse=reverse)
    arr = aligner.align_mapping_multi(devices, genome, reads, cands, reverse=reverse, arrays=True, best=True, lanes_per_pair=lanes)
    check_best(arr, eds, cigars, offsets_of(cands), what="multi %r lanes=%d" % (devices, lanes))
    api.load_library().scrg_multi_release()


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (64, 2), (192, 97), (256, 127)])
def test_kernel_classes(aligner, oracle, W, O):
    genome, reads, cands = make_mapping(400, [150, 700, 2500], seed=404 + W + O, profile="ont")
    eds, cigars = oracle_mapping(oracle, genome, reads, cands, W=W, O=O)
    arr = aligner.align_mapping(genome, reads, cands, arrays=True, best=True, W=W, O=O)
    check_best(arr, eds, cigars, offsets_of(cands), what="W=%d O=%d" % (W, O))


@pytest.mark.gpu
def test_lanes_per_pair_64(aligner, short_batch):
    genome, reads, cands, eds, cigars = short_batch
    reads, cands = reads[:300], cands[:300]
    n = sum(len(c) for c in cands)
    arr = aligner.align_mapping(genome, reads, cands, arrays=True, best=True, lanes_per_pair=64)
    check_best(arr, eds[:n], cigars[:n], offsets_of(cands), what="lanes_per_pair=64")


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_groups_larger_than_a_chunk(aligner, oracle, devices):
    """40 reads x 3 000 candidates of a 50 bp read: groups span wavefronts, workgroups and what would be chunk cuts; the winner
    (the true locus, once) first, last or somewhere inside, the rest random loci and, for some reads, a later duplicate of it."""
    rng = np.random.Generator(np.random.PCG64(55))
    G, L, K = 30000, 50, 3000
    genome = synth.random_seq(G + 1024, rng)
    reads, cands = [], []
    for r in range(40):
        s = int(rng.integers(0, G - L))
        q = bytearray(genome[s:s + L])
        q[7] = ord("A") if q[7] != ord("A") else ord("C")
        reads.append(bytes(q))
        cs = [int(x) for x in rng.integers(0, G, K)]
        cs[(0, K - 1, int(rng.integers(1, K - 1)))[r % 3]] = s
        if r % 4 == 0:
            cs[K - 2 if r % 3 != 1 else 5] = s          # the same locus again: a tie across many wavefronts
        cands.append(cs)
    cands[3], cands[20] = cands[3][:1], []
    co = offsets_of(cands)
    # every distinct (read, locus) once through the oracle
    uniq = {}
    for r, cs in enumerate(cands):
        for c in cs:
            uniq.setdefault((r, c), len(uniq))
    keys = list(uniq)
    e_u, c_u = oracle_mapping(oracle, genome, [reads[r] for r, _ in keys], [[c] for _, c in keys])
    eds = [e_u[uniq[(r, c)]] for r, cs in enumerate(cands) for c in cs]
    cigars = [c_u[uniq[(r, c)]] for r, cs in enumerate(cands) for c in cs]
    _, first = api.host_plan_mapping([len(q) for q in reads], co, 1 if devices is None else len(devices), best=True)
    assert len(first) > 2, "the batch should be cut into several chunks"
    if devices is None:
        arr = aligner.align_mapping(genome, reads, cands, arrays=True, best=True)
    else:
        arr = aligner.align_mapping_multi(devices, genome, reads, cands, arrays=True, best=True)
        api.load_library().scrg_multi_release()
    want = check_best(arr, eds, cigars, co, what="large groups")
    pos = [w[0] - int(co[r]) for r, w in enumerate(want) if w[0] >= 0 and co[r + 1] - co[r] == K]
    assert 0 in pos and K - 1 in pos and any(0 < p < K - 1 for p in pos)


@pytest.mark.gpu
def test_with_an_edit_limit(aligner, short_batch):
    from tests.test_edit_limit import window_model
    genome, reads, cands, eds, cigars = short_batch
    co = offsets_of(cands)
    for max_edits in (12, 2):
        over, over_ed = [], []
        for p in range(len(eds)):
            o, e = window_model(cigars[p], max_edits)
            over.append(bool(o))
            over_ed.append(e)
        want = model_best(eds, over, co)
        assert any(w[0] < 0 and co[r + 1] > co[r] for r, w in enumerate(want)), "no read with every candidate over the limit"
        assert any(over) and not all(over)
        arr = aligner.align_mapping(genome, reads, cands, arrays=True, best=True, max_edits=max_edits)
        check_best(arr, eds, cigars, co, over=over, over_ed=over_ed, need_ties=max_edits == 12, what="max_edits=%d" % max_edits)
        # winners within the limit: the same pair as without a limit wherever that pair is within the limit
        free = model_best(eds, [False] * len(eds), co)
        assert all(w[0] == f[0] for w, f in zip(want, free) if f[0] >= 0 and not over[f[0]])


@pytest.mark.gpu
def test_golden_mapping_grouped_by_read(aligner, golden_mapping):
    gm = golden_mapping
    co = offsets_of(gm["candidates"])
    arr = aligner.align_mapping(gm["genome"], gm["reads"], gm["candidates"], arrays=True, best=True)
    check_best(arr, gm["ed"], gm["cigar"], co, need_ties=False, what="golden")
    got = api.best_per_read(arr["edit_distance"], arr["status"], co)
    assert got["best_pair"].tolist() == [w[0] for w in model_best(gm["ed"], [False] * len(gm["ed"]), co)]


@pytest.mark.gpu
def test_rejected_on_pairwise_calls(aligner):
    with pytest.raises(scrooge_amd.ScroogeError):
        aligner.align_pairs(["ACGTACGT"], ["ACGTACG"], best=True)
    with pytest.raises(scrooge_amd.ScroogeError):
        aligner.align_pairs_multi([0], ["ACGTACGT"], ["ACGTACG"], outputs=api.SCRG_OUT_BEST)
    api.load_library().scrg_multi_release()
    assert aligner.align_pairs(["ACGTACGT"], ["ACGTACG"]) == [("7=", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("edits", [False, True])
def test_select_best_device_layer(aligner, oracle, edits):
    """scrg_select_best after scrg_align_device / scrg_align_device_edits, then scrg_compact_runs: the dense array holds the
    winners' runs, in order, and nothing else."""
    import torch
    dev = torch.device("cuda", aligner.device)
    rng = np.random.Generator(np.random.PCG64(77))
    sizes = [1, 2, 64, 65, 300, 1, 1, 130] + [int(x) for x in rng.integers(1, 9, 150)]
    texts, reads, key = [], [], []
    for g, sz in enumerate(sizes):
        t, q = synth.make_pairs(1, 120, "ont", seed=1000 + g)
        for k in range(sz):
            # the group's read against its own text, shifted copies of it and unrelated texts
            kind = int(rng.integers(0, 4))
            texts.append(t[0] if kind == 0 else t[0][1:] if kind == 1 else b"A" + t[0] if kind == 2 else synth.random_seq(len(t[0]), rng))
            reads.append(q[0])
            key.append(7 * g + 3 if g % 5 else 12)          # (keys repeat in non-adjacent groups: only runs of equal keys are groups)
    n = len(texts)
    co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    eds, cigars, _, _ = oracle.align(texts, reads, threads=16)
    max_edits = 30 if not edits else None
    from tests.test_edit_limit import window_model
    over, over_ed = zip(*[window_model(c, max_edits) for c in cigars])
    want = model_best(eds, over, co)
    winners = sorted(w[0] for w in want if w[0] >= 0)
    assert any(w[2] > 1 for w in want) and any(w[2] == 1 and w[3] >= 0 for w in want)
    assert edits or (any(over) and any(w[0] < 0 for w in want))

    tw, rw = (max(map(len, texts)) + 31) // 32, (max(map(len, reads)) + 31) // 32
    wpr = tw + rw
    rows = np.zeros((n, wpr * 32), dtype=np.uint8)
    for k in range(n):
        rows[k, :len(texts[k])] = np.frombuffer(texts[k], dtype=np.uint8)
        rows[k, tw * 32: tw * 32 + len(reads[k])] = np.frombuffer(reads[k], dtype=np.uint8)
    saved = getattr(aligner, "_stream", None)
    aligner.set_stream(0)
    try:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        seq = torch.zeros(n * wpr + api.SEQ_PAD_WORDS, dtype=torch.int64, device=dev)
        aligner.pack_planar(torch.from_numpy(rows).to(dev).view(-1), seq, bad)
        idx = np.arange(n, dtype=np.int64)
        cap = (2 * rw * 32 + 16 + 15) // 16 * 16
        desc = np.stack([idx * wpr * 32, np.array([len(x) for x in texts]), (idx * wpr + tw) * 32, np.array([len(x) for x in reads]),
                         idx * cap, np.full(n, cap)], axis=1).astype(np.int64)
        desc_t = torch.from_numpy(desc).to(dev)
        slices = torch.zeros(n * cap * 2, dtype=torch.uint8, device=dev)
        ed = torch.empty(n, dtype=torch.int64, device=dev)
        ln = torch.empty(n, dtype=torch.int32, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        if edits:
            rc = torch.empty(n, dtype=torch.int32, device=dev)
            aligner.align_device_edits(n, seq, desc_t, slices, ed, ln, st, rc)
        else:
            aligner.align_device(n, seq, desc_t, slices, ed, ln, st, max_edits=max_edits)
        torch.cuda.synchronize()
        before = slices.cpu().numpy().copy()
        ln_before = ln.cpu().numpy().copy()
        key_t = torch.from_numpy(np.asarray(key, dtype=np.int32)).to(dev)
        is_best = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        aligner.select_best(n, key_t, ed, st, ln, is_best)
        torch.cuda.synchronize()
        assert int(bad) == 0
        got_best = is_best.cpu().numpy()
        assert np.flatnonzero(got_best).tolist() == winners and set(got_best.tolist()) <= {0, 1}
        st_h, ln_h, ed_h = st.cpu().numpy(), ln.cpu().numpy(), ed.cpu().numpy()
        for p in range(n):
            if over[p]:
                assert (st_h[p], ed_h[p], ln_h[p]) == (2, over_ed[p], 0), p
            elif got_best[p]:
                assert (st_h[p], ed_h[p], ln_h[p]) == (0, eds[p], ln_before[p]) and ln_h[p] > 0, p
            else:
                assert (st_h[p], ed_h[p], ln_h[p]) == (3, eds[p], 0), p
        assert np.array_equal(slices.cpu().numpy(), before)            # the slices themselves are not touched
        if edits:
            for p in winners:
                stream = before[2 * p * cap: 2 * p * cap + int(ln_h[p])].tobytes()
                assert api.edit_stream_to_cigar(stream, len(reads[p])) == cigars[p], p
        else:
            off = torch.cumsum(ln.to(torch.int64), 0) - ln.to(torch.int64)
            total = int(ln.sum())
            dense = torch.zeros(max(total, 1) * 2, dtype=torch.uint8, device=dev)
            aligner.compact_runs(n, desc_t, slices, ln, off, dense)
            torch.cuda.synchronize()
            d = dense.cpu().numpy()[:2 * total]
            assert "".join("%d%s" % (d[2 * q], chr(d[2 * q + 1])) for q in range(total)) == "".join(cigars[p] for p in winners)
    finally:
        aligner.restore_stream(saved)


SHIM_EXPECTED = [
    "best read=0 location=1 cigar=16= edit_distance=0",
    "best read=2 location=0 cigar=8= edit_distance=0",
]


@pytest.mark.gpu
def test_shim_align_best_runs(tmp_path):
    import subprocess
    p = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip().splitlines() == SHIM_EXPECTED
