"""Difference strings: SAM's MD:Z: and PAF's short cs:Z: of every pair, rendered on the GPU next to the CIGAR text
(scrooge_amd/csrc/diff_kernels.hip; scrg_ctx_set_diff / scrg_ctx_take_diff, scrg_diff_lengths / scrg_diff_render,
scrg_diff_from_runs, scrg_job_write_diff).

Expected strings come from tests/diff_model.py, a Python model written from the rules; it does not call the library.  The align
kernels are not under test here: wherever a call aligns, the runs of its own result are the model's input."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from tests import diff_model as dm
from tests.test_best_candidate import hand_result, offsets_of, write_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVER, NOT_BEST = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST
KINDS = ["md", "cs"]
NEW_API = ["scrg_ctx_set_diff", "scrg_ctx_get_diff", "scrg_ctx_take_diff", "scrg_diff_free", "scrg_diff_lengths", "scrg_diff_render"]
NEW_IO = ["scrg_job_write_diff", "scrg_diff_from_runs"]


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_model_reproduces_the_table():
    for text, read, cigar, md, cs in dm.TABLE:
        runs = dm.parse(cigar)
        assert dm.model("md", text, read, runs) == md and dm.model("cs", text, read, runs) == cs, cigar
        assert dm.apply_cs(text, cs) == (read, dm.consumed(runs)[0]) and dm.md_text_consumed(md) == dm.consumed(runs)[0], cigar
    assert dm.model("md", "ACGT", "", []) == "" and dm.model("cs", "ACGT", "", []) == ""
    assert dm.model("md", "A" * 50, "A" * 50, dm.parse("29=21=")) == "50"          # runs are never merged across windows; the numbers are


def test_header_library_and_bindings_have_the_entry_points(lib):
    from scrooge_amd import io as sio
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    for name in NEW_API:
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    for name in NEW_IO:
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS, name
    assert re.search(r"enum\s*\{\s*SCRG_DIFF_OFF\s*=\s*0,\s*SCRG_DIFF_MD\s*=\s*1,\s*SCRG_DIFF_CS\s*=\s*2\s*\}", hdr)
    assert (api.DIFF_OFF, api.DIFF_MD, api.DIFF_CS) == (0, 1, 2)
    # the feature is new entry points only: no struct of the interface moved
    assert lib.scrg_abi_version() == 8 == api.SCRG_ABI_VERSION
    assert api.Result._fields_[-1][0] == "text_end" and C.sizeof(api.Params) == 48
    assert C.sizeof(api.Diff) == 32


def host_diff(lib, kind, text, read, runs, cap=None, canary=0xEE):
    """scrg_diff_from_runs -> (status, measured length, the buffer's bytes); cap: the capacity passed (default: what was measured)."""
    text, read = text.encode(), read.encode()
    arr = (api.Run * max(1, len(runs)))(*[api.Run(c, o.encode()) for c, o in runs])
    fn = api._lazy(lib, "scrg_diff_from_runs")
    need = C.c_uint64(0)
    st = fn(api._diff_kind(kind), text, len(text), read, len(read), C.cast(arr, C.c_void_p), len(runs), None, 0, C.byref(need))
    if st != 0:
        return st, None, None
    room = int(need.value) + 8
    buf = (C.c_uint8 * room)(*([canary] * room))
    got = C.c_uint64(0)
    st = fn(api._diff_kind(kind), text, len(text), read, len(read), C.cast(arr, C.c_void_p), len(runs), C.cast(buf, C.c_void_p),
            int(need.value) if cap is None else cap, C.byref(got))
    assert got.value == need.value
    return st, int(need.value), bytes(buf)


@pytest.mark.parametrize("kind", KINDS)
def test_diff_from_runs_table(lib, kind):
    for text, read, cigar, md, cs in dm.TABLE:
        want = md if kind == "md" else cs
        st, n, buf = host_diff(lib, kind, text, read, dm.parse(cigar))
        assert st == 0 and n == len(want) + 1 and buf[:n] == want.encode() + b"\0" and set(buf[n:]) == {0xEE}, cigar
        assert api.diff_from_runs(kind, text, read, cigar) == want
    assert host_diff(lib, kind, "ACGT", "", [])[:2] == (0, 1)                      # no runs: ""


@pytest.mark.parametrize("kind", KINDS)
def test_diff_from_runs_random(lib, kind):
    """2 000 random valid run lists of 0..400 runs, counts 1..255, all four operations: the model's string, the measured length,
    and a capacity one short of it."""
    rng = np.random.Generator(np.random.PCG64(4711))
    seen = set()
    for k in range(2000):
        text, read, runs = dm.random_case(rng, int(rng.integers(0, 401)))
        want = dm.model(kind, text, read, runs).encode() + b"\0"
        st, n, buf = host_diff(lib, kind, text, read, runs)
        assert st == 0 and n == len(want) and buf[:n] == want and set(buf[n:]) == {0xEE}, k
        if k % 50 == 0:
            st, n, buf = host_diff(lib, kind, text, read, runs, cap=len(want) - 1)
            assert st != 0 and n == len(want) and set(buf[len(want) - 1:]) == {0xEE}, k       # an error, nothing past cap touched
        seen.update(o for _, o in runs)
    assert seen == set("=XID")


def test_diff_from_runs_rejects_what_is_no_alignment(lib):
    assert host_diff(lib, "md", "ACG", "ACGT", [(4, "=")])[0] == api.SCRG_ERR_INVALID_ARG          # one text base short
    assert host_diff(lib, "cs", "ACGT", "ACG", [(3, "="), (1, "X")])[0] == api.SCRG_ERR_INVALID_ARG  # one read base short
    assert host_diff(lib, "md", "ACGT", "ACGT", [(4, "M")])[0] == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        api.diff_from_runs("long", "ACGT", "ACGT", "4=")


def hand_diff(kind, strings):
    text = b"".join(s.encode() + b"\0" for s in strings)
    off = np.concatenate([[0], np.cumsum([len(s) + 1 for s in strings])]).astype(np.uint64)
    keep = {"off": (C.c_uint64 * len(off))(*[int(x) for x in off]), "text": C.create_string_buffer(text, len(text) + 1)}
    d = api.Diff()
    d.n_pairs, d.kind = len(strings), api._diff_kind(kind)
    d.offset = C.cast(keep["off"], C.POINTER(C.c_uint64))
    d.text = C.cast(keep["text"], C.POINTER(C.c_char))
    return d, keep


def write_with(job, res, diff, tmp_path, fmt, name):
    path = str(tmp_path / (name + "." + fmt))
    if os.path.exists(path):
        os.remove(path)
    fn = api._lazy(job.lib, "scrg_job_write_diff")
    st = fn(job.h, C.byref(res), C.byref(diff) if diff is not None else None, path.encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
    return st, (open(path, "rb").read() if os.path.exists(path) else None)


@pytest.mark.parametrize("kind", KINDS)
def test_job_write_diff(tmp_path, kind):
    """A hand-built result and diff: every line is scrg_job_write's line plus the tag; an unmapped SAM record has none."""
    job, chrom, reads, cands, names = write_job(tmp_path)
    n = job.n_pairs
    ed = [k % 4 for k in range(n)]
    st = [OK] * n
    st[4] = OVER
    cigars = ["" if st[k] == OVER else "%d=%dX1D%d=2I" % (20 - k, 1 + k % 3, 16 - k % 3) for k in range(n)]
    res, keep = hand_result(ed, st, cigars)
    strings = ["" if st[k] == OVER else "%s-string-%d" % (kind, k) for k in range(n)]          # (the writer copies what the diff holds)
    diff, keep_d = hand_diff(kind, strings)
    tag = "\tMD:Z:" if kind == "md" else "\tcs:Z:"
    for fmt in ("paf", "sam"):
        path = str(tmp_path / ("plain." + fmt))
        assert job.lib.scrg_job_write(job.h, C.byref(res), path.encode(), 1 if fmt == "sam" else 0) == 0
        plain = open(path, "rb").read()
        s, same = write_with(job, res, None, tmp_path, fmt, "null")
        assert s == 0 and same == plain                                        # diff == NULL: scrg_job_write exactly
        s, got = write_with(job, res, diff, tmp_path, fmt, "diff")
        assert s == 0
        want, k = [], 0
        kept = [p for p in range(n) if fmt == "sam" or st[p] != OVER]          # (PAF leaves a pair over the edit limit out)
        for line in plain.decode().splitlines():
            if line.startswith("@"):
                want.append(line)
                continue
            p = kept[k]
            k += 1
            unmapped = fmt == "sam" and int(line.split("\t")[1]) & 4
            assert bool(unmapped) == (st[p] == OVER)
            want.append(line if unmapped else line + tag + strings[p])
        assert k == len(kept) and got.decode().splitlines() == want
    s, got = write_with(job, res, diff, tmp_path, "tsv", "diff")
    assert s == api.SCRG_ERR_INVALID_ARG and got is None                      # TSV has no tags
    s, got = write_with(job, res, None, tmp_path, "tsv", "null")
    assert s == 0 and got
    short, keep_s = hand_diff(kind, strings[:-1])                              # a diff of another call
    assert write_with(job, res, short, tmp_path, "paf", "short")[0] == api.SCRG_ERR_INVALID_ARG


def test_cli_has_the_flags():
    run = lambda *a: subprocess.run([sys.executable, "-m", "scrooge_amd.cli"] + list(a), capture_output=True, text=True, cwd=ROOT)
    p = run("--help")
    assert p.returncode == 0 and "--md" in p.stdout and "--cs" in p.stdout
    files = ["--reference=none.fa", "--reads=none.fq", "--seeds=none.paf"]
    for bad in (["--md", "--cs"], ["--md", "--distance_only"], ["--cs", "--distance_only"], ["--md", "--format=tsv"], ["--cs", "--format=tsv"]):
        p = run(*bad, *files)
        assert p.returncode == 2 and ("--md" in p.stderr or "--cs" in p.stderr), bad       # an argument error, before anything is loaded


SHIM_SRC = r"""
#include <cstdio>
#include "scrooge_amd.hpp"
int main()
{
    if (scrg_device_count() == 0) { std::fprintf(stderr, "no usable HIP device\n"); return 2; }
    scrooge_amd::Handle h(0);
    std::vector<std::string> t = {"ACGTACGTACGTACGTAAAA", "ACGTACGT"}, q = {"ACGTACGTTCGTACGT", "ACGTACG"};
    for (int kind : {SCRG_DIFF_MD, SCRG_DIFF_CS}) {
        h.set_diff(kind);
        h.align_all(t, q);
        for (const std::string& s : h.take_diff()) std::printf("kind %d: %s\n", kind, s.c_str());
    }
    h.set_diff();
    h.align_all(t, q);
    try { h.take_diff(); } catch (const std::exception&) { std::printf("nothing to take\n"); }
    return 0;
}
"""


def build_shim(tmp_path):
    scrooge_amd.build_library()
    src, exe = str(tmp_path / "diff.cpp"), str(tmp_path / "diff")
    open(src, "w").write(SHIM_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lscrooge_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_shim_set_diff_take_diff_compiles_and_links(tmp_path):
    assert os.path.exists(build_shim(tmp_path))


def test_set_diff_round_trip(lib):
    if lib.scrg_device_count() == 0:
        pytest.skip("a handle needs a device")
    a = scrooge_amd.Aligner(0)
    try:
        assert a.diff() is None
        for kind in ("md", "cs", None):
            a.set_diff(kind)
            assert a.diff() == kind
        for other in (3, -1, 16):
            assert api._lazy(lib, "scrg_ctx_set_diff")(a.h, other) == api.SCRG_ERR_INVALID_ARG and a.diff() is None
        with pytest.raises(ValueError):
            a.set_diff("long")
        with pytest.raises(api.ScroogeError):
            a.take_diff()
    finally:
        a.close()


# ---------------------------------------------------------------------------------------------------------------
# GPU: the device layer on synthetic runs — no aligner
# ---------------------------------------------------------------------------------------------------------------
SHIFTS = [0, 1, 31, 13, 0, 17, 31, 1, 30, 2]          # text_off % 32 of the contiguous layout's texts
_cases = {}


def cases_of(n):
    """n pairs: the table's eleven verbatim (n >= 64), then random ones whose run counts walk dm.RUN_COUNTS — long counts where a
    pair has few runs or exactly 255 or 600 (a tile of more than 4096 bytes: stored without staging), short ones in the long pairs."""
    if n in _cases:
        return _cases[n]
    rng = np.random.Generator(np.random.PCG64(100 + n))
    out = [(t, r, dm.parse(c)) for t, r, c, _, _ in dm.TABLE] if n >= 64 else []
    counts = [1025] if n == 1 else dm.RUN_COUNTS + [600] + [int(x) for x in rng.integers(0, 40, size=n)]
    for k in range(n - len(out)):
        c = counts[k % len(counts)]
        out.append(dm.random_case(rng, c, max_count=255 if c <= 26 or c in (255, 600) else 12))
    _cases[n] = out
    return out


def device_diff(al, kind, cases, layout, source, text_len=None, read_len=None, gaps=True, short_capacity=False, text_rev=None,
                stranded=1):
    """scrg_diff_lengths, offsets made here, scrg_diff_render -> (lengths, offsets, the text buffer's bytes, bad count).
    Every second pair's read is stored as its reverse complement and flagged SCRG_READ_REVCOMP; source "slices": the runs lie in
    slices (stride 6 on the descriptors), "dense": back to back (stride 1).  short_capacity: diff_capacity ends one byte before
    the last pair's segment does."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    n = len(cases)
    texts = [c[0] for c in cases]
    rev = np.arange(n) % 2 == 1
    stored = [dm.revcomp(c[1]) if rv else c[1] for c, rv in zip(cases, rev)]
    if layout == "contiguous":
        words, offs = dm.pack_contiguous(texts + stored, [SHIFTS[k % len(SHIFTS)] for k in range(n)] + [0] * n)
        stride = 1
    else:
        words, offs = dm.pack_groups(texts + stored)
        stride = 64
    t_off, r_off = offs[:n], offs[n:] | np.where(rev, np.uint64(api.READ_REVCOMP), np.uint64(0))
    if text_rev is not None:                                                # pairs whose descriptor names a leftward text
        t_off = t_off | np.where(np.asarray(text_rev), np.uint64(api.TEXT_REVCOMP), np.uint64(0))
    tl = np.array([len(t) for t in texts] if text_len is None else text_len, dtype=np.uint64)
    rl = np.array([len(r) for r in stored] if read_len is None else read_len, dtype=np.uint64)
    cnt = np.array([len(c[2]) for c in cases], dtype=np.int64)
    cap = np.maximum(16, (cnt + 15) // 16 * 16)
    cig_off = np.concatenate([[0], np.cumsum(cap)])
    if source == "slices":
        runs = np.zeros((int(cig_off[n]), 2), dtype=np.uint8)               # (past a pair's runs: count 0, no operation)
        first = cig_off[:n]
    else:
        runs = np.zeros((int(cnt.sum()) + 1, 2), dtype=np.uint8)
        first = np.concatenate([[0], np.cumsum(cnt)])[:n]
    for k, c in enumerate(cases):
        if c[2]:
            runs[first[k]:first[k] + len(c[2])] = [(x, ord(o)) for x, o in c[2]]
    desc = np.stack([t_off, tl, r_off, rl, cig_off[:n].astype(np.uint64), cap.astype(np.uint64)], axis=1)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    seq_t, desc_t, runs_t = to(words.view(np.int64)), to(desc.view(np.int64)), to(runs)
    nruns_t = to(cnt.astype(np.int32))
    ro_t = None if source == "slices" else to(first.astype(np.int64))
    ro_stride = 6 if source == "slices" else 1
    dlen = torch.full((n,), -7, dtype=torch.int64, device=dev)
    kw = dict(text_stride_words=stride, read_stride_words=stride, stranded=stranded)
    al.diff_lengths(kind, n, seq_t, desc_t, runs_t, ro_t, ro_stride, nruns_t, dlen, **kw)
    torch.cuda.synchronize()
    lens = dlen.cpu().numpy()
    assert (lens >= 1).all() and lens.sum() < 1 << 26
    gap = (np.arange(n) % 3 == 0) * 3 if gaps else np.zeros(n, dtype=np.int64)       # room between segments that must stay untouched
    off = np.concatenate([[2], 2 + np.cumsum(lens + gap)])[:n]
    total = int(off[-1] + lens[-1]) + 5
    buf = torch.full((total,), 0xEE, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    al.diff_render(kind, n, seq_t, desc_t, runs_t, ro_t, ro_stride, nruns_t, dlen, to(off.astype(np.int64)), buf, bad,
                   capacity=int(off[-1] + lens[-1]) - 1 if short_capacity else None, **kw)
    torch.cuda.synchronize()
    return lens, off, buf.cpu().numpy().tobytes(), int(bad.cpu()[0])


def check_device(got, want, what):
    """Lengths, every string, and a buffer that is the canary outside every [offset, offset + len)."""
    lens, off, buf, bad = got
    assert bad == 0, what
    assert lens.tolist() == [len(w) + 1 for w in want], what
    exp = bytearray(b"\xEE" * len(buf))
    for k, w in enumerate(want):
        exp[int(off[k]):int(off[k]) + len(w) + 1] = w.encode() + b"\0"
    if bytes(exp) != buf:
        for k, w in enumerate(want):
            seg = buf[int(off[k]):int(off[k]) + len(w) + 1]
            assert seg == w.encode() + b"\0", "%s: pair %d differs: got %r want %r" % (what, k, seg[:80], w[:80])
        raise AssertionError("%s: bytes outside the pairs' segments were written" % what)


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["slices", "dense"])
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_device_layer(aligner, n, kind, layout, source):
    cases = cases_of(n)
    if n == 200:
        have = {len(c[2]) for c in cases}
        assert have >= {0, 1, 2, 24, 25, 255, 511, 512, 513, 1025} and have >= set(dm.RUN_COUNTS)
    want = [dm.model(kind, *c) for c in cases]
    if n >= 64:
        assert want[:len(dm.TABLE)] == [row[3 if kind == "md" else 4] for row in dm.TABLE]
    check_device(device_diff(aligner, kind, cases, layout, source), want, "n=%d %s %s %s" % (n, kind, layout, source))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_device_slices_cap_the_run_count(aligner, kind):
    """Stride 6: d_n_runs is capped at cigar_cap — a count of an overflowed pair names its first cigar_cap runs."""
    import torch
    rng = np.random.Generator(np.random.PCG64(5))
    text, read, runs = dm.random_case(rng, 32, max_count=9)
    dev = torch.device("cuda", aligner.device)
    aligner.set_stream(0)
    words, offs = dm.pack_contiguous([text, read], [3, 0])
    desc = np.array([[offs[0], len(text), offs[1], len(read), 0, 16]], dtype=np.uint64)
    r = np.array([(c, ord(o)) for c, o in runs], dtype=np.uint8)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    seq_t, desc_t, runs_t, n_t = to(words.view(np.int64)), to(desc.view(np.int64)), to(r), to(np.array([40], dtype=np.int32))
    dlen = torch.zeros(1, dtype=torch.int64, device=dev)
    aligner.diff_lengths(kind, 1, seq_t, desc_t, runs_t, None, 6, n_t, dlen)
    torch.cuda.synchronize()
    want = dm.model(kind, text, read, runs[:16])
    assert int(dlen[0]) == len(want) + 1
    buf = torch.full((len(want) + 9,), 0xEE, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    aligner.diff_render(kind, 1, seq_t, desc_t, runs_t, None, 6, n_t, dlen, to(np.array([4], dtype=np.int64)), buf, bad)
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xEE" * 4 + want.encode() + b"\0" + b"\xEE" * 4 and int(bad[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
@pytest.mark.parametrize("kind", KINDS)
def test_long_numbers_and_long_runs(aligner, kind, layout):
    """12 000 identical bases as 388 '=' runs: one number of five digits carried across lanes and tiles; a 255-base D and a
    255-base I run."""
    rng = np.random.Generator(np.random.PCG64(6))
    same = [(31, "=")] * 387 + [(3, "=")]
    assert len(same) == 388 and dm.consumed(same) == (12000, 12000)
    long_gap = dm.parse("10=255D5=255I10=1X")
    t2, q2 = dm.random_seq(rng, dm.consumed(long_gap)[0]), dm.random_seq(rng, dm.consumed(long_gap)[1])
    many = [(31, "=")] * 40 + long_gap + [(31, "=")] * 40                      # the same on the wavefront path
    t3, q3 = dm.random_seq(rng, dm.consumed(many)[0]), dm.random_seq(rng, dm.consumed(many)[1])
    cases = [("A" * 12000, "A" * 12000, same), (t2, q2, long_gap), (t3, q3, many)]
    want = [dm.model(kind, *c) for c in cases]
    assert want[0] == ("12000" if kind == "md" else ":12000")
    for source in ("slices", "dense"):
        check_device(device_diff(aligner, kind, cases, layout, source), want, "long %s %s %s" % (kind, layout, source))


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs", [5, 300])
@pytest.mark.parametrize("kind", KINDS)
def test_bad_input(aligner, kind, n_runs):
    """Runs that consume one base more than text_len, or than read_len: "" in both passes, counted by the render pass, the
    neighbours intact.  A segment outside diff_capacity: counted, not written."""
    rng = np.random.Generator(np.random.PCG64(7 + n_runs))
    cases = [dm.random_case(rng, n_runs, max_count=9, slack=0) for _ in range(5)]
    tl = [len(c[0]) for c in cases]
    rl = [len(c[1]) for c in cases]
    assert tl[1] > 0 and rl[3] > 0
    tl[1] -= 1
    rl[3] -= 1
    want = [dm.model(kind, *c) for c in cases]
    want[1] = want[3] = ""
    lens, off, buf, bad = device_diff(aligner, kind, cases, "contiguous", "slices", text_len=tl, read_len=rl)
    assert bad == 2
    check_device((lens, off, buf, 0), want, "bad input %s %d" % (kind, n_runs))
    # the last pair's segment ends one byte past the capacity
    good = [dm.model(kind, *c) for c in cases]
    lens, off, buf, bad = device_diff(aligner, kind, cases, "contiguous", "dense", short_capacity=True)
    assert bad == 1 and lens.tolist() == [len(w) + 1 for w in good]
    exp = bytearray(b"\xEE" * len(buf))
    for k, w in enumerate(good[:-1]):
        exp[int(off[k]):int(off[k]) + len(w) + 1] = w.encode() + b"\0"
    assert bytes(exp) == buf


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs", [5, 300])
@pytest.mark.parametrize("layout", ["contiguous", "groups"])
@pytest.mark.parametrize("kind", KINDS)
def test_strand_bits_the_kernels_do_not_serve(aligner, kind, layout, n_runs):
    """A descriptor with SCRG_TEXT_REVCOMP, and one with SCRG_READ_REVCOMP where params.stranded is 0: "" in both passes, counted
    by the render pass, no base read through the flagged offset; the pairs between them are intact."""
    rng = np.random.Generator(np.random.PCG64(11 + n_runs))
    cases = [dm.random_case(rng, n_runs, max_count=9) for _ in range(6)]
    want = [dm.model(kind, *c) for c in cases]
    flagged = [k in (1, 4) for k in range(6)]
    lens, off, buf, bad = device_diff(aligner, kind, cases, layout, "slices", text_rev=flagged)
    assert bad == 2
    check_device((lens, off, buf, 0), ["" if f else w for w, f in zip(want, flagged)], "text strand %s %s %d" % (kind, layout, n_runs))
    # device_diff stores every second pair's read reverse-complemented and flags it: without params.stranded pairs 1, 3, 5 are refused
    lens, off, buf, bad = device_diff(aligner, kind, cases, layout, "dense", stranded=0)
    assert bad == 3
    check_device((lens, off, buf, 0), ["" if k % 2 else w for k, w in enumerate(want)], "read strand %s %s %d" % (kind, layout, n_runs))


# ---------------------------------------------------------------------------------------------------------------
# GPU: the host layer against the model, from the same call's runs
# ---------------------------------------------------------------------------------------------------------------
def strings_of(off, text):
    off = np.asarray(off).astype(np.int64)
    assert off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off) >= 1)
    assert all(text[int(o) - 1] == 0 for o in off[1:])
    return [text[int(off[k]):int(off[k + 1]) - 1].decode() for k in range(len(off) - 1)]


def runs_of(arr, p):
    ro = arr["run_offset"]
    return [(int(c), chr(o)) for c, o in arr["runs"][int(ro[p]):int(ro[p + 1])]]


def check_against_runs(kind, arr, texts, reads, what):
    """Every pair's string is the model's for the runs the SAME result holds; for status OK the cs string turns the text into the
    read and the MD string accounts for the text the runs consume (neither check involves the model)."""
    got = strings_of(arr["diff_offset"], arr["diff_text"])
    assert len(got) == len(texts), what
    for p, s in enumerate(got):
        runs = runs_of(arr, p)
        assert s == dm.model(kind, texts[p], reads[p], runs), (what, p)
        if arr["status"][p] != OK or not runs:
            assert runs or s == "", (what, p)
            continue
        if kind == "cs":
            assert dm.apply_cs(texts[p], s) == (reads[p].decode(), dm.consumed(runs)[0]), (what, p)
        else:
            assert dm.md_text_consumed(s) == dm.consumed(runs)[0], (what, p)
    return got


_ont = {}


def ont_pairs():
    if not _ont:
        rng = np.random.Generator(np.random.PCG64(300))
        err, ratio = synth.PROFILES["ont"]
        texts, reads = [], []
        for _ in range(300):
            t, q = synth.make_pair(int(rng.integers(200, 3001)), err, ratio, rng, slack=0.1)
            texts.append(synth.BASES[t].tobytes())
            reads.append(synth.BASES[q].tobytes())
        texts[7], reads[7] = b"ACGTACGT", b""                       # an empty read: no runs, ""
        _ont["texts"], _ont["reads"] = texts, reads
    return _ont["texts"], _ont["reads"]


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (64, 0), (128, 65), (256, 129)])
@pytest.mark.parametrize("kind", KINDS)
def test_host_pairs_against_the_model(aligner, kind, W, O):
    texts, reads = ont_pairs()
    arr = aligner.align_pairs(texts, reads, arrays=True, diff=kind, W=W, O=O)
    assert aligner.diff() is None                                    # the per-call keyword restores the handle's setting
    got = check_against_runs(kind, arr, texts, reads, "%s W=%d O=%d" % (kind, W, O))
    assert (arr["status"] == OK).all() and got[7] == "" and sum(1 for s in got if len(s) > 50) > 250
    # the list form leaves the same strings in last_diff
    if (W, O) == (64, 33):
        aligner.align_pairs(texts[:20], reads[:20], diff=kind)
        assert aligner.last_diff == got[:20]


def mapping_texts(b, reads, reverse=None):
    """Per pair of a tests/test_host_layouts.py batch: the genome from its candidate on, and the read as aligned."""
    texts, qs = [], []
    for r, cs in enumerate(b["cands"]):
        for k, c in enumerate(cs):
            q = reads[r]
            if reverse is not None and reverse[r][k]:
                q = q.translate(dm.COMP)[::-1]
            texts.append(b["genome"][c:c + 2 * len(q) + 256])
            qs.append(q)
    return texts, qs


def with_diff(aligner, kind, call):
    """A host call of the handle level between set_diff(kind) and take_diff(arrays=True): its arrays with the strings among them."""
    aligner.set_diff(kind)
    try:
        arr = call()
        arr["diff_offset"], arr["diff_text"] = aligner.take_diff(arrays=True)
    finally:
        aligner.set_diff(None)
    return arr


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [65, 2 * 512 + 37])
def test_mapping(aligner, oracle, n, kind):
    """tests/test_host_layouts.py's batch (2 * 512 + 37 pairs: three chunks, the last group a partial one): the plain, the resident
    and the stranded call, best-candidate mode, an edit limit, both issue orders and all three outputs."""
    from tests.test_host_layouts import batch
    b = batch(oracle, n)
    co = offsets_of(b["cands"])
    texts, qs = mapping_texts(b, b["m_reads"])
    what = "mapping n=%d %s" % (n, kind)
    plain = aligner.align_mapping(b["genome"], b["m_reads"], b["cands"], arrays=True, diff=kind)
    want = check_against_runs(kind, plain, texts, qs, what)
    assert sum(1 for s in want if s) == n
    # resident genome; the issue order; the outputs (1 and 2 send no runs / no text back: the strings are the same ones)
    for kw in ({"sort_by_length": 0}, {"sort_by_length": 1}, {"outputs": api.SCRG_OUT_TEXT}, {"outputs": api.SCRG_OUT_RUNS}):
        arr = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, diff=kind, **kw)
        assert strings_of(arr["diff_offset"], arr["diff_text"]) == want, (what, kw)
    arr = aligner.align_mapping_rows(None, np.array([np.frombuffer(r.ljust(256, b"A"), dtype=np.uint8) for r in b["m_reads"]]),
                                     [len(r) for r in b["m_reads"]], co, [c for cs in b["cands"] for c in cs], diff=kind)
    assert strings_of(arr["diff_offset"], arr["diff_text"]) == want, what
    # best-candidate mode: the losers have no runs and ""
    best = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, diff=kind, best=True)
    got = check_against_runs(kind, best, texts, qs, what + " best")
    lost = best["status"] == NOT_BEST
    assert lost.sum() == n // 2 and all(got[p] == ("" if lost[p] else want[p]) for p in range(n))
    # an edit limit: pairs over it have ""
    lim = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, diff=kind, max_edits=12)
    got = check_against_runs(kind, lim, texts, qs, what + " limit")
    over = lim["status"] == OVER
    assert 0 < over.sum() < n and all(got[p] == ("" if over[p] else want[p]) for p in range(n))
    # both strands from one packed copy of the read (the stranded, resident call of the handle level)
    s_texts, s_qs = mapping_texts(b, b["s_reads"], b["reverse"])
    arr = with_diff(aligner, kind, lambda: aligner.align_mapping_directed(b["s_reads"], b["cands"], reverse=b["reverse"], arrays=True))
    got = check_against_runs(kind, arr, s_texts, s_qs, what + " stranded")
    assert sum(1 for s in got if s) == n and any(x for r in b["reverse"] for x in r)


@pytest.mark.gpu
def test_pairs_rows_and_chunks(aligner, oracle):
    """align_pairs_rows, and the pairwise call at three chunks with both issue orders."""
    from tests.test_host_layouts import batch
    b = batch(oracle, 2 * 512 + 37)
    texts, reads = b["texts"], b["reads"]
    a0 = aligner.align_pairs(texts, reads, arrays=True, diff="cs", sort_by_length=0)
    want = check_against_runs("cs", a0, texts, reads, "pairs")
    a1 = aligner.align_pairs(texts, reads, arrays=True, diff="cs", sort_by_length=1)
    assert strings_of(a1["diff_offset"], a1["diff_text"]) == want
    rows = np.zeros((len(texts), 512), dtype=np.uint8)
    for k, (t, r) in enumerate(zip(texts, reads)):
        rows[k, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        rows[k, 256:256 + len(r)] = np.frombuffer(r, dtype=np.uint8)
    a2 = aligner.align_pairs_rows(rows, 0, [len(t) for t in texts], 256, [len(r) for r in reads], diff="cs")
    assert strings_of(a2["diff_offset"], a2["diff_text"]) == want


@pytest.mark.gpu
def test_refusals(aligner, oracle):
    from tests.test_host_layouts import batch
    b = batch(oracle, 65)
    aligner.set_genome(b["genome"])
    aligner.set_diff("md")
    try:
        for call in (lambda: aligner.align_pairs(b["texts"], b["reads"], lanes_per_pair=8),
                     lambda: aligner.align_mapping(None, b["m_reads"], b["cands"], lanes_per_pair=64),
                     lambda: aligner.align_pairs(b["texts"], b["reads"], distance_only=True),
                     lambda: aligner.align_mapping(None, b["m_reads"], b["cands"], distance_only=True),
                     lambda: aligner.align_mapping_directed(b["m_reads"], b["cands"], leftward=[[1] * len(c) for c in b["cands"]]),
                     lambda: aligner.align_anchored(b["m_reads"], [[(c, 0) for c in cs] for cs in b["cands"]])):
            with pytest.raises(api.ScroogeError) as e:
                call()
            assert e.value.status == api.SCRG_ERR_INVALID_ARG
            with pytest.raises(api.ScroogeError):                     # a failed call leaves nothing to take
                aligner.take_diff()
        # leftward = all zero is the resident call: served
        aligner.align_mapping_directed(b["m_reads"], b["cands"], leftward=[[0] * len(c) for c in b["cands"]])
        first = aligner.take_diff()
        assert len(first) == 65 and all(first)
        with pytest.raises(api.ScroogeError) as e:                    # handed over once
            aligner.take_diff()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
        # strings nobody took are discarded by the next call
        aligner.align_pairs(b["texts"][:3], b["reads"][:3])
        aligner.align_pairs(b["texts"][:2], b["reads"][:2])
        assert len(aligner.take_diff()) == 2
    finally:
        aligner.set_diff(None)
    aligner.align_pairs(b["texts"][:2], b["reads"][:2])
    with pytest.raises(api.ScroogeError):                             # off: a call makes none
        aligner.take_diff()


@pytest.mark.gpu
def test_off_path_is_what_it_was(aligner, oracle):
    from tests.test_host_layouts import batch
    b = batch(oracle, 65)
    before = aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    aligner.set_diff("cs")
    try:
        aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    finally:
        aligner.set_diff(None)
    after = aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    assert sorted(before) == sorted(after) and "diff_text" not in after
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])) if not isinstance(before[k], bytes) else before[k] == after[k], k
    assert "".join("%d%s" % (c, chr(o)) for c, o in before["runs"][:int(before["run_offset"][1])]) == b["cigars"][0]


@pytest.mark.gpu
def test_shim_set_diff_take_diff_runs(tmp_path):
    p = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "nothing to take" and len(lines) == 5
    assert lines[0] == "kind 1: 8A7" and lines[2] == "kind 2: :8*at:7"              # ACGTACGT[A>T]CGTACGT against the text's prefix
    assert lines[1] == "kind 1: 7" and lines[3] == "kind 2: :7"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,fmt", [("cs", "paf"), ("md", "sam")])
def test_cli_end_to_end(tmp_path, capsys, kind, fmt):
    """--cs writes PAF, --md writes SAM: every record's tag is the model's string for the record's own CIGAR."""
    from scrooge_amd import cli
    from scrooge_amd import io as sio
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=12, seed=9)
    out = str(tmp_path / ("o." + fmt))
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--out=" + out, "--" + kind, "--format=" + fmt, "--reverse_strand"]) == 0
    capsys.readouterr()
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    genome, reads, cands, names = job.views()
    pairs = [(genome[start:], r.translate(dm.COMP)[::-1] if rv else r) for r, cs in zip(reads, cands) for start, rv in cs]
    lines = [x.split("\t") for x in open(out).read().splitlines() if not x.startswith("@")]
    assert len(lines) == job.n_pairs == len(pairs) > 0
    tag = "MD:Z:" if kind == "md" else "cs:Z:"
    edits = 0
    for (text, q), f in zip(pairs, lines):
        cigar = f[5] if fmt == "sam" else [x for x in f if x.startswith("cg:Z:")][0][5:]
        assert f[-1].startswith(tag) and f[-1][5:] == dm.model(kind, text, q, dm.parse(cigar)), f[0]
        edits += sum(c for c, o in dm.parse(cigar) if o != "=")
    assert edits > 0
