"""CIGAR forms: the CIGAR text of every pair in the merged and the M form, rendered on the GPU (scrooge_amd/csrc/host_path_kernels.hip;
scrg_ctx_set_cigar_form, scrg_cigar_text_lengths / scrg_cigar_text_render, scrg_cigar_from_runs).

Expected strings come from tests/cigar_form_model.py, a Python model written from the rules, applied to runs — a result's own
runs, or a fixture's CIGAR; it does not call the library.  The align kernels are not under test here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from tests import cigar_form_model as cm
from tests import diff_model as dm
from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, OVER, NOT_BEST = api.SCRG_OK, api.SCRG_PAIR_OVER_EDIT_LIMIT, api.SCRG_PAIR_NOT_BEST
FORMS = cm.FORMS
NEW_API = ["scrg_ctx_set_cigar_form", "scrg_ctx_get_cigar_form", "scrg_cigar_text_lengths", "scrg_cigar_text_render"]
NEW_IO = ["scrg_cigar_from_runs"]


@pytest.fixture(scope="module")
def lib():
    scrooge_amd.build_library()
    return scrooge_amd.load_library()


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_model_reproduces_the_table():
    for windowed, merged, m in cm.TABLE:
        runs = cm.parse(windowed)
        assert cm.model("windowed", runs) == windowed and cm.model("merged", runs) == merged and cm.model("m", runs) == m, windowed
    assert cm.model("merged", []) == "" and cm.model("m", []) == ""
    assert cm.model("m", cm.parse("4=1X2=1D2=")) == "7M1D2M" and cm.model("merged", cm.parse("31I13I16=2I2I")) == "44I16=4I"


def host_text(lib, form, runs, cap=None, canary=0xEE):
    """scrg_cigar_from_runs -> (status, measured length, the buffer's bytes); cap: the capacity passed (default: what was measured);
    form: a name, or a number passed as it is."""
    arr = (api.Run * max(1, len(runs)))(*[api.Run(c, o.encode() if isinstance(o, str) else bytes([o])) for c, o in runs])
    fn = api._lazy(lib, "scrg_cigar_from_runs")
    f = api._cigar_form(form) if isinstance(form, str) else form
    need = C.c_uint64(0)
    st = fn(f, C.cast(arr, C.c_void_p), len(runs), None, 0, C.byref(need))
    if st != 0:
        return st, None, None
    room = int(need.value) + 8
    buf = (C.c_uint8 * room)(*([canary] * room))
    got = C.c_uint64(0)
    st = fn(f, C.cast(arr, C.c_void_p), len(runs), C.cast(buf, C.c_void_p), int(need.value) if cap is None else cap, C.byref(got))
    assert got.value == need.value
    return st, int(need.value), bytes(buf)


@pytest.mark.parametrize("form", ["windowed"] + FORMS)
def test_cigar_from_runs_table(lib, form):
    for windowed, merged, m in cm.TABLE:
        want = {"windowed": windowed, "merged": merged, "m": m}[form]
        st, n, buf = host_text(lib, form, cm.parse(windowed))
        assert st == 0 and n == len(want) + 1 and buf[:n] == want.encode() + b"\0" and set(buf[n:]) == {0xEE}, windowed
        assert api.cigar_from_runs(form, windowed) == want


_random = []


def random_lists():
    """2 000 random run lists of 0..400 runs from tests/diff_model.py's generator: counts 1..255, all four operations, neighbours
    free to repeat an operation."""
    if not _random:
        rng = np.random.Generator(np.random.PCG64(1812))
        _random.extend(dm.random_runs(rng, int(rng.integers(0, 401))) for _ in range(2000))
        assert {o for runs in _random for _, o in runs} == set("=XID")
        assert sum(1 for runs in _random for a, b in zip(runs, runs[1:]) if a[1] == b[1]) > 10000
    return _random


@pytest.mark.parametrize("form", FORMS)
def test_cigar_from_runs_random(lib, form):
    """The model's string, the measured length, and a capacity one short of it."""
    for k, runs in enumerate(random_lists()):
        want = cm.model(form, runs).encode() + b"\0"
        st, n, buf = host_text(lib, form, runs)
        assert st == 0 and n == len(want) and buf[:n] == want and set(buf[n:]) == {0xEE}, k
        if k % 50 == 0:
            st, n, buf = host_text(lib, form, runs, cap=len(want) - 1)
            assert st == api.SCRG_ERR_CIGAR_OVERFLOW and n == len(want) and set(buf) == {0xEE}, k      # an error, nothing written


def test_cigar_from_runs_refusals(lib):
    assert host_text(lib, 3, [(4, "=")])[0] == api.SCRG_ERR_INVALID_ARG and host_text(lib, -1, [(4, "=")])[0] == api.SCRG_ERR_INVALID_ARG
    for form in ["windowed"] + FORMS:
        assert host_text(lib, form, [(4, "="), (0, "X")])[0] == api.SCRG_ERR_INVALID_ARG          # a zero count
        assert host_text(lib, form, [(4, "M")])[0] == api.SCRG_ERR_INVALID_ARG                     # an operation other than = X I D
        assert host_text(lib, form, [(4, "="), (1, 0)])[0] == api.SCRG_ERR_INVALID_ARG
        assert host_text(lib, form, [])[:2] == (0, 1)                                              # no runs: ""
    with pytest.raises(ValueError):
        api.cigar_from_runs("canonical", "4=")


def test_length_invariant():
    """A pair's merged or M text is never longer than its windowed text: what the pipeline sizes by run counts holds in every form."""
    for k, runs in enumerate(random_lists()):
        w = len(cm.model("windowed", runs))
        assert len(cm.model("m", runs)) <= len(cm.model("merged", runs)) <= w, k
    # the worst cases for the digits: sums that gain a digit (9 + 1, 99 + 1, 255 + 255 + ...) still lose a letter per run joined
    for runs in ([(9, "="), (1, "=")], [(99, "="), (1, "=")], [(255, "=")] * 4, [(1, "=")] * 10, [(5, "="), (5, "X")]):
        assert len(cm.model("m", runs)) <= len(cm.model("merged", runs)) <= len(cm.model("windowed", runs))


def test_header_library_and_bindings_have_the_entry_points(lib):
    from scrooge_amd import io as sio
    hdr = open(os.path.join(ROOT, "include", "scrooge_amd.h")).read()
    io_hdr = open(os.path.join(ROOT, "include", "scrooge_amd_io.h")).read()
    hpp = open(os.path.join(ROOT, "include", "scrooge_amd.hpp")).read()
    for name in NEW_API:
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in api.EXPORTED_SYMBOLS, name
    for name in NEW_IO:
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(lib, name) and name in sio.IO_SYMBOLS, name
    assert re.search(r"enum\s*\{\s*SCRG_CIGAR_WINDOWED\s*=\s*0,\s*SCRG_CIGAR_MERGED\s*=\s*1,\s*SCRG_CIGAR_M\s*=\s*2\s*\}", hdr)
    assert (api.CIGAR_WINDOWED, api.CIGAR_MERGED, api.CIGAR_M) == (0, 1, 2)
    assert re.search(r"void\s+set_cigar_form\s*\(", hpp)
    for name in ("set_cigar_form", "cigar_form", "cigar_text_lengths", "cigar_text_render"):
        assert callable(getattr(scrooge_amd.Aligner, name)), name
    assert callable(api.cigar_from_runs) and callable(sio.cigar_from_runs)
    # the feature is new entry points only: no struct of the interface moved
    assert lib.scrg_abi_version() == 8 == api.SCRG_ABI_VERSION
    assert api.Result._fields_[-1][0] == "text_end" and C.sizeof(api.Params) == 48


def check_setting(lib, a):
    assert a.cigar_form() == "windowed"
    for form in ("merged", "m", "windowed"):
        a.set_cigar_form(form)
        assert a.cigar_form() == form
    for other in (3, -1, 16):
        assert api._lazy(lib, "scrg_ctx_set_cigar_form")(a.h, other) == api.SCRG_ERR_INVALID_ARG and a.cigar_form() == "windowed"
    for other in ("canonical", None, True):
        with pytest.raises(ValueError):
            a.set_cigar_form(other)
    a.set_cigar_form(api.CIGAR_M)
    assert a.cigar_form() == "m"
    a.set_cigar_form()
    assert a.cigar_form() == "windowed"


def test_set_cigar_form_round_trip(lib):
    if lib.scrg_device_count() == 0:
        pytest.skip("a handle needs a device")
    a = scrooge_amd.Aligner(0)
    try:
        check_setting(lib, a)
    finally:
        a.close()


SHIM_SRC = r"""
#include <cstdio>
#include "scrooge_amd.hpp"
#include "scrooge_amd_io.h"
int main()
{
    scrg_run runs[2] = {{29, '='}, {21, '='}};
    char buf[16];
    uint64_t len = 0;
    if (scrg_cigar_from_runs(SCRG_CIGAR_M, runs, 2, buf, sizeof(buf), &len) != SCRG_OK) return 3;
    std::printf("host: %s\n", buf);
    if (scrg_device_count() == 0) { std::fprintf(stderr, "no usable HIP device\n"); return 2; }
    scrooge_amd::Handle h(0);
    std::vector<std::string> t = {"ACGTACGTACGTACGTAAAA", "ACGTACGT"}, q = {"ACGTACGTTCGTACGT", "ACGTACG"};
    for (int form : {SCRG_CIGAR_WINDOWED, SCRG_CIGAR_MERGED, SCRG_CIGAR_M}) {
        h.set_cigar_form(form);
        for (const auto& a : h.align_all(t, q)) std::printf("form %d: %s\n", form, a.cigar.c_str());
    }
    h.set_cigar_form();
    try { h.set_cigar_form(3); } catch (const std::exception&) { std::printf("refused\n"); }
    return 0;
}
"""


def build_shim(tmp_path):
    scrooge_amd.build_library()
    src, exe = str(tmp_path / "form.cpp"), str(tmp_path / "form")
    open(src, "w").write(SHIM_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir, "-lscrooge_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_shim_set_cigar_form_compiles_and_links(tmp_path):
    assert os.path.exists(build_shim(tmp_path))


def test_cli_has_the_flag(capsys):
    from scrooge_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--help"])
    assert e.value.code == 0 and "--cigar" in capsys.readouterr().out
    for bad in (["--cigar=m", "--validate"], ["--cigar=canonical"]):
        with pytest.raises(SystemExit) as e:                  # an argument error, before anything is loaded
            cli.main(["--reference=none.fa", "--reads=none.fq", "--seeds=none.paf"] + bad)
        assert e.value.code == 2
        capsys.readouterr()


@pytest.mark.parametrize("name", ["pairs_w64_o33.json", "pairs_w64_o0.json"])
def test_reference_cigars_through_the_host_function(lib, name):
    """Both forms tied to the reference's own answers with nothing of ours in between: the fixture's CIGAR, parsed, through
    scrg_cigar_from_runs equals the model."""
    cases = load_golden(name)["cases"]
    merged_some = 0
    for k, c in enumerate(cases):
        runs = cm.parse(c["cigar"])
        assert api.cigar_from_runs("windowed", runs) == c["cigar"], k
        for form in FORMS:
            assert api.cigar_from_runs(form, runs) == cm.model(form, runs), (k, form)
        merged_some += cm.model("merged", runs) != c["cigar"]
    assert merged_some > len(cases) // 4


# ---------------------------------------------------------------------------------------------------------------
# GPU: the device layer on synthetic runs — no aligner
# ---------------------------------------------------------------------------------------------------------------
RUN_COUNTS = [0, 1, 23, 24, 25, 26, 511, 512, 513, 1025]      # both sides of WALK_LANE_MAX_RUNS (24) and of WALK_TILE_RUNS (512)
_cases = {}


def cases_of(n):
    """n run lists whose lengths walk RUN_COUNTS (n = 1: 1 025 runs)."""
    if n not in _cases:
        rng = np.random.Generator(np.random.PCG64(500 + n))
        counts = [1025] if n == 1 else RUN_COUNTS
        _cases[n] = [dm.random_runs(rng, counts[k % len(counts)]) for k in range(n)]
    return _cases[n]


def raw(runs):
    """[(count, op)] with op a character or a byte value -> uint8 [n, 2]"""
    return np.array([(c, ord(o) if isinstance(o, str) else o) for c, o in runs], dtype=np.uint8).reshape(-1, 2)


def device_text(al, form, lists, source, cap_of=None, n_runs=None, lens_in=None, off_in=None, capacity=None):
    """scrg_cigar_text_lengths, offsets made here, scrg_cigar_text_render -> (lengths, offsets, the text buffer's bytes, bad count).
    source "slices": the runs lie in slices (stride 6 on descriptors), "dense": back to back (stride 1).  cap_of / n_runs: the
    slices' capacities and the counts passed, where they are not the lists' own; lens_in / off_in / capacity: what the render pass
    is told, where it is not what the length pass wrote."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    n = len(lists)
    cnt = np.array([len(r) for r in lists], dtype=np.int64)
    cap = np.maximum(16, (cnt + 15) // 16 * 16) if cap_of is None else np.asarray(cap_of, dtype=np.int64)
    room = np.maximum(cap, (cnt + 15) // 16 * 16)
    cig_off = np.concatenate([[0], np.cumsum(room)])
    if source == "slices":
        runs = np.zeros((int(cig_off[n]), 2), dtype=np.uint8)               # (past a pair's runs: count 0, no operation)
        first = cig_off[:n]
    else:
        runs = np.zeros((int(cnt.sum()) + 1, 2), dtype=np.uint8)
        first = np.concatenate([[0], np.cumsum(cnt)])[:n]
    for k, r in enumerate(lists):
        if r:
            runs[first[k]:first[k] + len(r)] = raw(r)
    zero = np.zeros(n, dtype=np.uint64)
    desc = np.stack([zero, zero, zero, zero, cig_off[:n].astype(np.uint64), cap.astype(np.uint64)], axis=1)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc_t, runs_t = to(desc.view(np.int64)), to(runs)
    nruns_t = to((cnt if n_runs is None else np.asarray(n_runs)).astype(np.int32))
    ro_t = None if source == "slices" else to(first.astype(np.int64))
    stride = 6 if source == "slices" else 1
    tlen = torch.full((n,), -7, dtype=torch.int64, device=dev)
    al.cigar_text_lengths(form, n, runs_t, ro_t, stride, nruns_t, tlen, pairs=desc_t)
    torch.cuda.synchronize()
    lens = tlen.cpu().numpy()
    assert (lens >= 1).all() and lens.sum() < 1 << 26
    gap = (np.arange(n) % 3 == 0) * 3                                      # room between segments that must stay untouched
    off = np.concatenate([[2], 2 + np.cumsum(lens + gap)])[:n] if off_in is None else np.asarray(off_in, dtype=np.int64)
    total = int(np.concatenate([[2], 2 + np.cumsum(lens + gap)])[-1]) + 5
    buf = torch.full((total,), 0xEE, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    al.cigar_text_render(form, n, runs_t, ro_t, stride, nruns_t, tlen if lens_in is None else to(np.asarray(lens_in, dtype=np.int64)),
                         to(off.astype(np.int64)), buf, bad, capacity=capacity, pairs=desc_t)
    torch.cuda.synchronize()
    return lens, off, buf.cpu().numpy().tobytes(), int(bad.cpu()[0])


def check_device(got, want, what, skip=()):
    """Lengths, every string, and a buffer that is the canary outside every [offset, offset + len); skip: pairs of which nothing
    may have been written."""
    lens, off, buf, bad = got
    assert lens.tolist() == [len(w) + 1 for w in want], what
    exp = bytearray(b"\xEE" * len(buf))
    for k, w in enumerate(want):
        if k not in skip:
            exp[int(off[k]):int(off[k]) + len(w) + 1] = w.encode() + b"\0"
    if bytes(exp) != buf:
        for k, w in enumerate(want):
            seg = buf[int(off[k]):int(off[k]) + len(w) + 1]
            assert k in skip or seg == w.encode() + b"\0", "%s: pair %d differs: got %r want %r" % (what, k, seg[:80], w[:80])
        raise AssertionError("%s: bytes outside the pairs' segments were written" % what)


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["slices", "dense"])
@pytest.mark.parametrize("form", ["windowed"] + FORMS)
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_device_layer(aligner, n, form, source):
    lists = cases_of(n)
    if n >= 64:
        assert {len(r) for r in lists} == set(RUN_COUNTS)
    want = [cm.model(form, r) for r in lists]
    got = device_text(aligner, form, lists, source)
    assert got[3] == 0
    check_device(got, want, "n=%d %s %s" % (n, form, source))


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs", [32, 600])
@pytest.mark.parametrize("form", FORMS)
def test_device_slices_cap_the_run_count(aligner, form, n_runs):
    """Stride 6: d_n_runs is capped at cigar_cap — the count of an overflowed pair names its first cigar_cap runs (16: the lane
    walk; 528: a second tile)."""
    rng = np.random.Generator(np.random.PCG64(5 + n_runs))
    runs = dm.random_runs(rng, n_runs)
    cap = 16 if n_runs == 32 else 528
    got = device_text(aligner, form, [runs, runs[:3]], "slices", cap_of=[cap, 16], n_runs=[n_runs + 8, 3])
    assert got[3] == 0
    check_device(got, [cm.model(form, runs[:cap]), cm.model(form, runs[:3])], "cap %s %d" % (form, n_runs))


def split(total, op, piece=255):
    """`total` bases under one operation as runs of at most `piece`"""
    return [(piece, op)] * (total // piece) + ([(total % piece, op)] if total % piece else [])


SUMS = [9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000]


def carried_cases():
    """-> [(what, runs, merged text or None, m text or None)]: the stretches that the wavefront walk carries from lane to lane and
    from tile to tile; a given text is asserted of the model before it is asked of the kernels."""
    out = [("1 300 '=' runs of 255: one stretch over three tiles", [(255, "=")] * 1300, "331500=", "331500M"),
           ("a stretch that ends at run 8, a lane border", [(5, "=")] * 8 + [(2, "I"), (3, "=")] * 10, "40=" + "2I3=" * 10, "40M" + "2I3M" * 10),
           ("a stretch that ends at run 512, a tile border", [(7, "=")] * 512 + [(2, "D"), (3, "=")] * 10, "3584=" + "2D3=" * 10,
            "3584M" + "2D3M" * 10),
           ("a stretch that ends at run 512 and a tile of one run", [(7, "=")] * 512 + [(2, "D")], "3584=2D", "3584M2D"),
           ("'=' and 'X' alternating over lane and tile borders", [(3, "="), (1, "X")] * 300, "3=1X" * 300, "1200M"),
           ("I and D alternating: nothing merges", [(2, "I"), (3, "D")] * 300, "2I3D" * 300, "2I3D" * 300)]
    every = []
    for s in SUMS:
        # by itself (few runs: the lane walk), in runs of 255 and in runs of 1 .. 3 (the wavefront walk for all but the smallest)
        out.append(("a stretch of %d" % s, [(1, "I")] + split(s, "=") + [(4, "D")], "1I%d=4D" % s, "1I%dM4D" % s))
        if s <= 10000:
            out.append(("a stretch of %d in small runs" % s, [(1, "D")] + split(s, "X", 3) + [(2, "I")], "1D%dX2I" % s, "1D%dM2I" % s))
        every += split(s, "=") + [(1, "I")]
    out.append(("all the sums in one pair", every, "".join("%d=1I" % s for s in SUMS), "".join("%dM1I" % s for s in SUMS)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["slices", "dense"])
@pytest.mark.parametrize("form", FORMS)
def test_carried_stretches(aligner, form, source):
    cases = carried_cases()
    lists = [c[1] for c in cases]
    want = [cm.model(form, r) for r in lists]
    for c, w in zip(cases, want):
        assert w == c[2 if form == "merged" else 3], c[0]
    assert len(lists[0]) > 2 * 512 and any(len(r) <= 24 for r in lists) and sum(1 for r in lists if len(r) > 512) >= 6
    got = device_text(aligner, form, lists, source)
    assert got[3] == 0
    lens, off, buf, _ = got
    for k, (c, w) in enumerate(zip(cases, want)):              # (by name first: which stretch it was)
        assert buf[int(off[k]):int(off[k]) + int(lens[k])] == w.encode() + b"\0", "%s (%s, %s)" % (c[0], form, source)
    check_device(got, want, "carried %s %s" % (form, source))


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs", [5, 300])
@pytest.mark.parametrize("form", FORMS)
def test_bad_input(aligner, form, n_runs):
    """A zero count, op 'M' and op 0 each give "" in both passes and are counted by the render pass, the neighbours intact.  A
    wrong length and a segment outside the capacity: counted, nothing of the pair written."""
    rng = np.random.Generator(np.random.PCG64(7 + n_runs))
    lists = [dm.random_runs(rng, n_runs) for _ in range(7)]
    at = n_runs - 2
    lists[1][at] = (0, "=")
    lists[3][at] = (4, "M")
    lists[5][at] = (4, 0)
    want = [cm.model(form, r) if k % 2 == 0 else "" for k, r in enumerate(lists)]
    for source in ("slices", "dense"):
        got = device_text(aligner, form, lists, source)
        assert got[3] == 3, source
        check_device(got, want, "bad runs %s %d %s" % (form, n_runs, source))
    # WINDOWED prints what the runs hold, as the pipeline always has
    got = device_text(aligner, "windowed", lists[:2], "dense")
    assert got[3] == 0
    check_device(got, ["".join("%d%s" % r for r in lists[0]), "".join("%d%s" % r for r in lists[1])], "windowed prints")
    # a length that is not the string's (one more, one less), a segment that ends one byte past the capacity, one that begins past it
    good = [dm.random_runs(rng, n_runs) for _ in range(6)]
    for f in (["windowed", form] if form == "merged" else [form]):
        want = [cm.model(f, r) for r in good]
        lens = np.array([len(w) + 1 for w in want])
        gap = (np.arange(6) % 3 == 0) * 3
        off = np.concatenate([[2], 2 + np.cumsum(lens + gap)])[:6]
        told = lens.copy()
        told[1] += 1
        told[3] -= 1
        off[5] = 1 << 40
        got = device_text(aligner, f, good, "dense", lens_in=told, off_in=off, capacity=int(off[4] + lens[4]) - 1)
        assert got[3] == 4, f
        check_device(got, want, "bad segments %s %d" % (f, n_runs), skip={1, 3, 4, 5})


# ---------------------------------------------------------------------------------------------------------------
# GPU: the host layer — every text against the model of the SAME result's runs
# ---------------------------------------------------------------------------------------------------------------
def texts_of(arr):
    off, text = np.asarray(arr["cigar_offset"]).astype(np.int64), arr["cigar_text"]
    assert off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off) >= 1)
    assert all(text[int(o) - 1] == 0 for o in off[1:])
    return [text[int(off[k]):int(off[k + 1]) - 1].decode() for k in range(len(off) - 1)]


def runs_of(arr, p):
    ro = arr["run_offset"]
    return [(int(c), chr(o)) for c, o in arr["runs"][int(ro[p]):int(ro[p + 1])]]


def check_against_runs(form, arr, what):
    got = texts_of(arr)
    for p, s in enumerate(got):
        assert s == cm.model(form, runs_of(arr, p)), (what, p)
    return got


_pairs = {}


def synthetic_pairs():
    """200 pairs of 50 .. 3 000 bp with ONT-profile edits; then identical pairs of 600 bp (few runs: the lane walk), 3 000 bp and
    10 000 bp (the wavefront walk at every window setting used), and an empty read."""
    if not _pairs:
        rng = np.random.Generator(np.random.PCG64(301))
        err, ratio = synth.PROFILES["ont"]
        texts, reads = [], []
        for _ in range(200):
            t, q = synth.make_pair(int(rng.integers(50, 3001)), err, ratio, rng, slack=0.1)
            texts.append(synth.BASES[t].tobytes())
            reads.append(synth.BASES[q].tobytes())
        for n in (600, 3000, 10000):
            s = synth.random_seq(n, rng)
            texts.append(s)
            reads.append(s)
        texts.append(b"ACGTACGT")
        reads.append(b"")
        _pairs["texts"], _pairs["reads"] = texts, reads
    return _pairs["texts"], _pairs["reads"]


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [(64, 33), (64, 0), (128, 65), (256, 129)])
@pytest.mark.parametrize("form", FORMS)
def test_host_pairs_against_the_model(aligner, form, W, O):
    from scrooge_amd import io as sio
    texts, reads = synthetic_pairs()
    what = "%s W=%d O=%d" % (form, W, O)
    arr = aligner.align_pairs(texts, reads, arrays=True, cigar_form=form, W=W, O=O)
    assert aligner.cigar_form() == "windowed"                    # the per-call keyword restores the handle's setting
    got = check_against_runs(form, arr, what)
    assert (arr["status"] == OK).all() and got[203] == ""
    letter = "=" if form == "merged" else "M"
    assert got[200:203] == ["600" + letter, "3000" + letter, "10000" + letter], what
    assert len(runs_of(arr, 200)) <= 24 < len(runs_of(arr, 202))                     # both walks
    if W == 64:
        assert len(runs_of(arr, 201)) > 24
    for p, s in enumerate(got):
        ops = [o for _, o in cm.stretches(s)]
        assert all(a != b for a, b in zip(ops, ops[1:])) and set(ops) <= set("=XID" if form == "merged" else "MID"), (what, p)
        if form == "merged" and s:
            assert sio.validate_alignment(texts[p], reads[p], s, int(arr["edit_distance"][p])) == 0, (what, p)
    assert sum(1 for p, s in enumerate(got) if s != cm.model("windowed", runs_of(arr, p))) > 170
    # text only: the same text; runs only: no text, and no error
    only = aligner.align_pairs(texts, reads, arrays=True, cigar_form=form, W=W, O=O, outputs=api.SCRG_OUT_TEXT)
    assert texts_of(only) == got and len(only["runs"]) == 0, what
    none = aligner.align_pairs(texts, reads, arrays=True, cigar_form=form, W=W, O=O, outputs=api.SCRG_OUT_RUNS)
    assert np.array_equal(none["runs"], arr["runs"]) and len(none["cigar_text"]) == 0, what
    # the list form
    if (W, O) == (64, 33):
        alns = aligner.align_pairs(texts[195:], reads[195:], cigar_form=form)
        assert [a.cigar for a in alns] == got[195:]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_pairs_rows_and_chunks(aligner, oracle, form):
    """The pairwise call at three chunks with both issue orders, align_pairs_rows, and the handle's own setting."""
    from tests.test_host_layouts import batch
    b = batch(oracle, 2 * 512 + 37)
    texts, reads = b["texts"], b["reads"]
    want = [cm.model(form, cm.parse(c)) for c in b["cigars"]]
    a0 = aligner.align_pairs(texts, reads, arrays=True, cigar_form=form, sort_by_length=0)
    assert check_against_runs(form, a0, "pairs") == want
    a1 = aligner.align_pairs(texts, reads, arrays=True, cigar_form=form, sort_by_length=1)
    assert texts_of(a1) == want
    rows = np.zeros((len(texts), 512), dtype=np.uint8)
    for k, (t, r) in enumerate(zip(texts, reads)):
        rows[k, :len(t)] = np.frombuffer(t, dtype=np.uint8)
        rows[k, 256:256 + len(r)] = np.frombuffer(r, dtype=np.uint8)
    a2 = aligner.align_pairs_rows(rows, 0, [len(t) for t in texts], 256, [len(r) for r in reads], cigar_form=form)
    assert texts_of(a2) == want
    with pytest.raises(api.ScroogeError):                            # the _multi calls have no handle
        aligner.align_pairs_rows(rows, 0, [len(t) for t in texts], 256, [len(r) for r in reads], devices=[0], cigar_form=form)
    aligner.set_cigar_form(form)
    try:
        for g in (1, 8, 64):                                          # the setting, whatever the kernel family
            a3 = aligner.align_pairs(texts[:130], reads[:130], arrays=True, lanes_per_pair=g)
            assert texts_of(a3) == want[:130], g
        # distance only: no text, no effect, no error
        d = aligner.align_pairs(texts[:130], reads[:130], arrays=True, distance_only=True)
        assert d["edit_distance"].tolist() == b["eds"][:130] and len(d["cigar_text"]) == 0
    finally:
        aligner.set_cigar_form("windowed")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_golden(aligner, golden_pairs, form):
    """tests/golden/pairs_w64_o33.json through align_pairs: every text is the model of the FIXTURE's CIGAR."""
    cases = golden_pairs["cases"]
    arr = aligner.align_pairs([c["text"] for c in cases], [c["read"] for c in cases], arrays=True, cigar_form=form,
                              W=golden_pairs["W"], O=golden_pairs["O"])
    assert texts_of(arr) == [cm.model(form, cm.parse(c["cigar"])) for c in cases]
    assert arr["edit_distance"].tolist() == [c["ed"] for c in cases]
    assert ["".join("%d%s" % r for r in runs_of(arr, p)) for p in range(len(cases))] == [c["cigar"] for c in cases]      # the runs stay


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_mapping(aligner, oracle, form):
    """Best-candidate mode: losers have ""; an edit limit: pairs over it have ""; the stranded call."""
    from tests.test_host_layouts import batch
    n = 65
    b = batch(oracle, n)
    want = [cm.model(form, cm.parse(c)) for c in b["m_cigars"]]
    plain = aligner.align_mapping(b["genome"], b["m_reads"], b["cands"], arrays=True, cigar_form=form)
    assert check_against_runs(form, plain, "mapping") == want and all(want)
    best = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, cigar_form=form, best=True)
    got = check_against_runs(form, best, "best")
    lost = best["status"] == NOT_BEST
    assert lost.sum() == n // 2 and all(got[p] == ("" if lost[p] else want[p]) for p in range(n))
    lim = aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, cigar_form=form, max_edits=12)
    got = check_against_runs(form, lim, "limit")
    over = lim["status"] == OVER
    assert 0 < over.sum() < n and all(got[p] == ("" if over[p] else want[p]) for p in range(n))
    arr = aligner.align_mapping_directed(b["s_reads"], b["cands"], reverse=b["reverse"], arrays=True, cigar_form=form)
    assert check_against_runs(form, arr, "stranded") == [cm.model(form, cm.parse(c)) for c in b["s_cigars"]]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_anchored(aligner, form):
    """The joined text is the model of the joined runs; a read cut from the genome is one "L=" across the seam."""
    from tests.anchored_inputs import mutated
    rng = np.random.Generator(np.random.PCG64(41))
    genome = synth.random_seq(30000, rng)
    reads, anchors = [], []
    for L, ra in ((600, 300), (3000, 1234), (40, 0), (40, 40)):       # cut from the genome: identical
        g0 = int(rng.integers(1000, 20000))
        reads.append(genome[g0:g0 + L])
        anchors.append([(g0 + ra, ra)])
    n_same = len(reads)
    for _ in range(30):                                               # with edits on both sides of twelve bases copied exactly
        ga = int(rng.integers(3000, 25000))
        la, lb = int(rng.integers(0, 1500)), int(rng.integers(0, 1500))
        left = mutated(genome[ga - la:ga], rng)
        reads.append(left + genome[ga:ga + 12] + mutated(genome[ga + 12:ga + 12 + lb], rng))
        anchors.append([(ga, len(left))])
    aligner.set_genome(genome)
    try:
        win = aligner.align_anchored(reads, anchors, arrays=True)
        arr = aligner.align_anchored(reads, anchors, arrays=True, cigar_form=form)
        assert aligner.cigar_form() == "windowed"
        only = aligner.align_anchored(reads, anchors, arrays=True, cigar_form=form, outputs=api.SCRG_OUT_TEXT)
    finally:
        aligner.clear_genome()
    got = check_against_runs(form, arr, "anchored")
    assert np.array_equal(arr["runs"], win["runs"]) and np.array_equal(arr["text_start"], win["text_start"])
    assert texts_of(win) == [cm.model("windowed", runs_of(win, p)) for p in range(len(reads))]
    assert texts_of(only) == got
    letter = "=" if form == "merged" else "M"
    assert got[:n_same] == ["%d%s" % (len(r), letter) for r in reads[:n_same]]
    assert len(runs_of(arr, 1)) > 24 and sum(1 for p in range(n_same, len(reads)) if len(got[p]) < len(texts_of(win)[p])) >= 25


@pytest.mark.gpu
def test_off_path_is_what_it_was(aligner, oracle):
    """With the form never set, and with it set and reset, every byte is the oracle's; the reset case fails if the setting leaks."""
    from tests.test_host_layouts import batch
    b = batch(oracle, 65)
    want_text = b"".join(c.encode() + b"\0" for c in b["cigars"])
    fresh = scrooge_amd.Aligner(aligner.device)                       # a handle on which the form was never set
    try:
        before = fresh.align_pairs(b["texts"], b["reads"], arrays=True)
    finally:
        fresh.close()
    assert before["cigar_text"] == want_text and before["edit_distance"].tolist() == b["eds"]
    aligner.set_cigar_form("merged")
    try:
        during = aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    finally:
        aligner.set_cigar_form("windowed")
    assert during["cigar_text"] != want_text
    after = aligner.align_pairs(b["texts"], b["reads"], arrays=True)
    explicit = aligner.align_pairs(b["texts"], b["reads"], arrays=True, cigar_form="windowed")
    for other in (after, explicit):
        assert sorted(before) == sorted(other)
        for k in before:
            assert np.array_equal(np.asarray(before[k]), np.asarray(other[k])) if not isinstance(before[k], bytes) else before[k] == other[k], k
    for k in ("edit_distance", "status", "run_offset", "runs"):      # what stays as it is in every form
        assert np.array_equal(before[k], during[k]), k


@pytest.mark.gpu
def test_setting_round_trip_on_the_gpu(aligner, lib):
    check_setting(lib, aligner)


@pytest.mark.gpu
def test_shim_set_cigar_form_runs(tmp_path):
    p = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip().splitlines() == ["host: 50M", "form 0: 8=1X7=", "form 0: 7=", "form 1: 8=1X7=", "form 1: 7=", "form 2: 16M", "form 2: 7M",
                                             "refused"]


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path, capsys):
    """--cigar merged --format sam: no record has two adjacent equal operations; --cigar m: only M I D; both give the same NM, and
    --verify (made from the runs) works with every form."""
    from scrooge_amd import cli
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=12, seed=9)
    recs = {}
    for form in ("windowed", "merged", "m"):
        out = str(tmp_path / (form + ".sam"))
        assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--out=" + out, "--format=sam", "--reverse_strand", "--verify",
                         "--cigar=" + form]) == 0
        assert " 0 failed" in capsys.readouterr().out
        recs[form] = [x.split("\t") for x in open(out).read().splitlines() if not x.startswith("@")]
    assert len(recs["windowed"]) == len(recs["merged"]) == len(recs["m"]) > 0
    nm = lambda f: [x for x in f if x.startswith("NM:i:")][0]
    for w, g, m in zip(recs["windowed"], recs["merged"], recs["m"]):
        assert w[:5] == g[:5] == m[:5] and w[6:10] == g[6:10] == m[6:10] and nm(w) == nm(g) == nm(m)
        runs = cm.parse(w[5])
        assert g[5] == cm.model("merged", runs) and m[5] == cm.model("m", runs)
        ops_g, ops_m = [o for _, o in cm.stretches(g[5])], [o for _, o in cm.stretches(m[5])]
        assert all(a != b for a, b in zip(ops_g, ops_g[1:])) and set(ops_g) <= set("=XID")
        assert all(a != b for a, b in zip(ops_m, ops_m[1:])) and set(ops_m) <= set("MID")
    assert any(g[5] != w[5] for w, g in zip(recs["windowed"], recs["merged"]))
    # PAF's cg:Z: gets the same text
    out = str(tmp_path / "m.paf")
    assert cli.main(["--reference=" + fa, "--reads=" + fq, "--seeds=" + seeds, "--out=" + out, "--reverse_strand", "--cigar=m"]) == 0
    capsys.readouterr()
    cg = [[x for x in line.split("\t") if x.startswith("cg:Z:")][0][5:] for line in open(out).read().splitlines()]
    assert cg == [m[5] for m in recs["m"]]
