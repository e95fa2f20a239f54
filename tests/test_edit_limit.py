"""The per-pair edit limit (scrg_ctx_set_edit_limit, include/scrooge_amd.h "EDIT LIMIT").

Every expected value comes from a reference CIGAR (the oracle's, or a golden one) through the window-end model: the edit
stream of a CIGAR (scrg_runs_to_edit_stream, no GPU) has one byte per edit and one per window end, so the running sum of edits
at every window end is known on the CPU.  A pair is over the limit exactly when its full edit distance exceeds it, and it is
reported with the running sum at the first window end where that sum exceeds the limit, no runs and status
SCRG_PAIR_OVER_EDIT_LIMIT (2 in d_pair_status of the device-pointer layer)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api, synth
from scrooge_amd import io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CIGAR = "31I13I16=2I2I"           # pair T x 44 + AAAACCCCGGGGTTTTAAAA vs AAAACCCCGGGGTTTT, ED 48
GOLDEN_TEXT, GOLDEN_READ = b"AAAACCCCGGGGTTTT", b"T" * 44 + b"AAAACCCCGGGGTTTTAAAA"


def window_model(cigar, lim, W=64, O=33):
    """(over, reported edit distance) for limit `lim` (None: no limit), from the running sum at every window end."""
    s = 0
    for b in api.cigar_to_edit_stream(cigar, W, O):
        if b >> 6:
            s += 1                                      # an X, I or D byte
        elif (b & 63) != 63 and lim is not None and s > lim:
            return True, s                              # a window end (0x3F: 63 matches, no window end)
    return False, s


def revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("read_len", [0, 1, 6, 7, 150, 999, 1000, 1001, 10_000, 123_457, (1 << 40) + 17, (1 << 64) - 1])
@pytest.mark.parametrize("max_edits", [None, 0, 15, 10_000])
@pytest.mark.parametrize("per_mille", [None, 1, 150, 999, 1000])
def test_limit_arithmetic(read_len, max_edits, per_mille):
    parts = []
    if max_edits is not None:
        parts.append(max_edits)
    if per_mille is not None:
        parts.append(min(per_mille * read_len // 1000, (1 << 63) - 1))
    assert api.edit_limit_for(read_len, max_edits, per_mille) == (min(parts) if parts else None)


def test_limit_arithmetic_edges():
    assert api.edit_limit_for(6, None, 150) == 0            # a short read: only an exact match is within
    assert api.edit_limit_for(100, -5, None) is None        # max_edits < 0: off
    for pm in (-1, 1001, 1 << 20):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            api.edit_limit_for(100, None, pm)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    lib = api.load_library()
    assert api._lazy(lib, "scrg_edit_limit_for")(-1, 0, 100, None) == api.SCRG_ERR_INVALID_ARG


def test_status_string_and_exports():
    lib = api.load_library()
    assert api.SCRG_PAIR_OVER_EDIT_LIMIT == 7
    assert lib.scrg_status_string(7).decode() == "pair over its edit limit"
    for name in ("scrg_ctx_set_edit_limit", "scrg_ctx_get_edit_limit", "scrg_edit_limit_for"):
        assert name in api.EXPORTED_SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("lim,expect", [(30, (True, 31)), (45, (True, 46)), (47, (True, 48)), (48, (False, 48)), (None, (False, 48))])
def test_window_model_on_golden(lim, expect):
    stream = api.cigar_to_edit_stream(GOLDEN_CIGAR)
    assert sum(1 for b in stream if b >> 6) == 48
    assert window_model(GOLDEN_CIGAR, lim) == expect


def _result_for(n, over):
    """A hand-built scrg_result: every pair '10=' at edit distance 0, except the pairs in `over` (no runs, "", ED 9)."""
    runs, roff, text, toff, st, ed = [], [0], b"", [0], [], []
    for k in range(n):
        if k in over:
            text += b"\0"
            st.append(api.SCRG_PAIR_OVER_EDIT_LIMIT)
            ed.append(9)
        else:
            runs.append((10, b"="))
            text += b"10=\0"
            st.append(0)
            ed.append(0)
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


def test_job_write_leaves_over_limit_pairs_unmapped(tmp_path):
    from tests.test_io import make_dataset
    fa, fq, seeds, _, truth = make_dataset(str(tmp_path), n_reads=6, seed=5)
    job = sio.Job(fa, fq, seeds, reverse_strand=1)
    n = job.n_pairs
    _, _, cands, names = job.views()
    rev = [rv for cs in cands for _, rv in cs]
    over = {1, n - 1}
    res, keep = _result_for(n, over)
    paf, sam = str(tmp_path / "o.paf"), str(tmp_path / "o.sam")
    assert job.lib.scrg_job_write(job.h, C.byref(res), paf.encode(), 0) == 0
    assert job.lib.scrg_job_write(job.h, C.byref(res), sam.encode(), 1) == 0
    lines = open(paf).read().splitlines()
    assert len(lines) == n - len(over)
    assert all(line.endswith("cg:Z:10=") for line in lines)
    recs = [line.split("\t") for line in open(sam).read().splitlines() if not line.startswith("@")]
    assert len(recs) == n
    for k, f in enumerate(recs):
        if k in over:
            assert int(f[1]) == (4 | 16 if rev[k] else 4) and f[5] == "*" and f[3] != "0"
            assert not any(x.startswith("NM:i:") for x in f[11:])
        else:
            assert int(f[1]) == (16 if rev[k] else 0) and f[5] == "10=" and "NM:i:0" in f[11:]


SHIM_SRC = r"""
#include <cstdio>
#include <stdexcept>
#include "scrooge_amd.hpp"
int main()
{
    if (scrg_device_count() == 0) { std::fprintf(stderr, "no usable HIP device\n"); return 2; }
    scrooge_amd::Handle h(0);
    std::vector<std::string> t = {"AAAACCCCGGGGTTTT", "ACGTACGT"}, q = {std::string(44, 'T') + "AAAACCCCGGGGTTTTAAAA", "ACGTACG"};
    h.set_edit_limit(30);
    for (const auto& a : h.align_all(t, q)) std::printf("limit30 cigar=%s edit_distance=%d\n", a.cigar.c_str(), (int)a.edit_distance);
    h.set_edit_limit(-1, 150);
    for (const auto& a : h.align_all(t, q)) std::printf("pm150 cigar=%s edit_distance=%d\n", a.cigar.c_str(), (int)a.edit_distance);
    h.set_edit_limit();
    for (const auto& a : h.align_all(t, q)) std::printf("none cigar=%s edit_distance=%d\n", a.cigar.c_str(), (int)a.edit_distance);
    try { h.set_edit_limit(5, 1001); std::printf("no throw\n"); } catch (const std::invalid_argument&) { std::printf("rejected\n"); }
    return 0;
}
"""


def build_shim(tmp_path):
    scrooge_amd.build_library()
    src, exe = tmp_path / "shim_limit.cpp", str(tmp_path / "shim_limit")
    src.write_text(SHIM_SRC)
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + libdir, "-lscrooge_amd", "-Wl,-rpath," + libdir, "-o", exe])
    return exe


def test_shim_set_edit_limit_compiles_and_links(tmp_path):
    exe = build_shim(tmp_path)
    if api.load_library().scrg_device_count() > 0:
        pytest.skip("GPU present; covered by the gpu test")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "no usable HIP device" in p.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_shim_set_edit_limit_runs(tmp_path):
    p = subprocess.run([build_shim(tmp_path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip().splitlines() == [
        "limit30 cigar= edit_distance=31", "limit30 cigar=7= edit_distance=0",
        "pm150 cigar= edit_distance=31", "pm150 cigar=7= edit_distance=0",       # floor(150 * 64 / 1000) = 9
        "none cigar=31I13I16=2I2I edit_distance=48", "none cigar=7= edit_distance=0", "rejected"]


def check_host(alns, status, reads, cigars, eds, max_edits, per_mille, W=64, O=33):
    for k, (a, st) in enumerate(zip(alns, status)):
        lim = api.edit_limit_for(len(reads[k]), max_edits, per_mille)
        over, ed = window_model(cigars[k], lim, W, O)
        if over:
            assert (st, a.cigar, a.edit_distance) == (api.SCRG_PAIR_OVER_EDIT_LIMIT, "", ed), (k, lim, cigars[k])
        else:
            assert (st, a.cigar, a.edit_distance) == (0, cigars[k], eds[k]), (k, lim)


@pytest.mark.gpu
def test_golden_pairs_at_limits(aligner, golden_pairs):
    cases = golden_pairs["cases"]
    texts, reads = [c["text"] for c in cases], [c["read"] for c in cases]
    cigars, eds = [c["cigar"] for c in cases], [c["ed"] for c in cases]
    seen = 0
    for lim in (0, 1, 15):
        alns = aligner.align_pairs(texts, reads, max_edits=lim)
        check_host(alns, aligner.last_status, reads, cigars, eds, lim, None)
        seen += sum(s == api.SCRG_PAIR_OVER_EDIT_LIMIT for s in aligner.last_status)
    for d in (-1, 0, 1):                                  # ED - 1, ED, ED + 1: one call per distinct limit
        by_lim = {}
        for k, e in enumerate(eds):
            if e + d >= 0:
                by_lim.setdefault(e + d, []).append(k)
        for lim, ks in by_lim.items():
            alns = aligner.align_pairs([texts[k] for k in ks], [reads[k] for k in ks], max_edits=lim)
            check_host(alns, aligner.last_status, [reads[k] for k in ks], [cigars[k] for k in ks], [eds[k] for k in ks], lim, None)
            assert all((s == api.SCRG_PAIR_OVER_EDIT_LIMIT) == (d < 0) for s in aligner.last_status)
    assert seen > 0 and aligner.edit_limit() == (None, None)


def make_batch(n, L, seed, decoys=0.5):
    """True ONT-like pairs, a share of them turned into decoys (the read against an unrelated random text)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    texts, reads = synth.make_pairs(n, L, "ont", seed=seed)
    for k in range(n):
        if rng.random() < decoys:
            texts[k] = synth.random_seq(len(texts[k]), rng)
    rev = [bool(x) for x in rng.random(n) < 0.5]
    return texts, reads, rev


def _pack_rows(al, texts, reads, layout, dev):
    """One bucket of pairs in rows of one width (a text slot and a read slot) -> (planar words on the device, text and read
    offsets in bases within them)."""
    import torch
    n = len(texts)
    tw, rw = (max(map(len, texts)) + 31) // 32, (max(map(len, reads)) + 31) // 32
    wpr = tw + rw
    rows = np.zeros((n, wpr * 32), dtype=np.uint8)
    for k in range(n):
        rows[k, :len(texts[k])] = np.frombuffer(texts[k], dtype=np.uint8)
        rows[k, tw * 32: tw * 32 + len(reads[k])] = np.frombuffer(reads[k], dtype=np.uint8)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    idx = np.arange(n, dtype=np.int64)
    if layout == "groups":
        seq = torch.zeros(((n + 63) // 64) * 64 * wpr + api.SEQ_PAD_WORDS_GROUPS, dtype=torch.int64, device=dev)
        al.pack_planar_groups(torch.from_numpy(rows).to(dev).view(-1), n, wpr, seq, bad)
        t_off = 32 * (((idx // 64) * wpr) * 64 + idx % 64)
        r_off = 32 * (((idx // 64) * wpr + tw) * 64 + idx % 64)
    else:
        seq = torch.zeros(n * wpr + api.SEQ_PAD_WORDS, dtype=torch.int64, device=dev)
        al.pack_planar(torch.from_numpy(rows).to(dev).view(-1), seq, bad)
        t_off, r_off = idx * wpr * 32, (idx * wpr + tw) * 32
    assert int(bad) == 0
    return seq, t_off, r_off


def pack_sequences(al, texts, reads, layout, long_over=None):
    """The pairs' sequences packed once on the device -> (planar words, text offsets, read offsets in bases, word stride).
    long_over: pairs with a text or read longer than this get rows of their own width behind the others (a few 20 kb pairs
    among 50 000 short ones do not widen every row)."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    n = len(texts)
    is_long = np.array([long_over is not None and max(len(t), len(r)) > long_over for t, r in zip(texts, reads)], dtype=bool)
    t_off, r_off, seqs, base = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), [], 0
    for sel in (np.flatnonzero(~is_long), np.flatnonzero(is_long)):
        if len(sel):
            seq, t, r = _pack_rows(al, [texts[k] for k in sel], [reads[k] for k in sel], layout, dev)
            t_off[sel], r_off[sel] = t + 32 * base, r + 32 * base
            base += seq.numel()
            seqs.append(seq)
    return (seqs[0] if len(seqs) == 1 else torch.cat(seqs)), t_off, r_off, (64 if layout == "groups" else 1)


def device_run(al, texts, reads, rev, W, O, layout, edits, stranded, max_edits, per_mille, select=0, waves_per_cu=0, perm=None,
               caps=None, packed=None, raw=False, **params):
    """One align_device / align_device_edits call on packed sequences -> (ed, status, n, per-pair bytes of the slice).

    perm: descriptor k points at pair perm[k] (any length, pairs may repeat: the sequences are stored once, every descriptor has
    a slice of its own); the results are per descriptor.  caps: every PAIR's slice capacity in runs (multiples of 16; the slices
    are laid out by a prefix sum over the descriptors), None = one capacity that fits the longest read.  waves_per_cu and other
    scrg_params by keyword.  packed: the result of pack_sequences for these pairs and this layout, to pack once for many
    launches.  raw=True: the outputs as numpy arrays, for batches that are compared without a loop over pairs (check_device_raw)."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    seq, t_off, r_off, stride = packed if packed is not None else pack_sequences(al, texts, reads, layout)
    read_len = np.array([len(x) for x in reads], dtype=np.uint64)
    text_len = np.array([len(x) for x in texts], dtype=np.uint64)
    perm = np.arange(len(texts), dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)
    n = len(perm)
    if caps is None:
        caps = np.full(len(texts), (2 * ((int(read_len.max()) + 31) // 32) * 32 + 16 + 15) // 16 * 16, dtype=np.int64)
    cap = np.asarray(caps, dtype=np.int64)[perm]
    assert (cap % 16 == 0).all()
    cig_off = np.concatenate([[0], np.cumsum(cap)])
    r_off = r_off.astype(np.uint64)
    if stranded:
        r_off = r_off | np.array([np.uint64(api.READ_REVCOMP) if r else np.uint64(0) for r in rev], dtype=np.uint64)
    desc = np.stack([t_off.astype(np.uint64)[perm], text_len[perm], r_off[perm], read_len[perm], cig_off[:-1].astype(np.uint64),
                     cap.astype(np.uint64)], axis=1)
    desc_t = torch.from_numpy(desc.view(np.int64)).to(dev)
    slices = torch.zeros(int(cig_off[-1]) * 2, dtype=torch.uint8, device=dev)
    ed = torch.empty(n, dtype=torch.int64, device=dev)
    ln = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    kw = dict(W=W, O=O, text_stride_words=stride, read_stride_words=stride, stranded=int(stranded), **params)
    if waves_per_cu:
        kw["waves_per_cu"] = waves_per_cu
    p = al._params(kw)
    p.reserved[0] = select            # (the test build: 512 / 1024 force the split / one-wavefront form)
    with al._call_limit(max_edits, per_mille):
        if edits:
            rc = torch.empty(n, dtype=torch.int32, device=dev)
            al._check(al.lib.scrg_align_device_edits(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, slices, ed, ln, st, rc)]))
        else:
            rc = None
            al._check(al.lib.scrg_align_device(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, slices, ed, ln, st)]))
        torch.cuda.synchronize()
    sl = slices.cpu().numpy()
    lh = ln.cpu().numpy()
    if raw:
        return {"ed": ed.cpu().numpy(), "status": st.cpu().numpy(), "len": lh.astype(np.int64), "slices": sl, "perm": perm,
                "byte_off": 2 * cig_off[:-1], "run_count": rc.cpu().numpy() if rc is not None else None}
    out = [sl[2 * cig_off[k]: 2 * cig_off[k] + (int(lh[k]) if edits else 2 * int(lh[k]))].tobytes() for k in range(n)]
    return ed.cpu().tolist(), st.cpu().tolist(), lh.tolist(), out, (rc.cpu().tolist() if rc is not None else None)


def check_device(res, reads, cigars, eds, W, O, edits, max_edits, per_mille, perm=None):
    """perm: the descriptor permutation of the run (descriptor k is pair perm[k] of reads / cigars / eds)."""
    ed, st, ln, out, rc = res
    n_over = 0
    for k, b in enumerate(range(len(reads)) if perm is None else perm):
        lim = api.edit_limit_for(len(reads[b]), max_edits, per_mille)
        over, want = window_model(cigars[b], lim, W, O)
        if over:
            n_over += 1
            assert (st[k], ed[k], ln[k]) == (api.DEVICE_STATUS_OVER_EDIT_LIMIT, want, 0), (k, lim, cigars[b])
            if rc is not None:
                assert rc[k] == 0
            continue
        assert (st[k], ed[k]) == (0, eds[b]), (k, lim)
        if edits:
            got = api.edit_stream_to_cigar(out[k], len(reads[b]), W, O)
        else:
            r = out[k]
            got = "".join("%d%s" % (r[2 * q], chr(r[2 * q + 1])) for q in range(len(r) // 2))
        assert got == cigars[b], (k, lim)
    return n_over


def ragged_mismatch(got, got_off, want, want_off, lens, chunk=1 << 15):
    """Entries k with got[got_off[k] : got_off[k] + lens[k]] != want[want_off[k] : want_off[k] + lens[k]] (uint8 arrays, byte
    offsets), compared in chunks of entries without a loop over them."""
    bad = []
    for a in range(0, len(lens), chunk):
        ln = lens[a: a + chunk]
        total = int(ln.sum())
        if total == 0:
            continue
        start = np.cumsum(ln) - ln
        within = np.arange(total, dtype=np.int64) - np.repeat(start, ln)
        diff = got[np.repeat(got_off[a: a + chunk], ln) + within] != want[np.repeat(want_off[a: a + chunk], ln) + within]
        if diff.any():
            bad.append(a + np.unique(np.searchsorted(start, np.flatnonzero(diff), side="right") - 1))
    return np.concatenate(bad) if bad else np.zeros(0, dtype=np.int64)


def check_device_raw(res, want_ed, want_len, want_bytes, want_off, over=None, over_ed=None, want_runs=None):
    """check_device for a raw=True result, without a loop over pairs: every descriptor's edit distance, status, length and every
    byte of its slice up to that length against the expectations of its pair (arrays indexed by PAIR, taken through res['perm']:
    want_len in the unit of the output, runs or stream bytes; want_bytes / want_off: all pairs' expected bytes and where each
    pair's start; over / over_ed: the pairs over the edit limit and what they report; want_runs: the run counts an edit-stream
    launch reports as well).  -> the indices of the descriptors that differ (sorted; empty = all equal) and the number over."""
    perm, n = res["perm"], len(res["perm"])
    is_over = np.zeros(n, dtype=bool) if over is None else np.asarray(over, dtype=bool)[perm]
    w_ed = np.where(is_over, np.asarray(over_ed, dtype=np.int64)[perm], want_ed[perm]) if over is not None else want_ed[perm]
    w_len = np.where(is_over, 0, want_len[perm])
    bad = (res["ed"] != w_ed) | (res["status"] != np.where(is_over, api.DEVICE_STATUS_OVER_EDIT_LIMIT, 0)) | (res["len"] != w_len)
    if res["run_count"] is not None and want_runs is not None:
        bad |= res["run_count"] != np.where(is_over, 0, want_runs[perm])
    unit = 1 if res["run_count"] is not None else 2                 # stream bytes, or runs of two bytes
    ok = np.flatnonzero(~bad)                                       # (a wrong length is reported already: its bytes are not looked at)
    diff = ragged_mismatch(res["slices"], res["byte_off"][ok], want_bytes, unit * want_off[perm[ok]], unit * w_len[ok])
    bad[ok[diff]] = True
    return np.flatnonzero(bad), int(is_over.sum())


KERNELS = [(64, 33, 512), (64, 33, 1024), (96, 49, 0), (192, 97, 0), (256, 129, 0), (256, 1, 0), (64, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,O,select", KERNELS)
def test_seeded_batches_vs_oracle(aligner, aligner_select, oracle, W, O, select):
    """True pairs and random decoys, limits that split them, in every lane kernel (the split and the one-wavefront forms of
    the default one forced through the test build), both sequence layouts, stranded pairs, runs and edit streams."""
    texts, reads, rev = make_batch(160, 700, seed=W * 7 + O + select)
    reads_rc = [revcomp(r) if v else r for r, v in zip(reads, rev)]
    eds, cigars, _, _ = oracle.align(texts, reads, W=W, O=O)
    eds_rc, cigars_rc, _, _ = oracle.align(texts, reads_rc, W=W, O=O)
    med, med_rc, q3_rc = int(np.median(eds)), int(np.median(eds_rc)), int(np.percentile(eds_rc, 75))
    al = aligner_select if select else aligner
    total = 0
    for layout, edits, stranded, me, pm in (("contiguous", False, False, med, None), ("groups", True, False, None, 150),
                                           ("groups", False, True, med_rc, 150), ("contiguous", True, True, q3_rc, None)):
        if select and edits:
            continue                                   # (the switches choose between forms of the runs kernel)
        res = device_run(al, texts, reads, rev, W, O, layout, edits, stranded, me, pm, select)
        ce, cc = (eds_rc, cigars_rc) if stranded else (eds, cigars)
        n_over = check_device(res, reads, cc, ce, W, O, edits, me, pm)
        assert 0 < n_over < len(reads), (layout, edits, stranded, n_over)
        total += n_over
    assert al.edit_limit() == (None, None)


@pytest.mark.gpu
def test_host_entry_points(aligner, oracle):
    rng = np.random.Generator(np.random.PCG64(77))
    genome = synth.random_seq(60_000, rng)
    n_reads, L = 120, 600
    starts = rng.integers(0, len(genome) - 2 * L, n_reads)
    reads = []
    for s in starts:
        codes = np.searchsorted(synth.BASES, np.frombuffer(genome[s:s + L + 60], dtype=np.uint8)).astype(np.uint8)
        reads.append(synth.BASES[synth.mutate(codes, 0.08, (1, 1, 1), rng)[:L]].tobytes())
    cands = [[int(s), int(rng.integers(0, len(genome) - 2 * L))] for s in starts]       # true locus, random decoy
    m_texts = [genome[c:] for cs in cands for c in cs]
    m_reads = [reads[r] for r, cs in enumerate(cands) for _ in cs]
    eds, cigars, _, _ = oracle.align(m_texts, m_reads)
    lim = int(np.median(eds))
    for me, pm in ((lim, None), (None, 200)):
        alns = aligner.align_pairs(m_texts, m_reads, max_edits=me, max_edit_per_mille=pm)
        check_host(alns, aligner.last_status, m_reads, cigars, eds, me, pm)
        assert 0 < sum(s == api.SCRG_PAIR_OVER_EDIT_LIMIT for s in aligner.last_status) < len(m_reads)
        alns = aligner.align_mapping(genome, reads, cands, max_edits=me, max_edit_per_mille=pm)
        check_host(alns, aligner.last_status, m_reads, cigars, eds, me, pm)
        aligner.set_genome(genome)
        alns = aligner.align_mapping(None, reads, cands, max_edits=me, max_edit_per_mille=pm)
        check_host(alns, aligner.last_status, m_reads, cigars, eds, me, pm)
        aligner.clear_genome()
    assert aligner.edit_limit() == (None, None)
    # a limit set on the handle and taken off again: byte-identical to a handle that never had one
    fresh = scrooge_amd.Aligner(0)
    try:
        aligner.set_edit_limit(5, 100)
        assert aligner.edit_limit() == (5, 100)
        aligner.set_edit_limit(None)
        a = aligner.align_mapping(genome, reads, cands, arrays=True)
        b = fresh.align_mapping(genome, reads, cands, arrays=True)
        for key in ("edit_distance", "status", "run_offset", "runs", "cigar_offset", "cigar_text"):
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])) if key != "cigar_text" else a[key] == b[key], key
    finally:
        aligner.set_edit_limit(None)
        fresh.close()


@pytest.mark.gpu
def test_rejections(aligner):
    for pm in (1001, -1):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            aligner.set_edit_limit(None, pm)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    assert aligner.edit_limit() == (None, None)
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        aligner.align_pairs([GOLDEN_TEXT], [GOLDEN_READ], max_edits=10, lanes_per_pair=8)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(scrooge_amd.ScroogeError):
        aligner.align_pairs_multi([0], [GOLDEN_TEXT], [GOLDEN_READ], max_edits=10)
    assert aligner.edit_limit() == (None, None)
    assert aligner.align_pairs([GOLDEN_TEXT], [GOLDEN_READ], lanes_per_pair=8)[0].edit_distance == 48


@pytest.mark.gpu
def test_work_is_skipped(aligner):
    """10 kb pairs against random texts at max_edits = 50: each is dropped after a few of its ~330 windows."""
    texts, reads, rev = make_batch(4096, 10_000, seed=3, decoys=1.0)
    times = {}
    for me in (None, 50):
        best = None
        for _ in range(3):
            res = device_run(aligner, texts, reads, rev, 64, 33, "groups", False, False, me, None)
            ms = aligner.last_kernel_ms()
            best = ms if best is None else min(best, ms)
        times[me] = best
        if me is not None:
            assert all(s == api.DEVICE_STATUS_OVER_EDIT_LIMIT for s in res[1])
            assert all(50 < e <= 50 + 2 * 31 for e in res[0])        # (at most one window's edits past the limit)
    assert times[50] < 0.25 * times[None], times
