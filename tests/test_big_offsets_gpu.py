"""Every kernel with its buffers moved past 2^31 and 2^32 (tests/big_offsets.py: the batch, the placements, the decoys).

Expected values never come from the code under test at another placement: align calls are held to the oracle, the side passes
to the Python models of tests/.  Every buffer is allocated from element 0 to beyond its highest offset, a decoy or a sentinel
lies where an address that lost 2^31 or 2^32 would land (tests/test_big_offsets.py proves the decoys give other answers), so a
truncated offset shows as a mismatch.

Which argument is carried past the thresholds by which test: DESIGN.md, "Offsets past 2^31 and 2^32"."""
import os
import time

import numpy as np
import pytest

from tests import big_offsets as bo
from tests import plane_inputs as pi
from tests import seed_big as sb
from tests.test_edit_stream import py_encode

pytestmark = pytest.mark.gpu

T31, T32 = bo.T31, bo.T32
SENTINEL = 0xEE
MW = (128, 65)                                   # the multiword row kernel's setting
SETTINGS = pi.MAPPING_SETTINGS + [MW]


# ------------------------------------------------------------------------------------------------ expected values
@pytest.fixture(scope="module")
def expected(oracle):
    """(W, O, declare) -> (edit distances, CIGARs): "exact" texts, and texts declared as mapping declares them (the oracle gets
    the cut of tests/big_offsets.py)."""
    b = bo.batch()
    out = {}
    for W, O in SETTINGS:
        out[(W, O, "exact")] = oracle.align(b.texts, b.reads, W=W, O=O, threads=8)[:2]
        out[(W, O, "mapping")] = oracle.align([b.cut(k, W) for k in range(b.n)], b.reads, W=W, O=O, threads=8)[:2]
    return out


def _cigar_of(u8):
    u8 = np.asarray(u8).reshape(-1, 2)
    return "".join("%d%s" % (c, chr(o)) for c, o in u8)


def _runs_bytes(cigar):
    out = bytearray()
    for n, op in pi.cigar_runs(cigar):
        out += bytes((n, ord(op)))
    return bytes(out)


def _text_end(cigar):
    return sum(n for n, op in pi.cigar_runs(cigar) if op in "=XD")


# ------------------------------------------------------------------------------------------------ buffers
def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _upload(aligner, layout, swept):
    """-> (placement, sequence tensor, kw of the layout)"""
    torch, dev = _dev()
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if layout == "linear":
        P = bo.place_sequences(swept)
        seq = torch.zeros(bo.seq_words(), dtype=torch.int64, device=dev)
        wpp = bo.PAGE // 32
        for p, page in sorted(P.image.pages.items()):
            aligner.pack_planar(torch.from_numpy(page).to(dev), seq[p * wpp: (p + 1) * wpp], bad)
        kw = {}
    else:
        P = bo.place_groups(swept)
        seq = torch.zeros(bo.seq_words(bo.GROUP), dtype=torch.int64, device=dev)
        for base, wpr, rows in P.uploads():          # (decoys first: where two share a place, the true block is written last)
            n_words = (rows.shape[0] + bo.GROUP - 1) // bo.GROUP * bo.GROUP * wpr
            aligner.pack_planar_groups(torch.from_numpy(np.ascontiguousarray(rows)).to(dev).view(-1), rows.shape[0], wpr,
                                       seq[base: base + n_words], bad)
        kw = dict(text_stride_words=bo.GROUP, read_stride_words=bo.GROUP)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    return P, seq, kw


def _desc(seqdesc, off, cap, ks=None):
    """The descriptors as a device tensor: (text_off, text_len, read_off, read_len) per pair, the slices; ks: these pairs only."""
    torch, dev = _dev()
    ks = range(len(seqdesc)) if ks is None else ks
    a = np.array([list(seqdesc[k]) + [off[k], cap[k]] for k in ks], dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(dev).contiguous()


def _low_slices(b, ks=None):
    ks = range(b.n) if ks is None else ks
    caps = [b.cap(k) for k in range(b.n)]
    off, at = [0] * b.n, 0
    for k in ks:
        off[k] = at
        at += caps[k]
    return off, caps, at


def _fill_sentinels(buf_u8, S, unit):
    for lo, n in S.sentinels:
        buf_u8[unit * lo: unit * (lo + n)].fill_(SENTINEL)


def _sentinels_intact(buf_u8, S, unit):
    return all(bool((buf_u8[unit * lo: unit * (lo + n)] == SENTINEL).all().item()) for lo, n in S.sentinels)


class _Strands:
    """Text strands on for the call, and the handle on torch's stream."""

    def __init__(self, aligner, on=True):
        self.a, self.on = aligner, on

    def __enter__(self):
        self.a.set_stream(0)
        self.a.set_text_strands(self.on)

    def __exit__(self, *exc):
        self.a.set_text_strands(False)
        self.a.use_own_stream()


def _align_all_modes(aligner, seq, desc, ks, off, caps, arena, want, kw, modes=("runs", "edits", "distance"), W=64, O=33, tag=""):
    """One align call per mode on the pairs ks (rows of desc), each held to `want` = (edit distances, CIGARs) of the whole batch."""
    torch, dev = _dev()
    n = len(ks)
    eds = [want[0][k] for k in ks]
    ed = torch.empty(n, dtype=torch.int64, device=dev)
    nr = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    if "runs" in modes:
        ed.fill_(-1), nr.fill_(-1), st.fill_(-1)
        aligner.align_device(n, seq, desc, arena, ed, nr, st, W=W, O=O, **kw)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n, (tag, "status")
        cnt = nr.cpu().tolist()
        got = [_cigar_of(arena[2 * off[k]: 2 * (off[k] + cnt[j])].cpu().numpy()) for j, k in enumerate(ks)]
        bad = [k for j, k in enumerate(ks) if got[j] != want[1][k]]
        assert not bad, (tag, "runs", bad[:8])
        assert ed.cpu().tolist() == eds, (tag, "runs, distances")
    if "edits" in modes:
        ln = torch.full((n,), -1, dtype=torch.int32, device=dev)
        rc = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ed.fill_(-1), st.fill_(-1)
        aligner.align_device_edits(n, seq, desc, arena, ed, ln, st, rc, W=W, O=O, **kw)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n and ed.cpu().tolist() == eds, (tag, "edits")
        lh = ln.cpu().tolist()
        bad = [k for j, k in enumerate(ks) if arena[2 * off[k]: 2 * off[k] + lh[j]].cpu().numpy().tobytes() != py_encode(want[1][k], W, O)]
        assert not bad, (tag, "edits", bad[:8])
        assert rc.cpu().tolist() == [len(pi.cigar_runs(want[1][k])) for k in ks], (tag, "edits, run counts")
    if "distance" in modes:
        te = torch.full((n,), -1, dtype=torch.int32, device=dev)
        ed.fill_(-1), st.fill_(-1)
        aligner.align_device_distance(n, seq, desc, ed, te, st, W=W, O=O, **kw)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [0] * n and ed.cpu().tolist() == eds, (tag, "distance")
        assert te.cpu().tolist() == [_text_end(want[1][k]) for k in ks], (tag, "text_end")


# ------------------------------------------------------------------------------------------------ 1. sequence offsets and lengths
# one setting per kernel class (plane_inputs.MAPPING_SETTINGS), both forms of the default kernel (a launch this small takes the
# split form: two wavefronts per window; waves_per_cu = 16 the other), and the two GenASM-row mappings
VARIANTS = {
    "default, split": (64, 33, {}),
    "default, one wavefront": (64, 33, {"waves_per_cu": 16}),
    "halves": (64, 2, {}),
    "parts": (129, 65, {}),
    "hbm": (64, 0, {}),
    "rows, 8 lanes per pair": (64, 33, {"lanes_per_pair": 8}),
    "multiword rows, 32 lanes per pair": (128, 65, {"lanes_per_pair": 32}),
}


@pytest.mark.parametrize("swept", ["text", "read"])
@pytest.mark.parametrize("layout", ["linear", "groups"])
def test_sequence_offsets(aligner, expected, layout, swept):
    """text_off, text_len, read_off past 2^31 and 2^32 (and a straddler at each) in every align kernel class and output mode,
    on both strands, texts exact and declared as mapping declares them: forward suffixes up to the buffer's end (lengths past
    2^31 and, saturating, past 2^32 - 1), reversed stretches from base 0 (of which the last 2^32 - 1 bases are the text)."""
    torch, dev = _dev()
    b = bo.batch()
    t0 = time.perf_counter()
    P, seq, lay = _upload(aligner, layout, swept)
    plain = [k for k in range(b.n) if not b.read_rc[k] and not b.text_rc[k]]
    off, caps, total = _low_slices(b)
    arena = torch.zeros(2 * total, dtype=torch.uint8, device=dev)
    bo.plan_bytes(seq.numel() * 8, arena.numel())
    try:
        for declare in ("exact", "mapping"):
            sd = P.desc(declare)
            desc_all, desc_plain = _desc(sd, off, caps), _desc(sd, off, caps, plain)
            for name, (W, O, kw) in VARIANTS.items():
                rows = "lanes_per_pair" in kw
                if rows and layout == "groups":
                    continue                                          # word strides belong to the one-pair-per-lane kernels
                want = expected[(W, O, declare)]
                tag = (layout, swept, declare, name)
                with _Strands(aligner, on=not rows):
                    if rows:                                          # no strands in the row mappings: the unflagged pairs
                        _align_all_modes(aligner, seq, desc_plain, plain, off, caps, arena, want, kw, modes=("runs",), W=W, O=O, tag=tag)
                    else:
                        _align_all_modes(aligner, seq, desc_all, list(range(b.n)), off, caps, arena, want, dict(kw, stranded=1, **lay),
                                         W=W, O=O, tag=tag)
    finally:
        del seq, arena
        torch.cuda.empty_cache()
    print("test_sequence_offsets[%s-%s]: %.2f s" % (layout, swept, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ 2. run-slice offsets
def _need_gib(level):
    """The 2^32 level holds buffers of 8 GiB: skipped only on a device with less than 32 GiB free."""
    torch, dev = _dev()
    if level == 32 and torch.cuda.mem_get_info()[0] < 32 << 30:
        pytest.skip("needs 8 GiB buffers: less than 32 GiB of device memory free")


def _aligned_arena(aligner, expected, level, declare="mapping"):
    """The batch aligned (64/33, linear layout, texts swept) into slices placed at `level` -> (P, seq, desc, S, arena, nr, ed, st)"""
    torch, dev = _dev()
    b = bo.batch()
    want = expected[(64, 33, declare)]
    n_runs = [len(pi.cigar_runs(c)) for c in want[1]]
    S = bo.place_slices([b.cap(k) for k in range(b.n)], n_runs, level)
    P, seq, _ = _upload(aligner, "linear", "text")
    arena = torch.empty(2 * S.size, dtype=torch.uint8, device=dev)
    _fill_sentinels(arena, S, 2)
    desc = _desc(P.desc(declare), S.off, S.cap)
    return b, want, n_runs, P, seq, desc, S, arena


@pytest.mark.parametrize("level", [31, 32])
def test_run_slice_offsets(aligner, expected, level):
    """cigar_off past 2^31 runs (byte 2^32) and 2^32 runs, a slice straddling each, in both writing modes (runs; edit streams at
    byte 2 cigar_off); then scrg_compact_runs / _packed from those slices to low dense offsets and to dense
    offsets past both thresholds (odd destinations, pairs of <= 16 and of more runs), and scrg_unpack_runs on the packed
    buffer.  Where an offset that lost 2^31 or 2^32 would write lies a sentinel, untouched afterwards."""
    _need_gib(level)
    torch, dev = _dev()
    t0 = time.perf_counter()
    b, want, n_runs, P, seq, desc, S, arena = _aligned_arena(aligner, expected, level)
    dense = packed = back = None
    try:
        ks = list(range(b.n))
        with _Strands(aligner):
            for mode in ("edits", "runs"):                                # (the runs last: the compactions take them from there)
                _align_all_modes(aligner, seq, desc, ks, S.off, S.cap, arena, want, dict(stranded=1), modes=(mode,), tag=("slices", level))
                assert _sentinels_intact(arena, S, 2), mode
        del seq
        seq = None
        nr = torch.tensor(n_runs, dtype=torch.int32, device=dev)
        aligner.set_stream(0)
        # scrg_encode_edit_stream reads the slices (its stream offsets are its own output: a cursor that starts at 0)
        streams = [py_encode(c, 64, 33) for c in want[1]]
        need = sum((len(x) + 3) // 4 * 4 for x in streams)
        stream = torch.zeros(need + 64, dtype=torch.uint8, device=dev)
        s_off = torch.empty(b.n, dtype=torch.int64, device=dev)
        s_len = torch.empty(b.n, dtype=torch.int32, device=dev)
        tot = torch.empty(2, dtype=torch.int64, device=dev)
        aligner.encode_edit_stream(b.n, desc, arena, nr, stream, s_off, s_len, tot)
        torch.cuda.synchronize()
        assert tot.cpu().tolist() == [need, 0] and s_len.cpu().tolist() == [len(x) for x in streams]
        sh, oh = stream.cpu().numpy().tobytes(), s_off.cpu().tolist()
        assert all(sh[o: o + len(x)] == x for o, x in zip(oh, streams))
        for where in ("low", "high"):
            if where == "low":
                D = None
                d_off = np.cumsum([0] + n_runs[:-1]) + 1                   # (odd first destination)
                size = int(sum(n_runs)) + 16
            else:
                D = bo.place_slices(n_runs, n_runs, level, align=1)
                d_off, size = np.array(D.off), D.size
            assert {int(o) % 2 for o, m in zip(d_off, n_runs) if m} == {0, 1}
            assert any(0 < m <= 16 for m in n_runs) and any(m > 16 for m in n_runs)
            doff = torch.from_numpy(d_off.astype(np.int64)).to(dev)
            # --- two bytes per run
            bo.plan_bytes(arena.numel(), 2 * size)
            dense = torch.empty(2 * size, dtype=torch.uint8, device=dev)
            if D:
                _fill_sentinels(dense, D, 2)
            aligner.compact_runs(b.n, desc, arena, nr, doff, dense)
            torch.cuda.synchronize()
            for k in range(b.n):
                got = dense[2 * int(d_off[k]): 2 * (int(d_off[k]) + n_runs[k])].cpu().numpy().tobytes()
                assert got == _runs_bytes(want[1][k]), (where, "compact_runs", k)
            assert D is None or _sentinels_intact(dense, D, 2)
            if D:
                # scrg_select_best on these arrays (groups of three consecutive pairs; it takes no offsets itself), then the
                # winners alone gathered from the high slices to the high destinations: the losers' places stay as they were
                key = torch.tensor([k // 3 for k in range(b.n)], dtype=torch.int32, device=dev)
                ed_t = torch.tensor(want[0], dtype=torch.int64, device=dev)
                st_t = torch.zeros(b.n, dtype=torch.int32, device=dev)
                nr_b, is_best = nr.clone(), torch.full((b.n,), 9, dtype=torch.uint8, device=dev)
                aligner.select_best(b.n, key, ed_t, st_t, nr_b, is_best)
                win = [min(range(g, min(g + 3, b.n)), key=lambda k: (want[0][k], k)) for g in range(0, b.n, 3)]
                marks = [1 if k in win else 0 for k in range(b.n)]
                torch.cuda.synchronize()
                assert is_best.cpu().tolist() == marks and st_t.cpu().tolist() == [0 if m else 3 for m in marks]
                assert nr_b.cpu().tolist() == [m * x for m, x in zip(marks, n_runs)]
                for k in range(b.n):
                    dense[2 * int(d_off[k]): 2 * (int(d_off[k]) + n_runs[k])].fill_(0x77)
                aligner.compact_runs(b.n, desc, arena, nr_b, doff, dense)
                torch.cuda.synchronize()
                for k in range(b.n):
                    got = dense[2 * int(d_off[k]): 2 * (int(d_off[k]) + n_runs[k])].cpu().numpy().tobytes()
                    assert got == (_runs_bytes(want[1][k]) if marks[k] else b"\x77" * (2 * n_runs[k])), ("winners", k)
                assert _sentinels_intact(dense, D, 2)
            dense = None
            # --- one byte per run, and back
            packed = torch.empty(size, dtype=torch.uint8, device=dev)
            if D:
                _fill_sentinels(packed, D, 1)
            aligner.compact_runs_packed(b.n, desc, arena, nr, doff, packed)
            torch.cuda.synchronize()
            for k in range(b.n):                                          # op in bits 7..6 (= X I D), count in bits 5..0
                got = packed[int(d_off[k]): int(d_off[k]) + n_runs[k]].cpu().numpy().tolist()
                assert "".join("%d%s" % (x & 63, "=XID"[x >> 6]) for x in got) == want[1][k], (where, "compact_runs_packed", k)
            assert D is None or _sentinels_intact(packed, D, 1)
            if where == "high":                                           # unpack the whole buffer: run indices past the thresholds
                keep = arena
                arena = None
                del keep                                                  # (the arena makes room: 8 GiB of runs come back)
                back = torch.empty(2 * size, dtype=torch.uint8, device=dev)
                aligner.unpack_runs(size, packed, back)
                torch.cuda.synchronize()
                for k in range(b.n):
                    got = back[2 * int(d_off[k]): 2 * (int(d_off[k]) + n_runs[k])].cpu().numpy().tobytes()
                    assert got == _runs_bytes(want[1][k]), ("unpack_runs", k)
                back = None
            packed = None
    finally:
        aligner.use_own_stream()
        del seq, arena, dense, packed, back
        torch.cuda.empty_cache()
    print("test_run_slice_offsets[%d]: %.2f s" % (level, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ 3. edit streams
def _write_at(buf_u8, off, data):
    """data (bytes) -> buf_u8[off:]: a copy of its own, so that nothing but these bytes of an uninitialised buffer is written."""
    torch, dev = _dev()
    if len(data):
        buf_u8[off: off + len(data)].copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(dev))


@pytest.mark.parametrize("level", [31, 32])
def test_edit_stream_offsets(aligner, expected, level, monkeypatch):
    """scrg_decode_edit_stream with stream_off past 2^31 and 2^32 bytes and dense_off past 2^31 and 2^32 runs (a straddler at
    each), count-only and full, in the lane kernel, the quad kernel and the default choice, against the oracle's runs."""
    _need_gib(level)
    torch, dev = _dev()
    t0 = time.perf_counter()
    b = bo.batch()
    W, O = 64, 33
    want = expected[(W, O, "mapping")]
    streams = [py_encode(c, W, O) for c in want[1]]
    n_runs = [len(pi.cigar_runs(c)) for c in want[1]]
    lens = [len(s) for s in streams]
    S = bo.place_slices([(x + 3) // 4 * 4 for x in lens], lens, level, align=4)              # bytes
    D = bo.place_slices(n_runs, n_runs, level, align=1)                                      # runs
    assert all(o % 4 == 0 for o in S.off)
    bo.plan_bytes(S.size, 2 * D.size)
    stream = torch.empty(S.size, dtype=torch.uint8, device=dev)
    dense = torch.empty(2 * D.size, dtype=torch.uint8, device=dev)
    try:
        _fill_sentinels(stream, S, 1)                                   # (read by a decoder whose stream offset lost 2^31 or 2^32)
        for k in range(b.n):
            _write_at(stream, S.off[k], streams[k] + bytes((-lens[k]) % 4))
        s_off = torch.tensor(S.off, dtype=torch.int64, device=dev)
        s_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        d_off = torch.tensor(D.off, dtype=torch.int64, device=dev)
        r_len = torch.tensor([len(r) for r in b.reads], dtype=torch.int64, device=dev)
        aligner.set_stream(0)
        for dec in ("lane", "quad", None):
            if dec:
                monkeypatch.setenv("SCRG_DEC_KERNEL", dec)
            else:
                monkeypatch.delenv("SCRG_DEC_KERNEL", raising=False)
            cnt = torch.full((b.n,), -1, dtype=torch.int32, device=dev)
            nbad = torch.zeros(1, dtype=torch.int32, device=dev)
            aligner.decode_edit_stream(b.n, stream, s_off, s_len, r_len, 1, None, None, cnt, nbad, W=W, O=O)
            torch.cuda.synchronize()
            assert cnt.cpu().tolist() == n_runs and int(nbad.item()) == 0, (dec, "count only")
            _fill_sentinels(dense, D, 2)
            for k in range(b.n):
                dense[2 * D.off[k]: 2 * (D.off[k] + n_runs[k])].zero_()
            aligner.decode_edit_stream(b.n, stream, s_off, s_len, r_len, 1, d_off, dense, cnt, nbad, W=W, O=O)      # (the counts go in)
            torch.cuda.synchronize()
            assert int(nbad.item()) == 0, (dec, "full")
            bad = [k for k in range(b.n) if _cigar_of(dense[2 * D.off[k]: 2 * (D.off[k] + n_runs[k])].cpu().numpy()) != want[1][k]]
            assert not bad, (dec, bad[:8])
            assert _sentinels_intact(dense, D, 2), dec
    finally:
        aligner.use_own_stream()
        del stream, dense
        torch.cuda.empty_cache()
    print("test_edit_stream_offsets[%d]: %.2f s" % (level, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ 4. the walk passes
def _runs_buffer(S, cigars):
    """An uninitialised buffer of S.size runs with every pair's runs at its offset and sentinels where a wrapped offset lands."""
    torch, dev = _dev()
    buf = torch.empty(2 * S.size, dtype=torch.uint8, device=dev)
    _fill_sentinels(buf, S, 2)
    for k, c in enumerate(cigars):
        _write_at(buf, 2 * S.off[k], _runs_bytes(c))
    return buf


@pytest.mark.parametrize("level", [31, 32])
def test_encoder_stream_offsets(aligner, expected, level):
    """scrg_encode_edit_stream with its stream cursor carried past 2^31 and 2^32 bytes: its offsets are its own output (one
    reservation per wavefront from a cursor that starts at 0), so millions of descriptors repeat the batch's slices — mostly the
    long noisy pairs, every sixteenth row the next pair of the whole batch, empty ones included — until the streams fill the
    buffer past the threshold.  The slices themselves lie past the thresholds (runs straight from the oracle's CIGARs).  Every
    stream is compared on the device with the encoding of its pair's CIGAR at the offset the call reports; the reservations are
    disjoint and add up to the total, so the place an offset that lost 2^31 or 2^32 would write is another row's stream, which
    is compared too; behind the total lies a sentinel."""
    _need_gib(level)
    torch, dev = _dev()
    t0 = time.perf_counter()
    b = bo.batch()
    W, O = 64, 33
    cigars = expected[(W, O, "exact")][1]
    streams = [py_encode(c, W, O) for c in cigars]
    n_runs = [len(pi.cigar_runs(c)) for c in cigars]
    lens = np.array([len(x) for x in streams], dtype=np.int64)
    r4 = (lens + 3) // 4 * 4
    long_ = [k for k in range(b.n) if b.groups[k] == "long_noisy"]
    top = (T31 if level == 31 else T32) + (1 << 26)
    per16 = int(r4[long_].mean() * 15 + r4.mean())                   # bytes per 16 rows, roughly
    n = (top // per16 + 2) * 16
    rows = np.arange(n)
    src = np.where(rows % 16 == 0, (rows // 16) % b.n, np.array(long_)[rows % len(long_)])
    total = int(r4[src].sum())
    assert total > top and n < 1 << 24
    S = bo.place_slices([b.cap(k) for k in range(b.n)], n_runs, level)
    tail = 1 << 16
    bo.plan_bytes(2 * S.size, total + tail, n * (48 + 4 + 8 + 4))
    arena = _runs_buffer(S, cigars)
    stream = torch.empty(total + tail, dtype=torch.uint8, device=dev)
    try:
        stream[total:].fill_(SENTINEL)
        src_t = torch.from_numpy(src).to(dev)
        small = np.zeros((b.n, 6), dtype=np.int64)
        small[:, 3], small[:, 4], small[:, 5] = [len(r) for r in b.reads], S.off, S.cap
        desc = torch.from_numpy(small).to(dev)[src_t].contiguous()
        nr = torch.tensor(n_runs, dtype=torch.int32, device=dev)[src_t].contiguous()
        s_off = torch.full((n,), -2, dtype=torch.int64, device=dev)
        s_len = torch.full((n,), -1, dtype=torch.int32, device=dev)
        tot = torch.empty(2, dtype=torch.int64, device=dev)
        aligner.set_stream(0)
        aligner.encode_edit_stream(n, desc, arena, nr, stream, s_off, s_len, tot, W=W, O=O)
        torch.cuda.synchronize()
        assert tot.cpu().tolist() == [total, 0]
        assert bool((stream[total:] == SENTINEL).all().item())
        lens_t, r4_t = torch.from_numpy(lens).to(dev)[src_t], torch.from_numpy(r4).to(dev)[src_t]
        assert torch.equal(s_len.to(torch.int64), lens_t)
        # disjoint reservations of whole dwords that fill [0, total): sorted by offset, each begins where the one before ends
        busy = r4_t > 0
        so, order = torch.sort(s_off[busy])
        ends = so + r4_t[busy][order]
        assert int(so[0].item()) == 0 and int(ends[-1].item()) == total and torch.equal(so[1:], ends[:-1]) and bool((so % 4 == 0).all().item())
        assert int(so[-1].item()) > (T31 if level == 31 else T32)
        # every stream, and its padding up to the dword, on the device: the rows of one pair in chunks
        for k in sorted(set(src.tolist())):
            if not r4[k]:
                continue
            want = torch.from_numpy(np.frombuffer(streams[k] + bytes(int(r4[k] - lens[k])), dtype=np.uint8).copy()).to(dev)
            at = s_off[src_t == k]
            step = max(1, (64 << 20) // int(r4[k]))
            col = torch.arange(int(r4[k]), dtype=torch.int64, device=dev)
            for a in range(0, at.numel(), step):
                got = stream[at[a: a + step, None] + col[None, :]]
                assert bool((got == want[None, :]).all().item()), ("stream of pair", k, "rows from", a)
        # the straddlers and a sample on the host
        oh = s_off.cpu().numpy()
        T = T31 if level == 31 else T32
        pick = set(np.nonzero((oh < T) & (oh + r4[src] > T))[0].tolist()) | set(np.nonzero((oh < T31) & (oh + r4[src] > T31))[0].tolist())
        assert pick                                                   # (the reservations are gapless: one lies across each threshold below the total)
        pick |= set(range(0, n, max(1, n // 150)))
        for r in sorted(pick):
            k = int(src[r])
            assert stream[int(oh[r]): int(oh[r]) + len(streams[k])].cpu().numpy().tobytes() == streams[k], (r, k)
        assert _sentinels_intact(arena, S, 2)
    finally:
        aligner.use_own_stream()
        del arena, stream
        torch.cuda.empty_cache()
    print("test_encoder_stream_offsets[%d]: %.2f s, %d rows, %d bytes of streams" % (level, time.perf_counter() - t0, n, total))


def _render_and_check(call, lengths_call, want, textbuf, level, what):
    """lengths pass, then the render pass into textbuf at offsets past the thresholds; want: every pair's string."""
    torch, dev = _dev()
    n = len(want)
    tl = torch.full((n,), -1, dtype=torch.int64, device=dev)
    lengths_call(tl)
    torch.cuda.synchronize()
    assert tl.cpu().tolist() == [len(s) + 1 for s in want], (what, "lengths")
    sizes = [len(s) + 1 for s in want]
    X = bo.place_slices(sizes, sizes, level, align=1)                                        # bytes
    assert X.size <= textbuf.numel()
    _fill_sentinels(textbuf, X, 1)
    off = torch.tensor(X.off, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call(tl, off, textbuf, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0, (what, "bad")
    wrong = [k for k in range(n) if textbuf[X.off[k]: X.off[k] + sizes[k]].cpu().numpy().tobytes() != want[k].encode() + b"\0"]
    assert not wrong, (what, wrong[:8])
    assert _sentinels_intact(textbuf, X, 1), what


@pytest.mark.parametrize("level", [31, 32])
def test_walk_pass_offsets(aligner, expected, level):
    """scrg_cigar_text_lengths / _render (three forms), scrg_diff_lengths / _render (md, cs), scrg_report_device and
    scrg_clip_device (plain and applied), fed runs at stride 6 from slices and at stride 1 from dense offsets past 2^31 and 2^32
    runs, sequences at the offsets of group 1 in both layouts and on both strands, and text_offset / diff_offset past 2^31 and
    2^32 bytes; against the models.  `bad` stays 0 and every report verdict is 0."""
    _need_gib(level)
    from scrooge_amd import api
    from tests import cigar_form_model as fm, clip_model as cm, diff_model as dm, report_model as rm
    torch, dev = _dev()
    t0 = time.perf_counter()
    b = bo.batch()
    W, O = 64, 33
    eds, cigars = expected[(W, O, "exact")]
    runs = [pi.cigar_runs(c) for c in cigars]
    n_runs = [len(r) for r in runs]
    n = b.n
    nr = torch.tensor(n_runs, dtype=torch.int32, device=dev)
    ed = torch.tensor(eds, dtype=torch.int64, device=dev)
    textbuf = torch.empty((T31 if level == 31 else T32) + (1 << 27), dtype=torch.uint8, device=dev)
    want_forms = {form: [fm.model(form, r) for r in runs] for form in ("windowed", "merged", "m")}
    want_clip = [cm.model(r) for r in runs]
    want_rep = [rm.model(b.texts[k], b.reads[k], runs[k], eds[k]) for k in range(n)]
    assert all(w["verdict"] == 0 for w in want_rep)
    buf = seq = None
    try:
        for source, layout, swept in (("slices", "linear", "text"), ("dense", "groups", "read")):
            P, seq, lay = _upload(aligner, layout, swept)
            if source == "slices":
                S = bo.place_slices([b.cap(k) for k in range(n)], n_runs, level)
                ro, stride = None, 6
            else:
                S = bo.place_slices(n_runs, n_runs, level, align=1)
                ro, stride = torch.tensor(S.off, dtype=torch.int64, device=dev), 1
            bo.plan_bytes(textbuf.numel(), 2 * S.size, seq.numel() * 8)
            buf = _runs_buffer(S, cigars)
            sd = P.desc("exact")
            desc = _desc(sd, S.off, S.cap)
            # the diff kernels take forward texts only: the stored stretch, unflagged (for a reversed text the model's text is
            # what is stored — the strings are a rendering of runs over bases, whatever aligned them)
            fwd_text = [bo.revcomp(b.texts[k]) if b.text_rc[k] else b.texts[k] for k in range(n)]
            desc_fwd = _desc([(to & (bo.FLAG - 1), tl, r, rl) for to, tl, r, rl in sd], S.off, S.cap)
            what = (source, layout, level)
            with _Strands(aligner):
                for form in ("windowed", "merged", "m"):
                    _render_and_check(lambda tl, off, out, bad: aligner.cigar_text_render(form, n, buf, ro, stride, nr, tl, off, out, bad, pairs=desc),
                                      lambda tl: aligner.cigar_text_lengths(form, n, buf, ro, stride, nr, tl, pairs=desc),
                                      want_forms[form], textbuf, level, what + (form,))
                for kind in ("md", "cs"):
                    want = [dm.model(kind, fwd_text[k], b.reads[k], runs[k]) for k in range(n)]
                    _render_and_check(lambda tl, off, out, bad: aligner.diff_render(kind, n, seq, desc_fwd, buf, ro, stride, nr, tl, off, out, bad,
                                                                                    stranded=1, **lay),
                                      lambda tl: aligner.diff_lengths(kind, n, seq, desc_fwd, buf, ro, stride, nr, tl, stranded=1, **lay),
                                      want, textbuf, level, what + (kind,))
                rep = torch.full((n, 8), -1, dtype=torch.int32, device=dev)
                fail = torch.zeros(1, dtype=torch.int32, device=dev)
                aligner.report_device(n, seq, desc, buf, ro, stride, nr, ed, None, rep, fail, stranded=1, **lay)
                torch.cuda.synchronize()
                got = rep.cpu().numpy().view(np.uint32).copy().view(api.report_dtype()).reshape(n)
                for k in range(n):
                    assert {f: int(got[k][f]) for f in rm.FIELDS} == want_rep[k], what + ("report", k)
                assert int(fail.item()) == 0
                for apply in (False, True):
                    rec = torch.full((n, 8), -1, dtype=torch.int32, device=dev)
                    nr2, desc2 = nr.clone(), desc.clone()
                    ro2 = None if ro is None else ro.clone()
                    aligner.clip_device(n, buf, ro2, stride, nr2, None, rec, apply=apply, pairs=desc2)
                    torch.cuda.synchronize()
                    got = rec.cpu().numpy().view(np.uint32).copy().view(api.clip_dtype()).reshape(n)
                    for k in range(n):
                        assert {f: int(got[k][f]) for f in cm.FIELDS} == want_clip[k], what + ("clip", apply, k)
                    first = [w["first_run"] if apply else 0 for w in want_clip]
                    assert nr2.cpu().tolist() == [w["n_runs"] if apply else m for w, m in zip(want_clip, n_runs)]
                    after = desc2.cpu().numpy().view(np.uint64)
                    if stride == 6:
                        assert after[:, 4].tolist() == [o + f for o, f in zip(S.off, first)], what + ("clip offsets", apply)
                        assert after[:, 5].tolist() == [c - f for c, f in zip(S.cap, first)]
                    else:
                        assert ro2.cpu().tolist() == [o + f for o, f in zip(S.off, first)], what + ("clip offsets", apply)
            assert _sentinels_intact(buf, S, 2), what
            buf = seq = None
            torch.cuda.empty_cache()
    finally:
        del buf, seq, textbuf
        torch.cuda.empty_cache()
    print("test_walk_pass_offsets[%d]: %.2f s" % (level, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ 5. pileup and sites
TARGET = 4096


@pytest.mark.parametrize("level", [31, 32])
def test_pileup_offsets(aligner, expected, level):
    """scrg_pileup_add with runs in slices past the thresholds and reads at the offsets of group 1 into a target of 4096
    positions, then adds with every target_start moved up by 2^31 and by 2^32 — nothing may land (a wrapped position would) and
    every pair with runs counts as out of range —, then scrg_pileup_sites_mark / _write with genome_off past 2^32 against
    site_model.  (An accumulator that itself reaches past 2^31 positions would take 60 GB: DESIGN.md.)"""
    _need_gib(level)
    from tests import pileup_model as pm, site_model as sm
    torch, dev = _dev()
    t0 = time.perf_counter()
    b = bo.batch()
    n = b.n
    cigars = expected[(64, 33, "exact")][1]
    runs = [pi.cigar_runs(c) for c in cigars]
    n_runs = [len(r) for r in runs]
    starts = [(131 * k) % 3900 if k % 7 else TARGET - 40 + k for k in range(n)]            # some start inside and end outside, some outside
    want, outside = pm.empty(TARGET), 0
    for k in range(n):
        if runs[k]:
            outside += pm.model(runs[k], b.reads[k], starts[k], TARGET, counts=want)[1]
    assert 0 < outside < n and want[pm.INS].sum() > 50 and want[pm.DEL].sum() > 50
    with_runs = sum(1 for r in runs if r)
    S = bo.place_slices([b.cap(k) for k in range(n)], n_runs, level)
    P, seq, lay = _upload(aligner, "linear", "read")
    buf = _runs_buffer(S, cigars)
    bo.plan_bytes(2 * S.size, seq.numel() * 8)
    try:
        desc = _desc(P.desc("exact"), S.off, S.cap)
        nr = torch.tensor(n_runs, dtype=torch.int32, device=dev)
        acc = torch.zeros(pm.PLANES * (TARGET + 1), dtype=torch.int32, device=dev)
        oor = torch.zeros(1, dtype=torch.int32, device=dev)
        aligner.set_stream(0)
        for shift, expect_oor in ((0, outside), (T31, with_runs), (T32, with_runs), (T32 + T31, with_runs)):
            ts = torch.tensor([s + shift for s in starts], dtype=torch.int64, device=dev)
            oor.zero_()
            aligner.pileup_add(n, seq, desc, buf, None, 6, nr, None, ts, TARGET, acc, oor, stranded=1)
            torch.cuda.synchronize()
            assert int(oor.item()) == expect_oor, ("target_start +", shift)
            edges = acc.cpu().numpy().view(np.uint32).reshape(pm.PLANES, TARGET + 1)
            assert pm.edges_to_counts(edges).tobytes() == want.tobytes(), ("target_start +", shift)
        # the same from dense offsets (stride 1) past the thresholds, into a second accumulator
        del buf
        D = bo.place_slices(n_runs, n_runs, level, align=1)
        buf = _runs_buffer(D, cigars)
        acc2 = torch.zeros_like(acc)
        oor.zero_()
        aligner.pileup_add(n, seq, desc, buf, torch.tensor(D.off, dtype=torch.int64, device=dev), 1, nr, None,
                           torch.tensor(starts, dtype=torch.int64, device=dev), TARGET, acc2, oor, stranded=1)
        aligner.pileup_finish(TARGET, acc2)
        torch.cuda.synchronize()
        assert int(oor.item()) == outside and acc2.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
        # sites: the genome is what the sequence buffer holds from a base past 2^32 (an odd offset modulo 32)
        k0 = max(range(n), key=lambda k: len(b.texts[k]))
        genome_off = P.extent("text", k0)[0] + 5
        assert genome_off > T32 and genome_off % 32 != 0
        genome = P.image.read(genome_off, TARGET)
        decoys = [P.image.read(genome_off - T, TARGET) for T in bo.THRESHOLDS]
        assert all(d != genome for d in decoys)
        for rule in ((1, 1, 0), (3, 2, 200)):
            model = sm.sites(want, sm.ref_codes(genome), rule)
            assert len(model) > 20 and all(sm.sites(want, sm.ref_codes(d), rule).tobytes() != model.tobytes() for d in decoys)
            scratch = torch.zeros(aligner.pileup_sites_scratch_bytes(TARGET) // 8, dtype=torch.int64, device=dev)
            n_sites = torch.full((1,), -1, dtype=torch.int64, device=dev)
            aligner.pileup_sites_mark(TARGET, acc2, seq, genome_off, rule, scratch, n_sites)
            torch.cuda.synchronize()
            assert int(n_sites.item()) == len(model), rule
            out = torch.zeros(5 * len(model), dtype=torch.int64, device=dev)
            aligner.pileup_sites_write(TARGET, acc2, seq, genome_off, scratch, len(model), out)
            torch.cuda.synchronize()
            assert out.cpu().numpy().view(np.uint8).view(sm.DTYPE).tobytes() == model.tobytes(), rule
    finally:
        aligner.use_own_stream()
        del buf, seq
        torch.cuda.empty_cache()
    print("test_pileup_offsets[%d]: %.2f s" % (level, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ 6. selection
@pytest.mark.parametrize("team", [4, 64])
def test_mate_starts_past_the_thresholds(aligner, team):
    """scrg_select_mates with every start raised by 2^31 + 12345 and by 2^32 + 12345, and with spans that straddle a threshold
    (one mate below, one above): mate_model on the shifted starts, which must also be its answer on the unshifted batch with
    the start fields shifted — winners, costs, spans and flags do not depend on where the genome's origin is."""
    from tests import mate_model as mm
    from tests.test_mates_gpu import SHAPES, draw_mate, run_and_check
    rng = np.random.Generator(np.random.PCG64(6400 + team))
    shapes = SHAPES[team]
    mates = [draw_mate(rng, a, b, 0) for a, b in [shapes[0]] + [shapes[int(k)] for k in rng.integers(0, len(shapes), 70)]]
    rule = (200, 900, mm.FR, 1)
    aligner.set_stream(0)
    try:
        base = run_and_check(aligner, [[dict(s) for s in m] for m in mates], rule, team=team)
        assert sum(1 for w in base if w["flags"] & mm.PROPER) > 5
        for shift in (T31 + 12345, T32 + 12345):
            moved = [[dict(s, start=[x + shift for x in s["start"]]) for s in m] for m in mates]
            got = run_and_check(aligner, moved, rule, team=team)                               # (asserts the kernel = the model)
            assert got == base                                                                 # and the model = itself, unshifted
        # spans across a threshold: starts drawn 0..2000 around T - 1000, so that mates fall on either side of it
        for T in bo.THRESHOLDS:
            moved = [[dict(s, start=[x + T - 1000 for x in s["start"]]) for s in m] for m in mates]
            assert sum(1 for a, b_ in moved if a["start"] and b_["start"] and min(a["start"]) < T <= max(b_["start"])) > 5
            assert run_and_check(aligner, moved, rule, team=team) == base
        # spans of more than 2^31 and 2^32 themselves: proper only under a rule that admits them, saturated in the record
        far = [[dict(m[0]), dict(m[1], start=[x + T32 + 12345 for x in m[1]["start"]])] for m in mates]
        wants = run_and_check(aligner, far, (0, 2 ** 64 - 1, mm.ANY, 0), team=team)
        assert any(w["span"] == mm.NONE32 for w in wants)
        wants = run_and_check(aligner, far, (T31, T32 + (1 << 20), mm.ANY, 0), team=team)
        assert sum(1 for w in wants if w["flags"] & mm.PROPER) > 5
        assert not any(w["flags"] & mm.PROPER for w in run_and_check(aligner, far, rule, team=team))
    finally:
        aligner.use_own_stream()


# ------------------------------------------------------------------------------------------------ 7. the host path
GENOME_LEN = T31 + (1 << 22)
LOCUS = 20_000


class _Cut:
    """The genome as the oracle gets it: genome[pos:] is cut to K bases, genome[:pos] to its last K (tests/anchored_inputs.py
    composes its expectations from these two slices)."""

    def __init__(self, g, k):
        self.g, self.k = g, k

    def __getitem__(self, s):
        if s.start is None:
            return self.g[max(0, s.stop - self.k): s.stop].tobytes()
        assert s.stop is None
        return self.g[s.start: s.start + self.k].tobytes()


@pytest.fixture(scope="module")
def big_genome(aligner):
    """One resident genome of 2^31 + 2^22 bases, set once: one letter with random stretches planted — near the beginning,
    across 2^31, past it, and up to the last base — and reads drawn from them."""
    t0 = time.perf_counter()
    inp = sb.big_inputs()                            # (tests/seed_big.py draws them, so that its sparse model knows the same genome)
    assert (sb.GENOME_LEN, sb.LOCUS) == (GENOME_LEN, LOCUS)
    g = inp["genome"].array()
    t1 = time.perf_counter()
    aligner.set_genome_array(g)
    t2 = time.perf_counter()
    print("big_genome: %.2f s to make the array, %.2f s to set it (pack and upload)" % (t1 - t0, t2 - t1))
    yield dict(g=g, cut=_Cut(g, 4 * 3000 + 4 * 64), reads=inp["reads"], where=inp["where"], loci=inp["loci"], stored=inp["stored"],
               sparse=inp["genome"])
    aligner.clear_genome()


def test_host_path_past_2_31(aligner, oracle, big_genome):
    """The resident-genome calls with candidate starts below, across and past 2^31 and texts that end with the genome's last
    base: scrg_align_mapping_directed on both strands, leftward candidates whose positions lie past 2^31 (text_off = 0 | REVCOMP,
    text_len = position), scrg_align_mapping_paired with mates on either side of 2^31, scrg_align_mapping_anchored with seeds
    past 2^31, a diff="md" and a report=True call — each against the oracle on the cut suffix (or prefix)."""
    from scrooge_amd import api
    from tests import anchored_inputs as ai, diff_model as dm, mate_model as mm, report_model as rm
    from tests.test_mates_gpu import check_paired, model_records
    t0 = time.perf_counter()
    G = big_genome
    cut, where = G["cut"], G["where"]
    named = G["reads"]
    n = len(named)
    assert sum(p > T31 for p in where) >= 4 and any(p < T31 < p + len(r) for p, r in zip(where, named)) and any(p + len(r) > GENOME_LEN for p, r in zip(where, named))
    # --- both strands, rightward: the true start and one wrong location on the other side of 2^31
    rev = [[k % 2, (k + 1) % 2] for k in range(n)]
    stored = [ai.revcomp(r) if k % 2 else r for k, r in enumerate(named)]
    cands = [[p, (p + T31 + 777) % (GENOME_LEN - 100)] for p in where]
    left = [[0, 0] for _ in range(n)]
    want = ai.directed_expectation(oracle, cut, stored, cands, rev, left)
    out = aligner.align_mapping_directed(stored, cands, reverse=rev, arrays=True, outputs=2)
    assert out["edit_distance"].tolist() == want["eds"] and not out["status"].any()
    assert ai.cigars_from_arrays(out, 2) == want["cigars"]
    assert all(want["eds"][2 * k] < len(named[k]) // 4 for k in range(n) if where[k] + len(named[k]) <= GENOME_LEN)      # (true loci really align)
    # the forward-only call on the forward reads
    fwd = [k for k in range(n) if k % 2 == 0]
    got = aligner.align_mapping(None, [stored[k] for k in fwd], [[where[k]] for k in fwd], arrays=True, outputs=0)
    assert got["edit_distance"].tolist() == [want["eds"][2 * k] for k in fwd]
    assert ai.cigars_from_arrays(got, 0) == [want["cigars"][2 * k] for k in fwd]
    # --- leftward candidates: where the rightward alignment ends, past 2^31 for most; every strand combination
    ends = [where[k] + want["text_end"][2 * k] for k in range(n)]
    l_cands = [[ends[k], ends[k]] for k in range(n)]
    l_rev = [[k % 2, k % 2] for k in range(n)]
    l_left = [[1, 0] for _ in range(n)]
    assert sum(e > T31 for e in ends) >= 5
    want_l = ai.directed_expectation(oracle, cut, stored, l_cands, l_rev, l_left)
    for outputs in (2, 16):
        out = aligner.align_mapping_directed(stored, l_cands, reverse=l_rev, leftward=l_left, arrays=True, outputs=outputs)
        assert out["edit_distance"].tolist() == want_l["eds"] and not out["status"].any(), outputs
        if outputs == 2:
            assert ai.cigars_from_arrays(out, 2) == want_l["cigars"]
        else:
            assert out["text_end"].tolist() == want_l["text_end"]
    assert all(want_l["eds"][2 * k] < len(named[k]) // 3 for k in range(n) if where[k] + len(named[k]) <= GENOME_LEN)
    # --- a mate pair on either side of 2^31 (reads 1: across, forward; a mate made here: past it, reverse), and one past it
    g = G["g"]
    p_b = T31 + 1200
    mate_b = ai.revcomp(ai.mutated(g[p_b: p_b + 300].tobytes(), np.random.Generator(np.random.PCG64(5)), err=0.03)[:250])
    p_a = T31 - 900
    mate_a = ai.mutated(g[p_a: p_a + 300].tobytes(), np.random.Generator(np.random.PCG64(6)), err=0.03)[:250]
    m_reads = [mate_a, mate_b, stored[4], stored[5]]
    m_cands = [[p_a, where[0]], [where[7], p_b], [where[4], p_a], [where[5]]]
    m_rev = [[0, 0], [1, 1], [0, 1], [1]]
    rule = (200, 5000, mm.FR, 2)
    plain = aligner.align_mapping_directed(m_reads, m_cands, reverse=m_rev, arrays=True)
    want_m = ai.directed_expectation(oracle, cut, m_reads, m_cands, m_rev, [[0] * len(c) for c in m_cands])
    assert plain["edit_distance"].tolist() == want_m["eds"]
    wants, _ = model_records(plain, m_reads, m_cands, m_rev, rule)
    got, mates = aligner.align_mapping_paired(m_reads, m_cands, reverse=m_rev, rule=api.MateRule(*rule), arrays=True)
    check_paired(got, mates, plain, wants)
    assert wants[0]["flags"] & mm.PROPER and wants[0]["winner"] == (0, 3) and wants[0]["span"] == p_b + 250 - p_a
    # --- anchors: seeds past 2^31 (and one across it)
    a_reads, anchors, a_rev = [], [], []
    for k in (1, 4, 7):
        ra = len(named[k]) // 2
        t_used = ai.text_used(oracle.align([cut[where[k]:]], [named[k][:ra]])[1][0])
        a_reads.append(stored[k]), anchors.append([(where[k] + t_used, ra)]), a_rev.append([k % 2])
    assert all(a[0][0] > T31 for a in anchors)
    want_a = ai.anchored_expectation(oracle, cut, a_reads, anchors, a_rev)
    out = aligner.align_anchored(a_reads, anchors, reverse=a_rev, arrays=True, outputs=2)
    assert out["edit_distance"].tolist() == want_a["ed"] and out["text_start"].tolist() == want_a["text_start"]
    assert ai.cigars_from_arrays(out, 2) == want_a["cigars"] and min(want_a["text_start"]) > T31 - 2000
    # --- side outputs: MD strings and the report of the rightward true candidates
    t_cands = [[p] for p in where]
    t_rev = [[k % 2] for k in range(n)]
    out = aligner.align_mapping_directed(stored, t_cands, reverse=t_rev, arrays=True, outputs=2, report=True)
    texts = [cut[p:] for p in where]
    runs = [ai.runs_of(want["cigars"][2 * k]) for k in range(n)]
    for k in range(n):
        assert {f: int(out["report"][k][f]) for f in rm.FIELDS} == rm.model(texts[k], named[k], runs[k], want["eds"][2 * k]), ("report", k)
    assert all(int(r["verdict"]) == 0 for r in out["report"])
    out = aligner.align_mapping(None, [stored[k] for k in fwd], [[where[k]] for k in fwd], arrays=True, outputs=2, diff="md")
    off, text = out["diff_offset"], out["diff_text"]
    assert [text[int(off[j]): int(off[j + 1]) - 1].decode() for j in range(len(fwd))] == [dm.model("md", texts[k], named[k], runs[k]) for k in fwd]
    print("test_host_path_past_2_31: %.2f s" % (time.perf_counter() - t0))


def _seed_bucket_bits(n_entries, k):
    """The bucket table's bits as DESIGN.md §3.12 states them: min(2k, clamp(ceil log2 entries, 8, 26))."""
    bits = 8
    while bits < 26 and (1 << bits) < n_entries:
        bits += 1
    return min(bits, 2 * k)


def _device_buffer(n_bytes):
    """What a device buffer of the host layer takes for n_bytes asked: an eighth and 256 bytes on top."""
    return n_bytes + n_bytes // 8 + 256


def test_seeding_past_2_31(aligner, oracle, big_genome):
    """scrg_genome_index and scrg_find_candidates on the resident genome of 2^31 + 2^22 bases, at the defaults (k 13, stride 4:
    2^29 + 2^20 - 3 entries, a 26-bit table with a bucket per key, the lookup reads no key) and at (16, 8) (2^28 entries, 64 keys
    per bucket, the searched form), unsampled and sampled (s = 5, s = 7: count, scan and emit over 2^21 workgroups), each at a hit
    budget of 1 MB and at the default.  The expected values are the plain Python model's on the sparse index of tests/seed_big.py —
    the host twin compiles the same seed_rule.h as the kernels and is not run at this size — which tests/test_seed_big.py holds
    to the dense model and the twin on 150 kb, and whose answers for these reads it shows to be their true loci.

    What it would catch.  p = e * stride in 32 bits, a signed index into genome[p >> 5], or (int32) p stored: the keys of every
    position past 2^31 become those of a position 2^31 lower (filler) or the positions wrap — test_a_lost_bit_31_changes_the_answer
    shows that either gives other candidates for every read used here that lies past 2^31 (nine candidate starts do, and one
    read straddles it), so the result is a mismatch, never luck.  A 32-bit d + 2^32 in the hit word, a 31-bit start in the
    anchor word or the rank, a signed copy of the uint32 starts into the uint64 output: the starts past 2^31 come back negative,
    low or clamped to 0, and the arrays differ.  A bucket table sized or indexed in int: keys in the upper half of the 2^26 table
    (any k-mer that starts with G or T) find no entries and their reads lose votes.  A block_base scan or a ballot prefix that
    breaks beyond 65 535 workgroups: n_entries differs from the model's count, which includes every filler window.  The read
    that runs from filler into a locus and the all-T read meet a key of 2^29 entries: an entry count kept in 16 bits, or
    hi - lo taken signed, would count them as hits instead of n_keys_over_max_occ."""
    from scrooge_amd import api
    from tests import anchored_inputs as ai
    G = big_genome
    stored, sparse = G["stored"], G["sparse"]
    t_all = time.perf_counter()
    try:
        # a rule whose entries do not count in 31 bits is refused, and leaves no index behind
        assert sb.n_positions(GENOME_LEN, 13, 1) == T31 + (1 << 22) - 12 > T31 - 1
        with pytest.raises(api.ScroogeError) as e:
            aligner.index_genome(api.SeedRule(stride=1))
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
        with pytest.raises(api.ScroogeError):
            aligner.index_info()
        for rule, s in sb.SETUPS:
            index, n_entries, considered = sb.sparse_index(sparse, rule[0], rule[1], s)
            want = sb.model_candidates(rule, s, index, stored)
            assert considered == (GENOME_LEN - rule[0]) // rule[1] + 1 and (n_entries == considered if s == 0 else n_entries < considered)
            assert sum(x > T31 for c in want[0] for x in c) >= 5
            assert any(x < T31 < x + len(r) for c, r in zip(want[0], stored) for x in c)
            assert want[3]["n_keys_over_max_occ"] > 0
            bits = _seed_bucket_bits(n_entries, rule[0])
            assert (bits, 2 * rule[0] - bits) == ((26, 0) if rule[0] == 13 else (26, 6))
            aligner.set_seed_sampling(s)
            for mb in (1, 0):
                t0 = time.perf_counter()
                info = aligner.index_genome(api.SeedRule(*rule, mb))
                t1 = time.perf_counter()
                tag = (rule, s, mb)
                assert info["n_entries"] == n_entries and info["n_positions"] == considered and info["smer"] == s, (tag, info)
                assert info["rule"] == api.SeedRule(*rule, mb or 256)
                assert info["device_bytes"] == 2 * _device_buffer(4 * (n_entries + 1)) + _device_buffer(4 * ((1 << bits) + 1)), (tag, info)
                got = aligner.find_candidates(stored, info=True)
                t2 = time.perf_counter()
                print("test_seeding_past_2_31: k %d stride %d s %d budget %d MB: %d entries, %.1f MiB on the device, index %.2f s, find_candidates %.3f s"
                      % (rule[0], rule[1], s, mb or 256, n_entries, info["device_bytes"] / 2**20, t1 - t0, t2 - t1))
                for what, g, w in zip(("starts", "strands", "votes"), got, want):
                    assert g == w, (tag, what, g, w)
                for counter in ("n_hits", "n_clusters", "n_keys_over_max_occ", "n_lookups"):
                    assert got[3][counter] == want[3][counter], (tag, counter)
            if (rule, s) == (sb.K13, 0):
                # end to end: the candidates found go into the resident mapping call; its distances are the oracle's on the cut suffix
                t0 = time.perf_counter()
                cands, rev = got[0], got[1]
                exp = ai.directed_expectation(oracle, G["cut"], stored, cands, rev, [[0] * len(c) for c in cands])
                out = aligner.align_mapping_directed(stored, cands, reverse=rev, arrays=True, best=True)
                assert out["edit_distance"].tolist() == exp["eds"] and len(exp["eds"]) == sum(len(c) for c in cands) >= 12
                assert all(len(c) <= 1 for c in cands) and not out["status"].any()          # (one candidate a read: each is its read's best)
                at = np.cumsum([0] + [len(c) for c in cands])
                assert all(exp["eds"][at[k]] < len(stored[k]) // 4 for k in range(len(G["where"])) if G["where"][k] + len(stored[k]) <= GENOME_LEN)
                assert aligner.index_info()["n_entries"] == n_entries          # (the mapping call left the index alone)
                print("test_seeding_past_2_31: the mapping call on the candidates found and the oracle: %.2f s" % (time.perf_counter() - t0))
    finally:
        aligner.set_seed_sampling(0)
        aligner.clear_index()
    print("test_seeding_past_2_31: %.2f s" % (time.perf_counter() - t_all))


def test_paf_positions_past_2_31(aligner, oracle, big_genome, tmp_path):
    """The loader on the same genome as a FASTA file, seeds below, across and past 2^31 and one at the genome's last bases: the
    alignments are the oracle's on the cut suffix, and the PAF writer's target length, start and end columns are the large
    positions (start + the text the alignment consumed)."""
    from scrooge_amd import io as sio
    from tests import anchored_inputs as ai
    t0 = time.perf_counter()
    g, where, reads = big_genome["g"], big_genome["where"], big_genome["reads"]
    assert GENOME_LEN % 64 == 0
    fa, fq, seeds = (str(tmp_path / x) for x in ("genome.fa", "reads.fq", "seeds.paf"))
    lines = np.empty((GENOME_LEN // 64, 65), dtype=np.uint8)
    lines[:, :64] = g.reshape(-1, 64)
    lines[:, 64] = ord("\n")
    with open(fa, "wb") as f:
        f.write(b">chrBig one letter with planted stretches\n")
        lines.tofile(f)
    del lines
    ks = [0, 1, 4, 7]
    with open(fq, "w") as f, open(seeds, "w") as s:
        for k in ks:
            L = len(reads[k])
            stored = ai.revcomp(reads[k]) if k % 2 else reads[k]
            f.write("@read%d\n%s\n+\n%s\n" % (k, stored.decode(), "I" * L))
            s.write("read%d\t%d\t0\t%d\t%s\tchrBig\t%d\t%d\t%d\t%d\t%d\t60\n" % (k, L, L, "-" if k % 2 else "+", GENOME_LEN, where[k], where[k] + L, L, L))
    t1 = time.perf_counter()
    try:
        job = sio.Job(fa, fq, seeds, reverse_strand=1)
    finally:
        os.unlink(fa)                                                   # (2 GiB: loaded, not left behind in the temp directory)
    try:
        assert job.genome_len == GENOME_LEN and job.n_pairs == len(ks) and job.n_reads == len(ks)
        ks = [int(job.lib.scrg_job_read_name(job.h, r).decode()[4:]) for r in range(job.n_reads)]       # the loader's order of the reads
        out = str(tmp_path / "out.paf")
        alns = job.align(aligner, out_path=out)
    finally:
        job.close()
    eds, cigars, _, _ = oracle.align([big_genome["cut"][where[k]:] for k in ks], [reads[k] for k in ks])
    assert [a.edit_distance for a in alns] == eds and [a.cigar for a in alns] == cigars
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert len(rows) == len(ks)
    for row, k, c in zip(rows, ks, cigars):
        assert row[0] == "read%d" % k and row[4] == ("-" if k % 2 else "+") and row[5] == "chrBig"
        assert (int(row[6]), int(row[7]), int(row[8])) == (GENOME_LEN, where[k], where[k] + ai.text_used(c)), row[:12]
    assert sum(int(r[7]) > T31 for r in rows) >= 2 and any(int(r[7]) < T31 < int(r[8]) for r in rows)
    print("test_paf_positions_past_2_31: %.2f s to write the files, %.2f s in all" % (t1 - t0, time.perf_counter() - t0))
