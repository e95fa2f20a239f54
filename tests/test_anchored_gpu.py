"""Anchored alignment on the GPU: texts taken as the reverse complement of their stretch (SCRG_TEXT_REVCOMP, every
one-pair-per-lane kernel), candidates with a direction (scrg_align_mapping_directed) and both sides of an anchor joined
(scrg_align_mapping_anchored).  Expected values are always the oracle's on explicitly reverse-complemented Python strings,
never another path of the library."""
import ctypes as C
import re

import numpy as np
import pytest

from scrooge_amd import synth

pytestmark = pytest.mark.gpu

_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _revcomp(b):
    return b.translate(_RC)[::-1]


def _runs(cigar):
    return [(int(c), o) for c, o in re.findall(r"(\d+)([=XID])", cigar)]


def _text_used(cigar):
    return sum(c for c, o in _runs(cigar) if o != "I")


def _mutated(seq, rng, err=0.10):
    """seq with ONT-profile edits (synth.mutate)."""
    if not seq:
        return b""
    codes = np.searchsorted(synth.BASES, np.frombuffer(seq, dtype=np.uint8)).astype(np.uint8)
    return synth.BASES[synth.mutate(codes, err, synth.PROFILES["ont"][1], rng)].tobytes()


# ================================================================================================ device layer
N_PAIRS = 256
ROW_BASES = 768            # a text row: the stretch (at most 640 bases) somewhere in its first 736 bases, random bases around it
READ_MAX = 600
CASES = [(64, 33, "split"), (64, 33, "one"), (16, 0, "one"), (64, 2, "one"), (128, 65, "one"), (192, 97, "one"), (256, 1, "one"), (64, 0, "one")]
_device_inputs = {}


def device_inputs(oracle, W, O):
    """256 pairs for the window setting, built and handed to the oracle once.  Pair k: read flag k & 1, text flag NOT k >> 1 & 1 —
    the four combinations side by side in every wavefront, and pairs 0 and 1 are the flagged ones with either read flag —; its
    stretch lies at base j0 of row trow[k] = k (every residue mod 32), inside random bases.  Pairs 0 to 3 have a stretch shorter
    than a window at base 0 of their row, and pair 1 takes its text from row 0 like pair 0: the two flagged pairs' stretches
    start at word 0 of the sequence array in both layouts, where a load that reached below its stretch would leave the array.  The text the pair is aligned against is the stretch, or its reverse complement where the text
    flag is set; the read as aligned is a mutated prefix of that text; what is stored is the stretch and — where the read flag is
    set — the reverse complement of the read as aligned."""
    if (W, O) in _device_inputs:
        return _device_inputs[(W, O)]
    rng = np.random.Generator(np.random.PCG64(9000 + 7 * W + O))
    rows = synth.BASES[rng.integers(0, 4, (N_PAIRS, ROW_BASES), dtype=np.uint8)]
    text_len = rng.integers(100, 640, N_PAIRS)
    read_len = np.where(rng.random(N_PAIRS) < 0.3, rng.integers(4, 60, N_PAIRS), rng.integers(60, READ_MAX + 1, N_PAIRS))      # (very different lengths: lanes retire at different times)
    read_len = np.minimum(read_len, (text_len * 0.95).astype(np.int64))
    j0 = (np.arange(N_PAIRS) * 7 + 3) % 96
    # the edges: a stretch at offset 0 shorter than a window (all four combinations, the flagged ones at word 0 of the array);
    # texts of 0, 1, W - 1, W, W + 1 bases (all four); reads that are empty, of one base, shorter than a window
    trow = np.arange(N_PAIRS)
    trow[1] = 0
    for c in range(4):
        j0[c], text_len[c], read_len[c] = 0, W - 3, (40, 9, 40, 9)[c]
    for i, tl in enumerate((0, 1, W - 1, W, W + 1)):
        for c in range(4):
            k = 8 + 4 * i + c
            text_len[k], read_len[k] = tl, (50, 7, 130)[c % 3]
    for c in range(4):
        read_len[40 + c], read_len[44 + c], read_len[48 + c] = 0, 1, max(1, W - 5)
    tflag, rflag = ((np.arange(N_PAIRS) >> 1) & 1) ^ 1, np.arange(N_PAIRS) & 1
    assert tflag[0] and tflag[1] and rflag[0] != rflag[1] and trow[0] == trow[1] == 0 and j0[0] == j0[1] == 0 and text_len[0] < W
    texts, want_reads, stored = [], [], []
    for k in range(N_PAIRS):
        stretch = rows[trow[k], j0[k]: j0[k] + text_len[k]].tobytes()
        text = _revcomp(stretch) if tflag[k] else stretch
        src = text[: int(read_len[k] * 1.1) + 8]
        r = _mutated(src, rng)[: read_len[k]]
        r = r + synth.random_seq(int(read_len[k]) - len(r), rng)           # (a text too short for the read: random bases on)
        texts.append(text), want_reads.append(r), stored.append(_revcomp(r) if rflag[k] else r)
    eds, cigars, _, _ = oracle.align(texts, want_reads, W=W, O=O, threads=8)
    inp = dict(rows=rows, trow=trow, j0=j0, text_len=text_len, read_len=np.array([len(x) for x in stored]), tflag=tflag, rflag=rflag, stored=stored,
               want_reads=want_reads, eds=eds, cigars=cigars, text_end=[_text_used(c) for c in cigars])
    _device_inputs[(W, O)] = inp
    return inp


def pack_device(aligner, torch, inp, layout, flags=True):
    """-> (seq, desc [n, 6] without slices, stride keywords): the 256 pairs on the device in one of the two layouts."""
    import scrooge_amd
    dev = torch.device("cuda", 0)
    n, tw, rw, G = N_PAIRS, ROW_BASES // 32, (READ_MAX + 31) // 32, scrooge_amd.api.GROUP
    r_rows = np.zeros((n, rw * 32), dtype=np.uint8)
    for k in range(n):
        r_rows[k, :len(inp["stored"][k])] = np.frombuffer(inp["stored"][k], dtype=np.uint8)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    trow = torch.from_numpy(inp["trow"].astype(np.int64)).to(dev)
    j0 = torch.from_numpy(inp["j0"].astype(np.int64)).to(dev)
    if layout == "linear":
        seq = torch.zeros(n * (tw + rw) + scrooge_amd.api.SEQ_PAD_WORDS, dtype=torch.int64, device=dev)
        aligner.pack_planar(torch.from_numpy(inp["rows"]).to(dev).view(-1), seq[: n * tw], bad)
        aligner.pack_planar(torch.from_numpy(r_rows).to(dev).view(-1), seq[n * tw:], bad)
        t_off, r_off, lay = trow * tw * 32 + j0, (n * tw + idx * rw) * 32, {}
    else:
        seq = torch.zeros(n * (tw + rw) + scrooge_amd.api.SEQ_PAD_WORDS_GROUPS, dtype=torch.int64, device=dev)
        aligner.pack_planar_groups(torch.from_numpy(inp["rows"]).to(dev).view(-1), n, tw, seq[: n * tw], bad)
        aligner.pack_planar_groups(torch.from_numpy(r_rows).to(dev).view(-1), n, rw, seq[n * tw:], bad)
        t_off = ((trow // G) * tw * G + trow % G + (j0 // 32) * G) * 32 + j0 % 32
        r_off = (n * tw + (idx // G) * rw * G + idx % G) * 32
        lay = dict(text_stride_words=G, read_stride_words=G)
    assert int(bad.item()) == 0 and int(t_off[0]) == int(t_off[1]) == 0
    tl = torch.from_numpy(inp["text_len"].astype(np.int64)).to(dev)
    ql = torch.from_numpy(inp["read_len"].astype(np.int64)).to(dev)
    if flags:
        t_off = t_off | (torch.from_numpy(inp["tflag"].astype(np.int64)).to(dev) << 63)
        r_off = r_off | (torch.from_numpy(inp["rflag"].astype(np.int64)).to(dev) << 63)
    return seq, torch.stack([t_off, tl, r_off, ql], dim=1), lay


def with_slices(torch, desc4, cap):
    n = desc4.shape[0]
    idx = torch.arange(n, dtype=torch.int64, device=desc4.device)
    return torch.cat([desc4, (idx * cap)[:, None], torch.full_like(idx, cap)[:, None]], dim=1).contiguous()


def run_mode(aligner, torch, seq, desc, cap, mode, **kw):
    """-> dict of host arrays: ed, status, and runs + n_runs / streams + len / text_end."""
    n, dev = desc.shape[0], seq.device
    ed = torch.empty(n, dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    out = {}
    if mode == "distance":
        aligner.align_device_distance(n, seq, desc, ed, cnt, st, **kw)
    else:
        buf = torch.zeros(n * cap * 2, dtype=torch.uint8, device=dev)
        (aligner.align_device if mode == "runs" else aligner.align_device_edits)(n, seq, desc, buf, ed, cnt, st, **kw)
        out["buf"] = None
    torch.cuda.synchronize()
    if mode != "distance":
        out["buf"] = buf.cpu().numpy()
    out.update(ed=ed.cpu().numpy(), status=st.cpu().numpy(), count=cnt.cpu().numpy())
    return out


def cigars_of(res, cap, mode, read_lens, W, O):
    import scrooge_amd
    h, cnt, out = res["buf"], res["count"], []
    for k in range(len(cnt)):
        if mode == "runs":
            seg = h[2 * k * cap: 2 * (k * cap + int(cnt[k]))]
            out.append("".join("%d%s" % (seg[2 * j], chr(seg[2 * j + 1])) for j in range(int(cnt[k]))))
        else:
            out.append(scrooge_amd.api.edit_stream_to_cigar(h[2 * k * cap: 2 * k * cap + int(cnt[k])].tobytes(), int(read_lens[k]), W=W, O=O))
    return out


@pytest.fixture
def strands(aligner):
    """The session's handle with text strands switched on, on the null stream; both restored afterwards."""
    aligner.set_stream(0)
    aligner.set_text_strands(True)
    try:
        yield aligner
    finally:
        aligner.set_text_strands(False)
        aligner.use_own_stream()


@pytest.mark.parametrize("W,O,form", CASES)
def test_reversed_texts_on_the_device(strands, oracle, W, O, form):
    """Every one-pair-per-lane kernel, both layouts, all three output modes: read flag x text flag interleaved pair by pair,
    stretches that end on every residue mod 32, a stretch at the very beginning of its row that is shorter than a window, texts
    of 0, 1, W - 1, W, W + 1 bases, reads that are empty, of one base, shorter than a window.  Edit distance, runs (decoded
    streams) and text end are the oracle's for every pair."""
    import torch
    aligner = strands
    inp = device_inputs(oracle, W, O)
    cap = (2 * READ_MAX + 16 + 15) // 16 * 16
    kw = dict(W=W, O=O, stranded=1)
    if form == "one":
        kw["waves_per_cu"] = 16 if W <= 64 and W - O <= 31 else 8        # (a caller-set geometry keeps the default kernel in one wavefront per window)
    for layout in ("linear", "groups"):
        seq, desc4, lay = pack_device(aligner, torch, inp, layout)
        desc = with_slices(torch, desc4, cap)
        for mode in (("runs",) if form == "split" else ("runs", "edits", "distance")):
            res = run_mode(aligner, torch, seq, desc, cap, mode, **kw, **lay)
            where = (layout, mode)
            bad = [k for k in range(N_PAIRS) if int(res["ed"][k]) != inp["eds"][k]]
            assert not bad, (where, bad[:8], [(int(inp["tflag"][k]), int(inp["rflag"][k])) for k in bad[:8]])
            assert not res["status"].any(), where
            if mode == "distance":
                assert res["count"].tolist() == inp["text_end"], where
            else:
                got = cigars_of(res, cap, mode, inp["read_len"], W, O)
                bad = [k for k in range(N_PAIRS) if got[k] != inp["cigars"][k]]
                assert not bad, (where, bad[:8], [(int(inp["tflag"][k]), int(inp["rflag"][k])) for k in bad[:8]])


@pytest.mark.parametrize("W,O", [(64, 33), (128, 65), (192, 97), (256, 1)])
def test_lanes_take_reversed_and_forward_texts_in_turn(strands, oracle, W, O):
    """One case per kernel family with three times as many pairs as the launch has lanes and 37 more (one wavefront per CU;
    descriptors that point at the 256 packed pairs, whose reads have 0 to 600 bases, in a seeded order, each with a slice of its
    own), so at least two thirds of the descriptors go to a lane that has retired a pair while its neighbours are in the middle
    of theirs: a lane's next pair from the queue has another direction than its last about every second time."""
    import torch
    aligner = strands
    inp = device_inputs(oracle, W, O)
    seq, desc4, lay = pack_device(aligner, torch, inp, "groups")
    p = aligner._params(dict(W=W, O=O, stranded=1, waves_per_cu=1, **lay))
    n_waves, per_wave = C.c_int32(), C.c_int32()
    aligner._check(aligner.lib.scrg_query_launch(aligner.h, C.byref(p), C.byref(n_waves), C.byref(per_wave), None, None))
    slots = n_waves.value * per_wave.value               # (the lanes of this launch: all are taken in the first round of claims)
    n = 3 * slots + 37
    assert slots >= 64 and per_wave.value == 64
    rng = np.random.Generator(np.random.PCG64(W + O))
    perm = np.concatenate([rng.permutation(N_PAIRS) for _ in range(n // N_PAIRS + 1)])[:n]
    cap = (2 * READ_MAX + 16 + 15) // 16 * 16
    desc = with_slices(torch, desc4[torch.from_numpy(perm).to(seq.device)], cap)
    res = run_mode(aligner, torch, seq, desc, cap, "runs", W=W, O=O, stranded=1, waves_per_cu=1, **lay)
    assert res["ed"].tolist() == [inp["eds"][p] for p in perm]
    assert not res["status"].any()
    base = {}
    for k in range(n):
        p = int(perm[k])
        seg = res["buf"][2 * k * cap: 2 * (k * cap + int(res["count"][k]))].tobytes()
        if p not in base:
            base[p] = b"".join(bytes([c, ord(o)]) for c, o in _runs(inp["cigars"][p]))
        assert seg == base[p], (k, p)


def test_the_setting_changes_nothing_for_unflagged_pairs(aligner, oracle):
    """With the setting off a batch gives byte-identical results before and after it was switched on and off again on the same
    handle; with it on and no pair flagged the results are those with it off.  (And the GenASM-row mappings refuse it.)"""
    import torch
    import scrooge_amd
    inp = device_inputs(oracle, 64, 33)
    cap = (2 * READ_MAX + 16 + 15) // 16 * 16
    aligner.set_stream(0)
    try:
        assert aligner.text_strands() is False
        seq, desc4, lay = pack_device(aligner, torch, inp, "groups", flags=False)
        desc = with_slices(torch, desc4, cap)
        for mode in ("runs", "edits", "distance"):
            before = run_mode(aligner, torch, seq, desc, cap, mode, **lay)
            aligner.set_text_strands(True)
            assert aligner.text_strands() is True
            on = run_mode(aligner, torch, seq, desc, cap, mode, **lay)
            aligner.set_text_strands(False)
            after = run_mode(aligner, torch, seq, desc, cap, mode, **lay)
            for key in ("ed", "status", "count"):
                assert np.array_equal(before[key], after[key]) and np.array_equal(before[key], on[key]), (mode, key)
            if mode != "distance":
                # (a pair's output: the first `count` runs / bytes of its slice; what follows them in the slice's last dword
                # is whatever the lane's staging ring held)
                unit = 2 if mode == "runs" else 1
                def valid(r):
                    return b"".join(r["buf"][2 * k * cap: 2 * k * cap + unit * int(r["count"][k])].tobytes() for k in range(N_PAIRS))
                assert valid(before) == valid(after) == valid(on), mode
        aligner.set_text_strands(True)
        with pytest.raises(scrooge_amd.ScroogeError):
            run_mode(aligner, torch, seq, desc, cap, "runs", lanes_per_pair=8)
        with pytest.raises(scrooge_amd.ScroogeError) as e:         # the host calls refuse the combination too
            aligner.align_pairs([b"ACGT"], [b"ACGT"], lanes_per_pair=8)
        assert e.value.status == scrooge_amd.api.SCRG_ERR_INVALID_ARG
        assert aligner.align_pairs([b"ACGT"], [b"ACGT"])[0].edit_distance == 0
    finally:
        aligner.set_text_strands(False)
        aligner.use_own_stream()


# ================================================================================================ host layer
GENOME_LEN = 20_000
_host = {}


def host_inputs(oracle):
    """A 20 kb genome, 200 reads with 1 to 3 candidates of mixed strand and direction, and the oracle's alignment of every
    candidate on explicit strings: a leftward candidate is the reverse complement of the read as aligned against the reverse
    complement of the genome up to its position."""
    if _host:
        return _host
    rng = np.random.Generator(np.random.PCG64(77))
    genome = synth.random_seq(GENOME_LEN, rng)
    reads, cands, rev, left = [], [], [], []
    o_text, o_read = [], []
    special = [0, 1, GENOME_LEN, 37]                      # (37: within one window of the genome's beginning)
    for r in range(200):
        L = int(rng.integers(1, 500)) if r % 10 else (0 if r == 0 else 1)
        g0 = int(rng.integers(0, GENOME_LEN - 600))
        as_aligned = _mutated(genome[g0: g0 + L + 50], rng)[:L]          # the read as its TRUE candidate aligns it, left to right on the genome
        L = len(as_aligned)
        c_pos, c_rev, c_left = [], [], []
        for c in range(1 + r % 3):
            lw, rv = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            if c == 0:
                pos = g0 + int(_text_used(oracle.align([genome[g0:]], [as_aligned])[1][0])) if lw else g0
            else:
                pos = special[(r + c) % 4] if (r + c) % 3 == 0 else int(rng.integers(0, GENOME_LEN + 1))
            c_pos.append(pos), c_rev.append(rv), c_left.append(lw)
        # the read as stored: such that its FIRST candidate, with its strand flag, names `as_aligned`
        stored = _revcomp(as_aligned) if c_rev[0] else as_aligned
        for pos, rv, lw in zip(c_pos, c_rev, c_left):
            named = _revcomp(stored) if rv else stored                 # R'
            o_text.append(_revcomp(genome[:pos]) if lw else genome[pos:])
            o_read.append(_revcomp(named) if lw else named)
        reads.append(stored), cands.append(c_pos), rev.append(c_rev), left.append(c_left)
    eds, cigars, _, _ = oracle.align(o_text, o_read, threads=8)
    _host.update(genome=genome, reads=reads, cands=cands, rev=rev, left=left, eds=eds, cigars=cigars, text_end=[_text_used(c) for c in cigars],
                 read_len=[len(x) for x in o_read], offs=np.cumsum([0] + [len(c) for c in cands]))
    return _host


def _cigars_from_arrays(out, outputs):
    n = len(out["edit_distance"])
    if outputs == 2:
        ro, runs = out["run_offset"], out["runs"]
        return ["".join("%d%s" % (c, chr(o)) for c, o in runs[int(ro[k]): int(ro[k + 1])]) for k in range(n)]
    co, text = out["cigar_offset"], out["cigar_text"]
    return [text[int(co[k]): int(co[k + 1]) - 1].decode() for k in range(n)]


@pytest.mark.parametrize("limit", [None, (25, 120)])
@pytest.mark.parametrize("outputs", [0, 2, 16, 4])
def test_directed_candidates(aligner, oracle, outputs, limit):
    """scrg_align_mapping_directed against the oracle per candidate: runs / text / distance-only / best-candidate output, with
    and without an edit limit (a pair is over the limit exactly when its full distance exceeds min(max_edits, per_mille x L))."""
    import scrooge_amd
    api = scrooge_amd.api
    h = host_inputs(oracle)
    aligner.set_genome(h["genome"])
    kw = dict(max_edits=limit[0], max_edit_per_mille=limit[1]) if limit else {}
    out = aligner.align_mapping_directed(h["reads"], h["cands"], reverse=h["rev"], leftward=h["left"], arrays=True, outputs=outputs, **kw)
    n = len(h["eds"])
    lim = [api.edit_limit_for(L, *limit) if limit else None for L in h["read_len"]]
    over = [lim[k] is not None and h["eds"][k] > lim[k] for k in range(n)]
    best = [True] * n
    if outputs & 4:
        for r in range(len(h["reads"])):
            a, b = int(h["offs"][r]), int(h["offs"][r + 1])
            elig = [k for k in range(a, b) if not over[k]]
            win = min(elig, key=lambda k: (h["eds"][k], k)) if elig else None
            for k in range(a, b):
                best[k] = k == win
    cig = None if outputs == 16 else _cigars_from_arrays(out, outputs)
    for k in range(n):
        what = (k, outputs, limit)
        if over[k]:
            assert out["status"][k] == api.SCRG_PAIR_OVER_EDIT_LIMIT and lim[k] < out["edit_distance"][k] <= h["eds"][k], what
        else:
            assert out["edit_distance"][k] == h["eds"][k], what
            assert out["status"][k] == (api.SCRG_OK if best[k] else api.SCRG_PAIR_NOT_BEST), what
        shown = best[k] and not over[k]
        if outputs == 16:
            assert out["text_end"][k] == (h["text_end"][k] if shown else 0), what
        else:
            assert cig[k] == (h["cigars"][k] if shown else ""), what


def test_directed_without_directions_is_the_resident_call(aligner, oracle):
    """cand_leftward NULL (and all zero): scrg_align_mapping_resident byte for byte, strands included."""
    api = __import__("scrooge_amd").api
    h = host_inputs(oracle)
    aligner.set_genome(h["genome"])
    reads, offs, (starts, rev) = aligner._flat_candidates(h["reads"], h["cands"], (("candidates", h["cands"]), ("reverse", h["rev"])))
    nr, n = len(reads), offs[-1]
    rp = (C.c_char_p * nr)(*reads)
    rl = (C.c_uint64 * nr)(*[len(r) for r in reads])
    co, cs, cr = (C.c_uint64 * (nr + 1))(*offs), (C.c_uint64 * n)(*starts), (C.c_uint8 * n)(*rev)
    res = C.POINTER(api.Result)()
    st = aligner.lib.scrg_align_mapping_resident(aligner.h, C.byref(aligner.params), nr, C.cast(rp, C.c_void_p), C.cast(rl, C.c_void_p),
                                                 C.cast(co, C.c_void_p), C.cast(cs, C.c_void_p), C.cast(cr, C.c_void_p), C.byref(res))
    assert st == 0
    want = aligner._collect_arrays(res, st)
    none = [[0] * len(c) for c in h["cands"]]
    for leftward in (None, none):
        got = aligner.align_mapping_directed(h["reads"], h["cands"], reverse=h["rev"], leftward=leftward, arrays=True)
        for key in want:
            assert np.array_equal(np.asarray(want[key]), np.asarray(got[key])) if not isinstance(want[key], bytes) else want[key] == got[key], key
    # lanes_per_pair != 1: fine without a leftward candidate, refused with one
    aligner.align_mapping_directed(h["reads"][:4], h["cands"][:4], leftward=none[:4], lanes_per_pair=8)
    with pytest.raises(api.ScroogeError):
        aligner.align_mapping_directed(h["reads"][:4], h["cands"][:4], leftward=[[1] * len(c) for c in h["cands"][:4]], lanes_per_pair=8)


_anch = {}


def anchored_inputs(oracle):
    """Reads that are a genome stretch with ONT-profile edits around 12 bases copied exactly: the anchor (genome position of the
    copy, its position in the read) is known to match.  Every third read is stored as its reverse complement; anchors at the
    read's first and last position and at the genome's first are among them.  Expected: two oracle calls per pair, composed."""
    if _anch:
        return _anch
    h = host_inputs(oracle)
    genome = h["genome"]
    rng = np.random.Generator(np.random.PCG64(78))
    reads, anchors, rev, named_reads = [], [], [], []
    for r in range(120):
        ga = int(rng.integers(300, GENOME_LEN - 400))
        la, lb = int(rng.integers(0, 280)), int(rng.integers(0, 300))
        left_part, right_part = _mutated(genome[ga - la: ga], rng), genome[ga: ga + 12] + _mutated(genome[ga + 12: ga + 12 + lb], rng)
        if r % 7 == 1:
            left_part = b""                                # ra = 0
        if r % 7 == 2:
            right_part = b""                               # ra = L
        if r % 7 == 3:
            ga, left_part = 0, left_part[:9]               # ga = 0: whatever lies left of the anchor is inserted
            right_part = genome[:12] + _mutated(genome[12: 12 + lb], rng)
        named = left_part + right_part                     # R'
        rv = 1 if r % 3 == 0 else 0
        reads.append(_revcomp(named) if rv else named), named_reads.append(named)
        anchors.append([(ga, len(left_part))]), rev.append([rv])
    o_text = [_revcomp(genome[:a[0][0]]) for a in anchors] + [genome[a[0][0]:] for a in anchors]
    o_read = [_revcomp(nm[:a[0][1]]) for nm, a in zip(named_reads, anchors)] + [nm[a[0][1]:] for nm, a in zip(named_reads, anchors)]
    eds, cigars, _, _ = oracle.align(o_text, o_read, threads=8)
    n = len(reads)
    joined, start, used = [], [], []
    for k in range(n):
        lr, rr = _runs(cigars[k]), _runs(cigars[n + k])
        joined.append("".join("%d%s" % x for x in lr[::-1] + rr))
        start.append(anchors[k][0][0] - _text_used(cigars[k]))
        used.append(_text_used(cigars[k]) + _text_used(cigars[n + k]))
    _anch.update(genome=genome, reads=reads, anchors=anchors, rev=rev, named=named_reads, ed=[eds[k] + eds[n + k] for k in range(n)],
                 cigars=joined, text_start=start, text_used=used)
    return _anch


@pytest.mark.parametrize("outputs", [0, 1, 2, 16])
def test_anchored_alignment(aligner, oracle, outputs):
    """Joined distance, runs, text and text_start are the composition of two oracle calls; every joined CIGAR is a valid
    alignment of R' against genome[text_start : text_start + consumed); distance-only mode agrees."""
    from scrooge_amd import io as sio
    a = anchored_inputs(oracle)
    aligner.set_genome(a["genome"])
    out = aligner.align_anchored(a["reads"], a["anchors"], reverse=a["rev"], arrays=True, outputs=outputs)
    n = len(a["reads"])
    assert out["edit_distance"].tolist() == a["ed"]
    assert out["text_start"].tolist() == a["text_start"]
    assert not out["status"].any()
    if outputs == 16:
        assert out["text_end"].tolist() == a["text_used"]
        assert not out["run_offset"].any() and not out["cigar_offset"].any()
        return
    if outputs != 1:
        assert _cigars_from_arrays(out, 2) == a["cigars"]
    else:
        assert not out["run_offset"].any()
    if outputs != 2:
        text = _cigars_from_arrays(out, 0)
        assert text == a["cigars"]
        for k in range(n):
            ts = a["text_start"][k]
            assert sio.validate_alignment(a["genome"][ts: ts + a["text_used"][k]], a["named"][k], text[k], a["ed"][k]) == 0, k
    else:
        assert not out["cigar_offset"].any()


def test_anchored_list_form_and_rejections(aligner, oracle):
    import scrooge_amd
    api = scrooge_amd.api
    a = anchored_inputs(oracle)
    aligner.set_genome(a["genome"])
    got, text_start = aligner.align_anchored(a["reads"][:10], a["anchors"][:10], reverse=a["rev"][:10])
    assert [x.cigar for x in got] == a["cigars"][:10] and [x.edit_distance for x in got] == a["ed"][:10] and text_start == a["text_start"][:10]
    few = (a["reads"][:3], a["anchors"][:3])
    for kw in (dict(best=True), dict(lanes_per_pair=8), dict(outputs=20)):
        with pytest.raises(api.ScroogeError) as e:
            aligner.align_anchored(*few, **kw)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG, kw
    aligner.set_edit_limit(max_edits=10)
    try:
        with pytest.raises(api.ScroogeError) as e:
            aligner.align_anchored(*few)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    finally:
        aligner.set_edit_limit()
    with pytest.raises(api.ScroogeError) as e:                     # a genome position past the genome: the library's check
        aligner.align_anchored([b"ACGT"], [[(GENOME_LEN + 1, 2)]])
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
