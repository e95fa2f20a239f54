"""Directed and anchored host calls that are cut into several chunks, in every kernel family (tests/anchored_inputs.py builds the
inputs, tests/test_anchored_inputs.py asserts on the CPU that they are cut the way these tests need).

The host layer packs the genome with text stride 1 at word 0 and a chunk's reads with stride 64; only these calls produce
that layout together with a reversed text, and only a call of several chunks has the two halves of an anchor — sorted apart by
their lengths — aligned on different slots and brought side by side again by the permutation back.  Expected values are the
oracle's on explicitly reverse-complemented Python strings, never another path of the library; every comparison is exact."""
import numpy as np
import pytest

from tests import anchored_inputs as ai

pytestmark = pytest.mark.gpu

# window settings -> the kernel that aligns them with one pair per lane (genasm_kernels.h: align_form).  The host layer hands
# every chunk's launch the RESOLVED parameters, whose waves_per_cu is never 0, and a launch with a set geometry keeps the default
# kernel in one wavefront per window (align_device_impl): no host call reaches the default kernel's split form, so 64/33 and
# 16/0 run its one-wavefront form here.  test_split_form_with_the_host_layout runs the split form on the host layer's layout.
FAMILIES = [(64, 33), (16, 0),              # default, one wavefront per window
            (64, 2), (128, 65),             # wide
            (192, 97), (256, 129),          # parts
            (64, 0), (256, 1)]              # mw
LIMIT = (25, 120)


def check_directed(api, d, out, outputs, limit=None):
    """Every candidate's edit distance, status and CIGAR (outputs 0 / 2 / 4) or text_end (16 / 20) against the oracle's — the
    expectations of tests/test_anchored_gpu.py::test_directed_candidates: in best-candidate mode the winner is the first
    candidate with the fewest edits among those not over the limit, losers return their distance and SCRG_PAIR_NOT_BEST; a pair is
    over the limit exactly when its full distance exceeds it, and returns a partial distance in (limit, full]."""
    n, offs = len(d["eds"]), d["offs"]
    assert len(out["edit_distance"]) == n
    lim = [api.edit_limit_for(L, *limit) if limit else None for L in d["read_len"]]
    over = [lim[k] is not None and d["eds"][k] > lim[k] for k in range(n)]
    best = [True] * n
    if outputs & 4:
        for r in range(len(d["reads"])):
            a, b = int(offs[r]), int(offs[r + 1])
            elig = [k for k in range(a, b) if not over[k]]
            win = min(elig, key=lambda k: (d["eds"][k], k)) if elig else None
            for k in range(a, b):
                best[k] = k == win
    ed, status = out["edit_distance"].tolist(), out["status"].tolist()
    cig = None if outputs & 16 else ai.cigars_from_arrays(out, outputs)
    text_end = out["text_end"].tolist() if outputs & 16 else None
    for k in range(n):
        what = (k, d["W"], d["O"], outputs, limit)
        if over[k]:
            assert status[k] == api.SCRG_PAIR_OVER_EDIT_LIMIT and lim[k] < ed[k] <= d["eds"][k], what
        else:
            assert ed[k] == d["eds"][k], what
            assert status[k] == (api.SCRG_OK if best[k] else api.SCRG_PAIR_NOT_BEST), what
        shown = best[k] and not over[k]
        if outputs & 16:
            assert text_end[k] == (d["text_end"][k] if shown else 0), what
        else:
            assert cig[k] == (d["cigars"][k] if shown else ""), what
    return sum(over), n - sum(best)


def run_directed(aligner, d, outputs, limit=None, **kw):
    if limit:
        kw.update(max_edits=limit[0], max_edit_per_mille=limit[1])
    return aligner.align_mapping_directed(d["reads"], d["cands"], reverse=d["rev"], leftward=d["left"], arrays=True, outputs=outputs,
                                          W=d["W"], O=d["O"], **kw)


@pytest.mark.parametrize("W,O", FAMILIES)
def test_directed_candidates_in_every_kernel_family(aligner, oracle, W, O):
    """2 536 candidates of 1 024 reads in four chunks, every (strand, direction) combination in each: runs against the oracle's
    CIGARs, distance-only mode against the text they consume."""
    import scrooge_amd
    d = ai.directed_inputs(oracle, W, O)
    aligner.set_genome(d["genome"])
    for outputs in (2, 16):
        check_directed(scrooge_amd.api, d, run_directed(aligner, d, outputs), outputs)


def test_directed_candidates_with_a_caller_set_geometry(aligner, oracle):
    """waves_per_cu = 16 given by the caller: a launch with a caller-set geometry keeps the default kernel in one wavefront per
    window.  As the host layer stands it hands every chunk the resolved parameters — 16 for this window setting — whether the caller
    set one or not, so these are the launches of the 64/33 case above; the case holds the one-wavefront form in place should the
    host layer ever pass the caller's own value (0 = not set) on, which would send the case above to the split form."""
    import scrooge_amd
    d = ai.directed_inputs(oracle, 64, 33)
    aligner.set_genome(d["genome"])
    for outputs in (2, 16):
        check_directed(scrooge_amd.api, d, run_directed(aligner, d, outputs, waves_per_cu=16), outputs)


@pytest.mark.parametrize("form", ["split", "one"])
def test_split_form_with_the_host_layout(aligner, oracle, form):
    """The device layer on the layout the host layer builds — texts with word stride 1 from word 0 of the sequence array, reads
    behind them in groups with word stride 64 — with reversed texts and reverse-strand reads interleaved pair by pair: the
    default kernel's split form (no geometry given, 256 pairs: at most one wavefront per SIMD), which no host call reaches, and
    its one-wavefront form on the same arrays.  The pairs, their edge cases and the oracle's answers are those of
    tests/test_anchored_gpu.py (device_inputs)."""
    import torch
    import scrooge_amd
    from tests import test_anchored_gpu as tg
    G, n = scrooge_amd.api.GROUP, tg.N_PAIRS
    inp = tg.device_inputs(oracle, 64, 33)
    dev = torch.device("cuda", 0)
    tw, rw = tg.ROW_BASES // 32, (tg.READ_MAX + 31) // 32
    assert n % G == 0
    r_rows = np.zeros((n, rw * 32), dtype=np.uint8)
    for k in range(n):
        r_rows[k, :len(inp["stored"][k])] = np.frombuffer(inp["stored"][k], dtype=np.uint8)
    cap = (2 * tg.READ_MAX + 16 + 15) // 16 * 16
    aligner.set_stream(0)
    aligner.set_text_strands(True)
    try:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        seq = torch.zeros(n * (tw + rw) + scrooge_amd.api.SEQ_PAD_WORDS_GROUPS, dtype=torch.int64, device=dev)
        aligner.pack_planar(torch.from_numpy(inp["rows"]).to(dev).view(-1), seq[: n * tw], bad)
        aligner.pack_planar_groups(torch.from_numpy(r_rows).to(dev).view(-1), n, rw, seq[n * tw: n * (tw + rw)], bad)
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        t_off = torch.from_numpy((inp["trow"].astype(np.int64) * tw * 32 + inp["j0"]) | (inp["tflag"].astype(np.int64) << 63)).to(dev)
        r_off = ((n * tw + (idx // G) * rw * G + idx % G) * 32) | (torch.from_numpy(inp["rflag"].astype(np.int64)).to(dev) << 63)
        desc4 = torch.stack([t_off, torch.from_numpy(inp["text_len"].astype(np.int64)).to(dev), r_off,
                             torch.from_numpy(inp["read_len"].astype(np.int64)).to(dev)], dim=1)
        assert int(bad.item()) == 0 and (int(t_off[0]) & ((1 << 63) - 1)) == 0
        kw = dict(W=64, O=33, stranded=1, read_stride_words=G)
        if form == "one":
            kw["waves_per_cu"] = 16
        res = tg.run_mode(aligner, torch, seq, tg.with_slices(torch, desc4, cap), cap, "runs", **kw)
    finally:
        aligner.set_text_strands(False)
        aligner.use_own_stream()
    flags = [(int(inp["tflag"][k]), int(inp["rflag"][k])) for k in range(n)]
    bad = [k for k in range(n) if int(res["ed"][k]) != inp["eds"][k]]
    assert not bad, (bad[:8], [flags[k] for k in bad[:8]])
    assert not res["status"].any()
    got = tg.cigars_of(res, cap, "runs", inp["read_len"], 64, 33)
    bad = [k for k in range(n) if got[k] != inp["cigars"][k]]
    assert not bad, (bad[:8], [flags[k] for k in bad[:8]])


@pytest.mark.parametrize("limit", [None, LIMIT])
@pytest.mark.parametrize("outputs", [0, 4, 20])
@pytest.mark.parametrize("W,O", [(64, 33), (192, 97)])
def test_best_candidate_and_edit_limit_across_chunks(aligner, oracle, W, O, outputs, limit):
    """Best-candidate selection and the edit limit meet leftward candidates in a call of several chunks."""
    import scrooge_amd
    d = ai.directed_inputs(oracle, W, O)
    aligner.set_genome(d["genome"])
    n_over, n_lost = check_directed(scrooge_amd.api, d, run_directed(aligner, d, outputs, limit), outputs, limit)
    # (the inputs make both expectations bite: wrong locations are over the limit, reads with several candidates have losers)
    assert (n_over >= 500) == bool(limit) and (n_lost >= 500) == bool(outputs & 4)


@pytest.mark.parametrize("W,O", [(64, 33), (128, 65), (192, 97), (256, 1)])
def test_anchored_alignment_across_chunks(aligner, oracle, W, O):
    """1 415 anchors of 716 reads, up to three per read, true seeds and wrong locations: 2 830 halves in four chunks, the two halves
    of most anchors in different ones.  Joined distance, runs, text, text_start and (distance-only mode) text_end are the
    composition of two oracle calls; every joined CIGAR is a valid alignment of R' against genome[text_start : text_start + consumed)."""
    from scrooge_amd import io as sio
    a = ai.anchored_inputs(oracle, W, O)
    aligner.set_genome(a["genome"])
    n = len(a["ed"])
    for outputs in ((0, 16, 1, 2) if (W, O) == (64, 33) else (0, 16)):
        out = aligner.align_anchored(a["reads"], a["anchors"], reverse=a["rev"], arrays=True, outputs=outputs, W=W, O=O)
        what = (W, O, outputs)
        ed, ts = out["edit_distance"].tolist(), out["text_start"].tolist()
        bad = [q for q in range(n) if ed[q] != a["ed"][q] or ts[q] != a["text_start"][q]]
        assert len(ed) == n and not bad, (what, bad[:8], [a["kinds"][q] for q in bad[:8]])
        assert not out["status"].any(), what
        if outputs == 16:
            assert out["text_end"].tolist() == a["text_used"], what
            assert not out["run_offset"].any() and not out["cigar_offset"].any(), what
            continue
        if outputs != 1:
            got = ai.cigars_from_arrays(out, 2)
            bad = [q for q in range(n) if got[q] != a["cigars"][q]]
            assert not bad, (what, bad[:8], [a["kinds"][q] for q in bad[:8]])
        else:
            assert not out["run_offset"].any(), what
        if outputs != 2:
            text = ai.cigars_from_arrays(out, 0)
            assert text == a["cigars"], what
        else:
            assert not out["cigar_offset"].any(), what
        if outputs == 0:
            for q in range(n):
                s = a["text_start"][q]
                assert sio.validate_alignment(a["genome"][s: s + a["text_used"][q]], a["named"][q], text[q], a["ed"][q]) == 0, (what, q)


def test_nothing_of_a_directed_call_leaks_into_the_next(aligner, oracle):
    """A directed call with leftward candidates switches the text-strand setting on in the slots' own handles; the plain
    resident call after it on the same handle gives the oracle's results for the same reads with their rightward candidates
    (forward strand: the plain call has no strands), and the handle's own setting is still off."""
    import scrooge_amd
    api = scrooge_amd.api
    d = ai.directed_inputs(oracle, 64, 33)
    aligner.set_genome(d["genome"])
    assert aligner.text_strands() is False
    out = run_directed(aligner, d, 2)
    assert out["edit_distance"].tolist() == d["eds"]
    cands = [[p for p, lw in zip(c, l) if not lw] for c, l in zip(d["cands"], d["left"])]
    texts = [d["genome"][p:] for c in cands for p in c]
    reads = [r for r, c in zip(d["reads"], cands) for _ in c]
    assert len(texts) >= 1_000 and any(not c for c in cands)
    eds, cigars, _, _ = oracle.align(texts, reads, threads=8)
    got = aligner.align_mapping(None, d["reads"], cands, arrays=True, outputs=0)
    assert got["edit_distance"].tolist() == eds
    assert not got["status"].any()
    assert ai.cigars_from_arrays(got, 0) == cigars and ai.cigars_from_arrays(got, 2) == cigars
    assert aligner.text_strands() is False
