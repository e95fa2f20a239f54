"""The oracle and the kernels pinned to the REFERENCE across the whole W/O plane.

tests/golden/plane_wW_oO.json hold the answers of the unmodified reference (oracle/Makefile builds it at every setting of
plane_inputs.SETTINGS) on one adversarial input set per setting (tests/plane_inputs.py): both sides of every border between the
one-pair-per-lane kernels, odd and multi-word W, W-O = 1, O = 0; lengths placed on the window arithmetic, reads that outlast
their texts, low-complexity pairs, long gaps.  The CPU tests hold the oracle (and, where it is built, the live reference) to
them; the GPU tests hold every kernel form to them directly, no oracle in between.  No pair is left out of any comparison.
W = 256 with O = 0 is refused (W-O <= 255: a run count is one byte)."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest

import scrooge_amd
from scrooge_amd import api
from tests import cigar_check
from tests import plane_inputs as pi
from tests.conftest import GOLDEN
from tests.test_edit_limit import device_run, revcomp

SETTINGS = pi.SETTINGS
IDS = ["%d-%d" % s for s in SETTINGS]
one_per_setting = pytest.mark.parametrize("W,O", SETTINGS, ids=IDS)


@functools.lru_cache(maxsize=None)
def load(W, O):
    """-> (texts, reads, groups, fixture) of a setting; fails if the generator no longer makes the inputs of the fixture."""
    with open(os.path.join(GOLDEN, pi.fixture_name(W, O))) as f:
        fx = json.load(f)
    t, q, g = pi.plane_inputs(W, O)
    assert (fx["W"], fx["O"], fx["n"]) == (W, O, len(t)), "generator drifted: W=%d O=%d has %d pairs, the fixture %d" % (W, O, len(t), fx["n"])
    assert pi.inputs_digest(t, q, g) == fx["inputs_sha256"], "generator drifted: the inputs of W=%d O=%d are not those of the fixture" % (W, O)
    assert [name for name, cnt in fx["groups"] for _ in range(cnt)] == g
    fx["cigar"] = pi.unpack_cigars(fx["cigar"])
    if "mapping" in fx:
        fx["mapping"]["cigar"] = pi.unpack_cigars(fx["mapping"]["cigar"])
    assert len(fx["ed"]) == len(fx["cigar"]) == len(t)
    return t, q, g, fx


def compare(W, O, form, groups, got_eds, got_cigars, want_eds, want_cigars):
    """Every pair; the message names setting, kernel form, group and pair index and prints got/want."""
    assert len(got_eds) == len(got_cigars) == len(want_eds) == len(want_cigars) == len(groups)
    bad = [k for k in range(len(want_eds)) if got_eds[k] != want_eds[k] or not pi.same_cigar(got_cigars[k], want_cigars[k])]
    if bad:
        k = bad[0]
        raise AssertionError("W=%d O=%d (class %s), %s: %d/%d pairs differ from the reference, groups %s; first: pair %d (%s): "
                             "got (%d, %s) want (%d, %s)" % (W, O, pi.kernel_class(W, O), form, len(bad), len(want_eds),
                                                             sorted({groups[j] for j in bad}), k, groups[k], got_eds[k],
                                                             got_cigars[k][:120], want_eds[k], want_cigars[k][:120]))


# ================================================================================================================ CPU
def test_settings_are_the_reference_builds():
    """SETTINGS = the VARIANTS of oracle/Makefile (+ the default build 64/33), 256/0 apart; every setting has its fixture
    and no fixture is left over; the fixtures stay within their size caps."""
    mk = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "oracle", "Makefile")).read()
    body = re.search(r"^VARIANTS := ((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ")
    variants = [tuple(int(x) for x in v.split("_")) for v in body.split()]
    assert variants == pi.VARIANTS and len(set(variants)) == len(variants) == 58
    assert pi.REFUSED in variants and pi.REFUSED not in SETTINGS and len(SETTINGS) == 58
    names = sorted(f for f in os.listdir(GOLDEN) if f.startswith("plane_"))
    assert names == sorted(pi.fixture_name(W, O) for W, O in SETTINGS)
    sizes = [os.path.getsize(os.path.join(GOLDEN, f)) for f in names]
    assert max(sizes) <= 323_178 and sum(sizes) < 1_000_000, (max(sizes), sum(sizes))
    assert all(s in SETTINGS for s in pi.MAPPING_SETTINGS)
    for c in pi.CLASSES:
        assert sum(pi.kernel_class(W, O) == c for W, O in pi.MAPPING_SETTINGS) == 1, c


def test_every_kernel_class_and_border_is_covered():
    """At least two settings in every class of kernel_class, and one on each side of every border between the kernels (or
    between a kernel's one-word and two-word builds), each side served by the class the border says.  If the dispatch moves,
    this names the border that lost its cover."""
    for c in pi.CLASSES:
        assert sum(pi.kernel_class(W, O) == c for W, O in SETTINGS) >= 2, "fewer than two settings in class %s" % c
    for name, (a, b) in pi.border_cover(SETTINGS).items():
        assert a and b, "border %s: no setting on one side (%s | %s)" % (name, a, b)
        for side, cls in zip((a, b), pi.BORDERS[name][2:]):
            assert {pi.kernel_class(*s) for s in side} == {cls}, "border %s: %s should all be served by %s" % (name, side, cls)
    # the statement itself, at the corners named by README and genasm_kernels.h
    for (W, O), c in {(64, 33): "default", (64, 32): "halves", (64, 0): "hbm", (65, 34): "hbm", (128, 65): "halves", (128, 64): "parts",
                      (129, 66): "parts", (129, 98): "parts", (128, 97): "hbm", (256, 129): "parts", (256, 128): "hbm", (255, 0): "hbm",
                      (65, 0): "parts", (2, 1): "default", (31, 0): "default", (32, 0): "halves", (256, 255): "parts"}.items():
        assert pi.kernel_class(W, O) == c, (W, O)


@one_per_setting
def test_inputs_hold_every_group(W, O):
    t, q, g, fx = load(W, O)                                  # (the digest: "generator drifted")
    assert 90 <= len(t) <= 250 and max(map(len, t + q)) <= 1100
    assert [name for k, name in enumerate(g) if k == 0 or g[k - 1] != name] == list(pi.GROUPS)
    T = W - O
    lat = [k for k in range(len(t)) if g[k] == "lattice"]
    for L in (T, W, W + T, 2 * W):                            # a read that ends exactly on a boundary, against itself
        assert any(len(q[k]) == L and t[k] == q[k] for k in lat), L
    assert all(fx["cigar"][k][:1] != "#" for k in range(len(t)) if g[k] in pi.FULL_TEXT_GROUPS)


@one_per_setting
def test_oracle_equals_reference_fixture(oracle, W, O):
    t, q, g, fx = load(W, O)
    eds, cigars, _, _ = oracle.align(t, q, W=W, O=O, threads=8)
    compare(W, O, "oracle", g, eds, cigars, fx["ed"], fx["cigar"])
    if "mapping" in fx:
        genome, reads, cands = pi.mapping_inputs(W, O)
        eds, cigars, _, _ = oracle.align([genome[c[0]:] for c in cands], reads, W=W, O=O, threads=8)
        compare(W, O, "oracle, mapping-shaped", g, eds, cigars, fx["mapping"]["ed"], fx["mapping"]["cigar"])


@one_per_setting
def test_live_reference_equals_fixture(W, O):
    """Where oracle/_ref holds the reference build of this setting: a stale fixture is caught.  (Elsewhere the fixture stands
    for it: there is nothing to compare, and the test passes on the fixture's own consistency.)"""
    from oracle.pyoracle import Reference
    t, q, g, fx = load(W, O)
    assert len(fx["ed"]) == len(t)
    if not Reference.available(W, O):
        return
    ref = Reference(W, O)
    eds, cigars, _ = ref.align(t, q, threads=8)
    compare(W, O, "live reference", g, eds, cigars, fx["ed"], fx["cigar"])
    if "mapping" in fx:
        eds, cigars, _ = ref.align_mapping(*pi.mapping_inputs(W, O), threads=8)
        compare(W, O, "live reference, mapping-shaped", g, eds, cigars, fx["mapping"]["ed"], fx["mapping"]["cigar"])


@one_per_setting
def test_coverage_conditions_and_validity(oracle, W, O):
    """The conditions the input set exists for, on the reference's answers (the oracle's CIGARs, once they are shown equal to
    the fixture's, text or digest): a full window of '=' and one of 'I' (runs of exactly min(W-O, 255)), a pair that consumes
    its whole text with read left over, an exact pair and one of nothing but edits — and every CIGAR passes the reference's
    own validateCigarString rules (tests/cigar_check.py)."""
    t, q, g, fx = load(W, O)
    eds, cigars, _, _ = oracle.align(t, q, W=W, O=O, threads=8)
    compare(W, O, "oracle", g, eds, cigars, fx["ed"], fx["cigar"])
    full = min(W - O, 255)
    runs = [pi.cigar_runs(c) for c in cigars]
    assert any((full, "=") in r for r in runs), "no run of exactly %d '='" % full
    assert any((full, "I") in r for r in runs), "no run of exactly %d 'I'" % full
    assert any(len(t[k]) > 0 and sum(n for n, o in r if o != "I") == len(t[k]) and sum(n for n, o in r if o != "D") == len(q[k])
               and r[-1][1] == "I" for k, r in enumerate(runs) if r), "no pair consumes its whole text with read left over"
    assert any(eds[k] == 0 and len(q[k]) > 0 for k in range(len(t))), "no exact pair"
    assert any(eds[k] == len(q[k]) > 0 for k in range(len(t))), "no pair with ed == len(read)"
    for k in range(len(t)):
        why = cigar_check.validate(t[k], q[k], cigars[k], fx["ed"][k])
        assert why is None, "W=%d O=%d pair %d (%s): %s: %s" % (W, O, k, g[k], why, cigars[k][:120])


@one_per_setting
def test_edit_stream_round_trip_on_fixture_cigars(W, O):
    from tests.test_edit_stream import round_trip
    t, q, g, fx = load(W, O)
    done = 0
    for k, c in enumerate(fx["cigar"]):
        if not c.startswith("#"):
            round_trip(c, len(q[k]), fx["ed"][k], W, O)
            done += 1
    assert done >= sum(x in pi.FULL_TEXT_GROUPS for x in g)


# ---------------------------------------------------------------------------------------------------------- 256/0 is refused
def test_256_0_is_refused_without_a_gpu(oracle):
    lib = api.load_library()
    p, out = api.Params(), api.Params()
    lib.scrg_params_default(C.byref(p))
    for (W, O), want in (((256, 0), api.SCRG_ERR_INVALID_ARG), ((255, 0), api.SCRG_OK), ((256, 1), api.SCRG_OK)):
        p.W, p.O = W, O
        assert lib.scrg_params_resolve(C.byref(p), C.byref(out)) == want, (W, O)
    # the stream helpers (scrg_edit_stream_to_runs, its lane form, scrg_runs_to_edit_stream)
    for lane_form in (False, True):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            api.edit_stream_to_cigar(b"\x04", 4, W=256, O=0, lane_form=lane_form)
        assert e.value.status == api.SCRG_ERR_INVALID_ARG
    with pytest.raises(scrooge_amd.ScroogeError) as e:
        api.cigar_to_edit_stream("4=", W=256, O=0)
    assert e.value.status == api.SCRG_ERR_INVALID_ARG
    assert api.edit_stream_to_cigar(api.cigar_to_edit_stream("4=", W=256, O=1), 4, W=256, O=1) == "4="
    with pytest.raises(ValueError):
        oracle.align([b"ACGT"], [b"ACGT"], W=256, O=0)
    with pytest.raises(RuntimeError):
        oracle.align_rows(np.frombuffer(b"ACGTACGT", dtype=np.uint8).reshape(1, 8), 0, 4, 4, 4, W=256, O=0)
    assert oracle.align([b"ACGT"], [b"ACGT"], W=256, O=1)[1] == ["4="]


def test_why_256_0_is_refused():
    """Live reference only.  At W = 256, O = 0 a window that is one run is a run of 256: the reference's run counter is a
    uint8_t that is flushed only if it is > 0 (src/genasm_cpu.cpp:305, 388-401), so the run is dropped and the CIGAR of a
    300-base read against itself does not consume the read — it fails the reference's own validateCigarString.  There is no
    valid answer to be bit-identical to."""
    from oracle.pyoracle import Reference
    if not Reference.available(*pi.REFUSED):
        pytest.skip("oracle/_ref not built")
    base = scrooge_amd.synth.random_seq(300, np.random.Generator(np.random.PCG64(256)))
    eds, cigars, _ = Reference(*pi.REFUSED).align([base], [base])
    used = sum(n for n, op in pi.cigar_runs(cigars[0]) if op != "D")
    assert eds == [0] and used == 300 - 256 and cigars[0] == "44="
    assert cigar_check.validate(base, base, cigars[0], 0) == "read not consumed exactly (44 of 300)"
    eds, cigars, _ = Reference(255, 0).align([base], [base])            # one short of it: the count byte at its maximum
    assert (eds, cigars) == ([0], ["255=45="])


# ================================================================================================================ GPU
def _forced(al, W, O, switch, t, q, **kw):
    """align_pairs through the test build with reserved[0] = switch (conftest.aligner_select)."""
    p = al.make_params(W=W, O=O, **kw)
    p.reserved[0] = switch
    keep = al.params
    al.params = p
    try:
        return al.align_pairs(t, q)
    finally:
        al.params = keep


def _host(alns):
    return [a.edit_distance for a in alns], [a.cigar for a in alns]


@pytest.mark.gpu
@one_per_setting
def test_pairs_through_the_shipped_library(aligner, W, O):
    """One pair per lane, whatever kernel the dispatch picks, in caller order and sorted by length."""
    t, q, g, fx = load(W, O)
    for sort in (0, 1):
        compare(W, O, "align_pairs sort_by_length=%d" % sort, g, *_host(aligner.align_pairs(t, q, W=W, O=O, sort_by_length=sort)), fx["ed"], fx["cigar"])


ALTERNATES = {"default": ((512, "two wavefronts per window"), (1024, "one wavefront")), "halves": ((256, "table in HBM"),),
              "parts": ((256, "table in HBM"),), "hbm": ()}


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [s for s in SETTINGS if ALTERNATES[pi.kernel_class(*s)]],
                         ids=["%d-%d" % s for s in SETTINGS if ALTERNATES[pi.kernel_class(*s)]])
def test_forced_alternate_kernels(aligner_select, W, O):
    """The other forms of the same table, forced through the test build: the split and the one-wavefront form of the default
    kernel; the kernel with the table in HBM where the two-halves or the parts kernel is the default."""
    t, q, g, fx = load(W, O)
    for switch, name in ALTERNATES[pi.kernel_class(W, O)]:
        compare(W, O, "reserved[0]=%d (%s)" % (switch, name), g, *_host(_forced(aligner_select, W, O, switch, t, q)), fx["ed"], fx["cigar"])


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", [s for s in SETTINGS if s[1] >= 1], ids=["%d-%d" % s for s in SETTINGS if s[1] >= 1])
def test_genasm_row_mappings(aligner, W, O):
    """The GenASM-row kernels (they refuse O = 0): 8 and 64 lanes per pair for W <= 64, 32 and 64 beyond; once with few rows
    in LDS (the spill path)."""
    t, q, g, fx = load(W, O)
    lanes = (8, 64) if W <= 64 else (32, 64)
    for lp, rows in ((lanes[0], 0), (lanes[1], 0), (lanes[0], 3 if W <= 64 else 4)):
        alns = aligner.align_pairs(t, q, W=W, O=O, lanes_per_pair=lp, lds_rows=rows)
        compare(W, O, "lanes_per_pair=%d lds_rows=%d" % (lp, rows), g, *_host(alns), fx["ed"], fx["cigar"])


def _runs_text(b):
    return "".join("%d%s" % (b[2 * j], chr(b[2 * j + 1])) for j in range(len(b) // 2))


def gpu_decode(al, streams, read_lens, W, O):
    """Edit streams -> CIGARs through scrg_decode_edit_stream (count pass, then the runs)."""
    import torch
    dev = torch.device("cuda", al.device)
    n = len(streams)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    r4 = (lens + 3) & -4
    off = np.cumsum(r4) - r4
    buf = np.zeros(int(r4.sum()) + 8, dtype=np.uint8)
    for k, s in enumerate(streams):
        buf[off[k]: off[k] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    stream, s_off = torch.from_numpy(buf).to(dev), torch.from_numpy(off).to(dev)
    s_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    rl = torch.tensor(read_lens, dtype=torch.int64, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    nbad = torch.zeros(1, dtype=torch.int32, device=dev)
    al.decode_edit_stream(n, stream, s_off, s_len, rl, 1, None, None, cnt, nbad, W=W, O=O)
    torch.cuda.synchronize()
    assert int(nbad.item()) == 0, "the GPU decoder rejects %d streams" % int(nbad.item())
    c64 = cnt.to(torch.int64)
    d_off = torch.cumsum(c64, 0) - c64
    dense = torch.zeros(int(c64.sum().item()) * 2 + 8, dtype=torch.uint8, device=dev)
    al.decode_edit_stream(n, stream, s_off, s_len, rl, 1, d_off, dense, cnt, nbad, W=W, O=O)
    torch.cuda.synchronize()
    assert int(nbad.item()) == 0
    d, o, c = dense.cpu().numpy(), d_off.cpu().tolist(), cnt.cpu().tolist()
    return [_runs_text(d[2 * o[k]: 2 * (o[k] + c[k])]) for k in range(n)]


@pytest.mark.gpu
@one_per_setting
def test_device_layer(aligner, W, O):
    """scrg_align_device / scrg_align_device_edits on packed sequences, both layouts: the runs; the edit streams decoded on
    the host and by the GPU decoder."""
    t, q, g, fx = load(W, O)
    rev = [False] * len(t)
    try:
        for layout in ("contiguous", "groups"):
            ed, st, ln, out, _ = device_run(aligner, t, q, rev, W, O, layout, False, False, None, None)
            assert set(st) == {0}, (W, O, layout, sorted(set(st)))
            compare(W, O, "align_device, %s" % layout, g, ed, [_runs_text(b) for b in out], fx["ed"], fx["cigar"])
            ed, st, ln, out, rc = device_run(aligner, t, q, rev, W, O, layout, True, False, None, None)
            assert set(st) == {0}, (W, O, layout, sorted(set(st)))
            host = [api.edit_stream_to_cigar(s, len(q[k]), W, O) for k, s in enumerate(out)]
            compare(W, O, "align_device_edits, %s, host decoder" % layout, g, ed, host, fx["ed"], fx["cigar"])
            assert rc == [len(pi.cigar_runs(c)) for c in host], "W=%d O=%d %s: run counts of the streams" % (W, O, layout)
            dec = gpu_decode(aligner, out, [len(x) for x in q], W, O)
            compare(W, O, "align_device_edits, %s, GPU decoder" % layout, g, ed, dec, fx["ed"], fx["cigar"])
    finally:
        aligner.use_own_stream()


@pytest.mark.gpu
@one_per_setting
def test_minus_strand(aligner, W, O):
    """Every read stored as its reverse complement with SCRG_READ_REVCOMP set: the fixture's answer for the original read."""
    t, q, g, fx = load(W, O)
    stored, rev = [revcomp(r) for r in q], [True] * len(q)
    try:
        for layout in ("contiguous", "groups"):
            ed, st, ln, out, _ = device_run(aligner, t, stored, rev, W, O, layout, False, True, None, None)
            assert set(st) == {0}, (W, O, layout, sorted(set(st)))
            compare(W, O, "minus strand, %s" % layout, g, ed, [_runs_text(b) for b in out], fx["ed"], fx["cigar"])
    finally:
        aligner.use_own_stream()


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", pi.MAPPING_SETTINGS, ids=["%d-%d" % s for s in pi.MAPPING_SETTINGS])
def test_mapping_shaped_call(aligner, W, O):
    """One setting per kernel class: every read against one genome (the concatenated texts), candidate = the start of its
    text, the last texts reaching the genome's end.  The reference's text is the genome's suffix: its align_mapping answers."""
    t, q, g, fx = load(W, O)
    genome, reads, cands = pi.mapping_inputs(W, O)
    alns = aligner.align_mapping(genome, reads, cands, W=W, O=O, best=False)
    compare(W, O, "align_mapping", g, *_host(alns), fx["mapping"]["ed"], fx["mapping"]["cigar"])


@pytest.mark.gpu
def test_256_0_is_refused_by_every_entry_point(aligner):
    import torch
    t, q = [b"ACGT" * 100], [b"ACGT" * 100]
    for call in (lambda: aligner.align_pairs(t, q, W=256, O=0),
                 lambda: aligner.align_mapping(t[0], q, [[0]], W=256, O=0),
                 lambda: device_run(aligner, t, q, [False], 256, 0, "contiguous", False, False, None, None),
                 lambda: device_run(aligner, t, q, [False], 256, 0, "groups", True, False, None, None)):
        try:
            with pytest.raises(scrooge_amd.ScroogeError) as e:
                call()
        finally:
            aligner.use_own_stream()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG and "a run count is one byte" in str(e.value), str(e.value)
    dev = torch.device("cuda", aligner.device)
    z64, z32 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    u8 = torch.zeros(64, dtype=torch.uint8, device=dev)
    for call in (lambda: aligner.decode_edit_stream(1, u8, z64, z32, z64, 1, None, None, z32, z32, W=256, O=0),
                 lambda: aligner.encode_edit_stream(1, z64, u8, z32, u8, z64, z32, z64, W=256, O=0)):
        with pytest.raises(scrooge_amd.ScroogeError) as e:
            call()
        assert e.value.status == api.SCRG_ERR_INVALID_ARG and "a run count is one byte" in str(e.value), str(e.value)
    # the settings next to it, count byte at its maximum, are served
    base = scrooge_amd.synth.random_seq(300, np.random.Generator(np.random.PCG64(256)))
    assert aligner.align_pairs([base], [base], W=255, O=0) == [("255=45=", 0)]
    assert aligner.align_pairs([base], [base], W=256, O=1) == [("255=45=", 0)]
