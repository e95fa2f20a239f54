"""The work queue's refill path, in every align kernel form.

Every align kernel is persistent: a lane (in the GenASM-row kernels: a slot of lanes_per_pair lanes) claims a pair from an atomic
queue, aligns it, retires it and claims the next while its neighbours are in the middle of theirs.  The hand-over resets a dozen
per-lane registers and reuses the lane's LDS ring, its spill area and its rows or checkpoints in HBM, none of which is cleared,
and the wavefront-uniform decisions then see a mix of old and new pairs.  A launch gets there only when it has more pairs than
slots (wavefronts x pairs per wavefront), and scrg_align_device launches as many slots as there are pairs up to 131 072 or
262 144 of them: the other tests' launches never hand a lane a second pair by construction.

Here every launch is cut down to one wavefront per CU (waves_per_cu = 1: 16 384 slots at one pair per lane on 256 CUs; the split
form of the default kernel cannot be cut down and gets 2 x its 131 072 slots) and given at least 3 x its slots + 37 descriptors
of very different lengths (tests/refill_inputs.py), so at least two thirds of all pairs are taken by a lane that has retired one.
Every descriptor's edit distance, status, length and every run or stream byte is compared with the oracle's result for its pair
(oracle.pyoracle.Oracle, pinned to the reference by tests/test_oracle.py and tests/test_plane.py); nothing is sampled or left out."""
import ctypes as C

import numpy as np
import pytest

from scrooge_amd import api
from tests import refill_inputs as ri
from tests.test_edit_limit import check_device_raw, device_run, pack_sequences, ragged_mismatch, window_model

SPLIT, HBM = 512, 256              # scrg_params.reserved[0] of the test build: the split form of the default kernel; the table in HBM

# (kernel, W, O, reserved[0], sequence layout, edit streams?, "" | "stranded" | "limit")
LANE_CASES = [
    # the default kernel, one wavefront per window (the shipped library: a caller-set waves_per_cu suppresses the split)
    ("default", 64, 33, 0, "contiguous", False, ""), ("default", 64, 33, 0, "groups", True, ""),
    ("default", 17, 9, 0, "groups", False, ""), ("default", 17, 9, 0, "contiguous", True, ""),
    ("default", 64, 33, 0, "groups", False, "stranded"), ("default", 64, 33, 0, "contiguous", True, "limit"),
    # its split form (a producer and a consumer wavefront per window)
    ("split", 64, 33, SPLIT, "groups", False, ""), ("split", 64, 33, SPLIT, "contiguous", False, "stranded"),
    ("split", 64, 33, SPLIT, "groups", False, "limit"),
    # the table in two halves: one word, two words
    ("halves", 64, 2, 0, "contiguous", False, ""), ("halves", 64, 2, 0, "groups", True, ""),
    ("halves", 128, 65, 0, "groups", False, ""), ("halves", 128, 65, 0, "contiguous", True, ""),
    ("halves", 64, 2, 0, "groups", False, "stranded"), ("halves", 128, 65, 0, "contiguous", True, "limit"),
    # the table in parts: NW = 3, NW = 4, and W > 128 with W - O <= 63
    ("parts", 192, 97, 0, "contiguous", False, ""), ("parts", 192, 97, 0, "groups", True, ""),
    ("parts", 256, 129, 0, "groups", False, ""), ("parts", 256, 129, 0, "contiguous", True, ""),
    ("parts", 256, 200, 0, "contiguous", False, ""), ("parts", 256, 200, 0, "groups", True, ""),
    ("parts", 192, 97, 0, "groups", False, "stranded"), ("parts", 256, 129, 0, "contiguous", True, "limit"),
    # the table in HBM (a new claim reuses the lane's rows there): <4, 4>, <1, 2>, <2, 3>, and forced where another kernel serves
    ("hbm", 256, 1, 0, "contiguous", False, ""), ("hbm", 256, 1, 0, "groups", True, ""),
    ("hbm", 64, 0, 0, "groups", False, ""), ("hbm", 64, 0, 0, "contiguous", True, ""),
    ("hbm", 128, 0, 0, "contiguous", False, ""), ("hbm", 128, 0, 0, "groups", True, ""),
    ("hbm", 128, 65, HBM, "groups", False, ""), ("hbm", 192, 97, HBM, "contiguous", False, ""),
    ("hbm", 256, 1, 0, "groups", False, "stranded"), ("hbm", 64, 0, 0, "contiguous", True, "limit"),
]
# GenASM rows: (W, O, lanes_per_pair, lds_rows (0: the default)); the spill area is per slot and is reused
ROW_CASES = [(64, 33, 8, 3), (64, 33, 64, 0), (128, 65, 32, 4), (128, 65, 64, 0), (256, 129, 32, 0), (256, 129, 64, 0)]


def case_id(c):
    return "-".join(str(x) for x in c if x not in ("", 0, False)).replace("True", "edits")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_base_set_and_batches_meet_their_conditions():
    """The conditions the GPU tests rely on, so that they cannot pass vacuously: what the base set holds, and where the stragglers
    sit in every batch size the GPU tests build (805 ... 262 181 descriptors)."""
    base = ri.base_set()
    rl, tl = base["read_len"], base["text_len"]
    assert len(rl) == ri.N_BASE
    med = float(np.median(rl))
    assert len(base["stragglers"]) >= ri.MIN_STRAGGLERS and (rl[base["stragglers"]] >= ri.STRAGGLER_FACTOR * med).all()
    assert int((rl == 0).sum()) >= ri.MIN_EMPTY_READS and int((tl == 0).sum()) >= ri.MIN_EMPTY_TEXTS
    assert int((rl > tl).sum()) >= ri.MIN_READ_OUTLASTS_TEXT
    assert {"ont", "unrelated", "low_complexity", "straggler"} == set(base["kind"])
    assert 0.2 < base["rev"].mean() < 0.4
    assert (ri.caps_for(rl) % 16 == 0).all() and (ri.caps_for(rl) >= 2 * rl + 16).all()
    print("base set: %d pairs, %.1f M read bases, median read %d, %d stragglers, %d empty reads, %d empty texts, %d reads longer than their text"
          % (len(rl), rl.sum() / 1e6, med, len(base["stragglers"]), (rl == 0).sum(), (tl == 0).sum(), (rl > tl).sum()))
    for n, slots in ((3 * 256 + 37, 256), (3 * 512 + 37, 512), (3 * 2048 + 37, 2048), (3 * 16384 + 37, 16384), (2 * 131072 + 37, 131072)):
        perm = ri.build_batch(base, n, seed=n, slots=slots)
        f = ri.batch_facts(base, perm)
        print("batch of %d: %r" % (n, f))
        assert len(perm) == n and n % 64 != 0 and perm.min() >= 0 and perm.max() < ri.N_BASE
        assert f["first_round"] >= 1 and f["tail"] >= 1 and f["uneven_groups"] >= ri.MIN_UNEVEN_GROUPS
        if n >= ri.N_BASE:
            assert len(np.unique(perm)) == ri.N_BASE          # every pair of the base set is in it
        if slots > ri.SLOTS_MIN:                                # a straggler in the first round of claims of THIS launch too
            assert np.isin(perm[ri.SLOTS_MIN:slots], base["stragglers"]).any()


def test_expectations_and_checker(oracle):
    """The vectorised pieces against the per-pair ones they replace: CIGAR text -> run bytes, runs -> edit streams, and the
    comparison itself (it finds a changed byte, length, edit distance and status, and nothing in an exact copy)."""
    base = ri.base_set()
    pick = np.concatenate([np.arange(400), base["stragglers"][:2], np.flatnonzero(base["read_len"] == 0)[:3]])
    sub = {"texts": [base["texts"][k] for k in pick], "reads": [base["reads"][k] for k in pick], "rev": base["rev"][pick]}
    for W, O, stranded in ((64, 33, False), (256, 129, True)):
        exp = ri.expected(oracle, sub, W, O, stranded)
        flat, off = exp["runs"], exp["run_off"]
        for k, c in enumerate(exp["cigars"]):
            r = flat[2 * off[k]: 2 * off[k + 1]]
            assert "".join("%d%s" % (r[2 * q], chr(r[2 * q + 1])) for q in range(len(r) // 2)) == c
        streams, soff = ri.expected_streams(exp)
        for k, c in enumerate(exp["cigars"]):
            assert streams[soff[k]: soff[k + 1]].tobytes() == api.cigar_to_edit_stream(c, W, O)
        # a launch that got everything right, as device_run(raw=True) would report it
        perm = np.resize(np.random.Generator(np.random.PCG64(3)).permutation(len(pick)), 1000)
        n_runs = np.diff(off)
        for edits in (False, True):
            w_bytes, w_off = (streams, soff) if edits else (flat, off)
            unit = 1 if edits else 2
            lens = np.diff(w_off)
            caps = ri.caps_for(np.array([len(x) for x in sub["reads"]]))[perm]
            byte_off = 2 * (np.cumsum(caps) - caps)
            sl = np.zeros(2 * int(caps.sum()), dtype=np.uint8)
            for k, b in enumerate(perm):
                sl[byte_off[k]: byte_off[k] + unit * lens[b]] = w_bytes[unit * w_off[b]: unit * w_off[b + 1]]
            res = {"ed": exp["ed"][perm].copy(), "status": np.zeros(1000, np.int32), "len": lens[perm].copy(), "slices": sl, "perm": perm,
                   "byte_off": byte_off, "run_count": n_runs[perm].astype(np.int32) if edits else None}
            args = (exp["ed"], lens, w_bytes, w_off)
            assert len(check_device_raw(res, *args, want_runs=n_runs)[0]) == 0
            k = int(np.flatnonzero(lens[perm] > 3)[5])
            sl[byte_off[k] + unit * lens[perm[k]] - 1] ^= 1
            res["ed"][7] += 1
            res["status"][11] = 1
            res["len"][13] += 1
            assert sorted(check_device_raw(res, *args, want_runs=n_runs)[0]) == sorted({7, 11, 13, k})
    assert list(ragged_mismatch(np.arange(10, dtype=np.uint8), np.array([0, 4, 4, 8]), np.array([0, 1, 2, 4, 5, 9, 9], dtype=np.uint8),
                                np.array([0, 3, 3, 5]), np.array([3, 0, 2, 2]))) == [3]


# ---------------------------------------------------------------------------------------------------------------- GPU
_packed = {}


def packed_base(al, base, layout):
    """The base set's sequences on the device, packed once per layout."""
    if layout not in _packed:
        _packed[layout] = pack_sequences(al, base["texts"], base["reads"], layout, long_over=ri.LONG_OVER)
    return _packed[layout]


def launch_slots(al, select, **kw):
    """Slots of the launch these parameters get (scrg_query_launch with the very struct, reserved[0] included); the split form of
    the default kernel has a geometry of its own: eight producer wavefronts per CU."""
    p = al._params(kw)
    p.reserved[0] = select
    n_waves, ppw, n_cus = C.c_int32(), C.c_int32(), C.c_int32()
    al._check(al.lib.scrg_query_launch(al.h, C.byref(p), C.byref(n_waves), C.byref(ppw), None, C.byref(n_cus)))
    return n_cus.value * 8 * 64 if select == SPLIT else n_waves.value * ppw.value


def over_limit(exp, max_edits):
    """(over [n], reported edit distance [n]) of every pair of an expected() result at this limit: window_model of tests/test_edit_limit.py."""
    key = ("over", max_edits)
    if key not in exp:
        res = [window_model(c, max_edits, exp["W"], exp["O"]) for c in exp["cigars"]]
        exp[key] = np.array([r[0] for r in res], dtype=bool), np.array([r[1] for r in res], dtype=np.int64)
    return exp[key]


def run_and_compare(al, oracle, W, O, select, layout, edits, mode, seed, **params):
    base = ri.base_set()
    stranded = mode == "stranded"
    kw = dict(W=W, O=O, stranded=int(stranded), text_stride_words=64 if layout == "groups" else 1,
              read_stride_words=64 if layout == "groups" else 1, **params)
    if select != SPLIT:
        kw["waves_per_cu"] = 1
    slots = launch_slots(al, select, **kw)
    times = 2 if select == SPLIT else 3
    n = times * slots + 37
    assert slots >= ri.SLOTS_MIN and n >= times * slots and n % 64 != 0
    perm = ri.build_batch(base, n, seed=seed, slots=slots)
    facts = ri.batch_facts(base, perm)
    assert facts["first_round"] >= 1 and facts["tail"] >= 1, facts
    exp = ri.expected(oracle, base, W, O, stranded)
    max_edits = over = over_ed = None
    if mode == "limit":
        max_edits = int(np.median(exp["ed"]))
        assert api.edit_limit_for(1000, max_edits, None) == max_edits
        over, over_ed = over_limit(exp, max_edits)
    res = device_run(al, base["texts"], base["reads"], base["rev"], W, O, layout, edits, stranded, max_edits, None, select,
                     waves_per_cu=kw.get("waves_per_cu", 0), perm=perm, caps=ri.caps_for(base["read_len"]),
                     packed=packed_base(al, base, layout), raw=True, **params)
    ms = al.last_kernel_ms()
    assert len(res["ed"]) == len(res["status"]) == len(res["len"]) == n
    w_bytes, w_off = ri.expected_streams(exp) if edits else (exp["runs"], exp["run_off"])
    bad, n_over = check_device_raw(res, exp["ed"], np.diff(w_off), w_bytes, w_off, over, over_ed, want_runs=np.diff(exp["run_off"]))
    print("%d descriptors on %d slots (%.1f per slot), kernel %.1f ms, %d over the limit, %d differ" % (n, slots, n / slots, ms, n_over, len(bad)))
    assert len(bad) == 0, "%d of %d descriptors differ from the oracle (%d of them at or above the %d slots); the first: %s" % (
        len(bad), n, int((bad >= slots).sum()), slots,
        ["descriptor %d (pair %d, %s, read %d, status %d)" % (k, perm[k], base["kind"][perm[k]], base["read_len"][perm[k]], res["status"][k]) for k in bad[:8]])
    if mode == "limit":
        assert 0.1 * n < n_over < 0.9 * n, (n_over, n)
    else:
        assert n_over == 0 and not res["status"].any()
    assert al.edit_limit() == (None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LANE_CASES, ids=case_id)
def test_lanes_refill_from_the_queue(aligner, aligner_select, oracle, case):
    """One pair per lane: every lane goes through three pairs and more of very different lengths, in every kernel, both sequence
    layouts, runs and edit streams; once per kernel with minus-strand pairs among the others (forward and reverse lanes come and go
    inside one wavefront) and once with an edit limit at the median edit distance (a dropped pair is followed by a claim)."""
    kernel, W, O, select, layout, edits, mode = case
    run_and_compare(aligner_select if select else aligner, oracle, W, O, select, layout, edits, mode, seed=LANE_CASES.index(case))


@pytest.mark.gpu
@pytest.mark.parametrize("W,O,lanes_per_pair,lds_rows", ROW_CASES)
def test_genasm_row_slots_refill_from_the_queue(aligner, oracle, W, O, lanes_per_pair, lds_rows):
    """The GenASM-row kernels (one word and multiword): a slot of lanes_per_pair lanes takes its next pair, with its per-slot spill
    area reused, once per kernel with few rows in LDS so that it is used."""
    params = dict(lanes_per_pair=lanes_per_pair)
    if lds_rows:
        params["lds_rows"] = lds_rows
    run_and_compare(aligner, oracle, W, O, 0, "contiguous", False, "", seed=100 + lanes_per_pair + W, **params)
