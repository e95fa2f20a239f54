"""Every per-handle output of a host call at once, across chunks: 2 * 512 + 37 pairs are three chunks, the last with a partial
group (tests/test_host_layouts.py), in both issue orders — where the code the outputs share can go wrong: a chunk's base, the
permutation into caller order, one kind's buffer taken for the other's.

With the report, a difference-string kind and the merged CIGAR form on, each output is the one a call with only that output on
gives, the result is the one a call with neither gives, and the records and strings are those of the Python models.  Clipping,
which goes with neither, runs alone at the same size."""
import numpy as np
import pytest

from scrooge_amd import api
from tests import cigar_form_model as fm
from tests import diff_model as dm
from tests import report_model as rm
from tests.test_clip_gpu import check_clipped, cigars_of, runs_of
from tests.test_host_layouts import batch
from tests.test_pair_report_gpu import mapping_texts

N = 2 * 512 + 37
OK = api.SCRG_OK
RESULT = ("edit_distance", "status", "run_offset", "cigar_offset")
# the call, and the statuses that leave a pair without an alignment
MODES = {"pairs": ({}, ()), "best": ({"best": True}, (api.SCRG_PAIR_NOT_BEST,)), "limit": ({"max_edits": 12}, (api.SCRG_PAIR_OVER_EDIT_LIMIT,))}


def call(aligner, b, mode, **kw):
    kw.update(MODES[mode][0])
    if mode == "pairs":
        return aligner.align_pairs(b["texts"], b["reads"], arrays=True, **kw)
    return aligner.align_mapping(None, b["m_reads"], b["cands"], arrays=True, **kw)


def same_result(got, want, what):
    for k in RESULT:
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["runs"].tobytes() == want["runs"].tobytes() and got["cigar_text"] == want["cigar_text"], what


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_report_diff_and_form_together(aligner, oracle, mode, sort):
    b = batch(oracle, N)
    aligner.set_genome(b["genome"])
    what = "%s sort_by_length=%d" % (mode, sort)
    texts, reads = (b["texts"], b["reads"]) if mode == "pairs" else mapping_texts(b, b["m_reads"])
    every = call(aligner, b, mode, report=True, diff="cs", cigar_form="merged", sort_by_length=sort)
    only_report = call(aligner, b, mode, report=True, sort_by_length=sort)
    only_diff = call(aligner, b, mode, diff="cs", sort_by_length=sort)
    neither = call(aligner, b, mode, cigar_form="merged", sort_by_length=sort)
    windowed = call(aligner, b, mode, sort_by_length=sort)
    assert len(every["status"]) == N and set(every) == set(neither) | {"report", "diff_offset", "diff_text"}, what
    assert every["report"].tobytes() == only_report["report"].tobytes(), what
    assert np.array_equal(every["diff_offset"], only_diff["diff_offset"]) and every["diff_text"] == only_diff["diff_text"], what
    same_result(every, neither, what)
    same_result(only_report, windowed, what)
    same_result(only_diff, windowed, what)
    # the models, on the runs of the call with neither
    off = every["diff_offset"].astype(np.int64)
    assert off[0] == 0 and off[N] == len(every["diff_text"]), what
    cigars, missing = cigars_of(every), 0
    for p in range(N):
        runs = runs_of(windowed, p)
        none = windowed["status"][p] in MODES[mode][1]
        missing += none
        assert (windowed["status"][p] == OK) != none and (not none or not runs), (what, p)
        want = rm.record(verdict=rm.NO_ALIGNMENT) if none else rm.model(texts[p], reads[p], runs, int(windowed["edit_distance"][p]))
        assert {f: int(every["report"][p][f]) for f in rm.FIELDS} == want and (none or want["verdict"] == 0), (what, p)
        assert every["diff_text"][off[p]:off[p + 1]] == ("" if none else dm.model("cs", texts[p], reads[p], runs)).encode() + b"\0", (what, p)
        assert cigars[p] == fm.model("merged", runs), (what, p)
    assert missing == {"pairs": 0, "best": N // 2}.get(mode, missing) and (mode != "limit" or 0 < missing < N), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_clip_alone(aligner, oracle, mode):
    b = batch(oracle, N)
    aligner.set_genome(b["genome"])
    for sort in (0, 1):
        off = call(aligner, b, mode, sort_by_length=sort)
        on = call(aligner, b, mode, clip=True, sort_by_length=sort)
        assert set(on) == set(off) | {"clip"}
        check_clipped(on, off, "clip %s sort_by_length=%d" % (mode, sort))
