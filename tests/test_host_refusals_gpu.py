"""Every refusal of the host align calls, pinned: status and the exact text of scrg_last_error (the _multi calls:
scrg_multi_last_error) as recorded from the library before the host layer's options were gathered into one struct
(tests/golden/host_refusals.json names the recording commit).

A case sets the handle's options, makes one call that breaks one rule — or two, which pins the order the rules are tried in —
and is replayed after a good call that left side results (and, with the pileup on, an accumulator) on the handle: whatever the
refusal, nothing is left to take afterwards.  `python -m tests.test_host_refusals_gpu FILE` records the cases of the loaded
library (SCRG_LIB) into FILE."""
import json
import os

import pytest

from scrooge_amd import api
from tests.test_host_layouts import batch

N = 65
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_refusals.json")
LONG_TEXT = 4300000             # bases: with the costs below (this + a read) * 510 passes 2^31
WORST_COSTS = (1, 255, 255, 255)


def _leftward(b):
    return [[1] * len(c) for c in b["cands"]]


def _anchors(b):
    return [[(c, 0) for c in cs] for cs in b["cands"]]


def _pairs(**kw):
    return lambda a, b: a.align_pairs(b["texts"], b["reads"], **kw)


def _mapping(**kw):
    return lambda a, b: a.align_mapping(None, b["m_reads"], b["cands"], **kw)


def _directed(**kw):
    return lambda a, b: a.align_mapping_directed(b["m_reads"], b["cands"], leftward=_leftward(b), **kw)


def _anchored(**kw):
    return lambda a, b: a.align_anchored(b["m_reads"], _anchors(b), **kw)


def _long_text(a, b):
    return a.align_pairs([b"A" * LONG_TEXT] + b["texts"][1:], b["reads"])


def _multi(call):
    def run(a, b):
        try:
            return call(a, b)
        finally:
            api.load_library().scrg_multi_release()
    return run


# name -> (the handle's options, the refused call)
CASES = {
    # one option, one rule: in the order the rules are tried
    "limit_lanes": ({"limit": (5, None)}, _pairs(lanes_per_pair=8)),
    "strands_lanes": ({"strands": True}, _pairs(lanes_per_pair=8)),
    "diff_lanes": ({"diff": "md"}, _pairs(lanes_per_pair=8)),
    "diff_distance": ({"diff": "md"}, _mapping(distance_only=True)),
    "diff_leftward": ({"diff": "cs"}, _directed()),
    "report_lanes": ({"report": True}, _mapping(lanes_per_pair=64)),
    "report_distance": ({"report": True}, _pairs(distance_only=True)),
    "clip_distance": ({"clip": True}, _pairs(distance_only=True)),
    "clip_lanes": ({"clip": True}, _mapping(lanes_per_pair=8)),
    "clip_diff": ({"clip": True, "diff": "md"}, _pairs()),
    "clip_report": ({"clip": True, "report": True}, _mapping()),
    "pileup_pairwise": ({"pileup": True}, _pairs()),
    "pileup_distance": ({"pileup": True}, _mapping(distance_only=True)),
    "pileup_lanes": ({"pileup": True}, _mapping(lanes_per_pair=8)),
    "pileup_leftward": ({"pileup": True}, _directed()),
    "pileup_clip": ({"pileup": True, "clip": True}, _mapping()),
    "distance_lanes": ({}, _pairs(distance_only=True, lanes_per_pair=8)),
    "leftward_lanes": ({}, _directed(lanes_per_pair=8)),
    "pairs_best": ({}, _pairs(best=True)),        # (pairs: the entry point's own check answers before the rule "best without mapping" is tried)
    "clip_scores": ({"clip": WORST_COSTS}, _long_text),
    # the same rules through the calls without a handle
    "multi_distance_lanes": ({}, _multi(lambda a, b: a.align_pairs_multi([0], b["texts"], b["reads"], distance_only=True, lanes_per_pair=8))),
    "multi_mapping_distance_lanes": ({}, _multi(lambda a, b: a.align_mapping_multi([0], b["genome"], b["m_reads"], b["cands"], distance_only=True,
                                                                                   lanes_per_pair=64))),
    "multi_pairs_best": ({}, _multi(lambda a, b: a.align_pairs_multi([0], b["texts"], b["reads"], best=True))),
    # two rules at once: the first in the order answers
    "limit_strands_lanes": ({"limit": (None, 100), "strands": True}, _mapping(lanes_per_pair=8)),
    "diff_distance_lanes": ({"diff": "cs"}, _pairs(distance_only=True, lanes_per_pair=8)),
    "report_distance_lanes": ({"report": True}, _pairs(distance_only=True, lanes_per_pair=8)),
    "clip_diff_report": ({"clip": True, "diff": "cs", "report": True}, _pairs()),
    "clip_distance_lanes": ({"clip": True}, _mapping(distance_only=True, lanes_per_pair=8)),
    "pileup_pairwise_distance": ({"pileup": True}, _pairs(distance_only=True)),
    "pileup_clip_leftward": ({"pileup": True, "clip": True}, _directed()),
    "diff_report_leftward": ({"diff": "md", "report": True}, _directed()),
    "clip_scores_diff": ({"clip": WORST_COSTS, "diff": "md"}, _long_text),
    # the anchored call's own
    "anchored_best": ({}, _anchored(best=True)),
    "anchored_limit": ({"limit": (5, None)}, _anchored()),
    "anchored_diff": ({"diff": "md"}, _anchored()),
    "anchored_report": ({"report": True}, _anchored()),
    "anchored_clip": ({"clip": True}, _anchored()),
    "anchored_pileup": ({"pileup": True}, _anchored()),
    "anchored_lanes": ({}, _anchored(lanes_per_pair=8)),
    "anchored_diff_report_clip": ({"diff": "cs", "report": True, "clip": True}, _anchored()),
    "anchored_best_pileup": ({"pileup": True}, _anchored(best=True)),
    "anchored_pileup_lanes": ({"pileup": True}, _anchored(lanes_per_pair=8)),
}

# the good call before the refused one runs with one of these, so that the handle holds every kind of side result once
PRIMES = ({"diff": "cs", "report": True}, {"clip": True})
TAKES = ("take_diff", "take_report", "take_clip", "take_pileup")


def apply(a, o):
    a.set_edit_limit(*o.get("limit", (None, None)))
    a.set_text_strands(o.get("strands", False))
    a.set_diff(o.get("diff"))
    a.set_report(o.get("report", False))
    clip = o.get("clip", False)
    a.set_clip(None if clip in (True, False) else clip, clip is not False)
    if a.pileup() != o.get("pileup", False):       # (switching it off discards the accumulator: only where the case says so)
        a.set_pileup(o.get("pileup", False))


def replay(a, b, name):
    """-> {"status", "error", "left"} of the case's refusal after each of the good calls; asserts that it is a refusal and that
    nothing — no side result, no pileup — is left to take."""
    opts, call = CASES[name]
    seen = []
    try:
        for prime in PRIMES:
            if opts.get("pileup") and "clip" in prime:     # (a good call cannot have both)
                continue
            apply(a, {})
            apply(a, dict(prime, pileup=opts.get("pileup", False)))
            a.align_mapping(None, b["m_reads"], b["cands"])
            apply(a, opts)
            with pytest.raises(api.ScroogeError) as e:
                call(a, b)
            left = []
            for take in TAKES:
                try:
                    getattr(a, take)()
                    left.append(take)
                except api.ScroogeError as t:
                    assert t.status == api.SCRG_ERR_INVALID_ARG, (name, take)
            # what may be left, and is recorded with the rest: the accumulator where a rule of the anchored call before its pileup
            # rule answers, and everything after a call without a handle, which does not touch this one
            if not name.startswith("multi_"):
                assert left in ([], ["take_pileup"]) and (not left or (name.startswith("anchored_") and name != "anchored_pileup")), (name, left)
            seen.append({"status": int(e.value.status), "error": str(e.value).split(": ", 1)[1], "left": left})
    finally:
        apply(a, {})
    return seen


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(aligner, oracle, golden, name):
    b = batch(oracle, N)
    aligner.set_genome(b["genome"])
    assert replay(aligner, b, name) == golden["cases"][name], name


if __name__ == "__main__":
    import subprocess
    import sys

    import scrooge_amd
    from oracle.pyoracle import Oracle
    a = scrooge_amd.Aligner(0)
    b = batch(Oracle(), N)
    a.set_genome(b["genome"])
    commit = os.environ.get("SCRG_RECORDED_AT") or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    cases = {}
    for name in sorted(CASES):
        try:
            cases[name] = replay(a, b, name)
        except Exception as e:                       # (a case that cannot be recorded must not cost the others)
            cases[name] = "NOT RECORDED: %r" % (e,)
            print(name, cases[name])
    out = {"recorded_at_commit": commit, "library": os.path.basename(api.library_path()), "abi_version": int(a.lib.scrg_abi_version()),
           "cases": cases}
    a.close()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d cases" % len(out["cases"]))
