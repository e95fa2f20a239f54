"""The alignment report (scrg_pair_report) as a Python model written from the rules of include/scrooge_amd.h (ALIGNMENT REPORT), and
the inputs of tests/test_pair_report.py and tests/test_pair_report_gpu.py.  Nothing here calls the library.

The verdict is a walk over the runs in order, t and q the positions in the text and in the read as aligned:
  per run: count 0 -> 2 (before the operation is looked at); an operation other than = X I D -> 1;
           '=' / 'X': past the read -> 3, then past the text -> 4, then a base whose equality disagrees with the operation -> 5;
           'I': past the read -> 3;  'D': past the text -> 4;
  after the last run: read not consumed exactly -> 3, then n_mismatch + n_ins + n_del != edit distance -> 6.
The first failure wins; bad_run is its run (the number of runs for the two met after the last run).  The counts cover all runs for
verdict 0, 6 and the 3 met after the last run, and are 0 otherwise.  Runs here are (count, op) with op a one-character str."""
import numpy as np

from tests import diff_model as dm

FIELDS = ("n_match", "n_mismatch", "n_ins", "n_del", "n_gap_open", "n_indel", "verdict", "bad_run")
NO_ALIGNMENT = 7
COSTS = (2, 4, 4, 2)


def record(**kw):
    r = dict.fromkeys(FIELDS, 0)
    r.update(kw)
    return r


def model(text, read, runs, edit_distance):
    """-> dict with FIELDS"""
    text = (text.decode() if isinstance(text, (bytes, bytearray)) else text).upper()
    read = (read.decode() if isinstance(read, (bytes, bytearray)) else read).upper()
    n = dict.fromkeys(FIELDS[:6], 0)
    t = q = 0
    prev = None
    for k, (c, op) in enumerate(runs):
        if c == 0:
            return record(verdict=2, bad_run=k)
        if op in "=X" and len(op) == 1:
            if q + c > len(read):
                return record(verdict=3, bad_run=k)
            if t + c > len(text):
                return record(verdict=4, bad_run=k)
            if any((text[t + j] == read[q + j]) != (op == "=") for j in range(c)):
                return record(verdict=5, bad_run=k)
            n["n_match" if op == "=" else "n_mismatch"] += c
            t += c
            q += c
        elif op == "I":
            if q + c > len(read):
                return record(verdict=3, bad_run=k)
            n["n_ins"] += c
            q += c
        elif op == "D":
            if t + c > len(text):
                return record(verdict=4, bad_run=k)
            n["n_del"] += c
            t += c
        else:
            return record(verdict=1, bad_run=k)
        if op in "ID":
            n["n_gap_open"] += prev not in ("I", "D")
            n["n_indel"] += prev != op
        prev = op
    if q != len(read):
        return record(verdict=3, bad_run=len(runs), **n)
    if n["n_mismatch"] + n["n_ins"] + n["n_del"] != edit_distance:
        return record(verdict=6, bad_run=len(runs), **n)
    return record(**n)


def score(rep, costs=COSTS):
    m, x, o, e = costs
    return m * rep["n_match"] - x * rep["n_mismatch"] - o * rep["n_gap_open"] - e * (rep["n_ins"] + rep["n_del"])


def divergence(rep):
    """de: the gap-compressed divergence"""
    num = rep["n_mismatch"] + rep["n_indel"]
    return num / (rep["n_match"] + num) if rep["n_match"] + num else 0.0


def edits(runs):
    return sum(c for c, o in runs if o != "=")


# text, read, runs, edit distance -> the record, written out by hand: one case per verdict, both kinds of 3
TABLE = [
    ("ACGTACGTAC", "ACGTTCGAC", "4=1X2=1D2=", 2, record(n_match=8, n_mismatch=1, n_del=1, n_gap_open=1, n_indel=1)),
    # adjacent I and D runs share one opening and are two stretches; D D is one of each
    ("AC", "GTG", "1D1I1D2I", 5, record(n_ins=3, n_del=2, n_gap_open=1, n_indel=4)),
    ("ACGTACGTTA", "ACGTGTA", "2=2=1X1X1D2D1=", 5, record(n_match=5, n_mismatch=2, n_del=3, n_gap_open=1, n_indel=1)),
    ("ACGT", "", "", 0, record()),                                                        # an empty read, no runs: ok
    ("acgt", "ACGT", "4=", 0, record(n_match=4)),                                         # case-blind
    ("ACGT", "ACGT", [(2, "="), (2, "M")], 0, record(verdict=1, bad_run=1)),
    ("ACGT", "ACGT", [(2, "="), (0, "M"), (2, "=")], 0, record(verdict=2, bad_run=1)),    # the count is checked before the operation
    ("ACGTA", "ACGT", "3=2=", 0, record(verdict=3, bad_run=1)),                           # past the read, at a run
    ("ACGT", "ACGTA", "4=", 0, record(verdict=3, bad_run=1, n_match=4)),                  # read not consumed, after the last run: counts
    ("ACGT", "ACGTA", "", 0, record(verdict=3, bad_run=0)),
    ("ACG", "ACGT", "2=2=", 0, record(verdict=4, bad_run=1)),
    ("ACG", "ACGTT", "3=1D1I", 2, record(verdict=4, bad_run=1)),
    ("ACGT", "ACCT", "1=3=", 0, record(verdict=5, bad_run=1)),
    ("ACGT", "ACCT", "2=1X1=", 1, record(n_match=3, n_mismatch=1)),
    ("ACGT", "ACGA", "2=2X", 2, record(verdict=5, bad_run=1)),                            # an X base that is equal
    ("ACGT", "ACCT", "2=1X1=", 2, record(verdict=6, bad_run=3, n_match=3, n_mismatch=1)),
    ("ACGT", "ACGT", "3=2=", 0, record(verdict=3, bad_run=1)),                            # past both: past the read is met first
]


def flip(base):
    return "ACGT"[("ACGT".index(base.upper()) + 1) % 4]


CORRUPTIONS = ["zero_count", "op_M", "extra_I", "extra_D", "flip_in_eq", "equal_in_X", "ed_off"]


def corrupt(kind, text, read, runs, ed, rng):
    """One of the seven ways the tests spoil a valid case; -> (text, read, runs, ed), or None where the case has no place for it
    (no '=' run, no 'X' run, no runs at all)."""
    runs = list(runs)
    if kind == "ed_off":
        return text, read, runs, ed + 1
    if kind in ("extra_I", "extra_D"):
        return text, read, runs + [(1, kind[-1])], ed
    if not runs:
        return None
    if kind in ("zero_count", "op_M"):
        k = int(rng.integers(0, len(runs)))
        runs[k] = (0, runs[k][1]) if kind == "zero_count" else (runs[k][0], "M")
        return text, read, runs, ed
    want = "=" if kind == "flip_in_eq" else "X"
    at = [k for k, (c, o) in enumerate(runs) if o == want]
    if not at:
        return None
    k = at[int(rng.integers(0, len(at)))]
    t, q = dm.consumed(runs[:k])
    j = int(rng.integers(0, runs[k][0]))
    read = list(read)
    read[q + j] = flip(text[t + j]) if kind == "flip_in_eq" else text[t + j]
    return text, "".join(read), runs, ed


def valid_case(rng, n_runs, max_count=255, slack=None):
    """dm.random_case with the read made to agree with the runs: '=' bases equal the text's, 'X' bases differ.  -> (text, read, runs, ed)"""
    text, read, runs = dm.random_case(rng, n_runs, max_count, slack)
    read = list(read)
    t = q = 0
    for c, op in runs:
        if op in "=X":
            for j in range(c):
                read[q + j] = text[t + j] if op == "=" else flip(text[t + j])
        if op != "I":
            t += c
        if op != "D":
            q += c
    return text, "".join(read), runs, edits(runs)


def cigar_runs(cigar):
    """A CIGAR with counts of any size -> runs with counts of at most 255 (a long count split into runs of the same operation)."""
    import re
    out = []
    for n, o in re.findall(r"(\d+)([=XID])", cigar):
        n = int(n)
        while n > 255:
            out.append((255, o))
            n -= 255
        if n:
            out.append((n, o))
    return out


def sequences_for(runs, rng):
    """A text and a read that the runs are an alignment of."""
    tl, ql = dm.consumed(runs)
    text = dm.random_seq(rng, tl)
    read = list(dm.random_seq(rng, ql))
    t = q = 0
    for c, op in runs:
        if op in "=X":
            for j in range(c):
                read[q + j] = text[t + j] if op == "=" else flip(text[t + j])
        if op != "I":
            t += c
        if op != "D":
            q += c
    return text, "".join(read)


def as_dict(rec):
    """A row of a structured array / a ctypes record -> dict"""
    if isinstance(rec, dict):
        return rec
    if isinstance(rec, np.void):
        return {f: int(rec[f]) for f in FIELDS}
    return {f: int(getattr(rec, f)) for f in FIELDS}
