"""The pileup in plain Python: THE RULE of include/scrooge_amd.h (PILEUP), twice — run by run as the rule states it (model), and
column by column from the expanded CIGAR (brute) — which tests/test_pileup.py holds equal, the host function
scrg_pileup_from_runs to them, and tests/test_pileup_gpu.py the kernels to that."""
import numpy as np

from tests.clip_model import OPS, random_runs

MATCH, A, C, G, T, DEL, INS = range(7)
PLANES = 7
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def empty(target_len):
    return np.zeros((PLANES, target_len + 1), dtype=np.uint32)


def _read(read_aligned):
    return (read_aligned.decode("latin-1") if isinstance(read_aligned, (bytes, bytearray)) else read_aligned).upper()


def model(runs, read_aligned, start, target_len, counts=None):
    """One alignment, run by run -> (counts: (7, target_len + 1) uint32, added to `counts` if given; out_of_range)."""
    n = empty(target_len) if counts is None else counts
    read = _read(read_aligned)
    L = target_len
    t = q = 0
    prev = None
    outside = False
    for c, op in runs:
        g = start + t
        if op == "I":
            if prev != "I":                   # directly adjacent I runs are one insertion, in front of the next text column
                if g > L:
                    outside = True
                else:
                    n[INS, g] += 1
        else:
            lo, hi = min(g, L), min(g + c, L)
            outside |= g + c > L
            if op == "=":
                n[MATCH, lo:hi] += 1
            elif op == "D":
                n[DEL, lo:hi] += 1
            else:
                for k in range(hi - lo):
                    n[A + CODE[read[q + k]], lo + k] += 1
        t += c if op != "I" else 0
        q += c if op != "D" else 0
        prev = op
    return n, outside


def brute(runs, read_aligned, start, target_len):
    """The same from the CIGAR expanded to one operation per column."""
    n = empty(target_len)
    read = _read(read_aligned)
    cols = "".join(op * c for c, op in runs)
    t = q = 0
    outside = False
    for k, op in enumerate(cols):
        g = start + t
        if op == "I":
            if k == 0 or cols[k - 1] != "I":
                if g <= target_len:
                    n[INS, g] += 1
                else:
                    outside = True
            q += 1
            continue
        if g < target_len:
            n[MATCH if op == "=" else DEL if op == "D" else A + CODE[read[q]], g] += 1
        else:
            outside = True
        t += 1
        q += op != "D"
    return n, outside


def consumed(runs):
    """-> (text, read) bases the runs consume."""
    return sum(c for c, op in runs if op != "I"), sum(c for c, op in runs if op != "D")


def random_read(rng, n):
    return bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=n))


def random_alignment(rng, n_runs, max_count=255, p_match=0.5):
    """n_runs random valid runs (tests/clip_model.py: directly adjacent runs may repeat an operation) and a random read, as
    aligned, of exactly the length they consume."""
    runs = random_runs(rng, n_runs, max_count=max_count, p_match=p_match)
    return runs, random_read(rng, consumed(runs)[1])


def edges_to_counts(acc):
    """What scrg_pileup_finish computes: the inclusive prefix sums of planes 0 and 5 mod 2^32, the other planes as they are."""
    out = np.array(acc, dtype=np.uint32, copy=True)
    for plane in (MATCH, DEL):
        out[plane] = (np.cumsum(acc[plane].astype(np.int64)) & 0xFFFFFFFF).astype(np.uint32)
    return out


assert OPS == "=XID"
