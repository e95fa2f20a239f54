"""Soft clipping in plain Python: THE RULE of include/scrooge_amd.h (SOFT CLIPPING), twice — a quadratic brute force over all
stretches (i, j) for short lists, and the linear procedure — which tests/test_clip.py holds equal, the host function
scrg_clip_from_runs to them, and tests/test_clip_gpu.py the kernel to that."""
import numpy as np

FIELDS = ("read_start", "read_end", "text_start", "text_end", "first_run", "n_runs", "score", "n_edits")
COSTS = (2, 4, 4, 2)              # match, mismatch, gap open, gap extend
OPS = "=XID"


def record(**kw):
    r = dict.fromkeys(FIELDS, 0)
    r.update(kw)
    return r


def is_run(count, op):
    return 0 < count <= 255 and op in OPS


def weights(runs, costs=COSTS):
    """w_k of every run: +match c, -mismatch c, -gap_extend c and a further -gap_open unless the run before is I or D."""
    m, x, o, e = costs
    w = []
    for k, (c, op) in enumerate(runs):
        if op == "=":
            w.append(m * c)
        elif op == "X":
            w.append(-x * c)
        else:
            w.append(-e * c - (0 if k and runs[k - 1][1] in "ID" else o))
    return w


def cuts(runs):
    """(text, read, edits) in front of every run, and behind the last."""
    t = q = e = 0
    out = [(0, 0, 0)]
    for c, op in runs:
        t += c if op != "I" else 0
        q += c if op != "D" else 0
        e += c if op != "=" else 0
        out.append((t, q, e))
    return out


def stretch(runs, i, j, score):
    at = cuts(runs)
    return record(read_start=at[i][1], read_end=at[j + 1][1], text_start=at[i][0], text_end=at[j + 1][0], first_run=i, n_runs=j - i + 1,
                  score=score, n_edits=at[j + 1][2] - at[i][2])


def brute(runs, costs=COSTS):
    """All stretches i <= j that begin and end on '=': the greatest score, then the greatest j, then the least i."""
    runs = list(runs)
    if not all(is_run(c, op) for c, op in runs):
        return record()
    P = np.concatenate([[0], np.cumsum(weights(runs, costs), dtype=np.int64)])
    best = None
    for i in range(len(runs)):
        if runs[i][1] != "=":
            continue
        for j in range(i, len(runs)):
            if runs[j][1] != "=":
                continue
            key = (int(P[j + 1] - P[i]), j, -i)
            if best is None or key > best:
                best = key
    return record() if best is None else stretch(runs, -best[2], best[1], best[0])


def model(runs, costs=COSTS):
    """The linear procedure: for each j the earliest i <= j of the least P_i, then the latest j of the greatest score."""
    runs = list(runs)
    if not all(is_run(c, op) for c, op in runs):
        return record()
    w = weights(runs, costs)
    P, low, low_i, best = 0, None, 0, None
    for k, (c, op) in enumerate(runs):
        if op == "=" and (low is None or P < low):
            low, low_i = P, k
        P += w[k]
        if op == "=" and (best is None or P - low >= best[0]):
            best = (P - low, low_i, k)
    return record() if best is None else stretch(runs, best[1], best[2], best[0])


def random_runs(rng, n, max_count=255, p_match=0.5):
    """n runs: '=' with probability p_match, else X / I / D; directly adjacent runs may repeat an operation, as windows leave them."""
    ops = np.where(rng.random(n) < p_match, 0, rng.integers(1, 4, size=n))
    counts = rng.integers(1, max_count + 1, size=n)
    return [(int(c), OPS[int(o)]) for c, o in zip(counts, ops)]


def random_costs(rng):
    """match in 1..255, the others in 0..255 — small ones and zeros often, so that ties happen."""
    small = rng.random() < 0.7
    hi = 4 if small else 256
    return (int(rng.integers(1, hi)),) + tuple(int(x) for x in rng.integers(0, hi, size=3))


def kept(runs, rec):
    return list(runs)[rec["first_run"]:rec["first_run"] + rec["n_runs"]]
