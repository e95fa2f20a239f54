"""Inputs for the work-queue refill tests (tests/test_queue_refill.py): one base set of very uneven pairs and a builder that
turns it into device-layer batches of any size.

A plain module like tests/plane_inputs.py: no fixtures, no pytest settings, everything a function of a seed.

Every align kernel is persistent: a lane claims a pair from an atomic queue, retires it and claims the next while its 63
neighbours are in the middle of theirs.  A launch only gets there when it has more pairs than slots, so the batches here are
DESCRIPTOR REPLICATIONS of the base set: the packed sequences are stored once, a batch is n descriptors that point at them in a
seeded permutation (repeated as often as n asks for), each with a CIGAR slice of its own, sized per pair.  Expected results are
the oracle's for the base set, indexed through the permutation (expected(), cached per window setting).

The conditions the tests assert about these inputs (tests/test_queue_refill.py: test_base_set_and_batches_meet_their_conditions)
are constants here."""
import ctypes as C
import functools

import numpy as np

from scrooge_amd import api, synth

N_BASE = 50_000
STRAGGLER_LEN = 20_000
READ_CAP = 1_500
LONG_OVER = 2 * READ_CAP          # pairs with a longer text or read are packed in rows of their own (pack_sequences: long_over)
SLOTS_MIN = 256                   # the smallest slot count of any launch: one wavefront per CU, one pair per wavefront, 256 CUs
TAIL = 1_000                      # "near the end of the queue": the last TAIL descriptors
# what the base set must hold (the issue's conditions; the CPU test asserts them)
MIN_STRAGGLERS, STRAGGLER_FACTOR, MIN_EMPTY_READS, MIN_EMPTY_TEXTS, MIN_READ_OUTLASTS_TEXT = 20, 50, 100, 10, 1_000
UNEVEN_FACTOR, MIN_UNEVEN_GROUPS = 10, 0.05

_RC = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(_RC)[::-1]


@functools.lru_cache(maxsize=2)
def base_set(seed=1, n=N_BASE):
    """-> dict: texts, reads (lists of bytes), kind (list of str), stragglers (indices), rev (bool [n]: the pairs that the
    stranded launches align as reverse complements, about 30 %), read_len / text_len (int64 [n])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    err, ratio = synth.PROFILES["ont"]
    two = [np.frombuffer(x, np.uint8) for x in (b"AC", b"GT", b"AT")]
    stragglers = set(int(x) for x in rng.choice(n, max(24, n // 1600), replace=False))

    def geo():
        return int(min(READ_CAP, rng.geometric(1.0 / 250)))

    texts, reads, kind = [], [], []
    for k in range(n):
        u = rng.random()
        if k in stragglers:
            t, q = synth.make_pair(STRAGGLER_LEN, err, ratio, rng)
            t, q, what = synth.BASES[t].tobytes(), synth.BASES[q].tobytes(), "straggler"
        elif u < 0.15:                                  # unrelated, ragged: empty reads, empty texts, reads that outlast their text
            v = rng.random()
            t = b"" if 0.03 <= v < 0.035 else synth.random_seq(geo(), rng)
            q = b"" if v < 0.03 else synth.random_seq(geo(), rng)
            what = "unrelated"
        elif u < 0.153:                                 # low complexity: a two-letter alphabet (ties), homopolymers
            v = rng.random()
            if v < 0.5:
                ab = two[int(rng.integers(0, 3))]
                t, q = bytes(rng.choice(ab, int(rng.integers(1, 500)))), bytes(rng.choice(ab, int(rng.integers(1, 500))))
            else:
                a, b = b"ACGT"[int(rng.integers(0, 4))], b"ACGT"[int(rng.integers(0, 4))]
                t, q = bytes([a]) * int(rng.integers(1, 600)), bytes([b]) * int(rng.integers(1, 600))
            what = "low_complexity"
        else:
            t, q = synth.make_pair(geo(), err, ratio, rng)
            t, q, what = synth.BASES[t].tobytes(), synth.BASES[q].tobytes(), "ont"
        texts.append(t), reads.append(q), kind.append(what)
    return {"texts": texts, "reads": reads, "kind": kind, "stragglers": np.array(sorted(stragglers), dtype=np.int64),
            "rev": rng.random(n) < 0.3,
            "read_len": np.array([len(x) for x in reads], dtype=np.int64), "text_len": np.array([len(x) for x in texts], dtype=np.int64)}


def caps_for(read_len):
    """Per-pair slice capacities in runs: roundup16(2 * read_len + 16)."""
    return (2 * np.asarray(read_len, dtype=np.int64) + 16 + 15) // 16 * 16


def build_batch(base, n, seed=0, slots=None):
    """-> int64 [n]: descriptor k points at base pair perm[k].  A seeded permutation of the base set, repeated (or cut) to n;
    then stragglers are put where both kinds of hand-over meet them: in the first round of claims (below SLOTS_MIN, and below
    `slots` if given: a lane stays in one pair while its neighbours go through dozens) and among the last descriptors of the queue
    (a lane runs on while its neighbours sit idle with the queue empty)."""
    N = len(base["reads"])
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    perm = np.resize(rng.permutation(N), n).astype(np.int64)
    want = [5, 70, 200] + ([slots // 3, slots - 9] if slots and SLOTS_MIN < slots <= n - TAIL else []) + [n - 700, n - 41, n - 3]
    want = [p for p in dict.fromkeys(want) if 0 <= p < n]
    stragglers = base["stragglers"][rng.permutation(len(base["stragglers"]))][:len(want)]
    for p, s in zip(want, stragglers):
        at = np.flatnonzero(perm == s)
        at = at[~np.isin(at, want)]
        if len(at):
            perm[at[0]] = perm[p]                       # a swap where the permutation holds s already
        perm[p] = s
    return perm


def batch_facts(base, perm):
    """What the conditions ask of a built batch."""
    n, rl = len(perm), base["read_len"][perm]
    is_s = np.isin(perm, base["stragglers"])
    full = rl[: n // 64 * 64].reshape(-1, 64)
    med = np.median(full, axis=1)
    return {"first_round": int(is_s[:SLOTS_MIN].sum()), "tail": int(is_s[-TAIL:].sum()),
            "uneven_groups": float(np.mean(full.max(axis=1) >= UNEVEN_FACTOR * np.maximum(med, 1)))}


# ------------------------------------------------------------------------------------------------ expected results
def parse_cigars(cigars):
    """CIGAR texts -> (run bytes uint8 [2 * total] = count, op, ..., offsets int64 [n + 1] in runs), without a loop over pairs."""
    a = np.frombuffer(("\n".join(cigars) + "\n").encode(), dtype=np.uint8)
    digit = (a >= 48) & (a <= 57)
    stops = np.flatnonzero(~digit)                      # operations and line ends
    ops = stops[a[stops] != 10]
    before = np.concatenate([[-1], stops])[np.searchsorted(stops, ops)]
    nd = ops - before - 1
    assert len(ops) == 0 or (nd.min() >= 1 and nd.max() <= 3), "a run count of 1 to 3 digits before every operation"
    d = np.concatenate([np.zeros(3, np.int64), a.astype(np.int64) - 48])      # (three zeros in front: ops - 3 never wraps)
    val = d[ops + 2] + np.where(nd >= 2, 10 * d[ops + 1], 0) + np.where(nd >= 3, 100 * d[ops], 0)
    assert len(ops) == 0 or (val.min() >= 1 and val.max() <= 255)
    assert np.isin(a[ops], np.frombuffer(b"=XID", np.uint8)).all()
    flat = np.stack([val.astype(np.uint8), a[ops]], axis=1).reshape(-1)
    off = np.concatenate([[0], np.searchsorted(ops, np.flatnonzero(a == 10))]).astype(np.int64)
    return flat, off


def runs_to_streams(flat, off, W, O):
    """The canonical edit stream of every pair's runs (scrg_runs_to_edit_stream, no GPU) -> (bytes uint8, offsets int64 [n + 1])."""
    lib = api.load_library()
    p = api.Params()
    lib.scrg_params_default(C.byref(p))
    p.W, p.O = int(W), int(O)
    n = len(off) - 1
    flat = np.ascontiguousarray(flat)
    # (a byte per edited character, per 63 matches and per window end: no more than every run's count, a byte per run, and slack)
    out = np.zeros(int(flat[0::2].sum(dtype=np.int64)) + len(flat) + 8 * n + 64, dtype=np.uint8)
    soff = np.zeros(n + 1, dtype=np.int64)
    nb, pos, src, dst, pp = C.c_uint64(0), 0, flat.ctypes.data, out.ctypes.data, C.byref(p)
    fn = lib.scrg_runs_to_edit_stream
    for k in range(n):
        st = fn(pp, src + 2 * int(off[k]), int(off[k + 1] - off[k]), dst + pos, len(out) - pos, C.byref(nb))
        assert st == 0, (k, st)
        pos += nb.value
        soff[k + 1] = pos
    return out[:pos].copy(), soff


_expected = {}


def expected(oracle, base, W, O, stranded=False, threads=16):
    """The oracle's results for the base set at W/O (stranded: the pairs of base['rev'] with their reads reverse-complemented)
    -> dict: ed int64 [n], cigars (list of str), runs / run_off (parse_cigars).  Computed once per setting."""
    key = (id(base), W, O, bool(stranded))
    if key not in _expected:
        reads = [revcomp(r) if v else r for r, v in zip(base["reads"], base["rev"])] if stranded else base["reads"]
        eds, cigars, _, _ = oracle.align(base["texts"], reads, W=W, O=O, threads=threads)
        flat, off = parse_cigars(cigars)
        _expected[key] = {"ed": np.array(eds, dtype=np.int64), "cigars": cigars, "runs": flat, "run_off": off, "W": W, "O": O,
                          "base": base}                 # (kept alive: the key holds its id)
    return _expected[key]


def expected_streams(exp):
    """(stream bytes, offsets) of an expected() result, added to it on first use."""
    if "streams" not in exp:
        exp["streams"], exp["stream_off"] = runs_to_streams(exp["runs"], exp["run_off"], exp["W"], exp["O"])
    return exp["streams"], exp["stream_off"]
