"""The two traceback passes of genasm_lane_kernel (genasm_lane_kernel.hip) on the GPU, on pairs made for what they pass through LDS.

Pass 1 leaves one byte per kept column (the length of the insertion run that begins there), pass 2 reads the bytes of the columns
that hold an event and turns the masks into runs, two events per trip, looking at the staging ring from the fifth trip on.  The
batches here put into ONE wavefront, per W/O:

  insertion runs   of every length that fits, beginning in the first, a middle and the last kept column.  A window ends when W-O
                   read characters are consumed, so a run that begins in column c after c diagonal steps has at most W-O - c
                   members: lengths 1 .. W-O in column 0, 1 .. W-O - c in column c, 1 in the last one.  Every length byte 1 .. W-O
                   is written and read back, in every column a run can begin in;
  busy windows     with an event in every kept column — X / = alternating, D / = alternating: pass 2 runs 16 trips (W-O = 31),
                   the ring guard fires and the ring wraps;
  clean lanes      next to them, long and short ones (lanes retire at different rounds), and — the pair count is no multiple of
                   64 — lanes without a pair.

The crafted windows of a lane are spaced so that the windows in between are clean and a W = 64 wavefront has band rounds that
commit (runs up to 15 and X / = windows stay under the band's threshold) next to rounds that are redone (longer runs, D / =
windows): both walk forms write the bytes.  W/O = 64/33 is the unrolled walk, 64/40, 64/63 and 48/20 the one with the
per-column limit; 48/20 has no band.  Runs, edit streams and distances are compared byte for byte with the oracle, for the shipped
build and for the test build with the band off (reserved[0] = 4096) and in every eligible round (8192).

What the batches hold is asserted on the CPU from the oracle's CIGARs, replayed window by window (test_the_windows_hold_...)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from scrooge_amd import api, synth
from tests.test_edit_limit import pack_sequences
from tests.test_gpu_band_table import BAND_ALWAYS, NO_BAND, compare

CONFIGS = ((64, 33), (64, 40), (64, 63), (48, 20))
N_PAIRS = 150                    # two wavefronts and 22 lanes of a third: 42 lanes without a pair
MAX_READ = 400
LETTERS = b"ACGT"


def _other(rng, *avoid):
    """A base that is none of `avoid`."""
    return int(rng.choice([b for b in LETTERS if b not in avoid]))


def _rand(rng, n):
    return bytes(rng.choice(np.frombuffer(LETTERS, np.uint8), n)) if n else b""


def slots(W, T):
    """The rounds a lane's crafted windows sit in: far enough apart that no window sees two of them, the last one early enough
    that a read of MAX_READ bases still has a full window there."""
    step = -(-W // T) + 1
    return list(range(1, (MAX_READ - W) // T + 1, step))


def cases(T):
    """(column, length) of the insertion runs: every length that fits in the first, a middle and the last kept column."""
    return [(c, L) for c in sorted({0, T // 2, T - 1}) for L in range(1, T - c + 1)]


def _window(kind, T, rng, before, first):
    """One window's stretch of (text, read), made so that the window consumes exactly it -> (text, read, the base the next
    window's read has to begin with or None).  before: the base in front (text and read agree there); first: the base this
    window's read has to begin with, if the window before it asked for one (never an "ins" window: those stand alone)."""
    if kind[0] == "ins":                         # c matches, L inserted bases, the rest of the window's W-O read characters
        _, c, L = kind
        m1, m2 = _rand(rng, c), _rand(rng, T - c - L)
        after = m2[0] if m2 else int(rng.choice(np.frombuffer(LETTERS, np.uint8)))      # (the next window's first base if the run ends this one)
        left = (m1 or bytes([before]))[-1]
        # No inserted base is the text base behind the run or the one in front of it.  The removed characters of an optimal
        # alignment are then the run's and no others (a kept inserted base would have to be one of the two), so the walk — which
        # takes an insertion wherever one lies on an optimal path — cannot begin the run early or split it.
        ins = bytes(_other(rng, left, after) for _ in range(L))
        return m1 + m2, m1 + bytes(ins) + m2, (None if m2 else after)
    if kind[0] == "xeq":                         # a substitution in every even column
        # (the read repeats no base within two places and a substituted text base is none of the read's around it where that
        # can be had: fewer stretches in which an insertion and a deletion cost no more than the substitutions between them —
        # the walk takes those; what is left of them is sorted out by batch(), which asks the oracle)
        q = bytearray()
        for i in range(T):
            q.append(first if (i == 0 and first is not None) else _other(rng, *(list(q[-2:]) or [before])))
        after = _other(rng, *q[-2:])
        t = bytearray(q)
        ext = bytes([before]) * 2 + bytes(q) + bytes([after]) * 2
        for i in range(0, T, 2):
            near = ext[i + 1:i + 4]              # q[i - 1], q[i], q[i + 1]
            far = [b for b in (ext[i], ext[i + 4]) if len(set(near) | {b}) < 4]
            t[i] = _other(rng, *near, *far[:4 - 1 - len(set(near))])
        return bytes(t), bytes(q), (after if T % 2 == 1 else None)
    if kind[0] == "deq":                         # a deletion in each of the first kind[1] even columns, substitutions in the others
        # (a deleted text base is neither the read base in front of it nor the one behind; the columns behind the deletions as in "xeq")
        nD = kind[1]
        q, t = bytearray(), bytearray()
        after = int(rng.choice(np.frombuffer(LETTERS, np.uint8)))
        nq = T - nD
        for i in range(nq):
            q.append(first if (i == 0 and first is not None) else _other(rng, *(list(q[-2:]) or [before])))
        if nq == 0 and first is not None:
            after = first
        k = 0                                    # read characters consumed
        for c in range(T):
            prev, here, nxt = (q[k - 1] if k else before), (q[k] if k < nq else after), (q[k + 1] if k + 1 < nq else after)
            if c % 2 == 0 and c < 2 * nD:
                t.append(_other(rng, prev, here))
            elif c % 2 == 0:
                t.append(_other(rng, prev, here, nxt))
                k += 1
            else:
                t.append(here)
                k += 1
        assert k == nq
        return bytes(t), bytes(q), after
    m = bytearray(_rand(rng, T))
    if first is not None:
        m[0] = first
    return bytes(m), bytes(m), None


def _pair(plan, T, length, rng):
    """plan: {round: kind} -> (text, read) of `length` read bases; clean windows everywhere else (round 0 always), 64 more text
    bases at the end."""
    t, q, first, r = bytearray(), bytearray(), None, 0
    while len(q) < length:
        kind = plan.get(r, ("clean",))
        assert first is None or kind[0] != "ins"
        wt, wq, first = _window(kind, T, rng, q[-1] if q else LETTERS[0], first)
        t += wt
        q += wq
        r += 1
    cut = len(q) - length                        # (inside a clean window: text and read end together)
    return bytes(t[:len(t) - cut] + _rand(rng, 64)), bytes(q[:length])


def _realised(plan, W, O, length, rng):
    """A pair made for the plan, if the oracle's windows come out as planned; else None."""
    t, q = _pair(plan, W - O, length, rng)
    if plan and not holds(plan, _oracle().align([t], [q], W=W, O=O)[1][0], len(q), W, W - O):
        return None
    return t, q


@functools.lru_cache(maxsize=None)
def batch(W, O):
    """-> dict(texts, reads, plans): pair k is lane k % 64 of wavefront k // 64; every wavefront follows the same lane plan."""
    T = W - O
    rng = np.random.Generator(np.random.PCG64(1000 * W + O))
    sl = slots(W, T)
    full = sl[-1] * T + W                       # a read this long has a full window in the last crafted round
    cs = cases(T)
    big = [x for x in cs if x[1] > 15]
    small = [x for x in cs if x[1] <= 15]
    lane_plans = []
    # insertion lanes: a long run (the band cannot hold it: these share the first slot, so that the later slots' rounds stay safe)
    # and short ones in the later slots
    per = max(1, len(sl) - 1)
    n_ins = max(len(big), -(-len(small) // per))
    for k in range(n_ins):
        plan = {}
        if k < len(big):
            plan[sl[0]] = ("ins",) + big[k]
        for s, x in zip(sl[1:] if len(sl) > 1 else sl, small[k * per:(k + 1) * per]):
            plan[s] = ("ins",) + x
        lane_plans.append(plan)
    # busy lanes, one busy window per slot (two in a row cannot be had: with half of a window's 64 columns substituted the
    # window's best alignment is no longer the substitutions).  X / = windows stay under the band's threshold, D / = windows do
    # not (16 deletions leave the band): those stand in the first slot only.
    later = sl[1:] if len(sl) > 1 else sl
    # (a window owes its deletions back — its 64 read characters end that many columns later, past the window's text if there are
    # many — so with a small W the D / = pattern of a whole window is not the best alignment: as many deletions as come out as
    # made in at least one pair of four)
    deq = None
    for nD in range((T + 1) // 2, 0, -1):
        if sum(_realised({sl[0]: ("deq", nD)}, W, O, full, rng) is not None for _ in range(40)) >= 10:
            deq = ("deq", nD)
            break
    assert deq is not None
    lane_plans.append({s: ("xeq",) for s in later})
    lane_plans.append({s: ("xeq",) for s in sl})
    lane_plans.append({s: deq if s == sl[0] else ("xeq",) for s in sl})
    lane_plans.append({sl[0]: deq})
    lane_plans.append({sl[0]: ("xeq",)})
    lane_plans.append({sl[0]: deq, sl[-1]: ("xeq",)})
    assert len(lane_plans) <= 32, len(lane_plans)
    texts, reads, plans = [], [], []
    for k in range(N_PAIRS):
        lane = k % 64
        # crafted lanes in the odd places, clean ones between them; every fourth clean lane short (it retires in the first rounds)
        if lane % 2 == 1 and lane // 2 < len(lane_plans):
            plan, length = lane_plans[lane // 2], int(rng.integers(full, MAX_READ + 1))
        elif lane % 8 == 0:
            plan, length = {}, int(rng.integers(64, min(64 + T, full) + 1))
        else:
            plan, length = {}, int(rng.integers(full, MAX_READ + 1))
        # (a crafted pair is made again until the oracle's walk does with it what the plan says: see _window)
        for attempt in range(400):
            got = _realised(plan, W, O, length, rng)
            if got:
                t, q = got
                break
        else:
            raise AssertionError("no pair for plan %r" % (plan,))
        texts.append(t), reads.append(q), plans.append(plan)
    return dict(texts=texts, reads=reads, plans=plans, rflag=np.zeros(N_PAIRS, bool), tflag=np.zeros(N_PAIRS, bool))


def windows_of(cigar, read_len, W, T):
    """The window loop replayed on a pair's CIGAR -> per window {"ins": {column: length}, "step": [letter per column walked]}.
    A window walks columns while fewer than W-O columns and fewer than min(rows left, W-O) read characters are consumed."""
    ops = [op for cnt, op in re.findall(r"(\d+)([=XID])", cigar) for _ in range(int(cnt))]
    out, k, read_idx = [], 0, 0
    while read_idx < read_len:
        jlim = min(W, read_len - read_idx, T)
        i = j = 0
        win = dict(ins={}, step=[])
        while i < T and j < jlim and k < len(ops):
            if ops[k] == "I":
                win["ins"][i] = win["ins"].get(i, 0) + 1
                j += 1
            else:
                win["step"].append(ops[k])
                i += 1
                j += ops[k] != "D"
            k += 1
        out.append(win)
        read_idx += j
        if i == 0 and j == 0:
            break
    assert k == len(ops), (k, len(ops))
    return out


def events(win):
    """-> (columns with an event of the runs form: an insertion run or the start of a D / X / = run, runs committed)."""
    cols, runs, prev = set(win["ins"]), len(win["ins"]), None
    for c, s in enumerate(win["step"]):
        if s != prev or c in win["ins"]:
            cols.add(c)
            runs += 1
        prev = s
    return cols, runs


def guard_looks(lanes):
    """The staging rings of a wavefront, round by round as the kernel keeps them (runs form) -> how often the guard inside pass 2
    made the wavefront look.  lanes: per lane its windows.  Before the table a lane with 16 or more runs pending writes a piece of
    16; pass 2 takes two events per trip, and before the fifth and every later trip a lane with 27 or more pending makes every
    lane with 16 or more write one."""
    pending, looks = [0] * len(lanes), 0
    for r in range(max(len(w) for w in lanes)):
        live = [k for k, w in enumerate(lanes) if r < len(w)]
        per = {}
        for k in live:
            pending[k] -= 16 if pending[k] >= 16 else 0
            win, prev, ev = lanes[k][r], None, []
            for c, s in enumerate(win["step"]):
                starts = s != prev or c in win["ins"]
                if starts or c in win["ins"]:
                    ev.append((c in win["ins"]) + starts)
                prev = s
            if len(win["step"]) in win["ins"]:          # (a run that ends the window: no step behind it)
                ev.append(1)
            per[k] = ev
        for trip in range(max(-(-len(e) // 2) for e in per.values()) if per else 0):
            if trip >= 4 and any(pending[k] >= 27 for k in live):
                looks += 1
                for k in live:
                    pending[k] -= 16 if pending[k] >= 16 else 0
            for k in live:
                pending[k] += sum(per[k][2 * trip:2 * trip + 2])
                assert pending[k] <= 32, "the model's ring runs over"
    return looks


def holds(plan, cigar, read_len, W, T):
    """The windows of the plan came out as made: one insertion run of the planned length in the planned column and nothing else in
    that window; an event in every kept column of a busy window, of the planned letters."""
    wins = windows_of(cigar, read_len, W, T)
    for r, kind in plan.items():
        if r >= len(wins):
            return False
        if kind[0] == "ins":
            if wins[r]["ins"] != {kind[1]: kind[2]} or set(wins[r]["step"]) - {"="}:
                return False
        else:
            nD = kind[1] if kind[0] == "deq" else 0
            want = "".join("=" if c % 2 else ("D" if c < 2 * nD else "X") for c in range(T))
            if wins[r]["ins"] or "".join(wins[r]["step"]) != want:
                return False
    return True


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


_expected = {}


def expected(oracle, W, O):
    if (W, O) not in _expected:
        b = batch(W, O)
        eds, cigars, _, _ = oracle.align(b["texts"], b["reads"], W=W, O=O)
        runs = [np.array([x for c, op in api._parse_cigar(cg) for x in (c, ord(op))], dtype=np.uint8) for cg in cigars]
        streams = [np.frombuffer(api.cigar_to_edit_stream(cg, W, O), dtype=np.uint8) for cg in cigars]
        text_end = np.array([sum(c for c, op in api._parse_cigar(cg) if op in "=XD") for cg in cigars], dtype=np.int64)
        _expected[(W, O)] = dict(ed=np.array(eds, dtype=np.int64), cigars=cigars, runs=runs, streams=streams, text_end=text_end)
    return _expected[(W, O)]


@pytest.mark.parametrize("W,O", CONFIGS)
def test_the_windows_hold_what_they_say(oracle, W, O):
    """(CPU.)  From the oracle's CIGARs, window by window, for the lanes of the first wavefront: the insertion runs are where the
    plan put them, with every length in every one of the three columns; busy windows have an event in every kept column, far more
    than the eight that four trips take; the rings wrap and, by a model of them, the guard inside pass 2 makes the wavefront look."""
    T = W - O
    b, exp = batch(W, O), expected(oracle, W, O)
    assert N_PAIRS % 64 != 0 and N_PAIRS <= 256
    assert all(64 <= len(q) <= MAX_READ for q in b["reads"])
    seen, busy, most_events, clean, lanes = set(), 0, 0, 0, []
    for k in range(64):
        wins = windows_of(exp["cigars"][k], len(b["reads"][k]), W, T)
        plan = b["plans"][k]
        clean += exp["ed"][k] == 0
        assert holds(plan, exp["cigars"][k], len(b["reads"][k]), W, T), (k, plan, exp["cigars"][k])
        for r, kind in plan.items():
            if kind[0] == "ins":
                seen.add((kind[1], kind[2]))
            else:
                cols, runs = events(wins[r])
                assert cols == set(range(T)) and runs == T, (k, r, kind, sorted(cols))
                busy += 1
                most_events = max(most_events, len(cols))
        lanes.append(wins)
    assert seen == set(cases(T)), sorted(set(cases(T)) - seen)
    assert {L for c, L in seen if c == 0} == set(range(1, T + 1))
    assert busy >= 8 and most_events == T and clean >= 20
    assert max(sum(events(w)[1] for w in wins) for wins in lanes) > 32          # the ring wraps
    if T >= 24:
        assert most_events > 2 * 4 + 8          # pass 2 goes well past four trips, and past the guard's first look
        assert guard_looks(lanes) >= 2
    if (W, O) == (64, 33):
        # what the band does with the first wavefront, replayed from its C restatement (tests/test_gpu_band_table.py): the round in
        # front of the long runs and the D / = windows sees them and is redone (their own round has the short lanes' last windows
        # and goes to the full table directly), the later slots' rounds commit with most lanes live
        from tests.test_gpu_band_table import replay
        rounds = replay(dict(texts=b["texts"][:64], reads=b["reads"][:64]))[0]
        sl = slots(W, T)
        assert rounds[sl[0] - 1][0] == "redone" and rounds[sl[0]][0] == "short" and all(rounds[s] == ("committed", rounds[s][1]) and rounds[s][1] >= 40 for s in sl[1:]), rounds
    lens = sorted(len(q) for q in b["reads"][:64])
    assert lens[0] < 64 + T + 1 and lens[-1] > lens[8] > lens[0]


def launch(al, b, W, O, layout, mode, select=0):
    """One scrg_align_device / _edits / _distance launch on the batch -> host arrays (tests/test_gpu_band_table.py: launch, for any W/O)."""
    import torch
    dev = torch.device("cuda", al.device)
    al.set_stream(0)
    seq, t_off, r_off, stride = pack_sequences(al, b["texts"], b["reads"], layout)
    n = len(b["texts"])
    tl = np.array([len(x) for x in b["texts"]], dtype=np.uint64)
    ql = np.array([len(x) for x in b["reads"]], dtype=np.uint64)
    cap = (2 * (MAX_READ + 64) + 16 + 15) // 16 * 16
    cig_off = np.arange(n, dtype=np.uint64) * np.uint64(cap)
    desc = np.stack([t_off.astype(np.uint64), tl, r_off.astype(np.uint64), ql, cig_off, np.full(n, cap, dtype=np.uint64)], axis=1)
    desc_t = torch.from_numpy(desc.view(np.int64)).to(dev)
    ed = torch.full((n,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=dev)
    st = torch.full((n,), -7, dtype=torch.int32, device=dev)
    # (waves_per_cu as the caller's choice keeps a small launch on genasm_lane_kernel: see tests/test_gpu_band_table.py)
    p = al._params(dict(W=W, O=O, text_stride_words=stride, read_stride_words=stride, waves_per_cu=16))
    p.reserved[0] = select
    out = dict(cap=cap)
    if mode == "distance":
        al._check(al.lib.scrg_align_device_distance(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, ed, cnt, st)]))
    else:
        buf = torch.zeros(n * cap * 2, dtype=torch.uint8, device=dev)
        if mode == "edits":
            rc = torch.full((n,), -7, dtype=torch.int32, device=dev)
            al._check(al.lib.scrg_align_device_edits(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, buf, ed, cnt, st, rc)]))
        else:
            al._check(al.lib.scrg_align_device(al.h, C.byref(p), n, *[api._ptr(x) for x in (seq, desc_t, buf, ed, cnt, st)]))
    torch.cuda.synchronize()
    if mode != "distance":
        out["buf"] = buf.cpu().numpy()
    if mode == "edits":
        out["run_count"] = rc.cpu().numpy().astype(np.int64)
    out.update(ed=ed.cpu().numpy(), status=st.cpu().numpy(), count=cnt.cpu().numpy().astype(np.int64))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W,O", CONFIGS)
def test_length_bytes_and_busy_windows(aligner, aligner_select, oracle, W, O):
    """Runs, edit streams and distances of the crafted wavefronts, byte for byte: the shipped build, the test build without the band
    and with the band in every eligible round, both sequence layouts."""
    b, exp = batch(W, O), expected(oracle, W, O)
    for layout in ("contiguous", "groups"):
        for mode in ("runs", "edits", "distance"):
            compare(launch(aligner, b, W, O, layout, mode), exp, mode, "shipped, %d/%d, %s, %s" % (W, O, mode, layout))
            for select in (NO_BAND, BAND_ALWAYS):
                compare(launch(aligner_select, b, W, O, layout, mode, select), exp, mode,
                        "reserved[0] = %d, %d/%d, %s, %s" % (select, W, O, mode, layout))
