"""Batches for the launch geometry of the per-pair output passes (scrooge_amd/csrc/run_walk.h: for_each_group; seq_kernels.hip: the
run compaction's own copy of that loop), for tests/test_walk_geometry.py (CPU) and tests/test_walk_geometry_gpu.py.

What changes with the number of pairs is `split` (the wavefronts that share a group of 64 pairs), the number of trips a wavefront
takes through the group loop once the grid is capped, and what a wavefront keeps from trip to trip.  The sizes at which each
happens come from scrooge_amd/csrc/launch_grid.h, compiled here for the host (tests/proto/launch_grid_host.cpp), and from the
device's CU count — not from literals.

A batch of n pairs is made of D = 61 DISTINCT pairs (a text, a read, runs, a status, a target start) and two more of 513 and
1 025 runs: pair i is distinct[(7 i) % 61], and every 1 009th pair is one of the two tile pairs instead.  Every descriptor points
at the one copy of its distinct pair's sequences and runs, so a million pairs cost a few arrays of n numbers, all made with numpy;
the Python models (tests/diff_model.py, report_model.py, cigar_form_model.py, clip_model.py, pileup_model.py) answer for the 63
distinct pairs once, and the expected output of pair i is the answer of distinct pair idx[i].  61 is coprime with 64, so every
lane of a group meets every distinct pair, and a pair given a neighbour's answer is a mismatch (the CPU test holds the answers of
neighbours apart).  Nothing here calls the library."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import cigar_form_model as cfm
from tests import clip_model as clm
from tests import diff_model as dm
from tests import pileup_model as pm
from tests import report_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

D = 61                            # distinct pairs of the first period; coprime with 64
STEP = 7                          # pair i is distinct[(STEP * i) % D]
TILE_PERIOD, TILE_AT = 1009, 20   # pair i with i % 1009 == 20 is a tile pair: 513 runs (i // 1009 even) or 1 025 (odd)
CAP_PERIOD, CAP_AT = 4099, 31     # pair i with i % 4099 == 31, if it is a plain one: its render segment lies outside the capacity
LANE_MAX_RUNS, COMPACT_LANE_MAX_RUNS, TILE_RUNS = 24, 16, 512      # run_walk.h, seq_kernels.hip
TARGET_LEN = 9000                 # the pileup's target
START_SHIFTS, START_SHIFT = 5, 17                # pair i starts START_SHIFT * (i % START_SHIFTS) behind its distinct pair's start
OK, OVER, NOT_BEST = 0, 2, 3      # pair statuses (include/scrooge_amd.h)
CANARY = 0xEE
FORMS = ["windowed", "merged", "m"]
KINDS = ["md", "cs"]
CU_COUNTS = [1, 8, 104, 256, 304]
MAX_PAIRS, MAX_RUNS = 1 << 22, 1 << 25

# (sort, runs): the special pairs, then plain alignments.  Sorts: "ok" an alignment; "bad_run" a run with count 0 (the short one)
# or an operation that is none (the long one); "over_text" / "over_read" runs that consume one base more than the descriptor's
# text_len / read_len; "status" a status other than done; "outside" a target start that puts columns behind the target.
SPECIAL = [("ok", 0), ("ok", 1), ("ok", 16), ("ok", 17), ("ok", 24), ("ok", 25), ("outside", 40), ("ok", 300),
           ("bad_run", 5), ("bad_run", 30), ("over_text", 6), ("over_text", 26), ("over_read", 7), ("over_read", 27),
           ("status", 4), ("status", 33), ("outside", 9)]
FILLER_RUNS = [2, 3, 5, 8, 9, 12, 4, 18, 6, 20, 7, 22, 10, 23, 11, 15, 13, 14, 19, 21, 3, 2]
COUNTED_SORTS = ["bad_run", "over_text", "over_read", "status", "outside", "capacity"]


# ---------------------------------------------------------------------------------------------------------------
# launch_grid.h on the host
# ---------------------------------------------------------------------------------------------------------------
_grid = None


def grid_lib():
    global _grid
    if _grid is None:
        so = os.path.join(HERE, "proto", "liblaunch_grid_host.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "scrooge_amd", "csrc"), "-o", so,
                               os.path.join(HERE, "proto", "launch_grid_host.cpp")])
        lib = C.CDLL(so)
        for name, args in (("lg_group_grid", [C.c_uint64, C.c_int, C.c_void_p]), ("lg_compact_runs_grid", [C.c_uint64, C.c_int, C.c_void_p]),
                           ("lg_compact_runs_packed_grid", [C.c_uint64, C.c_int]), ("lg_unpack_runs_grid", [C.c_uint64, C.c_int]),
                           ("lg_pack_planar_grid", [C.c_uint64, C.c_int]), ("lg_pack_planar_groups_items", [C.c_uint64, C.c_uint64]),
                           ("lg_pack_planar_groups_grid", [C.c_uint64, C.c_int])):
            getattr(lib, name).restype = C.c_uint64
            getattr(lib, name).argtypes = args
        _grid = lib
    return _grid


def _with_split(fn, n, n_cus):
    split = C.c_uint32(0xdead)
    blocks = int(fn(int(n), int(n_cus), C.byref(split)))
    return blocks, int(split.value)


def group_grid(n, n_cus):
    """-> (workgroups of four wavefronts, split) of a for_each_group launch"""
    return _with_split(grid_lib().lg_group_grid, n, n_cus)


def compact_runs_grid(n, n_cus):
    return _with_split(grid_lib().lg_compact_runs_grid, n, n_cus)


def compact_runs_packed_grid(n, n_cus):
    return int(grid_lib().lg_compact_runs_packed_grid(int(n), int(n_cus)))


def unpack_runs_grid(n_runs, n_cus):
    return int(grid_lib().lg_unpack_runs_grid(int(n_runs), int(n_cus)))


def pack_planar_grid(n_words, n_cus):
    return int(grid_lib().lg_pack_planar_grid(int(n_words), int(n_cus)))


def pack_planar_groups_grid(n_rows, words_per_row, n_cus):
    """-> (the threads' items, workgroups; 0 items: no launch)"""
    items = int(grid_lib().lg_pack_planar_groups_items(int(n_rows), int(words_per_row)))
    return items, (int(grid_lib().lg_pack_planar_groups_grid(items, int(n_cus))) if items else 0)


def group_waves(grid, n, n_cus):
    """The wavefronts that take groups in a launch of `grid` (group_grid or compact_runs_grid) -> (n_waves, split): what the
    kernels compute from gridDim — whole sets of `split`, the rest of the last workgroup idle."""
    blocks, split = grid(n, n_cus)
    return blocks * 4 // split, split


def trips(grid, n, n_cus):
    """The number of groups every taking wavefront walks: group g belongs to wavefront g % n_waves -> an array of n_waves counts"""
    n_waves, _ = group_waves(grid, n, n_cus)
    return np.bincount(np.arange((n + 63) // 64) % n_waves, minlength=n_waves)


def _sizes(grid, n_cus, classes):
    """One n per split class: 64 g - 27 at the smallest g of the class (the last group is not full); and "trips": the capped grid
    takes two whole trips and a part of a third.  A class the device never reaches (few CUs) is left out."""
    out = {}
    g = 1
    for s in classes:
        while grid(64 * g, n_cus)[1] > s:
            g += 1
        if grid(64 * g, n_cus)[1] == s:
            out["split%d" % s] = 64 * g - 27
    cap_waves = 4 * grid(1 << 40, n_cus)[0]                       # the grid of a batch of any size: the cap
    out["trips"] = 64 * (2 * cap_waves + cap_waves // 64 + 1) - 27
    return out


def group_sizes(n_cus):
    return _sizes(group_grid, n_cus, [64, 32, 16, 8, 4, 2, 1])


def compact_sizes(n_cus):
    return _sizes(compact_runs_grid, n_cus, [8, 4, 2, 1])


def packed_size(n_cus):
    """compact_runs_packed: three trips of one wavefront per pair, and 5 pairs"""
    cap_waves = 4 * compact_runs_packed_grid(MAX_PAIRS, n_cus)
    return 3 * cap_waves + 5


# ---------------------------------------------------------------------------------------------------------------
# the distinct pairs
# ---------------------------------------------------------------------------------------------------------------
def _plan():
    """-> D (sort, runs): the specials at the positions 0, 3, 6 ..: no two of them are neighbours in a batch (positions 7 apart mod
    61) or in this list, so pairs with the same answer (the "" of every refused pair, the zero record) never meet"""
    plan = [None] * D
    for k, s in enumerate(SPECIAL):
        plan[3 * k] = s
    rest = [k for k in range(D) if plan[k] is None]
    for j, k in enumerate(rest):
        plan[k] = ("ok", FILLER_RUNS[j % len(FILLER_RUNS)])
    return plan


class Catalog:
    """The D + 2 distinct pairs, their sequences and runs as the device gets them, and every model's answer for each."""

    def __init__(self):
        rng = np.random.Generator(np.random.PCG64(6161))
        plan = _plan() + [("ok", TILE_RUNS + 1), ("ok", 2 * TILE_RUNS + 1)]
        self.n = len(plan)
        self.sort = [s for s, _ in plan]
        self.text, self.read, self.runs, self.ed = [], [], [], []
        for k, (sort, c) in enumerate(plan):
            while True:               # (an alignment keeps something under clipping: the zero record is the refused pairs' alone)
                text, read, runs, ed = rm.valid_case(rng, c, max_count=6, slack=0 if sort == "over_text" else None)
                if c == 0 or clm.model(runs)["n_runs"] > 0:
                    break
            if sort == "bad_run":
                at = c - 2 if c <= LANE_MAX_RUNS else 20
                runs = list(runs)
                runs[at] = (0, runs[at][1]) if c <= LANE_MAX_RUNS else (runs[at][0], "M")
            self.text.append(text)
            self.read.append(read)
            self.runs.append(runs)
            self.ed.append(ed)
        self.cnt = np.array([len(r) for r in self.runs], dtype=np.int64)
        sort = np.array(self.sort)
        self.plain = sort == "ok"
        # lengths as the descriptors state them
        self.tl = np.array([len(t) for t in self.text], dtype=np.int64) - (sort == "over_text")
        self.rl = np.array([len(r) for r in self.read], dtype=np.int64) - (sort == "over_read")
        # every third plain pair's read, and the longer tile pair's, is stored reverse-complemented and flagged
        self.read_rev = self.plain & (np.arange(self.n) % 3 == 1)
        self.read_rev[D:] = [False, True]
        self.status = np.zeros(self.n, dtype=np.int32)
        for k in np.flatnonzero(sort == "status"):
            self.status[k] = OVER if self.cnt[k] <= LANE_MAX_RUNS else NOT_BEST
        # the pileup's: a pair with a run that is none adds what is not specified, and the model cannot read past a shortened read
        self.status_pile = np.where((sort == "bad_run") | (sort == "over_read"), OVER, self.status).astype(np.int32)
        span = np.array([dm.consumed([r for r in runs if r[1] in "=XID"])[0] for runs in self.runs], dtype=np.int64)
        self.start = rng.integers(0, TARGET_LEN - 4200, size=self.n).astype(np.int64)
        for k in np.flatnonzero(sort == "outside"):           # (the shifts move it further out: some copies begin behind the target)
            self.start[k] = TARGET_LEN - span[k] // 2
        assert (self.start[sort != "outside"] + span[sort != "outside"] + START_SHIFT * START_SHIFTS < TARGET_LEN).all()
        self._pack()
        self._answers()

    # what the device gets -------------------------------------------------------------------------------------
    def _pack(self):
        stored = [dm.revcomp(r) if rv else r for r, rv in zip(self.read, self.read_rev)]
        shifts = [[0, 1, 31, 13, 17][k % 5] for k in range(self.n)] + [[0, 5, 30][k % 3] for k in range(self.n)]
        self.words, offs = dm.pack_contiguous(self.text + stored, shifts)
        self.t_off = offs[:self.n].astype(np.uint64)
        self.r_off = offs[self.n:].astype(np.uint64) | np.where(self.read_rev, np.uint64(1 << 63), np.uint64(0))
        raw = lambda runs: np.array([(c, ord(o)) for c, o in runs], dtype=np.uint8).reshape(-1, 2)
        # dense: back to back, so a pair's first run lies at any 2-byte boundary; one run of padding behind
        self.dense_first = np.concatenate([[0], np.cumsum(self.cnt)])[:self.n]
        self.dense_tab = np.concatenate([raw(r) for r in self.runs] + [np.zeros((1, 2), np.uint8)])
        # slices: capacities in multiples of 16 runs (32-byte aligned slices), zeros behind a pair's runs
        self.slice_cap = np.maximum(16, (self.cnt + 15) // 16 * 16)
        self.slice_first = np.concatenate([[0], np.cumsum(self.slice_cap)])[:self.n]
        self.slice_tab = np.zeros((int(self.slice_cap.sum()), 2), dtype=np.uint8)
        for k, r in enumerate(self.runs):
            if r:
                self.slice_tab[self.slice_first[k]:self.slice_first[k] + len(r)] = raw(r)

    def descriptors(self, idx):
        """scrg_pair_desc of every pair: [n, 6] uint64"""
        return np.stack([self.t_off[idx], self.tl[idx].astype(np.uint64), self.r_off[idx], self.rl[idx].astype(np.uint64),
                         self.slice_first[idx].astype(np.uint64), self.slice_cap[idx].astype(np.uint64)], axis=1)

    # the models' answers ---------------------------------------------------------------------------------------
    def _strings(self, strings):
        """D + 2 strings -> (lengths incl. the NUL, all of them with their NULs back to back, where each begins)"""
        lens = np.array([len(s) + 1 for s in strings], dtype=np.int64)
        return lens, np.frombuffer(b"".join(s.encode() + b"\0" for s in strings), dtype=np.uint8).copy(), np.concatenate([[0], np.cumsum(lens)])[:self.n]

    def _answers(self):
        sort = np.array(self.sort)
        valid = np.array([all(clm.is_run(c, o) for c, o in runs) for runs in self.runs])
        assert (valid == (sort != "bad_run")).all()
        fits = (sort != "over_text") & (sort != "over_read")
        self.text_strings = {"windowed": ["".join("%d%s" % r for r in runs) for runs in self.runs]}
        for form in cfm.FORMS:
            self.text_strings[form] = [cfm.model(form, runs) if ok else "" for runs, ok in zip(self.runs, valid)]
        self.text_bad = {form: np.zeros(self.n, np.int64) if form == "windowed" else (~valid).astype(np.int64) for form in FORMS}
        self.diff_strings = {kind: [dm.model(kind, t, r, runs) if ok else "" for t, r, runs, ok in zip(self.text, self.read, self.runs, valid & fits)]
                             for kind in KINDS}
        self.diff_bad = (~(valid & fits)).astype(np.int64)
        self.text_cat = {form: self._strings(s) for form, s in self.text_strings.items()}
        self.diff_cat = {kind: self._strings(s) for kind, s in self.diff_strings.items()}
        # the report: the sequences as the descriptors bound them
        self.report = [rm.record(verdict=rm.NO_ALIGNMENT) if self.status[k] != OK else
                       rm.model(self.text[k][:self.tl[k]], self.read[k][:self.rl[k]], self.runs[k], self.ed[k]) for k in range(self.n)]
        self.report_fail = np.array([r["verdict"] not in (0, rm.NO_ALIGNMENT) for r in self.report]).astype(np.int64)
        self.report_rec = np.array([[r[f] for f in rm.FIELDS] for r in self.report], dtype=np.int64)
        # clipping: a pair that is not done, or has a run that is none, gets the zero record and apply leaves it alone
        self.clip_touched = valid & (self.status == OK)
        self.clip = [clm.model(self.runs[k]) if self.clip_touched[k] else clm.record() for k in range(self.n)]
        self.clip_rec = np.array([[r[f] for f in clm.FIELDS] for r in self.clip], dtype=np.int64)
        # the pileup: one model per distinct pair and start shift
        self.pile_counted = (self.status_pile == OK) & (self.cnt > 0)
        self.pile, self.pile_outside = {}, np.zeros((self.n, START_SHIFTS), dtype=np.int64)
        for k in np.flatnonzero(self.pile_counted):
            for s in range(START_SHIFTS):
                counts, outside = pm.model(self.runs[k], self.read[k], int(self.start[k]) + s * START_SHIFT, TARGET_LEN)
                at = np.nonzero(counts)
                self.pile[(int(k), s)] = (at, counts[at].astype(np.int64))
                self.pile_outside[k, s] = int(outside)

    def pileup_expected(self, idx, shift):
        """The planes (counts form) and the out-of-range count of ONE add of the batch: every (distinct pair, shift) by its multiplicity"""
        mult = np.bincount(idx * START_SHIFTS + shift, minlength=self.n * START_SHIFTS).reshape(self.n, START_SHIFTS)
        want = np.zeros((pm.PLANES, TARGET_LEN + 1), dtype=np.int64)
        for (k, s), (at, v) in self.pile.items():
            want[at] += v * int(mult[k, s])
        return want, int((mult * self.pile_outside).sum()), int((mult * self.pile_counted[:, None]).sum())

    def multiplicity(self, idx, cap_out):
        """How many pairs of a batch are of each counted sort"""
        sort = np.array(self.sort)
        out = {s: int((sort[idx] == s).sum()) for s in COUNTED_SORTS[:-1]}
        out["capacity"] = int(cap_out.sum())
        return out


_catalog = None


def catalog():
    global _catalog
    if _catalog is None:
        _catalog = Catalog()
    return _catalog


# ---------------------------------------------------------------------------------------------------------------
# a batch by index
# ---------------------------------------------------------------------------------------------------------------
def batch_index(n):
    """-> (idx: the distinct pair of every pair, shift: its start shift, cap_out: the pairs whose render segment lies outside the
    capacity) — numpy, no loop over pairs"""
    i = np.arange(n, dtype=np.int64)
    idx = (STEP * i) % D
    tile = i % TILE_PERIOD == TILE_AT
    idx[tile] = D + (i[tile] // TILE_PERIOD) % 2
    cap_out = (i % CAP_PERIOD == CAP_AT) & catalog().plain[idx]
    return idx, i % START_SHIFTS, cap_out


def segments(lens, cap_out):
    """Where the render pass is told to put every pair's string: behind each other from byte 2, three bytes of room behind every
    third, and a pair of cap_out at an offset past the capacity (its room stays a canary) -> (offsets, capacity = the buffer's size)"""
    n = len(lens)
    gap = (np.arange(n) % 3 == 0) * 3
    ends = 2 + np.cumsum(lens + gap)
    off = np.concatenate([[2], ends])[:n]
    total = int(ends[-1]) + 5 if n else 7
    return np.where(cap_out, total + 5, off), off, total


def long_per_group(idx, limit=LANE_MAX_RUNS):
    """The pairs of more than `limit` runs in every group of 64"""
    big = catalog().cnt[idx] > limit
    pad = (-len(big)) % 64
    return np.concatenate([big, np.zeros(pad, bool)]).reshape(-1, 64).sum(axis=1)


def total_runs(idx):
    return int(catalog().cnt[idx].sum())


def byte_to_run(b):
    """What unpack_runs makes of a packed byte: the operation of bits 7..6 (0 '=', 1 'X', 2 'I', 3 'D') over the count of bits 5..0"""
    b = np.asarray(b, dtype=np.uint16)
    return (np.frombuffer(b"=XID", dtype=np.uint8).astype(np.uint16)[b >> 6] << 8) | (b & 63)


def run_to_byte(run16):
    """A run of one of the four operations with a count of at most 63, as compact_runs_packed packs it"""
    run16 = np.asarray(run16, dtype=np.uint16)
    code = np.zeros(256, dtype=np.uint8)
    for k, o in enumerate(b"=XID"):
        code[o] = k
    return ((code[run16 >> 8] << 6) | (run16 & 63).astype(np.uint8)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# the host path's own text kernels (text_len_kernel, render_text_kernel: no device entry point): mapping calls by period
# ---------------------------------------------------------------------------------------------------------------
HOST_SPLITS = [32, 16, 8]         # the classes the planned chunks of the three call sizes fall into
HOST_CAND_SHIFT = 5               # every read's second candidate: its locus shifted, the loser of best-candidate mode


class HostCatalog:
    """D reads with two candidates each on one genome — 2 D distinct (read, candidate) pairs, aligned once by the oracle — and the
    models' answers for each: the merged and the windowed CIGAR text, the cs string, the report, and best-candidate mode's winners.
    Every eighth read is long enough for more than LANE_MAX_RUNS runs (the wavefront walk); the others are short."""

    def __init__(self, oracle):
        from scrooge_amd import api, synth
        from tests.test_best_candidate import oracle_mapping
        rng = np.random.Generator(np.random.PCG64(6262))
        texts, self.reads = [], []
        for k in range(D):
            t, q = synth.make_pair(int(rng.integers(300, 500)) if k % 8 == 3 else int(rng.integers(24, 90)), 0.1, (1, 1, 1), rng, slack=0.1)
            texts.append(synth.BASES[t].tobytes())
            self.reads.append(synth.BASES[q].tobytes())
        starts = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
        self.genome = b"".join(texts) + pm.random_read(rng, 1500)
        self.cands = [[int(starts[k]), int(starts[k]) + HOST_CAND_SHIFT] for k in range(D)]
        eds, cigars = oracle_mapping(oracle, self.genome, self.reads, self.cands)
        self.ed = np.array(eds, dtype=np.int64)
        self.runs = [dm.parse(c) for c in cigars]
        self.cnt = np.array([len(r) for r in self.runs], dtype=np.int64)
        pair_text = [self.genome[c:c + 2 * len(self.reads[k]) + 256] for k in range(D) for c in self.cands[k]]
        pair_read = [self.reads[k] for k in range(D) for _ in self.cands[k]]
        best = api.best_per_read(self.ed, np.zeros(2 * D, dtype=np.int64), np.arange(0, 2 * D + 1, 2))["best_pair"]
        self.wins = np.zeros(2 * D, dtype=bool)
        self.wins[best] = True
        self.strings, self.report_rec = {}, {}
        for mode in ("all", "best"):
            has = np.ones(2 * D, bool) if mode == "all" else self.wins
            self.strings[mode] = {
                "windowed": _strings_of(["".join("%d%s" % r for r in runs) if h else "" for runs, h in zip(self.runs, has)]),
                "merged": _strings_of([cfm.model("merged", runs) if h else "" for runs, h in zip(self.runs, has)]),
                "cs": _strings_of([dm.model("cs", t, q, runs) if h else "" for t, q, runs, h in zip(pair_text, pair_read, self.runs, has)])}
            recs = [rm.model(t, q, runs, int(e)) if h else rm.record(verdict=rm.NO_ALIGNMENT)
                    for t, q, runs, e, h in zip(pair_text, pair_read, self.runs, self.ed, has)]
            assert all(r["verdict"] in (0, rm.NO_ALIGNMENT) for r in recs)
            self.report_rec[mode] = np.array([[r[f] for f in rm.FIELDS] for r in recs], dtype=np.uint32)

    def call(self, n_reads):
        """A mapping call of n_reads reads by period -> (reads, candidates, the distinct pair of every pair of the call)"""
        which = (STEP * np.arange(n_reads)) % D
        return [self.reads[k] for k in which], [self.cands[k] for k in which], (2 * which[:, None] + np.arange(2)[None, :]).reshape(-1)

    def read_lens(self, n_reads):
        return np.array([len(r) for r in self.reads], dtype=np.uint64)[(STEP * np.arange(n_reads)) % D]


def _strings_of(strings):
    lens = np.array([len(s) + 1 for s in strings], dtype=np.int64)
    return lens, np.frombuffer(b"".join(s.encode() + b"\0" for s in strings), dtype=np.uint8).copy(), np.concatenate([[0], np.cumsum(lens)])[:-1]


_host = None


def host_catalog(oracle):
    global _host
    if _host is None:
        _host = HostCatalog(oracle)
    return _host


def host_chunk_classes(hc, n_reads, n_cus, **params):
    """The `split` of the text kernels' launch for every planned chunk of a call (scrg_host_plan_mapping: no GPU involved)"""
    from scrooge_amd import api
    _, first = api.host_plan_mapping(hc.read_lens(n_reads), np.arange(0, 2 * n_reads + 1, 2), **params)
    return [group_grid(int(b - a), n_cus)[1] for a, b in zip(first[:-1], first[1:])]


def host_call_reads(hc, n_cus, split, **params):
    """The smallest call, in steps of half a chunk of the class's size, whose first planned chunks are of `split`'s class"""
    size = group_sizes(n_cus)["split%d" % split]
    for k in range(2, 200):
        n_reads = k * size // 4
        classes = host_chunk_classes(hc, n_reads, n_cus, **params)
        if len(classes) >= 2 and classes[0] == split:
            return n_reads
    raise AssertionError("no call size plans chunks of split %d" % split)
