"""Seeding, measured: scrg_genome_index and scrg_find_candidates on the read-mapping bench's shape (N x 150 bp reads, 1 % errors,
against a synthetic chromosome) and on long reads (N x 10 kb, ont errors), timed at the C entry points (no per-candidate Python
objects), with the host twin on 16 threads and the mapping call the candidates feed as yardsticks.  Prints one JSON line.

    python tests/tools/bench_seeding.py [--genome 20000000] [--short 1000000] [--long 100000] [--repeats 5] [--twin-long 10000]
    python tests/tools/bench_seeding.py --profile short|long      # one warm and one more find_candidates: the run to put under a kernel trace
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import scrooge_amd
from scrooge_amd import api, synth


def short_reads(gcodes, n, rng):
    """150 bp, 0.9 % substitutions and an indel in 15 % of the reads (tests/tools/bench_mapping.py's batch), alternating strands"""
    L = 150
    starts = rng.integers(0, len(gcodes) - 400, n)
    seg = gcodes[starts[:, None] + np.arange(L + 8)[None, :]]
    sub = rng.random((n, L + 8)) < 0.009
    seg = np.where(sub, (seg + rng.integers(1, 4, seg.shape, dtype=np.uint8)) & 3, seg)
    codes = seg[:, :L].copy()
    for r in np.nonzero(rng.random(n) < 0.075)[0]:
        p = int(rng.integers(1, L - 1))
        codes[r, p:] = seg[r, p + 1:L + 1]
    for r in np.nonzero(rng.random(n) < 0.075)[0]:
        p = int(rng.integers(1, L - 1))
        codes[r, p + 1:] = codes[r, p:L - 1].copy()
        codes[r, p] = rng.integers(0, 4)
    codes[1::2] = 3 - codes[1::2, ::-1]                  # every other read from the reverse strand
    ascii_reads = synth.BASES[codes]
    return [ascii_reads[r].tobytes() for r in range(n)], starts


def long_reads(gcodes, n, rng, L=10000):
    err, ratio = synth.PROFILES["ont"]
    starts = rng.integers(0, len(gcodes) - int(L * 1.3) - 64, n)
    reads = []
    for i, s in enumerate(starts):
        codes = synth.mutate(gcodes[s:s + int(L * 1.3) + 64], err, ratio, rng)[:L]
        reads.append(synth.BASES[3 - codes[::-1] if i % 2 else codes].tobytes())
    return reads, starts


class Timed:
    def __init__(self, aligner, reads):
        self.a, self.n = aligner, len(reads)
        self.rp = (C.c_char_p * self.n)(*reads)
        self.rl = (C.c_uint64 * self.n)(*[len(r) for r in reads])
        self.find = api._lazy(aligner.lib, "scrg_find_candidates")
        self.free = api._lazy(aligner.lib, "scrg_candidates_free")

    def once(self, keep=False):
        cp = C.POINTER(api.Candidates)()
        t = time.perf_counter()
        st = self.find(self.a.h, self.n, C.cast(self.rp, C.c_void_p), C.cast(self.rl, C.c_void_p), C.byref(cp))
        dt = time.perf_counter() - t
        self.a._check(st)
        if keep:
            return dt, cp
        self.free(cp)
        return dt, None

    def twin(self, genome, n=None):
        n = self.n if n is None else min(n, self.n)
        cp = C.POINTER(api.Candidates)()
        t = time.perf_counter()
        st = api._lazy(self.a.lib, "scrg_candidates_from_genome")(None, genome, len(genome), n, C.cast(self.rp, C.c_void_p), C.cast(self.rl, C.c_void_p), C.byref(cp))
        dt = time.perf_counter() - t
        assert st == 0
        return dt, n, cp

    def mapping(self, cp, repeats):
        """scrg_align_mapping_resident in best-candidate mode, distance and CIGAR text, on the candidates as they are"""
        c = cp.contents
        p = self.a._params({"best": True})
        times = []
        for _ in range(repeats):
            res = C.POINTER(api.Result)()
            t = time.perf_counter()
            st = self.a.lib.scrg_align_mapping_resident(self.a.h, C.byref(p), self.n, C.cast(self.rp, C.c_void_p), C.cast(self.rl, C.c_void_p),
                                                        C.cast(c.cand_offsets, C.c_void_p), C.cast(c.cand_start, C.c_void_p), C.cast(c.cand_reverse, C.c_void_p),
                                                        C.byref(res))
            times.append(time.perf_counter() - t)
            self.a._check(st, allow=(api.SCRG_ERR_CIGAR_OVERFLOW,))
            self.a.lib.scrg_result_free(res)
        return times


def same(a, b, n):
    ca, cb = a.contents, b.contents
    na = int(ca.cand_offsets[n])
    view = lambda p, k, t: np.ctypeslib.as_array(p, shape=(max(k, 1),)).view(t)[:k]
    return na == int(cb.cand_offsets[n]) and all(np.array_equal(view(getattr(ca, f), k, t), view(getattr(cb, f), k, t)) for f, k, t in
                                                 (("cand_offsets", n + 1, np.uint64), ("cand_start", na, np.uint64), ("cand_reverse", na, np.uint8),
                                                  ("cand_votes", na, np.uint32)))


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def span(xs):
    return {"min_ms": round(min(xs) * 1e3, 3), "median_ms": round(sorted(xs)[len(xs) // 2] * 1e3, 3), "max_ms": round(max(xs) * 1e3, 3), "n": len(xs)}


def measure(a, genome, gcodes, kind, n, repeats, twin_n):
    reads, starts = (short_reads if kind == "short" else long_reads)(gcodes, n, rng_of(7 if kind == "short" else 8))
    t = Timed(a, reads)
    t.once()                                             # warm-up: the buffers of this size
    times = [t.once()[0] for _ in range(repeats)]
    dt, cp = t.once(keep=True)
    c = cp.contents
    n_pairs = int(c.cand_offsets[n])
    lookups = sum(2 * max(0, len(r) - 13 + 1) for r in reads)
    out = {"reads": n, "read_len": len(reads[0]), "find_candidates": span(times), "candidates": n_pairs, "n_hits": int(c.n_hits), "n_clusters": int(c.n_clusters),
           "n_keys_over_max_occ": int(c.n_keys_over_max_occ), "key_lookups_per_pass": lookups,
           "reads_with_a_candidate_at_the_truth": int(sum(1 for r in range(n) if any(abs(int(c.cand_start[p]) - int(starts[r])) <= (4 if kind == "short" else 40)
                                                                                       and int(c.cand_reverse[p]) == r % 2
                                                                                       for p in range(int(c.cand_offsets[r]), int(c.cand_offsets[r + 1])))))}
    tw, tn, tp = t.twin(genome, twin_n)
    out["twin_16_threads"] = {"reads": tn, "s": round(tw, 3), "identical_to_device": bool(same(tp, cp, tn))}
    t.free(tp)
    a.align_mapping_directed(reads[:1000], [[0]] * 1000)                   # warm-up of the mapping path
    out["mapping_call_on_these_candidates"] = span(t.mapping(cp, 3)[1:] or [0])
    t.free(cp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--short", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twin-long", type=int, default=10_000)
    ap.add_argument("--profile", choices=["short", "long"], default=None)
    args = ap.parse_args()
    gcodes = rng_of(42).integers(0, 4, args.genome, dtype=np.uint8)
    genome = synth.BASES[gcodes].tobytes()
    a = scrooge_amd.Aligner(0)
    a.set_genome(genome)
    if args.profile:
        a.index_genome()
        n = args.short if args.profile == "short" else args.long
        reads, _ = (short_reads if args.profile == "short" else long_reads)(gcodes, n, rng_of(7 if args.profile == "short" else 8))
        t = Timed(a, reads)
        print(json.dumps({"profile": args.profile, "reads": n, "find_candidates_s": [t.once()[0], t.once()[0]]}))
        return
    a.index_genome()
    build = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        info = a.index_genome()
        build.append(time.perf_counter() - t0)
    out = {"genome_bp": args.genome, "rule": "defaults (k 13, stride 4, max_occ 64, band 32, min_hits 2, max_candidates 4, both strands, 256 MB)",
           "index_build": span(build), "index_entries": info["n_entries"], "index_device_bytes": info["device_bytes"]}
    if args.short:
        out["short"] = measure(a, genome, gcodes, "short", args.short, args.repeats, None)
    if args.long:
        out["long"] = measure(a, genome, gcodes, "long", args.long, max(2, args.repeats // 2), args.twin_long)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
