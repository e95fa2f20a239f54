"""Seed sampling, measured: scrg_genome_index and scrg_find_candidates on bench_seeding.py's two batches (N x 150 bp, N x 10 kb
against a synthetic chromosome) for three rules — the defaults (stride 4, no sampling), (13, stride 1, s = 7) and (13, stride 1,
s = 5) — timed at the C entry points.  Prints one JSON line.

    python tests/tools/bench_seed_sampling.py [--genome 20000000] [--short 1000000] [--long 100000] [--repeats 5] [--twin 10000]
    python tests/tools/bench_seed_sampling.py --profile short|long --rule default|s7|s5   # the run to put under a kernel trace
    python tests/tools/bench_seed_sampling.py --against OTHER_LIBRARY.so [--short N]      # smer = 0 of this library and another
                                                                                          # build (the parent commit's), alternating
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import scrooge_amd
from scrooge_amd import api, synth
from bench_seeding import Timed, long_reads, rng_of, same, short_reads, span

RULES = {"default": (api.SeedRule(), 0), "s7": (api.SeedRule(stride=1), 7), "s5": (api.SeedRule(stride=1), 5)}


def twin_sampled(t, rule, smer, genome, n):
    cp, ne, nl = C.POINTER(api.Candidates)(), C.c_uint64(), C.c_uint64()
    st = api._lazy(t.a.lib, "scrg_candidates_from_genome_sampled")(api._seed_rule(rule), smer, genome, len(genome), n, C.cast(t.rp, C.c_void_p),
                                                                   C.cast(t.rl, C.c_void_p), C.byref(cp), C.byref(ne), C.byref(nl))
    assert st == 0
    return cp, int(ne.value), int(nl.value)


def build(a, rule, smer, repeats):
    a.set_seed_sampling(smer)
    a.index_genome(rule)
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        info = a.index_genome(rule)
        times.append(time.perf_counter() - t0)
    return {"index_build": span(times), "index_entries": info["n_entries"], "index_positions": info["n_positions"], "index_device_bytes": info["device_bytes"]}


def measure(a, t, reads, starts, kind, repeats, rule, smer, genome, twin_n):
    n = len(reads)
    t.once()
    times = [t.once()[0] for _ in range(repeats)]
    dt, cp = t.once(keep=True)
    c = cp.contents
    tol = 4 if kind == "short" else 40
    offs = np.ctypeslib.as_array(c.cand_offsets, shape=(n + 1,)).astype(np.int64)
    n_pairs = int(offs[n])
    start = np.ctypeslib.as_array(c.cand_start, shape=(max(n_pairs, 1),))[:n_pairs].astype(np.int64)
    rev = np.ctypeslib.as_array(c.cand_reverse, shape=(max(n_pairs, 1),))[:n_pairs]
    read_of = np.repeat(np.arange(n), np.diff(offs))
    good = (np.abs(start - np.asarray(starts, dtype=np.int64)[read_of]) <= tol) & (rev == (read_of % 2))
    at_truth = int(len(np.unique(read_of[good])))
    lanes = sum(2 * max(0, len(r) - rule.k + 1) for r in reads)
    budget = (rule.hit_budget_mb or 256) * 2**20 // 48
    out = {"reads": n, "find_candidates": span(times), "candidates": n_pairs, "n_lookups": a.seed_sampling_info()["n_lookups"], "lanes": lanes,
           "n_hits": int(c.n_hits), "n_clusters": int(c.n_clusters), "n_keys_over_max_occ": int(c.n_keys_over_max_occ),
           "chunks_at_least": max(-(-int(c.n_hits) // budget), -(-lanes // (4 * budget))), "reads_with_a_candidate_at_the_truth": at_truth}
    if twin_n:
        tn = min(twin_n, n)
        tp, ne, nl = twin_sampled(t, rule, smer, genome, tn)
        out["twin"] = {"reads": tn, "identical_to_device": bool(same(tp, cp, tn)), "n_entries_equal": ne == a.index_info()["n_entries"]}
        t.free(tp)
    t.free(cp)
    return out


def against(args, genome, gcodes):
    """smer = 0 of this library and of another build of it, alternating in one loop on the defaults"""
    reads, _ = short_reads(gcodes, args.short, rng_of(7))
    handles = {"this": scrooge_amd.Aligner(0)}
    this_lib, api._LIB = api._LIB, None                  # a second library in this process: load_library() keeps one, so it is swapped out for the load
    os.environ["SCRG_LIB"] = args.against
    try:
        handles["other"] = scrooge_amd.Aligner(0)
    finally:
        api._LIB = this_lib
        del os.environ["SCRG_LIB"]
    assert handles["other"].lib is not handles["this"].lib
    for h in handles.values():
        h.set_genome(genome)
        h._check(api._lazy(h.lib, "scrg_genome_index")(h.h, None))          # (the entry point itself: the other library has no sampling info to report)
    timed = {name: Timed(h, reads) for name, h in handles.items()}
    for t in timed.values():
        t.once()
    times = {name: [] for name in timed}
    for _ in range(args.repeats):
        for name, t in timed.items():
            times[name].append(t.once()[0])
    a, b = (t.once(keep=True)[1] for t in timed.values())
    print(json.dumps({"against": args.against, "reads": args.short, "find_candidates": {k: span(v) for k, v in times.items()},
                      "identical": bool(same(a, b, args.short))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--short", type=int, default=1_000_000)
    ap.add_argument("--long", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twin", type=int, default=10_000)
    ap.add_argument("--profile", choices=["short", "long"], default=None)
    ap.add_argument("--rule", choices=sorted(RULES), default="s5")
    ap.add_argument("--against", default=None)
    args = ap.parse_args()
    gcodes = rng_of(42).integers(0, 4, args.genome, dtype=np.uint8)
    genome = synth.BASES[gcodes].tobytes()
    if args.against:
        return against(args, genome, gcodes)
    a = scrooge_amd.Aligner(0)
    a.set_genome(genome)
    if args.profile:
        rule, smer = RULES[args.rule]
        a.set_seed_sampling(smer)
        a.index_genome(rule)
        n = args.short if args.profile == "short" else args.long
        reads, _ = (short_reads if args.profile == "short" else long_reads)(gcodes, n, rng_of(7 if args.profile == "short" else 8))
        t = Timed(a, reads)
        print(json.dumps({"profile": args.profile, "rule": args.rule, "reads": n, "find_candidates_s": [t.once()[0], t.once()[0]]}))
        return
    out = {"genome_bp": args.genome, "rules": {k: "k %d, stride %d, smer %d" % (r.k, r.stride, s) for k, (r, s) in RULES.items()}}
    batches = {}
    if args.short:
        batches["short"] = short_reads(gcodes, args.short, rng_of(7))
    if args.long:
        batches["long"] = long_reads(gcodes, args.long, rng_of(8))
    timed = {kind: Timed(a, reads) for kind, (reads, _) in batches.items()}
    for name, (rule, smer) in RULES.items():
        out[name] = build(a, rule, smer, args.repeats)
        for kind, (reads, starts) in batches.items():
            out[name][kind] = measure(a, timed[kind], reads, starts, kind, args.repeats if kind == "short" else max(2, args.repeats // 2), rule, smer, genome,
                                      args.twin)
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
